"""TEST INFRASTRUCTURE ONLY - writes tests/golden/efficientnet_*.pt: what the reference's own MBConvBlock / EfficientNet classes
(drop_connect_rate = 0, dropout_rate = 0 for the whole models) return for the seeded inputs of tests/test_efficientnet.py, the keep mask of
the drop-connect case, and the numbers the host-only tests compare with (recorded tensors, names and shapes only; the weights are regenerated
by golden_util.deterministic_fill on both sides).  Run where the reference tree exists:  python tests/make_efficientnet_golden.py

The 1e-4 bar on the training logits is a condition on the input: the reference's own fp32 logits must lie within a third of it of its fp64
logits, or no fp32 implementation could be expected to meet it.  This writer checks that on the chosen input (4 x 3 x 64 x 64, seed 5) and
refuses to write a fixture that misses it (the remedy is a larger input, 96 x 96, or another seed - in test_efficientnet._model_inputs)."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
os.environ["SGX_WRITE_GOLDEN"] = "1"

import torch  # noqa: E402

import test_efficientnet as T  # noqa: E402
from oracle import golden_util as G  # noqa: E402
from oracle import ref_shim  # noqa: E402
from util import rel_err  # noqa: E402

if __name__ == "__main__":
    if not ref_shim.available():
        raise SystemExit("the reference tree is not on this machine")
    torch.manual_seed(1234)
    fx = T._block_reference()
    print(f"blocks: {[k for k in fx]}; drop-connect keep mask {T._drop_connect_reference()['keep'].tolist()}")
    T._host_reference()
    for name in T.MODELS:
        fx = T._model_reference(name)
        e = rel_err(fx["logits"].double(), fx["logits_f64"])
        t64, t32 = fx["grad_norms_f64"], fx["grad_norms"]
        print(f"{name}: {len(fx['state_layout'])} state entries; reference fp32 against fp64: logits {e:.2e}, per-parameter gradient norms overall "
              f"{float((t32 - t64).norm() / t64.norm()):.2e}")
        if e > 1e-4 / 3:
            raise SystemExit(f"{name}: the reference's own fp32 logits are {e:.2e} from its fp64 logits - more than a third of the 1e-4 bar: enlarge the input or reseed")
    for name in ["efficientnet_block_reference", "efficientnet_drop_connect_reference", "efficientnet_host_reference"] + [f"efficientnet_{m}_reference" for m in T.MODELS]:
        path = os.path.join(G.GOLDEN_DIR, f"{name}.pt")
        print(f"{path}: {os.path.getsize(path)} bytes")

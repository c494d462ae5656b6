"""TEST INFRASTRUCTURE ONLY - writes tests/golden/regseg_*.pt: what the reference's own DBlock and RegSeg48 return for the seeded inputs of
tests/test_regseg.py (recorded tensors only).  Run where the reference tree exists:  python tests/make_regseg_golden.py"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
os.environ["SGX_WRITE_GOLDEN"] = "1"

import torch  # noqa: E402

import test_regseg as T  # noqa: E402
from oracle import golden_util as G  # noqa: E402
from oracle import ref_shim  # noqa: E402

if __name__ == "__main__":
    if not ref_shim.available():
        raise SystemExit("the reference tree is not on this machine")
    torch.manual_seed(1234)
    fx = T._block_reference()
    for name, rec in fx.items():
        print(f"{name}: y {tuple(rec['y'].shape)}, {len(rec['state'])} state entries")
    m = T._model_reference()  # (asserts the reference's stage extents 16 x 24, 8 x 12, 4 x 6 and the output shape)
    print(f"regseg48: {len(m['state_layout'])} state entries; reference fp32 against fp64: {m['bars']}")
    for name in ("regseg_block_reference", "regseg_regseg48_reference", "regseg_regseg48_logits0", "regseg_regseg48_logits1"):
        path = os.path.join(G.GOLDEN_DIR, f"{name}.pt")
        size = os.path.getsize(path)
        print(f"{path}: {size} bytes")
        assert size < 1 << 20, "a committed file may not exceed 1 MiB"

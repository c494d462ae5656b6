"""TEST INFRASTRUCTURE ONLY - writes tests/golden/dappm_reference.pt: what the reference's own DAPPM returns in fp64 for the seeded inputs of
tests/test_dappm.py (recorded tensors only).  Run where the reference tree exists:  python tests/make_dappm_golden.py"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
os.environ["SGX_WRITE_GOLDEN"] = "1"

import torch  # noqa: E402

import test_dappm as T  # noqa: E402
from oracle import golden_util as G  # noqa: E402
from oracle import ref_shim  # noqa: E402

if __name__ == "__main__":
    if not ref_shim.available():
        raise SystemExit("the reference tree is not on this machine")
    torch.manual_seed(1234)
    for name, rec in T._reference().items():
        print(f"{name}: y {tuple(rec['y'].shape)}, {len(rec['state'])} state entries, smallest |pre-activation| {float(rec['min_preact'].min()):.3e}")
        assert float(rec["min_preact"].min()) > 1e-5, "choose another seed: a pre-activation lies within 1e-5 of zero"
    path = os.path.join(G.GOLDEN_DIR, "dappm_reference.pt")
    print(f"{path}: {os.path.getsize(path)} bytes")
    assert os.path.getsize(path) < 1 << 20, "a committed file may not exceed 1 MiB"

"""Child process of tests/test_mfv_edges_gpu.py::test_larger_lds_after_smaller_in_a_fresh_process (not a test module).

More than 64 KiB of dynamic LDS needs a per-kernel attribute, and the host remembers per process what it has set.  In a process that
has launched nothing yet, every encoder kernel that can pass 64 KiB is called at a smaller size first and a larger one after it
(tests/mfv_cases.py: LDS_*), and every result is held to the float64 oracle at the bars of the other encoder tests: a launch above
what the attribute allows either fails (a return code, caught here) or computes garbage (caught by the oracle).  One line per call,
"LDS-CHILD-OK" at the end; any failure is a non-zero exit status.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import mfv_cases as M  # noqa: E402


def cloud(N, m):
    p = np.random.default_rng([11, N, m]).uniform(-0.8, 0.8, size=(1, N, 3)).astype(np.float32)
    ref = M.make_ref(p, m, M.S0)
    M.check_conditioning(ref, (N, m))
    return p, ref


def forward(dev, m, N, fwd2):
    assert M.uses_fwd2(N) == fwd2 and M.LDS_OPT_IN < M.fwd_lds_bytes(N, m) <= M.LDS_CAP
    p, ref = cloud(N, m)
    rc, fv, band = M.gpu_forward(torch.tensor(p, device=dev), m, M.S0)
    assert rc == 0, ("dpd_mfv3d_fwd", m, N, rc)
    M.check_forward(fv, band, ref, m, ("lds", "fwd2" if fwd2 else "fwd", m, N, M.fwd_lds_bytes(N, m)))


def backward(dev, m, N, sliced):
    p, ref = cloud(N, m)
    dfv = M.upstream(ref.fv64, [13, N, m])
    g64, g32 = M.oracle_backward(p, dfv, m, M.S0)
    bref = M.BwdRef(dfv, g64, g32, *M.backward_bars(g64, g32))
    rc, dpts, bands, _ = M.gpu_backward(torch.tensor(p, device=dev), torch.tensor(dfv, device=dev), m, M.S0, sliced)
    assert rc == 0, ("dpd_mfv3d_bwd", m, N, sliced, rc)
    lds = M.bwd_sliced_lds_bytes(N, m) if sliced else M.bwd_lds_bytes(N, m)
    M.check_backward(dpts, bands, bref, ("lds", "sliced" if sliced else "one-launch", m, N, lds))


def main():
    M.check_lds_plan()
    assert torch.cuda.is_available(), "no GPU is visible"
    dev = torch.device("cuda:0")
    for m, N in M.LDS_FWD2:
        forward(dev, m, N, True)
    for m, N in M.LDS_FWD:          # after fwd2 has been opted in: the two forward kernels have the same signature
        forward(dev, m, N, False)
    for m, N in M.LDS_BWD_ONE:
        backward(dev, m, N, False)
    for m, N in M.LDS_BWD_SLICED:
        backward(dev, m, N, True)
    print("LDS-CHILD-OK")


if __name__ == "__main__":
    main()

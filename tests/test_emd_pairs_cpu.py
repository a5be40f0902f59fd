"""Per-pair Earth Mover's distance (csrc/emd_pairs.hip, dpdist_amd.emd: emd_pairs / EMDPairs) without a GPU: the floors behind the bars of
tests/test_emd_pairs_gpu.py, the cases, and the argument errors of the C entries and the wrappers."""
import ctypes
import os

import numpy as np
import pytest

from tests import baseline_pairs_cases as PC
from tests import emd_matrix_cases as EC

NAMES = ("dpd_emd_pairs_workspace_bytes", "dpd_emd_pairs_fwd", "dpd_emd_pairs_bwd")


def test_recorded_floors_are_the_measured_ones():
    """EMD_FLOOR is the float32 restatement's worst deviation from float64 on these pairs as measured when the test was written; numpy's
    exp and pairwise sums differ by an ulp between CPUs, so the recomputed floor has to stay within a factor of four of the recorded one"""
    worst = PC.emd_floors()
    print("measured floors:", {q: "%.3g" % v for q, v in worst.items()})
    for q, v in worst.items():
        assert PC.EMD_FLOOR[q] / 4 <= v <= PC.EMD_FLOOR[q] * 4, (q, v, PC.EMD_FLOOR[q])


def test_cases_are_the_diagonals_of_the_matrix_cases():
    want = {"tiny": ((1, 5), (7, 2)), "tiles": ((65, 130), (63, 67)), "dup_far": ((48, 48), (40, 40)), "wide": ((300,), (257,)),
            "cap": ((2048,), (2048,))}
    assert "self" not in PC.EMD_CASES
    for name in PC.EMD_CASES:
        A, B, cA, cB, W = PC.emd_make(name)
        mA, mB, _, _, mW = EC.make(name)
        assert (cA, cB) == want[name] and W.shape == (len(cA),) and A.shape[0] == B.shape[0] == len(cA) == len(cB)
        for b in range(len(cA)):
            assert np.array_equal(A[b], mA[b]) and np.array_equal(B[b], mB[b]) and W[b] == mW[b, b]
    ref = PC.emd_oracle("tiles")
    full = EC.oracle("tiles")
    assert np.array_equal(ref["dist"], np.diagonal(full["dist"]))   # a pair's distance does not know the other pairs
    for b, (n, m) in enumerate(zip(*PC.emd_make("tiles")[2:4])):
        assert not ref["dA"][b, n:].any() and not ref["dB"][b, m:].any()


@pytest.fixture(scope="module")
def lib():
    from dpdist_amd import build, lib as L
    build.build(verbose=False)
    return L.load()


def test_exports_and_header_agree(lib):
    from dpdist_amd import lib as L
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dpdist_capi.h")).read()
    for name in NAMES:
        assert hasattr(lib, name) and name in L.SIGNATURES and name + "(" in header
    import dpdist_amd
    from dpdist_amd import build, emd
    assert dpdist_amd.emd_pairs is emd.emd_pairs and dpdist_amd.EMDPairs is emd.EMDPairs
    assert "emd_pairs.hip" in build.SOURCES


def test_workspace_bytes(lib):
    ws = lib.dpd_emd_pairs_workspace_bytes
    assert ws(2, 5, 7) == 2 * (3 * 5 + 2 * 7) * 4
    assert ws(1, 2048, 2048) == 5 * 2048 * 4
    assert ws((1 << 31) - 1, 2048, 2048) == ((1 << 31) - 1) * 5 * 2048 * 4      # 64-bit all the way
    for bad in ((0, 5, 7), (-1, 5, 7), (2, 0, 7), (2, 5, 0), (2, 2049, 7), (2, 5, 2049)):
        assert ws(*bad) == 0, bad


def test_refusals_without_a_device(lib):
    p = ctypes.c_void_p(1 << 30)                                  # any non-NULL "device address": nothing is dereferenced
    E_NULL, E_DIM, E_UNSUPPORTED, E_WORKSPACE = -1, -2, -3, -4
    need = lib.dpd_emd_pairs_workspace_bytes(2, 5, 7)

    def fwd(A=p, B=p, Wa=5, Wb=7, P=2, form=0, cost=p, dist=p, ws=p, nb=need):
        return lib.dpd_emd_pairs_fwd(A, p, Wa, B, None, Wb, P, form, cost, dist, ws, nb, None)

    def bwd(A=p, B=p, Wa=5, Wb=7, P=2, form=0, W=p, dA=p, dB=p, ws=p, nb=need):
        return lib.dpd_emd_pairs_bwd(A, None, Wa, B, p, Wb, P, form, W, dA, dB, ws, nb, None)

    assert fwd(A=None) == E_NULL and fwd(B=None) == E_NULL and fwd(cost=None, dist=None) == E_NULL
    assert bwd(A=None) == E_NULL and bwd(B=None) == E_NULL and bwd(W=None) == E_NULL and bwd(dA=None, dB=None) == E_NULL
    for P in (0, -1):
        assert fwd(P=P, nb=1 << 40) == E_DIM and bwd(P=P, nb=1 << 40) == E_DIM
    for form in (-1, 3):
        assert fwd(form=form) == E_DIM and bwd(form=form) == E_DIM
    for Wa, Wb in ((0, 7), (5, 0), (2049, 7), (5, 2049), (-3, 7)):
        assert fwd(Wa=Wa, Wb=Wb, nb=1 << 40) == E_UNSUPPORTED and bwd(Wa=Wa, Wb=Wb, nb=1 << 40) == E_UNSUPPORTED, (Wa, Wb)
    for form in (0, 1, 2):
        assert fwd(form=form, nb=need - 1) == E_WORKSPACE and fwd(form=form, ws=None) == E_WORKSPACE
        assert bwd(form=form, nb=need - 1) == E_WORKSPACE and bwd(form=form, ws=None) == E_WORKSPACE


def test_wrappers_refuse_bad_arguments(lib):
    import torch
    from dpdist_amd import EMDPairs, emd_pairs
    a, b = torch.zeros(2, 8, 3), torch.zeros(2, 9, 3)
    for call in (emd_pairs, EMDPairs()):
        with pytest.raises(ValueError, match="same number of clouds"):
            call(a, torch.zeros(3, 9, 3))                          # unequal P
        with pytest.raises(ValueError):
            call(a, b)                                             # CPU tensors
        with pytest.raises(ValueError):
            call(a, b, countsA=[8, 9])                             # a count beyond the width
        with pytest.raises(ValueError):
            call(a, b, countsA=[8, 0])
        with pytest.raises(ValueError):
            call(a, b, countsB=[9, 9, 9])                          # one count per cloud
        with pytest.raises(ValueError, match="2048"):
            call(torch.zeros(1, 2049, 3), torch.zeros(1, 8, 3))    # the cap, checked before the device
        with pytest.raises(ValueError, match="2048"):
            call(torch.zeros(1, 8, 3), torch.zeros(1, 2049, 3))
        with pytest.raises(ValueError):
            call(a.double(), b.double())

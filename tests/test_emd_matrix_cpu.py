"""All-pairs Earth Mover's distance (csrc/emd_matrix.hip, dpdist_amd.emd: emd_matrix / EMDMatrix) without a GPU: the composed oracle's
own check, the floors behind the bars of tests/test_emd_matrix_gpu.py, and the argument errors of the C entries and the wrappers."""
import ctypes
import os

import numpy as np
import pytest

from tests import emd_matrix_cases as EC
from tests.test_emd_cpu import approx_match_pair, match_cost_pair

NAMES = ("dpd_emd_matrix_workspace_bytes", "dpd_emd_matrix_fwd", "dpd_emd_matrix_bwd")


def test_composed_gradient_is_the_derivative_of_the_weighted_matrix_with_the_matches_frozen():
    """2 x 2 clouds, ragged: dA and dB of the oracle against central differences of sum(W * dist) with every pair's match held"""
    rng = np.random.default_rng(3)
    A, B = rng.uniform(-0.8, 0.8, (2, 9, 3)), rng.uniform(-0.8, 0.8, (2, 7, 3))
    cA, cB = (9, 4), (5, 7)
    W = rng.standard_normal((2, 2))
    ref = EC.compose(A, B, cA, cB, W)
    match = {(i, j): approx_match_pair(A[i, :cA[i]], B[j, :cB[j]]) for i in range(2) for j in range(2)}

    def total(a, b):
        return sum(W[i, j] * match_cost_pair(a[i, :cA[i]], b[j, :cB[j]], match[i, j])[0] / cA[i] for i in range(2) for j in range(2))

    h = 1e-6
    for which, X, g, counts in ((0, A, ref["dA"], cA), (1, B, ref["dB"], cB)):
        for c in range(2):
            assert not g[c, counts[c]:].any()
            for k in range(counts[c]):
                for d in range(3):
                    p, q = X.copy(), X.copy()
                    p[c, k, d] += h
                    q[c, k, d] -= h
                    fd = (total(*((p, B) if which == 0 else (A, p))) - total(*((q, B) if which == 0 else (A, q)))) / (2 * h)
                    assert abs(fd - g[c, k, d]) <= 1e-8 + 1e-7 * abs(g[c, k, d]), (which, c, k, d, fd, g[c, k, d])


def test_recorded_floors_are_the_measured_ones():
    """FLOOR is the float32 restatement's worst deviation from float64 on the cases as measured when the test was written; numpy's exp
    and pairwise sums differ by an ulp between CPUs, so the recomputed floor has to stay within a factor of four of the recorded one"""
    worst = EC.floors()
    print("measured floors:", {q: "%.3g" % v for q, v in worst.items()})
    for q, v in worst.items():
        assert EC.FLOOR[q] / 4 <= v <= EC.FLOOR[q] * 4, (q, v, EC.FLOOR[q])


def test_cases_hold_what_they_are_for():
    A, B, cA, cB, _ = EC.make("dup_far")
    d0 = ((A[0][:, None, :] - B[0][None, :, :]) ** 2).sum(-1)
    assert (d0 == 0).sum() >= 16                                   # shared points
    assert np.exp(np.float32(-0.25) * ((A[:, :, None, 0] - B[1, None, None, :, 0]) ** 2).min()) == 0   # nothing moves before level 0
    A, B, cA, cB, _ = EC.make("self")
    assert B is A and cB == cA
    for name in EC.CASES:
        A, B, cA, cB, W = EC.make(name)
        assert W.shape == (len(cA), len(cB)) and max(A.shape[1], B.shape[1]) <= EC.MAX_POINTS
        assert all(1 <= n <= A.shape[1] for n in cA) and all(1 <= m <= B.shape[1] for m in cB)


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
    from dpdist_amd import emd
    assert dpdist_amd.emd_matrix is emd.emd_matrix and dpdist_amd.EMDMatrix is emd.EMDMatrix
    assert emd.MAX_POINTS == EC.MAX_POINTS and "#define DPD_EMD_MAX_POINTS %d" % EC.MAX_POINTS in header


def test_workspace_bytes(lib):
    ws = lib.dpd_emd_matrix_workspace_bytes
    assert ws(2, 5, 3, 7) == 2 * 3 * (5 + 7) * 3 * 4
    assert ws(1, 2048, 1, 2048) == 4096 * 3 * 4
    assert ws(46340, 2048, 46340, 2048) == 46340 * 46340 * 4096 * 3 * 4          # 64-bit all the way
    for bad in ((0, 5, 3, 7), (2, 5, 0, 7), (2, 0, 3, 7), (2, 5, 3, 0), (2, 2049, 3, 7), (2, 5, 3, 2049), (-1, 5, 3, 7), (1 << 16, 5, 1 << 15, 7)):
        assert ws(*bad) == 0, bad


def test_refusals_without_a_device(lib):
    p = ctypes.c_void_p(1 << 30)                                  # any non-NULL "device address": nothing is dereferenced
    E_NULL, E_DIM, E_UNSUPPORTED, E_WORKSPACE = -1, -2, -3, -4
    fwd = lambda A, B, Ca, Na, Cb, Nb, cost, dist: lib.dpd_emd_matrix_fwd(A, p, Ca, Na, B, None, Cb, Nb, cost, dist, None)   # noqa: E731
    assert fwd(None, p, 2, 5, 3, 7, p, p) == E_NULL and fwd(p, None, 2, 5, 3, 7, p, p) == E_NULL and fwd(p, p, 2, 5, 3, 7, None, None) == E_NULL
    need = lib.dpd_emd_matrix_workspace_bytes(2, 5, 3, 7)
    bwd = lambda A, B, Ca, Na, Cb, Nb, W, dA, dB, ws, nb: lib.dpd_emd_matrix_bwd(A, None, Ca, Na, B, p, Cb, Nb, W, dA, dB, 0, ws, nb, None)   # noqa: E731
    for A, B, W, dA, dB in ((None, p, p, p, p), (p, None, p, p, p), (p, p, None, p, p), (p, p, p, None, None)):
        assert bwd(A, B, 2, 5, 3, 7, W, dA, dB, p, need) == E_NULL
    for Ca, Cb in ((0, 3), (2, 0), (-1, 3), (1 << 16, 1 << 15), (46341, 46341)):
        assert fwd(p, p, Ca, 5, Cb, 7, p, p) == E_DIM and bwd(p, p, Ca, 5, Cb, 7, p, p, p, p, 1 << 40) == E_DIM, (Ca, Cb)
    for Na, Nb in ((0, 7), (5, 0), (2049, 7), (5, 2049), (-3, 7)):
        assert fwd(p, p, 2, Na, 3, Nb, p, p) == E_UNSUPPORTED and bwd(p, p, 2, Na, 3, Nb, p, p, p, p, 1 << 40) == E_UNSUPPORTED, (Na, Nb)
    assert bwd(p, p, 2, 5, 3, 7, p, p, p, p, need - 1) == E_WORKSPACE and bwd(p, p, 2, 5, 3, 7, p, p, None, p, 0) == E_WORKSPACE
    assert bwd(p, p, 2, 5, 3, 7, p, p, p, None, need) == E_WORKSPACE


def test_wrappers_refuse_bad_arguments(lib):
    import torch
    from dpdist_amd import EMDMatrix, emd_matrix
    a, b = torch.zeros(2, 8, 3), torch.zeros(3, 9, 3)
    mod = EMDMatrix()
    for call in (emd_matrix, mod):
        with pytest.raises(ValueError):
            call(a, b)                                             # CPU tensors
        with pytest.raises(ValueError):
            call(a, b, countsA=[8, 9])                             # a count beyond the width
        with pytest.raises(ValueError):
            call(a, b, countsA=[8, 0])
        with pytest.raises(ValueError):
            call(a, b, countsB=[9, 9])                             # one count per cloud
        with pytest.raises(ValueError, match="countsB"):
            call(a, countsB=[8, 8])                                # countsB without cloudsB
        with pytest.raises(ValueError, match="2048"):
            call(torch.zeros(1, 2049, 3), torch.zeros(1, 8, 3))                # the cap, checked before the device
        with pytest.raises(ValueError, match="2048"):
            call(torch.zeros(1, 8, 3), torch.zeros(1, 2049, 3))
        with pytest.raises(ValueError):
            call(a.double(), b.double())

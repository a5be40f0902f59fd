"""Per-pair Chamfer / Hausdorff (csrc/chamfer_pairs.hip, dpdist_amd.baselines: chamfer_pairs / hausdorff_pairs / ChamferPairs) without a
GPU: the cases hold what they are for, the header, the library and the bindings agree, and the argument errors of the C entries and of
the wrappers come before any device work."""
import ctypes
import os

import numpy as np
import pytest

from tests import baseline_cases as BC
from tests import baseline_pairs_cases as PC

NAMES = ("dpd_chamfer_pairs_fwd", "dpd_chamfer_pairs_bwd")


def test_cases_hold_what_they_are_for():
    A, B, cA, cB = PC.chamfer_make("full")
    assert np.array_equal(A[0], B[0]) and np.array_equal(A[0, 0], A[0, 1])
    assert BC.d2_f32(B[0], A[0]).min(1).max() == 0                  # zero minima in the planted pair
    assert BC.d2_f32(B[0], A[0]).argmin(1)[1] == 0                  # the duplicate's tie goes to the lowest index
    A, B, cA, cB = PC.chamfer_make("ragged")
    assert 1 in cA and 1 in cB
    A, B, cA, cB = PC.chamfer_make("chunks")
    assert max(cA) > 256 and max(cB) > 256 and max(cB) % 256 and any(n <= A.shape[1] - 256 for n in cA)   # a chunk wholly in the padding
    for name in PC.CHAMFER_CASES:
        A, B, cA, cB = PC.chamfer_make(name)
        assert A.shape[0] == B.shape[0] == len(cA) == len(cB) and max(A.shape[1], B.shape[1]) <= PC.MAX_POINTS
        assert all(1 <= n <= A.shape[1] for n in cA) and all(1 <= m <= B.shape[1] for m in cB)
    assert PC.MANY[1] > 1 << 20 and PC.MANY[1] > 65535


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
    from dpdist_amd import baselines
    assert dpdist_amd.chamfer_pairs is baselines.chamfer_pairs and dpdist_amd.hausdorff_pairs is baselines.hausdorff_pairs
    assert dpdist_amd.ChamferPairs is baselines.ChamferPairs and baselines.MAX_POINTS == PC.MAX_POINTS
    from dpdist_amd import build
    assert "chamfer_pairs.hip" in build.SOURCES


def test_refusals_without_a_device(lib):
    p = ctypes.c_void_p(1 << 30)                                  # any non-NULL "device address": nothing is dereferenced
    E_NULL, E_DIM, E_UNSUPPORTED = -1, -2, -3

    def fwd(A=p, B=p, Wa=5, Wb=7, P=2, mins=(p, p, p, p), outs=(p, p, p)):
        return lib.dpd_chamfer_pairs_fwd(A, None, Wa, B, p, Wb, P, *mins, *outs, None)

    def bwd(A=p, B=p, Wa=5, Wb=7, P=2, form=0, args=(p, p), G=(p, p), d=(p, p)):
        return lib.dpd_chamfer_pairs_bwd(A, p, Wa, B, None, Wb, P, form, *args, *G, *d, None)

    assert fwd(A=None) == E_NULL and fwd(B=None) == E_NULL
    for k in range(4):
        assert fwd(mins=tuple(None if i == k else p for i in range(4))) == E_NULL, k
    assert bwd(A=None) == E_NULL and bwd(B=None) == E_NULL and bwd(args=(None, p)) == E_NULL and bwd(args=(p, None)) == E_NULL
    assert bwd(G=(None, None)) == E_NULL and bwd(d=(None, None)) == E_NULL
    for P in (0, -1):
        assert fwd(P=P) == E_DIM and bwd(P=P) == E_DIM
    for form in (-1, 2):
        assert bwd(form=form) == E_DIM
    for Wa, Wb in ((0, 7), (5, 0), (4097, 7), (5, 4097), (-3, 7)):
        assert fwd(Wa=Wa, Wb=Wb) == E_UNSUPPORTED and bwd(Wa=Wa, Wb=Wb) == E_UNSUPPORTED, (Wa, Wb)


def test_wrappers_refuse_bad_arguments(lib):
    import torch
    from dpdist_amd import ChamferPairs, chamfer_pairs, hausdorff_pairs
    a, b = torch.zeros(2, 8, 3), torch.zeros(2, 9, 3)
    for call in (chamfer_pairs, hausdorff_pairs, ChamferPairs(), ChamferPairs("sqrt")):
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
        with pytest.raises(ValueError, match="4096"):
            call(torch.zeros(1, 4097, 3), torch.zeros(1, 8, 3))    # the cap, checked before the device
        with pytest.raises(ValueError, match="4096"):
            call(torch.zeros(1, 8, 3), torch.zeros(1, 4097, 3))
        with pytest.raises(ValueError):
            call(a.double(), b.double())
        with pytest.raises((ValueError, TypeError)):
            call(a)                                                # no set against itself
    with pytest.raises(ValueError):
        chamfer_pairs(a, b, form="l1")
    with pytest.raises(ValueError):
        ChamferPairs("l1")

"""Exact-value edge tests of the window gather (csrc/patch_rows.hip, patch_rows_bwd.h) through its C entries dpd_patch_rows_fwd,
dpd_patch_rows_fwd_scaled, dpd_patch_rows_bwd, dpd_asloss_combine, dpd_stack_clouds and dpd_padded_width.

tests/window_cases.py holds the numpy references (none of them calls the library), the query / Fisher-vector / ssq families, the
checkers and the case tables; tests/test_window_edges_cpu.py holds the references to the oracle and proves that the checkers have
teeth.  The distinct-window and all-pairs suites compare their gathers with dpd_patch_rows_fwd_scaled; this file is what checks that
anchor against something independent.  Every comparison is an equality of bit patterns or of a return code: mask, voxel id, fp32 rows,
RC planes for all Q rows, R8 planes for exactly Qb rows, the backward's n-ascending float32 sums (and exact integer sums), every
buffer's guard bands.  The forward table reaches each of the six kernel forms at its smallest shapes (window_cases.fwd_cases: the
form stands next to each entry and is asserted against a restatement of the host's dispatch on the CPU): every m in 1 .. 10 and k
in {1, 3, 5, 7} through both fp32 forms, every cell face of every m with its float32 neighbours (the gaps of m = 6, 7, 9, 10, where
0.0 belongs to no cell for m = 6 and 10), NaN / inf / +-1, clipped corner windows, ssq scales at the 1e-12 clamp, Qb < Q and Qb = 0,
the fall-backs between the forms and the one refusal."""
import ctypes

import numpy as np
import pytest
import torch

from dpdist_amd import lib as L

from . import window_cases as W

pytestmark = pytest.mark.gpu

FWD = W.fwd_cases()
BWD = W.bwd_cases()


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible")
    L.load()     # raises if the HIP extension is missing -- never fall back
    return torch.device("cuda:0")


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def call_fwd(run):
    """dpd_patch_rows_fwd_scaled with the run's buffers (dpd_patch_rows_fwd where the case has no ssq); returns the code"""
    case, lib = run.case, L.load()
    pl = run.descriptor()
    args = (case.C, case.N, case.m, case.k, run.KP, P(run.X), P(run.mask), P(run.vox), None if pl is None else ctypes.byref(pl), L.cur_stream())
    if run.ssq is None:
        return lib.dpd_patch_rows_fwd(P(run.q), P(run.fv), *args)
    return lib.dpd_patch_rows_fwd_scaled(P(run.q), P(run.fv), P(run.ssq), *args)


@pytest.mark.parametrize("case", FWD, ids=[c.id for c in FWD])
def test_forward_case(dev, case):
    """one launch on one table entry: return code, mask, vox, X, RC / R8 planes, untouched plane buffers and every guard band
    (window_cases.check_fwd)"""
    run = W.FwdRun(case, dev)
    W.check_fwd(run, call_fwd(run))


def test_unscaled_entry_is_the_scaled_entry_without_ssq(dev):
    """dpd_patch_rows_fwd_scaled(ssq = NULL) and dpd_patch_rows_fwd are one function"""
    case = W.fwd_case("L-3x16")
    run = W.FwdRun(case, dev)
    code = L.load().dpd_patch_rows_fwd_scaled(P(run.q), P(run.fv), None, case.C, case.N, case.m, case.k, run.KP, P(run.X), P(run.mask),
                                               P(run.vox), None, L.cur_stream())
    W.check_fwd(run, code)


# ------------------------------------------------------------------------------------------------ backward
def call_bwd(run):
    case = run.case
    code = L.load().dpd_patch_rows_bwd(P(run.dX), P(run.vox), case.C, case.N, case.m, case.k, W.kp(case), P(run.dq), P(run.dfv), L.cur_stream())
    assert code == 0, code


@pytest.mark.parametrize("case", BWD, ids=[c.id for c in BWD])
def test_backward_case(dev, case):
    """dfv bit for bit against the n-ascending float32 sums (integer dX: the exact int64 sums), dq a copy of the three columns; masked
    queries add to the window of voxel 0; columns behind E + 3 hold NaN and are never read"""
    run = W.BwdRun(case, dev)
    call_bwd(run)
    W.check_bwd(run)


@pytest.mark.parametrize("cid,rws", W.ONEHOT_CASES, ids=[c for c, _ in W.ONEHOT_CASES])
def test_backward_is_the_elementwise_transpose(dev, cid, rws):
    """dX one-hot at (row, column): dfv is one-hot, with the same value, at the (cell, channel) the forward reads that column from,
    and all zero for a clipped column"""
    case = W.bwd_case(cid)
    d = W.bwd_data(case)
    E = W.E_of(case.k)
    for row in rws:
        for col, src in W.onehot_columns(case, row):
            dX = d.dX.copy()
            dX[:, :E + 3] = 0.0
            dX[row, col] = 1.5
            want = np.zeros((case.C, case.m ** 3, W.F), np.float32)
            if src is not None:
                want[row // case.N, src[0], src[1]] = 1.5
            run = W.BwdRun(case, dev, dX=dX, dq=False)
            call_bwd(run)
            W.check_bwd(run, (want, None))


# ------------------------------------------------------------------------------------------------ combine, stack, padded width
@pytest.mark.parametrize("case", W.combine_cases(), ids=[c.id for c in W.combine_cases()])
def test_asloss_combine_case(dev, case):
    run = W.CombineRun(case, dev)
    code = L.load().dpd_asloss_combine(P(run.dpts), P(run.dX), P(run.scale), case.B, case.N, case.k, W.kp(case), P(run.gA), P(run.gB), L.cur_stream())
    assert code == 0, code
    run.check()


@pytest.mark.parametrize("noise", [False, True])
@pytest.mark.parametrize("B,N", W.COMBINE_SHAPES)
def test_stack_clouds_case(dev, B, N, noise):
    run = W.StackRun(B, N, noise, dev)
    code = L.load().dpd_stack_clouds(P(run.pcA), P(run.pcB), P(run.noise), B, N, P(run.pts), P(run.q), L.cur_stream())
    assert code == 0, code
    run.check()


def test_padded_width():
    lib = L.load()
    for k, w in W.PADDED_WIDTHS.items():
        assert lib.dpd_padded_width(k) == w == (k ** 3 * 20 + 3 + 31) // 32 * 32

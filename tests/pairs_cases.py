"""Paired DPDist for clouds of different sizes (dpdist_amd.pairs: dpd_patch_rows_fwd_counts, dpd_decoder_out_pairs, dpd_pairs_combine,
dpdist_pairs / DPDistPairs, the counts of DPDistLoss): cases and the composed float64 oracle, for tests/test_pairs_gpu.py;
tests/test_pairs_cpu.py runs the admission of every case here without a GPU.  The oracle of one direction, the weights, the bars and the
checkers are those of tests/ragged_cases.py, tests/test_cross_gpu.py and tests/test_cross_grad_gpu.py (imported, not restated).  Not a
test module and not a conftest.

A set is a padded tensor [B, W, 3] plus counts [B]; pair b is (A_b[:nA[b]], B_b[:nB[b]]).  The reference of a pair is the oracle of
tests/ragged_cases.py on the two TRUNCATED clouds alone, one call per pair and direction.
"""
import functools

import numpy as np
import torch

from dpdist_amd import synth

from . import ragged_cases as RC
from . import test_cross_gpu as X
from . import test_cross_grad_gpu as XG

M_GRID, K_WIN, H_DEC, KP, NG = X.M_GRID, X.K_WIN, X.H_DEC, X.KP, X.NG
E = XG.E
FWD_BAR, ADMIT_FWD, ADMIT_GRAD = RC.FWD_BAR, RC.ADMIT_FWD, RC.ADMIT_GRAD
NAN_OUT = RC.M.NAN_OUT
U24 = XG.U24

# the bar of a pair mean against the float64 mean of the fp32 pred[:, 0] it was formed from: a depth-12 fp32 tree over at most 4096 values
# in [0, 2] (an exact sum with one rounding lies inside it)
DD_BAR = 12 * U24 * 2

# ------------------------------------------------------------------------------------------------ the reference case
COUNTS_A, COUNTS_B = (64, 37, 5), (40, 1, 23)
# (P, Wa, Wb, countsA, countsB) of the output-layer and combine entries: the smallest; the reference counts (segments of 37, 5, 1 rows that
# align with nothing, the two halves of different lengths); rectangular without counts, Q = 176 rows (no multiple of 32)
ENTRY_SHAPES = ((1, 1, 1, None, None), (3, 64, 40, COUNTS_A, COUNTS_B), (2, 24, 64, None, None))


@functools.lru_cache(maxsize=None)
def sets():
    """A [3, 64, 3] with counts (64, 37, 5), B [3, 40, 3] with counts (40, 1, 23): float32, read-only"""
    A = np.ascontiguousarray(synth.s2_modelnet_shaped(3, 64, 100)[0].astype(np.float32))
    B = np.ascontiguousarray(synth.s2_modelnet_shaped(3, 40, 101)[1].astype(np.float32))
    for t in (A, B):
        t.setflags(write=False)
    return A, B


@functools.lru_cache(maxsize=None)
def rect_sets():
    """rectangular, no counts: A [2, 64, 3], B [2, 24, 3]"""
    A = np.ascontiguousarray(synth.s2_modelnet_shaped(2, 64, 100)[0].astype(np.float32))
    B = np.ascontiguousarray(synth.s2_modelnet_shaped(2, 24, 101)[1].astype(np.float32))
    for t in (A, B):
        t.setflags(write=False)
    return A, B


@functools.lru_cache(maxsize=None)
def large_sets(Wa, Wb):
    """one pair beyond the plain encoder's caps: A [1, Wa, 3], B [1, Wb, 3]"""
    seed = RESEED.get((Wa, Wb), 100)
    A = np.ascontiguousarray(synth.s2_modelnet_shaped(1, Wa, seed)[0].astype(np.float32))
    B = np.ascontiguousarray(synth.s2_modelnet_shaped(1, Wb, seed + 1)[1].astype(np.float32))
    for t in (A, B):
        t.setflags(write=False)
    return A, B


LARGE = ((712, 64), (1640, 8))        # the forward over tiles of points; the backward over tiles too
# seeds replaced because the float32 autograd oracle they gave missed the admission (tests/test_pairs_cpu.py): at seed 100 the gradient of
# the 712-point cloud lies 1.5e-2 from float64 (a near-tie the two precisions resolve differently), at seed 108 5e-7
RESEED = {(712, 64): 108}


def full(P):
    return (P.shape[1],) * P.shape[0]


@functools.lru_cache(maxsize=None)
def upstream(B):
    """G, G_AB, G_BA [B]: the random upstream vectors (float32, fixed seed), as tests/test_cross_grad_gpu.py draws its matrices (the draw
    keyed by the 104 rows of a reference pair: no pair's G_AB + G / 2 or G_BA + G / 2 comes out below 0.24, so every cloud of the reference
    case has a gradient with structure -- the draw keyed by 7 left 0.006 on pair 1; tests/test_pairs_cpu.py asserts it per cloud)"""
    return tuple(g[:, 0].copy() for g in XG._upstream((B, 1, 104)))


def _pairs(a, b, dtype):
    """(D, D_AB, D_BA) [B] of the lists of truncated clouds a, b: one oracle call per pair and direction"""
    d_ab = torch.stack([RC.directed([x], [y], dtype)[0, 0] for x, y in zip(a, b)])
    d_ba = torch.stack([RC.directed([y], [x], dtype)[0, 0] for x, y in zip(a, b)])
    return (d_ab + d_ba) / 2, d_ab, d_ba


def oracle(A, B, cA, cB, dtype):
    """float64 numpy (D, D_AB, D_BA) [B] of the oracle run in `dtype` on the truncated clouds"""
    with torch.no_grad():
        out = _pairs(RC._truncated(A, cA, dtype, False), RC._truncated(B, cB, dtype, False), dtype)
    return tuple(t.double().numpy() for t in out)


def oracle_grads(A, B, cA, cB, dtype):
    """gradients of (G D).sum() + (G_AB D_AB).sum() + (G_BA D_BA).sum() through the same composition, at the padded shapes (zeros on the
    padding) -> (gA, gB) float64 numpy"""
    a, b = RC._truncated(A, cA, dtype, True), RC._truncated(B, cB, dtype, True)
    loss = XG._loss(_pairs(a, b, dtype), upstream(len(a)), True, dtype)
    g = torch.autograd.grad(loss, a + b)
    return RC._padded_grads(a, g[:len(a)], A.shape[1]), RC._padded_grads(b, g[len(a):], B.shape[1])


def _case(name):
    if name == "reference":
        return sets() + (COUNTS_A, COUNTS_B)
    if name == "rect":
        A, B = rect_sets()
    else:
        A, B = large_sets(*name)
    return A, B, full(A), full(B)


@functools.lru_cache(maxsize=None)
def case_oracle(name, dtype):
    return oracle(*_case(name), dtype)


@functools.lru_cache(maxsize=None)
def case_grads(name, dtype):
    return oracle_grads(*_case(name), dtype)


def grad_bars(name):
    """[(ref, bar)] for gA, gB, formed as tests/ragged_cases.py: grad_bars forms them"""
    r64, r32 = case_grads(name, torch.float64), case_grads(name, torch.float32)
    return [(a, max(4.0 * np.abs(b - a).max(), 2e-4 * max(1.0, np.abs(a).max()))) for a, b in zip(r64, r32)]


def seg_rows(P, Wa, Wb, cA, cB):
    """[(direction, pair, first row, width, count)] of the row layout: the AB half (queries B, Wb rows per pair) first, the BA half at P Wb"""
    cA, cB = cA or (Wa,) * P, cB or (Wb,) * P
    return [(0, b, b * Wb, Wb, cB[b]) for b in range(P)] + [(1, b, P * Wb + b * Wa, Wa, cA[b]) for b in range(P)]

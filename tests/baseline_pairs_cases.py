"""Cases and helpers of the per-pair baselines (dpd_chamfer_pairs_fwd / _bwd, dpd_emd_pairs_fwd / _bwd; dpdist_amd: chamfer_pairs,
hausdorff_pairs, ChamferPairs, emd_pairs, EMDPairs), shared by tests/test_baseline_pairs_*.py and tests/test_emd_pairs_*.py.  Not a test
module.  The restatements, oracles and bars are those of tests/baseline_cases.py, tests/emd_matrix_cases.py and tests/test_emd_cpu.py,
applied pair by pair; points are drawn as baseline_cases.draw and emd_matrix_cases.make draw them.

Chamfer / Hausdorff cases: smallest shapes at which the kernels take another path -- a workgroup scans 256 queries of one (pair,
direction), a finish workgroup reduces a (pair, direction), the gradient kernel owns 256 points of one (pair, set).

EMD cases: the diagonals of emd_matrix_cases (pair b = cloud b of A with cloud b of B, upstream W[b, b]).  `self` is left out: a cloud
against itself has a distance near 0, so a bar relative to the largest magnitude says nothing.  Tolerances, by the rule of
emd_matrix_cases: EMD_FLOOR[q] is the worst deviation of the restatement run in float32 from the float64 run over EMD_ORACLE_CASES,
relative to the case's largest float64 magnitude of q, measured on the CPU and rounded up; the GPU bar is GPU_FACTOR = 8 times that.
tests/test_emd_pairs_cpu.py recomputes the floors and holds them within a factor of four.

    measured floors (numpy float32 vs float64)     dist 1.73e-7 (wide)   dA 5.24e-7 (tiles)   dB 1.50e-6 (tiles)
    recorded (rounded up)                          dist 1.8e-7           dA 5.3e-7            dB 1.6e-6
    GPU bars (8 x recorded)                        dist 1.44e-6          dA 4.24e-6           dB 1.28e-5
The matrix file's floors do not transfer: a pair alone has a smaller largest magnitude than a row or column of pairs summed.
"""
import functools

import numpy as np

from tests import baseline_cases as BC
from tests import emd_matrix_cases as EC

F = np.float32

# ------------------------------------------------------------------------------------------------ Chamfer / Hausdorff
# name: (seed, P, width of A, width of B, countsA, countsB)
CHAMFER = {
    "full": (20, 3, 64, 64, None, None),                              # B[0] = A[0], a duplicated surface point: zero minima, ties
    "ragged": (21, 4, 37, 70, (37, 5, 1, 20), (70, 33, 64, 1)),       # one-point clouds on either side
    "chunks": (22, 3, 300, 257, (300, 256, 1), (257, 1, 129)),        # several 256-query workgroups, a partial one, one wholly in padding
    "cap": (23, 1, 4096, 64, None, None),
    "caps": (24, 1, 4096, 4096, None, None),                          # both widths at the cap
}
CHAMFER_CASES = list(CHAMFER)
MANY = (25, (1 << 20) + 3, 1, 1)                                      # forward only: the stride over pairs, beyond a grid's y / z extent
MAX_POINTS = 4096


@functools.lru_cache(maxsize=None)
def chamfer_make(name):
    """-> (A [P,Wa,3], B [P,Wb,3], countsA, countsB) read-only, with the planted edges; counts are tuples (a full set: its width)"""
    seed, P, Wa, Wb, cA, cB = CHAMFER[name]
    A, B = BC.draw(seed, P, P, Wa, Wb)
    A[0, 1] = A[0, 0]                                                 # a duplicate surface point: every tie goes to index 0
    if name == "full":
        B[0] = A[0]                                                   # minima exactly 0 in both directions, sqrt-form gradient 0
    for a in (A, B):
        a.setflags(write=False)
    return A, B, tuple(cA or (Wa,) * P), tuple(cB or (Wb,) * P)


def chamfer_make_many():
    seed, P, Wa, Wb = MANY
    return BC.draw(seed, P, P, Wa, Wb)


@functools.lru_cache(maxsize=None)
def chamfer_upstreams(name):
    """random upstreams (G, G_ab, G_ba), each [P] float32, read-only"""
    P = CHAMFER[name][1]
    rng = np.random.default_rng(900 + CHAMFER_CASES.index(name))
    out = tuple(rng.standard_normal(P).astype(F) for _ in range(3))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def chamfer_fwd_oracle(name):
    """per pair, baseline_cases.directed_fwd of each direction -> {"ab": [dict per pair], "ba": [...]} (mean_sq / mean_rt float64, max_sq
    float32 exact, n)"""
    A, B, cA, cB = chamfer_make(name)
    out = {"ab": [], "ba": []}
    for b in range(len(cA)):
        out["ab"].append(BC.directed_fwd(A[b:b + 1], [cA[b]], B[b:b + 1], [cB[b]]))
        out["ba"].append(BC.directed_fwd(B[b:b + 1], [cB[b]], A[b:b + 1], [cA[b]]))
    return out


def chamfer_bwd_oracle(name, form, G=None, Gab=None, Gba=None):
    """per pair, baseline_cases.matrix_bwd on the pair alone under the pair's upstreams -> [(Grad A_b, Grad B_b)]"""
    A, B, cA, cB = chamfer_make(name)
    pick = lambda g, b: None if g is None else np.asarray(g, np.float64)[b].reshape(1, 1)   # noqa: E731
    return [BC.matrix_bwd(A[b:b + 1], [cA[b]], B[b:b + 1], [cB[b]], form, pick(G, b), pick(Gab, b), pick(Gba, b)) for b in range(len(cA))]


# ------------------------------------------------------------------------------------------------ Earth Mover's distance
GPU_FACTOR = EC.GPU_FACTOR
EMD_FLOOR = {"dist": 1.8e-7, "dA": 5.3e-7, "dB": 1.6e-6}
# name: number of pairs taken from the diagonal of emd_matrix_cases' case of that name
EMD = {"tiny": 2, "tiles": 2, "dup_far": 2, "wide": 1, "cap": 1}
EMD_CASES = list(EMD)
EMD_ORACLE_CASES = [c for c in EMD_CASES if c != "cap"]               # cap: bitwise only


@functools.lru_cache(maxsize=None)
def emd_make(name):
    """-> (A [P,Wa,3], B [P,Wb,3], countsA, countsB, W [P]) read-only: pair b = (A_b, B_b) of emd_matrix_cases.make(name), W[b] its
    W[b, b]"""
    A, B, cA, cB, W = EC.make(name)
    P = EMD[name]
    out = (np.ascontiguousarray(A[:P]), np.ascontiguousarray(B[:P]), tuple(cA[:P]), tuple(cB[:P]),
           np.ascontiguousarray(np.diagonal(W)[:P]).astype(F))
    for a in (out[0], out[1], out[4]):
        a.setflags(write=False)
    return out


def emd_compose(A, B, cA, cB, W, dtype=np.float64):
    """emd_matrix_cases.compose pair by pair -> {"dist" [P], "dA" [P,Wa,3], "dB" [P,Wb,3]} in `dtype`; rows beyond the counts are 0"""
    out = {"dist": np.zeros(len(cA), dtype), "dA": np.zeros(A.shape, dtype), "dB": np.zeros(B.shape, dtype)}
    for b in range(len(cA)):
        one = EC.compose(A[b:b + 1], B[b:b + 1], cA[b:b + 1], cB[b:b + 1], np.asarray(W[b:b + 1]).reshape(1, 1), dtype)
        out["dist"][b], out["dA"][b], out["dB"][b] = one["dist"][0, 0], one["dA"][0], one["dB"][0]
    return out


@functools.lru_cache(maxsize=None)
def emd_oracle(name):
    """float64 oracle of a case, computed once per process and read-only"""
    out = emd_compose(*emd_make(name))
    for a in out.values():
        a.setflags(write=False)
    return out


def emd_deviation(got, want):
    """{quantity: largest |got - want| relative to the largest magnitude of the float64 `want`}"""
    return {q: float(np.abs(np.asarray(got[q], np.float64) - want[q]).max() / np.abs(want[q]).max()) for q in EMD_FLOOR}


def emd_floors():
    worst = dict.fromkeys(EMD_FLOOR, 0.0)
    for name in EMD_ORACLE_CASES:
        dev = emd_deviation(emd_compose(*emd_make(name), dtype=np.float32), emd_oracle(name))
        print(name, {q: "%.3g" % v for q, v in dev.items()})
        worst = {q: max(worst[q], dev[q]) for q in worst}
    return worst

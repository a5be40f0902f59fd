"""Cases and float64 oracle of the all-pairs Earth Mover's distance (dpd_emd_matrix_fwd / _bwd, dpdist_amd.emd: emd_matrix, EMDMatrix),
shared by tests/test_emd_matrix_cpu.py and tests/test_emd_matrix_gpu.py.  Not a test module.

The oracle is composed per pair from the restatement of the contract in tests/test_emd_cpu.py (approx_match_pair, match_cost_pair):
    dist[i,j] = cost(A_i[:n_i], B_j[:m_j]) / n_i
    dA[i]     = sum_j (W[i,j] / n_i) d cost / d xyz1 of the pair        dB[j] = sum_i (W[i,j] / n_i) d cost / d xyz2 of the pair
with the match a constant.  Points are uniform in [-0.8, 0.8]^3 with fixed seeds; on the device the padding holds a quiet NaN
(tests/baseline_cases.py: padded).

Tolerances, by the rule of tests/test_emd_cpu.py: FLOOR[q] is the worst deviation of the restatement run in float32 from the float64
run over CASES (without `cap`), relative to the case's largest float64 magnitude of q, measured on the CPU and rounded up; the GPU bar
is GPU_FACTOR = 8 times that.  tests/test_emd_matrix_cpu.py recomputes the floors and holds them within a factor of four.

    measured floors (numpy float32 vs float64)     dist 1.73e-7   dA 9.95e-7   dB 1.05e-6
    recorded (rounded up)                          dist 1.8e-7    dA 1.0e-6    dB 1.1e-6
    GPU bars (8 x recorded)                        dist 1.44e-6   dA 8.0e-6    dB 8.8e-6
The worst cases are wide (dist), self (dA) and tiles (dB); these clouds are small and evenly spread, so no point's mass hangs on a few
sharp weights and the floors stay two orders below those of tests/test_emd_cpu.py (whose worst cases are 64 / 2048-point batches).
"""
import functools

import numpy as np

from tests.test_emd_cpu import approx_match_pair, match_cost_pair

F = np.float32
GPU_FACTOR = 8.0
FLOOR = {"dist": 1.8e-7, "dA": 1.0e-6, "dB": 1.1e-6}
MAX_POINTS = 2048

# name: (Ca, Cb, width of A, width of B, countsA, countsB); Cb = None: the set against itself
SHAPES = {
    "tiny": (2, 3, 5, 7, (1, 5), (7, 2, 3)),                  # empty quarters, m < 4, n = 1
    "tiles": (2, 2, 130, 67, (65, 130), (63, 67)),            # several owner tiles with tails, per not dividing m, n != m both ways
    "dup_far": (2, 2, 48, 40, None, None),                    # d2 = 0 exactly; nothing moves before level 0
    "self": (3, None, 40, 40, (40, 17, 1), None),             # a set against itself, ragged
    "wide": (1, 2, 300, 257, None, None),                     # at and above the width from which four tiles are in flight
    "cap": (1, 1, 2048, 2048, None, None),                    # the LDS opt-in above 64 KiB; bitwise against dpd_emd_fwd only
}
CASES = list(SHAPES)
ORACLE_CASES = [c for c in CASES if c != "cap"]


@functools.lru_cache(maxsize=None)
def make(name):
    """-> (A [Ca,Na,3], B [Cb,Nb,3], countsA, countsB, W [Ca,Cb]) read-only; for "self" B is A and countsB is countsA"""
    Ca, Cb, Na, Nb, cA, cB = SHAPES[name]
    rng = np.random.default_rng(7300 + CASES.index(name))
    A = rng.uniform(-0.8, 0.8, (Ca, Na, 3)).astype(F)
    if Cb is None:
        B, Cb, cB = A, Ca, cA
    else:
        B = rng.uniform(-0.8, 0.8, (Cb, Nb, 3)).astype(F)
    if name == "dup_far":
        B[0, :16] = A[0, 20:36]                               # B_0 shares points with A_0: d2 = 0 exactly
        B[0, 30:] = B[0, :10]                                 # and repeats points of its own
        B[1, :, 0] += F(40.0)                                 # exp(-0.25 d2) = 0 in fp32 for every pair with B_1: nothing moves before level 0
    W = rng.standard_normal((Ca, Cb)).astype(F)
    cA = tuple(cA or (Na,) * Ca)
    cB = tuple(cB or (Nb,) * Cb)
    for a in (A, B, W):
        a.setflags(write=False)
    return A, B, cA, cB, W


def compose(A, B, cA, cB, W, dtype=np.float64):
    """the restatement, pair by pair -> {"dist" [Ca,Cb], "dA" [Ca,Na,3], "dB" [Cb,Nb,3]} in `dtype`; rows beyond the counts are 0"""
    T = dtype
    out = {"dist": np.zeros((len(cA), len(cB)), T), "dA": np.zeros(A.shape, T), "dB": np.zeros(B.shape, T)}
    for i, n in enumerate(cA):
        for j, m in enumerate(cB):
            x1, x2 = A[i, :n], B[j, :m]
            mt = approx_match_pair(x1, x2, T)
            c, g1, g2 = match_cost_pair(x1, x2, mt, T)
            out["dist"][i, j] = c / T(n)
            w = T(W[i, j]) / T(n)
            out["dA"][i, :n] += w * g1
            out["dB"][j, :m] += w * g2
    return out


@functools.lru_cache(maxsize=None)
def oracle(name):
    """float64 oracle of a case, computed once per process and read-only.  "self": dA and dB are the two routes of the one call (the
    module's gradient is their sum)"""
    out = compose(*make(name))
    for a in out.values():
        a.setflags(write=False)
    return out


def deviation(got, want):
    """{quantity: largest |got - want| relative to the largest magnitude of the float64 `want`}"""
    return {q: float(np.abs(np.asarray(got[q], np.float64) - want[q]).max() / np.abs(want[q]).max()) for q in FLOOR}


def floors():
    worst = dict.fromkeys(FLOOR, 0.0)
    for name in ORACLE_CASES:
        dev = deviation(compose(*make(name), dtype=np.float32), oracle(name))
        print(name, {q: "%.3g" % v for q, v in dev.items()})
        worst = {q: max(worst[q], dev[q]) for q in worst}
    return worst

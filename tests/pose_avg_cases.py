"""Exact-value cases of the pose network's AVERAGE-pool encoder (models/ipcr_model.py:236-271, `--pn_pool avg`;
csrc/pose_point.hip <.., AVG>, csrc/pose_point_bwd.hip pose_avg_*): the float64 reference, its wrong-on-purpose restatements and the
patterns of tests/test_pose_avg_gpu.py (tests/test_pose_avg_cpu.py proves on the CPU that every table entry keeps its exactness bound,
that the table holds the patterns the GPU cases are there for, and that the checker has teeth).  Not a test module and not a conftest.

The method, the integer networks, the clouds and the case table are those of tests/pose_cases.py.  From its layer-5 activations a5
[C, N, 1024] (integers, >= 0):

    S    = a5.sum(1)                      an integer; exact in fp32 in any order while it stays below 2^24
    f    = float32(S / N)                 ONE correctly rounded division.  The float64 quotient rounded to float32 equals the float32
                                          quotient (53 >= 2 * 24 + 2 bits: double rounding is innocuous for a quotient); the CPU module
                                          checks that on every case
    gate = a5 > 0                         packed like the tie words: bit b of word w is point 64 w + b
    df   = N * k                          k integers in [-3, 3], DENSE (every column of every cloud): coef = df / N is the integer k
    g5   = gate * k                       and the ten gradients follow as in pose_cases.point_backward

`bound` is the largest sum of absolute values of the terms of any reduction; it is asserted below 2^24 where it is computed."""
import functools

import numpy as np

from . import pose_cases as P
from .gemm_cases import EXACT

AVG_NAMES = ("f", "h1", "h2", "h3", "h4", "words") + P.POINT_NAMES[6:]
FORWARD_FAULTS = ("pad_in_sum", "div_64nw", "tie_bits", "drop_last")
BACKWARD_FAULTS = ("coef_popcount", "drop_cloud")


def origin_a5(net):
    """relu(layer 5) of the origin, the point a partial pass is padded with: [1024]"""
    return P.point_forward(net, np.zeros((1, 1, 3), dtype=np.int64))["a5"][0, 0]


def avg_forward(net, pts, fault=None):
    """pts [C, N, 3] integers -> dict h1 .. h4, a5, S [C, OUT], f [C, OUT] (the float32 quotient, held as float64), gate [C, N, OUT]
    bool, words (uint64), bound.

    fault (restatements that are WRONG on purpose, which the checker must reject):
      "pad_in_sum"  the origin rows that pad the last 64-point pass are summed
      "div_64nw"    the sum is divided by the padded point count 64 ceil(N / 64)
      "tie_bits"    the words are the max pool's tie words
      "drop_last"   the last point of a partial pass reaches neither the sum nor its word"""
    C, N, _ = pts.shape
    NW = (N + P.PP - 1) // P.PP
    fwd = P.point_forward(net, pts)
    a5 = fwd["a5"]
    live = np.ones(N, dtype=bool)
    if fault == "drop_last" and N % P.PP:
        live[N - 1] = False
    S = (a5 * live[None, :, None]).sum(1)
    if fault == "pad_in_sum":
        S = S + (NW * P.PP - N) * origin_a5(net)[None, :]
    gate = (a5 > 0) & live[None, :, None]
    div = NW * P.PP if fault == "div_64nw" else N
    bound = max(fwd["bound"], float(S.max()))
    if fault is None:
        assert bound < EXACT, ("the forward breaks the exactness bound", bound)
    out = {n: fwd[n] for n in ("h1", "h2", "h3", "h4", "a5")}
    out.update(S=S, f=np.float32(S / div).astype(np.float64), gate=gate, words=fwd["ties"] if fault == "tie_bits" else P.pack_ties(gate),
               bound=bound)
    return out


def avg_backward(net, pts, fwd, k, fault=None):
    """All ten gradients for df = N * k (k [C, OUT] integers): dict dW1 .. dW5, db1 .. db5, df, bound.

    fault: "coef_popcount"  coef = df / (number of open gates of the column) -- the max pool's even share -- instead of df / N
           "drop_cloud"     the last cloud is missing from dW5"""
    C, N, _ = pts.shape
    gate = fwd["gate"]
    df = float(N) * P._f64(k)
    coef = df / N
    assert np.array_equal(coef, P._f64(k))
    if fault == "coef_popcount":
        cnt = gate.sum(1)
        coef = np.where(cnt > 0, df / np.maximum(cnt, 1), 0.0)
    g = (gate * coef[:, None, :]).reshape(C * N, P.OUT)
    hs = [P._f64(pts).reshape(C * N, 3)] + [fwd["h%d" % l] for l in range(1, 5)]
    out, bound = {"df": df}, float(np.abs(df).max())
    for l in range(4, -1, -1):
        keep = (C - 1) * N if (fault == "drop_cloud" and l == 4) else C * N
        out["dW%d" % (l + 1)] = g[:keep].T @ hs[l][:keep]
        out["db%d" % (l + 1)] = g.sum(0)
        bound = max(bound, P._absdot(g.T, hs[l]), float(np.abs(g).sum(0).max()))
        if l:
            bound = max(bound, P._absdot(g, P._f64(net.W[l])))
            g = (g @ P._f64(net.W[l])) * (hs[l] > 0)
    if fault is None:
        assert bound < EXACT, ("the backward breaks the exactness bound", bound)
    out["bound"] = bound
    return out


def _want(fwd, bwd):
    want = {n: fwd[n] for n in AVG_NAMES[:6]}
    want.update({n: bwd[n] for n in AVG_NAMES[6:]})
    return want


@functools.lru_cache(maxsize=None)
def avg_reference(case):
    """everything the library must produce for a table entry of pose_cases.POINT_CASES under the average pool (computed once per
    process, shared, not modified): the forward dict, the backward dict, and `want` -- the arrays of AVG_NAMES"""
    net = P.point_net(case.net)
    pts = np.concatenate(P.point_clouds(case))
    fwd = avg_forward(net, pts)
    bwd = avg_backward(net, pts, fwd, P.point_k(case))
    want = _want(fwd, bwd)
    for v in want.values():
        v.setflags(write=False)
    return fwd, bwd, want


def avg_faulty(case, fault):
    """`want` of a wrong restatement (see avg_forward / avg_backward); the backward of a forward fault runs on the faulty forward"""
    net = P.point_net(case.net)
    pts = np.concatenate(P.point_clouds(case))
    fwd = avg_forward(net, pts, fault if fault in FORWARD_FAULTS else None)
    bwd = avg_backward(net, pts, fwd, P.point_k(case), fault if fault in BACKWARD_FAULTS else None)
    return _want(fwd, bwd)


def avg_patterns(case):
    """What the reference of a table entry holds of the patterns the GPU cases are there for: counts of (cloud, column)s or words"""
    fwd, _, _ = avg_reference(case)
    N = case.N
    zero = origin_a5(P.point_net(case.net))
    return {
        "partial_last_pass": int(N % P.PP != 0),
        "full_words": int((fwd["words"] == np.uint64(0xFFFFFFFFFFFFFFFF)).sum()),
        "origin_wins": int(((zero[None, :] > 0) & (fwd["S"] == 0)).sum()),          # a padded row would be the column's only term
        "dead": int((fwd["S"] == 0).sum()),
        "open_gates": float(fwd["gate"].mean()),
    }

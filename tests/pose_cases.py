"""Exact-value cases of the pose network's units (csrc/pose.hip, pose_point.hip, pose_point_bwd.hip, pose_head.hip): the float64
references, the integer networks and inputs, the checker and the case tables of tests/test_pose_edges_gpu.py
(tests/test_pose_edges_cpu.py proves on the CPU that every table entry keeps its exactness bound, that the tables hold the patterns the
GPU cases are there for, and that the checker has teeth).  Not a test module and not a conftest.

The method: an INTEGER network.  Points, biases and upstream gradients are small integers, weights are sparse with entries in
{-1, 0, 1}.  Every term of every reduction of the forward and the backward is then an integer, and while the sum of the ABSOLUTE
values of the terms of a reduction stays below 2^24 every partial sum -- in any order, with or without FMA, on the matrix cores or the
vector ALU -- is exactly representable in fp32.  A float64 restatement of the layers must then equal the library value for value: the
max pool's ties are exact equalities, no ReLU gate sits at rounding distance from zero, and the tie words follow from the reference
alone.  The upstream gradient of the pooled features is df = cnt * k (cnt = the reference's own tie count, k a small integer), so the
even share df / cnt is the integer k whatever the tie count.

Every reference returns, next to its values, `bound`: the largest sum of absolute values of the terms of any reduction that produced
one of them.  It is asserted below 2^24 where it is computed.
"""
import collections
import functools

import numpy as np

from .gemm_cases import EXACT

OUT = 1024                  # width of the pooled feature
PP = 64                     # points per pass of the shared MLP = bits per tie word
POINT_WIDTHS = ((3, 64), (64, 64), (64, 64), (64, 128), (128, 1024))          # (in, out) of the shared MLP
HEAD_WIDTHS = ((2048, 1024), (1024, 512), (512, 256), (256, 7))               # (in, out) of the head
POINT_NAMES = ("f", "h1", "h2", "h3", "h4", "ties") + tuple("dW%d" % i for i in range(1, 6)) + tuple("db%d" % i for i in range(1, 6))
HEAD_NAMES = ("h1", "h2", "h3", "pred", "dW1", "db1", "dW2", "db2", "dW3", "db3", "dW4", "db4", "df")

Net = collections.namedtuple("Net", "W b")          # int64 weights [out, in] and biases per layer


def _relu(x):
    return np.maximum(x, 0.0)


def _f64(x):
    return np.asarray(x, dtype=np.float64)


def _absdot(a, b):
    """largest sum_k |a[i, k]| |b[k, j]|"""
    return float((np.abs(a) @ np.abs(b)).max()) if a.size and b.size else 0.0


# ------------------------------------------------------------------------------------------------ integer networks
def sparse_pm1(rng, rows, cols, per_row):
    """[rows, cols] with exactly `per_row` entries of +-1 per row"""
    W = np.zeros((rows, cols), dtype=np.int64)
    for r in range(rows):
        W[r, rng.choice(cols, per_row, replace=False)] = rng.choice((-1, 1), per_row)
    return W


@functools.lru_cache(maxsize=None)
def point_net(variant="plain"):
    """The shared MLP with W1 dense in {-1, 0, 1}, four +-1 entries per row of W2 .. W5 and biases in [-2, 2].

    "dead":    b5 = -4096 everywhere: no column of any cloud has a positive maximum.
    "padwins": an ORIGIN DETECTOR is built into the first units of every layer, and b1 .. b4 of those units are set so that it is
               2 - |x| - |y| style arithmetic on integers:  h1[0..5] = relu(+-x), relu(+-y), relu(+-z);  h2[0..3] = relu(2 - two of
               |x|, |y|, |z|), which sum to 8 at the origin and to at most 6 at every other integer point;  h3[0..3] = relu(that sum - 6):
               2 at the origin, 0 elsewhere;  h4[0..3] = their sum: 8 at the origin, 0 elsewhere.  Every 16th column of W5 reads
               h4[0..3] with bias 0: it scores 32 at the origin -- the point the kernel pads a partial pass with -- and 0 at every
               real point, so the column is DEAD in every cloud that does not hold the origin, and a padded row that reaches the
               max or the tie word shows."""
    rng = np.random.default_rng({"plain": 11, "dead": 12, "padwins": 13}[variant])
    W = [rng.integers(-1, 2, size=(64, 3)).astype(np.int64)] + [sparse_pm1(rng, o, i, 4) for i, o in POINT_WIDTHS[1:]]
    b = [rng.integers(-2, 3, size=o).astype(np.int64) for _, o in POINT_WIDTHS]
    if variant == "dead":
        b[4][:] = -4096
    if variant == "padwins":
        W[0][:6] = [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]]
        b[0][:6] = 0
        for r, units in enumerate(((0, 1, 2, 3), (2, 3, 4, 5), (0, 1, 4, 5), (0, 1, 2, 3))):
            W[1][r] = 0
            W[1][r, list(units)] = -1
            b[1][r] = 2
        for l, bias in ((2, -6), (3, 0)):
            W[l][:4] = 0
            W[l][:4, :4] = 1
            b[l][:4] = bias
        W[4][5::16] = 0
        W[4][5::16, :4] = 1
        b[4][5::16] = 0
    return Net(tuple(W), tuple(b))


@functools.lru_cache(maxsize=None)
def head_net():
    """The head with eight +-1 entries per row of the three wide layers, a dense {-1, 0, 1} last layer and biases in [-2, 2]"""
    rng = np.random.default_rng(21)
    W = [sparse_pm1(rng, o, i, 8) for i, o in HEAD_WIDTHS[:3]] + [rng.integers(-1, 2, size=(7, 256)).astype(np.int64)]
    b = [rng.integers(-2, 3, size=o).astype(np.int64) for _, o in HEAD_WIDTHS]
    return Net(tuple(W), tuple(b))


# ------------------------------------------------------------------------------------------------ shared MLP: the reference
def pack_ties(tie):
    """[C, N, OUT] bool -> uint64 words [C, ceil(N / 64), OUT]: bit b of word w is point 64 w + b"""
    C, N, K = tie.shape
    NW = (N + PP - 1) // PP
    t = np.zeros((C, NW * PP, K), dtype=np.uint64)
    t[:, :N] = tie
    t = t.reshape(C, NW, PP, K) << np.arange(PP, dtype=np.uint64)[None, None, :, None]
    return np.bitwise_or.reduce(t, axis=2)


def unpack_ties(words, N):
    """uint64 words [C, NW, OUT] -> [C, NW * 64, OUT] bool (all bits, also those at or beyond N)"""
    C, NW, K = words.shape
    bits = (words[:, :, None, :] >> np.arange(PP, dtype=np.uint64)[None, None, :, None]) & np.uint64(1)
    return bits.reshape(C, NW * PP, K).astype(bool)


def point_forward(net, pts):
    """pts [C, N, 3] integers -> dict: h1 .. h4 [C N, width], a5 [C, N, OUT], f [C, OUT], tie [C, N, OUT] bool, cnt [C, OUT],
    ties (uint64 words), bound.  Bit set iff the point attains the column's maximum and that maximum is positive."""
    C, N, _ = pts.shape
    x = _f64(pts).reshape(C * N, 3)
    out, bound = {}, 0.0
    for l in range(5):
        W, b = _f64(net.W[l]), _f64(net.b[l])
        bound = max(bound, float((np.abs(x) @ np.abs(W).T + np.abs(b)).max()))
        x = _relu(x @ W.T + b)
        out["h%d" % (l + 1)] = x
    a5 = out.pop("h5").reshape(C, N, OUT)
    f = a5.max(1)
    tie = (a5 == f[:, None, :]) & (f[:, None, :] > 0)
    assert bound < EXACT, ("the forward breaks the exactness bound", bound)
    out.update(a5=a5, f=f, tie=tie, cnt=tie.sum(1), ties=pack_ties(tie), bound=bound)
    return out


def point_backward(net, pts, fwd, k, fault=None):
    """All ten gradients for df = cnt * k (k [C, OUT] integers): dict dW1 .. dW5, db1 .. db5, df, bound.

    fault (tests/test_pose_edges_cpu.py: restatements that are WRONG on purpose, which the checker must reject):
      "first_only"    the whole gradient of a column goes to its first tied point
      "cnt_one_word"  the share divides by the tied points of the point's own 64-point word instead of all of them
      "drop_cloud"    the last cloud is missing from every weight-gradient sum"""
    C, N, _ = pts.shape
    tie, cnt = fwd["tie"], fwd["cnt"]
    df = _f64(cnt) * _f64(k)
    share = np.where(cnt > 0, df / np.maximum(cnt, 1), 0.0)
    assert np.array_equal(share, np.rint(share)), "df / cnt is not an integer"
    g = tie * share[:, None, :]
    if fault == "first_only":
        first = tie & (np.cumsum(tie, axis=1) == 1)
        g = first * df[:, None, :]
    if fault == "cnt_one_word":
        words = unpack_ties(fwd["ties"], N).reshape(C, -1, PP, OUT)
        per_word = np.repeat(words.sum(2), PP, axis=1)[:, :N]                # tied points of the word each point lies in
        g = tie * (df[:, None, :] / np.maximum(per_word, 1))
    g = g.reshape(C * N, OUT)
    keep = C * N if fault != "drop_cloud" else (C - 1) * N
    hs = [_f64(pts).reshape(C * N, 3)] + [fwd["h%d" % l] for l in range(1, 5)]
    out, bound = {"df": df}, float(np.abs(df).max())
    for l in range(4, -1, -1):
        out["dW%d" % (l + 1)] = g[:keep].T @ hs[l][:keep]
        out["db%d" % (l + 1)] = g[:keep].sum(0)
        bound = max(bound, _absdot(g.T, hs[l]), float(np.abs(g).sum(0).max()))
        if l:
            bound = max(bound, _absdot(g, _f64(net.W[l])))
            g = (g @ _f64(net.W[l])) * (hs[l] > 0)
    if fault is None:
        assert bound < EXACT, ("the backward breaks the exactness bound", bound)
    out["bound"] = bound
    return out


def point_forward_passes(net, ptsA, ptsB, N, fault=None):
    """A second restatement of the forward, pass by pass as a kernel would run it: 64-row passes padded with the origin, one tie word
    per pass against the pass maximum, a running maximum, and the words of overtaken passes cleared at the end.  With fault = None
    it must equal `point_forward` (the CPU module asserts that).

    fault: "pad_in_max"  the padded rows of a partial pass take part in the pass maximum
           "drop_last"   the last point of a partial pass is left out
           "stale"       the word of a pass that a later pass overtook stays
           "b_offset"    cloud c of the second set is read at index c instead of c - nA (wrapped into the set)"""
    nA, nB = len(ptsA), len(ptsB)
    C = nA + nB
    clouds = [ptsA[c] if c < nA else ptsB[(c if fault == "b_offset" else c - nA) % nB] for c in range(C)]
    pts = _f64(np.stack(clouds))
    NW = (N + PP - 1) // PP
    hs = [np.zeros((C, N, o)) for _, o in POINT_WIDTHS[:4]]
    f = np.zeros((C, OUT))
    words = np.zeros((C, NW, OUT), dtype=np.uint64)
    stale = np.zeros((C, NW, OUT), dtype=bool)
    for w in range(NW):
        p0 = w * PP
        n = min(PP, N - p0)
        x = np.zeros((C, PP, 3))
        x[:, :n] = pts[:, p0:p0 + n]
        for l in range(5):
            x = _relu(x @ _f64(net.W[l]).T + _f64(net.b[l]))
            if l < 4:
                hs[l][:, p0:p0 + n] = x[:, :n]
        valid = n - 1 if (fault == "drop_last" and n < PP) else n
        pmax = x[:, :PP if fault == "pad_in_max" else valid].max(1) if valid else np.zeros((C, OUT))
        pmax = np.maximum(pmax, 0.0)
        higher, equal = pmax > f, (pmax == f) & (pmax > 0)
        stale[:, :w] |= higher[:, None, :] & (words[:, :w] != 0)
        m = np.where(higher | equal, pmax, 0.0)
        bits = np.zeros((C, PP, OUT), dtype=bool)
        bits[:, :valid] = (x[:, :valid] == m[:, None, :]) & (m[:, None, :] > 0)
        words[:, w] = pack_ties(bits)[:, 0]
        f = np.maximum(f, pmax)
    if fault != "stale":
        words[stale] = 0
    out = {"h%d" % (l + 1): hs[l].reshape(C * N, -1) for l in range(4)}
    out.update(f=f, ties=words)
    return out


# ------------------------------------------------------------------------------------------------ shared MLP: the table
PointCase = collections.namedtuple("PointCase", "id nA nB N kind net seed")
# kind: "plain" integers in [-4, 4]; "dup" the first half of every cloud repeated as its second half; "const" every point of a cloud
# equal; "far" no coordinate is 0 (the cloud does not hold the origin: the "padwins" net)


def _point_table():
    t = []
    add = lambda *a: t.append(PointCase("%s-%s-N%d-C%d+%d" % (a[4], a[3], a[2], a[0], a[1]), *a, seed=len(t)))      # noqa: E731
    for N in (1, 31, 32, 33, 63, 64, 65):           # one point; the second 32-row tile empty, partial, begun; the pass boundary
        add(2, 1, N, "plain", "plain")
    for N in (127, 128, 129, 200):                  # ties that span passes
        add(2, 1, N, "plain", "plain")
        add(2, 1, N, "dup", "plain")
    add(1, 0, 2048, "plain", "plain")               # 32 passes: bit 31 of the pass sets
    add(1, 1, 2048, "plain", "plain")
    for C in (64, 65, 66):                          # the 64-cloud outer loop of the dW5 role and its clamp
        add(C - 30, 30, 8, "plain", "plain")
    add(5, 0, 8, "plain", "plain")                  # the nA / nB split
    add(1, 4, 8, "plain", "plain")
    add(2, 1, 130, "const", "plain")                # cnt = N in every positive column, every word full up to N
    add(2, 1, 33, "far", "padwins")
    add(2, 1, 65, "far", "padwins")
    add(2, 1, 33, "plain", "dead")
    add(2, 1, 70, "plain", "dead")
    return tuple(t)


POINT_CASES = _point_table()


def point_clouds(case):
    """(ptsA [nA, N, 3], ptsB [nB, N, 3]) int64"""
    rng = np.random.default_rng(1000 + case.seed)
    C, N = case.nA + case.nB, case.N
    pts = rng.integers(-4, 5, size=(C, N, 3)).astype(np.int64)
    if case.kind == "dup":
        pts[:, N // 2:] = pts[:, :N - N // 2]
    if case.kind == "const":
        pts[:] = pts[:, :1]
    if case.kind == "far":
        pts = np.where(pts == 0, rng.choice((-1, 1), size=pts.shape), pts)
    return pts[:case.nA], pts[case.nA:]


def point_k(case):
    """the integer k [C, OUT] in [-3, 3] of df = cnt * k"""
    return np.random.default_rng(2000 + case.seed).integers(-3, 4, size=(case.nA + case.nB, OUT)).astype(np.int64)


@functools.lru_cache(maxsize=None)
def point_reference(case):
    """everything the library must produce for a table entry (computed once per process, shared, not modified): the forward dict, the
    backward dict, and `want` -- the arrays of POINT_NAMES as float64 (ties: uint64)"""
    net = point_net(case.net)
    A, B = point_clouds(case)
    pts = np.concatenate([A, B])
    fwd = point_forward(net, pts)
    bwd = point_backward(net, pts, fwd, point_k(case))
    want = {n: fwd[n] for n in ("f", "h1", "h2", "h3", "h4", "ties")}
    want.update({n: bwd[n] for n in POINT_NAMES[6:]})
    for v in want.values():
        v.setflags(write=False)
    return fwd, bwd, want


def point_patterns(case):
    """What the reference of a table entry holds of the patterns the GPU cases are there for: a dict of counts of (cloud, column)s"""
    fwd, _, _ = point_reference(case)
    C, N = case.nA + case.nB, case.N
    NW = (N + PP - 1) // PP
    a5 = np.zeros((C, NW * PP, OUT))
    a5[:, :N] = fwd["a5"]
    pmax = a5.reshape(C, NW, PP, OUT).max(2)                                   # pass maxima (relu outputs: >= 0)
    f, cnt = fwd["f"], fwd["cnt"]
    hit = fwd["ties"] != 0                                                     # [C, NW, OUT] passes that attain the maximum
    nhit = hit.sum(1)
    first, last = hit.argmax(1), NW - 1 - hit[:, ::-1].argmax(1)
    before = np.maximum.accumulate(np.concatenate([np.zeros((C, 1, OUT)), pmax[:, :-1]], 1), axis=1)      # running maximum before a pass
    below = (pmax > 0) & (pmax < f[:, None, :])
    return {
        "dead": int((f == 0).sum()),
        "last_pass_only": int(((nhit == 1) & hit[:, NW - 1] & (NW > 1)).sum()),
        "non_adjacent_passes": int(((nhit >= 2) & (last - first + 1 > nhit)).sum()),
        "overtaken_pass": int((below & (pmax > before)).any(1).sum()),         # its word was stored, then has to be cleared
        "smaller_later_pass": int((below & (pmax <= before)).any(1).sum()),    # its word is stored as zero at once
        "cnt_not_power_of_two": int(((cnt > 0) & ((cnt & (cnt - 1)) != 0)).sum()),
        "cnt_above_one": int((cnt > 1).sum()),
        "bit31_pass": int(hit[:, 31].sum()) if NW == 32 else 0,
        "full_words": int((fwd["ties"] == np.uint64(0xFFFFFFFFFFFFFFFF)).sum()),
    }


def origin_wins(case):
    """per cloud: the number of columns in which the origin scores above every real point"""
    fwd, _, _ = point_reference(case)
    zero = point_forward(point_net(case.net), np.zeros((1, 1, 3), dtype=np.int64))["f"]
    return (zero > fwd["f"]).sum(1)


# ------------------------------------------------------------------------------------------------ head: the reference and the table
HeadCase = collections.namedtuple("HeadCase", "id B mask")
HEAD_CASES = tuple(HeadCase("B%d-%s" % (B, "mask" if m else "nomask"), B, m) for B in (1, 15, 16, 17, 32, 33) for m in (False, True))


def head_inputs(case):
    """f [2B, 1024] integers in [-4, 4], the dropout mask [B, 256] in {0, 2} (or None), dpred [B, 7] integers in [-3, 3]"""
    rng = np.random.default_rng(3000 + case.B)
    f = rng.integers(-4, 5, size=(2 * case.B, OUT)).astype(np.int64)
    mask = 2 * rng.integers(0, 2, size=(case.B, 256)).astype(np.int64)
    dpred = rng.integers(-3, 4, size=(case.B, 7)).astype(np.int64)
    return f, (mask if case.mask else None), dpred


def head_forward(net, f, mask):
    """f [2B, 1024] (source rows, then template rows) -> dict x [B, 2048], h1, h2, h3 (mask applied), pred, bound"""
    B = len(f) // 2
    x = np.concatenate([_f64(f[:B]), _f64(f[B:])], 1)
    out, bound = {"x": x}, 0.0
    for l in range(4):
        W, b = _f64(net.W[l]), _f64(net.b[l])
        bound = max(bound, float((np.abs(x) @ np.abs(W).T + np.abs(b)).max()))
        x = x @ W.T + b
        if l < 3:
            x = _relu(x)
        if l == 2 and mask is not None:
            x = x * _f64(mask)
            bound = max(bound, float(np.abs(x).max()))
        out["h%d" % (l + 1) if l < 3 else "pred"] = x
    assert bound < EXACT, ("the head's forward breaks the exactness bound", bound)
    out["bound"] = bound
    return out


def head_backward(net, fwd, mask, dpred, fault=None):
    """the eight gradients and df [2B, 1024]; fault "drop_row": the last row of the batch is missing from every weight-gradient sum"""
    B = len(dpred)
    keep = B - 1 if fault == "drop_row" else B
    xs = [fwd["x"], fwd["h1"], fwd["h2"], fwd["h3"]]
    g = _f64(dpred)
    out, bound = {}, 0.0
    for l in range(3, -1, -1):
        out["dW%d" % (l + 1)] = g[:keep].T @ xs[l][:keep]
        out["db%d" % (l + 1)] = g[:keep].sum(0)
        bound = max(bound, _absdot(g.T, xs[l]), float(np.abs(g).sum(0).max()), _absdot(g, _f64(net.W[l])))
        g = g @ _f64(net.W[l])
        if l == 3 and mask is not None:
            g = g * _f64(mask)
            bound = max(bound, float(np.abs(g).max()))
        if l:
            g = g * (xs[l] > 0)
    out["df"] = np.concatenate([g[:, :OUT], g[:, OUT:]], 0)
    if fault is None:
        assert bound < EXACT, ("the head's backward breaks the exactness bound", bound)
    out["bound"] = bound
    return out


@functools.lru_cache(maxsize=None)
def head_reference(case):
    net = head_net()
    f, mask, dpred = head_inputs(case)
    fwd = head_forward(net, f, mask)
    bwd = head_backward(net, fwd, mask, dpred)
    want = {n: (fwd[n] if n in fwd else bwd[n]) for n in HEAD_NAMES}
    for v in want.values():
        v.setflags(write=False)
    return fwd, bwd, want


# ------------------------------------------------------------------------------------------------ refinement, first loop
RefineCase = collections.namedtuple("RefineCase", "id B N mask")
REFINE_CASES = tuple(RefineCase("B%d-N%d-%s" % (B, N, "mask" if m else "nomask"), B, N, m)
                     for B, N, m in ((1, 50, False), (1, 65, True), (17, 50, True), (17, 65, False)))
REFINE_LIM = 45.0           # the network's default rotation limit


def refine_inputs(case):
    """src, tmpl [B, N, 3] integers in [-4, 4]; the dropout mask [1, B, 256] in {0, 2} or None"""
    rng = np.random.default_rng(4000 + 100 * case.B + case.N)
    src = rng.integers(-4, 5, size=(case.B, case.N, 3)).astype(np.int64)
    tmpl = rng.integers(-4, 5, size=(case.B, case.N, 3)).astype(np.int64)
    mask = 2 * rng.integers(0, 2, size=(1, case.B, 256)).astype(np.int64)
    return src, tmpl, (mask if case.mask else None)


@functools.lru_cache(maxsize=None)
def refine_reference(case):
    """pred [B, 7] of the first loop on the integer network (exact), bound"""
    src, tmpl, mask = refine_inputs(case)
    pf = point_forward(point_net("plain"), np.concatenate([src, tmpl]))
    hf = head_forward(head_net(), np.rint(pf["f"]).astype(np.int64), None if mask is None else mask[0])
    return hf["pred"], max(pf["bound"], hf["bound"])


# ------------------------------------------------------------------------------------------------ pose algebra: the exact family
APPLY_N = (1, 63, 64, 65, 130)
APPLY_B = (1, 3)
# quaternions of norm exactly 1 or 2: the rotation is a signed permutation matrix and every fp32 operation of the chain is exact
EXACT_QUATS = ((0, 1, 0, 0), (1, 1, 1, 1), (0, 0, -1, 0), (1, -1, 1, -1), (-1, 0, 0, 0), (1, 1, -1, 1), (0, 0, 0, 1), (-1, -1, -1, 1))


def quat_to_mat64(q):
    """helper.py:552-554 on one quaternion, float64"""
    q0, q1, q2, q3 = _f64(q)
    return np.array([[q0 * q0 + q1 * q1 - q2 * q2 - q3 * q3, 2 * (q1 * q2 - q0 * q3), 2 * (q1 * q3 + q0 * q2)],
                     [2 * (q1 * q2 + q0 * q3), q0 * q0 + q2 * q2 - q1 * q1 - q3 * q3, 2 * (q2 * q3 - q0 * q1)],
                     [2 * (q1 * q3 - q0 * q2), 2 * (q2 * q3 + q0 * q1), q0 * q0 + q3 * q3 - q1 * q1 - q2 * q2]])


def apply_exact_case(B, N):
    """pred [B, 7], src [B, N, 3], T_in [B, 4, 4] (integers; last row 0 0 0 1) and the expected moved, T_out = M T_in and M = [R t; 0 1]
    itself, the composition onto the identity (float64, integers)"""
    rng = np.random.default_rng(5000 + 10 * N + B)
    pred = np.zeros((B, 7), dtype=np.int64)
    pred[:, :3] = rng.integers(-5, 6, size=(B, 3))
    for b in range(B):
        pred[b, 3:] = EXACT_QUATS[(b + N) % len(EXACT_QUATS)]
    src = rng.integers(-9, 10, size=(B, N, 3)).astype(np.int64)
    T = rng.integers(-3, 4, size=(B, 4, 4)).astype(np.int64)
    T[:, 3] = (0, 0, 0, 1)
    moved, T_out, Ms = np.zeros((B, N, 3)), np.zeros((B, 4, 4)), np.zeros((B, 4, 4))
    for b in range(B):
        q = _f64(pred[b, 3:])
        R = quat_to_mat64(q / np.sqrt((q * q).sum()))
        assert np.array_equal(R, np.rint(R)) and np.array_equal(np.abs(R).sum(0), np.ones(3)) and np.array_equal(np.abs(R).sum(1), np.ones(3))
        moved[b] = _f64(src[b]) @ R.T + _f64(pred[b, :3])
        M = np.eye(4)
        M[:3, :3], M[:3, 3] = R, _f64(pred[b, :3])
        T_out[b], Ms[b] = M @ _f64(T[b]), M
    return pred, src, T, moved, T_out, Ms


# ------------------------------------------------------------------------------------------------ the checker
def same_values(got, want, name):
    """Equality of VALUES, element for element: -0 equals +0 (a zero's sign carries no information in these sums), a NaN never matches.
    got: what the library wrote (any real dtype, or uint64 tie words); want: the reference."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        raise AssertionError("%s: shape %s, want %s" % (name, got.shape, want.shape))
    if want.dtype == np.uint64:
        got = got.view(np.uint64) if got.dtype == np.int64 else got
        assert got.dtype == np.uint64, (name, got.dtype)
        ok = got == want
    else:
        ok = got.astype(np.float64) == want.astype(np.float64)
    if not ok.all():
        idx = np.argwhere(~ok)
        i = tuple(int(v) for v in idx[0])
        raise AssertionError("%s: %d of %d elements differ; first at %s: got %r, want %r" % (name, len(idx), ok.size, i, got[i], want[i]))


def check(got, want, names):
    """every named array of `got` equals `want` (same_values)"""
    for n in names:
        same_values(got[n], want[n], n)


def rejects(got, want, names):
    """the name of the first array the checker rejects, or None"""
    for n in names:
        try:
            same_values(got[n], want[n], n)
        except AssertionError:
            return n
    return None

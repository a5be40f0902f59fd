"""The pose network's exact-value cases on the CPU (tests/pose_cases.py; the GPU module is tests/test_pose_edges_gpu.py): every table
entry keeps the exactness condition, the tables hold every pattern the GPU cases are there to exercise, two independent restatements
of the shared MLP's forward agree, and the checker rejects restatements that are wrong on purpose -- each of the mistakes a kernel of
this family can make without a tolerance test noticing."""
import numpy as np
import pytest

from . import pose_cases as P
from .gemm_cases import EXACT

POINT_IDS = [c.id for c in P.POINT_CASES]
FWD_NAMES = P.POINT_NAMES[:6]
BWD_NAMES = P.POINT_NAMES[6:]


def _case(net, kind, N, C=None):
    hits = [c for c in P.POINT_CASES if c.net == net and c.kind == kind and c.N == N and (C is None or c.nA + c.nB == C)]
    assert hits, (net, kind, N, C)
    return hits[0]


# ------------------------------------------------------------------------------------------------ the tables are what the issue lists
def test_point_table_holds_the_listed_shapes():
    have = {(c.nA + c.nB, c.N, c.kind, c.net) for c in P.POINT_CASES}
    for N in (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200):
        assert (3, N, "plain", "plain") in have
    for N in (127, 128, 129, 200):
        assert (3, N, "dup", "plain") in have
    assert {(1, 2048, "plain", "plain"), (2, 2048, "plain", "plain"), (3, 130, "const", "plain")} <= have
    assert all((C, 8, "plain", "plain") in have for C in (64, 65, 66))
    assert {(c.nA, c.nB) for c in P.POINT_CASES if c.nA + c.nB == 5} == {(5, 0), (1, 4)}
    assert {c.N for c in P.POINT_CASES if c.net == "padwins"} == {33, 65} and any(c.net == "dead" for c in P.POINT_CASES)
    assert all(c.N <= 200 or (c.N == 2048 and c.nA + c.nB <= 2) for c in P.POINT_CASES)          # the large size only with one or two clouds
    assert len(set(POINT_IDS)) == len(POINT_IDS)
    assert [c.B for c in P.HEAD_CASES if c.mask] == [1, 15, 16, 17, 32, 33] == [c.B for c in P.HEAD_CASES if not c.mask]
    assert {(c.B, c.N) for c in P.REFINE_CASES} == {(1, 50), (1, 65), (17, 50), (17, 65)}


def test_networks_are_sparse_integers():
    for variant in ("plain", "dead", "padwins"):
        net = P.point_net(variant)
        assert [w.shape for w in net.W] == [(o, i) for i, o in P.POINT_WIDTHS]
        assert all(set(np.unique(w)) <= {-1, 0, 1} for w in net.W)
        if variant != "padwins":
            assert all((np.abs(w).sum(1) == 4).all() for w in net.W[1:])
    head = P.head_net()
    assert [w.shape for w in head.W] == [(o, i) for i, o in P.HEAD_WIDTHS] and all(set(np.unique(w)) <= {-1, 0, 1} for w in head.W)


# ------------------------------------------------------------------------------------------------ exactness
@pytest.mark.parametrize("case", P.POINT_CASES, ids=POINT_IDS)
def test_point_case_is_exact(case):
    """every reduction of the forward and the backward keeps sum |terms| < 2^24, every value is an integer, df / cnt is an integer
    (asserted inside point_backward), and the two restatements of the forward agree"""
    fwd, bwd, want = P.point_reference(case)
    assert fwd["bound"] < EXACT and bwd["bound"] < EXACT
    for n in P.POINT_NAMES:
        if n != "ties":
            assert np.array_equal(want[n], np.rint(want[n])) and float(np.abs(want[n]).max(initial=0)) < EXACT, n
    NW = (case.N + P.PP - 1) // P.PP
    assert want["ties"].shape == (case.nA + case.nB, NW, P.OUT) and want["ties"].size == (case.nA + case.nB) * NW * 1024
    if case.N % P.PP:
        assert not (want["ties"][:, NW - 1] >> np.uint64(case.N % P.PP)).any()                      # no bit at or beyond N
    assert np.array_equal(P.unpack_ties(want["ties"], case.N)[:, :case.N], fwd["tie"])
    A, B = P.point_clouds(case)
    P.check(P.point_forward_passes(P.point_net(case.net), A, B, case.N), want, FWD_NAMES)
    if case.net == "dead":
        assert not want["f"].any() and not want["ties"].any() and not any(want[n].any() for n in BWD_NAMES)
    else:
        live = np.mean([float((want[n] > 0).mean()) for n in ("h1", "h2", "h3", "h4")])
        assert 0.2 < live < 0.8, live
        if case.N > 1:
            assert all(float((want[n] != 0).mean()) > 0.25 for n in BWD_NAMES), [float((want[n] != 0).mean()) for n in BWD_NAMES]


@pytest.mark.parametrize("case", P.HEAD_CASES, ids=[c.id for c in P.HEAD_CASES])
def test_head_case_is_exact(case):
    fwd, bwd, want = P.head_reference(case)
    assert fwd["bound"] < EXACT and bwd["bound"] < EXACT
    assert all(np.array_equal(v, np.rint(v)) and float(np.abs(v).max()) < EXACT for v in want.values())      # mask products included
    assert 0.2 < np.mean([float((want[n] > 0).mean()) for n in ("h1", "h2", "h3")]) < 0.8
    assert all(float((want[n] != 0).mean()) > (0.4 if case.B >= 15 else 0.1) for n in P.HEAD_NAMES[4:])


@pytest.mark.parametrize("case", P.REFINE_CASES, ids=[c.id for c in P.REFINE_CASES])
def test_refine_case_is_exact(case):
    pred, bound = P.refine_reference(case)
    assert bound < EXACT and np.array_equal(pred, np.rint(pred)) and pred.shape == (case.B, 7)
    assert np.abs(pred[:, 4:]).sum(1).min() > 0            # a rotation axis in every row: the pose moves the cloud


@pytest.mark.parametrize("N", P.APPLY_N)
@pytest.mark.parametrize("B", P.APPLY_B)
def test_apply_exact_case_is_a_signed_permutation(B, N):
    pred, src, T, moved, T_out, M = P.apply_exact_case(B, N)
    assert set(np.rint(np.sqrt((pred[:, 3:] ** 2).sum(1))).astype(int)) <= {1, 2}
    assert np.array_equal(moved, np.rint(moved)) and np.array_equal(T_out, np.rint(T_out)) and np.abs(moved).max() < 64
    assert np.array_equal(np.sort(np.abs(moved - pred[:, None, :3]), axis=2), np.sort(np.abs(src), axis=2))      # a permutation with signs
    assert np.array_equal(T_out[:, 3], T[:, 3]) and np.array_equal(M[:, :3, 3], pred[:, :3]) and np.array_equal(T_out, M @ T)


# ------------------------------------------------------------------------------------------------ pattern coverage
def test_point_table_covers_every_pattern():
    total = {}
    for case in P.POINT_CASES:
        pat = P.point_patterns(case)
        for k, v in pat.items():
            total[k] = total.get(k, 0) + v
        if case.N == 2048:
            assert pat["bit31_pass"] > 0, case.id                              # bit 31 of the pass sets
        if case.kind == "const":
            fwd = P.point_reference(case)[0]
            assert set(np.unique(fwd["cnt"])) <= {0, case.N} and pat["full_words"] > 0 and pat["cnt_not_power_of_two"] > 0
        if case.kind == "dup":
            fwd = P.point_reference(case)[0]
            assert float((fwd["cnt"][fwd["f"] > 0] >= 2).mean()) > 0.95
    print(total)
    for k in ("dead", "last_pass_only", "non_adjacent_passes", "overtaken_pass", "smaller_later_pass", "cnt_not_power_of_two", "cnt_above_one"):
        assert total[k] > 0, k
    plain = [c for c in P.POINT_CASES if c.net == "plain" and c.kind == "plain" and c.N > 1]
    assert all(float((P.point_reference(c)[0]["f"] > 0).mean()) > 0.5 for c in plain)


@pytest.mark.parametrize("case", [c for c in P.POINT_CASES if c.net == "padwins"], ids=lambda c: c.id)
def test_padding_would_win_in_every_cloud(case):
    """no cloud holds the origin, and in every cloud the origin -- the point a partial pass is padded with -- beats every real point
    in at least one column"""
    A, B = P.point_clouds(case)
    assert np.abs(np.concatenate([A, B])).sum(2).min() > 0
    wins = P.origin_wins(case)
    assert wins.shape == (case.nA + case.nB,) and wins.min() >= 1, wins
    assert case.N % P.PP                                                       # there ARE padded rows


# ------------------------------------------------------------------------------------------------ teeth
FORWARD_FAULTS = {
    "pad_in_max": [("padwins", "far", 33), ("padwins", "far", 65)],
    "drop_last": [("plain", "plain", 65), ("plain", "plain", 33), ("plain", "plain", 129)],
    "stale": [("plain", "plain", 200), ("plain", "plain", 129), ("plain", "plain", 2048)],
    "b_offset": [("plain", "plain", 8)],
}
BACKWARD_FAULTS = {
    "first_only": [("plain", "dup", 128), ("plain", "plain", 200)],      # (not the constant cloud: its tied points are equal, so is their share)
    "cnt_one_word": [("plain", "dup", 200), ("plain", "const", 130)],
    "drop_cloud": [("plain", "plain", 8), ("plain", "plain", 65)],
}


@pytest.mark.parametrize("fault", sorted(FORWARD_FAULTS))
def test_checker_rejects_a_wrong_forward(fault):
    found = []
    for net, kind, N in FORWARD_FAULTS[fault]:
        for case in (c for c in P.POINT_CASES if (c.net, c.kind, c.N) == (net, kind, N) and (fault != "b_offset" or c.nB > 1)):
            A, B = P.point_clouds(case)
            got = P.point_forward_passes(P.point_net(case.net), A, B, case.N, fault)
            found.append((case.id, P.rejects(got, P.point_reference(case)[2], FWD_NAMES)))
    print(found)
    assert found and any(name for _, name in found), found
    if fault == "pad_in_max":
        assert all(name == "f" for _, name in found)            # h1 .. h4 are right: the first array that differs is f
    if fault == "stale":
        assert all(name in (None, "ties") for _, name in found)


@pytest.mark.parametrize("fault", sorted(BACKWARD_FAULTS))
def test_checker_rejects_a_wrong_backward(fault):
    found = []
    for net, kind, N in BACKWARD_FAULTS[fault]:
        case = _case(net, kind, N)
        A, B = P.point_clouds(case)
        fwd, _, want = P.point_reference(case)
        got = P.point_backward(P.point_net(case.net), np.concatenate([A, B]), fwd, P.point_k(case), fault)
        found.append((case.id, P.rejects(got, want, BWD_NAMES)))
    print(found)
    assert all(name for _, name in found), found


def test_checker_rejects_a_row_left_out_of_the_heads_sums():
    for case in P.HEAD_CASES:
        fwd, _, want = P.head_reference(case)
        f, mask, dpred = P.head_inputs(case)
        got = P.head_backward(P.head_net(), fwd, mask, dpred, "drop_row")
        assert P.rejects(got, want, P.HEAD_NAMES[4:]) == "dW1", case.id


def test_checker_semantics():
    """-0 equals +0, NaN never matches (not even NaN), a single wrong tie bit and a wrong shape are mismatches"""
    a = np.array([0.0, 1.0, -2.0])
    P.same_values(np.array([-0.0, 1.0, -2.0], dtype=np.float32), a, "signed zero")
    for bad in (np.array([0.0, np.nan, -2.0]), np.array([0.0, 1.0, -2.0000002]), np.array([0.0, 1.0])):
        with pytest.raises(AssertionError):
            P.same_values(bad.astype(np.float32), a, "bad")
    with pytest.raises(AssertionError):
        P.same_values(np.array([np.nan], dtype=np.float32), np.array([np.nan]), "nan against nan")
    w = np.array([[5, 0]], dtype=np.uint64)
    P.same_values(w.view(np.int64), w, "words")
    with pytest.raises(AssertionError):
        P.same_values((w ^ np.uint64(1 << 63)).view(np.int64), w, "bit 63")
    assert np.array_equal(P.pack_ties(P.unpack_ties(w[None], 64)), w[None])

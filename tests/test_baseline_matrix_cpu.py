"""All-pairs Chamfer / Hausdorff, the host side: the test inputs' tie condition, the float32 restatement against float64, the bars
against simulated fp32 implementations, every refusal of the two C entries (before any HIP call), the Python argument errors, the exports."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import baseline_cases as BC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dpd_chamfer_matrix_fwd", "dpd_chamfer_matrix_bwd")


@pytest.fixture(scope="module")
def lib():
    from dpdist_amd import build, lib as L
    build.build(verbose=False)
    return L.load()


def _pairs(A, cA, B, cB):
    for i in range(len(cA)):
        for j in range(len(cB)):
            yield A[i, :cA[i]], B[j, :cB[j]]


@pytest.mark.parametrize("name", list(BC.CASES))
def test_inputs_have_no_argmin_ties(name):
    """the oracle (np.argmin) and the kernel must pair the same points: apart from the planted duplicate no query has two nearest points"""
    A, B, cA, cB = BC.make(name)
    assert (A[0, 1] == A[0, 0]).all()
    for a, b in _pairs(A, cA, B, cB):
        assert BC.ties(a, b) == 0 and BC.ties(b, a) == 0
    if name == "full":                                               # the planted zero minima and the tie they go through
        d = BC.d2_f32(B[0], A[0])
        assert (d.min(1) == 0).all() and d.argmin(1)[0] == 0 and d.argmin(1)[1] == 0 and (d[:2, :2] == 0).all()


def test_many_and_self_inputs_have_no_ties():
    A, B = BC.make_many()
    d = BC._full_scan(A, B)                                          # [2, 65537, 1, 2]
    assert (d[..., 0] != d[..., 1]).all()
    dt = BC._full_scan(B, A)                                         # one surface point: no tie possible
    assert dt.shape == (65537, 2, 2, 1)
    S = BC.make_self()
    for i in range(len(S)):
        for j in range(len(S)):
            if i != j:
                assert BC.ties(S[i], S[j]) == 0
    # a cloud against itself: every minimum is the point itself, 0, attained once
    assert all(((BC.d2_f32(s, s) == 0).sum(1) == 1).all() for s in S)


def test_added_shapes_have_no_ties():
    """the queries-per-thread case (1024 pairs) and the two-caps case; the stride case has one point per cloud: no tie possible"""
    S, Q, cS, cQ = BC.make_queries()
    assert sorted(set(-(-n // 256) for n in cQ)) == [1, 2, 3, 4]      # waves with 1 .. 4 live queries per thread
    for s_, q_ in _pairs(S, cS, Q, cQ):
        assert BC.ties(s_, q_) == 0
    A, B = BC.draw(*BC.CAPS)
    assert BC.ties(A[0], B[0]) == 0
    assert BC.STRIDE[1] > 1 << 20 and BC.STRIDE[3] == BC.STRIDE[4] == 1


def test_the_tie_counter_has_teeth():
    S = np.array([[0, 0, 0], [2, 0, 0], [2, 0, 0]], BC.F)
    assert BC.ties(S, np.array([[1, 0, 0]], BC.F)) == 1              # two different points at the same distance
    assert BC.ties(S, np.array([[1.5, 0, 0]], BC.F)) == 0            # the duplicate alone is no tie


@pytest.mark.parametrize("name", list(BC.CASES))
def test_restatement_against_float64(name):
    """d2 in float32 against float64 on the same inputs: three roundings of squares, two of sums, the differences' own: 6 u relative to
    the sum of squares is ample; and the minima's argmins agree with float64 wherever float64 separates the two best by more than that"""
    A, B, cA, cB = BC.make(name)
    for a, b in _pairs(A, cA, B, cB):
        d32 = BC.d2_f32(b, a)
        d64 = ((b[:, None, :].astype(np.float64) - a[None, :, :].astype(np.float64)) ** 2).sum(-1)
        assert (np.abs(d32 - d64) <= 6 * BC.U * d64).all()
        assert d32.dtype == BC.F


def _seq_sum(v):
    acc = BC.F(0)
    for x in v:
        acc = BC.F(acc + x)
    return acc


def _tree_sum(v):
    t = np.asarray(v, BC.F)
    while len(t) > 1:
        if len(t) % 2:
            t = np.append(t, BC.F(0))
        t = (t[0::2] + t[1::2]).astype(BC.F)
    return t[0]


@pytest.mark.parametrize("name", ["full", "ragged", "chunks"])
def test_mean_bar_holds_a_sequential_and_a_pairwise_fp32_sum(name):
    """the bar comes from the arithmetic, not from the kernel: two plain fp32 implementations stay well inside it.  Measured: 0.066
    (full), 0.244 (ragged), 0.164 (chunks) of the bar.  The 0.12 stated when the bar was set was measured against the float32 roots
    taken as exact; this oracle takes the roots in float64, so sqrtf's own half unit counts, and among the ragged case's short clouds
    (n = 1, 5) that half unit is a visible share of (n + 2) u.  Asserted: 0.3"""
    A, B, cA, cB = BC.make(name)
    worst = 0.0
    for S, cS, Q, cQ in ((A, cA, B, cB), (B, cB, A, cA)):
        ref = BC.directed_fwd(S, cS, Q, cQ)
        for i in range(len(cS)):
            for j in range(len(cQ)):
                mn = BC.d2_f32(Q[j, :cQ[j]], S[i, :cS[i]]).min(1)
                for vals, key in ((mn, "mean_sq"), (np.sqrt(mn), "mean_rt")):
                    for total in (_seq_sum(vals), _tree_sum(vals)):
                        ok, ratio = BC.mean_ok(BC.F(total / BC.F(len(vals))), ref[key][i, j], len(vals))
                        assert ok
                        worst = max(worst, ratio)
    print("worst error / bar", worst)
    assert worst < 0.3


@pytest.mark.parametrize("form", [0, 1])
def test_gradient_bar_holds_a_plain_fp32_implementation(form):
    """per-term fp32 arithmetic and a sequential fp32 sum, 1 / sqrtf standing in for the hardware reciprocal square root.  Measured
    on the ragged case under this upstream: 0.366 / 0.452 of the bar (squared: surface / query route), 0.326 / 0.310 (sqrt).  The 0.4
    stated when the bar was set came from another upstream and term order (2 * diff * w, where this one forms w * (2 * diff) as the
    kernel does); the query route's worst element sums a single term, where c = 4 is most of the bar.  Asserted: 0.5"""
    A, B, cA, cB = BC.make("ragged")
    W = np.random.default_rng(11).standard_normal((len(cA), len(cB))).astype(BC.F)
    refS, refQ = BC.directed_bwd(A, cA, B, cB, form, W)
    gS, gQ = np.zeros(A.shape, BC.F), np.zeros(B.shape, BC.F)
    for i in range(len(cA)):
        for j in range(len(cB)):
            s, q = A[i, :cA[i]], B[j, :cB[j]]
            d = BC.d2_f32(q, s)
            arg, mn = d.argmin(1), d.min(1)
            w = BC.F(W[i, j] / BC.F(cB[j]))
            for n in range(len(q)):
                diff = (q[n] - s[arg[n]]).astype(BC.F)
                if form == 0:
                    t = (w * (BC.F(2) * diff).astype(BC.F)).astype(BC.F)
                elif mn[n] == 0:
                    continue
                else:
                    t = (w * (BC.F(BC.F(1) / np.sqrt(mn[n])) * diff).astype(BC.F)).astype(BC.F)
                gQ[j, n] = (gQ[j, n] + t).astype(BC.F)
                gS[i, arg[n]] = (gS[i, arg[n]] - t).astype(BC.F)
    for got, ref in ((gS, refS), (gQ, refQ)):
        ok, ratio = BC.grad_ok(got, ref, 4 if form == 0 else 8)
        print("worst error / bar", ratio)
        assert ok and ratio < 0.5, ratio


def test_oracle_gradient_is_the_derivative_of_the_oracle_mean():
    """central differences of the float64 means (argmins fixed: the inputs have no ties) against the oracle's gradient, both forms"""
    A, B, cA, cB = BC.make("ragged")
    A64, B64 = A.astype(np.float64), B.astype(np.float64)
    W = np.random.default_rng(5).standard_normal((len(cA), len(cB)))

    def loss(S, Q, form):
        tot = 0.0
        for i in range(len(cA)):
            for j in range(len(cB)):
                d = ((Q[j, :cB[j], None, :] - S[i, None, :cA[i], :]) ** 2).sum(-1).min(1)
                tot += W[i, j] * (d if form == 0 else np.sqrt(d)).mean()
        return tot

    r = np.random.default_rng(6)
    for form in (0, 1):
        gS, gQ = BC.directed_bwd(A, cA, B, cB, form, W)
        for X, g, c, which in ((A64, gS.g, cA, 0), (B64, gQ.g, cB, 1)):
            for _ in range(6):
                k = int(r.integers(len(c)))
                n = int(r.integers(c[k]))
                if which == 0 and k == 0 and n < 2:
                    continue                                          # the duplicated point: the minimum is not differentiable there
                e = int(r.integers(3))
                h = 1e-6
                P, M = X.copy(), X.copy()
                P[k, n, e] += h
                M[k, n, e] -= h
                fd = (loss(P, B64, form) - loss(M, B64, form)) / (2 * h) if which == 0 else (loss(A64, P, form) - loss(A64, M, form)) / (2 * h)
                assert abs(fd - g[k, n, e]) <= 1e-6 * max(1.0, abs(fd)), (form, which, k, n, e)


def test_entries_are_declared_and_bound(lib):
    from dpdist_amd import lib as L
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dpdist_capi.h")).read(), flags=re.S)
    for name in NAMES:
        assert hasattr(lib, name) and name in L.SIGNATURES and re.search(r"\b%s\s*\(" % name, header), name
    decl = {n: re.search(r"\b%s\s*\(([^)]*)\)" % n, header).group(1).split(",") for n in NAMES}
    for name in NAMES:
        res, args = L.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == len(decl[name]), name
        for a, d in zip(args, decl[name]):
            assert (a is ctypes.c_int) == ("*" not in d), (name, d)


def test_forward_refusals_before_any_hip_call(lib):
    """a negative code is an argument error returned before the first HIP call: nothing was launched"""
    p = ctypes.c_void_p(1 << 30)                                     # any non-null "device address": nothing is dereferenced
    fwd = lambda S=p, Q=p, Cs=3, Ns=64, Cq=2, Nq=64, o=(p, p, p): lib.dpd_chamfer_matrix_fwd(S, None, Cs, Ns, Q, None, Cq, Nq, *o, None)   # noqa: E731
    assert fwd(S=None) == -1 and fwd(Q=None) == -1 and fwd(o=(None, None, None)) == -1
    assert fwd(Cs=0) == -2 and fwd(Cq=0) == -2 and fwd(Cs=-1) == -2
    assert fwd(Cs=1 << 16, Cq=1 << 15) == -2 and fwd(Cs=46341, Cq=46341) == -2        # Cs Cq >= 2^31
    assert fwd(Ns=4097) == -3 and fwd(Nq=4097) == -3 and fwd(Ns=0) == -3 and fwd(Nq=0) == -3 and fwd(Nq=-5) == -3
    assert fwd(S=None, Ns=4097) == -1                                # a missing pointer comes first


def test_backward_refusals_before_any_hip_call(lib):
    p = ctypes.c_void_p(1 << 30)
    bwd = lambda S=p, Q=p, Cs=3, Ns=64, Cq=2, Nq=64, form=0, W=p, dS=p, dQ=p: lib.dpd_chamfer_matrix_bwd(   # noqa: E731
        S, None, Cs, Ns, Q, None, Cq, Nq, form, W, dS, dQ, None)
    assert bwd(S=None) == -1 and bwd(Q=None) == -1 and bwd(W=None) == -1 and bwd(dS=None, dQ=None) == -1
    assert bwd(form=2) == -2 and bwd(form=-1) == -2
    assert bwd(Cs=0) == -2 and bwd(Cq=0) == -2 and bwd(Cs=1 << 16, Cq=1 << 15) == -2
    assert bwd(Ns=4097) == -3 and bwd(Nq=4097) == -3 and bwd(Ns=0) == -3 and bwd(Nq=0) == -3
    assert bwd(W=None, form=7) == -1


def test_exports():
    import dpdist_amd
    from dpdist_amd import baselines
    assert dpdist_amd.chamfer_matrix is baselines.chamfer_matrix
    assert dpdist_amd.hausdorff_matrix is baselines.hausdorff_matrix
    assert dpdist_amd.ChamferMatrix is baselines.ChamferMatrix
    assert "forward only" in baselines.hausdorff_matrix.__doc__.lower()
    assert "chamfer_matrix.hip" in __import__("dpdist_amd.build", fromlist=["SOURCES"]).SOURCES


def test_python_argument_errors(lib):
    from dpdist_amd import ChamferMatrix, chamfer_matrix, hausdorff_matrix
    a = torch.zeros(2, 64, 3)
    for fn in (chamfer_matrix, hausdorff_matrix, ChamferMatrix("sqrt")):
        with pytest.raises(ValueError, match="GPU"):
            fn(a)
        with pytest.raises(ValueError, match="GPU"):
            fn(a, torch.zeros(3, 36, 3))                             # different widths are allowed: the device check is what fails
        with pytest.raises(ValueError, match=r"\[C, N, 3\]"):
            fn(torch.zeros(64, 3))
        with pytest.raises(ValueError, match=r"\[C, N, 3\]"):
            fn(a, torch.zeros(2, 64, 2))
        with pytest.raises(ValueError, match="countsB given without cloudsB"):
            fn(a, countsB=[64, 64])
        with pytest.raises(ValueError, match="one count per cloud"):
            fn(a, countsA=[64])
        with pytest.raises(ValueError, match=r"\[1, 64\]"):
            fn(a, countsA=[64, 65])
        with pytest.raises(ValueError, match=r"\[1, 64\]"):
            fn(a, a, countsB=[0, 3])
        with pytest.raises(ValueError, match="integers"):
            fn(a, countsA=[1.5, 2.0])
        with pytest.raises(ValueError, match="cap is 4096"):
            fn(torch.zeros(1, 4097, 3))
        with pytest.raises(ValueError, match="cap is 4096"):
            fn(a, torch.zeros(1, 5000, 3))
    with pytest.raises(ValueError, match="form"):
        chamfer_matrix(a, form="l1")
    with pytest.raises(ValueError, match="form"):
        ChamferMatrix("root")
    assert ChamferMatrix().form == "squared"


def test_mapped_refusals():
    from dpdist_amd import baselines
    with pytest.raises(ValueError, match="refuses this shape"):
        baselines._check(-3, "dpd_chamfer_matrix_fwd")
    with pytest.raises(RuntimeError):
        baselines._check(-1, "dpd_chamfer_matrix_fwd")
    baselines._check(0, "dpd_chamfer_matrix_fwd")

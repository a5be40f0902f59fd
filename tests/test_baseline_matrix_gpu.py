"""All-pairs Chamfer / Hausdorff on the GPU (dpd_chamfer_matrix_fwd / _bwd, dpdist_amd/baselines.py) against the float32 restatement
(bit for bit) and the float64 oracle (at the bars) of tests/baseline_cases.py.  Outputs of the C entries sit in NaN-payload guard
bands, input padding holds a quiet NaN: padding that reached a result would poison it."""
import functools

import numpy as np
import pytest
import torch

from tests import baseline_cases as BC
from tests import gemm_cases as G

pytestmark = pytest.mark.gpu
DEV = "cuda"
CAP = 4096                 # points per cloud the entries take; a padded width cannot exceed it either
FORMS = {"squared": 0, "sqrt": 1}


@pytest.fixture(scope="module")
def lib():
    from dpdist_amd import build, lib as L
    build.build(verbose=False)
    return L.load()


@functools.lru_cache(maxsize=None)
def case(name):
    """(A, B, cA, cB) and the references of both directions, computed once and shared (nothing writes to them)"""
    A, B, cA, cB = BC.make(name)
    return A, B, cA, cB, BC.directed_fwd(A, cA, B, cB), BC.directed_fwd(B, cB, A, cA)


def dev_set(X, counts, width=None):
    """the set on the device: cut to its counts, padded to `width` with NaN; counts as an int32 device tensor"""
    width = X.shape[1] if width is None else width
    return torch.from_numpy(BC.padded(X, counts, width)).to(DEV), torch.tensor(counts, dtype=torch.int32, device=DEV)


def bits(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy()


def entry_fwd(lib, S, cS, Q, cQ, wS=None, wQ=None, counts=True):
    """dpd_chamfer_matrix_fwd into guard-banded outputs -> (mean_sq, mean_rt, max_sq) as numpy [Cs,Cq]; the bands are checked"""
    from dpdist_amd import lib as L
    s, sc = dev_set(S, cS, wS)
    q, qc = dev_set(Q, cQ, wQ)
    Cs, Cq = len(cS), len(cQ)
    outs = [G.banded_flat(Cs * Cq, device=DEV) for _ in range(3)]
    rc = lib.dpd_chamfer_matrix_fwd(L.ptr(s), L.ptr(sc) if counts else None, Cs, s.shape[1], L.ptr(q), L.ptr(qc) if counts else None, Cq, q.shape[1],
                                    *[L.ptr(v) for v, _ in outs], L.cur_stream())
    assert rc == 0
    torch.cuda.synchronize()
    for _, check in outs:
        check()
    return [v.cpu().numpy().reshape(Cs, Cq).copy() for v, _ in outs]


def entry_bwd(lib, S, cS, Q, cQ, form, W, wS=None, wQ=None):
    """dpd_chamfer_matrix_bwd into guard-banded gradients -> (dS [Cs,wS,3], dQ [Cq,wQ,3]) as torch CPU tensors; the bands are checked"""
    from dpdist_amd import lib as L
    s, sc = dev_set(S, cS, wS)
    q, qc = dev_set(Q, cQ, wQ)
    w = torch.from_numpy(np.ascontiguousarray(W, np.float32)).to(DEV)
    (ds, ck_s), (dq, ck_q) = G.banded_flat(s.numel(), device=DEV), G.banded_flat(q.numel(), device=DEV)
    rc = lib.dpd_chamfer_matrix_bwd(L.ptr(s), L.ptr(sc), len(cS), s.shape[1], L.ptr(q), L.ptr(qc), len(cQ), q.shape[1], form, L.ptr(w), L.ptr(ds),
                                    L.ptr(dq), L.cur_stream())
    assert rc == 0
    torch.cuda.synchronize()
    ck_s(), ck_q()
    return ds.cpu().view(s.shape).clone(), dq.cpu().view(q.shape).clone()


def assert_padding_is_plus_zero(g, counts):
    """rows at or beyond a cloud's count: the bit pattern of +0.0"""
    b = g.contiguous().view(torch.int32)
    for c, n in enumerate(counts):
        assert not b[c, n:].any(), c


@pytest.mark.parametrize("name", list(BC.CASES))
def test_forward_entry(lib, name):
    """both directions: max_sq bit for bit, the means at their bar; a second call, a wider padding and each pair alone give the same bits"""
    A, B, cA, cB, ref_ab, ref_ba = case(name)
    for S, cS, Q, cQ, ref in ((A, cA, B, cB, ref_ab), (B, cB, A, cA, ref_ba)):
        msq, mrt, mx = entry_fwd(lib, S, cS, Q, cQ)
        assert np.array_equal(mx.view(np.int32), ref["max_sq"].view(np.int32))
        for got, key in ((msq, "mean_sq"), (mrt, "mean_rt")):
            ok, ratio = BC.mean_ok(got, ref[key], ref["n"])
            print(name, key, "worst error / bar", ratio)
            assert ok, (key, ratio)
        again = entry_fwd(lib, S, cS, Q, cQ)
        wide = entry_fwd(lib, S, cS, Q, cQ, min(CAP, S.shape[1] + 29), min(CAP, Q.shape[1] + 131))
        for x, y, z in zip((msq, mrt, mx), again, wide):
            assert np.array_equal(x.view(np.int32), y.view(np.int32)) and np.array_equal(x.view(np.int32), z.view(np.int32))
        for i in range(len(cS)):
            for j in range(len(cQ)):
                alone = entry_fwd(lib, S[i:i + 1], [cS[i]], Q[j:j + 1], [cQ[j]], cS[i], cQ[j], counts=False)
                for x, y in zip((msq, mrt, mx), alone):
                    assert x[i, j].view(np.int32) == y[0, 0].view(np.int32), (i, j)
    if name == "full":
        assert msq[0, 0] == 0 and mrt[0, 0] == 0 and mx[0, 0] == 0      # B[0] = A[0]: exactly zero in either direction


@pytest.mark.parametrize("name", list(BC.CASES))
def test_matrices(lib, name):
    """chamfer_matrix (both forms) at the bar of D, hausdorff_matrix bit for bit, on NaN-padded sets with device counts"""
    from dpdist_amd import chamfer_matrix, hausdorff_matrix
    A, B, cA, cB, ref_ab, ref_ba = case(name)
    a, ca = dev_set(A, cA, min(CAP, A.shape[1] + 3))
    b, cb = dev_set(B, cB)
    for form, key in (("squared", "mean_sq"), ("sqrt", "mean_rt")):
        D, d_ab, d_ba = chamfer_matrix(a, b, form, True, countsA=ca, countsB=cb)
        assert torch.equal(chamfer_matrix(a, b, form, countsA=ca, countsB=cb), D)
        r_ab, r_ba = ref_ab[key], ref_ba[key].T
        n_ab, n_ba = ref_ab["n"], ref_ba["n"].T
        for got, ref, n, extra in ((d_ab, r_ab, n_ab, 2), (d_ba, r_ba, n_ba, 2), (D, (r_ab + r_ba) / 2, np.maximum(n_ab, n_ba), 3)):
            ok, ratio = BC.mean_ok(got.cpu().numpy(), ref, n, extra)
            assert ok, (form, ratio)
        assert torch.equal(D, (d_ab + d_ba) / 2)
    H, h_ab, h_ba = hausdorff_matrix(a, b, True, countsA=list(cA), countsB=cb)       # host counts on one side: checked and copied
    m_ab, m_ba = ref_ab["max_sq"], ref_ba["max_sq"].T
    assert np.array_equal(bits(H), np.sqrt(np.maximum(m_ab, m_ba)).view(np.int32))
    assert np.array_equal(bits(h_ab), np.sqrt(m_ab).view(np.int32)) and np.array_equal(bits(h_ba), np.sqrt(m_ba).view(np.int32))
    assert torch.equal(hausdorff_matrix(a, b, countsA=ca, countsB=cb), H)


def _upstreams(Ca, Cb, which, seed=17):
    r = np.random.default_rng(seed)
    g = [r.standard_normal((Ca, Cb)).astype(np.float32) for _ in range(3)]
    return (g[0], None, None) if which == "D" else tuple(g)


@pytest.mark.parametrize("which", ["D", "all"])
@pytest.mark.parametrize("form", ["squared", "sqrt"])
@pytest.mark.parametrize("name", list(BC.CASES))
def test_gradients(lib, name, form, which):
    """ChamferMatrix under an upstream on D alone and on D, D_AB, D_BA together, against the float64 oracle per element"""
    from dpdist_amd import ChamferMatrix
    A, B, cA, cB = case(name)[:4]
    f, c = (0, 4) if form == "squared" else (1, 8)
    ups = _upstreams(len(cA), len(cB), which)
    refA, refB = BC.matrix_bwd(A, cA, B, cB, f, *ups)
    a, ca = dev_set(A, cA)
    b, cb = dev_set(B, cB, B.shape[1] + 5)
    grads = []
    for _ in range(2):
        a_, b_ = a.clone().requires_grad_(), b.clone().requires_grad_()
        outs = ChamferMatrix(form)(a_, b_, True, countsA=ca, countsB=cb)
        loss = sum((o * torch.from_numpy(g).to(DEV)).sum() for o, g in zip(outs, ups) if g is not None)
        loss.backward()
        grads.append((a_.grad.cpu(), b_.grad.cpu()))
    (gA, gB), (gA2, gB2) = grads
    assert torch.equal(gA.view(torch.int32), gA2.view(torch.int32)) and torch.equal(gB.view(torch.int32), gB2.view(torch.int32))
    assert_padding_is_plus_zero(gA, cA), assert_padding_is_plus_zero(gB, cB)
    for got, ref, n in ((gA, refA, A.shape[1]), (gB, refB, B.shape[1])):
        ok, ratio = BC.grad_ok(got[:, :n].numpy(), ref, c)
        print(name, form, which, "worst error / bar", ratio)
        assert ok, ratio
    if name == "full" and form == "sqrt" and which == "D":
        # the pair (A_0, B_0 = A_0) has zero minima throughout: it adds nothing; the other pairs still reach both clouds
        only = BC.matrix_bwd(A[:1], cA[:1], B[:1], cB[:1], 1, ups[0][:1, :1])
        assert not only[0].S.any() and not only[1].S.any()
        z = torch.zeros(1, 1, device=DEV)
        a0 = a[:1].clone().requires_grad_()
        b0 = b[:1, :64].clone().requires_grad_()
        ChamferMatrix("sqrt")(a0, b0).backward(z + 1)
        assert not bits(a0.grad).any() and not bits(b0.grad).any()


@pytest.mark.parametrize("form", [0, 1])
def test_backward_entry_in_guard_bands(lib, form):
    """the entry itself on the ragged case: guard bands intact, padded rows +0.0 at a wider padding, the same bits at either width, and a
    NULL gradient skips its route without changing the other"""
    from dpdist_amd import lib as L
    A, B, cA, cB = case("chunks")[:4]
    W = np.random.default_rng(3).standard_normal((len(cA), len(cB))).astype(np.float32)
    dS, dQ = entry_bwd(lib, A, cA, B, cB, form, W)
    dSw, dQw = entry_bwd(lib, A, cA, B, cB, form, W, A.shape[1] + 77, B.shape[1] + 1)
    assert_padding_is_plus_zero(dSw, cA), assert_padding_is_plus_zero(dQw, cB)
    assert torch.equal(dS.view(torch.int32), dSw[:, :A.shape[1]].contiguous().view(torch.int32))
    assert torch.equal(dQ.view(torch.int32), dQw[:, :B.shape[1]].contiguous().view(torch.int32))
    refS, refQ = BC.directed_bwd(A, cA, B, cB, form, W)
    for got, ref in ((dS, refS), (dQ, refQ)):
        ok, ratio = BC.grad_ok(got.numpy(), ref, 8 if form else 4)
        assert ok, ratio
    s, sc = dev_set(A, cA)
    q, qc = dev_set(B, cB)
    w = torch.from_numpy(W).to(DEV)
    for skip in (0, 1):
        out, check = G.banded_flat((q if skip == 0 else s).numel(), device=DEV)
        rc = lib.dpd_chamfer_matrix_bwd(L.ptr(s), L.ptr(sc), len(cA), s.shape[1], L.ptr(q), L.ptr(qc), len(cB), q.shape[1], form, L.ptr(w),
                                        None if skip == 0 else L.ptr(out), L.ptr(out) if skip == 0 else None, L.cur_stream())
        assert rc == 0
        torch.cuda.synchronize()
        check()
        assert torch.equal(out.cpu().view(torch.int32), (dQ if skip == 0 else dS).reshape(-1).view(torch.int32))


def test_refusals_leave_the_outputs_untouched(lib):
    from dpdist_amd import lib as L
    x = torch.zeros(2, 8, 3, device=DEV)
    out, check = G.banded_flat(4 * 8 * 3, device=DEV)
    assert lib.dpd_chamfer_matrix_fwd(L.ptr(x), None, 2, 4097, L.ptr(x), None, 2, 8, L.ptr(out), None, None, L.cur_stream()) == -3
    assert lib.dpd_chamfer_matrix_fwd(L.ptr(x), None, 0, 8, L.ptr(x), None, 2, 8, L.ptr(out), L.ptr(out), L.ptr(out), L.cur_stream()) == -2
    assert lib.dpd_chamfer_matrix_bwd(L.ptr(x), None, 2, 8, L.ptr(x), None, 2, 8, 2, L.ptr(x), L.ptr(out), L.ptr(out), L.cur_stream()) == -2
    assert lib.dpd_chamfer_matrix_bwd(L.ptr(x), None, 2, 8, L.ptr(x), None, 2, 8, 0, None, L.ptr(out), L.ptr(out), L.cur_stream()) == -1
    torch.cuda.synchronize()
    check()
    assert G.untouched(out)


def test_many_clouds(lib):
    """65537 clouds on either side of a direction: no cloud index sits on a grid dimension that cannot hold it"""
    from dpdist_amd import ChamferMatrix, hausdorff_matrix
    A, B = BC.make_many()
    ref_ab, ref_ba = BC.full_fwd(A, B), BC.full_fwd(B, A)
    a, b = torch.from_numpy(A).to(DEV).requires_grad_(), torch.from_numpy(B).to(DEV).requires_grad_()
    H = hausdorff_matrix(a, b)
    assert np.array_equal(bits(H), np.sqrt(np.maximum(ref_ab["max_sq"], ref_ba["max_sq"].T)).view(np.int32))
    Gd = np.random.default_rng(9).standard_normal((2, 65537)).astype(np.float32)
    for form, key, c in (("squared", "mean_sq", 4), ("sqrt", "mean_rt", 8)):
        a.grad = b.grad = None
        D = ChamferMatrix(form)(a, b)
        ok, ratio = BC.mean_ok(D.detach().cpu().numpy(), (ref_ab[key] + ref_ba[key].T) / 2, 2, 3)
        assert ok, ratio
        (D * torch.from_numpy(Gd).to(DEV)).sum().backward()
        sA, qB = BC.full_bwd(A, B, FORMS[form], Gd / 2)
        sB, qA = BC.full_bwd(B, A, FORMS[form], (Gd / 2).T)
        for got, ref in ((a.grad, sA + qA), (b.grad, qB + sB)):
            ok, ratio = BC.grad_ok(got.cpu().numpy(), ref, c)
            assert ok, (form, ratio)


def test_queries_per_thread_change_no_bit(lib):
    """the query route with 4, 2 and 1 queries per thread (512, 300 and 100 query clouds of 1024 points; counts that leave waves with
    4, 3, 2 and 1 live queries): the run of 4 meets the float64 oracle on both routes, and a query cloud's gradient has the same bits
    whatever the launch kept per thread"""
    S, Q, cS, cQ = BC.make_queries()
    W = np.random.default_rng(21).standard_normal((len(cS), len(cQ))).astype(np.float32)
    for form, c in ((0, 4), (1, 8)):
        runs = {C: entry_bwd(lib, S, cS, Q[:C], cQ[:C], form, W[:, :C]) for C in BC.QUERIES_SUBSETS}
        refS, refQ = BC.directed_bwd(S, cS, Q, cQ, form, W)
        for got, ref in zip(runs[512], (refS, refQ)):
            ok, ratio = BC.grad_ok(got.numpy(), ref, c)
            print("form", form, "worst error / bar", ratio)
            assert ok, ratio
        assert_padding_is_plus_zero(runs[512][1], cQ)
        for C in BC.QUERIES_SUBSETS[1:]:
            assert torch.equal(runs[C][1].view(torch.int32), runs[512][1][:C].contiguous().view(torch.int32)), C


def test_more_clouds_than_workgroups(lib):
    """2^20 + 3 one-point clouds against one: the forward, the surface route (that many surface clouds) and the query route (that many
    query clouds) stride over their units; gradient to the large set only, which needs exactly those two routes"""
    from dpdist_amd import ChamferMatrix, hausdorff_matrix
    A, B = BC.draw(*BC.STRIDE)
    ref_ab, ref_ba = BC.full_fwd(A, B), BC.full_fwd(B, A)
    a, b = torch.from_numpy(A).to(DEV).requires_grad_(), torch.from_numpy(B).to(DEV)
    assert np.array_equal(bits(hausdorff_matrix(a, b)), np.sqrt(np.maximum(ref_ab["max_sq"], ref_ba["max_sq"].T)).view(np.int32))
    Gd = np.random.default_rng(10).standard_normal((len(A), 1)).astype(np.float32)
    D = ChamferMatrix("squared")(a, b)
    ok, ratio = BC.mean_ok(D.detach().cpu().numpy(), (ref_ab["mean_sq"] + ref_ba["mean_sq"].T) / 2, 1, 3)
    assert ok, ratio
    (D * torch.from_numpy(Gd).to(DEV)).sum().backward()
    sA, _ = BC.full_bwd(A, B, 0, Gd / 2)
    _, qA = BC.full_bwd(B, A, 0, (Gd / 2).T)
    ok, ratio = BC.grad_ok(a.grad.cpu().numpy(), sA + qA, 4)
    assert ok, ratio


@pytest.mark.parametrize("form", [0, 1])
def test_backward_at_both_caps(lib, form):
    """Ns = Nq = 4096: the surface route's 64 KB of dynamic LDS (cloud and argmins) under 1024 threads, without an opt-in"""
    A, B = BC.draw(*BC.CAPS)
    W = np.array([[1.5]], np.float32)
    dS, dQ = entry_bwd(lib, A, [4096], B, [4096], form, W)
    refS, refQ = BC.directed_bwd(A, [4096], B, [4096], form, W)
    for got, ref in ((dS, refS), (dQ, refQ)):
        ok, ratio = BC.grad_ok(got.numpy(), ref, 8 if form else 4)
        assert ok, ratio


def test_a_set_against_itself(lib):
    """cloudsB = None runs one direction: the matrices are bit for bit those of the explicit call on (A, A); the gradient, which sums the
    two upstreams before the one backward, meets the oracle of the explicit call"""
    from dpdist_amd import ChamferMatrix, chamfer_matrix, hausdorff_matrix
    S = BC.make_self()
    counts = [40, 40, 17, 1]
    s, sc = dev_set(S, counts)
    for form in ("squared", "sqrt"):
        one, two = chamfer_matrix(s, None, form, True, countsA=sc), chamfer_matrix(s, s, form, True, countsA=sc, countsB=sc)
        for x, y in zip(one, two):
            assert np.array_equal(bits(x), bits(y))
        assert not bits(one[0]).reshape(4, 4).diagonal().any()          # a cloud against itself: exactly +0.0
    for x, y in zip(hausdorff_matrix(s, None, True, countsA=sc), hausdorff_matrix(s, s, True, countsA=sc, countsB=sc)):
        assert np.array_equal(bits(x), bits(y))
    ups = _upstreams(4, 4, "all", seed=23)
    for form, c in (("squared", 4), ("sqrt", 8)):
        s_ = s.clone().requires_grad_()
        outs = ChamferMatrix(form)(s_, None, True, countsA=sc)
        sum((o * torch.from_numpy(g).to(DEV)).sum() for o, g in zip(outs, ups)).backward()
        refA, refB = BC.matrix_bwd(S, counts, S, counts, FORMS[form], *ups)
        ok, ratio = BC.grad_ok(s_.grad.cpu().numpy(), refA + refB, c)
        assert ok, (form, ratio)
        assert_padding_is_plus_zero(s_.grad.cpu(), counts)


def test_against_the_paired_losses(lib):
    """the seed-0 case against the project's paired Chamfer losses: D[i,j] within twice the mean bar (both sides round), the gradients
    under G = 1 / (Ca Cb) against the paired losses' autograd summed over the pairs at the gradient bar with c doubled"""
    from dpdist_amd import ChamferMatrix, aue, regtest
    A, B, cA, cB, ref_ab, ref_ba = case("full")
    Ca, Cb = len(cA), len(cB)
    for form, paired, key, c in (("squared", aue.chamfer_dist, "mean_sq", 4), ("sqrt", regtest.chamfer_sqrt, "mean_rt", 8)):
        a, b = torch.from_numpy(A).to(DEV).requires_grad_(), torch.from_numpy(B).to(DEV).requires_grad_()
        D = ChamferMatrix(form)(a, b)
        (D.sum() / (Ca * Cb)).backward()
        gA, gB = a.grad.clone(), b.grad.clone()
        a.grad = b.grad = None
        ref = (ref_ab[key] + ref_ba[key].T) / 2
        total = 0
        for i in range(Ca):
            for j in range(Cb):
                d = paired(a[i:i + 1], b[j:j + 1])
                assert abs(float(d.detach()) - float(D[i, j].detach())) <= 2 * (64 + 3) * BC.U * ref[i, j], (form, i, j)
                total = total + d / (Ca * Cb)
        total.backward()
        oracle = BC.matrix_bwd(A, cA, B, cB, FORMS[form], np.full((Ca, Cb), 1.0 / (Ca * Cb)))
        for got, other, orc in ((gA, a.grad, oracle[0]), (gB, b.grad, oracle[1])):
            bar = (orc.T + 2 * c) * BC.U * orc.S
            err = np.abs(got.cpu().numpy().astype(np.float64) - other.cpu().numpy().astype(np.float64))
            assert (err <= bar).all(), (form, float((err / np.where(bar > 0, bar, 1)).max()))

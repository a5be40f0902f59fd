"""Paired DPDist for clouds of different sizes on the GPU (tests/pairs_cases.py): the counted window gather bit for bit the plain gather
on each cloud alone, the output layer with its per-pair reduction against the existing output layer and float64, the backward tail against
float64, and dpdist_pairs / DPDistPairs / DPDistLoss against the float64 oracle composed per pair on the truncated clouds.  Bars and
checkers are those of tests/ragged_cases.py, tests/test_cross_gpu.py and tests/test_cross_grad_gpu.py; every output of a new entry sits in
a NaN-payload guard band and input padding holds the NaN payload.
"""
import numpy as np
import pytest
import torch

from dpdist_amd import synth
from tests import gemm_cases as G
from tests import pairs_cases as PC
from tests import ragged_cases as RC
from tests import test_cross_gpu as X
from tests import test_cross_grad_gpu as XG

pytestmark = pytest.mark.gpu

M_GRID, K_WIN, H_DEC, KP, NG, E = PC.M_GRID, PC.K_WIN, PC.H_DEC, PC.KP, PC.NG, PC.E
U24 = PC.U24
_bits = X._bits


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible")
    from dpdist_amd import lib
    lib.load()
    return torch.device("cuda:0")


def _counts_dev(counts, dev):
    return None if counts is None else torch.tensor(counts, dtype=torch.int32, device=dev)


_SID = lambda s: "P%d-Wa%d-Wb%d" % s[:3]      # noqa: E731


# ------------------------------------------------------------------------------------------------------------ the counted gather
def _gather_counts(dev, q, counts, fv, C, N):
    """dpd_patch_rows_fwd_counts into guard-banded buffers -> (rc, X [C N, KP], mask, vox, band check)"""
    from dpdist_amd import lib as L
    Xo, b0 = G.banded((C * N, KP), KP, dtype=torch.float32, device=dev)
    mask, b1 = G.banded_flat(C * N, dtype=torch.float32, device=dev)
    vox, b2 = G.banded_flat(C * N, dtype=torch.int32, device=dev)
    rc = L.load().dpd_patch_rows_fwd_counts(L.ptr(q), L.ptr(counts), L.ptr(fv), C, N, M_GRID, K_WIN, KP, L.ptr(Xo), L.ptr(mask), L.ptr(vox),
                                            L.cur_stream())
    torch.cuda.synchronize()

    def bands():
        for b in (b0, b1, b2):
            b()
    return rc, Xo, mask, vox, bands


@pytest.mark.parametrize("kind", ["random", "outside"])
def test_counted_gather_is_the_plain_gather_on_each_cloud_alone(dev, kind):
    """real rows: the bits of dpd_patch_rows_fwd on the cloud alone ([1, n, 3]); padded rows: KP zeros, mask 0, voxel 0, by bits, and the
    padded queries hold the NaN payload (never read).  Counts (N, 1, N - 1); the out-of-range counts (0, N + 5) behave as (1, N).  A
    refusal writes nothing."""
    from dpdist_amd import lib as L
    lib, s = L.load(), L.cur_stream()
    C, N = 3, 64
    q_full = torch.tensor(X._queries(kind, C, N), device=dev)
    fv = torch.tensor(X._fv(C), device=dev)
    rc, Xo, mask, vox, bands = _gather_counts(dev, q_full, None, fv, C, N)
    assert rc == -1 and G.untouched(Xo) and G.untouched(mask) and bool((vox == G.NAN_OUT).all())
    bands()

    def nan_padded(counts):
        q = q_full.clone()
        for c, n in enumerate(counts):
            q.view(torch.int32)[c, n:] = G.NAN_OUT
        return q

    counts = (N, 1, N - 1)
    rc, Xo, mask, vox, bands = _gather_counts(dev, nan_padded(counts), _counts_dev(counts, dev), fv, C, N)
    assert rc == 0
    Xo, mask, vox = Xo.view(C, N, KP), mask.view(C, N), vox.view(C, N)
    for c, n in enumerate(counts):
        Xa, ma = torch.empty(n, KP, device=dev), torch.empty(n, device=dev)
        va = torch.empty(n, device=dev, dtype=torch.int32)
        L.check(lib.dpd_patch_rows_fwd(L.ptr(q_full[c:c + 1, :n].contiguous()), L.ptr(fv[c:c + 1]), 1, n, M_GRID, K_WIN, KP, L.ptr(Xa), L.ptr(ma),
                                       L.ptr(va), None, s), "dpd_patch_rows_fwd")
        torch.cuda.synchronize()
        assert torch.equal(_bits(Xo[c, :n]), _bits(Xa)) and torch.equal(_bits(mask[c, :n]), _bits(ma)) and torch.equal(vox[c, :n], va), (c, n)
        assert not _bits(Xo[c, n:]).any() and not _bits(mask[c, n:]).any() and not vox[c, n:].any(), (c, n)
    assert float(Xo[0].abs().max()) > 0
    if kind == "outside":
        assert int((mask[0] == 0).sum()) == 4 and int((mask[1, :1] == 0).sum()) == 1        # real queries outside the cube: mask 0, still real rows
    bands()
    clamped, as_if = (0, N + 5, N - 1), (1, N, N - 1)
    rc1, X1, m1, v1, bands1 = _gather_counts(dev, nan_padded(as_if), _counts_dev(clamped, dev), fv, C, N)
    rc2, X2, m2, v2, _ = _gather_counts(dev, nan_padded(as_if), _counts_dev(as_if, dev), fv, C, N)
    assert rc1 == 0 and rc2 == 0
    assert torch.equal(_bits(X1), _bits(X2)) and torch.equal(_bits(m1), _bits(m2)) and torch.equal(v1, v2)
    bands1()


# ------------------------------------------------------------------------------------------------------------ the output layer
class _Out:
    """one chunk's h3 from dpd_decoder_fwd on random rows (which also gives the existing output layer's y and pred), then
    dpd_decoder_out_pairs on that h3 into guard-banded buffers"""

    def __init__(self, dev, shape):
        from dpdist_amd import lib as L
        self.lib, self.s = lib, s = L.load(), L.cur_stream()
        P, Wa, Wb, cA, cB = shape
        self.shape, self.Q = shape, P * (Wa + Wb)
        Q, H = self.Q, H_DEC
        self.segs = PC.seg_rows(P, Wa, Wb, cA, cB)
        rng = np.random.default_rng([31, P, Wa, Wb])
        self.tens, self.cp = X._decoder_weights(dev, H, False)
        rows = torch.tensor((rng.standard_normal((Q, KP)) * 0.3).astype(np.float32), device=dev)
        mask = (rng.uniform(size=Q) < 0.8).astype(np.float32)
        self.real = np.zeros(Q, bool)
        self.cnt = np.ones(Q)
        for _, _, r0, W, n in self.segs:
            mask[r0 + n:r0 + W] = 0.0                                   # what the counted gather writes for a padded query
            self.real[r0:r0 + n] = True
            self.cnt[r0:r0 + W] = n
        self.mask = torch.tensor(mask, device=dev)
        f = lambda *sh: torch.empty(*sh, device=dev)   # noqa: E731
        h1, h2, self.h3, self.y_ref, self.pred_ref = f(Q, H), f(Q, H), f(Q, H), f(Q, 3), f(Q, 3)
        L.check(lib.dpd_decoder_fwd(L.ptr(rows), L.ptr(self.mask), Q, KP, H, self.cp, 0, L.ptr(h1), L.ptr(h2), L.ptr(self.h3), L.ptr(self.y_ref),
                                    L.ptr(self.pred_ref), None, 0, None, s), "dpd_decoder_fwd")
        self.cA, self.cB = _counts_dev(cA, dev), _counts_dev(cB, dev)
        self.dev = dev

    def run(self, backward=True, P=None, h3=None):
        from dpdist_amd import lib as L
        Pn, Wa, Wb, _, _ = self.shape
        Q, H = self.Q, H_DEC
        f32 = dict(dtype=torch.float32, device=self.dev)
        bufs, bands = {}, []
        for name, cols in (("y", 3), ("pred", 3), ("dy", 3), ("g3", H)):
            bufs[name], b = G.banded((Q, cols), cols, **f32)
            bands.append(b)
        bufs["Dd"], b = G.banded_flat(2 * Pn, **f32)
        bands.append(b)
        rc = self.lib.dpd_decoder_out_pairs(L.ptr(self.h3 if h3 is None else h3), L.ptr(self.mask), Pn if P is None else P, Wa, Wb, L.ptr(self.cA),
                                            L.ptr(self.cB), H, self.cp, L.ptr(bufs["y"]), L.ptr(bufs["pred"]), L.ptr(bufs["Dd"]),
                                            L.ptr(bufs["dy"]) if backward else None, L.ptr(bufs["g3"]) if backward is True else None, self.s)
        torch.cuda.synchronize()

        def check():
            for b in bands:
                b()
        return rc, bufs, check


@pytest.mark.parametrize("shape", PC.ENTRY_SHAPES, ids=_SID)
def test_output_layer_of_the_pairs(dev, shape):
    """y, pred: the bits of dpd_decoder_fwd's output layer on the same h3.  Dd [2, P]: within 12 * 2^-24 * 2 of the float64 mean of the
    GPU's own pred[:, 0] over each segment's real rows; twice the same bits; the same bits without the backward.  dy, g3 against float64
    from the same h3: the counted upstream spread of tests/test_ragged_gpu.py is ONE fp32 division and is held exactly; here the reference
    also holds the / 3 of relu6 / 3 (dy: three roundings) and the product with W4[:, 0] (g3: four), so the bars are 3 and 4 units of
    2^-24 relative, element by element (rows whose float64 y0 lies within 1e-5 of a relu6 corner are left out of that comparison).  The
    rows of padded queries are +0.0 by bits in dy and g3.  A refusal writes nothing."""
    o = _Out(dev, shape)
    P, Wa, Wb, cA, cB = shape
    Q, H = o.Q, H_DEC
    for kw in (dict(backward="dy only"), dict(P=0)):                    # dy without g3: DPD_E_NULL; no pairs: DPD_E_DIM
        rc, bufs, check = o.run(**kw)
        assert rc in (-1, -2) and all(G.untouched(t) for t in bufs.values())
        check()
    rc, bufs, check = o.run()
    assert rc == 0
    assert torch.equal(_bits(bufs["y"]), _bits(o.y_ref)) and torch.equal(_bits(bufs["pred"]), _bits(o.pred_ref))
    pred = bufs["pred"][:, 0].double().cpu().numpy()
    assert pred.min() >= 0 and pred.max() <= 2 and (pred.max() > 0 or P == 1)
    Dd = bufs["Dd"].double().cpu().numpy()
    for d, b, r0, W, n in o.segs:
        want = pred[r0:r0 + n].sum() / n
        err = abs(Dd[d * P + b] - want)
        print("Dd[%d, %d] (%d of %d rows): %.7f, %.2e from the float64 mean (bar %.2e)" % (d, b, n, W, want, err, PC.DD_BAR))
        assert err <= PC.DD_BAR
    check()
    rc2, again, check2 = o.run()
    rc3, fwd, check3 = o.run(backward=False)
    assert rc2 == 0 and rc3 == 0
    for name in ("y", "pred", "Dd", "dy", "g3"):
        assert torch.equal(_bits(again[name]), _bits(bufs[name])), name
    for name in ("y", "pred", "Dd"):
        assert torch.equal(_bits(fwd[name]), _bits(bufs[name])), name
    assert G.untouched(fwd["dy"]) and G.untouched(fwd["g3"])
    check2(), check3()
    # the output-layer backward of sum_b (D_AB[b] + D_BA[b]) in float64 from the same h3
    W4, b4 = o.tens[6].double().cpu().numpy(), o.tens[7].double().cpu().numpy()
    h3 = o.h3.double().cpu().numpy()
    y0 = h3 @ W4[:, 0] + b4[0]
    near = (np.abs(y0) < 1e-5) | (np.abs(y0 - 6.0) < 1e-5)
    assert near.sum() <= Q // 50
    gate = (y0 > 0) & (y0 < 6) & o.real
    dy_ref = gate * o.mask.double().cpu().numpy() / (3.0 * o.cnt)
    g3_ref = dy_ref[:, None] * W4[None, :, 0] * (h3 > 0)
    dy, g3 = bufs["dy"].double().cpu().numpy(), bufs["g3"].double().cpu().numpy()
    keep = ~near
    assert (dy_ref[keep] > 0).sum() >= Q // 8                       # open rows exist (none is asked of the two rows of the smallest shape)
    assert not dy[:, 1:].any()
    e_dy, e_g3 = np.abs(dy[keep, 0] - dy_ref[keep]), np.abs(g3[keep] - g3_ref[keep])
    print("dy: %.2e, g3: %.2e from float64 (largest |ref| %.2e, %.2e)" % (e_dy.max(), e_g3.max(), np.abs(dy_ref).max(), np.abs(g3_ref).max()))
    assert (e_dy <= 3 * U24 * np.abs(dy_ref[keep])).all() and (e_g3 <= 4 * U24 * np.abs(g3_ref[keep])).all()
    pad = torch.tensor(~o.real, device=dev)
    assert not _bits(bufs["dy"][pad]).any() and not _bits(bufs["g3"][pad]).any()
    if cA is not None:
        assert int(pad.sum()) == sum(W - n for _, _, _, W, n in o.segs) > 0


# ------------------------------------------------------------------------------------------------------------ the backward tail
@pytest.mark.parametrize("shape", PC.ENTRY_SHAPES, ids=_SID)
def test_combine_against_float64(dev, shape):
    """gA = G_ab dptsA + G_ba dq_BA, gB = G_ba dptsB + G_ab dq_AB on random operands against float64: two products and one sum in fp32,
    2 * 2^-24 (|first product| + |second product|) per element.  Rows at or beyond a cloud's count are +0.0 by bits; what lies there in
    dpts and dX holds the NaN payload.  One set alone: the same bits, the other output untouched."""
    from dpdist_amd import lib as L
    lib, s = L.load(), L.cur_stream()
    P, Wa, Wb, cA, cB = shape
    Q = P * (Wa + Wb)
    rng = np.random.default_rng([41, P, Wa, Wb])
    mk = lambda *sh: torch.tensor(rng.standard_normal(sh).astype(np.float32), device=dev)   # noqa: E731
    dA, dB, dX, g_ab, g_ba = mk(P, Wa, 3), mk(P, Wb, 3), mk(Q, KP), mk(P), mk(P)
    nA, nB = cA or (Wa,) * P, cB or (Wb,) * P
    for b in range(P):
        dA.view(torch.int32)[b, nA[b]:] = G.NAN_OUT
        dB.view(torch.int32)[b, nB[b]:] = G.NAN_OUT
    for _, _, r0, W, n in PC.seg_rows(P, Wa, Wb, cA, cB):
        dX.view(torch.int32)[r0 + n:r0 + W] = G.NAN_OUT
    cAd, cBd = _counts_dev(cA, dev), _counts_dev(cB, dev)

    def run(wantA=True, wantB=True, P_=P):
        gA, ba = G.banded_flat(P * Wa * 3, dtype=torch.float32, device=dev)
        gB, bb = G.banded_flat(P * Wb * 3, dtype=torch.float32, device=dev)
        rc = lib.dpd_pairs_combine(L.ptr(dA) if wantA else None, L.ptr(dB) if wantB else None, L.ptr(dX), L.ptr(g_ab), L.ptr(g_ba), P_, Wa, Wb,
                                   L.ptr(cAd), L.ptr(cBd), K_WIN, KP, L.ptr(gA) if wantA else None, L.ptr(gB) if wantB else None, s)
        torch.cuda.synchronize()
        ba(), bb()
        return rc, gA.view(P, Wa, 3), gB.view(P, Wb, 3)

    rc, gA, gB = run(P_=0)
    assert rc == -2 and G.untouched(gA) and G.untouched(gB)
    rc, gA, gB = run(False, False)
    assert rc == -1
    rc, gA, gB = run()
    assert rc == 0
    dq = dX[:, E:E + 3].double().cpu().numpy()
    dq_ab, dq_ba = dq[:P * Wb].reshape(P, Wb, 3), dq[P * Wb:].reshape(P, Wa, 3)
    a64, b64 = g_ab.double().cpu().numpy()[:, None, None], g_ba.double().cpu().numpy()[:, None, None]
    for name, got, t1, t2, counts in (("gA", gA, a64 * dA.double().cpu().numpy(), b64 * dq_ba, nA),
                                      ("gB", gB, b64 * dB.double().cpu().numpy(), a64 * dq_ab, nB)):
        got64 = got.double().cpu().numpy()
        for b in range(P):
            n = counts[b]
            err = np.abs(got64[b, :n] - (t1[b, :n] + t2[b, :n]))
            assert (err <= 2 * U24 * (np.abs(t1[b, :n]) + np.abs(t2[b, :n]))).all(), (name, b, err.max())
            assert not _bits(got[b, n:]).any(), (name, b)
        assert float(got.abs().max()) > 0
    rcA, oA, uB = run(wantB=False)
    rcB, uA, oB = run(wantA=False)
    assert rcA == 0 and rcB == 0 and torch.equal(_bits(oA), _bits(gA)) and torch.equal(_bits(oB), _bits(gB))
    assert G.untouched(uA) and G.untouched(uB)


# ------------------------------------------------------------------------------------------------------------ the public interface
def _cu(t, dev, grad=False):
    return torch.tensor(np.ascontiguousarray(t), device=dev).requires_grad_(grad)


def _run(dev, pad=None, max_rows=16384, needA=True, needB=True, pairs=slice(None), case="reference", device_counts=False):
    """DPDistPairs on a case of tests/pairs_cases.py (the padding set to `pad`; `pairs`: a slice of the batch, with the same padded widths
    and its own counts) -> (outputs, gradients of the loss of pairs_cases w.r.t. the sets that ask)"""
    from dpdist_amd import DPDistPairs
    A, B, cA, cB = PC._case(case)
    if pad is not None:
        A, B = RC.with_padding(A, cA, pad), RC.with_padding(B, cB, pad)
    a, b = _cu(A[pairs], dev, needA), _cu(B[pairs], dev, needB)
    kw = {}
    if case == "reference":
        kw = dict(countsA=_counts_dev(cA[pairs], dev) if device_counts else list(cA[pairs]), countsB=torch.tensor(cB[pairs]))
    out = DPDistPairs(X._params(dev), max_rows=max_rows)(a, b, return_directed=True, **kw)
    Gs = tuple(g[pairs] for g in PC.upstream(A.shape[0]))
    loss = XG._loss(out, Gs, True, dev)
    return out, list(torch.autograd.grad(loss, [t for t, need in ((a, needA), (b, needB)) if need]))


def _same(xs, ys):
    return all(torch.equal(_bits(x.detach()), _bits(y.detach())) for x, y in zip(xs, ys)) and len(xs) == len(ys)


def test_pairs_against_the_composed_oracle(dev):
    """D, D_AB, D_BA of dpdist_pairs on the reference case within 1e-4 absolute of the float64 oracle composed per pair on the truncated
    clouds; counts as a list, a CPU tensor and a device tensor are the same call; DPDistPairs gives the same bits"""
    from dpdist_amd import dpdist_pairs
    A, B = PC.sets()
    P = X._params(dev)
    got = dpdist_pairs(P, _cu(A, dev), _cu(B, dev), countsA=PC.COUNTS_A, countsB=list(PC.COUNTS_B), return_directed=True)
    Do = PC.case_oracle("reference", torch.float64)
    for name, g, want in zip(("D", "D_AB", "D_BA"), got, Do):
        err = float(np.abs(g.double().cpu().numpy() - want).max())
        print("%s %s vs the composed float64 oracle: %.3e" % (name, np.round(want, 4), err))
        assert g.shape == (3,) and err <= PC.FWD_BAR, name
    assert torch.equal(_bits(dpdist_pairs(P, _cu(A, dev), _cu(B, dev), PC.COUNTS_A, PC.COUNTS_B)), _bits(got[0]))
    cpu = dpdist_pairs(P, _cu(A, dev), _cu(B, dev), torch.tensor(PC.COUNTS_A), torch.tensor(PC.COUNTS_B, dtype=torch.int64), True)
    on_dev = dpdist_pairs(P, _cu(A, dev), _cu(B, dev), _counts_dev(PC.COUNTS_A, dev), _counts_dev(PC.COUNTS_B, dev), True)
    assert _same(cpu, got) and _same(on_dev, got)
    out, _ = _run(dev, device_counts=True)
    assert _same(out, got)


def test_gradients_against_the_composed_oracle(dev):
    """gradients of (G D).sum() + (G_AB D_AB).sum() + (G_BA D_BA).sum() against float64 autograd through the same composition, at the
    project's input-gradient bar; the gradients at padded points are +0.0 by bits"""
    _, (gA, gB) = _run(dev)
    for name, got, (ref, bar), counts in zip(("gA", "gB"), (gA, gB), PC.grad_bars("reference"), (PC.COUNTS_A, PC.COUNTS_B)):
        err = np.abs(got.double().cpu().numpy() - ref).max()
        print("%s vs the composed float64 oracle: %.3e (bar %.3e, max|ref| %.3e)" % (name, err, bar, np.abs(ref).max()))
        assert np.abs(ref).max() > 20 * bar, "a reference gradient without structure makes the bar vacuous"
        assert got.shape == ref.shape and err <= bar, name
        for c, n in enumerate(counts):
            assert not _bits(got[c, n:]).any(), (name, c)
            assert float(got[c, :n].abs().max()) > 0, (name, c)


def test_the_padding_changes_no_bit(dev):
    ref_out, ref_g = _run(dev, pad=0.0)
    for pad in (0.37, 5.0):
        out, g = _run(dev, pad=pad)
        assert _same(list(out) + g, list(ref_out) + ref_g), pad


def test_chunking_changes_no_bit(dev):
    one_out, one_g = _run(dev, max_rows=1 << 20)
    per_out, per_g = _run(dev, max_rows=1)                          # every chunk holds one pair
    assert _same(list(one_out) + one_g, list(per_out) + per_g)
    two_out, two_g = _run(dev, max_rows=208)                        # two pairs, then one
    assert _same(list(one_out) + one_g, list(two_out) + two_g)
    assert all(float(g.abs().max()) > 0 for g in one_g)


def test_a_pair_does_not_depend_on_the_rest_of_the_batch(dev):
    """pair b of the batch is bit for bit the call on that pair alone, with the same padded widths and its own counts"""
    out, (gA, gB) = _run(dev)
    for b in range(3):
        o1, (a1, b1) = _run(dev, pairs=slice(b, b + 1))
        assert _same([t[b:b + 1] for t in out], o1), b
        assert torch.equal(_bits(gA[b:b + 1]), _bits(a1)) and torch.equal(_bits(gB[b:b + 1]), _bits(b1)), b


def test_rectangular_sets_without_counts(dev):
    """A [2, 64, 3] against B [2, 24, 3], no counts: within 1e-4 of the oracle; DPDistPairs gives gradients of the two shapes"""
    from dpdist_amd import dpdist_pairs
    A, B = PC.rect_sets()
    got = dpdist_pairs(X._params(dev), _cu(A, dev), _cu(B, dev), return_directed=True)
    for name, g, want in zip(("D", "D_AB", "D_BA"), got, PC.case_oracle("rect", torch.float64)):
        err = float(np.abs(g.double().cpu().numpy() - want).max())
        print("rectangular %s %s vs the float64 oracle: %.3e" % (name, np.round(want, 4), err))
        assert g.shape == (2,) and err <= PC.FWD_BAR, name
    out, (gA, gB) = _run(dev, case="rect")
    assert _same(out, got) and gA.shape == (2, 64, 3) and gB.shape == (2, 24, 3)
    assert bool(torch.isfinite(gA).all()) and bool(torch.isfinite(gB).all()) and float(gA.abs().max()) > 0 and float(gB.abs().max()) > 0


def test_only_one_set_counted(dev):
    """countsA alone: B is full (all 40 points of every cloud), against the oracle on those clouds"""
    from dpdist_amd import dpdist_pairs
    A, B = PC.sets()
    got = dpdist_pairs(X._params(dev), _cu(A, dev), _cu(B, dev), countsA=PC.COUNTS_A, return_directed=True)
    want = PC.oracle(A, B, PC.COUNTS_A, PC.full(B), torch.float64)
    for name, g, w in zip(("D", "D_AB", "D_BA"), got, want):
        err = float(np.abs(g.double().cpu().numpy() - w).max())
        print("countsA alone, %s vs the float64 oracle: %.3e" % (name, err))
        assert err <= PC.FWD_BAR, name
    ref = PC.case_oracle("reference", torch.float64)
    assert np.abs(want[1] - ref[1]).max() > 0.01                     # not the reference case again


def test_partial_gradients(dev):
    """one set without requires_grad gets None; the other keeps its bits"""
    from dpdist_amd import DPDistPairs
    _, (gA, gB) = _run(dev)
    _, (oA,) = _run(dev, needB=False)
    _, (oB,) = _run(dev, needA=False)
    assert torch.equal(_bits(oA), _bits(gA)) and torch.equal(_bits(oB), _bits(gB))
    A, B = PC.sets()
    a, b = _cu(A, dev, True), _cu(B, dev)
    DPDistPairs(X._params(dev))(a, b, countsA=PC.COUNTS_A, countsB=PC.COUNTS_B).sum().backward()
    assert a.grad is not None and b.grad is None


@pytest.mark.parametrize("case", PC.LARGE, ids=lambda c: "Wa%d-Wb%d" % c)
def test_sizes_beyond_the_plain_encoder(dev, case):
    """one pair at Wa = 712 (the forward of the encoder runs over tiles of points) and at Wa = 1640 (its backward too): forward within
    1e-4 and gradients within the bar form of the float64 oracle"""
    from dpdist_amd import ops
    assert ops.encoder_tiled(case[0], M_GRID, ops.FITS_FWD if case[0] == 712 else ops.FITS_BWD_SLICED)
    out, grads = _run(dev, case=case)
    for name, g, want in zip(("D", "D_AB", "D_BA"), out, PC.case_oracle(case, torch.float64)):
        err = float(np.abs(g.detach().double().cpu().numpy() - want).max())
        print("%s %s %s vs the float64 oracle: %.3e" % (case, name, want, err))
        assert err <= PC.FWD_BAR, name
    for name, got, (ref, bar) in zip(("gA", "gB"), grads, PC.grad_bars(case)):
        err = np.abs(got.double().cpu().numpy() - ref).max()
        print("%s %s vs the float64 oracle: %.3e (bar %.3e, max|ref| %.3e)" % (case, name, err, bar, np.abs(ref).max()))
        assert np.abs(ref).max() > 20 * bar and got.shape == ref.shape and err <= bar, name


# ------------------------------------------------------------------------------------------------------------ DPDistLoss and the AUE task
def _model(dev):
    from dpdist_amd.model import DPDistModel
    mod = DPDistModel(Embedding_Size=512, k=K_WIN, localSNmlp=(H_DEC,) * 3, sigma3dmfv=0.125, device=dev)
    mod.load_tf_state_dict(synth.make_weights("wide", mlp=(H_DEC,) * 3))
    return mod


def test_loss_of_equal_shapes_is_the_as_loss_node(dev):
    """two full tensors of one shape, no counts: value and gradients are bit for bit those of _AsLossFn.apply called directly"""
    from dpdist_amd import DPDistLoss
    from dpdist_amd.model import _AsLossFn
    mod = _model(dev)
    loss = DPDistLoss(mod)
    A, B = X._sets(X.SHAPES[0])                                     # [3, 64, 3], [2, 64, 3]
    a, b = _cu(A[:2], dev, True), _cu(B, dev, True)
    got = loss(a, b)
    g = torch.autograd.grad(got, [a, b])
    a2, b2 = _cu(A[:2], dev, True), _cu(B, dev, True)
    want = _AsLossFn.apply(a2, b2, mod.params_.flat, mod.params_, M_GRID, K_WIN, 0.125)
    w = torch.autograd.grad(want, [a2, b2])
    assert got.dim() == 0 and _same([got] + list(g), [want] + list(w)) and float(g[0].abs().max()) > 0
    assert DPDistLoss.capturable is True


def test_loss_of_different_sizes_is_the_mean_of_the_pairs(dev):
    """(source [3, 64, 3], template [3, 40, 3], counts) == DPDistPairs(...).mean() by bits, value and gradients; two widths without counts
    take the same route; a bf16 model is refused with dpdist_matrix's message"""
    from dpdist_amd import DPDistLoss, DPDistPairs
    mod = _model(dev)
    loss = DPDistLoss(mod)
    A, B = PC.sets()

    def both(fn):
        a, b = _cu(A, dev, True), _cu(B, dev, True)
        v = fn(a, b)
        return [v] + list(torch.autograd.grad(v, [a, b]))

    got = both(lambda a, b: loss(a, b, PC.COUNTS_A, torch.tensor(PC.COUNTS_B)))
    want = both(lambda a, b: DPDistPairs(mod)(a, b, countsA=PC.COUNTS_A, countsB=PC.COUNTS_B).mean())
    assert got[0].dim() == 0 and _same(got, want)
    Do = PC.case_oracle("reference", torch.float64)[0]
    assert abs(float(got[0].detach()) - Do.mean()) <= PC.FWD_BAR
    assert not _bits(got[1][1, 37:]).any() and not _bits(got[2][1, 1:]).any()
    plain = both(lambda a, b: loss(a, b))                           # two widths, no counts
    assert _same(plain, both(lambda a, b: DPDistPairs(mod)(a, b).mean())) and not torch.equal(plain[0], got[0])
    half = _model(dev)
    half.params_.compute_dtype = "bf16"
    with pytest.raises(ValueError, match="fp32"):
        DPDistLoss(half)(_cu(A, dev), _cu(B, dev))
    with pytest.raises(ValueError, match="fp32"):
        DPDistLoss(half)(_cu(A, dev), _cu(A, dev), counts_source=PC.COUNTS_A)


def test_aue_step_from_256_points_to_64(dev):
    """one AUETask.step with PointNetAE(num_point=64) on 256-point inputs, B = 4: both losses finite, every autoencoder parameter with a
    finite gradient that is non-zero somewhere"""
    from dpdist_amd import DPDistLoss
    from dpdist_amd.aue import AUETask, PointNetAE
    torch.manual_seed(3)
    ae = PointNetAE(num_point=64).to(dev)
    task = AUETask(ae, DPDistLoss(_model(dev)), lr=1e-3, opt_type="ours")
    x1, x2, _ = synth.s2_modelnet_shaped(4, 256, 7)
    loss_p, loss_c = task.step(_cu(x1.astype(np.float32), dev), _cu(x2.astype(np.float32), dev))
    assert bool(torch.isfinite(loss_p)) and bool(torch.isfinite(loss_c)) and float(loss_p) > 0 and float(loss_c) > 0
    for name, p in ae.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, name

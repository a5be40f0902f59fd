"""Differentiable all-pairs DPDist (dpdist_amd.pairwise.DPDistMatrix; dpd_cross_invert, dpd_decoder_fwd_cross_keep, dpd_cross_slot_sum,
dpd_cross_scatter, dpd_cross_bwd).

The forward is a bit-for-bit statement against dpdist_matrix.  The backward's pieces are pinned one by one: the inverted index against
numpy, the slot sum and the query route against float64 (exact on integer operands, an addend bound on normal ones), the window scatter
against the library's own gather backward on the hand-tiled pairs, the gradients against the float64 oracle and against the pair path.
Every output of a new entry sits in a NaN-filled guard-banded buffer (tests/gemm_cases.py).  Shapes, query kinds, clouds and weights are
those of tests/test_cross_gpu.py.
"""
import functools

import numpy as np
import pytest
import torch

from dpdist_amd import synth
from tests import gemm_cases as G
from tests import test_cross_gpu as X

pytestmark = pytest.mark.gpu

M_GRID, K_WIN, H_DEC, KP, NG = X.M_GRID, X.K_WIN, X.H_DEC, X.KP, X.NG
E = K_WIN ** 3 * 20
SHAPES, KINDS = X.SHAPES, X.KINDS
U24 = 2.0 ** -24


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible")
    from dpdist_amd import lib
    lib.load()
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int32)


def gamma(n):
    """the worst case of an fp32 sum of n addends in any order, relative to the sum of their magnitudes: (n - 1) u / (1 - (n - 1) u)"""
    n = np.maximum(np.asarray(n, dtype=np.float64) - 1.0, 0.0)
    return n * U24 / (1.0 - n * U24)


# ---------------------------------------------------------------------------------------------------------------- the inverted index
class _Inv:
    """dpd_cross_invert on the index of a shared gather (tests/test_cross_gpu.py: _cross), into guard-banded buffers"""

    def __init__(self, x):
        from dpdist_amd import lib as L
        lib, s = L.load(), L.cur_stream()
        dev = x.q.device
        i32 = dict(dtype=torch.int32, device=dev)
        QN = x.Cb * x.N
        self.start, self.start_band = G.banded_flat(NG + 1, **i32)
        self.qlist, self.qlist_band = G.banded_flat(QN, **i32)
        self.svox, self.svox_band = G.banded_flat(NG, **i32)
        L.check(lib.dpd_cross_invert(L.ptr(x.vox), L.ptr(x.slot), L.ptr(x.ucount), x.Cb, x.N, M_GRID, L.ptr(self.start), L.ptr(self.qlist),
                                     L.ptr(self.svox), s), "dpd_cross_invert")
        torch.cuda.synchronize()

    def bands(self):
        for b in (self.start_band, self.qlist_band, self.svox_band):
            b()


@functools.lru_cache(maxsize=None)
def _inv(shape, kind, integer=False):
    return _Inv(X._cross(shape, kind, not integer, integer))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES)
def test_inverted_index(dev, shape, kind):
    """the queries sorted by slot == a stable argsort of the slots; the starts == the prefix of np.bincount; the voxel of every slot"""
    Ca, Cb, N = shape
    x, v = X._cross(shape, kind, True), _inv(shape, kind)
    QN = Cb * N
    vox = x.vox.cpu().numpy().astype(np.int64)
    slots = x.slot.cpu().numpy()[vox]
    assert slots.min() >= 0
    U = x.U
    counts = np.bincount(slots, minlength=U)
    assert len(counts) == U and counts.sum() == QN and counts.min() >= 1
    start = v.start.cpu().numpy()
    assert np.array_equal(start[:U + 1], np.concatenate([[0], np.cumsum(counts)]))
    assert (start[U:] == QN).all()
    assert np.array_equal(v.qlist.cpu().numpy(), np.argsort(slots, kind="stable"))
    svox = v.svox.cpu().numpy()
    assert np.array_equal(svox[:U], np.unique(vox)) and (svox[U:] == -1).all()
    if kind == "one_voxel":
        assert U == 1 and counts[0] == QN
    if kind == "distinct":
        assert U == QN and (counts == 1).all()
    v.bands()
    x.bands()


# -------------------------------------------------------------------------------------------------------- slot sum and query route
def _operands(dev, x, integer, seed, H=H_DEC):
    """g1 [rows_p, H] (pad rows zero, as the decoder's mask leaves them) and W1p [KP, H]; float32 on the device, float64 on the host"""
    rng = np.random.default_rng([seed, x.Ca, x.Cb, x.N, int(integer), H])
    if integer:
        g = G.small_int(rng, (x.rows_p, H), KP).astype(np.float64)
        W = G.small_int(rng, (KP, H), KP).astype(np.float64)
    else:
        g = rng.standard_normal((x.rows_p, H)).astype(np.float32).astype(np.float64)
        W = (rng.standard_normal((KP, H)) * 0.05).astype(np.float32).astype(np.float64)
    g[x.rows:] = 0.0
    return torch.tensor(g, dtype=torch.float32, device=dev), torch.tensor(W, dtype=torch.float32, device=dev), g, W


def _slot_sum(dev, x, v, g_t, W_t, want_gs=True, want_dq=True):
    from dpdist_amd import lib as L
    lib, s = L.load(), L.cur_stream()
    f32 = dict(dtype=torch.float32, device=dev)
    H = g_t.shape[1]
    gs, gs_band = G.banded((x.cap, H), H, **f32)
    dq, dq_band = G.banded((x.rows_p, 3), 3, **f32)
    L.check(lib.dpd_cross_slot_sum(L.ptr(g_t), L.ptr(x.cnt), L.ptr(v.start), L.ptr(v.qlist), L.ptr(W_t), x.Ca, x.Cb, x.N, M_GRID, K_WIN, KP,
                                   H, x.cap, L.ptr(gs) if want_gs else None, L.ptr(dq) if want_dq else None, s), "dpd_cross_slot_sum")
    torch.cuda.synchronize()
    return gs, gs_band, dq, dq_band


@pytest.mark.parametrize("integer", [True, False])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES)
def test_slot_sum_and_query_route_against_float64(dev, shape, kind, integer):
    """gs[i U + s] = the float64 index_add of the g1 rows of (surface i, slot s); dq[r] = the float64 dot products with the three
    q - centre rows of W1p.  Integer operands: equal.  Normal operands: within gamma(n) * sum |addend| per element, n = the length of the
    slot's list (gs) and H (dq, whose addends are the fp32 products).  Dead slots up to the capacity are ZERO rows; the pad
    rows of dq are untouched."""
    Ca, Cb, N = shape
    x, v = X._cross(shape, kind, not integer, integer), _inv(shape, kind, integer)
    g_t, W_t, g, W = _operands(dev, x, integer, 11)
    gs, gs_band, dq, dq_band = _slot_sum(dev, x, v, g_t, W_t)
    U, rows, QN = x.U, x.rows, Cb * N
    uid = x.uid.cpu().numpy()[:rows].astype(np.int64)
    want = np.zeros((Ca * U, H_DEC))
    mag = np.zeros((Ca * U, H_DEC))
    np.add.at(want, uid, g[:rows])
    np.add.at(mag, uid, np.abs(g[:rows]))
    n_seg = np.bincount(uid, minlength=Ca * U)
    got = gs.double().cpu().numpy()
    # the addends of dq are the fp32 products (the kernel multiplies in fp32, no FMA), their sum is compared in float64
    Wq32 = W[E:E + 3].astype(np.float32)
    prod = g[:rows, None, :].astype(np.float32) * Wq32[None]                     # [rows, 3, H] float32
    dq_want = prod.astype(np.float64).sum(-1)
    dq_mag = np.abs(prod.astype(np.float64)).sum(-1)
    dq_got = dq.double().cpu().numpy()
    if integer:
        assert np.array_equal(got[:Ca * U], want), "gs"
        assert np.array_equal(dq_got[:rows], dq_want), "dq"
    else:
        err, bound = np.abs(got[:Ca * U] - want), gamma(n_seg)[:, None] * mag
        print("gs: max error %.3e, max bound %.3e, longest list %d" % (err.max(), bound.max(), n_seg.max()))
        assert (err <= bound).all(), "gs"
        err, bound = np.abs(dq_got[:rows] - dq_want), gamma(H_DEC) * dq_mag
        print("dq: max error %.3e, max bound %.3e" % (err.max(), bound.max()))
        assert (err <= bound).all(), "dq"
    assert not _bits(gs[Ca * U:]).any()                             # dead slots: zero rows
    assert G.untouched(dq[rows:])
    if kind == "one_voxel":
        assert n_seg.max() == QN
    if kind == "distinct":
        assert n_seg.max() == 1 and np.array_equal(got[:Ca * U][uid], g[:rows])       # one addend: the row itself
    if kind == "outside":
        assert n_seg.max() > 1
    gs_band(), dq_band(), v.bands(), x.bands()
    # each half alone: the same bits, the other buffer untouched
    gs2, b2, dq2, c2 = _slot_sum(dev, x, v, g_t, W_t, want_dq=False)
    assert torch.equal(_bits(gs2), _bits(gs)) and G.untouched(dq2)
    gs3, b3, dq3, c3 = _slot_sum(dev, x, v, g_t, W_t, want_gs=False)
    assert torch.equal(_bits(dq3[:rows]), _bits(dq[:rows])) and G.untouched(gs3)
    b2(), c2(), b3(), c3()


@pytest.mark.parametrize("integer", [True, False])
@pytest.mark.parametrize("H", [64, 320, 1024])
def test_slot_sum_at_other_widths(dev, H, integer):
    """the kernel gives one wave to every 256 columns and adds the waves' partial dot products in ascending order: a quarter of a wave
    (64), a whole wave and a quarter (320), four waves (1024) -- the same statements as at the decoder width of the other tests"""
    shape, kind = SHAPES[1], "random"
    Ca, Cb, N = shape
    x, v = X._cross(shape, kind, not integer, integer), _inv(shape, kind, integer)
    g_t, W_t, g, W = _operands(dev, x, integer, 13, H)
    gs, gs_band, dq, dq_band = _slot_sum(dev, x, v, g_t, W_t)
    U, rows = x.U, x.rows
    uid = x.uid.cpu().numpy()[:rows].astype(np.int64)
    want, mag = np.zeros((Ca * U, H)), np.zeros((Ca * U, H))
    np.add.at(want, uid, g[:rows])
    np.add.at(mag, uid, np.abs(g[:rows]))
    prod = g[:rows, None, :].astype(np.float32) * W[E:E + 3].astype(np.float32)[None]
    dq_want, dq_mag = prod.astype(np.float64).sum(-1), np.abs(prod.astype(np.float64)).sum(-1)
    got, dq_got = gs.double().cpu().numpy(), dq.double().cpu().numpy()
    if integer:
        assert np.array_equal(got[:Ca * U], want) and np.array_equal(dq_got[:rows], dq_want)
    else:
        assert (np.abs(got[:Ca * U] - want) <= gamma(np.bincount(uid, minlength=Ca * U))[:, None] * mag).all(), "gs"
        err, bound = np.abs(dq_got[:rows] - dq_want), gamma(H) * dq_mag
        print("dq at H = %d: max error %.3e, max bound %.3e" % (H, err.max(), bound.max()))
        assert (err <= bound).all(), "dq"
    assert not _bits(gs[Ca * U:]).any() and G.untouched(dq[rows:])
    gs_band(), dq_band()


# ------------------------------------------------------------------------------------------------------------------ window scatter
def _scatter_f64(dX, vox, Ca, QN):
    """float64 window scatter of dX [Ca QN, KP] (rows (i, q)): dfv[i, p + d - h, ch] += dX[(i, q), (d, ch)] inside the grid"""
    m, k, h = M_GRID, K_WIN, (K_WIN - 1) // 2
    p = np.stack([vox // (m * m), (vox // m) % m, vox % m], -1)                          # [QN, 3]
    d = np.stack(np.meshgrid(np.arange(k), np.arange(k), np.arange(k), indexing="ij"), -1).reshape(-1, 3)      # [k^3, 3] in window order
    t = p[:, None, :] + d[None] - h                                                      # [QN, k^3, 3]
    ok = ((t >= 0) & (t < m)).all(-1)
    tv = (t[..., 0] * m + t[..., 1]) * m + t[..., 2]
    out = np.zeros((Ca, NG, 20))
    win = dX[:, :E].reshape(Ca, QN, k ** 3, 20)
    for i in range(Ca):
        np.add.at(out[i], tv[ok], win[i][ok])
    return out


@pytest.mark.parametrize("integer", [True, False])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES)
def test_window_scatter_against_the_gather_backward(dev, shape, kind, integer):
    """dfv of the slot form (slot sum, slot product, scatter over the slots) against dpd_patch_rows_bwd on the hand-tiled pairs' full
    dX = g1 W1p^T (dpd_decoder_bwd_data with dX; W2 = identity and an open gate make its g1 the given rows), summed over j in float64.
    Integer operands: equal.  Normal operands: both sides are fp32 evaluations of sum_{rows covering v} sum_h g[r, h] W[col, h]; with
    A = the sum of the magnitudes of those addends (float64), the slot form errs by at most (Cb N - 1) [list sums] + H [product] +
    (U - 1) [scatter] roundings on A, the pair form by H [product] + (N - 1) [gather]: the difference is within gamma of their sum."""
    from dpdist_amd import lib as L, ops
    lib, s = L.load(), L.cur_stream()
    Ca, Cb, N = shape
    x, v = X._cross(shape, kind, not integer, integer), _inv(shape, kind, integer)
    g_t, W_t, g, W = _operands(dev, x, integer, 12)
    rows, QN, U = x.rows, Cb * N, x.U
    f32 = dict(dtype=torch.float32, device=dev)
    # ---- the slot form
    gs, gs_band, _, _ = _slot_sum(dev, x, v, g_t, W_t, want_dq=False)
    WT = W_t.t().contiguous()
    dXs, dXs_band = G.banded((x.cap, KP), KP, **f32)
    ops.gemm_f32(gs.contiguous(), WT, tile=32, out=dXs)
    dfv, dfv_band = G.banded((Ca * NG, 20), 20, **f32)
    L.check(lib.dpd_cross_scatter(L.ptr(dXs), L.ptr(x.cnt), L.ptr(v.svox), Ca, Cb, N, M_GRID, K_WIN, KP, L.ptr(dfv), s), "dpd_cross_scatter")
    # ---- the pair form: dpd_decoder_bwd_data (phase 4: g1 = (g2 W2^T) * [h1 > 0], dX = g1 W1p^T), dpd_patch_rows_bwd
    eye, ones = torch.eye(H_DEC, **f32), torch.ones(rows, H_DEC, **f32)
    g1 = torch.empty(rows, H_DEC, **f32)
    dX = torch.empty(rows, KP, **f32)
    cp = L.make_params(W_t, eye, eye, eye, eye, eye, eye, eye)
    g2 = g_t[:rows].contiguous()
    L.check(lib.dpd_decoder_bwd_data(None, None, None, L.ptr(ones), L.ptr(ones), None, rows, KP, H_DEC, cp, 0, None, L.ptr(g2), L.ptr(g2),
                                     L.ptr(g1), L.ptr(dX), None, None, 0, None, 4, s), "dpd_decoder_bwd_data")
    assert torch.equal(_bits(g1), _bits(g2))
    vox_t = x.vox[None].expand(Ca, -1).reshape(-1).contiguous()
    _, dfv_pairs = ops.patch_rows_bwd(dX, vox_t, Ca * Cb, N, M_GRID, K_WIN, want_dq=False)
    torch.cuda.synchronize()
    want = dfv_pairs.double().view(Ca, Cb, NG, 20).sum(1).cpu().numpy()
    got = dfv.double().view(Ca, NG, 20).cpu().numpy()
    vox = x.vox.cpu().numpy().astype(np.int64)
    truth = _scatter_f64(g[:rows] @ W.T, vox, Ca, QN)
    assert np.abs(truth).max() > 0
    if integer:
        assert np.array_equal(want, truth), "the gather backward itself"
        assert np.array_equal(got, want)
    else:
        A = _scatter_f64(np.abs(g[:rows]) @ np.abs(W).T, vox, Ca, QN)
        n_slot, n_pair = (QN - 1) + H_DEC + (U - 1), H_DEC + (N - 1)
        for name, err, n in (("slot form vs float64", np.abs(got - truth), n_slot + 1), ("pair form vs float64", np.abs(want - truth), n_pair + 1),
                             ("slot form vs pair form", np.abs(got - want), n_slot + n_pair + 1)):
            bound = gamma(n) * A
            print("%s: max error %.3e, max bound %.3e" % (name, err.max(), bound.max()))
            assert (err <= bound).all(), name
    gs_band(), dXs_band(), dfv_band(), v.bands(), x.bands()


# ------------------------------------------------------------------------------------------------------ the chunk entry, guard-banded
@pytest.mark.parametrize("kind", ["random", "outside"])
def test_chunk_entries_write_nothing_beyond_their_extents(dev, kind):
    """dpd_decoder_fwd_cross_keep: h3, y, pred bitwise those of dpd_decoder_fwd_cross, h1 and h2 kept.  dpd_cross_bwd: every buffer inside
    its guard band; gs / dXs / dfv are bitwise the pieces run one by one; gQ is the fp32 chain over the surfaces continued from what it held."""
    from dpdist_amd import lib as L, ops
    lib, s = L.load(), L.cur_stream()
    shape = SHAPES[1]                                               # (2, 3, 36): pad rows
    Ca, Cb, N = shape
    x = X._cross(shape, kind, False)
    v = _Inv(x)
    rows, rows_p, H, QN = x.rows, x.rows_p, H_DEC, Cb * N
    P = X._params(dev)
    cp = L.make_params(*P.views(), *P.transposed())
    f32 = dict(dtype=torch.float32, device=dev)
    bufs, bands = {}, []
    for name, shp in (("Pu", (x.cap, H)), ("h1", (rows_p, H)), ("h2", (rows_p, H)), ("h3", (rows_p, H)), ("y", (rows_p, 3)), ("pred", (rows_p, 3)),
                      ("dpred", (rows_p, 3)), ("dy", (rows_p, 3)), ("ga", (rows_p, H)), ("gb", (rows_p, H)), ("dq", (rows_p, 3)),
                      ("gs", (x.cap, H)), ("dXs", (x.cap, KP)), ("dfv", (Ca * NG, 20)), ("gQ", (QN, 3)), ("act0", (rows_p, H)), ("act1", (rows_p, H)),
                      ("y0", (rows_p, 3)), ("pred0", (rows_p, 3)), ("Pu0", (x.cap, H))):
        bufs[name], b = G.banded(shp, shp[1], **f32)
        bands.append(b)
    Dd, Dd_band = G.banded_flat(Ca * Cb, **f32)
    Dk, Dk_band = G.banded_flat(Ca * Cb, **f32)
    bands += [Dd_band, Dk_band]
    p = {k: L.ptr(t) for k, t in bufs.items()}
    L.check(lib.dpd_decoder_fwd_cross(L.ptr(x.Xu), x.cap, x.cap, L.ptr(x.Xt), L.ptr(x.uid), L.ptr(x.cnt), p["Pu0"], L.ptr(x.maskr), Ca * Cb, N, KP, H,
                                      cp, p["act0"], p["act1"], p["y0"], p["pred0"], L.ptr(Dd), s), "dpd_decoder_fwd_cross")
    L.check(lib.dpd_decoder_fwd_cross_keep(L.ptr(x.Xu), x.cap, x.cap, L.ptr(x.Xt), L.ptr(x.uid), L.ptr(x.cnt), p["Pu"], L.ptr(x.maskr), Ca * Cb, N,
                                           KP, H, cp, p["h1"], p["h2"], p["h3"], p["y"], p["pred"], L.ptr(Dk), s), "dpd_decoder_fwd_cross_keep")
    assert lib.dpd_decoder_fwd_cross_keep(L.ptr(x.Xu), x.cap, x.cap, L.ptr(x.Xt), L.ptr(x.uid), L.ptr(x.cnt), p["Pu"], L.ptr(x.maskr), Ca * Cb, N,
                                          KP, H, cp, p["h1"], p["h1"], p["h3"], p["y"], p["pred"], None, s) == -2        # three distinct buffers
    for a, b in (("h3", "act0"), ("h2", "act1"), ("y", "y0"), ("pred", "pred0")):
        assert torch.equal(_bits(bufs[a]), _bits(bufs[b])), a
    assert torch.equal(_bits(Dk), _bits(Dd)) and float(bufs["h1"].max()) > 0
    Gd = torch.tensor(np.random.default_rng(21).standard_normal(Ca * Cb).astype(np.float32), device=dev)
    bufs["gQ"].fill_(0.25)                                          # what an earlier chunk left
    L.check(lib.dpd_cross_bwd(L.ptr(Gd), L.ptr(x.maskr), p["y"], p["h1"], p["h2"], p["h3"], L.ptr(x.cnt), L.ptr(v.start), L.ptr(v.qlist),
                              L.ptr(v.svox), Ca, Cb, N, M_GRID, K_WIN, KP, H, x.cap, cp, p["dpred"], p["dy"], p["ga"], p["gb"], p["dq"], p["gs"],
                              p["dXs"], p["dfv"], p["gQ"], s), "dpd_cross_bwd")
    torch.cuda.synchronize()
    dpred = bufs["dpred"]
    want = (Gd / N).repeat_interleave(N)
    assert torch.equal(_bits(dpred[:rows, 0]), _bits(want)) and not _bits(dpred[:rows, 1:]).any() and not _bits(dpred[rows:]).any()
    g1 = bufs["ga"]
    assert not g1[rows:].abs().max() > 0 and float(g1.abs().max()) > 0          # pad rows: exact zeros through the mask
    msk = x.maskr[:rows] == 0
    if kind == "outside":
        assert int(msk.sum()) == Ca * Cb * 4 and not g1[:rows][msk].abs().max() > 0 and not bufs["dq"][:rows][msk].abs().max() > 0
    gs, _, dq, _ = _slot_sum(dev, x, v, g1.contiguous(), P.view("W1p"))
    assert torch.equal(_bits(gs), _bits(bufs["gs"])) and torch.equal(_bits(dq[:rows]), _bits(bufs["dq"][:rows]))
    assert G.untouched(bufs["dq"][rows:])
    dXs = ops.gemm_f32(gs.contiguous(), P.transposed()[2], tile=32)
    assert torch.equal(_bits(dXs), _bits(bufs["dXs"]))
    acc = torch.full((QN, 3), 0.25, **f32)
    for i in range(Ca):
        acc = acc + bufs["dq"][i * QN:(i + 1) * QN]
    assert torch.equal(_bits(acc), _bits(bufs["gQ"]))
    assert torch.isfinite(bufs["dfv"]).all() and float(bufs["dfv"].abs().max()) > 0
    for b in bands:
        b()
    v.bands(), x.bands()


# ------------------------------------------------------------------------------------------------------------ the public interface
def _cu(t, dev, grad=False):
    return torch.tensor(t, device=dev).requires_grad_(grad)


@functools.lru_cache(maxsize=None)
def _upstream(shape):
    """G, G_AB, G_BA [Ca, Cb]: the random upstream matrices of a shape (float32, fixed seed)"""
    Ca, Cb, N = shape
    rng = np.random.default_rng([77, Ca, Cb, N])
    return tuple(rng.standard_normal((Ca, Cb)).astype(np.float32) for _ in range(3))


def _loss(out, Gs, directed, dev_or_dtype):
    """(G D).sum(), plus (G_AB D_AB).sum() + (G_BA D_BA).sum() with `directed`"""
    mk = (lambda g: torch.tensor(g, dtype=dev_or_dtype)) if isinstance(dev_or_dtype, torch.dtype) else (lambda g: torch.tensor(g, device=dev_or_dtype))
    D, d_ab, d_ba = out
    loss = (mk(Gs[0]) * D).sum()
    if directed:
        loss = loss + (mk(Gs[1]) * d_ab).sum() + (mk(Gs[2]) * d_ba).sum()
    return loss


@functools.lru_cache(maxsize=None)
def _oracle_grads(shape, directed, dtype, self_matrix=False):
    """gA, gB of the loss through oracle.restate.get_model / get_loss on the hand-tiled pairs (numpy float64 arrays)"""
    from oracle import restate as R
    Ca, Cb, N = shape
    A, B = X._sets(shape)
    if self_matrix:
        B = A
    W = R.as_torch_weights(synth.make_weights("wide", mlp=(H_DEC,) * 3), dtype)
    a = torch.tensor(A, dtype=dtype, requires_grad=True)
    b = torch.tensor(B, dtype=dtype, requires_grad=True)
    ps, _ = R.get_model(a.repeat_interleave(Cb, 0), b.repeat(Ca, 1, 1), W, m=M_GRID, k=K_WIN, sigma=0.125)
    d_ab = ps["pred_listAB"][:, :, 0, 0].mean(1).view(Ca, Cb)
    d_ba = ps["pred_listBA"][:, :, 0, 0].mean(1).view(Ca, Cb)
    D = torch.stack([R.get_loss({k: t[p:p + 1] for k, t in ps.items()}, torch.zeros(1, N, dtype=dtype))[1] for p in range(Ca * Cb)]).view(Ca, Cb)
    gA, gB = torch.autograd.grad(_loss((D, d_ab, d_ba), _upstream(shape), directed, dtype), [a, b])
    return gA.double().numpy(), gB.double().numpy()


def _bar(shape, directed, self_matrix=False):
    """the project's input-gradient bar (tests/test_gpu_parity.py: test_losses_and_input_gradients_golden) per gradient: max(4 x the
    distance of the float32 oracle from the float64 one, 2e-4 max(1, max|ref|)) -> [(ref, bar)] for gA, gB"""
    r64, r32 = _oracle_grads(shape, directed, torch.float64, self_matrix), _oracle_grads(shape, directed, torch.float32, self_matrix)
    return [(a, max(4.0 * np.abs(b - a).max(), 2e-4 * max(1.0, np.abs(a).max()))) for a, b in zip(r64, r32)]


def _matrix_grads(dev, shape, directed, max_rows=16384, needA=True, needB=True, retain=False):
    from dpdist_amd import DPDistMatrix
    A, B = X._sets(shape)
    a, b = _cu(A, dev, needA), _cu(B, dev, needB)
    out = DPDistMatrix(X._params(dev), max_rows=max_rows)(a, b, return_directed=True)
    loss = _loss(out, _upstream(shape), directed, dev)
    wrt = [t for t, need in ((a, needA), (b, needB)) if need]
    gs = list(torch.autograd.grad(loss, wrt, retain_graph=retain))
    again = list(torch.autograd.grad(loss, wrt)) if retain else None
    return gs, again, out


@pytest.mark.parametrize("shape", SHAPES)
def test_forward_is_bitwise_dpdist_matrix(dev, shape):
    from dpdist_amd import DPDistMatrix, dpdist_matrix
    A, B = X._sets(shape)
    P = X._params(dev)
    want = dpdist_matrix(P, _cu(A, dev), _cu(B, dev), return_directed=True)
    mod = DPDistMatrix(P)
    for grad in (True, False):
        got = mod(_cu(A, dev, grad), _cu(B, dev, grad), return_directed=True)
        assert all(g.requires_grad == grad for g in got)
        for g, w in zip(got, want):
            assert g.shape == w.shape and torch.equal(_bits(g), _bits(w))
    assert torch.equal(_bits(mod(_cu(A, dev, True), _cu(B, dev))), _bits(want[0]))
    # a set against itself
    want = dpdist_matrix(P, _cu(A, dev), return_directed=True)
    got = mod(_cu(A, dev, True), return_directed=True)
    for g, w in zip(got, want):
        assert g.requires_grad and torch.equal(_bits(g), _bits(w))


@pytest.mark.parametrize("shape,directed", [(SHAPES[0], True), (SHAPES[0], False), (SHAPES[1], False), (SHAPES[2], False)])
def test_gradients_against_the_float64_oracle(dev, shape, directed):
    """loss = (G D).sum() (+ the directed terms for one case) under a random upstream G: gA, gB against torch.autograd.grad through the
    float64 oracle on the hand-tiled pairs, at the project's input-gradient bar."""
    (gA, gB), _, _ = _matrix_grads(dev, shape, directed)
    for name, got, (ref, bar) in zip(("gA", "gB"), (gA, gB), _bar(shape, directed)):
        err = np.abs(got.double().cpu().numpy() - ref).max()
        print("%s vs float64 oracle: %.3e (bar %.3e, max|ref| %.3e)" % (name, err, bar, np.abs(ref).max()))
        assert np.abs(ref).max() > 20 * bar, "a reference gradient without structure makes the bar vacuous"
        assert got.shape == ref.shape and err <= bar, name


@pytest.mark.parametrize("shape", SHAPES)
def test_gradients_against_the_pair_path(dev, shape):
    """the same gradients through DPDistLoss on the hand-tiled pairs, each pair weighted by G[i, j]: within twice the oracle bar (both
    sit within that bar of the same float64 reference)"""
    from dpdist_amd.model import DPDistLoss, DPDistModel
    Ca, Cb, N = shape
    A, B = X._sets(shape)
    mod = DPDistModel(Embedding_Size=512, k=K_WIN, localSNmlp=(H_DEC,) * 3, sigma3dmfv=0.125, device=dev)
    mod.load_tf_state_dict(synth.make_weights("wide", mlp=(H_DEC,) * 3))
    loss_fn = DPDistLoss(mod)
    Gm = _upstream(shape)[0]
    wA, wB = torch.zeros(Ca, N, 3, dtype=torch.float64, device=dev), torch.zeros(Cb, N, 3, dtype=torch.float64, device=dev)
    for i in range(Ca):
        for j in range(Cb):
            a, b = _cu(A[i:i + 1], dev, True), _cu(B[j:j + 1], dev, True)
            ga, gb = torch.autograd.grad(loss_fn(a, b) * float(Gm[i, j]), [a, b])
            wA[i] += ga[0].double()
            wB[j] += gb[0].double()
    (gA, gB), _, _ = _matrix_grads(dev, shape, False)
    for name, got, want, (ref, bar) in zip(("gA", "gB"), (gA, gB), (wA, wB), _bar(shape, False)):
        err = float((got.double() - want).abs().max())
        print("%s vs the pair path: %.3e (twice the bar: %.3e)" % (name, err, 2 * bar))
        assert err <= 2 * bar, name


@pytest.mark.parametrize("shape", SHAPES[:2])
def test_chunking_changes_no_bit(dev, shape):
    (a1, b1), _, _ = _matrix_grads(dev, shape, True, max_rows=1 << 20)
    (a2, b2), _, _ = _matrix_grads(dev, shape, True, max_rows=1)          # one surface cloud per chunk
    assert torch.equal(_bits(a1), _bits(a2)) and torch.equal(_bits(b1), _bits(b2))
    assert float(a1.abs().max()) > 0 and float(b1.abs().max()) > 0


def test_self_matrix(dev):
    """B = None: D bitwise dpdist_matrix(P, A); the gradient == gA + gB of the two-set call on (A, A.clone()) within the oracle bar"""
    from dpdist_amd import DPDistMatrix, dpdist_matrix
    shape = (3, 3, 64)
    A = X._sets(SHAPES[0])[0]
    P = X._params(dev)
    Gs = _upstream(shape)
    a = _cu(A, dev, True)
    mod = DPDistMatrix(P)
    out = mod(a, return_directed=True)
    for g, w in zip(out, dpdist_matrix(P, _cu(A, dev), return_directed=True)):
        assert torch.equal(_bits(g), _bits(w))
    (g_self,) = torch.autograd.grad(_loss(out, Gs, True, dev), [a])
    a2, b2 = _cu(A, dev, True), _cu(A.copy(), dev, True)
    gA, gB = torch.autograd.grad(_loss(mod(a2, b2, return_directed=True), Gs, True, dev), [a2, b2])
    two = gA.double() + gB.double()
    A_ = np.array(A)

    @functools.lru_cache(maxsize=None)
    def oracle(dtype):
        from oracle import restate as R
        W = R.as_torch_weights(synth.make_weights("wide", mlp=(H_DEC,) * 3), dtype)
        t = torch.tensor(A_, dtype=dtype, requires_grad=True)
        ps, _ = R.get_model(t.repeat_interleave(3, 0), t.repeat(3, 1, 1), W, m=M_GRID, k=K_WIN, sigma=0.125)
        d_ab = ps["pred_listAB"][:, :, 0, 0].mean(1).view(3, 3)
        d_ba = ps["pred_listBA"][:, :, 0, 0].mean(1).view(3, 3)
        (g,) = torch.autograd.grad(_loss(((d_ab + d_ba) / 2, d_ab, d_ba), Gs, True, dtype), [t])
        return g.double().numpy()

    ref = oracle(torch.float64)
    bar = max(4.0 * np.abs(oracle(torch.float32) - ref).max(), 2e-4 * max(1.0, np.abs(ref).max()))
    e1 = float((g_self.double() - two).abs().max())
    e2 = np.abs(g_self.double().cpu().numpy() - ref).max()
    print("self vs two sets: %.3e; self vs float64 oracle: %.3e (bar %.3e, max|ref| %.3e)" % (e1, e2, bar, np.abs(ref).max()))
    assert np.abs(ref).max() > 20 * bar
    assert e1 <= bar and e2 <= bar


@pytest.mark.parametrize("shape", SHAPES[:2])
def test_partial_gradients(dev, shape):
    """only one set requires grad: bitwise the both-sets gradient, nothing for the other; a second backward gives the same bits"""
    (gA, gB), again, _ = _matrix_grads(dev, shape, True, retain=True)
    assert torch.equal(_bits(again[0]), _bits(gA)) and torch.equal(_bits(again[1]), _bits(gB))
    (oA,), againA, outA = _matrix_grads(dev, shape, True, needB=False, retain=True)
    (oB,), _, _ = _matrix_grads(dev, shape, True, needA=False)
    assert torch.equal(_bits(oA), _bits(gA)) and torch.equal(_bits(againA[0]), _bits(gA)) and torch.equal(_bits(oB), _bits(gB))
    # .backward() leaves no gradient on the set that asked for none
    from dpdist_amd import DPDistMatrix
    A, B = X._sets(shape)
    a, b = _cu(A, dev, True), _cu(B, dev)
    DPDistMatrix(X._params(dev))(a, b).sum().backward()
    assert a.grad is not None and b.grad is None


def test_masked_queries(dev):
    """kind `outside`: with the upstream on D_AB alone, gB is the query route of direction AB: exactly 0 on every masked query; gA (the
    surface route) keeps its bits when the masked queries are moved to other points outside the cube"""
    from dpdist_amd import DPDistMatrix
    shape = SHAPES[0]
    Ca, Cb, N = shape
    A = X._sets(shape)[0]
    Bq = np.array(X._queries("outside", Cb, N))
    masked = [0, 5, 20, N - 1]
    mod = DPDistMatrix(X._params(dev))
    Gab = torch.tensor(_upstream(shape)[1], device=dev)

    def grads(B_np):
        a, b = _cu(A, dev, True), _cu(B_np, dev, True)
        _, d_ab, _ = mod(a, b, return_directed=True)
        return torch.autograd.grad((Gab * d_ab).sum(), [a, b])

    gA, gB = grads(Bq)
    assert not _bits(gB[:, masked]).bitwise_and(0x7FFFFFFF).any()               # +0 or -0
    live = [n for n in range(N) if n not in masked]
    assert float(gB[:, live].abs().max()) > 0 and float(gA.abs().max()) > 0
    moved = Bq.copy()
    moved[:, masked] = np.array([[-2.0, 0.3, 5.0], [1.25, -1.5, 0.0], [0.5, 0.5, -1.0], [3.0, 3.0, 3.0]], dtype=np.float32)[None]
    gA2, gB2 = grads(moved)
    assert torch.equal(_bits(gA2), _bits(gA))
    assert not _bits(gB2[:, masked]).bitwise_and(0x7FFFFFFF).any()


def test_module_refuses_like_dpdist_matrix(dev):
    from dpdist_amd import DPDistMatrix
    from dpdist_amd.model import DPDistModel
    A, B = (torch.tensor(t, device=dev) for t in X._sets(SHAPES[0]))
    with pytest.raises(ValueError, match="fp32"):
        DPDistMatrix(X._params(dev, compute_dtype="bf16"))
    mod = DPDistMatrix(X._params(dev))
    with pytest.raises(ValueError, match="same number of points"):
        mod(A.requires_grad_(True), B[:, :36].contiguous())
    with pytest.raises(ValueError, match="not supported"):
        DPDistMatrix(X._params(dev), Embedding_Size=1331)(A, B)
    m = DPDistModel(Embedding_Size=512, k=K_WIN, localSNmlp=(H_DEC,) * 3, sigma3dmfv=0.125, device=dev)
    m.load_tf_state_dict(synth.make_weights("wide", mlp=(H_DEC,) * 3))
    with pytest.raises(ValueError, match="contradicts"):
        DPDistMatrix(m, Embedding_Size=1000)
    got = DPDistMatrix(m)(A.detach().requires_grad_(True), B)
    assert torch.equal(_bits(got), _bits(mod(A.detach(), B)))

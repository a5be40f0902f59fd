"""Slot-summed backward of the per-point field (dpd_field_invert, dpd_field_slot_sum, dpd_field_scatter, dpd_field_bwd;
dpdist_amd.field.DPDistField(backward="slots")).

The pieces are pinned one by one on the entry cases of tests/field_cases.py, in the structure of tests/test_cross_grad_gpu.py: the inverted
index against numpy, the slot sum and the query route against float64 (exact on integer operands, an addend bound on normal ones), the
window scatter against the library's own gather backward on the same chunk's full dX, the chunk entry against its pieces run one by one,
the module's gradients against the float64 oracle of tests/field_cases.py.  The numpy restatements are those of
tests/field_slots_cases.py, which tests/test_field_slots_cpu.py ties to the autograd oracle.  Every output of a new entry sits in a
NaN-filled guard-banded buffer (tests/gemm_cases.py).
"""
import functools

import numpy as np
import pytest
import torch

from tests import field_cases as FC
from tests import field_slots_cases as FS
from tests import gemm_cases as G
from tests import test_cross_grad_gpu as XG
from tests import test_cross_gpu as X
from tests import test_field_gpu as TF

pytestmark = pytest.mark.gpu

M_GRID, K_WIN, H_DEC, KP, NG, E = FC.M_GRID, FC.K_WIN, FC.H_DEC, FC.KP, FC.NG, FC.E
CASES = [c[0] for c in FC.ENTRY_CASES]
SUM_CASES = ["reference", "distinct", "one_voxel", "capacity"]
E_NULL, E_DIM, E_UNSUPPORTED = -1, -2, -3
gamma, _bits, _cu = XG.gamma, X._bits, TF._cu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible")
    from dpdist_amd import lib
    lib.load()
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------------------------------------------- the inverted index
class _Inv:
    """dpd_field_invert on a chunk's index (vox [n T], slot_of_vox [n, m^3], ucount [n]), into guard-banded buffers"""

    def __init__(self, vox, slot, ucount, n, T):
        from dpdist_amd import lib as L
        lib, s = L.load(), L.cur_stream()
        i32 = dict(dtype=torch.int32, device=vox.device)
        self.cap = cap = lib.dpd_field_slot_capacity(n, T, M_GRID)
        self.start, self.start_band = G.banded_flat(cap + 1, **i32)
        self.qlist, self.qlist_band = G.banded_flat(n * T, **i32)
        self.svox, self.svox_band = G.banded_flat(cap, **i32)
        self.scloud, self.scloud_band = G.banded_flat(cap, **i32)
        L.check(lib.dpd_field_invert(L.ptr(vox), L.ptr(slot), L.ptr(ucount), n, T, M_GRID, cap, L.ptr(self.start), L.ptr(self.qlist),
                                     L.ptr(self.svox), L.ptr(self.scloud), s), "dpd_field_invert")
        torch.cuda.synchronize()
        self.np = FS.invert(vox.cpu().numpy().reshape(n, T), cap)                 # the restatement on the same voxels

    def bands(self):
        for b in (self.start_band, self.qlist_band, self.svox_band, self.scloud_band):
            b()


@functools.lru_cache(maxsize=None)
def _inv(name, integer=False):
    x = TF._field(name, False, integer)
    return _Inv(x.vox, x.slot, x.ucount, x.n, x.T)


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("name", CASES)
def test_inverted_index(dev, name, shared):
    """per cloud, qlist == a stable argsort of the slots; slot_start == the prefix of np.bincount shifted to the cloud's rows, indexed by
    base_c + s; slot_vox, slot_cloud exact; the dead slots up to the capacity as the header states them"""
    x = TF._field(name, shared, False)
    v = _Inv(x.vox, x.slot, x.ucount, x.n, x.T) if shared else _inv(name)
    n, T, cap = x.n, x.T, x.cap
    assert v.cap == cap
    vox = x.vox.cpu().numpy().astype(np.int64).reshape(n, T)
    slot = x.slot.cpu().numpy().reshape(n, NG)
    base = np.concatenate([[0], np.cumsum(x.U)]).astype(np.int64)
    total = int(base[-1])
    want_q = np.zeros((n, T), dtype=np.int32)
    want_start = np.full(cap + 1, n * T, dtype=np.int32)
    want_vox, want_cloud = np.full(cap, -1, dtype=np.int32), np.full(cap, -1, dtype=np.int32)
    for c in range(n):
        slots = slot[c][vox[c]]
        assert slots.min() >= 0 and slots.max() == x.U[c] - 1
        counts = np.bincount(slots, minlength=x.U[c])
        assert counts.min() >= 1 and counts.sum() == T
        want_q[c] = np.argsort(slots, kind="stable")
        want_start[base[c]:base[c + 1]] = c * T + np.concatenate([[0], np.cumsum(counts)[:-1]])
        want_vox[base[c]:base[c + 1]] = np.unique(vox[c])
        want_cloud[base[c]:base[c + 1]] = c
    for got, want in ((v.qlist, want_q.reshape(-1)), (v.start, want_start), (v.svox, want_vox), (v.scloud, want_cloud)):
        assert torch.equal(got.cpu(), torch.tensor(want))
    # the restatement the other tests lean on says the same
    for got, key in ((v.qlist, "qlist"), (v.start, "slot_start"), (v.svox, "slot_vox"), (v.scloud, "slot_cloud")):
        assert np.array_equal(got.cpu().numpy(), v.np[key].reshape(-1))
    assert np.array_equal(x.uid.cpu().numpy()[:n * T], v.np["uid"].reshape(-1))
    assert total <= cap
    if name == "smallest":
        assert (n, T, total, cap) == (1, 1, 1, 32)
    if name == "distinct":
        assert x.U == [T] * n and (np.diff(want_start[:total + 1]) == 1).all()
    if name == "capacity":
        assert total == cap == NG                                    # no dead slot: slot_start[cap] alone holds the end
    if name == "one_voxel":
        assert x.U == [1] * n and want_start[:3].tolist() == [0, T, 2 * T]
    if name == "outside":
        assert (want_vox[base[:-1]] == 0).all()                      # masked queries: voxel 0's slot, the first of every cloud
    v.bands()
    x.bands()


# -------------------------------------------------------------------------------------------------------- slot sum and query route
def _operands(dev, rows, rows_p, integer, seed, H=H_DEC):
    """g1 [rows_p, H] (pad rows zero, as the decoder's mask leaves them) and W1p [KP, H]; float32 on the device, float64 on the host"""
    rng = np.random.default_rng([seed, rows, int(integer), H])
    if integer:
        g = G.small_int(rng, (rows_p, H), KP).astype(np.float64)
        W = G.small_int(rng, (KP, H), KP).astype(np.float64)
    else:
        g = rng.standard_normal((rows_p, H)).astype(np.float32).astype(np.float64)
        W = (rng.standard_normal((KP, H)) * 0.05).astype(np.float32).astype(np.float64)
    g[rows:] = 0.0
    return torch.tensor(g, dtype=torch.float32, device=dev), torch.tensor(W, dtype=torch.float32, device=dev), g, W


def _slot_sum(dev, n, T, cnt, v, g_t, W_t, want_gs=True, want_dq=True):
    from dpdist_amd import lib as L
    lib, s = L.load(), L.cur_stream()
    f32 = dict(dtype=torch.float32, device=dev)
    H = g_t.shape[1]
    gs, gs_band = G.banded((v.cap, H), H, **f32)
    dq, dq_band = G.banded((g_t.shape[0], 3), 3, **f32)
    L.check(lib.dpd_field_slot_sum(L.ptr(g_t), L.ptr(cnt), L.ptr(v.start), L.ptr(v.qlist), L.ptr(v.scloud), L.ptr(W_t), n, T, M_GRID, K_WIN, KP,
                                   H, v.cap, L.ptr(gs) if want_gs else None, L.ptr(dq) if want_dq else None, 3 * T, s), "dpd_field_slot_sum")
    torch.cuda.synchronize()
    return gs, gs_band, dq, dq_band


@pytest.mark.parametrize("integer", [True, False])
@pytest.mark.parametrize("name", SUM_CASES)
def test_slot_sum_and_query_route_against_float64(dev, name, integer):
    """gs[base_c + s] = the float64 index_add of the g1 rows of (cloud c, slot s); dq[r] = the float64 dot products with the three
    q - centre rows of W1p.  Integer operands: equal.  Normal operands: within gamma(n) * sum |addend| per element, n = the length of the
    slot's list (gs) and H (dq, whose addends are the fp32 products), the bound of tests/test_cross_grad_gpu.py.  Dead slots up to the
    capacity are ZERO rows; the pad rows of dq are untouched; each half alone gives the same bits and leaves the other buffer alone."""
    x, v = TF._field(name, False, integer), _inv(name, integer)
    n, T, rows = x.n, x.T, x.rows
    g_t, W_t, g, W = _operands(dev, rows, x.rows_p, integer, 11)
    gs, gs_band, dq, dq_band = _slot_sum(dev, n, T, x.cnt, v, g_t, W_t)
    total = sum(x.U)
    uid = x.uid.cpu().numpy()[:rows].astype(np.int64)
    want, mag = np.zeros((total, H_DEC)), np.zeros((total, H_DEC))
    np.add.at(want, uid, g[:rows])
    np.add.at(mag, uid, np.abs(g[:rows]))
    n_seg = np.bincount(uid, minlength=total)
    got = gs.double().cpu().numpy()
    prod = g[:rows, None, :].astype(np.float32) * W[E:E + 3].astype(np.float32)[None]          # [rows, 3, H]: the fp32 products
    dq_want, dq_mag = prod.astype(np.float64).sum(-1), np.abs(prod.astype(np.float64)).sum(-1)
    dq_got = dq.double().cpu().numpy()
    if integer:
        assert np.array_equal(got[:total], want), "gs"
        assert np.array_equal(got, FS.slot_sum(g, v.np)), "gs against the restatement"
        assert np.array_equal(dq_got[:rows], dq_want), "dq"
    else:
        err, bound = np.abs(got[:total] - want), gamma(n_seg)[:, None] * mag
        print("gs: max error %.3e, max bound %.3e, longest list %d" % (err.max(), bound.max(), n_seg.max()))
        assert (err <= bound).all(), "gs"
        err, bound = np.abs(dq_got[:rows] - dq_want), gamma(H_DEC) * dq_mag
        print("dq: max error %.3e, max bound %.3e" % (err.max(), bound.max()))
        assert (err <= bound).all(), "dq"
    assert not _bits(gs[total:]).any()                               # dead slots: zero rows
    assert G.untouched(dq[rows:])
    if name == "reference":
        assert total < x.cap and n_seg.max() > 1 and x.rows_p > rows
    if name == "distinct":
        assert n_seg.max() == 1 and np.array_equal(got[:total][uid], g[:rows])       # one addend: the row itself
    if name == "one_voxel":
        assert n_seg.tolist() == [T] * n
    if name == "capacity":
        assert total == x.cap and n_seg.max() > 1
    gs_band(), dq_band(), v.bands(), x.bands()
    gs2, b2, dq2, c2 = _slot_sum(dev, n, T, x.cnt, v, g_t, W_t, want_dq=False)
    assert torch.equal(_bits(gs2), _bits(gs)) and G.untouched(dq2)
    gs3, b3, dq3, c3 = _slot_sum(dev, n, T, x.cnt, v, g_t, W_t, want_gs=False)
    assert torch.equal(_bits(dq3[:rows]), _bits(dq[:rows])) and G.untouched(gs3)
    b2(), c2(), b3(), c3()


@pytest.mark.parametrize("H", [64, 320, 1024])
def test_slot_sum_at_other_widths(dev, H):
    """a quarter of a wave (64), a whole wave and a quarter (320), four waves (1024): exact on integer operands"""
    x, v = TF._field("reference", False, True), _inv("reference", True)
    g_t, W_t, g, W = _operands(dev, x.rows, x.rows_p, True, 13, H)
    gs, gs_band, dq, dq_band = _slot_sum(dev, x.n, x.T, x.cnt, v, g_t, W_t)
    assert np.array_equal(gs.double().cpu().numpy(), FS.slot_sum(g, v.np))
    assert np.array_equal(dq.double().cpu().numpy()[:x.rows], g[:x.rows] @ W[E:E + 3].T) and G.untouched(dq[x.rows:])
    gs_band(), dq_band()


def test_query_route_in_place_with_a_cloud_stride(dev):
    """the `tile` chunk (queries [64, 150) of three clouds with 150 each): with dq_cloud_stride = 3 * 150 the rows of cloud c are written in
    place at c * 450 floats into a gradient tensor [3, 150, 3]; the bits of the contiguous call, and the queries before the tile untouched"""
    from dpdist_amd import lib as L
    lib, s = L.load(), L.cur_stream()
    x, v = TF._field("tile", False, False), _inv("tile")
    n, T, t0, M = x.n, x.T, x.t0, FC.T_REF
    g_t, W_t, _, _ = _operands(dev, x.rows, x.rows_p, False, 14)
    _, _, dq, _ = _slot_sum(dev, n, T, x.cnt, v, g_t, W_t, want_gs=False)
    gq, gq_band = G.banded((n * M, 3), 3, dtype=torch.float32, device=dev)
    tile = gq.view(n, M, 3)[:, t0:]
    L.check(lib.dpd_field_slot_sum(L.ptr(g_t), L.ptr(x.cnt), L.ptr(v.start), L.ptr(v.qlist), L.ptr(v.scloud), L.ptr(W_t), n, T, M_GRID, K_WIN, KP,
                                   H_DEC, v.cap, None, L.ptr(tile), 3 * M, s), "dpd_field_slot_sum")
    torch.cuda.synchronize()
    assert t0 + T == M and torch.equal(_bits(tile), _bits(dq[:x.rows].view(n, T, 3))) and G.untouched(gq.view(n, M, 3)[:, :t0])
    gq_band()


# ------------------------------------------------------------------------------------------------------------------ window scatter
def _slot_form(dev, n, T, cnt, ucount, v, g_t, W_t, dfv=None, accumulate=0):
    """slot sum -> slot product -> scatter -> (dfv [n m^3, 20] in a guard band, its check)"""
    from dpdist_amd import lib as L, ops
    lib, s = L.load(), L.cur_stream()
    f32 = dict(dtype=torch.float32, device=dev)
    gs, gs_band, _, _ = _slot_sum(dev, n, T, cnt, v, g_t, W_t, want_dq=False)
    dXs, dXs_band = G.banded((v.cap, KP), KP, **f32)
    ops.gemm_f32(gs.contiguous(), W_t.t().contiguous(), tile=32, out=dXs)
    band = None
    if dfv is None:
        dfv, band = G.banded((n * NG, 20), 20, **f32)
    L.check(lib.dpd_field_scatter(L.ptr(dXs), L.ptr(ucount), L.ptr(v.svox), n, T, M_GRID, K_WIN, KP, accumulate, L.ptr(dfv), s), "dpd_field_scatter")
    torch.cuda.synchronize()
    gs_band(), dXs_band()
    return dfv, band


def _scatter_rows_f64(dX, vox, n, T):
    """float64 window scatter of dX [n T, KP] over the rows, every cloud with its own voxels vox [n, T]"""
    return np.concatenate([XG._scatter_f64(dX[c * T:(c + 1) * T], vox[c], 1, T) for c in range(n)])


@pytest.mark.parametrize("integer", [True, False])
@pytest.mark.parametrize("name", SUM_CASES)
def test_window_scatter_against_the_gather_backward(dev, name, integer):
    """dfv of the slot form (slot sum, slot product, scatter over the cloud's own slots) against dpd_patch_rows_bwd on the same chunk's
    full dX = g1 W1p^T.  Integer operands: equal, and equal to float64.  Normal operands: both sides are fp32 evaluations of
    sum_{rows covering v} sum_h g[r, h] W[col, h]; with A = the sum of the magnitudes of those addends (float64), the slot form errs by at
    most (T - 1) [list sums] + H [product] + (U - 1) [scatter] roundings on A, the row form by H [product] + (T - 1) [gather]: the
    difference is within gamma of their sum (the rounding-derived bound of tests/test_cross_grad_gpu.py)."""
    from dpdist_amd import ops
    x, v = TF._field(name, False, integer), _inv(name, integer)
    n, T, rows = x.n, x.T, x.rows
    g_t, W_t, g, W = _operands(dev, rows, x.rows_p, integer, 12)
    dfv, dfv_band = _slot_form(dev, n, T, x.cnt, x.ucount, v, g_t, W_t)
    dX = ops.gemm_f32(g_t[:rows].contiguous(), W_t.t().contiguous(), tile=32)
    _, dfv_rows = ops.patch_rows_bwd(dX, x.vox.contiguous(), n, T, M_GRID, K_WIN, want_dq=False)
    torch.cuda.synchronize()
    want = dfv_rows.double().cpu().numpy()
    got = dfv.double().view(n, NG, 20).cpu().numpy()
    vox = x.vox.cpu().numpy().astype(np.int64).reshape(n, T)
    truth = _scatter_rows_f64(g[:rows] @ W.T, vox, n, T)
    assert np.abs(truth).max() > 0
    if integer:
        assert np.array_equal(want, truth), "the gather backward itself"
        assert np.array_equal(got, want)
        assert np.array_equal(got, FS.scatter(FS.slot_sum(g, v.np) @ W.T, v.np)), "the restatement"
    else:
        A = _scatter_rows_f64(np.abs(g[:rows]) @ np.abs(W).T, vox, n, T)
        n_slot, n_rows = (T - 1) + H_DEC + (max(x.U) - 1), H_DEC + (T - 1)
        for what, err, cnt in (("slot form vs float64", np.abs(got - truth), n_slot + 1), ("row form vs float64", np.abs(want - truth), n_rows + 1),
                               ("slot form vs row form", np.abs(got - want), n_slot + n_rows + 1)):
            bound = gamma(cnt) * A
            print("%s: max error %.3e, max bound %.3e" % (what, err.max(), bound.max()))
            assert (err <= bound).all(), what
    uncovered = (_scatter_rows_f64(np.ones((rows, KP)), vox, n, T) == 0).all(-1)          # [n, m^3]: the voxels no window covers
    assert (uncovered.any() or name != "one_voxel") and not _bits(dfv.view(n, NG, 20)[torch.tensor(uncovered, device=dev)]).any()      # +0.0
    dfv_band(), v.bands(), x.bands()


class _Tile:
    """dpd_field_index + dpd_field_invert of the queries [t0, t0 + T) of the reference case's first cloud (all 150 real)"""

    def __init__(self, dev, t0, T):
        from dpdist_amd import lib as L
        lib, s = L.load(), L.cur_stream()
        f32, i32 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int32, device=dev)
        q = torch.tensor(FC.queries()[:1], device=dev)
        self.T, self.rows_p = T, (T + 31) // 32 * 32
        self.vox, self.slot, self.ucount = torch.empty(T, **i32), torch.empty(NG, **i32), torch.empty(1, **i32)
        L.check(lib.dpd_field_index(L.ptr(q[:, t0:]), 3 * FC.T_REF, None, t0, 1, T, M_GRID, L.ptr(torch.empty(T, **f32)), L.ptr(self.vox),
                                    L.ptr(self.slot), L.ptr(self.ucount), s), "dpd_field_index")
        torch.cuda.synchronize()
        self.cnt = torch.tensor([1, int(self.ucount[0]), 0, 0], **i32)      # what dpd_field_gather writes for the chunk
        self.inv = _Inv(self.vox, self.slot, self.ucount, 1, T)


def test_scatter_accumulates_the_tiles_of_a_cloud(dev):
    """integer operands: the tiles [0, 64) then [64, 150) of one cloud, the second with `accumulate`, equal the one-chunk result exactly;
    a preset dfv is continued, not overwritten; without the flag it is overwritten"""
    rows = FC.T_REF
    g_t, W_t, g, W = _operands(dev, rows, 160, True, 15)
    one = _Tile(dev, 0, rows)
    dfv_one, band_one = _slot_form(dev, 1, rows, one.cnt, one.ucount, one.inv, g_t, W_t)
    want = FS.scatter(FS.slot_sum(g, one.inv.np) @ W.T, one.inv.np)
    assert np.array_equal(dfv_one.double().view(1, NG, 20).cpu().numpy(), want) and np.abs(want).max() > 0
    dfv, band = G.banded((NG, 20), 20, dtype=torch.float32, device=dev)
    for t0, T in ((0, 64), (64, 86)):
        t = _Tile(dev, t0, T)
        g_tile = torch.zeros(t.rows_p, H_DEC, device=dev)
        g_tile[:T] = g_t[t0:t0 + T]
        _slot_form(dev, 1, T, t.cnt, t.ucount, t.inv, g_tile, W_t, dfv=dfv, accumulate=int(t0 > 0))
        if t0 == 0:
            assert not torch.isnan(dfv).any() and not torch.equal(_bits(dfv), _bits(dfv_one))
    assert torch.equal(_bits(dfv), _bits(dfv_one))
    preset = torch.tensor(G.small_int(np.random.default_rng(16), (NG, 20), KP).astype(np.float32), device=dev)
    dfv.copy_(preset)
    _slot_form(dev, 1, rows, one.cnt, one.ucount, one.inv, g_t, W_t, dfv=dfv, accumulate=1)
    assert torch.equal(dfv, preset + dfv_one) and float(preset.abs().max()) > 0
    _slot_form(dev, 1, rows, one.cnt, one.ucount, one.inv, g_t, W_t, dfv=dfv, accumulate=0)
    assert torch.equal(_bits(dfv), _bits(dfv_one))
    band(), band_one()


# ------------------------------------------------------------------------------------------------------ the chunk entry, guard-banded
@pytest.mark.parametrize("shared", [False, True])
def test_chunk_entry_against_its_pieces(dev, shared):
    """dpd_field_bwd on the reference chunk: every buffer inside its guard band; gs / dXs / dfv are bitwise the pieces run one by one; the
    rows of clouds with their own queries are written in place, a shared set is the fp32 chain over the clouds continued from what gq
    held; masked and padded queries get exact zeros; dfv = NULL or gq = NULL skips that half and changes no bit of the other; `accumulate`
    continues a preset dfv"""
    from dpdist_amd import lib as L, ops
    lib, s = L.load(), L.cur_stream()
    x = TF._field("reference", shared, False)
    v = _Inv(x.vox, x.slot, x.ucount, x.n, x.T)
    n, T, rows, rows_p, H = x.n, x.T, x.rows, x.rows_p, H_DEC
    P = X._params(dev)
    cp = L.make_params(*P.views(), *P.transposed())
    f32 = dict(dtype=torch.float32, device=dev)
    bufs, bands = {}, []
    for name, shp in (("Pu", (x.cap, H)), ("h1", (rows_p, H)), ("h2", (rows_p, H)), ("h3", (rows_p, H)), ("y", (rows_p, 3)), ("pred", (rows_p, 3)),
                      ("dy", (rows_p, 3)), ("ga", (rows_p, H)), ("gb", (rows_p, H)), ("dq", (rows_p, 3)), ("gs", (x.cap, H)), ("dXs", (x.cap, KP)),
                      ("dfv", (n * NG, 20)), ("gq", (T if shared else n * T, 3)), ("dfv2", (n * NG, 20)), ("gq2", (T if shared else n * T, 3))):
        bufs[name], b = G.banded(shp, shp[1], **f32)
        bands.append(b)
    p = {k: L.ptr(t) for k, t in bufs.items()}
    L.check(lib.dpd_decoder_fwd_cross_keep(L.ptr(x.Xu), x.cap, x.cap, L.ptr(x.Xt), L.ptr(x.uid), L.ptr(x.cnt), p["Pu"], L.ptr(x.maskr), n, T, KP, H, cp,
                                           p["h1"], p["h2"], p["h3"], p["y"], p["pred"], None, s), "dpd_decoder_fwd_cross_keep")
    dpred = torch.zeros(rows_p, 3, **f32)
    dpred[:rows] = _cu(FC.upstream(), dev).view(rows, 3)
    stride = 0 if shared else 3 * T

    def bwd(dfv, gq, accumulate=0):
        L.check(lib.dpd_field_bwd(L.ptr(dpred), L.ptr(x.maskr), p["y"], p["h1"], p["h2"], p["h3"], L.ptr(x.cnt), L.ptr(x.ucount), L.ptr(v.start),
                                  L.ptr(v.qlist), L.ptr(v.svox), L.ptr(v.scloud), n, T, M_GRID, K_WIN, KP, H, x.cap, cp, p["dy"], p["ga"], p["gb"],
                                  p["dq"] if (shared and gq is not None) else None, None if dfv is None else p["gs"],
                                  None if dfv is None else p["dXs"], dfv, accumulate, gq, stride, s), "dpd_field_bwd")
        torch.cuda.synchronize()

    if shared:
        bufs["gq"].fill_(0.25)                                       # what an earlier chunk left
        bufs["gq2"].fill_(0.25)
    bwd(p["dfv"], p["gq"])
    g1 = bufs["ga"]
    real = torch.tensor(x.real.reshape(-1), device=dev)
    dead = ~real | (x.maskr[:rows] == 0)
    assert int(dead.sum()) > int((~real).sum()) > 0
    assert not g1[rows:].abs().max() > 0 and not g1[:rows][dead].abs().max() > 0 and float(g1.abs().max()) > 0
    gs, _, dq, _ = _slot_sum(dev, n, T, x.cnt, v, g1.contiguous(), P.view("W1p"))
    assert torch.equal(_bits(gs), _bits(bufs["gs"]))
    dXs = ops.gemm_f32(gs.contiguous(), P.transposed()[2], tile=32)
    assert torch.equal(_bits(dXs), _bits(bufs["dXs"]))
    dfv, dfv_band = G.banded((n * NG, 20), 20, **f32)
    L.check(lib.dpd_field_scatter(L.ptr(dXs), L.ptr(x.ucount), L.ptr(v.svox), n, T, M_GRID, K_WIN, KP, 0, L.ptr(dfv), s), "dpd_field_scatter")
    torch.cuda.synchronize()
    assert torch.equal(_bits(dfv), _bits(bufs["dfv"])) and float(dfv.abs().max()) > 0
    assert not dq[:rows][dead].abs().max() > 0
    if shared:
        want = torch.full((T, 3), 0.25, **f32)
        for c in range(n):
            want = want + dq[:rows].view(n, T, 3)[c]
        assert torch.equal(_bits(bufs["gq"]), _bits(want)) and torch.equal(_bits(bufs["dq"][:rows]), _bits(dq[:rows]))
    else:
        assert torch.equal(_bits(bufs["gq"]), _bits(dq[:rows])) and G.untouched(bufs["dq"])
    # each half alone
    for t in (bufs["gs"], bufs["dXs"], bufs["dq"]):
        t.view(torch.int32).fill_(G.NAN_OUT)
    bwd(None, p["gq2"])
    assert torch.equal(_bits(bufs["gq2"]), _bits(bufs["gq"])) and G.untouched(bufs["gs"]) and G.untouched(bufs["dXs"]) and G.untouched(bufs["dfv2"])
    bufs["dfv2"].fill_(1.0)
    bufs["dq"].view(torch.int32).fill_(G.NAN_OUT)
    bwd(p["dfv2"], None, accumulate=1)
    assert G.untouched(bufs["dq"]) and float((bufs["dfv2"] - 1.0 - bufs["dfv"]).abs().max()) < 1e-3 * float(bufs["dfv"].abs().max())
    assert not torch.equal(_bits(bufs["dfv2"]), _bits(bufs["dfv"]))
    bwd(p["dfv2"], None)
    assert torch.equal(_bits(bufs["dfv2"]), _bits(bufs["dfv"]))
    for b in bands:
        b()
    dfv_band(), v.bands(), x.bands()


def test_refused_calls_touch_nothing(dev):
    """the DPD_E_* paths of dpd_field_invert and dpd_field_bwd with real device buffers: the return code, and every output still the NaN
    pattern of its guard-banded buffer (tests/test_field_slots_cpu.py covers every path without a device)"""
    from dpdist_amd import lib as L
    lib, s = L.load(), L.cur_stream()
    x = TF._field("reference", False, False)
    n, T, rows_p, H, cap = x.n, x.T, x.rows_p, H_DEC, x.cap
    f32, i32 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int32, device=dev)
    outs, bands = {}, []
    for name, cnt, kw in (("start", cap + 1, i32), ("qlist", n * T, i32), ("svox", cap, i32), ("scloud", cap, i32), ("dy", rows_p * 3, f32),
                          ("ga", rows_p * H, f32), ("gb", rows_p * H, f32), ("dq", rows_p * 3, f32), ("gs", cap * H, f32), ("dXs", cap * KP, f32),
                          ("dfv", n * NG * 20, f32), ("gq", n * T * 3, f32)):
        outs[name], b = G.banded_flat(cnt, **kw)
        bands.append(b)
    o = {k: L.ptr(t) for k, t in outs.items()}
    inv = lambda vox=L.ptr(x.vox), nn=n, m=M_GRID, c=cap, out=o["scloud"]: lib.dpd_field_invert(   # noqa: E731
        vox, L.ptr(x.slot), L.ptr(x.ucount), nn, T, m, c, o["start"], o["qlist"], o["svox"], out, s)
    assert inv(vox=None) == E_NULL and inv(out=None) == E_NULL
    assert inv(nn=0) == E_DIM and inv(c=cap - 32) == E_DIM and inv(c=cap + 32) == E_DIM
    assert inv(m=11) == E_UNSUPPORTED and inv(m=0) == E_UNSUPPORTED
    P = X._params(dev)
    cp = L.make_params(*P.views(), *P.transposed())
    a = torch.zeros(rows_p, H, **f32)
    z3 = torch.zeros(rows_p, 3, **f32)

    def bwd(dpred=L.ptr(z3), dfv=o["dfv"], gq=o["gq"], gs=o["gs"], dq=o["dq"], prm=cp, nn=n, c=cap, h=H, k=K_WIN, m=M_GRID, stride=3 * T):
        return lib.dpd_field_bwd(dpred, L.ptr(x.maskr), L.ptr(z3), L.ptr(a), L.ptr(a), L.ptr(a), L.ptr(x.cnt), L.ptr(x.ucount), L.ptr(x.vox),
                                 L.ptr(x.vox), L.ptr(x.vox), L.ptr(x.vox), nn, T, m, k, KP, h, c, prm, o["dy"], o["ga"], o["gb"], dq, gs, o["dXs"],
                                 dfv, 0, gq, stride, s)
    assert bwd(dpred=None) == E_NULL and bwd(dfv=None, gq=None) == E_NULL and bwd(prm=None) == E_NULL and bwd(gs=None) == E_NULL
    assert bwd(dq=None, stride=0) == E_NULL
    assert bwd(prm=L.make_params(*P.views())) == E_NULL              # the surface route needs the transposed W1p
    assert bwd(nn=0) == E_DIM and bwd(c=cap - 32) == E_DIM and bwd(stride=3 * T - 1) == E_DIM and bwd(h=0) == E_DIM
    assert bwd(h=200) == E_UNSUPPORTED and bwd(h=4160) == E_UNSUPPORTED and bwd(k=4) == E_UNSUPPORTED and bwd(m=11) == E_UNSUPPORTED
    torch.cuda.synchronize()
    assert all(G.untouched(t.view(torch.float32)) for t in outs.values())
    for b in bands:
        b()


# ---------------------------------------------------------------------------------------------------- DPDistField(backward="slots")
def _grads(dev, shared, max_rows=4096, need=(True, True), pad=None, backward="slots"):
    from dpdist_amd import DPDistField
    s, q = TF._inputs(dev, shared, pad, need)
    pred = DPDistField(X._params(dev), max_rows=max_rows, backward=backward)(s, q, counts=FC.COUNTS, query_counts=FC.QCOUNTS)
    loss = (pred * _cu(FC.upstream(), dev)).sum()
    g = iter(torch.autograd.grad(loss, [t for t, w in zip((s, q), need) if w]))
    return pred, [next(g) if w else None for w in need]


@functools.lru_cache(maxsize=None)
def _ref(shared):
    """the gradients at max_rows = 4096 (one chunk of whole clouds), shared by the tests below (none writes into them)"""
    return _grads(torch.device("cuda:0"), shared)


def _check_oracle(shared, gS, gQ, what):
    for name, got, (ref, bar) in zip(("surfaces", "queries"), (gS, gQ), FC.grad_bars(shared)):
        err = np.abs(got.double().cpu().numpy() - ref).max()
        print("%s, shared %s: g %s vs the composed float64 oracle: %.3e (bar %.3e, max|ref| %.3e)" % (what, shared, name, err, bar, np.abs(ref).max()))
        assert np.abs(ref).max() > 20 * bar, "a reference gradient without structure makes the bar vacuous"
        assert got.shape == ref.shape and err <= bar, name


@pytest.mark.parametrize("shared", [False, True])
def test_gradients_against_the_oracle(dev, shared):
    """gradients of (upstream * pred).sum() w.r.t. surfaces and queries against float64 autograd through the composed oracle, within the
    bars of tests/field_cases.py; exact zeros on the padding and at the masked query 8; pred is bit for bit dpdist_field's, and the rows
    backward's forward"""
    from dpdist_amd import dpdist_field
    pred, (gS, gQ) = _ref(shared)
    _check_oracle(shared, gS, gQ, "one chunk")
    for c, k in enumerate(FC.COUNTS):
        assert not gS[c, k:].any() and float(gS[c, :k].abs().max()) > 0
    if not shared:
        for c, k in enumerate(FC.QCOUNTS):
            assert not gQ[c, k:].any()
        assert not gQ[:, 8].any() and float(gQ[:, :8].abs().max()) > 0
    s, q = TF._inputs(dev, shared)
    fwd = dpdist_field(X._params(dev), s, q, counts=FC.COUNTS, query_counts=FC.QCOUNTS)
    rows_pred, (gS_rows, gQ_rows) = _grads(dev, shared, backward="rows")
    assert torch.equal(_bits(pred), _bits(fwd)) and torch.equal(_bits(rows_pred), _bits(fwd))
    # the two forms differ by rounding only
    for a, b, (ref, bar) in zip((gS, gQ), (gS_rows, gQ_rows), FC.grad_bars(shared)):
        assert float((a - b).abs().max()) <= 2 * bar


@pytest.mark.parametrize("shared", [False, True])
def test_chunking_and_padding(dev, shared):
    """query gradients: bit for bit the same for max_rows in {4096, 150, 64} (own queries: a query's gradient depends on its own row only;
    a shared set: one chain in ascending cloud continued across chunks and tiles).  Surface gradients: the same bits while a cloud's
    queries fit into a chunk (4096, 150); with tiles (64: tiles at 0 / 64 / 128, query counts 97 and 1 ending inside and before tiles)
    within the oracle's bars and bitwise reproducible.  The padding values 0, 0.37, 5.0 change no bit; gradients on the padding are 0."""
    pred, (gS, gQ) = _ref(shared)
    pred2, (gS2, gQ2) = _grads(dev, shared, max_rows=150, pad=0.37)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in ((pred, pred2), (gS, gS2), (gQ, gQ2)))
    pred3, (gS3, gQ3) = _grads(dev, shared, max_rows=64, pad=5.0)
    assert torch.equal(_bits(pred3), _bits(pred)) and torch.equal(_bits(gQ3), _bits(gQ))
    _check_oracle(shared, gS3, gQ3, "tiles of 64")
    pred4, (gS4, gQ4) = _grads(dev, shared, max_rows=64, pad=0.0)
    assert torch.equal(_bits(gS4), _bits(gS3)) and torch.equal(_bits(gQ4), _bits(gQ3))
    print("shared %s: surfaces, tiles of 64 vs one chunk: %.3e" % (shared, float((gS3 - gS).abs().max())))
    for g in (gS2, gS3):
        for c, k in enumerate(FC.COUNTS):
            assert not g[c, k:].any()
    if not shared:
        for g in (gQ2, gQ3):
            for c, k in enumerate(FC.QCOUNTS):
                assert not g[c, k:].any()
            assert not g[:, 8].any()


@pytest.mark.parametrize("max_rows", [4096, 64])
@pytest.mark.parametrize("shared", [False, True])
def test_partial_gradients(dev, shared, max_rows):
    """with needs_input_grad set for one input only, that input's gradient has the same bits, and the other gets None"""
    _, (gS, gQ) = _ref(shared) if max_rows == 4096 else _grads(dev, shared, max_rows=max_rows)
    _, (gS1, none_q) = _grads(dev, shared, max_rows=max_rows, need=(True, False))
    _, (none_s, gQ1) = _grads(dev, shared, max_rows=max_rows, need=(False, True))
    assert none_q is None and none_s is None and torch.equal(_bits(gS1), _bits(gS)) and torch.equal(_bits(gQ1), _bits(gQ))


def test_more_queries_than_max_rows(dev):
    """max_rows = 149 on the 150-query reference case: the slots backward walks tiles [0, 149) and [149, 150); the default still raises"""
    from dpdist_amd import DPDistField
    _, (gS, gQ) = _grads(dev, False, max_rows=149)
    _check_oracle(False, gS, gQ, "max_rows 149")
    assert torch.equal(_bits(gQ), _bits(_ref(False)[1][1]))
    s, q = TF._inputs(dev, False, grad=(True, True))
    for mod in (DPDistField(X._params(dev), max_rows=149), DPDistField(X._params(dev), max_rows=149, backward="rows")):
        with pytest.raises(ValueError, match="max_rows"):
            mod(s, q)


def test_beyond_8192_queries(dev):
    """one cloud of 64 points at 8193 queries of its own, one chunk: the smallest shape past the rows backward's LDS limit.  Gradients
    against the float64 oracle composed as tests/field_cases.py composes it, bars formed by the same rule on this case; pred within the
    forward's bar and bit for bit dpdist_field's; backward="rows" still raises on the same input"""
    from dpdist_amd import DPDistField, dpdist_field
    P = X._params(dev)
    s, q = _cu(FS.big_surface(), dev, True), _cu(FS.big_queries(), dev, True)
    pred = DPDistField(P, backward="slots")(s, q)
    gS, gQ = torch.autograd.grad((pred * _cu(FS.big_upstream(), dev)).sum(), [s, q])
    want = FS.big_oracle_grads(torch.float64)[0]
    err = float(np.abs(pred.detach().double().cpu().numpy() - want).max())
    print("pred vs the composed float64 oracle: %.3e" % err)
    assert pred.shape == (1, FS.M_BIG, 3) and err <= FC.FWD_BAR
    assert torch.equal(_bits(pred.detach()), _bits(dpdist_field(P, s.detach(), q.detach())))
    for name, got, (ref, bar) in zip(("surface", "queries"), (gS, gQ), FS.big_grad_bars()):
        err = np.abs(got.double().cpu().numpy() - ref).max()
        print("g %s vs the composed float64 oracle: %.3e (bar %.3e, max|ref| %.3e)" % (name, err, bar, np.abs(ref).max()))
        assert np.abs(ref).max() > 20 * bar, "a reference gradient without structure makes the bar vacuous"
        assert got.shape == ref.shape and err <= bar, name
    assert not gQ[0, 8].any()
    with pytest.raises(ValueError, match="not supported by the backward"):
        DPDistField(P, backward="rows")(s, q)
    with pytest.raises(ValueError, match="not supported by the backward"):
        DPDistField(P)(s, q)


def test_constructor_and_errors_before_any_launch(dev):
    from dpdist_amd import DPDistField
    P = X._params(dev)
    with pytest.raises(ValueError, match="backward"):
        DPDistField(P, backward="nonsense")
    s, q = TF._inputs(dev, False, grad=(True, True))
    with pytest.raises(ValueError, match="one set per cloud"):
        DPDistField(P, backward="slots")(s, q[:2])
    with pytest.raises(ValueError, match="not supported by the backward"):          # the encoder backward's m <= 8
        DPDistField(P, backward="slots", Embedding_Size=1000)(s, q)

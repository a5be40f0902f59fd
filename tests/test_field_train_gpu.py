"""Decoder gradients of the per-point field (dpd_field_bwd_train; dpdist_amd.field.DPDistField(backward="slots", decoder_grad=True)).

The C entry on the entry cases of tests/field_cases.py: the eight gradients exact on integer-valued operands (against numpy and against
the row form, dpd_decoder_bwd_weights on the materialised rows), inside a rounding bound of the row form on normal operands, the hazards
of the slot form (dead columns of Xu, g3 overwritten by g1), accumulation over tiles, the routes of dpd_field_bwd bit for bit.  The module
against the float64 autograd oracle of tests/field_train_cases.py, which tests/test_field_train_cpu.py admits without a GPU: the
gradients, one optimizer step (stale derived weights cannot pass) and a ten-step fitting trajectory.  Every output of the entry sits in
a NaN-filled guard-banded buffer (tests/gemm_cases.py).
"""
import functools

import numpy as np
import pytest
import torch

from tests import field_cases as FC
from tests import field_train_cases as FT
from tests import gemm_cases as G
from tests import test_cross_gpu as X
from tests import test_field_gpu as TF
from tests import test_field_slots_gpu as TS

pytestmark = pytest.mark.gpu

M_GRID, K_WIN, H_DEC, KP, KW, NG, E = FC.M_GRID, FC.K_WIN, FC.H_DEC, FC.KP, FC.KW, FC.NG, FC.E
CASES = [c[0] for c in FC.ENTRY_CASES]
NAMES = FT.NAMES
SHAPES = dict(W1p=(KP, H_DEC), b1=(1, H_DEC), W2=(H_DEC, H_DEC), b2=(1, H_DEC), W3=(H_DEC, H_DEC), b3=(1, H_DEC), W4=(H_DEC, 3), b4=(1, 3))
E_NULL, E_DIM, E_UNSUPPORTED, E_WORKSPACE = -1, -2, -3, -4
U24 = 2.0 ** -24
_bits, _cu = X._bits, TF._cu
H = H_DEC


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible")
    from dpdist_amd import lib
    lib.load()
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------------------------------------------- the C entry
class _Operands:
    """what dpd_field_bwd_train reads of one entry case.  integer: activations, weights, upstream gradient and the q - centre columns of Xt
    are small integers chosen so that every sum of the chain and of the eight gradients stays below 2^24 (asserted from the operands);
    else the decoder of tests/test_cross_gpu.py run forward on the gathered chunk (dpd_decoder_fwd_cross_keep), normal upstream"""

    def __init__(self, dev, name, integer, shared=False, all_masked=False):
        from dpdist_amd import lib as L
        lib, s = L.load(), L.cur_stream()
        f32 = dict(dtype=torch.float32, device=dev)
        self.x = x = TF._field(name, shared, integer)
        self.v = TS._inv(name, integer) if not shared else TS._Inv(x.vox, x.slot, x.ucount, x.n, x.T)
        n, T, rows, rows_p, cap = x.n, x.T, x.rows, x.rows_p, x.cap
        self.maskr = torch.zeros_like(x.maskr) if all_masked else x.maskr      # all_masked: every query counts as outside the cube
        rng = np.random.default_rng([CASES.index(name), int(integer), 23])
        # Xu is COPIED: the entry zeroes its dead columns, and the gathered chunk is shared with other tests.  The copy keeps the NaN
        # pattern the gather left in the dead columns
        self.Xu, self.Xu_band = G.banded((KW, cap), cap, **f32)
        self.Xu.copy_(x.Xu)
        self.Xt = x.Xt.clone()
        if integer:
            self.Xt[:rows, E - KW:E + 3 - KW] = torch.tensor(G.small_int(rng, (rows, 3), KP).astype(np.float32), device=dev)
            t = lambda a: torch.tensor(np.ascontiguousarray(a).astype(np.float32), device=dev)                    # noqa: E731
            sparse = lambda shp: rng.integers(-1, 2, size=shp) * (rng.integers(0, 16, size=shp) == 0)               # noqa: E731
            W = [sparse((KP, H)), np.zeros(H), sparse((H, H)), np.zeros(H), sparse((H, H)), np.zeros(H), rng.integers(-1, 2, size=(H, 3)),
                 np.zeros(3)]
            self.W = [t(w) for w in W]
            self.wT = [self.W[2].t().contiguous(), self.W[4].t().contiguous(), self.W[0].t().contiguous()]
            self.h1, self.h2, self.h3 = (t(rng.integers(0, 3, size=(rows_p, H))) for _ in range(3))
            y = np.ones((rows_p, 3))
            y[rng.integers(0, 8, size=(rows_p, 3)) == 0] = 7.0                                                      # the clamp of relu6
            self.y = t(y)
            dpred = 3 * rng.integers(-1, 2, size=(rows_p, 3))
        else:
            P = X._params(dev)
            self.W, self.wT = P.views(), P.transposed()
            Pu, self.Pu_band = G.banded((cap, H), H, **f32)                                                         # dead rows: NaN
            self.h1, self.h2, self.h3 = (torch.empty(rows_p, H, **f32) for _ in range(3))
            self.y, pred = torch.empty(rows_p, 3, **f32), torch.empty(rows_p, 3, **f32)
            cp = L.make_params(*self.W)
            L.check(lib.dpd_decoder_fwd_cross_keep(L.ptr(x.Xu), cap, cap, L.ptr(x.Xt), L.ptr(x.uid), L.ptr(x.cnt), L.ptr(Pu), L.ptr(x.maskr), n, T, KP,
                                                   H, cp, L.ptr(self.h1), L.ptr(self.h2), L.ptr(self.h3), L.ptr(self.y), L.ptr(pred), None, s),
                    "dpd_decoder_fwd_cross_keep")
            dpred = rng.standard_normal((rows_p, 3))
        dpred[rows:] = 0.0
        self.dpred = torch.tensor(dpred.astype(np.float32), device=dev)
        self.cp = L.make_params(*self.W, *self.wT)
        # the rows the row form contracts: [column uid[r] of Xu ; Xt[r]], pad rows zero (their g1 rows are zero through the mask)
        self.X = torch.zeros(rows_p, KP, **f32)
        self.X[:rows, :KW] = x.Xu.t()[x.uid[:rows].long()]
        self.X[:rows, KW:] = self.Xt[:rows]
        torch.cuda.synchronize()
        if not integer:
            assert torch.equal(_bits(self.X[:rows]), _bits(x.X_want))      # the rows dpd_patch_rows_fwd materialises, padding as the contract

    def chain64(self):
        """dy, g3, g2, g1 [rows_p, .] of the data chain in float64 from the operands"""
        d = lambda t: t.double().cpu().numpy()                                                                      # noqa: E731
        y, mask = d(self.y), d(self.maskr)
        dy = np.where((y > 0) & (y < 6), d(self.dpred) * mask[:, None] / 3.0, 0.0)
        g3 = (dy @ d(self.W[6]).T) * (d(self.h3) > 0)
        g2 = (g3 @ d(self.W[4]).T) * (d(self.h2) > 0)
        g1 = (g2 @ d(self.W[2]).T) * (d(self.h1) > 0)
        return dy, g3, g2, g1


class _Out:
    """the outputs of one call, each in its guard band"""

    def __init__(self, dev, x):
        f32 = dict(dtype=torch.float32, device=dev)
        self.t, self.bands = {}, []
        shapes = dict(dy=(x.rows_p, 3), ga=(x.rows_p, H), gb=(x.rows_p, H), dq=(x.rows_p, 3), gs=(x.cap, H), dXs=(x.cap, KP), dfv=(x.n * NG, 20),
                      gq=((x.T if x.shared else x.n * x.T), 3))
        shapes.update(SHAPES)
        for name, shp in shapes.items():
            self.t[name], b = G.banded(shp, shp[1], **f32)
            self.bands.append(b)

    def grads(self):
        return [self.t[n] for n in NAMES]

    def check(self):
        for b in self.bands:
            b()


def _workspace(dev, x, spare=0):
    from dpdist_amd import lib as L
    nbytes = L.load().dpd_field_bwd_train_workspace_bytes(x.n, x.T, M_GRID, K_WIN, KP, H)
    assert nbytes > 0
    ws, band = G.banded_flat(nbytes // 4 + spare, dtype=torch.float32, device=dev)
    return ws, band, nbytes


def _call(op, out, ws, nbytes, surface=True, query=True, weights=True, accumulate_w=0, accumulate=0, Xu=None, **over):
    from dpdist_amd import lib as L
    lib, s = L.load(), L.cur_stream()
    x, v, o = op.x, op.v, out.t
    shared = x.shared
    a = dict(dpred=L.ptr(op.dpred), n=x.n, T=x.T, m=M_GRID, k=K_WIN, h=H, cap=x.cap, ldu=x.cap, prm=op.cp, stride=0 if shared else 3 * x.T,
             wsp=L.ptr(ws), wsb=nbytes, gs=L.ptr(o["gs"]))
    a.update(over)
    w = [L.ptr(t) for t in out.grads()] if weights else [None] * 8
    return lib.dpd_field_bwd_train(a["dpred"], L.ptr(op.maskr), L.ptr(op.y), L.ptr(op.h1), L.ptr(op.h2), L.ptr(op.h3), L.ptr(x.cnt), L.ptr(x.ucount),
                                   L.ptr(v.start), L.ptr(v.qlist), L.ptr(v.svox), L.ptr(v.scloud), L.ptr(op.Xu if Xu is None else Xu), a["ldu"],
                                   L.ptr(op.Xt), a["n"], a["T"], a["m"], a["k"], KP, a["h"], a["cap"], a["prm"], L.ptr(o["dy"]), L.ptr(o["ga"]),
                                   L.ptr(o["gb"]), L.ptr(o["dq"]) if (shared and query) else None, a["gs"], L.ptr(o["dXs"]) if surface else None,
                                   L.ptr(o["dfv"]) if surface else None, accumulate, L.ptr(o["gq"]) if query else None, a["stride"], *w,
                                   accumulate_w, a["wsp"], a["wsb"], s)


def _run(dev, op, **kw):
    from dpdist_amd import lib as L
    out = _Out(dev, op.x)
    ws, band, nbytes = _workspace(dev, op.x)
    L.check(_call(op, out, ws, nbytes, **kw), "dpd_field_bwd_train")
    torch.cuda.synchronize()
    out.check(), band(), op.Xu_band()
    return out


def _row_form(dev, op, g3, g2, g1, dy):
    """the same eight gradients composed from dpd_decoder_bwd_weights on the materialised rows X and the given gradient rows"""
    from dpdist_amd import lib as L
    lib, s = L.load(), L.cur_stream()
    rows_p = op.x.rows_p
    ws = torch.empty(lib.dpd_workspace_bytes(rows_p, KP, H, 0), dtype=torch.uint8, device=dev)
    out = {n: torch.empty(*SHAPES[n], device=dev) for n in NAMES}
    for layer, act, lda, g, kin, nout, w, b in ((1, op.X, KP, g1, KP, H, "W1p", "b1"), (2, op.h1, H, g2, H, H, "W2", "b2"),
                                                (3, op.h2, H, g3, H, H, "W3", "b3"), (4, op.h3, H, dy, H, 3, "W4", "b4")):
        L.check(lib.dpd_decoder_bwd_weights(layer, L.ptr(act), lda, L.ptr(g), rows_p, kin, nout, 0, L.ptr(out[w]), L.ptr(out[b]), L.ptr(ws),
                                            ws.numel(), None, None, s), "dpd_decoder_bwd_weights")
    torch.cuda.synchronize()
    return out


def _data_chain(dev, op):
    """dy, g3, g2, g1 of dpd_decoder_bwd_data (phases 7) in buffers of their own: g3 survives"""
    from dpdist_amd import lib as L
    lib, s = L.load(), L.cur_stream()
    rows_p = op.x.rows_p
    dy = torch.empty(rows_p, 3, device=dev)
    g3, g2, g1 = (torch.empty(rows_p, H, device=dev) for _ in range(3))
    L.check(lib.dpd_decoder_bwd_data(L.ptr(op.dpred), L.ptr(op.maskr), L.ptr(op.y), L.ptr(op.h1), L.ptr(op.h2), L.ptr(op.h3), rows_p, KP, H, op.cp,
                                     0, L.ptr(dy), L.ptr(g3), L.ptr(g2), L.ptr(g1), None, None, None, 0, None, 7, s), "dpd_decoder_bwd_data")
    torch.cuda.synchronize()
    return dy, g3, g2, g1


@pytest.mark.parametrize("integer", [True, False])
@pytest.mark.parametrize("name", CASES)
def test_weight_gradients_slot_form_against_row_form(dev, name, integer):
    """the eight gradients of one chunk.  Integer operands (every sum below 2^24, asserted): equal to numpy and to the row form,
    dpd_decoder_bwd_weights on the materialised rows.  Normal operands: layers 2 - 4 are the row form's entries on the same rows (the same
    bits: g3 was not lost to g1); dW1p and db1 within (addends + 2) 2^-24 sum |addend| per element of the row form and of float64, addends =
    the chunk's rows, the bound formed in float64 from the operands.  The pad rows E + 3 .. KP - 1 of dW1p are +0.0; two runs give the
    same bits; with only the weights wanted the bits are the same and the routes'
    buffers stay untouched; guard bands intact."""
    op = _Operands(dev, name, integer)
    x, rows = op.x, op.x.rows
    out = _run(dev, op)
    got = {n: out.t[n].double().cpu().numpy() for n in NAMES}
    assert not any(np.isnan(g).any() for g in got.values())
    dy, g3, g2, g1 = _data_chain(dev, op)
    assert torch.equal(_bits(out.t["ga"]), _bits(g1)) and torch.equal(_bits(out.t["gb"]), _bits(g2)) and torch.equal(_bits(out.t["dy"]), _bits(dy))
    row = {n: t.double().cpu().numpy() for n, t in _row_form(dev, op, g3, g2, g1, dy).items()}
    d = lambda t: t.double().cpu().numpy()                                                                          # noqa: E731
    acts = dict(W1p=(d(op.X), d(g1)), W2=(d(op.h1), d(g2)), W3=(d(op.h2), d(g3)), W4=(d(op.h3), d(dy)))
    want, mag = {}, {}
    for w, b in (("W1p", "b1"), ("W2", "b2"), ("W3", "b3"), ("W4", "b4")):
        a, g = acts[w]
        want[w], mag[w] = a.T @ g, np.abs(a).T @ np.abs(g)
        want[b], mag[b] = g.sum(0)[None], np.abs(g).sum(0)[None]
    if integer:
        ref = op.chain64()
        for mine, lib_rows in zip(ref, (dy, g3, g2, g1)):
            assert np.array_equal(mine, d(lib_rows))
        gs_mag = np.zeros((x.cap, H))
        np.add.at(gs_mag, x.uid.cpu().numpy()[:rows].astype(np.int64), np.abs(ref[3][:rows]))
        assert max(m.max() for m in mag.values()) < G.EXACT and gs_mag.max() < G.EXACT, "the integer operands are not exact at this size"
        for n in NAMES:
            assert np.array_equal(got[n], want[n]), n
            assert np.array_equal(got[n], row[n]), n + " against the row form"
        if name not in ("outside", "smallest"):                                 # (one row may be masked or clamped)
            assert all(np.abs(want[n]).max() > 0 for n in NAMES)
    else:
        for n in ("W2", "b2", "W3", "b3", "W4", "b4"):
            assert np.array_equal(got[n], row[n]), n
        for n in NAMES:
            bound = (x.rows_p + 2) * U24 * mag[n]
            e_row, e_64 = np.abs(got[n] - row[n]), np.abs(got[n] - want[n])
            print("%s %s: vs row form %.3e, vs float64 %.3e, max bound %.3e, max |ref| %.3e" % (name, n, e_row.max(), e_64.max(), bound.max(),
                                                                                              np.abs(want[n]).max()))
            assert (e_row <= bound).all() and (e_64 <= bound).all(), n
    assert not _bits(out.t["W1p"][E + 3:]).any()                                                   # the zero pad of Xt: +0.0
    if name == "reference":
        assert sum(x.U) < x.cap and not G.untouched(op.Xu[:, sum(x.U):]) and not op.Xu[:, sum(x.U):].any()    # the dead columns were zeroed
    again = _run(dev, op)
    only = _run(dev, op, surface=False, query=False)
    for n in NAMES:
        assert torch.equal(_bits(again.t[n]), _bits(out.t[n])) and torch.equal(_bits(only.t[n]), _bits(out.t[n])), n
    assert torch.equal(_bits(only.t["gs"]), _bits(out.t["gs"])) and all(G.untouched(only.t[n]) for n in ("dXs", "dfv", "gq", "dq"))
    x.bands(), op.v.bands()


@pytest.mark.parametrize("integer", [True, False])
def test_all_masked_gives_exact_zeros(dev, integer):
    """the `outside` chunk with every query masked: dy, g3, g2, g1 are zero rows, gs is zero, and every one of the eight gradients is
    exactly +0.0 -- not -0.0 and, with the dead columns of Xu holding NaN, never NaN; dfv and gq are zeros as well"""
    op = _Operands(dev, "outside", integer, all_masked=True)
    out = _run(dev, op)
    assert sum(op.x.U) < op.x.cap and float(op.dpred.abs().max()) > 0
    for n in NAMES:
        assert not _bits(out.t[n]).any(), n
    for n in ("ga", "gb", "dy", "gs", "dfv", "gq"):
        assert not out.t[n].any() and not torch.isnan(out.t[n]).any(), n


def test_dead_columns_and_dead_rows_change_no_bit(dev):
    """the reference chunk has dead slots.  The dead columns of Xu and the dead rows of Pu hold the NaN pattern of their buffers in every
    run above; here they hold zeros, then quiet NaNs: the eight gradients, dfv and gq are the same bits"""
    op = _Operands(dev, "reference", False)
    total = sum(op.x.U)
    assert 0 < total < op.x.cap and G.untouched(op.Xu[:, total:])
    base = _run(dev, op)
    for fill in (0.0, float("nan")):
        op.Xu[:, total:] = fill
        out = _run(dev, op)
        for n in NAMES + ("dfv", "gq", "gs"):
            assert torch.equal(_bits(out.t[n]), _bits(base.t[n])), (n, fill)
        assert not op.Xu[:, total:].any()
    assert not any(torch.isnan(base.t[n]).any() for n in NAMES)


@pytest.mark.parametrize("shared", [False, True])
def test_routes_are_those_of_the_frozen_backward(dev, shared):
    """dfv and gq of dpd_field_bwd_train are bit for bit those of dpd_field_bwd on the same chunk: with the weight outputs, and with all
    eight NULL (the call is then dpd_field_bwd).  A shared query set continues the value gq held"""
    from dpdist_amd import lib as L
    lib, s = L.load(), L.cur_stream()
    op = _Operands(dev, "reference", False, shared)
    x, v = op.x, op.v
    ref = _Out(dev, x)
    runs = []
    for weights in (None, True, False):
        out = ref if weights is None else _Out(dev, x)
        ws, band, nbytes = _workspace(dev, x)
        if shared:
            out.t["gq"].fill_(0.25)
        if weights is None:
            o = out.t
            L.check(lib.dpd_field_bwd(L.ptr(op.dpred), L.ptr(x.maskr), L.ptr(op.y), L.ptr(op.h1), L.ptr(op.h2), L.ptr(op.h3), L.ptr(x.cnt),
                                      L.ptr(x.ucount), L.ptr(v.start), L.ptr(v.qlist), L.ptr(v.svox), L.ptr(v.scloud), x.n, x.T, M_GRID, K_WIN, KP, H,
                                      x.cap, op.cp, L.ptr(o["dy"]), L.ptr(o["ga"]), L.ptr(o["gb"]), L.ptr(o["dq"]) if shared else None,
                                      L.ptr(o["gs"]), L.ptr(o["dXs"]), L.ptr(o["dfv"]), 0, L.ptr(o["gq"]), 0 if shared else 3 * x.T, s),
                    "dpd_field_bwd")
        else:
            L.check(_call(op, out, ws, nbytes, weights=weights), "dpd_field_bwd_train")
        torch.cuda.synchronize()
        out.check(), band()
        runs.append(out)
    for out in runs[1:]:
        for n in ("dfv", "gq", "gs", "dXs", "ga", "gb", "dy"):
            assert torch.equal(_bits(out.t[n]), _bits(ref.t[n])), n
    assert float(ref.t["dfv"].abs().max()) > 0 and float(ref.t["gq"].abs().max()) > 0
    assert all(G.untouched(runs[2].t[n]) for n in NAMES) and not any(G.untouched(runs[1].t[n]) for n in NAMES)


def test_refused_calls_touch_nothing(dev):
    """the DPD_E_* paths with real device buffers: the return code, and every output still the NaN pattern of its guard-banded buffer
    (tests/test_field_train_cpu.py covers every path without a device)"""
    from dpdist_amd import lib as L
    op = _Operands(dev, "reference", False)
    x = op.x
    out = _Out(dev, x)
    ws, band, nbytes = _workspace(dev, x)
    xu = op.Xu.clone()
    P = X._params(dev)
    call = lambda **kw: _call(op, out, ws, nbytes, **kw)                                                            # noqa: E731
    assert call(dpred=None) == E_NULL and call(gs=None) == E_NULL and call(wsp=None) == E_NULL and call(prm=None) == E_NULL
    assert call(prm=L.make_params(*P.views())) == E_NULL                       # the surface route needs the transposed W1p
    assert call(n=0) == E_DIM and call(cap=x.cap - 32) == E_DIM and call(stride=3 * x.T - 1) == E_DIM and call(ldu=x.cap - 4) == E_DIM
    assert call(h=200) == E_UNSUPPORTED and call(h=4160) == E_UNSUPPORTED and call(k=4) == E_UNSUPPORTED and call(m=11) == E_UNSUPPORTED
    assert call(ldu=x.cap + 2) == E_UNSUPPORTED
    assert call(wsb=nbytes - 1) == E_WORKSPACE and call(wsb=0) == E_WORKSPACE
    torch.cuda.synchronize()
    assert all(G.untouched(t) for t in out.t.values()) and G.untouched(ws) and torch.equal(_bits(op.Xu), _bits(xu))
    out.check(), band()


class _Tile:
    """the chunk of the reference case's three clouds at the queries [t0, t0 + T): index, gather, forward and inverted index through the
    module's own helpers (dpdist_amd.field: _Chunk, _rows), then dpd_field_bwd_train with the weights alone into `grads`"""

    def __init__(self, dev, t0, T):
        from dpdist_amd import field, lib as L
        self.lib, self.s = lib, s = L.load(), L.cur_stream()
        self.P = P = X._params(dev)
        self.cp = L.make_params(*P.views(), *P.transposed())
        S, Q = TF._inputs(dev, False)
        cS, cQ = (torch.tensor(c, dtype=torch.int32, device=dev) for c in (FC.COUNTS, FC.QCOUNTS))
        fv = field._encode(lib, s, S, M_GRID, 0.125, cS)
        self.ck = ck = field._Chunk(lib, P, 3, T, M_GRID, dev, "slots")
        field._rows(lib, s, P, self.cp, M_GRID, ck, 0, t0, fv, Q, cQ, False, True)
        L.check(lib.dpd_field_invert(L.ptr(ck.vox), L.ptr(ck.slot), L.ptr(ck.ucount), 3, T, M_GRID, ck.cap, L.ptr(ck.slot_start), L.ptr(ck.qlist),
                                     L.ptr(ck.slot_vox), L.ptr(ck.slot_cloud), s), "dpd_field_invert")
        ck.dpred[:ck.rows].copy_(_cu(FC.upstream(), dev)[:, t0:t0 + T].reshape(ck.rows, 3))
        self.ws = torch.empty(lib.dpd_field_bwd_train_workspace_bytes(3, T, M_GRID, K_WIN, KP, H), dtype=torch.uint8, device=dev)

    def run(self, grads, accumulate_w):
        from dpdist_amd import lib as L
        ck, P = self.ck, self.P
        L.check(self.lib.dpd_field_bwd_train(L.ptr(ck.dpred), L.ptr(ck.maskr), L.ptr(ck.y), L.ptr(ck.h1), L.ptr(ck.h2), L.ptr(ck.h3), L.ptr(ck.cnt),
                                             L.ptr(ck.ucount), L.ptr(ck.slot_start), L.ptr(ck.qlist), L.ptr(ck.slot_vox), L.ptr(ck.slot_cloud),
                                             L.ptr(ck.Xu), ck.cap, L.ptr(ck.Xt), 3, ck.T, M_GRID, K_WIN, KP, H, ck.cap, self.cp, L.ptr(ck.dy),
                                             L.ptr(ck.ga), L.ptr(ck.gb), None, L.ptr(ck.gs), None, None, 0, None, 3 * ck.T,
                                             *[L.ptr(g) for g in grads], accumulate_w, L.ptr(self.ws), self.ws.numel(), self.s),
                "dpd_field_bwd_train")
        torch.cuda.synchronize()


def test_accumulation_over_tiles(dev):
    """the tiles [0, 64) and [64, 150) of the reference case: with accumulate_w the outputs hold the stored gradient of the first tile plus
    the stored gradient of the second, added in that order (the chunk's contribution is formed completely first, so these are the bits
    of one fp32 addition per element); a preset gradient is continued, not overwritten; the sum lies inside the oracle's bars"""
    new = lambda: [torch.full(SHAPES[n], float("nan"), device=dev) for n in NAMES]                                  # noqa: E731
    t1, t2 = _Tile(dev, 0, 64), _Tile(dev, 64, 86)
    g1, g2, acc = new(), new(), new()
    t1.run(g1, 0)
    t2.run(g2, 0)
    t1.run(acc, 0)
    t2.run(acc, 1)
    for n, a, b, c in zip(NAMES, g1, g2, acc):
        assert torch.equal(_bits(c), _bits(a + b)) and not torch.isnan(c).any() and float(b.abs().max()) > 0, n
    for n, got in zip(NAMES, acc):
        ref, bar = FT.weight_bars(False)[n]
        err = np.abs(got.double().cpu().numpy().reshape(ref.shape) - ref).max()
        print("two tiles, %s vs the float64 oracle: %.3e (bar %.3e)" % (n, err, bar))
        assert err <= bar, n
    rng = np.random.default_rng(31)
    preset = [torch.tensor(rng.standard_normal(SHAPES[n]).astype(np.float32), device=dev) for n in NAMES]
    acc = [p.clone() for p in preset]
    t1.run(acc, 1)
    for n, p, a, c in zip(NAMES, preset, g1, acc):
        assert torch.equal(_bits(c), _bits(p + a)), n


# ------------------------------------------------------------------------------------------------ DPDistField(decoder_grad=True)
def _module_grads(dev, shared, max_rows=4096, need=(True, True, True), pad=None, P=None):
    """-> (pred, [gS, gQ, gW as name -> block]) of (upstream * pred).sum(); an input that needs no gradient gets None"""
    from dpdist_amd import DPDistField
    P = X._params(dev) if P is None else P
    P.flat.requires_grad_(need[2])
    P.flat.grad = None
    s, q = TF._inputs(dev, shared, pad, need[:2])
    pred = DPDistField(P, max_rows=max_rows, backward="slots", decoder_grad=True)(s, q, counts=FC.COUNTS, query_counts=FC.QCOUNTS)
    (pred * _cu(FC.upstream(), dev)).sum().backward()
    return pred.detach(), [s.grad, q.grad, None if P.flat.grad is None else P.flat.grad.clone()], P


@functools.lru_cache(maxsize=None)
def _mref(shared):
    """the gradients at max_rows = 4096 (one chunk of whole clouds), shared by the tests below (none writes into them)"""
    return _module_grads(torch.device("cuda:0"), shared)


def _check_weights(P, flat_grad, shared, what, bars=None):
    bars = FT.weight_bars(shared) if bars is None else bars
    for n in NAMES:
        ref, bar = bars[n]
        got = P.view(n, flat_grad).double().cpu().numpy()
        err = np.abs(got - ref).max()
        print("%s, shared %s: g %s vs the float64 oracle: %.3e (bar %.3e, max|ref| %.3e)" % (what, shared, n, err, bar, np.abs(ref).max()))
        assert np.abs(ref).max() > 20 * bar, "a reference gradient without structure makes the bar vacuous"
        assert got.shape == ref.shape and err <= bar, n


@pytest.mark.parametrize("shared", [False, True])
def test_module_gradients_against_the_oracle(dev, shared):
    """all eight decoder gradients within the bars of tests/field_train_cases.py (own and shared queries); the alignment gaps of the flat
    gradient are exact zeros; P.tf_state_dict gives it under the TF names; gS and gQ are torch.equal to the frozen backward="slots"
    node's; pred is torch.equal to dpdist_field's"""
    from dpdist_amd import dpdist_field
    pred, (gS, gQ, gW), P = _mref(shared)
    _check_weights(P, gW, shared, "one chunk")
    used = torch.zeros_like(gW, dtype=torch.bool)
    for n in NAMES:
        off, cnt, _ = P._segments[n]
        used[off:off + cnt] = True
    assert int((~used).sum()) == 1 and not _bits(gW[~used]).any() and not _bits(P.view("W1p", gW)[E + 3:]).any()
    sd = P.tf_state_dict(gW)
    want = FT.oracle_weight_grads(torch.float64, shared)
    w1 = sd[FT.TF_NAME % (1, "weights")].reshape(E + 3, H)
    assert np.abs(w1[:3] - want["W1p"][E:E + 3]).max() <= FT.weight_bars(shared)["W1p"][1] and np.abs(w1[:3]).max() > 0
    _, (gS0, gQ0) = TS._ref(shared)
    assert torch.equal(gS, gS0) and torch.equal(gQ, gQ0)
    s, q = TF._inputs(dev, shared)
    assert torch.equal(pred, dpdist_field(X._params(dev), s, q, counts=FC.COUNTS, query_counts=FC.QCOUNTS))


@pytest.mark.parametrize("shared", [False, True])
def test_module_chunking_and_padding(dev, shared):
    """max_rows in {4096, 150, 64} with padding 0 / 0.37 / 5.0: every plan inside the oracle's bars; the padding changes no bit at a fixed
    max_rows; two runs give the same bits; gQ never depends on max_rows, gS and gQ stay those of the frozen node at the same max_rows"""
    pred, (gS, gQ, gW), P = _mref(shared)
    for max_rows, pads in ((4096, (0.0,)), (150, (0.37, 5.0)), (64, (5.0, 0.0, 5.0))):
        first = None
        for pad in pads:
            p2, (s2, q2, w2), _ = _module_grads(dev, shared, max_rows=max_rows, pad=pad)
            _check_weights(P, w2, shared, "max_rows %d, padding %s" % (max_rows, pad))
            assert torch.equal(_bits(p2), _bits(pred)) and torch.equal(_bits(q2), _bits(gQ))
            if first is None:
                first = (s2, w2)
                print("max_rows %d vs 4096: weights differ by %.3e" % (max_rows, float((w2 - gW).abs().max())))
            assert torch.equal(_bits(s2), _bits(first[0])) and torch.equal(_bits(w2), _bits(first[1])), (max_rows, pad)
        _, (s0, q0) = TS._grads(dev, shared, max_rows=max_rows)
        assert torch.equal(_bits(first[0]), _bits(s0)) and torch.equal(_bits(q2), _bits(q0))
        if max_rows == 4096:
            assert torch.equal(_bits(first[1]), _bits(gW))


@pytest.mark.parametrize("max_rows", [4096, 64])
def test_module_partial_needs(dev, max_rows):
    """only the decoder, decoder + queries, decoder + surfaces: what is computed has the same bits, the rest is None"""
    _, (gS, gQ, gW), _ = _mref(False) if max_rows == 4096 else _module_grads(dev, False, max_rows=max_rows)
    for need in ((False, False, True), (False, True, True), (True, False, True), (True, True, False)):
        _, got, _ = _module_grads(dev, False, max_rows=max_rows, need=need)
        for want, g, w in zip((gS, gQ, gW), got, need):
            assert (g is None) if not w else torch.equal(_bits(g), _bits(want)), need


def _tf_numpy(P):
    return {k: np.asarray(v) for k, v in P.tf_state_dict().items()}


def test_one_optimizer_step_uses_the_new_weights(dev):
    """one TFAdam step at lr = 0.05 moves the weights through raw pointers (no version bump).  The gradients of the next backward lie
    within the bars the oracle forms AT THE LIBRARY'S OWN UPDATED WEIGHTS, while the oracle's gradients there differ from the pre-step
    ones by far more than the bars: a stale transposed copy cannot pass.  The forward after the step is dpdist_field's on the same
    parameters"""
    from dpdist_amd import DPDistField, dpdist_field
    from dpdist_amd.optim import TFAdam
    P = X._params(dev)
    opt = TFAdam([P.flat], lr=0.05)
    mod = DPDistField(P, backward="slots", decoder_grad=True)
    s, q = TF._inputs(dev, False)
    up = _cu(FC.upstream(), dev)
    (mod(s, q, counts=FC.COUNTS, query_counts=FC.QCOUNTS) * up).sum().backward()
    _check_weights(P, P.flat.grad, False, "before the step")
    opt.step()
    opt.zero_grad()
    new = _tf_numpy(P)
    bars = FT.weight_bars(False, new)
    old = FT.oracle_weight_grads(torch.float64, False)
    for n in NAMES:
        moved = np.abs(bars[n][0] - old[n]).max()
        print("%s: the oracle's gradient moved by %.3g (bar %.3g)" % (n, moved, bars[n][1]))
        assert moved > 20 * bars[n][1], n
    pred = mod(s, q, counts=FC.COUNTS, query_counts=FC.QCOUNTS)
    (pred * up).sum().backward()
    _check_weights(P, P.flat.grad, False, "after the step", bars)
    assert torch.equal(pred.detach(), dpdist_field(P, s, q, counts=FC.COUNTS, query_counts=FC.QCOUNTS))


def test_fitting_trajectory(dev):
    """ten TFAdam steps at lr = 1e-4 on mean |pred[..., 0] - label| over the 248 real queries, labels = the float64 nearest distance to
    the truncated cloud: every loss within FWD_BAR of the float64 oracle's trajectory under oracle.restate.adam_tf_step, which falls by
    at least 0.006 per step (tests/test_field_train_cpu.py)"""
    from dpdist_amd import DPDistField
    from dpdist_amd.optim import TFAdam
    want = FT.trajectory(torch.float64)
    P = X._params(dev)
    opt = TFAdam([P.flat], lr=FT.LR)
    mod = DPDistField(P, backward="slots", decoder_grad=True)
    s, q = TF._inputs(dev, False)
    lab, real = (_cu(a, dev) for a in FT.labels_padded())
    got = []
    for _ in range(FT.STEPS):
        opt.zero_grad()
        pred = mod(s, q, counts=FC.COUNTS, query_counts=FC.QCOUNTS)
        loss = ((pred[..., 0] - lab).abs() * real).sum() / FT.N_REAL
        loss.backward()
        opt.step()
        got.append(float(loss.detach()))
    print("library", ["%.5f" % v for v in got])
    print("oracle ", ["%.5f" % v for v in want])
    print("max distance %.3e" % max(abs(a - b) for a, b in zip(got, want)))
    assert all(abs(a - b) <= FC.FWD_BAR for a, b in zip(got, want))
    assert all(a - b >= 0.006 for a, b in zip(want, want[1:]))

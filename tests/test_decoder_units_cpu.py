"""Host logic of the decoder's translation units (dpdist_amd/csrc/decoder*.hip): the code every backward and all-pairs entry returns for
an argument set it refuses, the process-wide GEMM plan as seen from the backward unit, and the source list of the build.

Every call here is refused by argument validation, which dereferences none of the placeholder pointers.  A library that got a check
wrong could fall through to a launch on those pointers, so the module does not run where a GPU is visible."""
import os

import pytest
import torch

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="placeholder device pointers: host validation only, not for a machine with a GPU")

E_NULL, E_DIM, E_UNSUPPORTED, E_WORKSPACE = -1, -2, -3, -4
P = 1 << 30                      # any 256-byte aligned "device address": validation never dereferences it
QB, KP, H = 64, 96, 64


@pytest.fixture(scope="module")
def lib():
    from dpdist_amd import build, lib as L
    build.build(verbose=False)
    return L.load()


def params(**kw):
    """All eight weights non-null, no transposed copies; kw overrides (None = NULL)."""
    from dpdist_amd import lib as L
    p = L.DecoderParams()
    for n in ("W1p", "b1", "W2", "b2", "W3", "b3", "W4", "b4"):
        setattr(p, n, P)
    for n, v in kw.items():
        setattr(p, n, v)
    return p


def small_grads(**kw):
    from dpdist_amd import lib as L
    sg = L.SmallGrads()
    for n, v in kw.items():
        setattr(sg, n, v)
    return sg


def planes(np_, Q=2 * QB, Qb=QB, **kw):
    from dpdist_amd import lib as L
    pl = L.Planes()
    pl.np, pl.Q, pl.Qb = np_, Q, Qb
    for n, v in kw.items():
        setattr(pl, n, v)
    return pl


def live_rows(zeroed=False, **kw):
    """A descriptor as dpd_live_rows_carve leaves it for (QB, KP, H), or all zero; kw overrides."""
    from dpdist_amd import lib as L
    lv = L.LiveRows()
    if not zeroed:
        lv.Qb, lv.KP, lv.H = QB, KP, H
        for n in ("cnt", "idx", "pos", "rowflag", "g3c", "h1c", "h2c", "Xc"):
            setattr(lv, n, P)
    for n, v in kw.items():
        setattr(lv, n, v)
    return lv


T = dict(W2T=P, W3T=P)           # the transposed weight copies the live entries want


def data_live(lib, **kw):
    a = dict(dpred=P, mask=P, y=P, h1=P, h2=P, h3=P, Qb=QB, KP=KP, H=H, p=params(), dtype=0, dy=P, g3=P, g2=P, g1=P, dX=None, sg=None,
             ws=None, ws_bytes=0, pl=None, phases=1, live=None)
    a.update(kw)
    return lib.dpd_decoder_bwd_data_live(a["dpred"], a["mask"], a["y"], a["h1"], a["h2"], a["h3"], a["Qb"], a["KP"], a["H"], a["p"], a["dtype"],
                                         a["dy"], a["g3"], a["g2"], a["g1"], a["dX"], a["sg"], a["ws"], a["ws_bytes"], a["pl"], a["phases"],
                                         a["live"], None)


def weights_live(lib, **kw):
    a = dict(layer=2, act=P, lda=H, g=P, Qb=QB, Kin=H, Nout=H, dtype=0, dW=P, db=None, ws=None, ws_bytes=0, pl=None, db_partials=None, live=None)
    a.update(kw)
    return lib.dpd_decoder_bwd_weights_live(a["layer"], a["act"], a["lda"], a["g"], a["Qb"], a["Kin"], a["Nout"], a["dtype"], a["dW"], a["db"],
                                            a["ws"], a["ws_bytes"], a["pl"], a["db_partials"], a["live"], None)


def weights_pair_live(lib, **kw):
    a = dict(actA=P, gA=P, dWA=P, actB=P, gB=P, dWB=P, lda=H, Qb=QB, Kin=H, Nout=H, dtype=0, ws=None, ws_bytes=0, pl=None, dbA=None,
             db_partials=None, live=None)
    a.update(kw)
    return lib.dpd_decoder_bwd_weights_pair_live(a["actA"], a["gA"], a["dWA"], a["actB"], a["gB"], a["dWB"], a["lda"], a["Qb"], a["Kin"], a["Nout"],
                                                 a["dtype"], a["ws"], a["ws_bytes"], a["pl"], a["dbA"], a["db_partials"], a["live"], None)


def weights_trio(lib, **kw):
    a = dict(Qb=QB, KP=KP, H=H, dtype=1, dW1=P, dW2=P, dW3=P, ws=None, ws_bytes=0, pl=planes(3))
    a.update(kw)
    return lib.dpd_decoder_bwd_weights_trio(a["Qb"], a["KP"], a["H"], a["dtype"], a["dW1"], a["dW2"], a["dW3"], a["ws"], a["ws_bytes"], a["pl"], None)


def pair_live(lib, **kw):
    a = dict(layer=3, g_in=P, g_out=P, dW=P, Qb=QB, H=H, p=params(**T), live=live_rows())
    a.update(kw)
    return lib.dpd_decoder_bwd_pair_live(a["layer"], a["g_in"], a["g_out"], a["dW"], a["Qb"], a["H"], a["p"], a["live"], None)


def chain_live(lib, **kw):
    a = dict(dpred=P, mask=P, y=P, h1=P, h2=P, h3=P, Qb=QB, KP=KP, H=H, p=params(**T), dy=P, g3=P, g2=P, g1=P, sg=None, ws=None, ws_bytes=0,
             defer_small=0, dW1=P, dW2=P, dW3=P, db1=None, db2=None, live=live_rows())
    a.update(kw)
    return lib.dpd_decoder_bwd_chain_live(a["dpred"], a["mask"], a["y"], a["h1"], a["h2"], a["h3"], a["Qb"], a["KP"], a["H"], a["p"], a["dy"], a["g3"],
                                          a["g2"], a["g1"], a["sg"], a["ws"], a["ws_bytes"], a["defer_small"], a["dW1"], a["dW2"], a["dW3"],
                                          a["db1"], a["db2"], a["live"], None)


def fwd_cross(lib, **kw):
    a = dict(Xu=P, ldu=64, slot_cap=64, Xt=P, uid=P, cnt=P, Pu=P, maskr=P, pairs=4, N=16, KP=KP, H=H, p=params(), act0=P, act1=P, y=P, pred=P, Dd=P)
    a.update(kw)
    return lib.dpd_decoder_fwd_cross(a["Xu"], a["ldu"], a["slot_cap"], a["Xt"], a["uid"], a["cnt"], a["Pu"], a["maskr"], a["pairs"], a["N"], a["KP"],
                                     a["H"], a["p"], a["act0"], a["act1"], a["y"], a["pred"], a["Dd"], None)


def fwd_cross_keep(lib, **kw):
    a = dict(Xu=P, ldu=64, slot_cap=64, Xt=P, uid=P, cnt=P, Pu=P, maskr=P, pairs=4, N=16, KP=KP, H=H, p=params(), h1=P, h2=P + 4096, h3=P + 8192,
             y=P, pred=P, Dd=P)
    a.update(kw)
    return lib.dpd_decoder_fwd_cross_keep(a["Xu"], a["ldu"], a["slot_cap"], a["Xt"], a["uid"], a["cnt"], a["Pu"], a["maskr"], a["pairs"], a["N"],
                                          a["KP"], a["H"], a["p"], a["h1"], a["h2"], a["h3"], a["y"], a["pred"], a["Dd"], None)


# (entry, what the set shows, overrides as a callable so that every case builds its own structs, the code recorded at the commit before
# the decoder was split into units).  "A before B": both checks would fire, A's code is the one returned.
CASES = [
    (data_live, "phases 0", lambda: dict(phases=0), E_DIM),
    (data_live, "phases 32", lambda: dict(phases=32), E_DIM),
    (data_live, "phases before the NULL checks", lambda: dict(phases=0, p=None), E_DIM),
    (data_live, "no parameters", lambda: dict(p=None), E_NULL),
    (data_live, "no g2 and no planes", lambda: dict(g2=None), E_NULL),
    (data_live, "labels without l1_pred", lambda: dict(sg=small_grads(l1_labels=P)), E_NULL),
    (data_live, "Qb 0", lambda: dict(Qb=0), E_DIM),
    (data_live, "dimensions before shapes", lambda: dict(Qb=0, H=48), E_DIM),
    (data_live, "H = 48", lambda: dict(H=48), E_UNSUPPORTED),
    (data_live, "dtype 3", lambda: dict(dtype=3), E_UNSUPPORTED),
    (data_live, "dtype 1 with no workspace", lambda: dict(dtype=1), E_WORKSPACE),
    (data_live, "planes of another compute type", lambda: dict(dtype=1, pl=planes(1)), E_DIM),
    (data_live, "planes of another Qb", lambda: dict(dtype=1, pl=planes(3, Qb=32)), E_DIM),
    (data_live, "fused loss at an H the fused kernel does not take", lambda: dict(sg=small_grads(l1_labels=P, l1_pred=P, l1_loss=P)), E_UNSUPPORTED),
    (data_live, "deferred reduction without sg->partials", lambda: dict(phases=17), E_NULL),
    (data_live, "no g3 and no planes", lambda: dict(g3=None), E_NULL),
    (data_live, "live: a zeroed descriptor and no W3T (the weights before check_live)", lambda: dict(live=live_rows(zeroed=True)), E_UNSUPPORTED),
    (data_live, "live: a zeroed descriptor", lambda: dict(p=params(**T), live=live_rows(zeroed=True)), E_NULL),
    (data_live, "live: db1 without db_partials before check_live", lambda: dict(p=params(**T), sg=small_grads(db1=P), live=live_rows(zeroed=True)), E_UNSUPPORTED),
    (data_live, "live: phase 8 before the missing sg->partials", lambda: dict(p=params(**T), phases=9, live=live_rows()), E_UNSUPPORTED),
    (data_live, "live: the shape checks before the live ones", lambda: dict(Qb=0, live=live_rows(zeroed=True)), E_DIM),
    (data_live, "live: descriptor of another Qb", lambda: dict(p=params(**T), live=live_rows(Qb=32)), E_DIM),
    (data_live, "live: descriptor of another H", lambda: dict(p=params(**T), live=live_rows(H=128)), E_DIM),
    (data_live, "live: descriptor of another KP", lambda: dict(p=params(**T), live=live_rows(KP=128)), E_DIM),
    (weights_live, "layer 5", lambda: dict(layer=5), E_DIM),
    (weights_live, "lda < Kin", lambda: dict(lda=H - 4), E_DIM),
    (weights_live, "Nout = 62", lambda: dict(Nout=62), E_UNSUPPORTED),
    (weights_live, "layer 4 with Nout 4", lambda: dict(layer=4, db=P, Nout=4), E_DIM),
    (weights_live, "layer 4 without a workspace", lambda: dict(layer=4, db=P, Nout=3), E_WORKSPACE),
    (weights_live, "db without a workspace", lambda: dict(db=P), E_WORKSPACE),
    (weights_live, "live: no dW", lambda: dict(dW=None, layer=5, live=live_rows(zeroed=True)), E_NULL),
    (weights_live, "live: layer 5 before check_live", lambda: dict(layer=5, live=live_rows(zeroed=True)), E_DIM),
    (weights_live, "live: db without db_partials before check_live", lambda: dict(db=P, live=live_rows(zeroed=True)), E_UNSUPPORTED),
    (weights_live, "live: layer 3 with db", lambda: dict(layer=3, db=P, db_partials=P, live=live_rows()), E_UNSUPPORTED),
    (weights_live, "live: dtype 1", lambda: dict(dtype=1, live=live_rows()), E_UNSUPPORTED),
    (weights_live, "live: a zeroed descriptor", lambda: dict(live=live_rows(zeroed=True)), E_NULL),
    (weights_live, "live: descriptor of another Qb", lambda: dict(live=live_rows(Qb=128)), E_DIM),
    (weights_live, "live: layer 1, descriptor of another KP", lambda: dict(layer=1, Kin=KP, live=live_rows(KP=128)), E_DIM),
    (weights_live, "live: layer 2 with Kin != H", lambda: dict(Kin=32, live=live_rows()), E_DIM),
    (weights_pair_live, "Qb = 33", lambda: dict(Qb=33), E_UNSUPPORTED),
    (weights_pair_live, "no dWB", lambda: dict(dWB=None), E_NULL),
    (weights_pair_live, "lda < Kin before the shapes", lambda: dict(lda=H - 4, Qb=33), E_DIM),
    (weights_pair_live, "dtype 1 with dbA", lambda: dict(dtype=1, dbA=P), E_UNSUPPORTED),
    (weights_pair_live, "dtype 1 without workspace or planes", lambda: dict(dtype=1), E_WORKSPACE),
    (weights_pair_live, "dbA without db_partials", lambda: dict(dbA=P), E_UNSUPPORTED),
    (weights_pair_live, "live: no gA", lambda: dict(gA=None, live=live_rows()), E_NULL),
    (weights_pair_live, "live: dbA without db_partials before check_live", lambda: dict(dbA=P, live=live_rows(zeroed=True)), E_UNSUPPORTED),
    (weights_pair_live, "live: a zeroed descriptor", lambda: dict(live=live_rows(zeroed=True)), E_NULL),
    (weights_pair_live, "live: descriptor of another H", lambda: dict(live=live_rows(H=128)), E_DIM),
    (weights_pair_live, "live: Kin != H", lambda: dict(Kin=32, live=live_rows()), E_DIM),
    (weights_trio, "dtype 0", lambda: dict(dtype=0), E_UNSUPPORTED),
    (weights_trio, "no planes", lambda: dict(pl=None), E_NULL),
    (weights_trio, "dimensions before the compute type", lambda: dict(Qb=0, dtype=0), E_DIM),
    (weights_trio, "shapes the planes do not take", lambda: dict(H=72), E_UNSUPPORTED),
    (weights_trio, "planes of another Qb", lambda: dict(pl=planes(3, Qb=32)), E_DIM),
    (weights_trio, "planes of another compute type", lambda: dict(pl=planes(1)), E_DIM),
    (weights_trio, "planes without the R8 operands", lambda: dict(), E_UNSUPPORTED),
    (pair_live, "layer 1", lambda: dict(layer=1), E_DIM),
    (pair_live, "layer 2 without g_in", lambda: dict(layer=2, g_in=None), E_NULL),
    (pair_live, "no W2T before check_live", lambda: dict(p=params(W3T=P), live=live_rows(zeroed=True)), E_UNSUPPORTED),
    (pair_live, "a zeroed descriptor", lambda: dict(live=live_rows(zeroed=True)), E_NULL),
    (pair_live, "descriptor of another H", lambda: dict(live=live_rows(H=128)), E_DIM),
    (pair_live, "Qb = 16", lambda: dict(Qb=16, live=live_rows(Qb=16)), E_UNSUPPORTED),
    (chain_live, "no descriptor", lambda: dict(live=None), E_NULL),
    (chain_live, "sg->db1 set", lambda: dict(sg=small_grads(db1=P, db_partials=P)), E_UNSUPPORTED),
    (chain_live, "db1 without sg->db_partials", lambda: dict(db1=P), E_UNSUPPORTED),
    (chain_live, "H = 48 (left to bwd_data_live)", lambda: dict(H=48, live=live_rows(zeroed=True)), E_UNSUPPORTED),
    (chain_live, "Qb 0 (left to bwd_data_live)", lambda: dict(Qb=0), E_DIM),
    (chain_live, "no W3T (left to bwd_data_live)", lambda: dict(p=params(W2T=P)), E_UNSUPPORTED),
    (chain_live, "a zeroed descriptor", lambda: dict(live=live_rows(zeroed=True)), E_NULL),
    (chain_live, "descriptor of another KP", lambda: dict(live=live_rows(KP=128)), E_DIM),
    (fwd_cross, "no Dd", lambda: dict(Dd=None), E_NULL),
    (fwd_cross, "no W4 before the dimensions", lambda: dict(pairs=0, p=params(W4=None)), E_NULL),
    (fwd_cross, "pairs 0", lambda: dict(pairs=0), E_DIM),
    (fwd_cross, "ldu < slot_cap before the shapes", lambda: dict(ldu=60, KP=32), E_DIM),
    (fwd_cross, "KP = 32", lambda: dict(KP=32), E_UNSUPPORTED),
    (fwd_cross, "slot_cap = 6", lambda: dict(slot_cap=6, ldu=8), E_UNSUPPORTED),
    (fwd_cross_keep, "no y", lambda: dict(y=None), E_NULL),
    (fwd_cross_keep, "h1 == h2", lambda: dict(h2=P), E_DIM),
    (fwd_cross_keep, "aliased activations before the weights", lambda: dict(h3=P, p=params(W4=None)), E_DIM),
    (fwd_cross_keep, "no b3", lambda: dict(p=params(b3=None)), E_NULL),
    (fwd_cross_keep, "N 0", lambda: dict(N=0), E_DIM),
    (fwd_cross_keep, "H = 48", lambda: dict(H=48), E_UNSUPPORTED),
    (fwd_cross_keep, "ldu = 66", lambda: dict(ldu=66), E_UNSUPPORTED),
]


@pytest.mark.parametrize("entry,what,overrides,code", CASES, ids=["%s: %s" % (c[0].__name__, c[1]) for c in CASES])
def test_refusal_codes(lib, entry, what, overrides, code):
    assert entry(lib, **overrides()) == code, what


def test_gemm_plan_reaches_the_backward_unit(lib):
    """dpd_set_gemm_plan writes the plan in one unit and the dense backward reads it in another: with the register-streamed kernel taken
    away from the NN dH products (op 6 on tile 8), the two-step bias gradients (sg->db_partials) are refused.  A unit with a private copy
    of the plan would go on with tile 32."""
    try:
        assert lib.dpd_set_gemm_plan(6, 8, 1) == 0
        assert data_live(lib, phases=2, p=params(**T), sg=small_grads(db_partials=P)) == E_UNSUPPORTED
    finally:
        assert lib.dpd_set_gemm_plan(6, 32, 1) == 0


def test_source_lists_agree():
    from dpdist_amd import build
    on_disk = sorted(f for f in os.listdir(build.CSRC) if f.endswith(".hip"))
    assert sorted(build.SOURCES) == on_disk
    assert len(set(build.SOURCES)) == len(build.SOURCES)

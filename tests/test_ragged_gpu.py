"""Ragged sets on the GPU (tests/ragged_cases.py): the per-cloud-count encoder entries bit for bit the tiled entries on each cloud alone,
the counted index / pair mean / upstream spread against the un-counted entries and float64, and the countsA / countsB keywords of
dpdist_matrix / DPDistMatrix against the composed float64 oracle.  Bars and checkers are those of tests/mfv_cases.py,
tests/test_cross_gpu.py and tests/test_cross_grad_gpu.py; every output and workspace of a new entry sits in a NaN-payload guard band.
"""
import numpy as np
import pytest
import torch

from tests import gemm_cases as G
from tests import mfv_cases as M
from tests import mfv_tiled_cases as T
from tests import ragged_cases as RC
from tests import test_cross_gpu as X
from tests import test_cross_grad_gpu as XG

pytestmark = pytest.mark.gpu

S0 = M.S0
M_GRID, K_WIN, H_DEC, KP, NG = X.M_GRID, X.K_WIN, X.H_DEC, X.KP, X.NG
_bits = X._bits


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible")
    from dpdist_amd import lib
    lib.load()
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------------------ the encoder entries
_ID = lambda c: "C%d-N%d-m%d" % (c.C, c.N, c.m)      # noqa: E731


@pytest.mark.parametrize("case", RC.ENC_CASES, ids=_ID)
def test_forward_counts_is_the_tiled_entry_on_each_cloud_alone(dev, case):
    """cloud c of dpd_mfv3d_fwd_counts == dpd_mfv3d_fwd_tiled on [1, n, 3] at the same tile, bit for bit, and within check_forward of the
    float64 oracle; the input padding holds the NaN payload (never read); the same call twice gives the same bits"""
    pts, counts = RC.nan_padded(case, dev), RC.counts_dev(case.counts, dev)
    rc, fv, band = RC.gpu_forward_counts(pts, counts, case.m, S0, case.tile)
    assert rc == 0
    rc2, fv2, band2 = RC.gpu_forward_counts(pts, counts, case.m, S0, case.tile)
    assert rc2 == 0 and torch.equal(_bits(fv), _bits(fv2))
    band2()
    for c, n in enumerate(case.counts):
        alone = torch.tensor(RC.cloud(case, c), device=dev)
        rca, fva, banda = T.gpu_forward_tiled(alone, case.m, S0, case.tile)
        assert rca == 0 and torch.equal(_bits(fv[c:c + 1]), _bits(fva)), (c, n)
        banda()
        M.check_forward(fv[c:c + 1], band, RC.enc_forward_ref(case, c), case.m, (_ID(case), "cloud %d of %d points" % (c, n)))


@pytest.mark.parametrize("case", [c for c in RC.ENC_CASES if c.backward], ids=_ID)
def test_backward_counts_is_the_tiled_entry_on_each_cloud_alone(dev, case):
    """cloud c of dpd_mfv3d_bwd_counts == dpd_mfv3d_bwd_tiled on [1, n, 3] at the same tile, bit for bit, and within check_backward of
    float64 autograd; the padded rows of dpts are +0.0 by bits; dpts and the workspace stay inside their guard bands; twice the same bits"""
    pts, counts = RC.nan_padded(case, dev), RC.counts_dev(case.counts, dev)
    G3 = case.m ** 3
    dfv = torch.empty(case.C, G3, M.F, device=dev)
    for c in range(case.C):
        dfv[c] = torch.tensor(RC.enc_backward_ref(case, c).dfv[0], device=dev)
    rc, dpts, bands = RC.gpu_backward_counts(pts, counts, dfv, case.m, S0, case.tile)
    assert rc == 0
    rc2, dpts2, bands2 = RC.gpu_backward_counts(pts, counts, dfv, case.m, S0, case.tile)
    assert rc2 == 0 and torch.equal(_bits(dpts), _bits(dpts2))
    bands2()
    for c, n in enumerate(case.counts):
        alone = torch.tensor(RC.cloud(case, c), device=dev)
        rca, ga, bandsa, _ = T.gpu_backward_tiled(alone, dfv[c:c + 1].contiguous(), case.m, S0, case.tile)
        assert rca == 0 and torch.equal(_bits(dpts[c:c + 1, :n]), _bits(ga)), (c, n)
        bandsa()
        assert not _bits(dpts[c, n:]).any(), "the padded rows are +0.0"
        M.check_backward(dpts[c:c + 1, :n], bands, RC.enc_backward_ref(case, c), (_ID(case), "cloud %d of %d points" % (c, n)))


def test_counts_out_of_range_are_clamped(dev):
    """a device count of 0 or beyond N cannot be refused (the host reads no device word): it is clamped into [1, N]"""
    case = RC.ENC_CASES[0]
    pts = torch.tensor(RC.enc_points(case), device=dev)
    _, want, _ = RC.gpu_forward_counts(pts, RC.counts_dev((24, 24, 1, 1), dev), case.m, S0, case.tile)
    rc, got, band = RC.gpu_forward_counts(pts, RC.counts_dev((1 << 30, 25, 0, -7), dev), case.m, S0, case.tile)
    assert rc == 0 and torch.equal(_bits(got), _bits(want))
    band()


# ------------------------------------------------------------------------------------------------------------ the cross entries
SHAPE = X.SHAPES[0]                                               # (Ca, Cb, N) = (3, 2, 64)


class _Index:
    """dpd_cross_index_counts into guard-banded buffers"""

    def __init__(self, dev, q, counts, Cb, N):
        from dpdist_amd import lib as L
        lib, s = L.load(), L.cur_stream()
        f32, i32 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int32, device=dev)
        self.mask, b0 = G.banded_flat(Cb * N, **f32)
        self.vox, b1 = G.banded_flat(Cb * N, **i32)
        self.slot, b2 = G.banded_flat(NG, **i32)
        self.ucount, b3 = G.banded_flat(1, **i32)
        self._bands = (b0, b1, b2, b3)
        L.check(lib.dpd_cross_index_counts(L.ptr(q), L.ptr(counts), Cb, N, M_GRID, L.ptr(self.mask), L.ptr(self.vox), L.ptr(self.slot),
                                           L.ptr(self.ucount), s), "dpd_cross_index_counts")
        torch.cuda.synchronize()

    def bands(self):
        for b in self._bands:
            b()


@pytest.mark.parametrize("kind", ["random", "outside"])
def test_index_counts(dev, kind):
    """counts all N: the bits of dpd_cross_index.  counts (64, 20): a padded query is a query outside the cube -- mask 0, voxel 0, voxel
    0 occupied (slot 0) -- and is not read (its coordinates hold the NaN payload); U = the voxels of the valid queries and voxel 0"""
    Ca, Cb, N = SHAPE
    x = X._cross(SHAPE, kind, False)
    full = _Index(dev, x.q, RC.counts_dev((N, N), dev), Cb, N)
    for a, b in ((full.mask, x.mask), (full.vox, x.vox), (full.slot, x.slot), (full.ucount, x.ucount)):
        assert torch.equal(_bits(a), _bits(b))
    full.bands()
    counts = (64, 20)
    q = x.q.clone()
    q.view(torch.int32)[1, 20:] = G.NAN_OUT
    r = _Index(dev, q, RC.counts_dev(counts, dev), Cb, N)
    mask, vox = r.mask.view(Cb, N), r.vox.view(Cb, N)
    assert not _bits(mask[1, 20:]).any() and not vox[1, 20:].any()
    assert torch.equal(_bits(mask[0]), _bits(x.mask.view(Cb, N)[0])) and torch.equal(vox[0], x.vox.view(Cb, N)[0])
    assert torch.equal(_bits(mask[1, :20]), _bits(x.mask.view(Cb, N)[1, :20])) and torch.equal(vox[1, :20], x.vox.view(Cb, N)[1, :20])
    valid = np.concatenate([x.vox.view(Cb, N)[0].cpu().numpy(), x.vox.view(Cb, N)[1, :20].cpu().numpy()])
    occupied = np.unique(np.concatenate([valid, [0]]))
    slot_ref = np.full(NG, -1, np.int32)
    slot_ref[occupied] = np.arange(len(occupied), dtype=np.int32)
    assert np.array_equal(r.slot.cpu().numpy(), slot_ref) and slot_ref[0] == 0 and int(r.ucount[0]) == len(occupied)
    r.bands()


@pytest.mark.parametrize("counts", [(64, 20), (64, 64), (1, 33)])
def test_pair_mean_and_spread_counts(dev, counts):
    """one chunk through dpd_decoder_fwd_cross_counts and dpd_cross_bwd_counts on a hand-made upstream: Dd[i, j] within sum_bound(count)
    of the float64 sum of the pred it wrote over n < counts[j], divided by the count; dpred == Gd[i, j] / counts[j] on those rows and 0 on
    the rest, exactly.  counts all N: Dd and dpred bitwise those of the un-counted entries."""
    from dpdist_amd import lib as L
    lib, s = L.load(), L.cur_stream()
    Ca, Cb, N = SHAPE
    x = X._cross(SHAPE, "random", False)
    qc = RC.counts_dev(counts, dev)
    r = _Index(dev, x.q, qc, Cb, N)
    rows, rows_p, H, pairs = x.rows, x.rows_p, H_DEC, Ca * Cb
    f32, i32 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int32, device=dev)
    Xu, Xu_band = G.banded((X.KW, x.cap), x.cap, **f32)
    Xt, Xt_band = G.banded((rows_p, 32), 32, **f32)
    uid, uid_band = G.banded_flat(rows_p, **i32)
    maskr, maskr_band = G.banded_flat(rows_p, **f32)
    cnt, cnt_band = G.banded_flat(4, **i32)
    L.check(lib.dpd_cross_gather(L.ptr(x.q), L.ptr(r.vox), L.ptr(r.mask), L.ptr(r.slot), L.ptr(r.ucount), L.ptr(x.fv), None, Ca, Cb, N, M_GRID,
                                 K_WIN, KP, L.ptr(Xu), x.cap, L.ptr(Xt), L.ptr(uid), L.ptr(maskr), L.ptr(cnt), s), "dpd_cross_gather")
    start, start_band = G.banded_flat(NG + 1, **i32)
    qlist, qlist_band = G.banded_flat(Cb * N, **i32)
    svox, svox_band = G.banded_flat(NG, **i32)
    L.check(lib.dpd_cross_invert(L.ptr(r.vox), L.ptr(r.slot), L.ptr(r.ucount), Cb, N, M_GRID, L.ptr(start), L.ptr(qlist), L.ptr(svox), s),
            "dpd_cross_invert")
    tens, _ = X._decoder_weights(dev, H, False)                                 # hand-made weights: about half of the rows leave relu6 open
    tens += [tens[2].t().contiguous(), tens[4].t().contiguous(), tens[0].t().contiguous()]      # W2T, W3T, W1pT for the backward
    cp = L.make_params(*tens)
    bufs, bands = {}, [Xu_band, Xt_band, uid_band, maskr_band, cnt_band, start_band, qlist_band, svox_band]
    for name, shp in (("Pu", (x.cap, H)), ("h1", (rows_p, H)), ("h2", (rows_p, H)), ("h3", (rows_p, H)), ("y", (rows_p, 3)), ("pred", (rows_p, 3)),
                      ("dpred", (rows_p, 3)), ("dy", (rows_p, 3)), ("ga", (rows_p, H)), ("gb", (rows_p, H)), ("dq", (rows_p, 3)),
                      ("gs", (x.cap, H)), ("dXs", (x.cap, KP)), ("dfv", (Ca * NG, 20)), ("gQ", (Cb * N, 3)), ("act0", (rows_p, H)), ("act1", (rows_p, H)),
                      ("y0", (rows_p, 3)), ("pred0", (rows_p, 3)), ("Pu0", (x.cap, H)), ("dpred0", (rows_p, 3))):
        bufs[name], b = G.banded(shp, shp[1], **f32)
        bands.append(b)
    Dd, Dd_band = G.banded_flat(pairs, **f32)
    D0, D0_band = G.banded_flat(pairs, **f32)
    bands += [Dd_band, D0_band]
    p = {k: L.ptr(t) for k, t in bufs.items()}
    L.check(lib.dpd_decoder_fwd_cross_counts(L.ptr(Xu), x.cap, x.cap, L.ptr(Xt), L.ptr(uid), L.ptr(cnt), p["Pu0"], L.ptr(maskr), L.ptr(qc), pairs,
                                             Cb, N, KP, H, cp, p["act0"], p["act1"], p["y0"], p["pred0"], L.ptr(Dd), s),
            "dpd_decoder_fwd_cross_counts")
    L.check(lib.dpd_decoder_fwd_cross_keep(L.ptr(Xu), x.cap, x.cap, L.ptr(Xt), L.ptr(uid), L.ptr(cnt), p["Pu"], L.ptr(maskr), pairs, N, KP, H, cp,
                                           p["h1"], p["h2"], p["h3"], p["y"], p["pred"], None, s), "dpd_decoder_fwd_cross_keep")
    Gd = torch.tensor(np.random.default_rng(21).standard_normal(pairs).astype(np.float32), device=dev)
    bufs["gQ"].fill_(0.0)
    back = (p["y"], p["h1"], p["h2"], p["h3"], L.ptr(cnt), L.ptr(start), L.ptr(qlist), L.ptr(svox), Ca, Cb, N, M_GRID, K_WIN, KP, H, x.cap, cp)
    rest = (p["dy"], p["ga"], p["gb"], p["dq"], p["gs"], p["dXs"], p["dfv"], p["gQ"], s)
    L.check(lib.dpd_cross_bwd_counts(L.ptr(Gd), L.ptr(maskr), L.ptr(qc), *back, p["dpred"], *rest), "dpd_cross_bwd_counts")
    torch.cuda.synchronize()
    pred = bufs["pred0"]
    assert torch.equal(_bits(pred), _bits(bufs["pred"])) and float(pred[:rows, 0].max()) > 0
    per = pred[:rows, 0].double().view(pairs, N).cpu().numpy()
    n_of = np.tile(np.array(counts), Ca)                                        # pair p = i * Cb + j
    want = np.array([per[pr, :n_of[pr]].sum() / n_of[pr] for pr in range(pairs)])
    err = np.abs(Dd.double().cpu().numpy() - want)
    bound = np.array([X.sum_bound(n) for n in n_of])
    print("Dd vs float64 sums over the counts %s: %s (bounds %s)" % (counts, " ".join("%.2e" % e for e in err), " ".join("%.2e" % b for b in bound)))
    assert (err <= bound).all() and want.max() > 0
    dpred = bufs["dpred"].cpu().numpy()
    want_d = np.zeros((rows_p, 3), np.float32)
    g = Gd.cpu().numpy()
    for pr in range(pairs):
        want_d[pr * N:pr * N + n_of[pr], 0] = g[pr] / np.float32(n_of[pr])
    assert np.array_equal(dpred.view(np.int32), want_d.view(np.int32))
    g1 = bufs["ga"]
    dead = torch.tensor(np.concatenate([np.arange(N) >= n for n in n_of] + [np.ones(rows_p - rows, bool)]), device=dev)
    assert not float(g1[dead].abs().sum()) > 0 and float(g1.abs().max()) > 0   # padded rows: exact zeros through dpred and the mask
    assert not float(bufs["dq"][:rows][dead[:rows]].abs().sum()) > 0
    gQ = bufs["gQ"].view(Cb, N, 3)
    for j, n in enumerate(counts):
        assert not _bits(gQ[j, n:]).any(), "the query route of a padded point is +0.0"
    if counts == (N, N):
        L.check(lib.dpd_decoder_fwd_cross(L.ptr(Xu), x.cap, x.cap, L.ptr(Xt), L.ptr(uid), L.ptr(cnt), p["Pu0"], L.ptr(maskr), pairs, N, KP, H, cp,
                                          p["act0"], p["act1"], p["y0"], p["pred0"], L.ptr(D0), s), "dpd_decoder_fwd_cross")
        L.check(lib.dpd_cross_bwd(L.ptr(Gd), L.ptr(maskr), *back, p["dpred0"], *rest), "dpd_cross_bwd")
        torch.cuda.synchronize()
        assert torch.equal(_bits(D0), _bits(Dd)) and torch.equal(_bits(bufs["dpred0"]), _bits(bufs["dpred"]))
    else:
        assert G.untouched(D0) and G.untouched(bufs["dpred0"])
    for b in bands:
        b()
    r.bands()
    del tens


# ------------------------------------------------------------------------------------------------------------ the public interface
def _cu(t, dev, grad=False):
    return torch.tensor(np.ascontiguousarray(t), device=dev).requires_grad_(grad)


def _run(dev, pad=0.0, max_rows=16384, needA=True, needB=True, self_matrix=False, device_counts=False):
    """DPDistMatrix on the two ragged sets (padding set to `pad`) -> (outputs, gradients of the loss of ragged_cases w.r.t. the sets that ask)"""
    from dpdist_amd import DPDistMatrix
    A, B = RC.sets()
    a = _cu(RC.with_padding(A, RC.COUNTS_A, pad), dev, needA)
    cA = RC.counts_dev(RC.COUNTS_A, dev) if device_counts else list(RC.COUNTS_A)
    mod = DPDistMatrix(X._params(dev), max_rows=max_rows)
    if self_matrix:
        out = mod(a, return_directed=True, countsA=cA)
        wrt = [a]
    else:
        b = _cu(RC.with_padding(B, RC.COUNTS_B, pad), dev, needB)
        out = mod(a, b, return_directed=True, countsA=cA, countsB=torch.tensor(RC.COUNTS_B))
        wrt = [t for t, need in ((a, needA), (b, needB)) if need]
    loss = XG._loss(out, RC.upstream(self_matrix), True, dev)
    return out, list(torch.autograd.grad(loss, wrt))


def test_matrix_against_the_composed_oracle(dev):
    """D, D_AB, D_BA of dpdist_matrix with counts within 1e-4 absolute of the float64 oracle composed per pair and direction on the
    truncated clouds; DPDistMatrix gives the same bits; counts as a list, a CPU tensor and a device tensor are the same call"""
    from dpdist_amd import dpdist_matrix
    A, B = RC.sets()
    P = X._params(dev)
    got = dpdist_matrix(P, _cu(A, dev), _cu(B, dev), return_directed=True, countsA=RC.COUNTS_A, countsB=torch.tensor(RC.COUNTS_B))
    Do = RC.matrix_oracle(torch.float64)
    assert float(Do[0].max() - Do[0].min()) > 0.05                  # a matrix with structure, not a constant
    for name, g, want in zip(("D", "D_AB", "D_BA"), got, Do):
        err = float(np.abs(g.double().cpu().numpy() - want).max())
        print("%s vs the composed float64 oracle: %.3e" % (name, err))
        assert g.shape == (3, 2) and err <= RC.FWD_BAR, name
    out, _ = _run(dev, device_counts=True)
    for g, o in zip(got, out):
        assert torch.equal(_bits(g), _bits(o.detach()))
    # only one set counted: the other is full, and the widths still differ
    one = dpdist_matrix(P, _cu(A, dev), _cu(B[:, :1], dev), return_directed=True, countsA=RC.COUNTS_A)
    assert torch.equal(_bits(one[1][:, 1]), _bits(got[1][:, 1]))    # D_AB: the counted surfaces A against the single query of B_1


def test_gradients_against_the_composed_oracle(dev):
    """gradients of (G D).sum() + the directed terms against float64 autograd through the same composition, at the project's
    input-gradient bar; the gradients at padded points are +0.0 by bits"""
    _, (gA, gB) = _run(dev)
    for name, got, (ref, bar), counts in zip(("gA", "gB"), (gA, gB), RC.grad_bars(), (RC.COUNTS_A, RC.COUNTS_B)):
        err = np.abs(got.double().cpu().numpy() - ref).max()
        print("%s vs the composed float64 oracle: %.3e (bar %.3e, max|ref| %.3e)" % (name, err, bar, np.abs(ref).max()))
        assert np.abs(ref).max() > 20 * bar, "a reference gradient without structure makes the bar vacuous"
        assert got.shape == ref.shape and err <= bar, name
        for c, n in enumerate(counts):
            assert not _bits(got[c, n:]).any(), (name, c)
            assert float(got[c, :n].abs().max()) > 0 or (name, c) == ("gB", 1)      # B_1: one point, on the lower relu6 saturation as a query


def test_the_padding_changes_no_bit(dev):
    ref_out, ref_g = _run(dev, pad=0.0)
    for pad in (0.37, 5.0):
        out, g = _run(dev, pad=pad)
        for a, b in zip(list(out) + g, list(ref_out) + ref_g):
            assert torch.equal(_bits(a.detach()), _bits(b.detach())), pad


def test_chunking_changes_no_bit(dev):
    one_out, one_g = _run(dev, max_rows=1 << 20)
    per_out, per_g = _run(dev, max_rows=1)                          # every chunk holds one surface cloud
    for a, b in zip(list(one_out) + one_g, list(per_out) + per_g):
        assert torch.equal(_bits(a.detach()), _bits(b.detach()))
    assert all(float(g.abs().max()) > 0 for g in one_g)


def test_self_matrix_with_counts(dev):
    out, (g,) = _run(dev, self_matrix=True)
    assert torch.equal(_bits(out[2].detach()), _bits(out[1].detach().t().contiguous()))
    Do = RC.matrix_oracle(torch.float64, True)
    for name, o, want in zip(("D", "D_AB", "D_BA"), out, Do):
        err = float(np.abs(o.detach().double().cpu().numpy() - want).max())
        print("self %s vs the composed float64 oracle: %.3e" % (name, err))
        assert err <= RC.FWD_BAR, name
    (ref, bar), = RC.grad_bars(True)
    err = np.abs(g.double().cpu().numpy() - ref).max()
    print("self gA vs the composed float64 oracle: %.3e (bar %.3e, max|ref| %.3e)" % (err, bar, np.abs(ref).max()))
    assert np.abs(ref).max() > 20 * bar and err <= bar
    for c, n in enumerate(RC.COUNTS_A):
        assert not _bits(g[c, n:]).any()


def test_partial_gradients_with_counts(dev):
    """one set without requires_grad gets None; the other keeps its bits"""
    from dpdist_amd import DPDistMatrix
    _, (gA, gB) = _run(dev)
    _, (oA,) = _run(dev, needB=False)
    _, (oB,) = _run(dev, needA=False)
    assert torch.equal(_bits(oA), _bits(gA)) and torch.equal(_bits(oB), _bits(gB))
    A, B = RC.sets()
    a, b = _cu(A, dev, True), _cu(B, dev)
    DPDistMatrix(X._params(dev))(a, b, countsA=RC.COUNTS_A, countsB=RC.COUNTS_B).sum().backward()
    assert a.grad is not None and b.grad is None


def test_full_counts_are_the_call_without_counts(dev):
    """counts equal to N everywhere: at N = 712 (both calls encode over tiles) the forward is bit for bit the call without counts; at
    N = 1640 (the backward runs over tiles too) so are the gradients"""
    from dpdist_amd import DPDistMatrix, dpdist_matrix
    from dpdist_amd import ops
    P = X._params(dev)
    rng = np.random.default_rng(712)
    N = 712
    assert ops.encoder_tiled(N, M_GRID)
    A, B = (torch.tensor(rng.uniform(-0.8, 0.8, size=(2, N, 3)).astype(np.float32), device=dev) for _ in range(2))
    want = dpdist_matrix(P, A, B, return_directed=True)
    got = dpdist_matrix(P, A, B, return_directed=True, countsA=[N, N], countsB=[N, N])
    for g, w in zip(got, want):
        assert torch.equal(_bits(g), _bits(w))
    N = 1640
    assert ops.encoder_tiled(N, M_GRID, ops.FITS_BWD_SLICED)
    A, B = (torch.tensor(rng.uniform(-0.8, 0.8, size=(c, N, 3)).astype(np.float32), device=dev) for c in (1, 2))
    Gs = XG._upstream((1, 2, N))
    mod = DPDistMatrix(P)

    def grads(**kw):
        a, b = A.clone().requires_grad_(True), B.clone().requires_grad_(True)
        out = mod(a, b, return_directed=True, **kw)
        return list(out) + list(torch.autograd.grad(XG._loss(out, Gs, True, dev), [a, b]))

    for g, w in zip(grads(countsA=[N], countsB=[N, N]), grads()):
        assert torch.equal(_bits(g.detach()), _bits(w.detach()))

"""The 3DmFV encoder over tiles of points (dpd_mfv3d_fwd_tiled / dpd_mfv3d_bwd_tiled, dpdist_amd/csrc/mfv3d.hip) against the float64
oracle: the tile logic at the smallest shapes where it can go wrong (ragged and one-point last tiles, empty point slices, a tile larger
than the cloud, two batches of Gaussians per wave), tiling that does not change the answer, ties and the 0/0 flag across tiles, clouds
beyond the plain entries' LDS caps, refusals, and the public interface (DPDistLoss, dpdist_matrix, DPDistMatrix) at such clouds.
Cases: tests/mfv_tiled_cases.py; method, bars and checkers: tests/mfv_cases.py (tests/test_mfv_tiled_cpu.py runs the admission of every
case on the CPU).  Outputs and workspaces sit in NaN-payload guard bands that must come back untouched."""
import functools

import numpy as np
import pytest
import torch

from dpdist_amd import synth

from . import mfv_cases as M
from . import mfv_tiled_cases as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible")
    from dpdist_amd import lib
    lib.load()     # raises if the HIP extension is missing -- never fall back
    return torch.device("cuda:0")


def _id(case):
    return "%s-C%d-N%d-m%d-s%g" % case


def _cu(a, dev):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device=dev)


def _forward(dev, case, tile):
    rc, fv, band = T.gpu_forward_tiled(_cu(T.points(case), dev), case[3], case[4], tile)
    assert rc == 0, rc
    M.check_forward(fv, band, T.forward_ref(case), case[3], (case, "tile", tile))
    return fv


def _backward(dev, case, tile):
    ref = T.backward_ref(case)
    rc, g, bands, ws = T.gpu_backward_tiled(_cu(T.points(case), dev), _cu(ref.dfv, dev), case[3], case[4], tile)
    assert rc == 0, rc
    assert not M.untouched(ws)
    M.check_backward(g, bands, ref, (case, "tile", tile))
    return g


# ------------------------------------------------------------------------------------------------ 1. tile logic
@pytest.mark.parametrize("case,tile,bwd", T.TILE_CASES, ids=["%s-t%d" % (_id(c), t) for c, t, _ in T.TILE_CASES])
def test_tile_logic_vs_float64(dev, case, tile, bwd):
    _forward(dev, case, tile)
    if bwd:
        _backward(dev, case, tile)


# ------------------------------------------------------------------------------------------------ 2. tiling does not change the answer
def test_tiling_does_not_change_the_answer(dev):
    case = T.SAME_CASE
    _, C, N, m, sigma = case
    fref, bref = T.forward_ref(case), T.backward_ref(case)
    pts, dfv = _cu(T.points(case), dev), _cu(bref.dfv, dev)
    fvs = [_forward(dev, case, t).clone() for t in T.SAME_TILES]
    gs = [_backward(dev, case, t).clone() for t in T.SAME_TILES]
    # the plain entries on the same cloud (N under every plain cap): each at its bar against float64, and the forms among each other
    rc, fv_p, band = M.gpu_forward(pts, m, sigma)
    assert rc == 0
    M.check_forward(fv_p, band, fref, m, (case, "plain"))
    fvs.append(fv_p)
    for sliced in (True, False):
        rc, g_p, bands, _ = M.gpu_backward(pts, dfv, m, sigma, sliced)
        assert rc == 0
        M.check_backward(g_p, bands, bref, (case, "plain", sliced))
        gs.append(g_p)
    for fv in fvs[1:]:
        assert float((fv.double() - fvs[0].double()).abs().max()) <= fref.bar
    for g in gs[1:]:
        M.check_forms_agree(g, gs[0], bref.scale, case)
    # the same call twice: the same bits
    for t in T.SAME_TILES:
        rc, fv2, band = T.gpu_forward_tiled(pts, m, sigma, t)
        rc2, g2, bands, _ = T.gpu_backward_tiled(pts, dfv, m, sigma, t)
        assert rc == 0 and rc2 == 0
        band(), bands()
        i = T.SAME_TILES.index(t)
        assert torch.equal(fv2.view(torch.int32), fvs[i].view(torch.int32)) and torch.equal(g2.view(torch.int32), gs[i].view(torch.int32))


# ------------------------------------------------------------------------------------------------ 3. ties across tiles
@pytest.mark.parametrize("case", T.TIE_CASES, ids=_id)
def test_ties_across_tiles(dev, case):
    """every copy of a point sits in another tile (tests/test_mfv_tiled_cpu.py): the share of a max / min gradient is 1 / (ties in the
    CLOUD), as float64 autograd splits it (the bar of check_backward: a share taken per tile would be off by a factor of two), and the
    copies of a point receive the same bits"""
    idx = torch.tensor(T.tie_partner(case[0], case[2]), device=dev)
    _forward(dev, case, 8)
    g = _backward(dev, case, 8)
    assert torch.equal(g[:, idx].view(torch.int32), g.view(torch.int32))


# ------------------------------------------------------------------------------------------------ 4. the 0/0 flag across tiles
@pytest.mark.parametrize("where", ["last", "first"])
def test_zero_over_zero_in_any_tile_poisons_the_cloud(dev, where):
    p = np.random.default_rng(5).uniform(-0.8, 0.8, size=(1, 24, 3)).astype(np.float32)
    p[0, 23 if where == "last" else 0] = 3.0          # every pdf underflows: the reference's 0/0 (utils/dpdist_util.py:74)
    rc, fv, band = T.gpu_forward_tiled(_cu(p, dev), 8, T.S0, 8)
    assert rc == 0 and bool(torch.isnan(fv).all())
    band()


# ------------------------------------------------------------------------------------------------ 5. beyond the plain caps
@pytest.mark.parametrize("case", T.BIG_FWD, ids=_id)
def test_forward_beyond_the_plain_cap(dev, case):
    from dpdist_amd import lib as L
    assert L.load().dpd_mfv3d_fits(case[2], case[3], 0) == 0
    rc, fv, band = M.gpu_forward(torch.zeros(1, case[2], 3, device=dev), case[3], case[4])
    assert rc == T.E_UNSUPPORTED and M.untouched(fv)          # the plain entry keeps its refusal
    _forward(dev, case, 0)


@pytest.mark.parametrize("case", T.BIG_BWD, ids=_id)
def test_backward_beyond_the_plain_cap(dev, case):
    from dpdist_amd import lib as L
    assert L.load().dpd_mfv3d_fits(case[2], case[3], 2) == 0
    _backward(dev, case, 0)


def test_ops_route_to_the_tiled_entries(dev):
    """ops.mfv3d_fwd / mfv3d_bwd beyond the plain caps return the bits of the tiled entries at their default tile; sliced=False beyond the
    one-launch cap falls through to the tiled entry with a workspace (N = 1640 is beyond both backward caps, N = 712 only beyond the
    forward's and the one-launch backward's)"""
    from dpdist_amd import ops
    bits = lambda t: t.contiguous().view(torch.int32)          # noqa: E731
    for case in (("u", 1, 1640, 8, T.S0), ("u", 1, 712, 8, T.S0)):
        _, C, N, m, sigma = case
        pts = _cu(T.points(case), dev)
        rc, fv, band = T.gpu_forward_tiled(pts, m, sigma, 0)
        assert rc == 0 and torch.equal(bits(ops.mfv3d_fwd(pts, m, sigma)), bits(fv))
        dfv = _cu(M.upstream(T.forward_ref(case).fv64, [7, C, N, m]), dev)
        rc, g, bands, _ = T.gpu_backward_tiled(pts, dfv, m, sigma, 0)
        assert rc == 0 and torch.equal(bits(ops.mfv3d_bwd(pts, dfv, m, sigma, sliced=False)), bits(g))
        if N > 1636:
            assert torch.equal(bits(ops.mfv3d_bwd(pts, dfv, m, sigma)), bits(g))
        else:       # the sliced plain entry takes it: its own launches, the same answer within the forms' bar
            rc, g_p, bands_p, _ = M.gpu_backward(pts, dfv, m, sigma, True)
            assert rc == 0 and torch.equal(bits(ops.mfv3d_bwd(pts, dfv, m, sigma)), bits(g_p))
            M.check_forms_agree(g_p, g, np.maximum(1.0, g.abs().amax((1, 2)).cpu().numpy()), case)


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals_leave_outputs_and_workspace_untouched(dev):
    pts = torch.zeros(2, 16, 3, device=dev)
    nan = float("nan")
    for kw, want in (({"m": 11}, T.E_UNSUPPORTED), ({"N": 0}, T.E_UNSUPPORTED), ({"N": 4097}, T.E_UNSUPPORTED), ({"tile": 12}, T.E_UNSUPPORTED),
                     ({"tile": 4}, T.E_UNSUPPORTED), ({"sigma": 0.0}, T.E_DIM), ({"sigma": nan}, T.E_DIM), ({"C": 0}, T.E_DIM)):
        a = dict({"m": 8, "sigma": T.S0, "C": None, "N": None, "tile": 0}, **kw)
        rc, fv, band = T.gpu_forward_tiled(pts, a["m"], a["sigma"], a["tile"], C=a["C"], N=a["N"])
        assert rc == want and M.untouched(fv), ("forward", kw, rc)
        band()
        dfv = torch.zeros(2, a["m"] ** 3, M.F, device=dev)
        rc, g, bands, ws = T.gpu_backward_tiled(pts, dfv, a["m"], a["sigma"], a["tile"], C=a["C"], N=a["N"])
        assert rc == want and M.untouched(g) and M.untouched(ws), ("backward", kw, rc)
        bands()
    # the backward keeps one Gaussian per lane pair: m = 9 is beyond it (the forward takes it); a workspace one byte short
    rc, g, bands, ws = T.gpu_backward_tiled(pts, torch.zeros(2, 729, M.F, device=dev), 9, T.S0, 0)
    assert rc == T.E_UNSUPPORTED and M.untouched(g) and M.untouched(ws)
    bands()
    rc, g, bands, ws = T.gpu_backward_tiled(pts, torch.zeros(2, 512, M.F, device=dev), 8, T.S0, 0, ws_short=1)
    assert rc == T.E_WORKSPACE and M.untouched(g) and M.untouched(ws)
    bands()


# ------------------------------------------------------------------------------------------------ 7. the public interface
H, K_WIN, M_GRID, SIGMA = 64, 5, 8, 0.125


def _model(dev):
    from dpdist_amd.model import DPDistModel
    mod = DPDistModel(Embedding_Size=M_GRID ** 3, k=K_WIN, localSNmlp=(H,) * 3, sigma3dmfv=SIGMA, device=dev)
    mod.load_tf_state_dict(synth.make_weights("wide", mlp=(H,) * 3))
    return mod


@functools.lru_cache(maxsize=None)
def _clouds(Ca, Cb, N):
    """seeds 106 / 107: of the seeds 100, 102 .. 108 the first at which the float32 ORACLE's input gradients sit within 5e-5 of the
    float64 ones at every shape used here (a max / min that flips between two near-ties in float32 moves a gradient by 1e-3, which says
    nothing about a kernel): the bars below are then the project's 2e-4 floor"""
    A = synth.s2_modelnet_shaped(Ca, N, 106)[0].astype(np.float32)
    B = synth.s2_modelnet_shaped(Cb, N, 107)[1].astype(np.float32)
    return A, B


@functools.lru_cache(maxsize=None)
def _pair_oracle(B, N, dtype):
    """loss_pred and its two input gradients through oracle.restate.get_model / get_loss (float64 numpy)"""
    from oracle import restate as R
    pa, pb = _clouds(B, B, N)
    W = R.as_torch_weights(synth.make_weights("wide", mlp=(H,) * 3), dtype)
    a, b = torch.tensor(pa, dtype=dtype, requires_grad=True), torch.tensor(pb, dtype=dtype, requires_grad=True)
    ps, _ = R.get_model(a, b, W, m=M_GRID, k=K_WIN, sigma=SIGMA)
    loss = R.get_loss(ps, torch.zeros(B, N, dtype=dtype))[1]
    gA, gB = torch.autograd.grad(loss, [a, b])
    return float(loss.detach()), gA.double().numpy(), gB.double().numpy()


def _grad_bar(ref64, ref32):
    """the project's input-gradient bar (tests/test_gpu_parity.py::test_losses_and_input_gradients_golden, tests/test_cross_grad_gpu.py::_bar):
    max(4 x the distance of the float32 oracle from the float64 one, 2e-4 max(1, max|ref|))"""
    return max(4.0 * np.abs(ref32 - ref64).max(), 2e-4 * max(1.0, np.abs(ref64).max()))


@pytest.mark.parametrize("B,N,engine", [(1, 712, True), (2, 1024, True), (2, 1024, False)])
def test_dpdist_loss_beyond_the_plain_cap(dev, monkeypatch, B, N, engine):
    from dpdist_amd.model import DPDistLoss
    monkeypatch.setattr("dpdist_amd.asloss.ENGINE", engine)
    l64, a64, b64 = _pair_oracle(B, N, torch.float64)
    _, a32, b32 = _pair_oracle(B, N, torch.float32)
    pa, pb = _clouds(B, B, N)
    a, b = _cu(pa, dev).requires_grad_(True), _cu(pb, dev).requires_grad_(True)
    loss = DPDistLoss(_model(dev))(a, b)
    gA, gB = torch.autograd.grad(loss, [a, b])
    print("loss %.8g oracle %.8g" % (loss.item(), l64))
    assert abs(loss.item() - l64) <= 2e-5                     # the project's loss bar (test_losses_and_input_gradients_golden)
    for name, got, r64, r32 in (("gA", gA, a64, a32), ("gB", gB, b64, b32)):
        bar = _grad_bar(r64, r32)
        err = np.abs(got.double().cpu().numpy() - r64).max()
        print("%s vs float64 oracle: %.3e (bar %.3e, max|ref| %.3e)" % (name, err, bar, np.abs(r64).max()))
        assert np.abs(r64).max() > 20 * bar, "a reference gradient without structure makes the bar vacuous"
        assert got.shape == r64.shape and err <= bar, name


@functools.lru_cache(maxsize=None)
def _matrix_oracle(shape, dtype):
    """D [Ca, Cb] and the gradients of (G D).sum() through the oracle on the hand-tiled pairs (tests/test_cross_grad_gpu.py::_oracle_grads)"""
    from oracle import restate as R
    Ca, Cb, N = shape
    A, B = _clouds(Ca, Cb, N)
    W = R.as_torch_weights(synth.make_weights("wide", mlp=(H,) * 3), dtype)
    a, b = torch.tensor(A, dtype=dtype, requires_grad=True), torch.tensor(B, dtype=dtype, requires_grad=True)
    ps, _ = R.get_model(a.repeat_interleave(Cb, 0), b.repeat(Ca, 1, 1), W, m=M_GRID, k=K_WIN, sigma=SIGMA)
    D = torch.stack([R.get_loss({k: t[p:p + 1] for k, t in ps.items()}, torch.zeros(1, N, dtype=dtype))[1] for p in range(Ca * Cb)]).view(Ca, Cb)
    G = torch.tensor(np.random.default_rng([77, Ca, Cb, N]).standard_normal((Ca, Cb)), dtype=dtype)
    gA, gB = torch.autograd.grad((G * D).sum(), [a, b])
    return D.detach().double().numpy(), G.double().numpy(), gA.double().numpy(), gB.double().numpy()


def test_matrix_beyond_the_plain_cap(dev):
    from dpdist_amd import DPDistMatrix, dpdist_matrix
    from dpdist_amd.model import DPDistParams
    shape = (2, 1, 712)
    D64, G, a64, b64 = _matrix_oracle(shape, torch.float64)
    _, _, a32, b32 = _matrix_oracle(shape, torch.float32)
    A, B = _clouds(*shape)
    P = DPDistParams(k=K_WIN, mlp=(H,) * 3, device=dev, init=None)
    P.load_tf_state_dict(synth.make_weights("wide", mlp=(H,) * 3))
    D = dpdist_matrix(P, _cu(A, dev), _cu(B, dev))
    assert D.shape == (2, 1) and np.abs(D.double().cpu().numpy() - D64).max() <= 2e-5
    a, b = _cu(A, dev).requires_grad_(True), _cu(B, dev).requires_grad_(True)
    Dm = DPDistMatrix(P)(a, b)
    assert torch.equal(Dm.detach().view(torch.int32), D.view(torch.int32))
    gA, gB = torch.autograd.grad((torch.tensor(G, dtype=torch.float32, device=dev) * Dm).sum(), [a, b])
    for name, got, r64, r32 in (("gA", gA, a64, a32), ("gB", gB, b64, b32)):
        bar = _grad_bar(r64, r32)
        err = np.abs(got.double().cpu().numpy() - r64).max()
        print("%s vs float64 oracle: %.3e (bar %.3e, max|ref| %.3e)" % (name, err, bar, np.abs(r64).max()))
        assert np.abs(r64).max() > 20 * bar, "a reference gradient without structure makes the bar vacuous"
        assert got.shape == r64.shape and err <= bar, name


def test_dpdist_loss_at_64_points_keeps_its_bits(dev, monkeypatch):
    """shapes the plain entries take run the launches they ran before: DPDistLoss at N = 64, with the engine and without, against the C
    entries called one by one with the PLAIN encoder entries (dpd_mfv3d_fwd_stacked, dpd_mfv3d_bwd), bit for bit"""
    from dpdist_amd import lib as L, ops
    from dpdist_amd.model import DPDistLoss
    B, N = 2, 64
    pa, pb = _clouds(B, B, N)
    mod = _model(dev)
    P = mod.params_
    lib, s = L.load(), L.cur_stream()
    pcA, pcB = _cu(pa, dev), _cu(pb, dev)
    f = lambda *sh: torch.empty(*sh, device=dev, dtype=torch.float32)   # noqa: E731
    pts, q, fv, ssq = f(2 * B, N, 3), f(2 * B, N, 3), f(2 * B, M_GRID ** 3, M.F), f(2 * B, M.SLICES, M.F)
    X, mask, vox = f(2 * B * N, P.KP), f(2 * B * N), torch.empty(2 * B * N, device=dev, dtype=torch.int32)
    L.check(lib.dpd_mfv3d_fwd_stacked(L.ptr(pcA), L.ptr(pcB), None, B, N, M_GRID, SIGMA, L.ptr(pts), L.ptr(q), L.ptr(fv), L.ptr(ssq), s), "enc")
    L.check(lib.dpd_patch_rows_fwd_scaled(L.ptr(q), L.ptr(fv), L.ptr(ssq), 2 * B, N, M_GRID, K_WIN, P.KP, L.ptr(X), L.ptr(mask), L.ptr(vox), None, s), "rows")
    params = P.views(P.flat)
    h1, h2, h3, _, _ = ops.decoder_fwd(X, mask, params, P.H, out_layer=False)
    _, _, loss, _, g3 = ops.out_asloss(h3, mask, params, B * N, want_grad=True)
    _, _, _, _, dX = ops.decoder_bwd_data(None, None, None, h1, h2, None, params, P.KP, True, transposed=P.transposed(P.flat), phases=6, g3=g3)
    _, dfv = ops.patch_rows_bwd(dX, vox, 2 * B, N, M_GRID, K_WIN, want_dq=False)
    dpts = torch.empty_like(pts)
    ws = torch.empty(lib.dpd_mfv3d_bwd_workspace_bytes(2 * B, M_GRID) // 4, device=dev)
    L.check(lib.dpd_mfv3d_bwd(L.ptr(pts), L.ptr(dfv), 2 * B, N, M_GRID, SIGMA, L.ptr(dpts), L.ptr(ws), ws.numel() * 4, s), "enc bwd")
    wA, wB = ops.asloss_combine(dpts, dX, torch.ones((), device=dev), B, N, K_WIN)
    bits = lambda t: t.detach().contiguous().view(torch.int32)          # noqa: E731
    for engine in (True, False):
        monkeypatch.setattr("dpdist_amd.asloss.ENGINE", engine)
        a, b = _cu(pa, dev).requires_grad_(True), _cu(pb, dev).requires_grad_(True)
        got = DPDistLoss(mod)(a, b)
        gA, gB = torch.autograd.grad(got, [a, b])
        assert torch.equal(bits(got.reshape(1)), bits(loss.reshape(1))), engine
        assert torch.equal(bits(gA), bits(wA)) and torch.equal(bits(gB), bits(wB)), engine

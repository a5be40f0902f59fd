"""csrc/regtest.hip on the GPU: the occlusion is exact against the numpy restatement of tests/test_regtest_cpu.py, the trace composes
the transforms with the refinement loop's own device functions (bit for bit) and measures them like the project's float64 host
functions, the square-rooted Chamfer shares its scan with the squared one, and regtest.no_stop_test strings them together."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

from dpdist_amd import lib as L
from dpdist_amd import registration as R
from dpdist_amd import regtest, synth
from tests.test_regtest_cpu import add_occlusions_np, key_permutation

pytestmark = pytest.mark.gpu

U = 2.0 ** -24          # fp32 unit roundoff


def cu(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()


# ------------------------------------------------------------------------------------------------------------------ occlusion

OCC_CASES = [(3, 64, 16), (2, 100, 37), (2, 300, 150), (1, 64, 0), (1, 64, 63), (1, 2048, 1024)]


@functools.lru_cache(maxsize=None)
def occ_case(B, N):
    rng = np.random.default_rng(7)
    src = rng.uniform(-1, 1, (B, N, 3)).astype(np.float32)
    seed = rng.integers(0, N, B).astype(np.int32)
    key = rng.random((B, N)).astype(np.float32)
    for a in (src, seed, key):
        a.setflags(write=False)
    return src, seed, key


@pytest.mark.parametrize("B,N,drop", OCC_CASES)
def test_occlusion_is_exact(B, N, drop):
    """One wave, a partial wave, more points than threads, both ends of `drop`, the LDS maximum."""
    src, seed, key = occ_case(B, N)
    for b in range(B):          # all distances distinct: the reference's unstable argsort gives the same answer as the stable one
        d = np.linalg.norm(src[b] - src[b, seed[b]], 2, -1)
        assert d.dtype == np.float32 and len(np.unique(d)) == N
        assert len(np.unique(key[b])) == N
    for k in (key, None):
        perms = None if k is None else key_permutation(src, seed, drop, k)
        want, want_kept = add_occlusions_np(src, seed, drop, perms, return_index=True)
        out, kept = regtest.occlude_with(cu(src), cu(seed), None if k is None else cu(k), drop, return_index=True)
        assert kept.dtype == torch.int32 and np.array_equal(kept.cpu().numpy(), want_kept)
        assert np.array_equal(out.cpu().numpy().view(np.int32), want.view(np.int32))
        only = regtest.occlude_with(cu(src), cu(seed), None if k is None else cu(k), drop)          # kept = NULL: the same clouds
        assert torch.equal(only, out)
    if drop == 0:               # no key, nothing dropped: survivors in distance order; and every point exactly once
        assert np.array_equal(np.sort(want_kept, 1), np.tile(np.arange(N, dtype=np.int32), (B, 1)))


def test_occlusion_ties_follow_distance_then_index():
    """The seed point stored four times (distance 0 four times) and two mirrored pairs at equal distance from it."""
    rng = np.random.default_rng(5)
    N = 16
    src = rng.uniform(0.5, 1, (1, N, 3)).astype(np.float32) * rng.choice([-1.0, 1.0], (1, N, 3)).astype(np.float32)
    for i in (2, 5, 7, 11):
        src[0, i] = 0.0
    v, w = np.float32([0.25, -0.125, 0.0625]), np.float32([0.3, 0.1, -0.2])
    src[0, 9], src[0, 1] = v, -v
    src[0, 4], src[0, 3] = w, -w
    seed = np.int32([7])
    d = np.linalg.norm(src[0] - src[0, 7], 2, -1)
    assert (d[[2, 5, 7, 11]] == 0).all() and d[1] == d[9] and d[3] == d[4] and d[1] < d[3] and d[3] < np.delete(d, [1, 2, 3, 4, 5, 7, 9, 11]).min()
    order = np.argsort(d, kind="stable")
    assert list(order[:8]) == [2, 5, 7, 11, 1, 9, 3, 4]
    for drop in (0, 2, 3, 5, 7):          # cuts inside the run of zeros and inside each mirrored pair
        out, kept = regtest.occlude_with(cu(src), cu(seed), None, drop, return_index=True)
        kept = kept.cpu().numpy()[0]
        assert np.array_equal(kept[:N - drop], order[drop:]), drop
        want, want_kept = add_occlusions_np(src, seed, drop, None, return_index=True)
        assert np.array_equal(kept, want_kept[0]) and np.array_equal(out.cpu().numpy(), want)
    key = np.zeros((1, N), np.float32)      # equal keys: the index decides
    _, kept = regtest.occlude_with(cu(src), cu(seed), cu(key), 5, return_index=True)
    assert np.array_equal(kept.cpu().numpy()[0, :N - 5], np.sort(order[5:]))


@pytest.mark.parametrize("B,N,drop", [(3, 64, 16), (2, 300, 150), (1, 2048, 1024)])
def test_occlusion_leaves_the_guard_bands_alone(B, N, drop):
    src, seed, key = occ_case(B, N)
    G = 64
    fo = torch.full((B * N * 3 + 2 * G,), -7.0, device="cuda")
    fk = torch.full((B * N + 2 * G,), -7, device="cuda", dtype=torch.int32)
    off = lambda t: ctypes.c_void_p(t.data_ptr() + 4 * G)      # noqa: E731
    s, sd, k = cu(src), cu(seed), cu(key)
    for kk in (k, None):
        fo.fill_(-7.0), fk.fill_(-7)
        L.check(L.load().dpd_occlude(L.ptr(s), L.ptr(sd), L.ptr(kk), B, N, drop, off(fo), off(fk), L.cur_stream()), "dpd_occlude")
        want, want_kept = regtest.occlude_with(s, sd, kk, drop, return_index=True)
        assert (fo[:G] == -7.0).all() and (fo[G + B * N * 3:] == -7.0).all() and (fk[:G] == -7).all() and (fk[G + B * N:] == -7).all()
        assert torch.equal(fo[G:G + B * N * 3].view(B, N, 3), want) and torch.equal(fk[G:G + B * N].view(B, N), want_kept)


def test_occlusion_refuses_bad_sizes_before_any_launch():
    s, sd = torch.zeros(1, 2049, 3, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    out = torch.full((1, 2049, 3), -7.0, device="cuda")
    lib = L.load()
    assert lib.dpd_occlude(L.ptr(s), L.ptr(sd), None, 1, 64, 64, L.ptr(out), None, L.cur_stream()) == -2         # drop = N
    assert lib.dpd_occlude(L.ptr(s), L.ptr(sd), None, 1, 2049, 16, L.ptr(out), None, L.cur_stream()) == -3       # N = 2049
    assert (out == -7.0).all()
    with pytest.raises(RuntimeError, match="DPD_E_DIM"):
        regtest.occlude_with(s[:, :64].contiguous(), sd, None, 64)
    with pytest.raises(RuntimeError, match="seed_idx"):
        regtest.occlude_with(s[:, :64].contiguous(), sd + 64, None, 16)
    with pytest.raises(RuntimeError, match="float32"):
        regtest.occlude(s[:, :64].double().contiguous(), 0.25)


def test_occlude_draws_on_the_device_and_keeps_the_survivors():
    src, _, _ = occ_case(3, 64)
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    a = regtest.occlude(cu(src), 0.25, g).cpu().numpy()
    g.manual_seed(1)
    b = regtest.occlude(cu(src), 0.25, g).cpu().numpy()
    assert np.array_equal(a, b)
    for c in range(3):          # 48 distinct points of the source survive, each one or two times
        rows = {tuple(r) for r in a[c]}
        assert len(rows) == 48 and rows <= {tuple(r) for r in src[c]}
    n = regtest.add_noise(cu(src), g).cpu().numpy() - src
    assert 0 < np.abs(n).max() < 0.04 * 6 and abs(n.mean()) < 0.005


# ---------------------------------------------------------------------------------------------------------------------- trace

def trace_case(L_, B, lim_rot):
    """Raw network outputs whose per-loop rotation is a few degrees, ground-truth poses U(-45, 45)^3 deg / U(-0.01, 0.01)^3 (float32: the
    entry takes them in float32, and the host side of the comparison is fed the same values)."""
    rng = np.random.default_rng(11)
    pred = rng.standard_normal((L_, B, 7))
    if lim_rot:
        pred *= np.array([0.3, 0.3, 0.3, 0.08, 1, 1, 1])          # t = 0.1 tanh(.), angle = lim_rot tanh(.)
    else:
        pred = np.concatenate([0.02 * pred[..., :3], 1 + 0.0 * pred[..., 3:4], 0.03 * pred[..., 4:]], -1)      # (t, q): the pose itself
    gt = np.concatenate([rng.uniform(-0.01, 0.01, (B, 3)), np.radians(rng.uniform(-45, 45, (B, 3)))], 1).astype(np.float32)
    shift = rng.uniform(-0.3, 0.3, (B, 3)).astype(np.float32)
    return pred.astype(np.float32), gt, shift


def check_convergence_np(prev_T, T):
    """check_convergenceT (results_itrPCRNet_no_stop.py:155-167) without the threshold"""
    e = T @ np.linalg.inv(prev_T) - np.eye(4)
    return float(np.sum(e * e))


def host_tables(T_all, gt, shift):
    """te, re, ce from the project's float64 host functions (pinned to the reference by tests/golden/pose_cases.npz)"""
    T_all = T_all.astype(np.float64)
    n, B = T_all.shape[:2]
    te, re, ce = np.zeros((n, B)), np.zeros((n, B)), np.ones((n, B))
    for l in range(n):
        fp = R.find_final_pose_inv(T_all[l])
        if shift is not None:
            fp[:, :3] += shift.astype(np.float64)
        for b in range(B):
            te[l, b], re[l, b] = R.find_errors(gt[b].astype(np.float64), fp[b])
            if l:
                ce[l, b] = check_convergence_np(T_all[l - 1, b], T_all[l, b])
    return te, re, ce


@pytest.mark.parametrize("with_shift", [False, True])
@pytest.mark.parametrize("lim_rot", [45.0, 0.0])
@pytest.mark.parametrize("L_,B", [(1, 1), (8, 5), (50, 3)])
def test_trace_tables_match_the_float64_host_functions(L_, B, lim_rot, with_shift):
    """Both sides are double arithmetic on the kernel's own fp32 T_all: 1e-9 (degrees, length units), three orders above ~100 double
    roundings x 57.3.  The host takes acos, so the cases keep the rotation error inside [0.1, 179] degrees (asserted, none dropped)."""
    pred, gt, shift = trace_case(L_, B, lim_rot)
    sh = shift if with_shift else None
    T_all, te, re, ce = regtest.pose_trace(cu(pred), cu(gt), None if sh is None else cu(sh), lim_rot)
    T_all, te, re, ce = (x.cpu().numpy() for x in (T_all, te, re, ce))
    assert T_all.shape == (L_ + 1, B, 4, 4) and T_all.dtype == np.float32 and te.shape == (L_ + 1, B) and te.dtype == np.float64
    assert np.array_equal(T_all[0], np.tile(np.eye(4, dtype=np.float32), (B, 1, 1))) and np.array_equal(T_all[:, :, 3], np.tile(np.float32([0, 0, 0, 1]), (L_ + 1, B, 1)))
    wte, wre, wce = host_tables(T_all, gt, sh)
    assert wre.min() >= 0.1 and wre.max() <= 179.0, (wre.min(), wre.max())
    print("L=%d B=%d lim_rot=%g shift=%s: max |dte| %.3g  |dre| %.3g  |dce| %.3g   (re in [%.2f, %.2f] deg)"
          % (L_, B, lim_rot, with_shift, np.abs(te - wte).max(), np.abs(re - wre).max(), np.abs(ce - wce).max(), wre.min(), wre.max()))
    assert np.abs(te - wte).max() <= 1e-9 and np.abs(re - wre).max() <= 1e-9 and np.abs(ce - wce).max() <= 1e-9
    assert (ce[0] == 1).all()
    # the transforms themselves: the torch restatement of the loop in float64 (registration.compose) on the same raw outputs; a loop's chain
    # is ~16 fp32 roundings deep (quat_normalize 6, the normalisation 2, quaternion -> R 4, the 4-term composition 4) on entries <= max |T|
    T = torch.eye(4, dtype=torch.float64).repeat(B, 1, 1)
    for l in range(L_):
        p = torch.from_numpy(pred[l]).double()
        pose = R.quat_normalize(p, lim_rot) if lim_rot else p
        pose = torch.cat([pose[:, :3], pose[:, 3:7] / pose[:, 3:7].norm(dim=1, keepdim=True).clamp_min(1e-12)], 1)
        T = R.compose(T, pose)
        assert np.abs(T.numpy() - T_all[l + 1]).max() <= 16 * (l + 1) * U * max(1.0, np.abs(T_all[l + 1]).max())
    # any subset of the outputs: the same bits
    d = torch.empty(L_ + 1, B, device="cuda", dtype=torch.float64)
    dp, dg, ds = cu(pred), cu(gt), None if sh is None else cu(sh)         # named: they own the memory until the launch has been read back
    L.check(L.load().dpd_pose_trace(L.ptr(dp), L_, B, lim_rot, L.ptr(dg), None if ds is None else L.ptr(ds), None, None, L.ptr(d), None,
                                    L.cur_stream()), "dpd_pose_trace")
    assert np.array_equal(d.cpu().numpy(), re)


@functools.lru_cache(maxsize=None)
def refined():
    """PoseNet() with seed 0 (untrained), 5 pairs of 64 points, 8 refinements on the library: (net, src, tmpl, gt, T_out, pred_out)"""
    torch.manual_seed(0)
    net = R.PoseNet().cuda()
    src, tmpl, gt = synth.registration_pairs(5, 64, seed=3)
    s, t = cu(src), cu(tmpl)
    with torch.no_grad():
        _, T, pred = R.pose_refine_native(net, s, t, 8, None, want_pred=True)
    return net, s, t, gt, T, pred


def test_trace_repeats_the_refinement_loops_transform_bit_for_bit():
    """dpd_pose_refine's T_out against T_all[L] for the loop's own raw outputs: the same device functions, the same bits."""
    net, s, t, gt, T, pred = refined()
    T_all, _, _, _ = regtest.pose_trace(pred, cu(gt.astype(np.float32)), None, net.lim_rot)
    assert torch.equal(T_all[8].view(torch.int32), T.view(torch.int32))
    assert not torch.equal(T_all[8], T_all[7])


def quat_mul(a, b):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]])


def test_trace_of_the_exact_inverse_has_no_error():
    """T = the inverse of the ground-truth pose (to fp32): here acos is the weak side, so this case is not compared against it."""
    rng = np.random.default_rng(12)
    B = 6
    gt = np.concatenate([rng.uniform(-0.01, 0.01, (B, 3)), np.radians(rng.uniform(-45, 45, (B, 3)))], 1).astype(np.float32)
    pred = np.zeros((1, B, 7), np.float32)
    for b in range(B):
        rx, ry, rz = (float(x) for x in gt[b, 3:])
        ax = lambda th, i: np.array([math.cos(th / 2)] + [math.sin(th / 2) if j == i else 0.0 for j in range(3)])      # noqa: E731
        q = quat_mul(quat_mul(ax(-rz, 2), ax(-ry, 1)), ax(-rx, 0))          # (Rx Ry Rz)^-1 = Rz(-rz) Ry(-ry) Rx(-rx)
        Rg = R.euler_to_mat(rx, ry, rz)
        pred[0, b] = np.concatenate([-Rg.T @ gt[b, :3].astype(np.float64), q])
    _, te, re, ce = regtest.pose_trace(cu(pred), cu(gt), None, 0.0)
    te, re = te.cpu().numpy(), re.cpu().numpy()
    print("exact inverse: max re %.3g deg, max te %.3g" % (re[1].max(), te[1].max()))
    assert re[1].max() < 1e-3 and te[1].max() < 1e-6 and re[0].min() > 1.0


# ---------------------------------------------------------------------------------------------------------------- sqrt-Chamfer

def chamfer_sqrt_f64(a, b, arg_a, arg_b, mask_zero=False):
    """utils/tf_util_loss.py:35-39 in float64 through the given argmins; mask_zero: a coincident pair's term is the constant 0"""
    na = torch.gather(b, 1, arg_a.long()[:, :, None].expand(-1, -1, 3))
    nb = torch.gather(a, 1, arg_b.long()[:, :, None].expand(-1, -1, 3))
    d1, d2 = ((a - na) ** 2).sum(-1), ((b - nb) ** 2).sum(-1)
    if mask_zero:
        r1 = torch.where(d1 > 0, torch.sqrt(torch.where(d1 > 0, d1, torch.ones_like(d1))), torch.zeros_like(d1))
        r2 = torch.where(d2 > 0, torch.sqrt(torch.where(d2 > 0, d2, torch.ones_like(d2))), torch.zeros_like(d2))
    else:
        r1, r2 = torch.sqrt(d1), torch.sqrt(d2)
    return (r1.mean() + r2.mean()) / 2


def chamfer_sqrt_raw(a, b):
    lib = L.load()
    B, N, M = a.shape[0], a.shape[1], b.shape[1]
    o = {"min_a": torch.empty(B, N, device="cuda"), "min_b": torch.empty(B, M, device="cuda"),
         "arg_a": torch.empty(B, N, device="cuda", dtype=torch.int32), "arg_b": torch.empty(B, M, device="cuda", dtype=torch.int32)}
    sq = {k: torch.empty_like(v) for k, v in o.items()}
    loss, loss_sq = torch.empty(1, device="cuda"), torch.empty(1, device="cuda")
    L.check(lib.dpd_chamfer_sqrt_fwd(L.ptr(a), L.ptr(b), B, N, M, L.ptr(o["min_a"]), L.ptr(o["arg_a"]), L.ptr(o["min_b"]), L.ptr(o["arg_b"]),
                                     L.ptr(loss), L.cur_stream()), "dpd_chamfer_sqrt_fwd")
    L.check(lib.dpd_chamfer_fwd(L.ptr(a), L.ptr(b), B, N, M, L.ptr(sq["min_a"]), L.ptr(sq["arg_a"]), L.ptr(sq["min_b"]), L.ptr(sq["arg_b"]),
                                L.ptr(loss_sq), L.cur_stream()), "dpd_chamfer_fwd")
    return o, sq, loss


@pytest.mark.parametrize("B,N,M", [(2, 64, 64), (3, 100, 37), (1, 1, 1)])
def test_chamfer_sqrt_against_float64_autograd(B, N, M):
    """Loss: relative n 2^-24, n = B (N + M) square roots in the two means.  Gradients: 8 x 2^-24 x max |grad| per entry (one
    rsqrt-class division and three multiplies)."""
    rng = np.random.default_rng(21)
    a, b = cu(rng.uniform(-1, 1, (B, N, 3)).astype(np.float32)), cu(rng.uniform(-1, 1, (B, M, 3)).astype(np.float32))
    o, sq, _ = chamfer_sqrt_raw(a, b)
    for k in o:                 # the squared form's minima and indices, bit for bit
        assert torch.equal(o[k].view(torch.int32), sq[k].view(torch.int32)), k
    ag, bg = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    loss = regtest.chamfer_sqrt(ag, bg)
    da, db = torch.autograd.grad(loss * 3.0, [ag, bg])
    a64, b64 = a.double().requires_grad_(True), b.double().requires_grad_(True)
    want = chamfer_sqrt_f64(a64, b64, o["arg_a"], o["arg_b"])
    wa, wb = torch.autograd.grad(want * 3.0, [a64, b64])
    rel = abs(loss.item() - want.item()) / want.item()
    ea, eb = (da.double() - wa).abs().max().item(), (db.double() - wb).abs().max().item()
    print("B=%d N=%d M=%d: loss rel err %.3g (bar %.3g)  grad err a %.3g (bar %.3g)  b %.3g (bar %.3g)"
          % (B, N, M, rel, B * (N + M) * U, ea, 8 * U * wa.abs().max().item(), eb, 8 * U * wb.abs().max().item()))
    assert rel <= B * (N + M) * U
    assert ea <= 8 * U * wa.abs().max().item() and eb <= 8 * U * wb.abs().max().item()
    only_a, = torch.autograd.grad(regtest.chamfer_sqrt(ag, b) * 3.0, [ag])          # one gradient asked for: the same bits
    assert torch.equal(only_a, da)


def test_chamfer_sqrt_coincident_points_contribute_zero():
    """DEVIATION from the reference, as documented: where a minimum is 0 its gradient is inf * 0 = NaN; here exactly zero."""
    rng = np.random.default_rng(22)
    a = rng.uniform(-1, 1, (2, 64, 3)).astype(np.float32)
    b = rng.uniform(-1, 1, (2, 64, 3)).astype(np.float32)
    a[0, 0] = 5.0               # outside the cube, >= 4 sqrt(3) from every other point, whose own nearest neighbour is <= 2 sqrt(3) away:
    b[0, 0] = a[0, 0]           # the coincident pair is nobody else's nearest neighbour
    ag, bg = cu(a).requires_grad_(True), cu(b).requires_grad_(True)
    o, _, _ = chamfer_sqrt_raw(ag.detach(), bg.detach())
    assert o["min_a"][0, 0] == 0 and o["min_b"][0, 0] == 0 and o["arg_a"][0, 0] == 0 and o["arg_b"][0, 0] == 0
    da, db = torch.autograd.grad(regtest.chamfer_sqrt(ag, bg), [ag, bg])
    assert torch.isfinite(da).all() and torch.isfinite(db).all()
    a64, b64 = ag.detach().double().requires_grad_(True), bg.detach().double().requires_grad_(True)
    ra, rb = torch.autograd.grad(chamfer_sqrt_f64(a64, b64, o["arg_a"], o["arg_b"]), [a64, b64])
    assert torch.isnan(ra[0, 0]).all() and torch.isnan(rb[0, 0]).all()          # the raw formula does give NaN there
    wa, wb = torch.autograd.grad(chamfer_sqrt_f64(a64, b64, o["arg_a"], o["arg_b"], mask_zero=True), [a64, b64])
    assert (da.double() - wa).abs().max() <= 8 * U * wa.abs().max() and (db.double() - wb).abs().max() <= 8 * U * wb.abs().max()
    # the two points carry that pair's term alone: exactly zero
    assert not (o["arg_b"][0, 1:] == 0).any() and not (o["arg_a"][0, 1:] == 0).any()
    assert (da[0, 0] == 0).all() and (db[0, 0] == 0).all()
    one = cu(a[:1, :1])          # a single coincident pair: everything is exactly zero
    oa, ob = one.clone().requires_grad_(True), one.clone().requires_grad_(True)
    l1 = regtest.chamfer_sqrt(oa, ob)
    g1a, g1b = torch.autograd.grad(l1, [oa, ob])
    assert l1.item() == 0 and (g1a == 0).all() and (g1b == 0).all()


# ------------------------------------------------------------------------------------------------------------------- protocol

def test_no_stop_test_end_to_end():
    """5 pairs in batches of 2 (a partial last batch), 3 iterations of the untrained network: shapes, row 0 = the identity's errors, the
    last row = the per-pair host path on IterativeRegistration.evaluate's T (the same refinements, the same bits; 1e-9), occlusion with a
    fixed generator is repeatable and changes the result.  Ground-truth poses are float32 at the entry: both sides get those values."""
    from dpdist_amd.aue import chamfer_dist
    torch.manual_seed(0)
    net = R.PoseNet().cuda()
    src, tmpl, gt = synth.registration_pairs(5, 64, seed=3)
    gt = gt.astype(np.float32).astype(np.float64)
    res = regtest.no_stop_test(net, src, tmpl, gt, iterations=3, batch=2)
    TE, RE, CE = res["TE"], res["RE"], res["CE"]
    assert TE.shape == RE.shape == CE.shape == (4, 5) and TE.dtype == np.float64 and res["T"].shape == (5, 4, 4) and res["pairs"] == 5
    ident = np.array([R.find_errors(gt[i], np.zeros(6)) for i in range(5)])
    assert np.abs(TE[0] - ident[:, 0]).max() <= 1e-9 and np.abs(RE[0] - ident[:, 1]).max() <= 1e-9 and (CE[0] == 1).all()
    reg = R.IterativeRegistration(net, lambda m, t: chamfer_dist(m, t), max_loops=3, graph=False)
    es, et = cu(src), cu(tmpl)
    errs = []
    for i in range(0, 5, 2):          # tools/registration_demo.py's per-pair loop as it was before the protocol ran on the device
        _, T = reg.evaluate(es[i:i + 2], et[i:i + 2])
        assert np.array_equal(T.cpu().numpy(), res["T"][i:i + 2])
        fp = R.find_final_pose_inv(T.double().cpu().numpy())
        errs += [R.find_errors(gt[i + j], fp[j]) for j in range(fp.shape[0])]
    reg.close()
    errs = np.array(errs)
    print("protocol: max |dTE| %.3g  max |dRE| %.3g" % (np.abs(TE[-1] - errs[:, 0]).max(), np.abs(RE[-1] - errs[:, 1]).max()))
    assert np.abs(TE[-1] - errs[:, 0]).max() <= 1e-9 and np.abs(RE[-1] - errs[:, 1]).max() <= 1e-9
    assert res["buckets"] == regtest.buckets(TE[-1], RE[-1]) and np.array_equal(res["per_iteration"]["rot_mean"], RE.mean(1))
    assert res["pairs_per_s"] > 0
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    occ1 = regtest.no_stop_test(net, src, tmpl, gt, iterations=3, batch=2, occlusions=0.25, generator=g)
    g.manual_seed(5)
    occ2 = regtest.no_stop_test(net, src, tmpl, gt, iterations=3, batch=2, occlusions=0.25, generator=g)
    for k in ("TE", "RE", "CE"):
        assert np.array_equal(occ1[k], occ2[k])
    assert np.array_equal(occ1["RE"][0], RE[0]) and not np.array_equal(occ1["RE"][1:], RE[1:])
    cen = regtest.no_stop_test(net, src, tmpl, gt, iterations=3, batch=2, noise=True, centroid_sub=True, generator=g)
    assert np.abs(cen["shift"] - src.mean(1)).max() <= 1e-6 and np.isfinite(cen["RE"]).all()
    assert np.abs(cen["RE"][0] - RE[0]).max() <= 1e-9          # the identity's rotation error does not see the shift ...
    want0 = [R.find_errors(gt[i], np.concatenate([cen["shift"][i].astype(np.float64), np.zeros(3)]))[0] for i in range(5)]
    assert np.abs(cen["TE"][0] - want0).max() <= 1e-9          # ... its translation error does (get_error adds the centroid)


def test_no_stop_test_refuses_a_network_the_library_does_not_implement():
    torch.manual_seed(0)
    net = R.PoseNet(out_features=512).cuda()
    src, tmpl, gt = synth.registration_pairs(2, 64, seed=3)
    with pytest.raises(RuntimeError, match="no torch fallback"):
        regtest.no_stop_test(net, src, tmpl, gt, iterations=2, batch=2)

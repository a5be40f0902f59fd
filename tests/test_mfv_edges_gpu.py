"""The 3DmFV encoder (dpdist_amd/csrc/mfv3d.hip) against the float64 oracle at the shapes its index arithmetic branches on: both
forward kernels (N % 8 == 0 or not), N < 8, m a power of two or not, Gaussian slices that are short (m = 3, 5, 7, 9) or empty (m = 1),
point slices of the sliced backward that are empty (N = 9) or hold one point (N = 10, 13), ties that span point slices, every kernel
above 64 KiB of dynamic LDS in ascending order in a fresh process, the 160 KiB cap and the refusals.  Cases, references, bars and
checkers: tests/mfv_cases.py (tests/test_mfv_edges_cpu.py shows on the CPU that they can fail).  Outputs and workspaces sit in
NaN-payload guard bands that must come back untouched."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import restate as R

from . import mfv_cases as M

pytestmark = pytest.mark.gpu

E_DIM, E_UNSUPPORTED = -2, -3


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


# ------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("case", M.FWD_CASES + M.TIE_CASES, ids=_id)
def test_forward_vs_float64(dev, case):
    rc, fv, band = M.gpu_forward(_cu(M.points(case), dev), case[3], case[4])
    assert rc == 0
    M.check_forward(fv, band, M.forward_ref(case), case[3], case)


@pytest.mark.parametrize("m", [5, 8])
def test_both_forward_kernels_agree_through_the_oracle(dev, m):
    """N = 16 runs the pair kernel, N = 17 (point 0 once more) the eight-group kernel.  In the oracle the max / min channels of the two
    clouds are equal (tests/test_mfv_edges_cpu.py::test_n16_and_n17_share_their_extrema); each kernel is held to its own oracle, and
    on those channels to the other's as well."""
    p16 = M.points(("u", 3, 16, 7, M.S0))
    p17 = np.concatenate([p16, p16[:, :1]], 1)
    assert M.uses_fwd2(16) and not M.uses_fwd2(17)
    ch = list(M.MAXMIN_CHANNELS)
    out = []
    for p in (p16, p17):
        ref = M.make_ref(p, m, M.S0)
        M.check_conditioning(ref, (m, p.shape[1]))
        rc, fv, band = M.gpu_forward(_cu(p, dev), m, M.S0)
        assert rc == 0
        M.check_forward(fv, band, ref, m, ("16 against 17", m, p.shape[1]))
        out.append((fv.cpu().numpy().astype(np.float64), ref))
    (a, ra), (b, rb) = out
    assert np.abs(ra.fv64[..., ch] - rb.fv64[..., ch]).max() <= 1e-12
    assert np.abs(a[..., ch] - rb.fv64[..., ch]).max() <= ra.bar and np.abs(b[..., ch] - ra.fv64[..., ch]).max() <= rb.bar


@pytest.mark.parametrize("case", M.FRONT_CASES, ids=_id)
def test_fused_front_end_at_uneven_splits(dev, case):
    """dpd_mfv3d_fwd_stacked leaves fv without its L2 norm and the per-slice sums of squares in ssq; dpd_patch_rows_fwd_scaled applies
    the norm while gathering.  Both against float64: fv * rsqrt(sum of the slices) and the window columns of X at the forward bar."""
    from dpdist_amd import lib as L
    lib, s = L.load(), L.cur_stream()
    _, _, N, m, sigma = case
    k, B, C, G = 5, 1, 2, m ** 3
    KP, E = lib.dpd_padded_width(k), k * k * k * M.F
    p, ref = M.points(case), M.forward_ref(case)
    pcA, pcB = _cu(p[:1], dev), _cu(p[1:], dev)
    (pts, b_pts), (q, b_q), (fv, b_fv), (ssq, b_ssq) = (M.banded_flat(n, device=dev) for n in (C * N * 3, C * N * 3, C * G * M.F, C * M.SLICES * M.F))
    (X, b_X), (mask, b_mask) = M.banded_flat(C * N * KP, device=dev), M.banded_flat(C * N, device=dev)
    vox = torch.full((C * N,), -1, device=dev, dtype=torch.int32)
    assert lib.dpd_mfv3d_fwd_stacked(L.ptr(pcA), L.ptr(pcB), None, B, N, m, sigma, L.ptr(pts), L.ptr(q), L.ptr(fv), L.ptr(ssq), s) == 0
    assert lib.dpd_patch_rows_fwd_scaled(L.ptr(q), L.ptr(fv), L.ptr(ssq), C, N, m, k, KP, L.ptr(X), L.ptr(mask), L.ptr(vox), None, s) == 0
    torch.cuda.synchronize()
    for b in (b_pts, b_q, b_fv, b_ssq, b_X, b_mask):
        b()
    assert np.array_equal(pts.view(C, N, 3).cpu().numpy(), p) and np.array_equal(q.view(C, N, 3).cpu().numpy(), p[::-1])
    # the per-slice norms: slices added in order, as the gather does
    ssq_h, fv_h = ssq.view(C, M.SLICES, M.F).cpu().double().numpy(), fv.view(C, G, M.F).cpu().double().numpy()
    assert np.isfinite(ssq_h).all() and (ssq_h[:, [s_ for s_, n in enumerate(M.gauss_slices(m)) if n == 0]] == 0).all()
    normed = fv_h / np.sqrt(np.maximum(ssq_h.sum(1), 1e-12))[:, None, :]
    err = np.abs(normed - ref.fv64).max()
    print("front end %s: fv err %.3g bar %.3g" % (case, err, ref.bar))
    assert err <= ref.bar
    for c in range(C):       # every slice's own sum of squares, against the un-normalised values it covers
        g0 = 0
        for s_, n in enumerate(M.gauss_slices(m)):
            want = (fv_h[c, g0:g0 + n] ** 2).sum(0)
            assert np.abs(ssq_h[c, s_] - want).max() <= 1e-5 * max(1.0, want.max()), (c, s_)
            g0 += n
    # the rows: queries [pcB ; pcA] look up the windows of [pcA ; pcB]
    qh = torch.tensor(np.ascontiguousarray(p[::-1]))
    v, msk, loc = R.voxel_lookup(qh, m)
    emb = R.local_window(torch.tensor(ref.fv64), m, k)
    rows = torch.gather(emb, 1, v[..., None].expand(-1, -1, emb.shape[-1])).reshape(C * N, -1).numpy()
    Xh = X.view(C * N, KP).cpu().numpy()
    assert msk.all() and np.array_equal(mask.cpu().numpy(), msk.reshape(-1).numpy())
    assert np.array_equal(vox.cpu().numpy().astype(np.int64), v.reshape(-1).numpy())
    errX = np.abs(Xh[:, :E].astype(np.float64) - rows).max()
    print("front end %s: X err %.3g" % (case, errX))
    assert errX <= ref.bar
    assert np.array_equal(Xh[:, E:E + 3], loc.reshape(-1, 3).numpy()) and not Xh[:, E + 3:].any()


# ------------------------------------------------------------------------------------------------ backward
def _backward_both(dev, p, ref, m, sigma, what):
    """sliced and one-launch on clouds p against ref; returns the two gradients"""
    N = p.shape[1]
    pts, dfv = _cu(p, dev), _cu(ref.dfv, dev)
    rc, g_s, bands_s, ws = M.gpu_backward(pts, dfv, m, sigma, True)
    assert rc == 0
    rc, g_1, bands_1, _ = M.gpu_backward(pts, dfv, m, sigma, False)
    assert rc == 0
    if M.takes_sliced(N):
        assert not M.untouched(ws)
    else:       # fewer than two points per slice: the entry runs the one-launch kernel, workspace or not
        assert M.untouched(ws) and torch.equal(g_s, g_1)
    M.check_backward(g_1, bands_1, ref, (what, "one launch"))
    M.check_backward(g_s, bands_s, ref, (what, "sliced"))
    M.check_forms_agree(g_s, g_1, ref.scale, what)
    return g_s, g_1


@pytest.mark.parametrize("case", M.BWD_CASES, ids=_id)
def test_backward_vs_float64(dev, case):
    _backward_both(dev, M.points(case), M.backward_ref(case), case[3], case[4], case)


@pytest.mark.parametrize("case", M.TIE_CASES, ids=_id)
def test_ties_across_point_slices(dev, case):
    """every copy of a point sits in another point slice (another workgroup of the sliced form): the share of a max / min gradient is
    1 / (ties in the CLOUD), as float64 autograd splits it, and the copies of a point receive the same bits"""
    idx = torch.tensor(M.tie_partner(case[0], case[2]), device=dev)
    for g in _backward_both(dev, M.points(case), M.backward_ref(case), case[3], case[4], case):
        assert torch.equal(g[:, idx], g)


@pytest.mark.parametrize("case", [("u", 2, 50, 5, M.S0), ("u", 2, 10, 8, M.S0), ("u", 2, 13, 3, M.S0)], ids=_id)
def test_backward_permutation(dev, case):
    """permuting the points permutes dpts, also when points change their slice"""
    _, C, N, m, sigma = case
    assert case in M.BWD_CASES
    ref, p = M.backward_ref(case), M.points(case)
    ns = (N + M.SLICES - 1) // M.SLICES
    for perm in (np.random.default_rng([3, N]).permutation(N), np.arange(N)[::-1].copy()):
        assert (perm // ns != np.arange(N) // ns).any()
        pts, dfv = _cu(p, dev), _cu(ref.dfv, dev)
        for sliced in (True, False):
            rc, g, bands, _ = M.gpu_backward(pts, dfv, m, sigma, sliced)
            rc2, gp, bands_p, _ = M.gpu_backward(_cu(p[:, perm], dev), dfv, m, sigma, sliced)
            assert rc == 0 and rc2 == 0
            bands(), bands_p()
            M.check_forms_agree(gp, g[:, torch.tensor(perm, device=dev)], ref.scale, (case, sliced))


# ------------------------------------------------------------------------------------------------ dynamic LDS
def test_larger_lds_after_smaller_in_a_fresh_process(dev):
    """tests/mfv_lds_child.py: every encoder kernel that can need more than 64 KiB of dynamic LDS, a smaller size first and a larger one
    after it, in a process that has launched nothing before; every result against float64"""
    M.check_lds_plan()
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "mfv_lds_child.py")
    r = subprocess.run([sys.executable, child], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    calls = len(M.LDS_FWD2 + M.LDS_FWD), len(M.LDS_BWD_ONE + M.LDS_BWD_SLICED)
    assert r.stdout.rstrip().endswith("LDS-CHILD-OK") and (r.stdout.count("forward ("), r.stdout.count("backward (")) == calls


@pytest.mark.parametrize("case", M.CAP_CASES, ids=_id)
def test_forward_at_the_lds_cap(dev, case):
    """the largest N that fits 160 KiB runs and matches; the next N that the same kernel takes is refused before anything is launched"""
    _, _, N, m, sigma = case
    fwd2 = M.uses_fwd2(N)
    assert M.fwd_lds_bytes(N, m) <= M.LDS_CAP
    rc, fv, band = M.gpu_forward(_cu(M.points(case), dev), m, sigma)
    assert rc == 0
    M.check_forward(fv, band, M.forward_ref(case), m, (case, M.fwd_lds_bytes(N, m)))
    above = N + (8 if fwd2 else 1)
    assert M.fwd_lds_bytes(above, m) > M.LDS_CAP and (not fwd2 or M.uses_fwd2(above))
    rc, fv, band = M.gpu_forward(torch.zeros(1, above, 3, device=dev), m, sigma)
    assert rc == E_UNSUPPORTED, rc
    assert M.untouched(fv)
    band()


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_the_outputs_untouched(dev):
    from dpdist_amd import lib as L
    lib = L.load()
    pts = torch.zeros(2, 16, 3, device=dev)
    nan = float("nan")
    for kw, want in (({"m": 0}, E_UNSUPPORTED), ({"m": 11}, E_UNSUPPORTED), ({"N": 0}, E_UNSUPPORTED), ({"N": 4097}, E_UNSUPPORTED),
                     ({"sigma": 0.0}, E_DIM), ({"sigma": -1.0}, E_DIM), ({"sigma": nan}, E_DIM), ({"C": 0}, E_DIM)):
        a = dict({"m": 8, "sigma": M.S0, "C": None, "N": None}, **kw)
        rc, fv, band = M.gpu_forward(pts, a["m"], a["sigma"], C=a["C"], N=a["N"])
        assert rc == want and M.untouched(fv), ("forward", kw, rc)
        band()
        if a["m"] != 0:
            dfv = torch.zeros(2, a["m"] ** 3, M.F, device=dev)
            for sliced in (True, False):
                rc, g, bands, ws = M.gpu_backward(pts, dfv, a["m"], a["sigma"], sliced, C=a["C"], N=a["N"])
                assert rc == want and M.untouched(g) and (ws is None or M.untouched(ws)), ("backward", kw, sliced, rc)
                bands()
    # the backward keeps one Gaussian per lane pair: m = 9 is beyond it (the forward takes it)
    dfv = torch.zeros(2, 729, M.F, device=dev)
    for sliced in (True, False):
        rc, g, bands, ws = M.gpu_backward(pts, dfv, 9, M.S0, sliced)
        assert rc == E_UNSUPPORTED and M.untouched(g) and (ws is None or M.untouched(ws))
        bands()
    # the three-launch as-loss tail has no one-launch form to fall back to: fewer than 8 points are the caller's to route
    B, N, m, k = 1, 7, 8, 5
    KP = lib.dpd_padded_width(k)
    dX, vox, p7 = torch.zeros(2 * B * N, KP, device=dev), torch.zeros(2 * B * N, device=dev, dtype=torch.int32), torch.zeros(2 * B, N, 3, device=dev)
    ws_bytes = lib.dpd_mfv3d_bwd_workspace_bytes(2 * B, m)
    outs = [M.banded_flat(n, device=dev) for n in (2 * B * m ** 3 * M.F, ws_bytes // 4, B * N * 3, B * N * 3)]
    (dfv7, _), (ws7, _), (gA, _), (gB, _) = outs
    rc = lib.dpd_asloss_tail(L.ptr(dX), L.ptr(vox), L.ptr(p7), None, B, N, m, k, KP, M.S0, L.ptr(dfv7), L.ptr(ws7), ws_bytes, L.ptr(gA), L.ptr(gB),
                             L.cur_stream())
    torch.cuda.synchronize()
    assert rc == E_UNSUPPORTED
    for view, band in outs:
        assert M.untouched(view)
        band()

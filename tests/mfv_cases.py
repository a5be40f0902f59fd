"""Encoder (3DmFV) edge cases against the float64 oracle: case tables, seeded input builders, the references and the checkers of
tests/test_mfv_edges_gpu.py (tests/test_mfv_edges_cpu.py proves on the CPU that the checkers can fail and that every case is well
conditioned in the oracle itself).  Not a test module and not a conftest.

The method: oracle.restate.mfv3d in float64 is the reference; the same oracle in float32 measures how far fp32 arithmetic of the SAME
formula sits from it on the SAME input (the conditioning of the case).  A forward case is admitted only when that distance is below the
encoder's bar of 3e-6 and no entry below 1e-6 changes sign; the kernel is then held to max(3e-6, 4 x that distance).  One missing or
double-counted point moves a statistic by about 1/N of its value and one missing Gaussian moves a channel norm by about 1/G, both
orders of magnitude above the bar at the sizes used here.  The backward bar is the one of test_mfv3d_backward_vs_oracle: the upstream
gradient is zeroed where |fv64| < 2e-3 (the power-1/2 normalisation amplifies round-off without bound at 0), and per cloud
err <= max(1e-4 x scale, 10 x the float32 autograd oracle's own distance from float64), scale = max(1, |ref|.max()).
"""
import collections
import functools
import math

import numpy as np
import torch

from oracle import restate as R

from .gemm_cases import FLAT_BAND, NAN_OUT, banded_flat, untouched  # noqa: F401  (re-exported for the two test modules)

F = R.F_PER_G
SLICES = 4                 # DPD_MFV_SLICES: Gaussian slices of the forward, point slices of the sliced backward
FWD_BAR = 3e-6             # the project's encoder bar (test_mfv3d_golden)
SIGN_FLOOR = 1e-6          # no |fv| below this may change sign between the float32 and the float64 oracle
NORM_TOL = 1e-5            # unit L2 norm over the Gaussian axis
DFV_FLOOR = 2e-3           # upstream gradient zeroed where |fv64| is below this
BWD_REL = 1e-4             # backward bar and sliced-against-one-launch bar, times scale
LDS_OPT_IN = 64 * 1024     # dynamic LDS above this needs the per-kernel attribute
LDS_CAP = 160 * 1024       # and above this the entry refuses
MAXMIN_CHANNELS = (1, 5, 6, 7, 8, 9, 10, 14, 15, 16, 17, 18, 19)


# ------------------------------------------------------------------------------------------------ the host's size rules, restated
def gauss_slices(m):
    """Gaussians per forward workgroup: gslice = ceil(G / 4); m = 5 -> [32, 32, 32, 29], m = 3 -> [7, 7, 7, 6], m = 1 -> [1, 0, 0, 0]"""
    G = m ** 3
    gs = (G + SLICES - 1) // SLICES
    return [max(0, min(G, (s + 1) * gs) - s * gs) for s in range(SLICES)]


def point_slices(N):
    """points per workgroup of the sliced backward: nslice = ceil(N / 4); N = 9 -> [3, 3, 3, 0], N = 10 -> [3, 3, 3, 1]"""
    ns = (N + SLICES - 1) // SLICES
    return [max(0, min(N, (s + 1) * ns) - min(N, s * ns)) for s in range(SLICES)]


def uses_fwd2(N):
    """the pair-of-points forward kernel takes N % 8 == 0, the eight-point-group kernel everything else"""
    return N >= 8 and N % 8 == 0


def takes_sliced(N):
    """the sliced backward needs two points per slice on average; below that the entry runs the one-launch kernel"""
    return N >= 2 * SLICES


def fwd_lds_bytes(N, m):
    return (6 * N * m + 6 * N + ((m ** 3 + SLICES - 1) // SLICES) * (F + 1) + 4 + 8 * F) * 4


def bwd_lds_bytes(N, m):
    return (6 * N * m + 3 * N + 16 * 2 * F + 2 * F + N + 16 * N * 3 + 4) * 4


def bwd_sliced_lds_bytes(N, m):
    """(statistics kernel, apply kernel)"""
    ns = (N + SLICES - 1) // SLICES
    return (6 * ns * m + 3 * ns + 4) * 4, (6 * ns * m + 3 * ns + ns + 16 * ns * 3 + 4) * 4


def largest_fwd_n(m, fwd2):
    """largest N whose forward LDS fits the cap, among the N that the chosen forward kernel takes"""
    N = 4096
    while N > 0 and (fwd_lds_bytes(N, m) > LDS_CAP or uses_fwd2(N) != fwd2):
        N -= 1
    return N


# ------------------------------------------------------------------------------------------------ case tables
# Forward: (kind, C, N, m, sigma); kind "u" = uniform in [-0.8, 0.8]^3, "b" = boundary cloud (grid centres and cell faces).
# Every N class (below 8 / the fwd2 kernel / the eight-group kernel, power of two or not) meets an m whose Gaussians split unevenly
# over the four slices (m = 1: 1,0,0,0; 3: 7,7,7,6; 5: 32,32,32,29; 7: 86,86,86,85; 9: 183,183,183,180) and an m that is a power of two
# (1, 2, 4, 8); m = 10 is the even split that is no power of two and the largest table.  m = 1 is FORWARD ONLY: its Q - w is exactly 0
# and the gradient of the power normalisation is undefined there.
S0 = 0.125
_U = (
    (2, 1, 3), (2, 1, 8), (1, 1, 1),
    (2, 2, 5), (2, 2, 4),
    (3, 7, 7), (3, 7, 8), (2, 7, 1),
    (3, 8, 3), (3, 8, 8), (2, 8, 10),
    (3, 9, 5), (3, 9, 2), (2, 9, 9),
    (3, 10, 9), (3, 10, 4),
    (3, 13, 3), (3, 13, 8),
    (3, 16, 7), (3, 16, 2), (2, 16, 1),
    (3, 50, 5), (3, 50, 8), (2, 50, 10),
    (2, 63, 9), (2, 63, 4),
    (5, 64, 3), (2, 64, 8), (2, 64, 7), (1, 64, 10),
    (2, 65, 5), (2, 65, 8),
    (2, 100, 7), (2, 100, 2), (2, 100, 10), (2, 100, 9),
)
_SIGMA_SHAPES = ((2, 50, 5), (2, 64, 8))          # the two shapes that also run sigma = 0.0625 and 0.25
BOUNDARY_N = {1: 9, 2: 10, 3: 13, 4: 16, 5: 50, 7: 63, 8: 64, 9: 65, 10: 100}
FWD_CASES = tuple([("u", C, N, m, S0) for C, N, m in _U] +
                  [("u", C, N, m, s) for C, N, m in _SIGMA_SHAPES for s in (0.0625, 0.25)] +
                  [("b", 1, N, m, S0) for m, N in BOUNDARY_N.items()])

# Backward: (kind, C, N, m, sigma), m <= 8 (the entry refuses m = 9), no m = 1 (above).  Each runs sliced and one-launch; N < 8 must
# take the one-launch kernel in both.  N = 9: an empty point slice (3,3,3,0); 10 and 13: a one-point last slice; 50: 13,13,13,11.
BWD_CASES = tuple(("u", C, N, m, S0) for C, N, m in (
    (2, 7, 3), (2, 7, 8),
    (2, 8, 5), (2, 8, 2),
    (3, 9, 3), (2, 9, 8),
    (3, 10, 5), (2, 10, 8), (2, 10, 2),
    (2, 13, 3), (2, 13, 8),
    (2, 50, 5), (2, 50, 8), (2, 50, 3),
    (2, 64, 5), (2, 64, 8), (2, 64, 2),
    (2, 100, 3), (2, 100, 8),
))
# Ties across slices: (kind, 1, N, m, sigma).  "t2": every point has a copy nslice or more indices away (N = 13: index 12 is a THIRD copy
# of point 0, alone in the last slice), so every extremum is a tie that spans workgroups; "t1": twelve distinct points and the copy of
# point 0 alone in the one-point last slice, so only the extrema that point 0 attains are ties.
TIE_CASES = tuple([("t2", 1, N, m, S0) for N, m in ((10, 5), (13, 3), (50, 8), (64, 5))] + [("t1", 1, 13, 8, S0), ("t1", 1, 13, 5, S0)])

# The fused front end (dpd_mfv3d_fwd_stacked with per-slice sums of squares + dpd_patch_rows_fwd_scaled) at short Gaussian slices and
# ragged N: cloud 0 is pcA, cloud 1 is pcB (B = 1).  The largest N whose forward LDS fits the 160 KiB cap, per forward kernel.
FRONT_CASES = tuple(("u", 2, N, m, S0) for m in (3, 5) for N in (9, 50))
CAP_CASES = tuple(("u", 1, largest_fwd_n(m, fwd2), m, S0) for m in (8, 10) for fwd2 in (True, False))

# seeds replaced because the float32 oracle of the cloud they gave missed the conditioning bar (tests/test_mfv_edges_cpu.py)
RESEED = {("u", 3, 9, 2, S0): 1, ("u", 3, 16, 2, S0): 2, ("u", 2, 10, 2, S0): 2,      # m = 2: a channel whose eight values all sit below the 1e-12 clamp
          ("b", 1, 10, 2, S0): 1, ("b", 1, 13, 3, S0): 1,                              # a statistic that cancels to 0 over a symmetric lattice
          ("b", 1, 16, 4, S0): 2, ("b", 1, 50, 5, S0): 3}                              # the same, seen only between two fp32 roundings of Q


def tie_partner(kind, N):
    """index of the original of every point (itself for an original)"""
    idx = np.arange(N)
    if kind == "t2":
        h = N // 2
        idx[h:2 * h] = np.arange(h)
        if N % 2:
            idx[N - 1] = 0
        assert h >= (N + SLICES - 1) // SLICES          # the copy never shares a point slice with its original
    elif kind == "t1":
        idx[N - 1] = 0
    return idx


def boundary_coords(m):
    """Coordinates of a boundary cloud: the m - 1 faces between the cells and every centre that float32 holds as float64 does (all of
    them for m = 1, 2, 4, 8; the middle one for odd m; +-0.5 for m = 10).  A point ON a centre that float32 rounds has z = 0 exactly in
    fp32 (the kernel's centres are the rounded ones) and z ~ 3e-7 in float64; where that point attains a max / min statistic the
    power-1/2 normalisation turns the difference into 1e-4 of fv.  That is the conditioning of the input, not an edge of the kernel,
    and no seed gets such a cloud past the float32 oracle (m = 3, 5, 7, 9: 12 of 12 seeds fail), so those centres are left out."""
    l = R.grid_axis(m)
    centres = [x for x in l if abs(float(np.float32(x)) - x) <= 1e-9 * abs(x)]
    return np.concatenate([centres, l[:-1] + 1.0 / m]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def points(case):
    """the case's clouds [C, N, 3] float32 (read-only)"""
    kind, C, N, m, sigma = case
    rng = np.random.default_rng([RESEED.get(case, 0), "ubt".index(kind[0]), C, N, m, int(round(sigma * 1e4))])
    if kind == "b":
        coords = boundary_coords(m)
        p = coords[rng.integers(0, coords.size, size=(C, N, 3))]
    else:
        p = rng.uniform(-0.8, 0.8, size=(C, N, 3)).astype(np.float32)
        if kind[0] == "t":
            p = p[:, tie_partner(kind, N)]
    p = np.ascontiguousarray(p, dtype=np.float32)
    p.setflags(write=False)
    return p


# ------------------------------------------------------------------------------------------------ references
FwdRef = collections.namedtuple("FwdRef", "fv64 fv32 d32 bar d32f", defaults=(None,))
BwdRef = collections.namedtuple("BwdRef", "dfv g64 g32 err32 scale bar")


def forward_bar(d32):
    return max(FWD_BAR, 4.0 * d32)


def factorised(p, m, sigma, dt=torch.float32):
    """The oracle's formula with the responsibility in its product form: the Gaussians have diagonal covariance on a product grid, so
    Q_ng = (ex[n][j] / Sx[n]) (ey[n][i] / Sy[n]) (ez[n][t] / Sz[n]), e_a[n][i] = exp(-z_a^2 / 2) -- algebraically the oracle's Q (in
    float64 the two agree to 1e-14, tests/test_mfv_edges_cpu.py), in float32 another legitimate rounding of it.  A case whose fv moves
    by more than the bar between two fp32 roundings of Q holds a statistic that cancels (a lattice cloud whose mean Q equals w for some
    Gaussian, say): the power-1/2 normalisation amplifies the last bits of Q there, and no fp32 kernel can be judged on it."""
    x = torch.tensor(p, dtype=dt)
    C, N, _ = x.shape
    G, w = m ** 3, 1.0 / m ** 3
    z = (x[..., None] - torch.tensor(R.grid_axis(m), dtype=dt)) / sigma            # [C, N, 3, m]
    e = torch.exp(-0.5 * z * z)
    q = e / e.sum(-1, keepdim=True)
    zx, zy, zz = z[:, :, 0, None, :, None], z[:, :, 1, :, None, None], z[:, :, 2, None, None, :]     # g = i m m + j m + t: (l[j], l[i], l[t])
    Q = ((q[:, :, 0, None, :, None] * q[:, :, 1, :, None, None]) * q[:, :, 2, None, None, :]).reshape(C, N, G)
    zg = torch.stack([a.expand(C, N, m, m, m) for a in (zx, zy, zz)], -1).reshape(C, N, G, 3)
    d_pi_all = (Q - w) / (math.sqrt(w) * N)
    d_pi = torch.stack([d_pi_all.mean(1), d_pi_all.amax(1)], -1)
    a, b = Q[..., None] * zg, Q[..., None] * (zg * zg - 1)
    d_mu = torch.cat([a.mean(1), a.amax(1), a.amin(1)], -1) * (1.0 / math.sqrt(w))
    d_sig = torch.cat([b.mean(1), b.amax(1), b.amin(1)], -1) * (1.0 / math.sqrt(2 * w))

    def norm(v):
        v = torch.sign(v) * torch.sqrt(torch.clamp_min(torch.abs(v), 1e-12))
        return v * torch.rsqrt(torch.clamp_min((v * v).sum(1, keepdim=True), 1e-12))

    return torch.cat([norm(d_pi), norm(d_mu), norm(d_sig)], -1).numpy()


def oracle_forward(p, m, sigma):
    """(fv64, fv32, distance) of float32 clouds p"""
    fv64 = R.mfv3d(torch.tensor(p, dtype=torch.float64), m, sigma).numpy()
    fv32 = R.mfv3d(torch.tensor(p, dtype=torch.float32), m, sigma).numpy()
    return fv64, fv32, float(np.abs(fv32.astype(np.float64) - fv64).max())


def make_ref(p, m, sigma):
    """references and conditioning figures of clouds p; the bar comes from the float32 ORACLE's distance alone"""
    fv64, fv32, d32 = oracle_forward(p, m, sigma)
    d32f = float(np.abs(factorised(p, m, sigma).astype(np.float64) - fv64).max())
    return FwdRef(fv64, fv32, d32, forward_bar(d32), d32f)


@functools.lru_cache(maxsize=None)
def forward_ref(case):
    return make_ref(points(case), case[3], case[4])


def upstream(fv64, seed):
    """standard normal upstream gradient, zeroed where the power normalisation is ill-conditioned"""
    dfv = np.random.default_rng(seed).standard_normal(fv64.shape).astype(np.float32)
    return np.where(np.abs(fv64) > DFV_FLOOR, dfv, 0).astype(np.float32)


def oracle_backward(p, dfv, m, sigma, fn=R.mfv3d):
    """(g64, g32): autograd of <fn(p), dfv> in float64 and float32"""
    out = []
    for dt in (torch.float64, torch.float32):
        x = torch.tensor(p, dtype=dt, requires_grad=True)
        (fn(x, m, sigma) * torch.tensor(dfv, dtype=dt)).sum().backward()
        out.append(x.grad.numpy().astype(np.float64))
    return out


def backward_bars(g64, g32):
    """per cloud: (err32, scale, bar)"""
    err32 = np.abs(g32 - g64).reshape(g64.shape[0], -1).max(1)
    scale = np.maximum(1.0, np.abs(g64).reshape(g64.shape[0], -1).max(1))
    return err32, scale, np.maximum(BWD_REL * scale, 10.0 * err32)


@functools.lru_cache(maxsize=None)
def backward_ref(case):
    kind, C, N, m, sigma = case
    dfv = upstream(forward_ref(case).fv64, [7, C, N, m])
    g64, g32 = oracle_backward(points(case), dfv, m, sigma)
    return BwdRef(dfv, g64, g32, *backward_bars(g64, g32))


# ------------------------------------------------------------------------------------------------ the checkers
def check_conditioning(ref, what):
    """the case is fit to judge a kernel: fp32 arithmetic of the oracle's own formula is within the bar, and no entry near 0 flips"""
    assert np.isfinite(ref.fv64).all() and np.isfinite(ref.fv32).all(), what
    assert ref.d32 <= FWD_BAR, ("float32 oracle is %.3g from float64: replace the seed" % ref.d32, what)
    # the kernel's is a third fp32 rounding (its own expf, its own order of sums): the second one may use half of the bar, no more
    assert ref.d32f is not None and ref.d32f <= 0.5 * ref.bar, ("fp32 with Q in product form is %.3g from float64: replace the seed" % ref.d32f, what)
    small = np.abs(ref.fv64) < SIGN_FLOOR
    # opposite signs; an fp32 pdf that underflows to 0 where float64 keeps 1e-90 gives 0 against +-1e-6 / norm, which is no flip
    flips = small & (np.sign(ref.fv32) * np.sign(ref.fv64) < 0)
    assert not flips.any(), ("%d entries below %g change sign: replace the seed" % (int(flips.sum()), SIGN_FLOOR), what)


def check_unit_norm(fv, m):
    """every channel has unit L2 norm over the Gaussian axis (m = 1: G = 1, and a channel that is exactly 0 stays 0)"""
    nrm = np.sqrt((np.asarray(fv, dtype=np.float64) ** 2).sum(1))                 # [C, 20]
    live = np.ones_like(nrm, dtype=bool) if m > 1 else (np.asarray(fv)[:, 0, :] != 0)
    bad = live & ~(np.abs(nrm - 1.0) <= NORM_TOL)
    assert not bad.any(), ("channel norms", nrm[bad][:4], np.argwhere(bad)[:4].tolist())
    assert not nrm[~live].any()


def check_forward(got, band, ref, m, what=None):
    """got [C, G, 20] float32 (a view into a guard-banded buffer) against the float64 oracle; returns the error"""
    got = got.detach().cpu().numpy()
    assert got.dtype == np.float32 and got.shape == ref.fv64.shape, (got.dtype, got.shape, ref.fv64.shape)
    diff = np.abs(got.astype(np.float64) - ref.fv64)
    err = float(np.nanmax(diff)) if np.isfinite(diff).any() else float("nan")
    print("forward %s: err %.3g  float32 oracle %.3g  bar %.3g" % (what, err, ref.d32, ref.bar))
    assert np.isfinite(got).all(), ("%d entries are not finite" % int((~np.isfinite(got)).sum()), what)
    if not err <= ref.bar:
        c, g, f = np.unravel_index(int(diff.argmax()), diff.shape)
        raise AssertionError("forward error %.3g above %.3g at cloud %d Gaussian %d channel %d (%d entries above): %r"
                             % (err, ref.bar, c, g, f, int((diff > ref.bar).sum()), what))
    check_unit_norm(got, m)
    band()
    return err


def check_backward(got, band, ref, what=None):
    """got [C, N, 3] float32 against float64 autograd, per cloud; returns the per-cloud errors over scale"""
    got = got.detach().cpu().numpy()
    assert got.dtype == np.float32 and got.shape == ref.g64.shape, (got.dtype, got.shape, ref.g64.shape)
    assert np.isfinite(got).all(), ("%d entries are not finite" % int((~np.isfinite(got)).sum()), what)
    err = np.abs(got.astype(np.float64) - ref.g64).reshape(got.shape[0], -1).max(1)
    print("backward %s: err/scale [%s]  float32 oracle/scale [%s]  bar/scale [%s]"
          % (what, *(" ".join("%.3g" % v for v in x / ref.scale) for x in (err, ref.err32, ref.bar))))
    for c in range(got.shape[0]):
        if not err[c] <= ref.bar[c]:
            n = int(np.abs(got[c] - ref.g64[c]).max(1).argmax())
            raise AssertionError("backward error %.3g above %.3g (scale %.3g) in cloud %d, worst at point %d: %r"
                                 % (err[c], ref.bar[c], ref.scale[c], c, n, what))
    band()
    return err / ref.scale


def check_forms_agree(a, b, scale, what=None):
    """two launch forms (or a cloud and its permutation) differ only by the association of sums: 1e-4 x scale, per cloud"""
    a, b = a.detach().cpu().numpy().astype(np.float64), b.detach().cpu().numpy().astype(np.float64)
    d = np.abs(a - b).reshape(a.shape[0], -1).max(1)
    assert (d <= BWD_REL * scale).all(), (d, BWD_REL * scale, what)


# ------------------------------------------------------------------------------------------------ larger LDS after smaller
# (kernel, calls in ascending order of that kernel's dynamic LDS; all C = 1).  Every call needs more than 64 KiB in the named kernel.
LDS_FWD2 = ((10, 168), (10, 536))          # (m, N): mfv3d_fwd2_kernel, N % 8 == 0
LDS_FWD = ((10, 169), (10, 535))           # mfv3d_fwd_kernel
LDS_BWD_ONE = ((8, 200), (8, 400))         # one-launch backward
LDS_BWD_SLICED = ((8, 656), (8, 1200), (8, 1300), (8, 1600))   # apply kernel above 64 KiB from the first, statistics kernel from the third


def check_lds_plan():
    """the sizes of the table above, from the host's formulas: each call above 64 KiB and under the cap, ascending per kernel"""
    for tab, fwd2 in ((LDS_FWD2, True), (LDS_FWD, False)):
        sizes = [fwd_lds_bytes(N, m) for m, N in tab]
        assert all(uses_fwd2(N) == fwd2 for _, N in tab)
        assert LDS_OPT_IN < sizes[0] < sizes[1] <= LDS_CAP, sizes
    assert [fwd_lds_bytes(N, m) for m, N in LDS_FWD2] == [66008, 163160]
    assert [fwd_lds_bytes(N, m) for m, N in LDS_FWD] == [66272, 162896]
    one = [bwd_lds_bytes(N, m) for m, N in LDS_BWD_ONE]
    assert one == [82736, 162736] and LDS_OPT_IN < one[0] < one[1] <= LDS_CAP
    st, ap = zip(*[bwd_sliced_lds_bytes(N, m) for m, N in LDS_BWD_SLICED])
    assert ap == (65616, 120016, 130016, 160016) and LDS_OPT_IN < ap[0] and ap[-1] <= LDS_CAP
    assert st == (33472, 61216, 66316, 81616) and st[1] <= LDS_OPT_IN < st[2] < st[3]
    assert all(takes_sliced(N) for _, N in LDS_BWD_SLICED)


# ------------------------------------------------------------------------------------------------ the C entries on guard-banded buffers
def gpu_forward(pts, m, sigma, C=None, N=None):
    """dpd_mfv3d_fwd on device tensor pts [C, N, 3] -> (return code, fv view [C, G, 20] inside a NaN-payload guard band, band check);
    C / N override the counts handed to the entry (for the refusals)"""
    from dpdist_amd import lib as L
    C = pts.shape[0] if C is None else C
    N = pts.shape[1] if N is None else N
    G = max(m, 1) ** 3
    view, band = banded_flat(max(C, 1) * G * F, device=pts.device)
    rc = L.load().dpd_mfv3d_fwd(L.ptr(pts), C, N, m, float(sigma), L.ptr(view), L.cur_stream())
    torch.cuda.synchronize()
    return rc, view.view(max(C, 1), G, F), band


def gpu_backward(pts, dfv, m, sigma, sliced, C=None, N=None):
    """dpd_mfv3d_bwd -> (return code, dpts view [C, N, 3] in a guard band, check of the dpts AND the workspace bands, workspace view);
    the workspace (sliced form only) is filled with the NaN payload before the call"""
    from dpdist_amd import lib as L
    lib = L.load()
    C = pts.shape[0] if C is None else C
    N = pts.shape[1] if N is None else N
    view, band = banded_flat(max(C, 1) * max(N, 1) * 3, device=pts.device)
    ws, ws_band, ws_bytes = None, (lambda: None), 0
    if sliced:
        ws_bytes = lib.dpd_mfv3d_bwd_workspace_bytes(max(C, 1), m)
        assert ws_bytes == max(C, 1) * SLICES * 33 * m ** 3 * 4
        ws, ws_band = banded_flat(ws_bytes // 4, device=pts.device)
    rc = lib.dpd_mfv3d_bwd(L.ptr(pts), L.ptr(dfv), C, N, m, float(sigma), L.ptr(view), L.ptr(ws), ws_bytes, L.cur_stream())
    torch.cuda.synchronize()

    def bands():
        band()
        ws_band()
    return rc, view.view(max(C, 1), max(N, 1), 3), bands, ws

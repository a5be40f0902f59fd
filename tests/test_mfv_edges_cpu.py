"""The encoder checkers of tests/mfv_cases.py have teeth, and every case of the GPU tables (tests/test_mfv_edges_gpu.py) is well
conditioned in the oracle itself: the float32 oracle, written into the guard-banded buffers as a stand-in for the kernel, passes
check_forward / check_backward on every case, and every way an encoder kernel can be subtly wrong -- a point dropped from the last
point slice, a Gaussian of the short last slice left out of the L2 norm, tie counts taken per slice, the meshgrid order swapped,
sigma applied twice, a store outside the output -- raises.  Runs without a GPU."""
import math

import numpy as np
import pytest
import torch

from oracle import restate as R

from . import mfv_cases as M

ALL_FWD = M.FWD_CASES + M.TIE_CASES + tuple(c for c in M.FRONT_CASES + M.CAP_CASES if c not in M.FWD_CASES)
ALL_BWD = M.BWD_CASES + M.TIE_CASES


def _id(case):
    return "%s-C%d-N%d-m%d-s%g" % case


# ------------------------------------------------------------------------------------------------ a restatement with faults
def variant(points, m, sigma, swap_ij=False, sigma_twice=False, norm_skip=None, amax=None, amin=None):
    """oracle.restate.mfv3d, operation for operation (test_variant_is_the_oracle), with the faults of the negative controls switchable"""
    amax = amax or (lambda x: x.amax(1))
    amin = amin or (lambda x: x.amin(1))
    dt = points.dtype
    Cn, N, D = points.shape
    G = m ** 3
    centres = R.grid_centers(m)
    if swap_ij:
        centres = centres[:, [1, 0, 2]]                                 # (l[i], l[j], l[t]) where (l[j], l[i], l[t]) belongs
    mu = torch.tensor(centres, dtype=dt)
    w = 1.0 / G
    z = (points[:, :, None, :] - mu[None, None]) / sigma
    if sigma_twice:
        z = z / sigma
    logp = -0.5 * (z * z).sum(-1) - (0.5 * D * math.log(2 * math.pi) + D * math.log(sigma))
    p = torch.exp(logp)
    wp = p * w
    Q = wp / wp.sum(-1, keepdim=True)
    d_pi_all = (Q - w) / (math.sqrt(w) * N)
    d_pi = torch.stack([d_pi_all.mean(1), amax(d_pi_all)], -1)
    d_mu_all = Q[..., None] * z
    d_mu = torch.cat([d_mu_all.mean(1), amax(d_mu_all), amin(d_mu_all)], -1) * (1.0 / math.sqrt(w))
    d_sig_all = Q[..., None] * (z * z - 1)
    d_sig = torch.cat([d_sig_all.mean(1), amax(d_sig_all), amin(d_sig_all)], -1) * (1.0 / math.sqrt(2 * w))

    def norm(x):
        x = torch.sign(x) * torch.sqrt(torch.clamp_min(torch.abs(x), 1e-12))
        xs = x if norm_skip is None else torch.cat([x[:, :norm_skip], x[:, norm_skip + 1:]], 1)
        ss = (xs * xs).sum(1, keepdim=True)
        return x * torch.rsqrt(torch.clamp_min(ss, 1e-12))

    return torch.cat([norm(d_pi), norm(d_mu), norm(d_sig)], -1)


def per_slice_ties(op):
    """an extremum over the points whose gradient is shared among the ties of each point slice separately (the value is the true one):
    a slice that attains the extremum hands the whole gradient to its own ties, so a two-way tie across slices gets 1/1 + 1/1"""
    def f(x):
        N = x.shape[1]
        ns = (N + M.SLICES - 1) // M.SLICES
        full = getattr(x, op)(1)
        fault = torch.zeros_like(full)
        for s in range(M.SLICES):
            xs = x[:, s * ns:(s + 1) * ns]
            if xs.shape[1]:
                e = getattr(xs, op)(1)
                fault = fault + torch.where(e == full, e, torch.zeros_like(e))
        return full.detach() + (fault - fault.detach())
    return f


@pytest.mark.parametrize("dt", [torch.float64, torch.float32])
def test_variant_is_the_oracle(dt):
    for case in (("u", 3, 10, 5, M.S0), ("t2", 1, 13, 3, M.S0), ("u", 2, 50, 5, 0.0625)):
        p = torch.tensor(M.points(case), dtype=dt)
        assert torch.equal(variant(p, case[3], case[4]), R.mfv3d(p, case[3], case[4]))


def test_product_form_is_the_oracle_in_float64():
    for case in (("u", 3, 10, 5, M.S0), ("b", 1, 100, 10, M.S0), ("u", 2, 64, 8, 0.25), ("u", 1, 1, 1, M.S0)):
        assert np.abs(M.factorised(M.points(case), case[3], case[4], torch.float64) - M.forward_ref(case).fv64).max() <= 1e-13


# ------------------------------------------------------------------------------------------------ stand-ins in guard-banded buffers
def fwd_buffer(shape):
    view, band = M.banded_flat(int(np.prod(shape)))
    assert M.untouched(view)
    return view.view(*shape), band


def standin_forward(case, fv):
    ref = M.forward_ref(case)
    view, band = fwd_buffer(ref.fv64.shape)
    view.copy_(torch.as_tensor(fv, dtype=torch.float32))
    return view, band, ref


def standin_backward(case, g):
    ref = M.backward_ref(case)
    view, band = fwd_buffer(ref.g64.shape)
    view.copy_(torch.as_tensor(g, dtype=torch.float32))
    return view, band, ref


def faulty_forward(case, **fault):
    return variant(torch.tensor(M.points(case)), case[3], case[4], **fault).numpy()


# ------------------------------------------------------------------------------------------------ conditioning and stand-in
@pytest.mark.parametrize("case", ALL_FWD, ids=_id)
def test_forward_case_is_well_conditioned_and_the_standin_passes(case):
    ref = M.forward_ref(case)
    M.check_conditioning(ref, case)
    p = M.points(case)
    assert p.dtype == np.float32 and p.shape == case[1:3] + (3,) and np.abs(p).max() < 1.0
    if case[0] != "b":
        assert np.abs(p).max() <= 0.8 + 1e-6
    assert ref.bar == max(3e-6, 4 * ref.d32) and ref.bar < 1.3e-5
    view, band, _ = standin_forward(case, ref.fv32)
    assert M.check_forward(view, band, ref, case[3], case) == ref.d32


@pytest.mark.parametrize("case", ALL_BWD, ids=_id)
def test_backward_case_is_well_conditioned_and_the_standin_passes(case):
    M.check_conditioning(M.forward_ref(case), case)
    ref = M.backward_ref(case)
    assert np.isfinite(ref.g64).all() and np.isfinite(ref.g32).all()
    assert (ref.dfv[np.abs(M.forward_ref(case).fv64) < M.DFV_FLOOR] == 0).all() and (ref.dfv != 0).mean() > 0.02
    # the float32 reference itself sits inside the flat part of the bar: the case is fit to judge a gradient at 1e-4 of scale
    assert (ref.err32 <= M.BWD_REL * ref.scale).all(), (ref.err32 / ref.scale, case)
    view, band, _ = standin_backward(case, ref.g32)
    M.check_backward(view, band, ref, case)


def test_a_bad_seed_fails_the_conditioning_check():
    """seed 0 of this m = 2 cloud leaves a channel whose eight values all sit below the clamp: the float32 oracle is 0.35 away"""
    case = ("u", 3, 9, 2, M.S0)
    rng = np.random.default_rng([0, 0, 3, 9, 2, 1250])
    p = rng.uniform(-0.8, 0.8, size=(3, 9, 3)).astype(np.float32)
    with pytest.raises(AssertionError, match="float32 oracle is .* replace the seed"):
        M.check_conditioning(M.make_ref(p, 2, M.S0), case)
    # seed 0 of the m = 4 lattice cloud: mean Q = w for one Gaussian, which only a second fp32 rounding of Q shows
    case = ("b", 1, 16, 4, M.S0)
    p = M.boundary_coords(4)[np.random.default_rng([0, 1, 1, 16, 4, 1250]).integers(0, M.boundary_coords(4).size, size=(1, 16, 3))]
    bad = M.make_ref(p, 4, M.S0)
    assert bad.d32 <= M.FWD_BAR < bad.d32f
    with pytest.raises(AssertionError, match="product form .* replace the seed"):
        M.check_conditioning(bad, case)
    flipped = M.forward_ref(("u", 3, 10, 5, M.S0))
    fv32 = flipped.fv32.copy()
    i = np.unravel_index(np.abs(np.where(flipped.fv64 == 0, np.inf, flipped.fv64)).argmin(), fv32.shape)
    assert 0 < abs(flipped.fv64[i]) < M.SIGN_FLOOR
    fv32[i] = -np.sign(flipped.fv64[i]) * 1e-7
    with pytest.raises(AssertionError, match="change sign"):
        M.check_conditioning(flipped._replace(fv32=fv32), "flip")


# ------------------------------------------------------------------------------------------------ the tables reach what they claim
def test_tables_cover_the_paths():
    fwd_n = {c[2] for c in M.FWD_CASES if c[0] == "u"}
    fwd_m = {c[3] for c in M.FWD_CASES if c[0] == "u"}
    assert fwd_n == {1, 2, 7, 8, 9, 10, 13, 16, 50, 63, 64, 65, 100} and fwd_m == {1, 2, 3, 4, 5, 7, 8, 9, 10}
    assert {c[3] for c in M.FWD_CASES if c[0] == "b"} == fwd_m
    uneven, pow2 = {1, 3, 5, 7, 9}, {1, 2, 4, 8}
    assert all(len(set(M.gauss_slices(m))) > 1 for m in uneven) and all(len(set(M.gauss_slices(m))) == 1 for m in (2, 4, 8, 10))
    for N in fwd_n:                                  # every N meets an uneven Gaussian split and a power-of-two m
        ms = {c[3] for c in M.FWD_CASES if c[0] == "u" and c[2] == N}
        assert ms & uneven and ms & pow2, (N, ms)
    assert all(c[1] <= 3 for c in M.FWD_CASES if c[1] not in (5,)) and sum(c[1] == 5 for c in M.FWD_CASES) == 1
    assert any(c[1] == 1 for c in M.FWD_CASES if c[0] == "u" and c[2] > 1)
    assert sorted({(c[1:4]) for c in M.FWD_CASES if c[4] != M.S0}) == [(2, 50, 5), (2, 64, 8)]
    assert {c[4] for c in M.FWD_CASES} == {0.125, 0.0625, 0.25}
    assert M.gauss_slices(5) == [32, 32, 32, 29] and M.gauss_slices(3) == [7, 7, 7, 6] and M.gauss_slices(1) == [1, 0, 0, 0]
    assert {c[2] for c in M.BWD_CASES} == {7, 8, 9, 10, 13, 50, 64, 100} and {c[3] for c in M.BWD_CASES} == {2, 3, 5, 8}
    assert all(1 < c[3] <= 8 for c in ALL_BWD)
    assert M.point_slices(9) == [3, 3, 3, 0] and M.point_slices(10) == [3, 3, 3, 1] and M.point_slices(13) == [4, 4, 4, 1]
    assert not M.takes_sliced(7) and M.takes_sliced(8)
    assert [M.uses_fwd2(N) for N in (1, 7, 8, 9, 16, 63, 64, 65)] == [False, False, True, False, True, False, True, False]
    assert len(set(ALL_FWD)) == len(ALL_FWD) and len(set(ALL_BWD)) == len(ALL_BWD)
    assert [c[2:4] for c in M.CAP_CASES] == [(704, 8), (705, 8), (536, 10), (538, 10)]


def test_tie_clouds_put_every_copy_in_another_slice():
    for case in M.TIE_CASES:
        kind, _, N, _, _ = case
        p, idx = M.points(case)[0], M.tie_partner(kind, N)
        ns = (N + M.SLICES - 1) // M.SLICES
        assert np.array_equal(p, p[idx])
        groups = [np.flatnonzero(idx == o) for o in np.unique(idx)]
        assert len(np.unique(p, axis=0)) == len(groups)
        for g in groups:
            assert len(set(g // ns)) == len(g)                       # no two copies of a point share a slice
        sizes = sorted(len(g) for g in groups)
        if kind == "t2":
            assert sizes[0] == 2 and sizes[-1] == (3 if N % 2 else 2)
        else:
            assert sizes == [1] * (N - 2) + [2] and M.point_slices(N)[-1] == 1 and idx[N - 1] == 0
        g64 = M.backward_ref(case).g64[0]
        assert np.abs(g64 - g64[idx]).max() <= 1e-12 * M.backward_ref(case).scale[0]   # autograd shares a tie evenly


def test_lds_plan_and_cap():
    M.check_lds_plan()
    assert (M.largest_fwd_n(8, True), M.largest_fwd_n(8, False)) == (704, 705)
    assert (M.largest_fwd_n(10, True), M.largest_fwd_n(10, False)) == (536, 538)
    for m, fwd2 in ((8, True), (8, False), (10, True), (10, False)):
        N = M.largest_fwd_n(m, fwd2)
        assert M.fwd_lds_bytes(N, m) <= M.LDS_CAP < M.fwd_lds_bytes(N + (8 if fwd2 else 1), m)
    assert M.fwd_lds_bytes(706, 8) > M.LDS_CAP and M.fwd_lds_bytes(539, 10) > M.LDS_CAP


def test_n16_and_n17_share_their_extrema():
    """a 17th point that repeats point 0 leaves every max / min over the points where it was; the 1 / N of d_pi is a constant factor
    that the L2 norm removes: the max / min channels of fv agree, across the two forward kernels (N = 16: pairs, N = 17: eight groups)"""
    for m in (5, 8):
        p16 = M.points(("u", 3, 16, 7, M.S0))
        p17 = np.concatenate([p16, p16[:, :1]], 1)
        a, b = (R.mfv3d(torch.tensor(p, dtype=torch.float64), m, M.S0).numpy() for p in (p16, p17))
        ch = list(M.MAXMIN_CHANNELS)
        assert np.abs(a[..., ch] - b[..., ch]).max() <= 1e-12
        assert np.abs(a - b).max() > 1e-3                              # while the mean channels move


# ------------------------------------------------------------------------------------------------ negative controls
NEG = ("u", 3, 10, 5, M.S0)         # point slices 3,3,3,1 and Gaussian slices 32,32,32,29


def test_untouched_forward_output_raises():
    ref = M.forward_ref(NEG)
    view, band = fwd_buffer(ref.fv64.shape)
    with pytest.raises(AssertionError, match="not finite"):
        M.check_forward(view, band, ref, NEG[3])


def test_point_dropped_from_the_last_point_slice_raises():
    p = torch.tensor(M.points(NEG))
    fv = R.mfv3d(p[:, :-1], NEG[3], NEG[4]).numpy()
    view, band, ref = standin_forward(NEG, fv)
    with pytest.raises(AssertionError, match="forward error"):
        M.check_forward(view, band, ref, NEG[3])
    # backward: the statistics miss the point and it receives no gradient
    bref = M.backward_ref(NEG)
    x = p.clone().requires_grad_(True)
    (R.mfv3d(x[:, :-1], NEG[3], NEG[4]) * torch.tensor(bref.dfv)).sum().backward()
    view, band, _ = standin_backward(NEG, x.grad.numpy())
    with pytest.raises(AssertionError, match="backward error"):
        M.check_backward(view, band, bref)


def test_gaussian_of_the_short_slice_left_out_of_the_norm_raises():
    G = NEG[3] ** 3
    assert M.gauss_slices(NEG[3])[-1] == 29
    fv = faulty_forward(NEG, norm_skip=G - 1)
    view, band, ref = standin_forward(NEG, fv)
    with pytest.raises(AssertionError, match="forward error"):
        M.check_forward(view, band, ref, NEG[3])
    with pytest.raises(AssertionError, match="channel norms"):
        M.check_unit_norm(fv, NEG[3])
    # m = 3: the one Gaussian that makes slice 3 shorter than the others (7, 7, 7, 6)
    case = ("u", 3, 13, 3, M.S0)
    view, band, ref = standin_forward(case, faulty_forward(case, norm_skip=26))
    with pytest.raises(AssertionError, match="forward error"):
        M.check_forward(view, band, ref, 3)


@pytest.mark.parametrize("case", M.TIE_CASES, ids=_id)
def test_tie_count_per_slice_raises(case):
    bref = M.backward_ref(case)
    x = torch.tensor(M.points(case), requires_grad=True)
    fv = variant(x, case[3], case[4], amax=per_slice_ties("amax"), amin=per_slice_ties("amin"))
    assert torch.equal(fv.detach(), R.mfv3d(x.detach(), case[3], case[4]))      # the forward is untouched: only the shares differ
    (fv * torch.tensor(bref.dfv)).sum().backward()
    view, band, _ = standin_backward(case, x.grad.numpy())
    with pytest.raises(AssertionError, match="backward error"):
        M.check_backward(view, band, bref)


def test_tie_fault_is_invisible_without_ties():
    """the same per-slice count on a cloud without ties is the right count: the control above fails for the ties, nothing else"""
    bref = M.backward_ref(NEG)
    x = torch.tensor(M.points(NEG), requires_grad=True)
    (variant(x, NEG[3], NEG[4], amax=per_slice_ties("amax"), amin=per_slice_ties("amin")) * torch.tensor(bref.dfv)).sum().backward()
    view, band, _ = standin_backward(NEG, x.grad.numpy())
    M.check_backward(view, band, bref)


@pytest.mark.parametrize("fault", ["swap_ij", "sigma_twice"])
def test_wrong_centres_or_sigma_raise(fault):
    for case in (NEG, ("u", 2, 64, 8, M.S0), ("u", 2, 2, 4, M.S0)):
        view, band, ref = standin_forward(case, faulty_forward(case, **{fault: True}))
        with pytest.raises(AssertionError, match="forward error|not finite"):
            M.check_forward(view, band, ref, case[3])


@pytest.mark.parametrize("where", ["before", "after", "first", "last"])
@pytest.mark.parametrize("which", ["forward", "backward"])
def test_touched_guard_band_raises(which, where):
    if which == "forward":
        view, band, ref = standin_forward(NEG, M.forward_ref(NEG).fv32)
    else:
        view, band, ref = standin_backward(NEG, M.backward_ref(NEG).g32)
    n = view.numel()
    off = {"before": M.FLAT_BAND - 1, "after": M.FLAT_BAND + n, "first": 0, "last": band.raw.numel() - 1}[where]
    band.raw[off] = 0                      # a stray store of 0.0f
    with pytest.raises(AssertionError, match="guard band changed at 1 raw elements, first at offset %d" % off):
        if which == "forward":
            M.check_forward(view, band, ref, NEG[3])
        else:
            M.check_backward(view, band, ref)


def test_forms_agree_bar():
    ref = M.backward_ref(NEG)
    a = torch.tensor(ref.g32, dtype=torch.float32)
    M.check_forms_agree(a, a + 0.5e-4, ref.scale)
    with pytest.raises(AssertionError):
        M.check_forms_agree(a, a + 2e-4 * float(ref.scale.max()), ref.scale)

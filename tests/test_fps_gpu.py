"""Farthest-point sampling on the GPU (csrc/fps.hip through dpdist_amd/sampling.py): the order is defined bit for bit -- fp32 distances
(dx*dx + dy*dy) + dz*dz, ties to the lowest index through every merge (rounds of a thread, lanes, waves), chosen points excluded -- so it
is compared for EQUALITY with the numpy restatement of tests/fps_cases.py, across every kernel form: the register-resident templates
(1 / 2 / 4 / 8 / 16 points per thread) and the streamed form beyond DPD_FPS_RESIDENT_POINTS.  radius may differ by sqrtf's 1 ulp, the
allowance of tests/test_nn_dist_gpu.py."""
import functools

import numpy as np
import pytest
import torch

from dpdist_amd import ops
from dpdist_amd import sampling as SM
from dpdist_amd import chamfer_pairs, farthest_point_order, farthest_point_sample

from . import fps_cases as F

pytestmark = pytest.mark.gpu

T, R = SM.FPS_THREADS, SM.FPS_RESIDENT_POINTS
SMAX = 3
FULL = [1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 3]          # K = N
WIDE = [4 * T + 1, R - 1, R, R + 1, 2 * R + 5]                 # K = 257: the 8- and 16-point templates, the last resident and the first
KWIDE = 257                                                    # streamed shape, both boundaries of thread ownership


def cu(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()      # a copy: the cached references are read-only


@functools.lru_cache(maxsize=None)
def case(kind, N, K):
    """SMAX different clouds of N points and their restated (order, radius): fp32 for random clouds, float64 for lattice clouds"""
    build = {"random": F.random_cloud, "lattice": F.lattice_cloud_with_duplicates}[kind]
    dtype = np.float32 if kind == "random" else np.float64
    pts = np.stack([build(N, 10 + s) for s in range(SMAX)])
    ref = [F.fps_reference(pts[s], K, dtype=dtype) for s in range(SMAX)]
    order, radius = np.stack([r[0] for r in ref]), np.stack([r[1] for r in ref]).astype(np.float32)
    for a in (pts, order, radius):
        a.setflags(write=False)
    return pts, order, radius


def run(pts, K, **kw):
    order, radius = farthest_point_order(cu(pts), K, return_radius=True, **kw)
    torch.cuda.synchronize()
    return order.cpu().numpy(), radius.cpu().numpy()


def check(order, radius, want_order, want_radius):
    assert order.dtype == np.int32 and radius.dtype == np.float32
    assert np.array_equal(order, want_order)
    assert np.isposinf(radius[..., 0]).all()
    ulp = F.ulp_distance(radius[..., 1:], want_radius[..., 1:])
    print("radius: max ulp difference to np.sqrt = %d" % ulp)
    assert ulp <= 1


@pytest.mark.parametrize("S", [1, SMAX])
@pytest.mark.parametrize("N", FULL)
def test_full_permutation_equals_the_fp32_restatement(S, N):
    pts, want_o, want_r = case("random", N, N)
    order, radius = run(pts[:S], N)
    check(order, radius, want_o[:S], want_r[:S])
    for s in range(S):
        assert sorted(order[s].tolist()) == list(range(N))


@pytest.mark.parametrize("S", [1, SMAX])
@pytest.mark.parametrize("N", WIDE)
def test_wide_clouds_equal_the_fp32_restatement(S, N):
    pts, want_o, want_r = case("random", N, KWIDE)
    order, radius = run(pts[:S], KWIDE)
    check(order, radius, want_o[:S], want_r[:S])


@pytest.mark.parametrize("N,K", [(193, 193), (T + 1, T + 1), (2 * T + 3, 2 * T + 3), (R, KWIDE), (R + 1, KWIDE)])
def test_exact_ties_across_lanes_waves_and_forms(N, K):
    """Lattice clouds with a tenth of the points duplicated at higher indices: few distinct distances, so almost every maximum is a tie,
    and with K = N the tail is all dmin = 0.  float64 restatement == float32 there; a merge on dmin alone fails this."""
    pts, want_o, want_r = case("lattice", N, K)
    order, radius = run(pts, K)
    check(order, radius, want_o, want_r)


def test_all_identical_cloud():
    pts = np.full((1, 7, 3), 0.25, np.float32)
    order, radius = run(pts, 7, start=[3])
    assert order[0].tolist() == [3, 0, 1, 2, 4, 5, 6]
    assert np.isposinf(radius[0, 0]) and (radius[0, 1:] == 0).all() and not np.signbit(radius[0, 1:]).any()


@pytest.mark.parametrize("N", [65, 2 * T + 3, R + 1])
def test_start_per_cloud_and_default(N):
    K = min(N, 40)
    pts = case("random", N, N if N in FULL else KWIDE)[0]
    starts = [N - 1, 0, N // 2]
    want = [F.fps_reference(pts[s], K, start=starts[s]) for s in range(SMAX)]
    order, radius = run(pts, K, start=starts)
    check(order, radius, np.stack([w[0] for w in want]), np.stack([w[1] for w in want]))
    order_t, _ = run(pts, K, start=torch.tensor(starts, dtype=torch.int32).cuda())      # a device tensor
    assert np.array_equal(order_t, order)
    zero, rz = run(pts, K, start=[0, 0, 0])
    none, rn = run(pts, K)
    assert np.array_equal(zero, none) and np.array_equal(rz.view(np.int32), rn.view(np.int32))
    clamped, _ = run(pts, K, start=torch.tensor([N + 5, -3, N // 2], dtype=torch.int32).cuda())   # device values are clamped into the cloud
    assert np.array_equal(clamped, order)


@pytest.mark.parametrize("W", [70, 2 * T + 3, R + 1])
@pytest.mark.parametrize("K", [4, 20])
def test_ragged_batch_equals_each_cloud_alone(W, K):
    """counts (1, 5, 37, W) in one launch, K below and above some of them.  The padding holds finite points far outside the cloud: read,
    they would be chosen first."""
    counts = [1, 5, 37, W]
    rng = np.random.default_rng([W, K])
    pts = rng.uniform(-1, 1, (4, W, 3)).astype(np.float32)
    for c, n in enumerate(counts):
        pts[c, n:] = 1000.0 + rng.uniform(-1, 1, (W - n, 3))
    order, radius = run(pts, K, counts=counts)
    order_t, radius_t = run(pts, K, counts=torch.tensor(counts, dtype=torch.int32).cuda())
    assert np.array_equal(order, order_t) and np.array_equal(radius.view(np.int32), radius_t.view(np.int32))
    for c, n in enumerate(counts):
        kn = min(K, n)
        alone_o, alone_r = run(pts[c:c + 1, :n], kn)                       # the cloud alone at width n
        assert np.array_equal(order[c, :kn], alone_o[0]) and np.array_equal(radius[c, :kn].view(np.int32), alone_r[0].view(np.int32))
        assert (order[c, kn:] == -1).all() and (radius[c, kn:] == 0).all() and not np.signbit(radius[c, kn:]).any()
        want_o, want_r = F.fps_reference(pts[c, :n], K)
        assert np.array_equal(order[c], want_o)
        F.check_properties(order[c], radius[c], n)


@pytest.mark.parametrize("N,K", [(T + 1, T + 1), (R + 1, KWIDE)])
def test_repeated_call_gives_equal_bits(N, K):
    pts = case("random", N, K)[0]
    a, ra = run(pts, K)
    b, rb = run(pts, K)
    assert np.array_equal(a, b) and np.array_equal(ra.view(np.int32), rb.view(np.int32))


def test_one_cloud_without_batch_dimension():
    pts, want_o, _ = case("random", 65, 65)
    order = farthest_point_order(cu(pts[0]), 10)
    assert tuple(order.shape) == (10,) and np.array_equal(order.cpu().numpy(), want_o[0, :10])
    with pytest.raises(RuntimeError):
        farthest_point_order(cu(pts).transpose(0, 1), 2)                   # [65,3,3] but not contiguous: refused at the boundary


# ---------------------------------------------------------------------------------------------------------------------
# gather
# ---------------------------------------------------------------------------------------------------------------------
GW, GK, GCOUNTS = 2 * T + 3, 50, [7, 2 * T + 3, 37]


@functools.lru_cache(maxsize=None)
def gather_case():
    rng = np.random.default_rng(77)
    pts = rng.uniform(-1, 1, (3, GW, 3)).astype(np.float32)
    order = np.stack([F.fps_reference(pts[c, :n], GK)[0] for c, n in enumerate(GCOUNTS)])
    pts.setflags(write=False), order.setflags(write=False)
    return pts, order


@pytest.mark.parametrize("Dm", [1, 3, 6])
def test_gather_forward_and_backward(Dm):
    _, order = gather_case()
    rng = np.random.default_rng(Dm)
    src = rng.uniform(-1, 1, (3, GW, Dm)).astype(np.float32)
    dout = rng.uniform(-1, 1, (3, GK, Dm)).astype(np.float32)
    dout[0, 1, 0] = -0.0                                                   # a negative zero travels as it is
    out = ops.fps_gather_fwd(cu(src), cu(order)).cpu().numpy()
    dsrc = ops.fps_gather_bwd(cu(dout), cu(order), GW).cpu().numpy()
    want = np.zeros((3, GK, Dm), np.float32)
    want_d = np.zeros((3, GW, Dm), np.float32)
    for c in range(3):
        v = order[c] >= 0
        want[c, v] = src[c, order[c, v]]
        want_d[c, order[c, v]] = dout[c, v]
    assert (order[0] == -1).any() and (order[1] >= 0).all()
    assert np.array_equal(out.view(np.int32), want.view(np.int32))         # +0.0 rows at -1: the sign bit is compared too
    assert np.array_equal(dsrc.view(np.int32), want_d.view(np.int32))      # every row not chosen, and every row behind -1, is +0.0


def test_sample_and_its_gradients():
    pts, order = gather_case()
    rng = np.random.default_rng(5)
    feat = rng.uniform(-1, 1, (3, GW, 6)).astype(np.float32)
    G, H = rng.uniform(-1, 1, (3, GK, 3)).astype(np.float32), rng.uniform(-1, 1, (3, GK, 6)).astype(np.float32)
    clouds, features = cu(pts).requires_grad_(), cu(feat).requires_grad_()
    points, counts_out, got_order, got_feat = farthest_point_sample(clouds, GK, counts=GCOUNTS, features=features)
    assert np.array_equal(got_order.cpu().numpy(), order) and not got_order.requires_grad
    assert counts_out.dtype == torch.int32 and counts_out.cpu().tolist() == [min(GK, n) for n in GCOUNTS]
    want_p, want_f = np.zeros((3, GK, 3), np.float32), np.zeros((3, GK, 6), np.float32)
    want_dp, want_df = np.zeros_like(pts), np.zeros_like(feat)
    for c in range(3):
        v = order[c] >= 0
        want_p[c, v], want_f[c, v] = pts[c, order[c, v]], feat[c, order[c, v]]
        want_dp[c, order[c, v]], want_df[c, order[c, v]] = G[c, v], H[c, v]
    assert np.array_equal(points.detach().cpu().numpy().view(np.int32), want_p.view(np.int32))
    assert np.array_equal(got_feat.detach().cpu().numpy().view(np.int32), want_f.view(np.int32))
    ((points * cu(G)).sum() + (got_feat * cu(H)).sum()).backward()
    assert np.array_equal(clouds.grad.cpu().numpy().view(np.int32), want_dp.view(np.int32))
    assert np.array_equal(features.grad.cpu().numpy().view(np.int32), want_df.view(np.int32))
    p3, c3, o3 = farthest_point_sample(cu(pts), GK)                        # without counts and features: three values, counts_out None
    assert c3 is None and tuple(p3.shape) == (3, GK, 3) and (o3.cpu().numpy() >= 0).all()
    one = farthest_point_sample(cu(pts[1]), 5)                             # one cloud [W,3]
    assert tuple(one[0].shape) == (5, 3) and one[2].cpu().tolist() == order[1, :5].tolist()


def test_sample_feeds_the_ragged_arguments_of_chamfer_pairs():
    pts, order = gather_case()
    B = cu(np.random.default_rng(9).uniform(-1, 1, (3, 40, 3)).astype(np.float32))
    cB = [40, 11, 29]
    points, counts_out, _ = farthest_point_sample(cu(pts), GK, counts=GCOUNTS)
    got = chamfer_pairs(points, B, form="sqrt", countsA=counts_out, countsB=cB).cpu().numpy()
    for c, n in enumerate(GCOUNTS):
        kn = min(GK, n)
        alone = chamfer_pairs(cu(pts[c, order[c, :kn]][None]), B[c:c + 1, :cB[c]].contiguous(), form="sqrt").cpu().numpy()
        assert got[c].view(np.int32) == alone[0].view(np.int32)

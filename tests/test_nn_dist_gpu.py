"""dpd_nn_dist (csrc/nn_dist.hip) on the GPU: the nearest-point distance is defined bit for bit -- sqrt of the fp32 minimum of
(dx*dx + dy*dy) + dz*dz -- and ties go to the lowest index through every merge (LDS chunks, waves of a workgroup)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from dpdist_amd import dataset as D
from dpdist_amd import lib as L

pytestmark = pytest.mark.gpu

CHUNK, TILE = D.NN_CHUNK, D.NN_TILE
PS = [1, 63, 65, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3, 10007]
MS = [1, 255, 257, TILE + 1, 1000]          # TILE + 1 == 257 for the 256-query tile
MMAX, SMAX = max(MS), 3


def cu(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()      # a copy: the cached references are read-only


def fp32_sq_matrix(q, p):
    """[M,P] float32: the kernel's expression, term by term in np.float32 (numpy does not fuse)"""
    q, p = q.astype(np.float32), p.astype(np.float32)
    dx, dy, dz = (q[:, None, c] - p[None, :, c] for c in range(3))
    return (dx * dx + dy * dy) + dz * dz


def f64_min(q, p):
    from scipy.spatial.distance import cdist
    return cdist(q.astype(np.float64), p.astype(np.float64)).min(1)


@functools.lru_cache(maxsize=None)
def case(P):
    """Clouds in [-1,1]^3, different per shape; the reference for MMAX queries is computed once per P (fewer queries are a prefix)."""
    rng = np.random.default_rng(1000 + P)
    p = rng.uniform(-1, 1, (SMAX, P, 3)).astype(np.float32)
    q = rng.uniform(-1, 1, (SMAX, MMAX, 3)).astype(np.float32)
    d2 = [fp32_sq_matrix(q[s], p[s]) for s in range(SMAX)]
    want = np.stack([np.sqrt(m.min(1)) for m in d2])
    arg = np.stack([m.argmin(1) for m in d2]).astype(np.int32)
    d64 = np.stack([f64_min(q[s], p[s]) for s in range(SMAX)])
    for a in (p, q, want, arg, d64):
        a.setflags(write=False)
    return p, q, want, arg, d64


@pytest.mark.parametrize("S", [1, SMAX])
@pytest.mark.parametrize("P", PS)
def test_exact_against_the_fp32_minimum(S, P):
    """Observed on MI355X: dist is EQUAL to np.sqrt of the fp32 minimum (0 ulp) in every case; the assertion allows 1 ulp for sqrtf."""
    p, q, want, arg, d64 = case(P)
    worst = 0
    for M in MS:
        dist, idx = D.nn_distance(cu(p[:S]), cu(q[:S, :M]), return_index=True)
        assert dist.shape == (S, M) and idx.shape == (S, M) and idx.dtype == torch.int32
        dist, idx = dist.cpu().numpy(), idx.cpu().numpy()
        ulp = np.abs(dist.view(np.int32).astype(np.int64) - want[:S, :M].view(np.int32).astype(np.int64)).max()
        worst = max(worst, int(ulp))
        assert ulp <= 1, (S, P, M, ulp)
        assert np.array_equal(idx, arg[:S, :M]), (S, P, M)                      # np.argmin: the first index
        assert np.allclose(dist, d64[:S, :M], rtol=1e-6, atol=1e-7), (S, P, M)  # sanity bound on the formula itself
        only = D.nn_distance(cu(p[:S]), cu(q[:S, :M]))                          # arg = NULL: the same dist
        assert np.array_equal(only.cpu().numpy(), dist)
    print("S=%d P=%d: max ulp difference to np.sqrt(fp32 min) = %d" % (S, P, worst))
    if S == 1:                                                                  # the unbatched [P,3] / [M,3] form
        d1 = D.nn_distance(cu(p[0]), cu(q[0, :257]))
        assert d1.shape == (257,) and np.array_equal(d1.cpu().numpy().view(np.int32), D.nn_distance(cu(p[:1]), cu(q[:1, :257])).cpu().numpy()[0].view(np.int32))


def test_ties_go_to_the_lowest_index_across_chunks_and_waves():
    """10 % of the reference points are duplicated at higher indices, in a later LDS chunk than their original, and the queries sit next
    to duplicated points: the minimum is attained twice, bit for bit.  An original at index i of chunk 0 is held by wave i // (CHUNK/16), its
    duplicate in chunk 1 or 2 mostly by ANOTHER wave, often a lower one -- a merge on the distance alone returns the duplicate."""
    rng = np.random.default_rng(7)
    base, dup = 2 * CHUNK - 6, (2 * CHUNK - 6) // 10          # duplicates occupy the end of chunk 1 and the start of chunk 2
    src = rng.choice(CHUNK, dup, replace=False)               # originals: all in chunk 0
    p = rng.uniform(-1, 1, (2, base, 3)).astype(np.float32)
    p = np.concatenate([p, p[:, src]], 1)
    assert p.shape[1] > 2 * CHUNK
    q = (p[:, src] + rng.normal(0, 1e-4, (2, dup, 3))).astype(np.float32)
    q = np.concatenate([q, rng.uniform(-1, 1, (2, 300, 3)).astype(np.float32)], 1)
    dist, idx = D.nn_distance(cu(p), cu(q), return_index=True)
    idx = idx.cpu().numpy()
    for s in range(2):
        m = fp32_sq_matrix(q[s], p[s])
        assert np.array_equal(idx[s], m.argmin(1))
        assert np.array_equal(idx[s, :dup], src)              # the original, never base + k
        assert (m[np.arange(dup), src] == m[np.arange(dup), base + np.arange(dup)]).all()      # ... although the duplicate is as near
        assert np.array_equal(dist[s].cpu().numpy(), np.sqrt(m.min(1)))


def test_coincident_queries_have_distance_zero():
    rng = np.random.default_rng(8)
    p = rng.uniform(-1, 1, (2, CHUNK + 77, 3)).astype(np.float32)
    pick = rng.choice(p.shape[1], 500, replace=False)
    dist, idx = D.nn_distance(cu(p), cu(p[:, pick]), return_index=True)
    assert (dist == 0.0).all() and np.array_equal(idx.cpu().numpy(), np.stack([pick, pick]))


def test_near_surface_labels_keep_their_relative_accuracy():
    """Queries 0.001 - 0.002 off a dense cloud of norm ~0.5: the labels that matter most.  The exact-difference form keeps them to 1e-4
    relative; |p|^2 + |q|^2 - 2 p.q in fp32 (the matrix-core form this kernel refuses) does not, which is the reason the kernel is on the VALU."""
    rng = np.random.default_rng(9)
    g = rng.standard_normal((10000, 3))
    p = (0.5 * g / np.linalg.norm(g, axis=1, keepdims=True)).astype(np.float32)
    pick = rng.choice(len(p), 2000, replace=False)
    u = rng.standard_normal((2000, 3))
    q = (p[pick] + u / np.linalg.norm(u, axis=1, keepdims=True) * rng.uniform(0.001, 0.002, (2000, 1))).astype(np.float32)
    dist = D.nn_distance(cu(p), cu(q)).cpu().numpy().astype(np.float64)
    d64 = f64_min(q, p)
    assert d64.max() < 0.00201 and d64.min() > 1e-5
    rel = np.abs(dist - d64) / d64
    print("near-surface: max relative error %.3g" % rel.max())
    assert rel.max() <= 1e-4
    pn, qn = p[pick], q                                        # the GEMM form on the generating pairs, in fp32
    mm = ((pn * pn).sum(1) + (qn * qn).sum(1)) - np.float32(2) * (pn * qn).sum(1)
    true = ((pn.astype(np.float64) - qn.astype(np.float64)) ** 2).sum(1)
    assert (np.abs(np.sqrt(np.maximum(mm, 0)).astype(np.float64) - np.sqrt(true)) / np.sqrt(true)).max() > 1e-3


@pytest.mark.parametrize("S,P,M", [(1, 1, 1), (3, 65, 255), (2, CHUNK + 1, TILE + 1), (2, 2 * CHUNK + 3, 2 * TILE - 1)])
def test_tail_shapes_leave_the_guard_bands_alone(S, P, M):
    rng = np.random.default_rng(10)
    p, q = cu(rng.uniform(-1, 1, (S, P, 3)).astype(np.float32)), cu(rng.uniform(-1, 1, (S, M, 3)).astype(np.float32))
    G = 1024
    fd = torch.full((S * M + 2 * G,), -7.0, device="cuda")
    fi = torch.full((S * M + 2 * G,), -7, device="cuda", dtype=torch.int32)
    off = lambda t: ctypes.c_void_p(t.data_ptr() + 4 * G)      # noqa: E731
    lib = L.load()
    L.check(lib.dpd_nn_dist(L.ptr(p), L.ptr(q), S, P, M, off(fd), off(fi), L.cur_stream()), "dpd_nn_dist")
    want_d, want_i = D.nn_distance(p, q, return_index=True)
    for f, want, sent in ((fd, want_d, -7.0), (fi, want_i, -7)):
        assert (f[:G] == sent).all() and (f[G + S * M:] == sent).all()
        assert torch.equal(f[G:G + S * M].view(S, M), want) and (f[G:G + S * M] >= 0).all()
    fd.fill_(-7.0)                                             # arg = NULL: dist alone, same bits, same bands
    L.check(lib.dpd_nn_dist(L.ptr(p), L.ptr(q), S, P, M, off(fd), None, L.cur_stream()), "dpd_nn_dist")
    assert (fd[:G] == -7.0).all() and (fd[G + S * M:] == -7.0).all() and torch.equal(fd[G:G + S * M].view(S, M), want_d)


def test_wrapper_refuses_other_dtypes_and_layouts():
    p, q = torch.zeros(8, 3, device="cuda"), torch.zeros(5, 3, device="cuda")
    with pytest.raises(RuntimeError, match="float32"):
        D.nn_distance(p.double(), q.double())
    with pytest.raises(RuntimeError, match="contiguous"):
        D.nn_distance(torch.zeros(3, 8, device="cuda").t(), q)
    with pytest.raises(RuntimeError, match="same number of shapes"):
        D.nn_distance(torch.zeros(2, 8, 3, device="cuda"), torch.zeros(3, 5, 3, device="cuda"))

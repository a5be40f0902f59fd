"""Ragged sets, the host side: the five per-cloud-count entries refuse before any HIP call, the counts checks of dpdist_matrix /
DPDistMatrix, pad_clouds, and the admission of every case tests/test_ragged_gpu.py runs (tests/ragged_cases.py)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import mfv_cases as M
from tests import mfv_tiled_cases as T
from tests import ragged_cases as RC

KP = 2528


@pytest.fixture(scope="module")
def lib():
    from dpdist_amd import build, lib as L
    build.build(verbose=False)
    return L.load()


def _params(**kw):
    from dpdist_amd.model import DPDistParams
    return DPDistParams(k=5, mlp=(64, 64, 64), device="cpu", **kw)


def test_count_entries_refuse_before_any_hip_call(lib):
    """NULL counts (and every other NULL) is DPD_E_NULL; every other refusal is that of the un-counted twin, without touching a device"""
    from dpdist_amd import lib as L
    p = ctypes.c_void_p(1 << 30)                          # any non-null "device address": nothing is dereferenced
    cp = L.DecoderParams(*([1 << 30] * 8 + [None] * 3))
    fwd = lambda pts=p, cnt=p, C=2, N=24, m=8, sigma=0.125, tile=8, fv=p: lib.dpd_mfv3d_fwd_counts(pts, cnt, C, N, m, sigma, tile, fv, None)   # noqa: E731
    assert fwd(cnt=None) == -1 and fwd(pts=None) == -1 and fwd(fv=None) == -1
    assert fwd(C=0) == -2 and fwd(sigma=0.0) == -2 and fwd(sigma=float("nan")) == -2
    assert fwd(N=0) == -3 and fwd(N=4097) == -3 and fwd(m=11) == -3 and fwd(m=0) == -3
    assert fwd(tile=4) == -3 and fwd(tile=12) == -3 and fwd(tile=-8) == -3
    big = next(t for t in range(8, 1 << 14, 8) if T.fwd_tiled_lds_bytes(t, 8) > M.LDS_CAP)
    assert fwd(N=4096, tile=big) == -3 and T.fwd_tiled_lds_bytes(big - 8, 8) <= M.LDS_CAP
    ws = 2 * 4 * 33 * 512 * 4
    assert lib.dpd_mfv3d_bwd_workspace_bytes(2, 8) == ws
    bwd = lambda pts=p, cnt=p, dfv=p, C=2, N=24, m=8, sigma=0.125, tile=8, dpts=p, w=p, wb=ws: lib.dpd_mfv3d_bwd_counts(   # noqa: E731
        pts, cnt, dfv, C, N, m, sigma, tile, dpts, w, wb, None)
    assert bwd(cnt=None) == -1 and bwd(pts=None) == -1 and bwd(dfv=None) == -1 and bwd(dpts=None) == -1
    assert bwd(C=0) == -2 and bwd(sigma=-1.0) == -2
    assert bwd(m=9) == -3 and bwd(N=4097) == -3 and bwd(tile=12) == -3
    assert bwd(w=None) == -4 and bwd(wb=ws - 1) == -4
    big = next(t for t in range(8, 1 << 14, 8) if T.bwd_tiled_lds_bytes(t, 8) > M.LDS_CAP)
    assert bwd(N=4096, tile=big) == -3
    idx = lambda q=p, cnt=p, Cb=2, N=64, m=8, uc=p: lib.dpd_cross_index_counts(q, cnt, Cb, N, m, p, p, p, uc, None)   # noqa: E731
    assert idx(cnt=None) == -1 and idx(q=None) == -1 and idx(uc=None) == -1
    assert idx(m=11) == -3 and idx(Cb=0) == -2 and idx(N=0) == -2 and idx(Cb=1 << 12, N=1 << 13) == -2
    dec = lambda xu=p, qc=p, pairs=6, Cb=2, h=256, cap=384, ldu=384, params=cp: lib.dpd_decoder_fwd_cross_counts(   # noqa: E731
        xu, ldu, cap, p, p, p, p, p, qc, pairs, Cb, 64, KP, h, params, p, p, p, p, p, None)
    assert dec(qc=None) == -1 and dec(xu=None) == -1 and dec(params=None) == -1 and dec(params=L.DecoderParams()) == -1
    assert dec(h=200) == -3 and dec(cap=386, ldu=388) == -3 and dec(cap=384, ldu=256) == -2
    assert dec(Cb=0) == -2 and dec(pairs=7) == -2                   # pairs = surface clouds x Cb
    cpb = L.DecoderParams(*([1 << 30] * 11))
    cap = lib.dpd_cross_slot_capacity(3, 2, 64, 8)
    back = lambda gd=p, qc=p, Ca=3, m=8, k=5, h=256, sc=cap, params=cpb, dfv=p, gq=p: lib.dpd_cross_bwd_counts(   # noqa: E731
        gd, p, qc, p, p, p, p, p, p, p, p, Ca, 2, 64, m, k, KP, h, sc, params, p, p, p, p, p, p, p, dfv, gq, None)
    assert back(qc=None) == -1 and back(gd=None) == -1 and back(params=None) == -1 and back(dfv=None, gq=None) == -1
    assert back(Ca=0) == -2 and back(sc=cap + 32) == -2
    assert back(m=11) == -3 and back(k=4) == -3 and back(h=200) == -3 and back(h=4160) == -3


def test_matrix_checks_the_counts(lib):
    from dpdist_amd import DPDistMatrix, dpdist_matrix
    a, b = torch.zeros(3, 64, 3), torch.zeros(2, 40, 3)
    P = _params()
    for call in (lambda *x, **kw: dpdist_matrix(P, *x, **kw), lambda *x, **kw: DPDistMatrix(P)(*x, **kw)):
        with pytest.raises(ValueError, match="same number of points"):          # differing widths without counts: the old message
            call(a, b)
        with pytest.raises(ValueError, match="one count per cloud"):
            call(a, b, countsA=[64, 37])
        with pytest.raises(ValueError, match="one count per cloud"):
            call(a, b, countsB=torch.tensor([40, 1, 1]))
        with pytest.raises(ValueError, match=r"\[1, 64\]"):
            call(a, b, countsA=[64, 0, 5])
        with pytest.raises(ValueError, match=r"\[1, 40\]"):
            call(a, b, countsA=[64, 37, 5], countsB=(41, 1))
        with pytest.raises(ValueError, match=r"\[1, 64\]"):
            call(a, countsA=np.array([65, 1, 1]))
        with pytest.raises(ValueError, match="integers"):
            call(a, b, countsA=[64.0, 37.0, 5.0])
        with pytest.raises(ValueError, match="countsB given without cloudsB"):
            call(a, countsA=[64, 37, 5], countsB=[1, 1, 1])
        # good counts get as far as the device check: the widths may differ once one set is counted
        with pytest.raises(ValueError, match="GPU"):
            call(a, b, countsA=[64, 37, 5])
        with pytest.raises(ValueError, match="GPU"):
            call(a, b, countsB=torch.tensor([40, 1]))
        with pytest.raises(ValueError, match="GPU"):
            call(a, countsA=(64, 37, 5))
    with pytest.raises(TypeError):                                          # keywords only
        dpdist_matrix(P, a, b, 16384, False, None, None, [64, 37, 5])


def test_chunk_check_walks_each_direction_by_its_query_width(lib):
    from dpdist_amd import pairwise

    class _P:
        k, KP, H = 5, KP, 64

    seen = []

    class _Lib:
        @staticmethod
        def report(ca, Cq, N, m, k, kp, H):
            seen.append((ca, Cq, N))
            return 1

    pairwise.check_chunks(_Lib, "report", _P, 8, 3, 2, 64, 100, Nb=40)
    assert sorted(seen) == [(1, 2, 40), (1, 3, 64)]        # A against B's queries: 80 rows per surface cloud; B against A's: 192
    seen.clear()
    pairwise.check_chunks(_Lib, "report", _P, 8, 3, 2, 64, 100)
    assert sorted(seen) == [(1, 2, 64), (1, 3, 64)]


def test_pad_clouds():
    import dpdist_amd
    from dpdist_amd import pairwise
    assert dpdist_amd.pad_clouds is pairwise.pad_clouds
    rng = np.random.default_rng(5)
    clouds = [torch.tensor(rng.standard_normal((n, 3)).astype(np.float32)) for n in (5, 1, 9)]
    pts, counts = dpdist_amd.pad_clouds(clouds)
    assert pts.shape == (3, 9, 3) and pts.dtype == torch.float32 and pts.is_contiguous()
    assert counts.dtype == torch.int32 and counts.tolist() == [5, 1, 9]
    for c, t in enumerate(clouds):
        assert torch.equal(pts[c, :t.shape[0]], t) and not pts[c, t.shape[0]:].view(torch.int32).any()        # +0.0 padding
    assert not pts.requires_grad
    for bad in ([], [torch.zeros(0, 3)], [torch.zeros(4, 2)], [torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.float64)], [np.zeros((4, 3))]):
        with pytest.raises(ValueError):
            dpdist_amd.pad_clouds(bad)


@pytest.mark.parametrize("case", RC.ENC_CASES, ids=lambda c: "C%d-N%d-m%d" % (c.C, c.N, c.m))
def test_encoder_cases_are_admitted(case):
    """every cloud of every ragged encoder case, alone: the admission of tests/mfv_cases.py, and the float32 oracle within a quarter of
    the bar the kernel is held to, forward and backward (else the case is reseeded: ragged_cases.RESEED)"""
    assert len(case.counts) == case.C and all(1 <= n <= case.N for n in case.counts) and max(case.counts) == case.N
    for c, n in enumerate(case.counts):
        ref = RC.enc_forward_ref(case, c)
        assert ref.fv64.shape == (1, case.m ** 3, M.F)
        M.check_conditioning(ref, (case, c))
        assert ref.d32 <= 0.25 * ref.bar, (case, c)
        if case.backward:
            b = RC.enc_backward_ref(case, c)
            assert b.g64.shape == (1, n, 3) and (b.err32 <= 0.25 * b.bar).all(), (case, c, b.err32, b.bar)
            assert np.abs(b.g64).max() > 20 * b.bar.max(), "a reference gradient without structure makes the bar vacuous"
    if case.counts in RC.BWD_SLICES:
        assert tuple(M.point_slices(n) for n in case.counts) == RC.BWD_SLICES[case.counts]
    if case.tile == 512:
        assert T.fwd_tiled_lds_bytes(512, case.m) == 121360 and M.LDS_OPT_IN < 121360 <= M.LDS_CAP and case.counts[1] % 512 == 1


def test_the_padding_of_a_case_is_not_part_of_its_reference():
    case = RC.ENC_CASES[0]
    assert RC.cloud(case, 1).shape == (1, 17, 3) and np.array_equal(RC.cloud(case, 1)[0], RC.enc_points(case)[1, :17])
    A, B = RC.sets()
    assert A.shape == (3, 64, 3) and B.shape == (2, 40, 3)
    moved = RC.with_padding(A, RC.COUNTS_A, 5.0)
    assert np.array_equal(moved[1, :37], A[1, :37]) and (moved[1, 37:] == 5.0).all() and (moved[2, 5:] == 5.0).all() and np.array_equal(moved[0], A[0])


@pytest.mark.parametrize("self_matrix", [False, True], ids=["two_sets", "self"])
def test_matrix_sets_are_admitted(self_matrix):
    """the composed oracle (oracle.restate.mfv3d, local_window, voxel_lookup, decoder per pair and direction on the truncated clouds) in
    float32 against float64: every directed distance within 1.5e-6 (a quarter of the 1e-4 bar is 2.5e-5), the gradients within a quarter
    of the bar they are held to; distances with structure (0 .. 1.44 for the two sets), gradients with structure"""
    o64, o32 = RC.matrix_oracle(torch.float64, self_matrix), RC.matrix_oracle(torch.float32, self_matrix)
    d32 = max(np.abs(a - b).max() for a, b in zip(o64, o32))
    lo, hi = min(x.min() for x in o64[1:]), max(x.max() for x in o64[1:])
    print("float32 oracle vs float64, distances: %.3e; directed distances %.4f .. %.4f" % (d32, lo, hi))
    assert d32 <= RC.ADMIT_FWD <= 0.25 * RC.FWD_BAR
    assert o64[0].max() - o64[0].min() > 0.05
    if self_matrix:
        assert np.array_equal(o64[2], o64[1].T)
    else:
        assert o64[0].shape == (3, 2) and lo == 0.0 and 1.43 < hi < 1.44           # the single query of B_1 on the lower relu6 saturation
    for name, (ref, bar), g32 in zip(("gA", "gB"), RC.grad_bars(self_matrix), RC.matrix_oracle_grads(torch.float32, self_matrix)):
        e32 = np.abs(g32 - ref).max()
        print("%s: max|ref| %.3f, float32 oracle within %.3e (%.3e of max|ref|), bar %.3e" % (name, np.abs(ref).max(), e32, e32 / np.abs(ref).max(), bar))
        assert e32 <= 0.25 * bar and e32 <= RC.ADMIT_GRAD * max(1.0, np.abs(ref).max()), name
        assert np.abs(ref).max() > 20 * bar, "a reference gradient without structure makes the bar vacuous"
    # the padded rows of the references are zero, the rest is not
    gA = RC.matrix_oracle_grads(torch.float64, self_matrix)[0]
    assert not gA[1, 37:].any() and not gA[2, 5:].any() and np.abs(gA[2, :5]).max() > 0

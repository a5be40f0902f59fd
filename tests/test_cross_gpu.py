"""All-pairs DPDist (dpd_cross_index + dpd_cross_gather + dpd_decoder_fwd_cross, dpdist_amd.pairwise.dpdist_matrix).

Every cloud of a set A (the surface clouds) against every query of a set B: the voxel of a query does not depend on the surface cloud,
so the index is taken once over the queries and layer 1 runs over Ca * U slots.  Data movement is a bit-for-bit statement against the
plain gather on the hand-tiled pairs, the decoder against dpd_decoder_fwd on those rows, the matrix against the float64 oracle and
against the library's own pair path.  Every output sits in a NaN-filled guard-banded buffer (tests/gemm_cases.py).
"""
import functools

import numpy as np
import pytest
import torch

from dpdist_amd import synth
from tests import gemm_cases as G

pytestmark = pytest.mark.gpu

M_GRID, K_WIN, H_DEC = 8, 5, 256
KP, KW = 2528, 2496
NG = M_GRID ** 3
SHAPES = [(3, 2, 64), (2, 3, 36), (1, 1, 64)]            # (Ca, Cb, N): not square; 108 rows per surface cloud (pad rows); the smallest
KINDS = ["random", "one_voxel", "distinct", "outside"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible")
    from dpdist_amd import lib
    lib.load()
    return torch.device("cuda:0")


def _centres():
    return (-1.0 + np.arange(M_GRID) * (2.0 / M_GRID)) + 1.0 / M_GRID


@functools.lru_cache(maxsize=None)
def _queries(kind, C, N):
    """q [C, N, 3] (float32, read-only), the kinds of tests/test_unique_l1_gpu.py over a whole SET of clouds.  random: C * N queries over
    4^3 voxels (repeats inside and across clouds); one_voxel: every query of every cloud in one voxel (U = 1); distinct: all C * N queries
    in different voxels (U = C * N, the bound); outside: `random` with queries outside the cube before, between and after real voxel-0
    queries (a masked query shares voxel 0's window)."""
    rng = np.random.default_rng([C, N, len(kind)])
    cen = _centres()
    jit = rng.uniform(-0.1, 0.1, size=(C, N, 3))               # half a cell is 0.125
    if kind in ("random", "outside"):
        q = rng.uniform(-0.5, 0.5, size=(C, N, 3))
        if kind == "outside":
            q[:, [0, 5, N - 1]] = (1.5, 0.0, 0.0)               # outside in x
            q[:, 20] = (0.0, -1.0, 0.0)                         # on the open lower face of the first cell: outside too
            q[:, [2, 6, 30]] = cen[0] + jit[:, [2, 6, 30]]      # voxel 0
    elif kind == "one_voxel":
        idx = rng.integers(0, M_GRID, size=(1, 1, 3))
        q = cen[idx] + jit
    else:
        assert kind == "distinct" and C * N <= NG
        v = rng.permutation(NG)[:C * N].reshape(C, N)
        q = cen[np.stack([v // 64, (v // 8) % 8, v % 8], -1)] + jit
    q = q.astype(np.float32)
    q.setflags(write=False)
    return q


def _fv(C, seed=3):
    return np.random.default_rng(seed).standard_normal((C, NG, 20)).astype(np.float32)


def _ssq(C, seed=4):
    return np.random.default_rng(seed).uniform(0.1, 2.0, size=(C, 4, 20)).astype(np.float32)


def _bits(t):
    return t.contiguous().view(torch.int32)


class _Cross:
    """dpd_cross_index + dpd_cross_gather into guard-banded buffers, next to the plain gather on the hand-tiled pairs"""

    def __init__(self, dev, Ca, Cb, N, q, fv, ssq):
        from dpdist_amd import lib as L
        lib, s = L.load(), L.cur_stream()
        assert lib.dpd_padded_width(K_WIN) == KP
        self.Ca, self.Cb, self.N = Ca, Cb, N
        self.rows = rows = Ca * Cb * N
        self.rows_p = rows_p = (rows + 31) // 32 * 32
        self.cap = cap = lib.dpd_cross_slot_capacity(Ca, Cb, N, M_GRID)
        assert cap == (Ca * min(NG, Cb * N) + 31) // 32 * 32
        f32, i32 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int32, device=dev)
        self.q, self.fv = torch.tensor(q, device=dev), torch.tensor(fv, device=dev)
        self.ssq = None if ssq is None else torch.tensor(ssq, device=dev)
        self.mask, self.mask_band = G.banded_flat(Cb * N, **f32)
        self.vox, self.vox_band = G.banded_flat(Cb * N, **i32)
        self.slot, self.slot_band = G.banded_flat(NG, **i32)
        self.ucount, self.ucount_band = G.banded_flat(1, **i32)
        self.Xu, self.Xu_band = G.banded((KW, cap), cap, **f32)                  # k-major: [column of X, slot]
        self.Xt, self.Xt_band = G.banded((rows_p, 32), 32, **f32)
        self.uid, self.uid_band = G.banded_flat(rows_p, **i32)
        self.maskr, self.maskr_band = G.banded_flat(rows_p, **f32)
        self.cnt, self.cnt_band = G.banded_flat(4, **i32)
        L.check(lib.dpd_cross_index(L.ptr(self.q), Cb, N, M_GRID, L.ptr(self.mask), L.ptr(self.vox), L.ptr(self.slot), L.ptr(self.ucount), s),
                "dpd_cross_index")
        L.check(lib.dpd_cross_gather(L.ptr(self.q), L.ptr(self.vox), L.ptr(self.mask), L.ptr(self.slot), L.ptr(self.ucount), L.ptr(self.fv),
                                     L.ptr(self.ssq), Ca, Cb, N, M_GRID, K_WIN, KP, L.ptr(self.Xu), cap, L.ptr(self.Xt), L.ptr(self.uid),
                                     L.ptr(self.maskr), L.ptr(self.cnt), s), "dpd_cross_gather")
        # the plain gather: the queries alone (voxel and mask of the index), then the hand-tiled pairs p = i * Cb + j
        self.mask_ref, self.vox_ref = torch.empty(Cb * N, **f32), torch.empty(Cb * N, **i32)
        Xq = torch.empty(Cb * N, KP, **f32)
        L.check(lib.dpd_patch_rows_fwd(L.ptr(self.q), L.ptr(self.fv[:1].expand(Cb, -1, -1).contiguous()), Cb, N, M_GRID, K_WIN, KP, L.ptr(Xq),
                                       L.ptr(self.mask_ref), L.ptr(self.vox_ref), None, s), "dpd_patch_rows_fwd")
        pairs = Ca * Cb
        q_t = self.q[None].expand(Ca, -1, -1, -1).reshape(pairs, N, 3).contiguous()
        fv_t = self.fv[:, None].expand(-1, Cb, -1, -1).reshape(pairs, NG, 20).contiguous()
        ssq_t = None if ssq is None else self.ssq[:, None].expand(-1, Cb, -1, -1).reshape(pairs, 4, 20).contiguous()
        self.X_ref = torch.empty(rows, KP, **f32)
        self.maskr_ref, voxr = torch.empty(rows, **f32), torch.empty(rows, **i32)
        L.check(lib.dpd_patch_rows_fwd_scaled(L.ptr(q_t), L.ptr(fv_t), L.ptr(ssq_t), pairs, N, M_GRID, K_WIN, KP, L.ptr(self.X_ref),
                                              L.ptr(self.maskr_ref), L.ptr(voxr), None, s), "dpd_patch_rows_fwd_scaled")
        torch.cuda.synchronize()
        self.U = int(self.ucount[0])

    def bands(self):
        for b in (self.mask_band, self.vox_band, self.slot_band, self.ucount_band, self.Xu_band, self.Xt_band, self.uid_band, self.maskr_band,
                  self.cnt_band):
            b()


@functools.lru_cache(maxsize=None)
def _cross(shape, kind, with_ssq, integer=False):
    """one gather per case, shared by the tests that read it (nothing below writes into it)"""
    Ca, Cb, N = shape
    dev = torch.device("cuda:0")
    fv = G.small_int(np.random.default_rng(9), (Ca, NG, 20), KP).astype(np.float32) if integer else _fv(Ca)
    return _Cross(dev, Ca, Cb, N, _queries(kind, Cb, N), fv, _ssq(Ca) if with_ssq else None)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES)
def test_cross_index(dev, shape, kind):
    """voxel and mask: the bits of dpd_patch_rows_fwd; slots: np.unique of the voxel ids, ascending"""
    Ca, Cb, N = shape
    x = _cross(shape, kind, False)
    assert torch.equal(_bits(x.mask), _bits(x.mask_ref)) and torch.equal(x.vox, x.vox_ref)
    vox = x.vox_ref.cpu().numpy()
    occupied = np.unique(vox)
    slot_ref = np.full(NG, -1, np.int32)
    slot_ref[occupied] = np.arange(len(occupied), dtype=np.int32)
    assert np.array_equal(x.slot.cpu().numpy(), slot_ref)
    assert x.U == len(occupied)
    if kind == "random" and Cb * N > 64:
        assert x.U % 32 and x.U < Cb * N                       # repeats, and a slot count that fills no whole tile
        per_cloud = [set(v) for v in vox.reshape(Cb, N)]
        assert all(len(s) < N for s in per_cloud)                                              # repeats inside a cloud
        assert Cb == 1 or (per_cloud[0] & per_cloud[1])                                        # ... and across clouds
    if kind == "one_voxel":
        assert x.U == 1
    if kind == "distinct":
        assert x.U == Cb * N
    if kind == "outside":
        msk = x.mask_ref.cpu().numpy().reshape(Cb, N)
        assert not msk[:, [0, 5, 20, N - 1]].any() and msk[:, [2, 6, 30]].all()
        v = vox.reshape(Cb, N)
        assert not v[:, [0, 2, 5, 6, 20, 30, N - 1]].any() and slot_ref[0] == 0 and (slot_ref == 0).sum() == 1      # voxel 0 owns one slot
    x.bands()


@pytest.mark.parametrize("with_ssq", [False, True])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES)
def test_cross_gather_is_bitwise_the_plain_gather(dev, shape, kind, with_ssq):
    Ca, Cb, N = shape
    x = _cross(shape, kind, with_ssq)
    U, rows, rows_p = x.U, x.rows, x.rows_p
    uid = x.uid.cpu().numpy()
    slot = x.slot.cpu().numpy()
    vox = x.vox_ref.cpu().numpy().astype(np.int64)
    uid_ref = (np.arange(Ca)[:, None] * U + slot[vox][None, :]).reshape(-1)
    assert np.array_equal(uid[:rows], uid_ref)
    assert x.cnt.cpu().tolist() == [U, Ca * U, 0, 0]
    idx = torch.tensor(uid_ref, device=dev)
    assert torch.equal(_bits(x.Xu[:, idx].t()), _bits(x.X_ref[:, :KW]))
    assert torch.equal(_bits(x.Xt[:rows]), _bits(x.X_ref[:, KW:]))
    assert torch.equal(_bits(x.maskr[:rows]), _bits(x.maskr_ref))
    assert torch.equal(_bits(x.maskr[:rows].view(Ca, Cb * N)), _bits(x.mask_ref[None].expand(Ca, -1)))
    assert G.untouched(x.Xu[:, Ca * U:])                        # nothing beyond the live slots
    if N == 36:
        assert rows_p > rows
    assert not uid[rows:].any() and not _bits(x.Xt[rows:]).any() and not _bits(x.maskr[rows:]).any()      # pad rows
    x.bands()


def _decoder_weights(dev, H, integer, seed=5):
    from dpdist_amd import lib as L
    rng = np.random.default_rng(seed)
    if integer:        # tests/gemm_cases.py: with small-integer operands every partial sum of the window columns is exact
        mk = lambda *s: torch.tensor(G.small_int(rng, s, KP).astype(np.float32), device=dev)   # noqa: E731
    else:
        mk = lambda *s: torch.tensor((rng.standard_normal(s) * 0.05).astype(np.float32), device=dev)   # noqa: E731
    t = [mk(KP, H), mk(H), mk(H, H), mk(H), mk(H, H), mk(H), mk(H, 3), mk(3)]
    return t, L.make_params(*t)


def sum_bound(N):
    """worst case of an fp32 sum of N values in [0, 2], as a bound on their mean: (N - 1) roundings of at most 2^-24 relative on
    partial sums of at most 2 N, divided by N"""
    return (N - 1) * 2.0 ** -24 * 2


@pytest.mark.parametrize("integer", [False, True])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES)
def test_cross_decoder_is_bitwise_the_plain_decoder(dev, shape, kind, integer):
    """y and pred on the real rows == dpd_decoder_fwd on the plain rows of the hand-tiled pairs, torch.equal; Dd == the float64 mean of
    that pred[:, 0] per pair within the fp32 summation bound.  Xu and Pu are NaN beyond the live slots.  one_voxel: Ca * U = Ca live
    slots, 1 at (1, 1, 64) -- fewer than one 32-row tile."""
    from dpdist_amd import lib as L
    lib, s = L.load(), L.cur_stream()
    Ca, Cb, N = shape
    H = H_DEC
    x = _cross(shape, kind, not integer, integer)
    rows, rows_p, pairs = x.rows, x.rows_p, Ca * Cb
    tens, cp = _decoder_weights(dev, H, integer)
    f32 = dict(dtype=torch.float32, device=dev)
    Pu, Pu_band = G.banded((x.cap, H), H, **f32)
    bands = [Pu_band]
    outs = []
    for cols in (H, H, 3, 3):
        v, b = G.banded((rows_p, cols), cols, **f32)
        outs.append(v)
        bands.append(b)
    act0, act1, y, pred = outs
    Dd, Dd_band = G.banded_flat(pairs, **f32)
    bands.append(Dd_band)
    L.check(lib.dpd_decoder_fwd_cross(L.ptr(x.Xu), x.cap, x.cap, L.ptr(x.Xt), L.ptr(x.uid), L.ptr(x.cnt), L.ptr(Pu), L.ptr(x.maskr), pairs, N,
                                      KP, H, cp, L.ptr(act0), L.ptr(act1), L.ptr(y), L.ptr(pred), L.ptr(Dd), s), "dpd_decoder_fwd_cross")
    ref = [torch.empty(rows, c, **f32) for c in (H, H, H, 3, 3)]
    L.check(lib.dpd_decoder_fwd(L.ptr(x.X_ref), L.ptr(x.maskr_ref), rows, KP, H, cp, 0, *[L.ptr(t) for t in ref], None, 0, None, s),
            "dpd_decoder_fwd")
    torch.cuda.synchronize()
    h3_ref, y_ref, pred_ref = ref[2], ref[3], ref[4]
    assert torch.isfinite(ref[0]).all() and float(ref[0].max()) > 0
    assert torch.equal(_bits(act0[:rows]), _bits(h3_ref)), "h3"
    assert torch.equal(_bits(y[:rows]), _bits(y_ref)), "y"
    assert torch.equal(_bits(pred[:rows]), _bits(pred_ref)), "pred"
    assert not _bits(pred[rows:]).any()                         # pad rows carry mask 0
    want = pred_ref[:, 0].double().view(pairs, N).mean(1)
    err = float((Dd.double() - want).abs().max())
    print("Dd vs float64 mean: %.3e (bound %.3e)" % (err, sum_bound(N)))
    assert err <= sum_bound(N)
    if kind == "one_voxel":
        assert x.U == 1 and x.cnt.cpu().tolist()[1] == Ca
    assert G.untouched(Pu[Ca * x.U:])
    for band in bands:
        band()
    x.bands()
    del tens


# ---- the public interface ----
@functools.lru_cache(maxsize=None)
def _sets(shape):
    Ca, Cb, N = shape
    A = synth.s2_modelnet_shaped(Ca, N, 100)[0].astype(np.float32)
    B = synth.s2_modelnet_shaped(Cb, N, 101)[1].astype(np.float32)
    for t in (A, B):
        t.setflags(write=False)
    return A, B


def _tiled(A, B):
    """the hand-tiled pairs p = i * Cb + j: (A_i, B_j)"""
    Ca, Cb = A.shape[0], B.shape[0]
    return np.repeat(A, Cb, axis=0), np.tile(B, (Ca, 1, 1))


@functools.lru_cache(maxsize=None)
def _oracle(shape):
    """D, D_AB, D_BA of oracle.restate.get_model / get_loss in float64 on the hand-tiled pairs"""
    from oracle import restate as R
    Ca, Cb, N = shape
    A, B = _sets(shape)
    W = R.as_torch_weights(synth.make_weights("wide", mlp=(H_DEC,) * 3), torch.float64)
    a, b = (torch.tensor(t, dtype=torch.float64) for t in _tiled(A, B))
    ps, _ = R.get_model(a, b, W, m=M_GRID, k=K_WIN, sigma=0.125)
    d_ab = ps["pred_listAB"][:, :, 0, 0].mean(1).view(Ca, Cb)
    d_ba = ps["pred_listBA"][:, :, 0, 0].mean(1).view(Ca, Cb)
    D = torch.stack([R.get_loss({k: v[p:p + 1] for k, v in ps.items()}, torch.zeros(1, N, dtype=torch.float64))[1] for p in range(Ca * Cb)])
    return D.view(Ca, Cb), d_ab, d_ba


def _params(dev, **kw):
    from dpdist_amd.model import DPDistParams
    P = DPDistParams(k=K_WIN, mlp=(H_DEC,) * 3, device=dev, init=None, **kw)
    P.load_tf_state_dict(synth.make_weights("wide", mlp=(H_DEC,) * 3))
    return P


@pytest.mark.parametrize("shape", SHAPES)
def test_matrix_against_the_oracle_and_the_pair_path(dev, shape):
    """D, D_AB, D_BA within 1e-4 absolute of the float64 oracle on the hand-tiled pairs (the fp32 forward bar); within the fp32
    summation bound of the library's own pair path (get_model on the tiled pairs, the mean over the points in float64)."""
    from dpdist_amd import dpdist_matrix
    from dpdist_amd import model as Mo
    Ca, Cb, N = shape
    A, B = _sets(shape)
    P = _params(dev)
    cu = lambda t: torch.tensor(t, device=dev)      # noqa: E731
    D, d_ab, d_ba = dpdist_matrix(P, cu(A), cu(B), return_directed=True)
    assert D.shape == d_ab.shape == d_ba.shape == (Ca, Cb)
    Do, abo, bao = _oracle(shape)
    assert float(Do.max() - Do.min()) > 0.05 or Ca * Cb == 1           # a matrix with structure, not a constant
    for name, got, want in (("D", D, Do), ("D_AB", d_ab, abo), ("D_BA", d_ba, bao)):
        err = float((got.double().cpu() - want).abs().max())
        print("%s vs float64 oracle: %.3e" % (name, err))
        assert err <= 1e-4, name
    a_t, b_t = (cu(t) for t in _tiled(A, B))
    with torch.no_grad():
        ps, _, _ = Mo.get_model(a_t, b_t, True, bn=0, pn="3dmfv", k=K_WIN, localSNmlp=[H_DEC] * 3, sigma3dmfv=0.125, params=P)
    for name, got, key in (("D_AB", d_ab, "pred_listAB"), ("D_BA", d_ba, "pred_listBA")):
        want = ps[key][:, :, 0, 0].double().mean(1).view(Ca, Cb)
        err = float((got.double() - want).abs().max())
        print("%s vs the pair path: %.3e (bound %.3e)" % (name, err, sum_bound(N)))
        assert err <= sum_bound(N), name


@pytest.mark.parametrize("shape", SHAPES[:2])
def test_matrix_does_not_depend_on_the_chunking(dev, shape):
    from dpdist_amd import dpdist_matrix
    A, B = (torch.tensor(t, device=dev) for t in _sets(shape))
    P = _params(dev)
    one = dpdist_matrix(P, A, B, max_rows=1 << 20, return_directed=True)
    per_cloud = dpdist_matrix(P, A, B, max_rows=1, return_directed=True)         # every chunk holds one surface cloud
    for x, y in zip(one, per_cloud):
        assert torch.equal(_bits(x), _bits(y))


def test_self_matrix_comes_from_one_direction(dev):
    from dpdist_amd import dpdist_matrix
    A = torch.tensor(_sets(SHAPES[0])[0], device=dev)
    P = _params(dev)
    D = dpdist_matrix(P, A)
    assert D.shape == (3, 3) and torch.equal(_bits(D), _bits(dpdist_matrix(P, A, A)))
    assert torch.equal(_bits(D), _bits(D.t()))


def test_matrix_takes_a_model_and_refuses_other_compute_types(dev):
    from dpdist_amd import dpdist_matrix
    from dpdist_amd.model import DPDistModel
    A, B = (torch.tensor(t, device=dev) for t in _sets(SHAPES[0]))
    mod = DPDistModel(Embedding_Size=512, k=K_WIN, localSNmlp=(H_DEC,) * 3, sigma3dmfv=0.125, device=dev)
    mod.load_tf_state_dict(synth.make_weights("wide", mlp=(H_DEC,) * 3))
    assert torch.equal(_bits(dpdist_matrix(mod, A, B)), _bits(dpdist_matrix(_params(dev), A, B)))
    with pytest.raises(ValueError, match="fp32"):
        dpdist_matrix(_params(dev, compute_dtype="bf16"), A, B)
    with pytest.raises(ValueError, match="same number of points"):
        dpdist_matrix(_params(dev), A, B[:, :36].contiguous())
    with pytest.raises(ValueError, match="contradicts"):
        dpdist_matrix(mod, A, B, Embedding_Size=1000)
    with pytest.raises(ValueError, match="contradicts"):
        dpdist_matrix(mod, A, B, sigma3dmfv=0.25)
    assert torch.equal(_bits(dpdist_matrix(mod, A, B, Embedding_Size=512, sigma3dmfv=0.125)), _bits(dpdist_matrix(mod, A, B)))
    with pytest.raises(ValueError, match="not supported"):          # a grid the entries do not take (m = 11)
        dpdist_matrix(_params(dev), A, B, Embedding_Size=1331)

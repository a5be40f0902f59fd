"""Layer 1 over distinct windows (dpd_patch_rows_fwd_unique + dpd_decoder_fwd_unique, trainer option `unique_l1`).

The window part of a decoder row depends on (cloud, voxel) only.  The index gives every row the slot of the first row of its cloud
with the same voxel, the gather writes the window once per slot (k-major: one column of Xu per slot), layer 1 contracts its first
KP - 32 columns over the slots and a finish launch continues each row's fp32 accumulator chain with the last 32 columns.  Everything here is a bit-for-bit statement:
data movement against dpd_patch_rows_fwd_scaled, the index against a numpy first-occurrence restatement, h1 against dpd_decoder_fwd,
the training step against the same trainer with the option off.  Every output sits in a wider NaN-filled buffer (tests/gemm_cases.py).
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from dpdist_amd import synth
from tests import gemm_cases as G

pytestmark = pytest.mark.gpu

M_GRID, K_WIN, N_PTS = 8, 5, 64
KP, KW = 2528, 2496                 # padded row width; the columns layer 1 contracts once per window


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
def _queries(kind, C):
    """q [C, N, 3] (float32, read-only).  random: 64 queries over 4^3 voxels (duplicates inside every cloud); one_voxel: all queries
    of a cloud in one voxel (U = C); distinct: 64 queries in 64 different voxels (U = Q); outside: `random` with queries outside the
    cube before, between and after real voxel-0 queries (a masked query shares voxel 0's window)."""
    rng = np.random.default_rng([C, len(kind)])
    cen = _centres()
    jit = rng.uniform(-0.1, 0.1, size=(C, N_PTS, 3))          # half a cell is 0.125
    if kind in ("random", "outside"):
        q = rng.uniform(-0.5, 0.5, size=(C, N_PTS, 3))
        if kind == "outside":
            q[:, [0, 5, 63]] = (1.5, 0.0, 0.0)                 # outside in x
            q[:, 40] = (0.0, -1.0, 0.0)                        # on the open lower face of the first cell: outside too
            q[:, [2, 6, 50]] = cen[0] + jit[:, [2, 6, 50]]     # voxel 0
    elif kind == "one_voxel":
        idx = rng.integers(0, M_GRID, size=(C, 1, 3))
        q = cen[idx] + jit
    else:
        assert kind == "distinct"
        q = np.empty((C, N_PTS, 3))
        for c in range(C):
            v = rng.permutation(M_GRID ** 3)[:N_PTS]
            q[c] = cen[np.stack([v // 64, (v // 8) % 8, v % 8], -1)] + jit[c]
    q = q.astype(np.float32)
    q.setflags(write=False)
    return q


def _first_occurrence(vox, C, Qb):
    """numpy restatement of the index: uid [Q], (U_AB, M_u, U_ABp), the rows that own a slot"""
    vox = vox.reshape(C, N_PTS)
    own = np.zeros((C, N_PTS), bool)
    firstrow = np.zeros((C, N_PTS), np.int64)
    for c in range(C):
        seen = {}
        for n in range(N_PTS):
            v = int(vox[c, n])
            if v not in seen:
                seen[v] = n
                own[c, n] = True
            firstrow[c, n] = c * N_PTS + seen[v]
    own = own.reshape(-1)
    u_ab = int(own[:Qb].sum())
    u_abp = (u_ab + 31) // 32 * 32
    slot = np.cumsum(own) - 1
    slot[Qb:] += u_abp - u_ab
    return slot[firstrow.reshape(-1)].astype(np.int32), (u_ab, u_abp + int(own[Qb:].sum()), u_abp), own


class _Unique:
    """one call of dpd_patch_rows_fwd_unique into guard-banded buffers, next to dpd_patch_rows_fwd_scaled on the same inputs"""

    def __init__(self, dev, q, fv, ssq):
        from dpdist_amd import lib as L
        lib, s = L.load(), L.cur_stream()
        C = q.shape[0]
        self.C, self.Q, self.Qb = C, C * N_PTS, (C // 2) * N_PTS
        Q, Qb = self.Q, self.Qb
        assert lib.dpd_padded_width(K_WIN) == KP
        self.q, self.fv = torch.tensor(q, device=dev), torch.tensor(fv, device=dev)
        self.ssq = None if ssq is None else torch.tensor(ssq, device=dev)
        f32, i32 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int32, device=dev)
        self.X, self.X_band = G.banded((Qb, KP), KP, **f32)
        self.Xu, self.Xu_band = G.banded((KW, Q + 32), Q + 32, **f32)           # k-major: [column of X, slot]
        self.Xt, self.Xt_band = G.banded((Q, 32), 32, **f32)
        self.mask, self.mask_band = G.banded_flat(Q, **f32)
        self.vox, self.vox_band = G.banded_flat(Q, **i32)
        self.uid, self.uid_band = G.banded_flat(Q, **i32)
        self.cnt, self.cnt_band = G.banded_flat(4, **i32)
        nb = lib.dpd_patch_rows_unique_scratch_bytes(C, N_PTS)
        self.scratch = torch.empty(nb, dtype=torch.uint8, device=dev)
        L.check(lib.dpd_patch_rows_fwd_unique(L.ptr(self.q), L.ptr(self.fv), L.ptr(self.ssq), C, N_PTS, M_GRID, K_WIN, KP, Qb, L.ptr(self.X), Qb,
                                              L.ptr(self.Xu), L.ptr(self.Xt), L.ptr(self.mask), L.ptr(self.vox), L.ptr(self.uid),
                                              L.ptr(self.cnt), L.ptr(self.scratch), nb, s), "dpd_patch_rows_fwd_unique")
        self.X_ref = torch.empty(Q, KP, **f32)
        self.mask_ref, self.vox_ref = torch.empty(Q, **f32), torch.empty(Q, **i32)
        L.check(lib.dpd_patch_rows_fwd_scaled(L.ptr(self.q), L.ptr(self.fv), L.ptr(self.ssq), C, N_PTS, M_GRID, K_WIN, KP, L.ptr(self.X_ref),
                                              L.ptr(self.mask_ref), L.ptr(self.vox_ref), None, s), "dpd_patch_rows_fwd_scaled")
        torch.cuda.synchronize()

    def bands(self):
        for b in (self.X_band, self.Xu_band, self.Xt_band, self.mask_band, self.vox_band, self.uid_band, self.cnt_band):
            b()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _fv(C, seed=3):
    return np.random.default_rng(seed).standard_normal((C, M_GRID ** 3, 20)).astype(np.float32)


def _ssq(C, seed=4):
    return np.random.default_rng(seed).uniform(0.1, 2.0, size=(C, 4, 20)).astype(np.float32)


@pytest.mark.parametrize("with_ssq", [False, True])
@pytest.mark.parametrize("kind", ["random", "one_voxel", "distinct", "outside"])
@pytest.mark.parametrize("B", [2, 3])
def test_window_index_and_gather(dev, B, kind, with_ssq):
    C = 2 * B
    u = _Unique(dev, _queries(kind, C), _fv(C), _ssq(C) if with_ssq else None)
    Q, Qb = u.Q, u.Qb
    assert torch.equal(_bits(u.mask), _bits(u.mask_ref)) and torch.equal(u.vox, u.vox_ref)
    uid_ref, (u_ab, m_u, u_abp), own = _first_occurrence(u.vox_ref.cpu().numpy(), C, Qb)
    if kind == "one_voxel":
        assert (u_ab, m_u) == (B, 32 + B)
    if kind == "distinct":
        assert (u_ab, m_u) == (Qb, Q)
    if kind == "outside":
        msk = u.mask_ref.cpu().numpy().reshape(C, N_PTS)
        assert not msk[:, [0, 5, 40, 63]].any() and msk[:, [2, 6, 50]].all()
        assert (uid_ref.reshape(C, N_PTS)[:, [2, 5, 6, 50, 63]] == uid_ref.reshape(C, N_PTS)[:, [0]]).all()      # one slot for voxel 0
    uid = u.uid.cpu().numpy()
    assert np.array_equal(uid, uid_ref)
    assert u.cnt.cpu().tolist() == [u_ab, m_u, u_abp, 0]
    # every row finds its window in its slot, and its own last 32 columns in Xt: bit for bit
    idx = torch.tensor(uid_ref.astype(np.int64), device=dev)
    assert torch.equal(_bits(u.Xu[:, idx].t()), _bits(u.X_ref[:, :KW]))
    assert torch.equal(_bits(u.Xt), _bits(u.X_ref[:, KW:]))
    assert torch.equal(_bits(u.X), _bits(u.X_ref[:Qb]))
    # gap slots are zero; nothing beyond the live slots is written
    assert not _bits(u.Xu[:, u_ab:u_abp]).any()
    assert G.untouched(u.Xu[:, m_u:])
    u.bands()


def _decoder_weights(dev, H, integer, seed=5):
    from dpdist_amd import lib as L
    rng = np.random.default_rng(seed)
    if integer:        # tests/gemm_cases.py: with small-integer operands every partial sum of the window columns is exact
        mk = lambda *s: torch.tensor(G.small_int(rng, s, KP).astype(np.float32), device=dev)   # noqa: E731
    else:
        mk = lambda *s: torch.tensor((rng.standard_normal(s) * 0.05).astype(np.float32), device=dev)   # noqa: E731
    t = [mk(KP, H), mk(H), mk(H, H), mk(H), mk(H, H), mk(H), mk(H, 3), mk(3)]
    return t, L.make_params(*t)


@pytest.mark.parametrize("integer", [False, True])
@pytest.mark.parametrize("kind", ["one_voxel", "random", "distinct"])
@pytest.mark.parametrize("Q", [128, 256, 384])
def test_layer1_over_distinct_windows_is_bitwise(dev, Q, kind, integer):
    """h1 (and everything behind it) of gather + layer 1 over the slots + finish == dpd_decoder_fwd on the plain rows, torch.equal.
    Live slots M_u: one_voxel 32 + B (the AB half fills B rows of its 32-row block, the smallest M_u the layout has), random: no
    multiple of 32, distinct: Q.  Xu and Pu are NaN beyond the live rows."""
    from dpdist_amd import lib as L
    lib, s = L.load(), L.cur_stream()
    C, H = Q // N_PTS, 256
    fv = G.small_int(np.random.default_rng(9), (C, M_GRID ** 3, 20), KP).astype(np.float32) if integer else _fv(C)
    u = _Unique(dev, _queries(kind, C), fv, None if integer else _ssq(C))
    m_u = int(u.cnt[1])
    if kind == "random":
        assert m_u % 32 and m_u < Q
    if kind == "distinct":
        assert m_u == Q
    if kind == "one_voxel":
        assert m_u == 32 + C // 2
    tens, cp = _decoder_weights(dev, H, integer)
    f32 = dict(dtype=torch.float32, device=dev)
    Pu, Pu_band = G.banded((Q + 32, H), H, **f32)
    outs, bands = [], [Pu_band]
    for which in range(2):
        o = []
        for cols in (H, H, H, 3, 3):
            v, b = G.banded((Q, cols), cols, **f32)
            o.append(v)
            bands.append(b)
        outs.append(o)
    a, b = outs
    L.check(lib.dpd_decoder_fwd_unique(L.ptr(u.Xu), L.ptr(u.Xt), L.ptr(u.uid), L.ptr(u.cnt), L.ptr(Pu), L.ptr(u.mask), Q, KP, H, cp,
                                       *[L.ptr(t) for t in a], s), "dpd_decoder_fwd_unique")
    L.check(lib.dpd_decoder_fwd(L.ptr(u.X_ref), L.ptr(u.mask_ref), Q, KP, H, cp, 0, *[L.ptr(t) for t in b], None, 0, None, s), "dpd_decoder_fwd")
    torch.cuda.synchronize()
    assert torch.isfinite(b[0]).all() and float(b[0].max()) > 0
    for name, x, y in zip(("h1", "h2", "h3", "y", "pred"), a, b):
        assert torch.equal(_bits(x), _bits(y)), name
    assert G.untouched(Pu[m_u:])
    for band in bands:
        band()
    u.bands()
    del tens


def _trainer(dev, B, W0, **kw):
    from dpdist_amd.model import DPDistParams
    from dpdist_amd.trainer import DPDistTrainer
    P = DPDistParams(device=dev)
    P.load_tf_state_dict(W0)
    return P, DPDistTrainer(P, B, base_lr=1e-3, distributed=False, **kw)


def test_trainer_with_distinct_windows_is_bitwise_the_plain_trainer(dev):
    """B = 4, exact fp32, two different batches in turn (the number of distinct windows changes between steps), then three more steps:
    loss, pred, activations, every gradient and the weights equal the option-off trainer's bit for bit (the weight gradient of layer 1
    still contracts over the rows of X, so it is bitwise too; tests/test_gpu_parity.py::test_trainer_steps_vs_oracle runs the same
    batch on the default form against the oracle).  The four-launch front end and the prefetch pipeline give the same bits."""
    B = 4
    cu = lambda a: torch.tensor(a, device=dev)      # noqa: E731
    batches = [tuple(cu(x) for x in synth.s2_modelnet_shaped(B, 64, 100 + i)) for i in range(2)]
    order = [0, 1, 0, 1, 0]
    W0 = synth.make_weights("wide")
    runs = {}
    for name, kw, prefetch in (("off", dict(options={"unique_l1": False}), False), ("on", {}, False),
                               ("front4", dict(options={"front2": False}), False), ("prefetch", {}, True)):
        P, tr = _trainer(dev, B, W0, **kw)
        assert tr.unique_l1 == (name != "off")
        snaps = []
        for i, bi in enumerate(order):
            a, b, l = batches[bi]
            nxt = batches[order[i + 1]][:2] + (None,) if prefetch and i + 1 < len(order) else None
            tr.step(a, b, l, prefetch=nxt)
            torch.cuda.synchronize()
            snaps.append({k: getattr(tr, k).clone() for k in ("loss", "pred", "h1", "h2", "h3", "g1", "g2", "g3", "grad")})
            snaps[-1]["params"] = P.flat.detach().clone()
        if prefetch:
            assert tr.prefetch_hits == len(order) - 1
        runs[name] = snaps
        if name == "on":
            counts = tr.ucnt.cpu().tolist()
            assert 0 < counts[0] < tr.BN and counts[2] % 32 == 0 and counts[1] < tr.Q
    for name in ("on", "front4", "prefetch"):
        for t, (x, y) in enumerate(zip(runs[name], runs["off"])):
            for k in x:
                assert torch.equal(_bits(x[k]), _bits(y[k])), (name, t, k)


def test_unique_l1_falls_back_by_shape(dev):
    """plane compute types and shapes the two entries do not take keep the plain gather"""
    from dpdist_amd.model import DPDistParams
    from dpdist_amd.trainer import DPDistTrainer
    P = DPDistParams(device=dev, compute_dtype="bf16")
    assert not DPDistTrainer(P, 2, distributed=False).unique_l1
    P = DPDistParams(device=dev)
    assert not DPDistTrainer(P, 2, num_point=36, distributed=False).unique_l1
    assert DPDistTrainer(P, 2, distributed=False).unique_l1
    lib = __import__("dpdist_amd.lib", fromlist=["load"]).load()
    assert lib.dpd_patch_rows_fwd_unique(None, None, None, 2, 64, 8, 5, KP, 64, None, 0, None, None, None, None, None, None, None,
                                         ctypes.c_size_t(0), None) == -1

"""Ragged sets (clouds of different sizes inside a set; dpd_mfv3d_fwd_counts / dpd_mfv3d_bwd_counts, dpd_cross_index_counts,
dpd_decoder_fwd_cross_counts, dpd_cross_bwd_counts, the countsA / countsB keywords of dpdist_matrix / DPDistMatrix): case tables, clouds,
references and the two encoder entries on guard-banded buffers, for tests/test_ragged_gpu.py; tests/test_ragged_cpu.py runs the admission
of every case here without a GPU.  Method, bars and checkers are those of tests/mfv_cases.py, tests/test_cross_gpu.py and
tests/test_cross_grad_gpu.py (imported, not restated).  Not a test module and not a conftest.

A ragged set is a padded tensor [C, N, 3] plus counts [C]: cloud c is its first counts[c] points.  The reference of every cloud is the
oracle on the TRUNCATED cloud alone; the matrix-level oracle is composed per pair and direction from oracle.restate.mfv3d, local_window,
voxel_lookup and decoder on the truncated clouds (oracle.restate.get_model itself needs equal sizes).
"""
import collections
import functools

import numpy as np
import torch

from dpdist_amd import synth
from oracle import restate as R

from . import mfv_cases as M
from . import test_cross_gpu as X
from . import test_cross_grad_gpu as XG

S0 = M.S0
M_GRID, K_WIN, H_DEC = X.M_GRID, X.K_WIN, X.H_DEC

# ------------------------------------------------------------------------------------------------ the encoder entries
# (C, N, m, counts, tile, backward too)
EncCase = collections.namedtuple("EncCase", "C N m counts tile backward")
ENC_CASES = (
    EncCase(4, 24, 8, (24, 17, 8, 1), 8, True),        # a full cloud, a last tile of one point, exactly one tile, a single point
    EncCase(2, 9, 3, (9, 3), 8, True),                 # m no power of two; a cloud smaller than the slices of its neighbour
    EncCase(2, 300, 8, (300, 249), 0, True),           # the library's tile: more than one tile per cloud (forward), per slice not
    EncCase(2, 600, 8, (600, 513), 512, False),       # 121 360 bytes of dynamic LDS: above the opt-in threshold; a last tile of one point
)
BWD_SLICES = {(24, 17, 8, 1): ([6, 6, 6, 6], [5, 5, 5, 2], [2, 2, 2, 2], [1, 0, 0, 0])}

# seeds replaced because the float32 oracle of a cloud they gave missed the admission of tests/mfv_cases.py (tests/test_ragged_cpu.py)
RESEED = {EncCase(2, 9, 3, (9, 3), 8, True): 4}      # m = 3, three points: seeds 0..3 leave the float32 oracle 1e-5 .. 6e-2 from float64


@functools.lru_cache(maxsize=None)
def enc_points(case):
    """the case's padded clouds [C, N, 3] float32 (read-only); what lies beyond a cloud's count is drawn too and never used as such"""
    rng = np.random.default_rng([RESEED.get(case, 0), 23, case.C, case.N, case.m])
    p = np.ascontiguousarray(rng.uniform(-0.8, 0.8, size=(case.C, case.N, 3)).astype(np.float32))
    p.setflags(write=False)
    return p


def cloud(case, c):
    """cloud c alone: [1, n, 3]"""
    return np.ascontiguousarray(enc_points(case)[c:c + 1, :case.counts[c]])


@functools.lru_cache(maxsize=None)
def enc_forward_ref(case, c):
    return M.make_ref(cloud(case, c), case.m, S0)


@functools.lru_cache(maxsize=None)
def enc_backward_ref(case, c):
    dfv = M.upstream(enc_forward_ref(case, c).fv64, [7, case.C, case.N, case.m, c])
    g64, g32 = M.oracle_backward(cloud(case, c), dfv, case.m, S0)
    return M.BwdRef(dfv, g64, g32, *M.backward_bars(g64, g32))


def nan_padded(case, dev):
    """the padded clouds on the device with the NaN payload of tests/gemm_cases.py in every padded row: the padding is never read"""
    p = torch.tensor(enc_points(case), device=dev)
    bits = p.view(torch.int32)
    for c, n in enumerate(case.counts):
        bits[c, n:] = M.NAN_OUT
    return p


def counts_dev(counts, dev):
    return torch.tensor(counts, dtype=torch.int32, device=dev)


def gpu_forward_counts(pts, counts, m, sigma, tile):
    """dpd_mfv3d_fwd_counts on device tensors -> (return code, fv view [C, G, 20] inside a NaN-payload guard band, band check)"""
    from dpdist_amd import lib as L
    C, N, _ = pts.shape
    G = m ** 3
    view, band = M.banded_flat(C * G * M.F, device=pts.device)
    rc = L.load().dpd_mfv3d_fwd_counts(L.ptr(pts), L.ptr(counts), C, N, m, float(sigma), tile, L.ptr(view), L.cur_stream())
    torch.cuda.synchronize()
    return rc, view.view(C, G, M.F), band


def gpu_backward_counts(pts, counts, dfv, m, sigma, tile):
    """dpd_mfv3d_bwd_counts -> (return code, dpts view [C, N, 3] in a guard band, check of the dpts AND the workspace bands); dpts and the
    workspace hold the NaN payload before the call"""
    from dpdist_amd import lib as L
    lib = L.load()
    C, N, _ = pts.shape
    view, band = M.banded_flat(C * N * 3, device=pts.device)
    ws_bytes = lib.dpd_mfv3d_bwd_workspace_bytes(C, m)
    ws, ws_band = M.banded_flat(ws_bytes // 4, device=pts.device)
    rc = lib.dpd_mfv3d_bwd_counts(L.ptr(pts), L.ptr(counts), L.ptr(dfv), C, N, m, float(sigma), tile, L.ptr(view), L.ptr(ws), ws_bytes,
                                  L.cur_stream())
    torch.cuda.synchronize()

    def bands():
        band()
        ws_band()
    return rc, view.view(C, N, 3), bands


# ------------------------------------------------------------------------------------------------ the public interface
COUNTS_A, COUNTS_B = (64, 37, 5), (40, 1)
FWD_BAR = 1e-4             # the fp32 forward bar of test_matrix_against_the_oracle_and_the_pair_path (absolute)
ADMIT_FWD = 1.5e-6         # float32 oracle against float64, every directed distance
ADMIT_GRAD = 2e-4          # float32 autograd oracle against float64, every gradient entry


@functools.lru_cache(maxsize=None)
def sets():
    """A [3, 64, 3] with counts (64, 37, 5), B [2, 40, 3] with counts (40, 1): float32, read-only; the padding is whatever the generator
    put there (the tests overwrite it)"""
    A = np.ascontiguousarray(synth.s2_modelnet_shaped(3, 64, 100)[0].astype(np.float32))
    B = np.ascontiguousarray(synth.s2_modelnet_shaped(2, 40, 101)[1].astype(np.float32))
    for t in (A, B):
        t.setflags(write=False)
    return A, B


def with_padding(P, counts, value):
    """a copy of the padded set with every padded row set to `value`"""
    out = np.array(P)
    for c, n in enumerate(counts):
        out[c, n:] = value
    return out


@functools.lru_cache(maxsize=None)
def _weights(dtype):
    return R.as_torch_weights(synth.make_weights("wide", mlp=(H_DEC,) * 3), dtype)


def directed(S, Q, dtype):
    """[len(S), len(Q)]: mean over the queries of Q_j of pred(surface S_i ; query)[0] -- models/dpdist_and_aue.py:56-69 and
    utils/dpdist_util.py:494-511, 695-698 for one direction, cloud by cloud (lists of [n, 3] tensors of any sizes)"""
    W = _weights(dtype)
    emb = [R.local_window(R.mfv3d(s[None], M_GRID, 0.125), M_GRID, K_WIN)[0] for s in S]       # [m^3, k^3 * 20]
    rows = []
    for i in range(len(S)):
        row = []
        for q in Q:
            v, mask, loc = R.voxel_lookup(q[None], M_GRID)
            x = torch.cat([loc[0], emb[i][v[0]]], -1)
            y, _ = R.decoder(x, W)
            row.append((y[:, 0] * mask[0]).mean())
        rows.append(torch.stack(row))
    return torch.stack(rows)


def _truncated(P, counts, dtype, grad):
    return [torch.tensor(P[c, :n], dtype=dtype).requires_grad_(grad) for c, n in enumerate(counts)]


def _padded_grads(leaves, grads, width):
    out = np.zeros((len(leaves), width, 3))
    for c, g in enumerate(grads):
        out[c, :g.shape[0]] = g.double().numpy()
    return out


@functools.lru_cache(maxsize=None)
def matrix_oracle(dtype, self_matrix=False):
    """(D, D_AB, D_BA) [Ca, Cb] of the truncated clouds (float64 numpy arrays of the oracle run in `dtype`)"""
    A, B = sets()
    a = _truncated(A, COUNTS_A, dtype, False)
    b = a if self_matrix else _truncated(B, COUNTS_B, dtype, False)
    with torch.no_grad():
        d_ab, d_ba = directed(a, b, dtype), directed(b, a, dtype).t()
    return tuple(t.double().numpy() for t in ((d_ab + d_ba) / 2, d_ab, d_ba))


def upstream(self_matrix=False):
    return XG._upstream((3, 3, 64) if self_matrix else (3, 2, 64))


@functools.lru_cache(maxsize=None)
def matrix_oracle_grads(dtype, self_matrix=False):
    """gradients of (G D).sum() + (G_AB D_AB).sum() + (G_BA D_BA).sum() through the same composition, at the padded shapes (zeros on the
    padding): (gA, gB), or (gA,) for a set against itself"""
    A, B = sets()
    a = _truncated(A, COUNTS_A, dtype, True)
    b = a if self_matrix else _truncated(B, COUNTS_B, dtype, True)
    d_ab, d_ba = directed(a, b, dtype), directed(b, a, dtype).t()
    loss = XG._loss(((d_ab + d_ba) / 2, d_ab, d_ba), upstream(self_matrix), True, dtype)
    if self_matrix:
        return (_padded_grads(a, torch.autograd.grad(loss, a), A.shape[1]),)
    g = torch.autograd.grad(loss, a + b)
    return _padded_grads(a, g[:len(a)], A.shape[1]), _padded_grads(b, g[len(a):], B.shape[1])


def grad_bars(self_matrix=False):
    """[(ref, bar)] per gradient, formed as tests/test_cross_grad_gpu.py: _bar forms it (which is tied to its own equal-sized sets)"""
    r64, r32 = matrix_oracle_grads(torch.float64, self_matrix), matrix_oracle_grads(torch.float32, self_matrix)
    return [(a, max(4.0 * np.abs(b - a).max(), 2e-4 * max(1.0, np.abs(a).max()))) for a, b in zip(r64, r32)]

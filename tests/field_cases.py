"""Per-point DPDist field (dpdist_amd.field: dpd_field_index, dpd_field_gather, dpd_decoder_fwd_field, dpdist_field / DPDistField): the
reference case and the composed oracle, for tests/test_field_gpu.py; tests/test_field_cpu.py runs the admission here without a GPU.
Constants, weights, bars and checkers are those of tests/test_cross_gpu.py, tests/ragged_cases.py, tests/pairs_cases.py and
tests/gemm_cases.py (imported, not restated).  Not a test module and not a conftest.

The oracle is composed per cloud from oracle.restate.mfv3d, local_window, voxel_lookup and decoder on the TRUNCATED cloud and its real
queries, exactly as ragged_cases.directed does, but without the mean.
"""
import functools

import numpy as np
import torch

from oracle import restate as R

from . import gemm_cases as G
from . import pairs_cases as PC
from . import ragged_cases as RC
from . import test_cross_gpu as X

M_GRID, K_WIN, H_DEC = X.M_GRID, X.K_WIN, X.H_DEC
KP, KW, NG = X.KP, X.KW, X.NG
E = PC.E
FWD_BAR, ADMIT_FWD, ADMIT_GRAD = RC.FWD_BAR, RC.ADMIT_FWD, RC.ADMIT_GRAD
DD_BAR = PC.DD_BAR
NAN_OUT = G.NAN_OUT

# ------------------------------------------------------------------------------------------------ the reference case
T_REF = 150
COUNTS, QCOUNTS = RC.COUNTS_A, (150, 97, 1)
# seeds replaced because the float32 oracle they gave missed the admission (tests/test_field_cpu.py): none so far
RESEED = {}


@functools.lru_cache(maxsize=None)
def surfaces():
    """[3, 64, 3] with counts (64, 37, 5): float32, read-only"""
    return RC.sets()[0]


@functools.lru_cache(maxsize=None)
def queries():
    """[3, 150, 3] with query counts (150, 97, 1): float32, read-only.  Query 7 lies on cell faces and on the closed upper face of the cube
    (inside), query 8 on the open lower face (masked)."""
    q = np.random.default_rng([RESEED.get("queries", 11), 3, T_REF]).uniform(-1.05, 1.05, (3, T_REF, 3)).astype(np.float32)
    q[:, 7] = (0.25, -0.5, 1.0)
    q[:, 8] = (-1.0, 0.0, 0.0)
    q.setflags(write=False)
    return q


def shared_queries():
    """the first cloud's queries as one set [150, 3] evaluated against every cloud"""
    return queries()[0]


@functools.lru_cache(maxsize=None)
def upstream():
    g = np.random.default_rng(5).standard_normal((3, T_REF, 3)).astype(np.float32)
    g.setflags(write=False)
    return g


def _field(s, q, dtype):
    """pred [n, 3], mask [n] of one cloud s [w, 3] at the queries q [n, 3]"""
    W = RC._weights(dtype)
    emb = R.local_window(R.mfv3d(s[None], M_GRID, 0.125), M_GRID, K_WIN)[0]       # [m^3, k^3 * 20]
    v, mask, loc = R.voxel_lookup(q[None], M_GRID)
    y, _ = R.decoder(torch.cat([loc[0], emb[v[0]]], -1), W)
    return y * mask[0][:, None], mask[0]


def _leaves(dtype, shared, grad):
    S = RC._truncated(surfaces(), COUNTS, dtype, grad)
    if shared:
        q = torch.tensor(shared_queries(), dtype=dtype).requires_grad_(grad)
        return S, q, [q[:n] for n in QCOUNTS]
    Q = RC._truncated(queries(), QCOUNTS, dtype, grad)
    return S, Q, Q


def _padded(parts, width):
    out = np.zeros((len(parts), width) + tuple(parts[0].shape[1:]))
    for c, p in enumerate(parts):
        out[c, :p.shape[0]] = p.detach().double().numpy()
    return out


@functools.lru_cache(maxsize=None)
def oracle(dtype, shared=False):
    """(pred [3, 150, 3], mask [3, 150]) of the oracle run in `dtype` on the truncated clouds and their real queries: float64 numpy arrays,
    zeros at the padded queries"""
    S, _, Q = _leaves(dtype, shared, False)
    with torch.no_grad():
        out = [_field(s, q, dtype) for s, q in zip(S, Q)]
    return _padded([o[0] for o in out], T_REF), _padded([o[1] for o in out], T_REF)


@functools.lru_cache(maxsize=None)
def oracle_grads(dtype, shared=False):
    """gradients of (upstream * pred).sum() through the same composition -> (g surfaces [3, 64, 3], g queries [3, 150, 3] or, shared,
    [150, 3]): float64 numpy arrays, zeros on the padding"""
    S, leafQ, Q = _leaves(dtype, shared, True)
    g = torch.tensor(upstream(), dtype=dtype)
    loss = sum((_field(s, q, dtype)[0] * g[c, :q.shape[0]]).sum() for c, (s, q) in enumerate(zip(S, Q)))
    if shared:
        grads = torch.autograd.grad(loss, S + [leafQ])
        return RC._padded_grads(S, grads[:3], surfaces().shape[1]), grads[3].double().numpy()
    grads = torch.autograd.grad(loss, S + leafQ)
    return RC._padded_grads(S, grads[:3], surfaces().shape[1]), RC._padded_grads(leafQ, grads[3:], T_REF)


def grad_bars(shared=False):
    """[(ref, bar)] for the surfaces and the queries, formed as tests/ragged_cases.py: grad_bars forms them"""
    r64, r32 = oracle_grads(torch.float64, shared), oracle_grads(torch.float32, shared)
    return [(a, max(4.0 * np.abs(b - a).max(), 2e-4 * max(1.0, np.abs(a).max()))) for a, b in zip(r64, r32)]


# ------------------------------------------------------------------------------------------------ the entries
# (name, n, T, query kind of tests/test_cross_gpu.py or "reference", query counts | None, first query t0)
ENTRY_CASES = (
    ("smallest", 1, 1, "random", None, 0),
    ("reference", 3, 150, "reference", QCOUNTS, 0),
    ("distinct", 2, 40, "distinct_per_cloud", None, 0),      # U_c = T: the bound of the slot capacity
    ("capacity", 1, 600, "random_wide", None, 0),            # T > m^3: the capacity is m^3
    ("one_voxel", 2, 40, "one_voxel", None, 0),              # U_c = 1
    ("outside", 3, 64, "outside", None, 0),
    ("tile", 3, 86, "reference", QCOUNTS, 64),               # a tile of queries [64, 150) with counts that end inside it (97) and before it (1)
)
PLAN_CASES = ((3, 150, 4096), (3, 150, 150), (3, 150, 64), (1, 1, 1), (2, 20000, 16384))


@functools.lru_cache(maxsize=None)
def entry_queries(name):
    """the WHOLE query tensor [n, M, 3] of an entry case (float32, read-only); the chunk is its queries [t0, t0 + T)"""
    _, n, T, kind, _, t0 = next(c for c in ENTRY_CASES if c[0] == name)
    if kind == "reference":
        return queries()
    if kind == "distinct_per_cloud":      # every query of a cloud in another voxel; the clouds overlap
        rng = np.random.default_rng([n, T, 17])
        cen = X._centres()
        v = np.stack([rng.permutation(NG)[:T] for _ in range(n)])
        q = cen[np.stack([v // 64, (v // 8) % 8, v % 8], -1)] + rng.uniform(-0.1, 0.1, size=(n, T, 3))
    elif kind == "random_wide":           # every voxel once, then the whole cube and a little beyond: more queries than voxels
        rng = np.random.default_rng([n, T, 19])
        cen = X._centres()
        v = np.stack([rng.permutation(NG) for _ in range(n)])
        q = np.concatenate([cen[np.stack([v // 64, (v // 8) % 8, v % 8], -1)] + rng.uniform(-0.1, 0.1, size=(n, NG, 3)),
                            rng.uniform(-1.02, 1.02, size=(n, T - NG, 3))], 1)
    else:
        return X._queries(kind, n, T)
    q = q.astype(np.float32)
    q.setflags(write=False)
    return q

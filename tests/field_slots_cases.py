"""Slot-summed backward of the per-point field (csrc/field_bwd.hip: dpd_field_invert, dpd_field_slot_sum, dpd_field_scatter,
dpd_field_bwd; DPDistField(backward="slots")): numpy restatements of the three steps and the case beyond 8192 queries, for
tests/test_field_slots_gpu.py; tests/test_field_slots_cpu.py shows without a GPU that the restatements composed with float64 g1 rows of
oracle/restate.py reproduce the autograd oracle of tests/field_cases.py.  Constants, weights, clouds and bars are those of
tests/field_cases.py (imported, not restated).  Not a test module and not a conftest.
"""
import functools

import numpy as np
import torch

from oracle import restate as R

from . import field_cases as FC
from . import ragged_cases as RC

M_GRID, K_WIN, H_DEC, KP, NG, E = FC.M_GRID, FC.K_WIN, FC.H_DEC, FC.KP, FC.NG, FC.E


# ------------------------------------------------------------------------------------------------ the three steps, restated
def invert(vox, cap=None):
    """the inverted index of a chunk: vox [n, T] (voxel of every row; a masked or padded query has voxel 0) -> dict with
    U [n], base [n], total; qlist [n, T] (a stable argsort of the slots per cloud); slot_start [cap + 1], slot_vox [cap], slot_cloud [cap]
    indexed by the GLOBAL slot base_c + s, the dead slots as the header states them; uid [n, T] the global slot of every row"""
    vox = np.asarray(vox, dtype=np.int64)
    n, T = vox.shape
    cap = (n * min(NG, T) + 31) // 32 * 32 if cap is None else cap
    occ = [np.unique(v) for v in vox]
    U = np.array([len(o) for o in occ])
    base = np.concatenate([[0], np.cumsum(U)[:-1]])
    total = int(U.sum())
    assert total <= cap
    qlist = np.zeros((n, T), dtype=np.int64)
    uid = np.zeros((n, T), dtype=np.int64)
    start = np.full(cap + 1, n * T, dtype=np.int64)
    svox, scloud = np.full(cap, -1, dtype=np.int64), np.full(cap, -1, dtype=np.int64)
    for c in range(n):
        slots = np.searchsorted(occ[c], vox[c])
        uid[c] = base[c] + slots
        qlist[c] = np.argsort(slots, kind="stable")
        counts = np.bincount(slots, minlength=U[c])
        start[base[c]:base[c] + U[c]] = c * T + np.concatenate([[0], np.cumsum(counts)[:-1]])
        svox[base[c]:base[c] + U[c]] = occ[c]
        scloud[base[c]:base[c] + U[c]] = c
    return dict(n=n, T=T, cap=cap, U=U, base=base, total=total, qlist=qlist, slot_start=start, slot_vox=svox, slot_cloud=scloud, uid=uid)


def slot_sum(g1, inv):
    """g1 [>= n T, H] (rows (c, t)) -> gs [cap, H]: row g = the sum of the rows of slot g's list, in list order; zero rows beyond total"""
    g1 = np.asarray(g1, dtype=np.float64)
    n, T = inv["n"], inv["T"]
    gs = np.zeros((inv["cap"], g1.shape[1]))
    flat = (np.arange(n)[:, None] * T + inv["qlist"]).reshape(-1)          # flat position in qlist -> row
    for g in range(inv["total"]):
        for pos in range(inv["slot_start"][g], inv["slot_start"][g + 1]):
            gs[g] += g1[flat[pos]]
    return gs


def scatter(win, inv, dfv=None):
    """win [>= total, >= E] (row g = the window columns (d0, d1, d2, channel) of slot g's dX) -> dfv [n, m^3, 20]:
    dfv[c, p + d - h] += win[g, d] inside the grid over the cloud's own slots in ascending order, continued from `dfv` when given"""
    m, k, h = M_GRID, K_WIN, (K_WIN - 1) // 2
    out = np.zeros((inv["n"], NG, 20)) if dfv is None else np.array(dfv, dtype=np.float64)
    d = np.stack(np.meshgrid(np.arange(k), np.arange(k), np.arange(k), indexing="ij"), -1).reshape(-1, 3)      # [k^3, 3] in window order
    for g in range(inv["total"]):
        v, c = inv["slot_vox"][g], inv["slot_cloud"][g]
        t = np.array([v // (m * m), (v // m) % m, v % m])[None] + d - h
        ok = ((t >= 0) & (t < m)).all(-1)
        tv = (t[:, 0] * m + t[:, 1]) * m + t[:, 2]
        out[c][tv[ok]] += np.asarray(win[g, :E], dtype=np.float64).reshape(k ** 3, 20)[ok]
    return out


# ------------------------------------------------------------------------------------------------ float64 g1 rows of the oracle
def oracle_rows(s, q, g, dtype=torch.float64):
    """one cloud s [w, 3] (a leaf that requires grad) at its queries q [t, 3] under the upstream g [t, 3] of pred: the oracle's own
    composition (tests/field_cases.py: _field) with the layer-1 pre-activation gradient taken out
    -> (vox [t], g1 [t, H], W1 [3 + E, H] in the ORACLE's column order (q - centre first), fv [1, m^3, 20] with its graph)"""
    W = RC._weights(dtype)
    fv = R.mfv3d(s[None], M_GRID, 0.125)
    emb = R.local_window(fv, M_GRID, K_WIN)[0]
    v, mask, loc = R.voxel_lookup(q[None], M_GRID)
    y, hs = R.decoder(torch.cat([loc[0], emb[v[0]]], -1), W)
    loss = (y * mask[0][:, None] * g).sum()
    gh1 = torch.autograd.grad(loss, hs[0], retain_graph=True)[0]
    g1 = (gh1 * (hs[0] > 0)).detach().numpy()
    w1 = W["pc_compare/dpdist_local/mapper_conv1/weights"]
    return v[0].numpy(), g1, w1.reshape(-1, w1.shape[-1]).detach().numpy(), fv


def restated_grads(shared=False, tile=None):
    """the gradients of tests/field_cases.py: oracle_grads(torch.float64, shared), formed by the three restatements above from the float64
    g1 rows: slot sum, one product per slot, scatter, the encoder's own autograd for the surfaces; g1 . W1[q - centre rows] for the queries.
    tile: the queries of a cloud in tiles of that many, each with its own index, accumulated into dfv in ascending tile order"""
    S, leafQ, Q = FC._leaves(torch.float64, shared, True)
    up = torch.tensor(FC.upstream(), dtype=torch.float64)
    gS, gQ = [], []
    for c, (s, q) in enumerate(zip(S, Q)):
        t_all = q.shape[0]
        vox, g1, W1, fv = oracle_rows(s, q.detach(), up[c, :t_all])
        dfv = None
        step = t_all if tile is None else tile
        for t0 in range(0, t_all, step):
            inv = invert(vox[None, t0:t0 + step])
            gs = slot_sum(g1[t0:t0 + step], inv)
            dfv = scatter(gs @ W1[3:].T, inv, dfv)
        gS.append(torch.autograd.grad(fv, s, torch.tensor(dfv))[0])
        gQ.append(g1 @ W1[:3].T)
    gS = RC._padded_grads(S, gS, FC.surfaces().shape[1])
    if shared:
        out = np.zeros((FC.T_REF, 3))
        for d in gQ:
            out[:d.shape[0]] += d
        return gS, out
    out = np.zeros((len(gQ), FC.T_REF, 3))
    for c, d in enumerate(gQ):
        out[c, :d.shape[0]] = d
    return gS, out


# ------------------------------------------------------------------------------------------------ beyond 8192 queries
# the smallest shape past the LDS limit of the rows backward (dpd_patch_rows_bwd: 8192 queries per cloud): one cloud, one chunk
M_BIG = 8193
# seeds replaced because the float32 oracle they gave missed the admission (tests/test_field_slots_cpu.py).  Among 8193 queries some
# pre-activation usually lies so close to a ReLU kink that float32 and float64 take different sides: seed 11 leaves the float32 surface
# gradient 2.1 from float64 at max |g| 317, seeds 13 to 16 leave 0.03 to 0.59; seeds 12 and 17 pass (3.8e-3 at 219, 4.4e-3 at 344)
RESEED = {"big_queries": 12}


@functools.lru_cache(maxsize=None)
def big_queries():
    """[1, 8193, 3] drawn like tests/field_cases.py: queries (a little beyond the cube, so some are masked): float32, read-only"""
    q = np.random.default_rng([RESEED.get("big_queries", 11), 1, M_BIG]).uniform(-1.05, 1.05, (1, M_BIG, 3)).astype(np.float32)
    q[:, 7] = (0.25, -0.5, 1.0)
    q[:, 8] = (-1.0, 0.0, 0.0)
    q.setflags(write=False)
    return q


def big_surface():
    """[1, 64, 3]: the first cloud of the reference case, all 64 points"""
    return FC.surfaces()[:1]


@functools.lru_cache(maxsize=None)
def big_upstream():
    g = np.random.default_rng(6).standard_normal((1, M_BIG, 3)).astype(np.float32)
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def big_oracle_grads(dtype):
    """(pred [1, 8193, 3], g surface [1, 64, 3], g queries [1, 8193, 3]) of the oracle composed as tests/field_cases.py composes it, run
    in `dtype`: float64 numpy arrays"""
    s = torch.tensor(big_surface()[0], dtype=dtype).requires_grad_(True)
    q = torch.tensor(big_queries()[0], dtype=dtype).requires_grad_(True)
    pred = FC._field(s, q, dtype)[0]
    gs, gq = torch.autograd.grad((pred * torch.tensor(big_upstream()[0], dtype=dtype)).sum(), [s, q])
    return tuple(t.detach().double().numpy()[None] for t in (pred, gs, gq))


def big_grad_bars():
    """[(ref, bar)] for the surface and the queries, by the rule of tests/field_cases.py: grad_bars on this case"""
    r64, r32 = big_oracle_grads(torch.float64)[1:], big_oracle_grads(torch.float32)[1:]
    return [(a, max(4.0 * np.abs(b - a).max(), 2e-4 * max(1.0, np.abs(a).max()))) for a, b in zip(r64, r32)]

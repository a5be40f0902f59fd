"""Cases of the encoder over tiles of points (dpd_mfv3d_fwd_tiled / dpd_mfv3d_bwd_tiled): tables, clouds, references and the two C
entries on guard-banded buffers, for tests/test_mfv_tiled_gpu.py; tests/test_mfv_tiled_cpu.py runs the admission of tests/mfv_cases.py
on every case here without a GPU.  Method, bars and checkers are those of tests/mfv_cases.py (imported, not restated); this module only
adds shapes.  Not a test module and not a conftest.

A case is (kind, C, N, m, sigma) as there.  Kinds: "u" uniform in [-0.8, 0.8]^3; "t2" / "t1" the tie clouds of mfv_cases.tie_partner;
"t3": N = 64, positions 8..15 of every 16 are copies of positions 0..7 of the same 16 -- with tile 8 every copy sits in another tile of
the SAME point slice of the backward (16 points per slice), and in another tile of the forward.
"""
import functools

import numpy as np
import torch

from . import mfv_cases as M

S0 = M.S0
E_DIM, E_UNSUPPORTED, E_WORKSPACE = -2, -3, -4

# 1. tile logic at the smallest shapes where it can go wrong: (case, tile, backward too)
TILE_CASES = (
    (("u", 2, 20, 8, S0), 8, True),        # three tiles, ragged last of 4; backward: slices of 5 points, one tile each
    (("u", 3, 9, 3, S0), 8, True),         # last tile of one point; the sliced backward's empty slice (3, 3, 3, 0)
    (("u", 1, 64, 5, S0), 16, True),       # exact multiples, m no power of two
    (("u", 2, 16, 8, S0), 16, True),       # a single tile
    (("u", 2, 16, 8, S0), 64, True),       # tile > N
    (("u", 1, 24, 10, S0), 8, False),      # more than one batch of Gaussians per wave (slices of 250): forward only (m > 8)
    (("u", 1, 24, 2, S0), 8, True),        # m = 2
    (("u", 2, 100, 8, S0), 8, True),       # backward: slices of 25 points = tiles of 8, 8, 8, 1
)
# 2. one cloud at several tiles, and against the plain entries (N under every plain cap)
SAME_CASE = ("u", 2, 100, 8, S0)
SAME_TILES = (8, 16, 0)
# 3. ties across tiles (tile 8)
TIE_CASES = (("t2", 1, 50, 8, S0), ("t2", 1, 64, 5, S0), ("t3", 1, 64, 5, S0), ("t3", 1, 64, 8, S0))
# 5. beyond the plain caps, default tile
BIG_FWD = (("u", 1, 706, 8, S0), ("u", 1, 712, 8, S0), ("u", 1, 539, 10, S0), ("u", 1, 544, 10, S0), ("u", 2, 2048, 8, S0),
           ("u", 1, 4096, 8, S0))
BIG_BWD = (("u", 1, 1640, 8, S0), ("u", 1, 1637, 8, S0), ("u", 2, 2048, 8, S0))

ALL_FWD = tuple(dict.fromkeys([c for c, _, _ in TILE_CASES] + [SAME_CASE] + list(TIE_CASES) + list(BIG_FWD) + list(BIG_BWD)))
ALL_BWD = tuple(dict.fromkeys([c for c, _, b in TILE_CASES if b] + [SAME_CASE] + list(TIE_CASES) + list(BIG_BWD)))

# seeds replaced because the float32 oracle of the cloud they gave missed the admission of tests/mfv_cases.py (test_mfv_tiled_cpu.py)
RESEED = {}


def tie_partner(kind, N):
    if kind == "t3":
        idx = np.arange(N)
        assert N % 16 == 0
        copy = idx % 16 >= 8
        idx[copy] -= 8
        return idx
    return M.tie_partner(kind, N)


@functools.lru_cache(maxsize=None)
def points(case):
    """the case's clouds [C, N, 3] float32 (read-only): the clouds of tests/mfv_cases.py for a case it has, seeded in its way otherwise"""
    kind, C, N, m, sigma = case
    if kind in ("u", "t1", "t2") and case in M.FWD_CASES + M.BWD_CASES + M.TIE_CASES:
        return M.points(case)
    rng = np.random.default_rng([RESEED.get(case, 0), 11 + "ut".index(kind[0]), C, N, m, int(round(sigma * 1e4))])
    p = rng.uniform(-0.8, 0.8, size=(C, N, 3)).astype(np.float32)
    if kind[0] == "t":
        p = p[:, tie_partner(kind, N)]
    p = np.ascontiguousarray(p, dtype=np.float32)
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def forward_ref(case):
    return M.make_ref(points(case), case[3], case[4])


@functools.lru_cache(maxsize=None)
def backward_ref(case):
    kind, C, N, m, sigma = case
    dfv = M.upstream(forward_ref(case).fv64, [7, C, N, m])
    g64, g32 = M.oracle_backward(points(case), dfv, m, sigma)
    return M.BwdRef(dfv, g64, g32, *M.backward_bars(g64, g32))


# ------------------------------------------------------------------------------------------------ the host's rules, restated
def fwd_tiled_lds_bytes(tile, m):
    """include/dpdist_capi.h, dpd_mfv3d_fwd_tiled"""
    return 4 * (6 * tile * m + 6 * tile + 21 * ((m ** 3 + M.SLICES - 1) // M.SLICES) + 4)


def bwd_tiled_lds_bytes(tile, m):
    """include/dpdist_capi.h, dpd_mfv3d_bwd_tiled (the apply kernel, the larger of the two)"""
    return 4 * (6 * tile * m + 52 * tile + 4)


# ------------------------------------------------------------------------------------------------ the C entries on guard-banded buffers
def gpu_forward_tiled(pts, m, sigma, tile, C=None, N=None):
    """dpd_mfv3d_fwd_tiled on device tensor pts [C, N, 3] -> (return code, fv view [C, G, 20] inside a NaN-payload guard band, band check)"""
    from dpdist_amd import lib as L
    C = pts.shape[0] if C is None else C
    N = pts.shape[1] if N is None else N
    G = min(max(m, 1), 11) ** 3
    view, band = M.banded_flat(max(C, 1) * G * M.F, device=pts.device)
    rc = L.load().dpd_mfv3d_fwd_tiled(L.ptr(pts), C, N, m, float(sigma), tile, L.ptr(view), L.cur_stream())
    torch.cuda.synchronize()
    return rc, view.view(max(C, 1), G, M.F), band


def gpu_backward_tiled(pts, dfv, m, sigma, tile, C=None, N=None, ws_short=0):
    """dpd_mfv3d_bwd_tiled -> (return code, dpts view [C, N, 3] in a guard band, check of the dpts AND the workspace bands, workspace view);
    the workspace is filled with the NaN payload before the call; ws_short: bytes by which the size handed over falls short"""
    from dpdist_amd import lib as L
    lib = L.load()
    C = pts.shape[0] if C is None else C
    N = pts.shape[1] if N is None else N
    view, band = M.banded_flat(max(C, 1) * max(N, 1) * 3, device=pts.device)
    ws_bytes = lib.dpd_mfv3d_bwd_workspace_bytes(max(C, 1), min(m, 11))
    ws, ws_band = M.banded_flat(ws_bytes // 4, device=pts.device)
    rc = lib.dpd_mfv3d_bwd_tiled(L.ptr(pts), L.ptr(dfv), C, N, m, float(sigma), tile, L.ptr(view), L.ptr(ws), ws_bytes - ws_short, L.cur_stream())
    torch.cuda.synchronize()

    def bands():
        band()
        ws_band()
    return rc, view.view(max(C, 1), max(N, 1), 3), bands, ws

"""Slot-summed backward of the per-point field, the part that needs no GPU: the numpy restatements of tests/field_slots_cases.py against
the autograd oracle (so that the references the GPU tests lean on are themselves shown right), the admission of the case beyond 8192
queries, the chunk order the accumulate chain relies on, the exported symbols, and every refusal of the new C entries (none of which
touches a device) and of the `backward` keyword.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from dpdist_amd import field
from dpdist_amd import lib as L

from . import field_cases as FC
from . import field_slots_cases as FS

E_NULL, E_DIM, E_UNSUPPORTED = -1, -2, -3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dpd_field_invert", "dpd_field_slot_sum", "dpd_field_scatter", "dpd_field_bwd")
KP = FC.KP


@pytest.mark.parametrize("tile", [None, 64])
@pytest.mark.parametrize("shared", [False, True])
def test_restatements_reproduce_the_autograd_oracle(shared, tile):
    """inverted index -> slot sum -> one product per slot -> scatter (whole clouds, and tiles of 64 queries accumulated in ascending
    order), composed in float64 with the g1 rows of the oracle: the gradients of FC.oracle_grads(torch.float64) to float64 rounding"""
    for name, got, ref in zip(("surfaces", "queries"), FS.restated_grads(shared, tile), FC.oracle_grads(torch.float64, shared)):
        err, top = np.abs(got - ref).max(), np.abs(ref).max()
        print("shared %s, tile %s: g %s restated vs autograd: %.3e at max |ref| %.3e" % (shared, tile, name, err, top))
        assert got.shape == ref.shape and top > 1e-2 and err <= 1e-10 * max(1.0, top), name


def test_inverted_index_restatement():
    """the restated index on the reference case: every row in exactly one list, lists contiguous and cloud-major, ids ascending in a slot"""
    vox = np.stack([FS.oracle_rows(torch.tensor(FC.surfaces()[0], dtype=torch.float64).requires_grad_(True),
                                   torch.tensor(FC.queries()[c], dtype=torch.float64), torch.zeros(FC.T_REF, 3, dtype=torch.float64))[0]
                    for c in range(3)])
    inv = FS.invert(vox)
    n, T, total = 3, FC.T_REF, inv["total"]
    assert inv["cap"] == 3 * 150 + 30 and total == inv["U"].sum() < inv["cap"]
    start = inv["slot_start"]
    assert start[0] == 0 and (np.diff(start[:total + 1]) >= 1).all() and (start[total:] == n * T).all()
    assert (inv["slot_vox"][total:] == -1).all() and (inv["slot_cloud"][total:] == -1).all()
    for g in range(total):
        c = inv["slot_cloud"][g]
        ids = inv["qlist"].reshape(-1)[start[g]:start[g + 1]]
        assert start[g] // T == c == (start[g + 1] - 1) // T and (np.diff(ids) > 0).all()
        assert (vox[c][ids] == inv["slot_vox"][g]).all() and (inv["uid"][c][ids] == g).all()
    assert sorted(inv["qlist"][1].tolist()) == list(range(T))


def test_admission_of_the_case_beyond_8192_queries():
    """float32 autograd oracle within ADMIT_GRAD * max(1, max |g64|) of float64 (the admission of tests/field_cases.py), so that the bars
    of the GPU test are the project's 2e-4 relative ones and not a multiple of a kink flip; masked queries occur; gradients with structure"""
    p64, gs64, gq64 = FS.big_oracle_grads(torch.float64)
    p32, gs32, gq32 = FS.big_oracle_grads(torch.float32)
    assert p64.shape == (1, FS.M_BIG, 3) and FS.M_BIG > field.MAX_BWD_QUERIES
    err = np.abs(p32 - p64).max()
    print("pred |f32 - f64| max %.3g" % err)
    assert err <= FC.FWD_BAR / 10      # (the maximum over 8193 rows: the oracle's own error must not use up the forward's bar)
    for name, g64, g32 in (("surface", gs64, gs32), ("queries", gq64, gq32)):
        err, top = np.abs(g32 - g64).max(), np.abs(g64).max()
        print("g %s |g32 - g64| max %.3g at max |g64| %.3g" % (name, err, top))
        assert err <= FC.ADMIT_GRAD * max(1.0, top) and top > 1e-2
    for ref, bar in FS.big_grad_bars():
        assert np.abs(ref).max() > 20 * bar
    assert not gq64[0, 8].any() and (gq64[0] == 0).all(-1).sum() > 100        # the masked queries have no gradient


def test_plan_is_cloud_outer_tile_inner():
    """what the accumulate chain of the slots backward relies on: the tiles of one cloud are consecutive and ascending, clouds ascending,
    and the last tile of a cloud ends at M"""
    for C, M, max_rows in ((3, 150, 64), (2, 20000, 16384), (1, 8193, 4096), (3, 150, 149)):
        plan = field.plan_chunks(C, M, max_rows)
        assert [(c0, t0) for c0, _, t0, _ in plan] == sorted((c0, t0) for c0, _, t0, _ in plan)
        assert all(n == 1 for _, n, _, _ in plan)
        per_cloud = -(-M // max_rows)
        for c in range(C):
            tiles = plan[c * per_cloud:(c + 1) * per_cloud]
            assert all(c0 == c for c0, _, _, _ in tiles) and tiles[0][2] == 0 and tiles[-1][2] + tiles[-1][3] == M
            assert all(a[2] + a[3] == b[2] for a, b in zip(tiles, tiles[1:]))
    assert field.plan_chunks(3, 150, 64)[:3] == [(0, 1, 0, 64), (0, 1, 64, 64), (0, 1, 128, 22)]
    for C, M, max_rows in ((3, 150, 4096), (3, 150, 150), (5, 150, 300)):      # whole clouds: every chunk starts at query 0 and ends at M
        assert all(t0 == 0 and T == M for _, _, t0, T in field.plan_chunks(C, M, max_rows))


def test_new_symbols_are_exported_and_declared():
    from dpdist_amd import build
    build.build(verbose=False)
    lib = L.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dpdist_capi.h")).read(), flags=re.S)
    for name in NEW:
        assert hasattr(lib, name) and name in L.SIGNATURES and re.search(r"\b%s\s*\(" % name, header), name
    assert "field_bwd.hip" in build.SOURCES


def test_entries_refuse_bad_arguments_without_a_device():
    """every DPD_E_* path of the new entries, before anything is launched: the pointers are never dereferenced"""
    lib = L.load()
    p = ctypes.c_void_p(1 << 30)
    cp = L.DecoderParams(*([1 << 30] * 11))
    inv = lambda vox=p, out=p, n=3, T=150, m=8, cap=480: lib.dpd_field_invert(vox, p, p, n, T, m, cap, p, p, p, out, None)   # noqa: E731
    assert inv(vox=None) == E_NULL and inv(out=None) == E_NULL
    assert inv(n=0) == E_DIM and inv(T=0) == E_DIM and inv(cap=0) == E_DIM and inv(cap=448) == E_DIM and inv(cap=512) == E_DIM
    assert inv(m=11) == E_UNSUPPORTED and inv(m=0) == E_UNSUPPORTED and inv(n=2, T=1 << 30, cap=1024) == E_UNSUPPORTED
    ssum = lambda g1=p, gs=p, dq=p, w=p, n=3, T=150, cap=480, h=256, k=5, m=8, kp=KP, stride=450: lib.dpd_field_slot_sum(   # noqa: E731
        g1, p, p, p, p, w, n, T, m, k, kp, h, cap, gs, dq, stride, None)
    assert ssum(g1=None) == E_NULL and ssum(gs=None, dq=None) == E_NULL and ssum(w=None) == E_NULL
    assert ssum(n=0) == E_DIM and ssum(T=-1) == E_DIM and ssum(cap=448) == E_DIM and ssum(stride=449) == E_DIM and ssum(h=0) == E_DIM
    for kw in (dict(h=200), dict(h=4160), dict(k=4), dict(k=9), dict(m=11), dict(kp=KP + 32)):
        assert ssum(**kw) == E_UNSUPPORTED, kw
    scat = lambda dXs=p, dfv=p, n=3, T=150, k=5, m=8, kp=KP: lib.dpd_field_scatter(dXs, p, p, n, T, m, k, kp, 0, dfv, None)   # noqa: E731
    assert scat(dXs=None) == E_NULL and scat(dfv=None) == E_NULL and scat(n=0) == E_DIM and scat(T=0) == E_DIM
    assert scat(k=4) == E_UNSUPPORTED and scat(m=11) == E_UNSUPPORTED and scat(kp=KP - 32) == E_UNSUPPORTED
    # dXs [slot_cap, KP] beyond the GEMMs' 32-bit byte offsets: 830 clouds x 512 slots x 2528 floats; 829 fit (the forward takes both)
    assert lib.dpd_field_slot_capacity(830, 600, 8) == 830 * 512
    assert scat(n=830, T=600) == E_UNSUPPORTED and ssum(n=830, T=600, cap=830 * 512, h=64, stride=1800) == E_UNSUPPORTED

    def bwd(dpred=p, dfv=p, gq=p, gs=p, dq=p, ucount=p, params=cp, n=3, T=150, cap=480, h=256, k=5, m=8, stride=450):
        return lib.dpd_field_bwd(dpred, p, p, p, p, p, p, ucount, p, p, p, p, n, T, m, k, KP, h, cap, params, p, p, p, dq, gs, p, dfv, 0, gq, stride,
                                 None)
    assert bwd(dpred=None) == E_NULL and bwd(dfv=None, gq=None) == E_NULL and bwd(params=None) == E_NULL
    assert bwd(gs=None) == E_NULL and bwd(ucount=None) == E_NULL          # the surface route's buffers
    assert bwd(dq=None, stride=0) == E_NULL                               # a shared query set goes through dq
    assert bwd(params=L.DecoderParams(*([1 << 30] * 8 + [None] * 3))) == E_NULL      # the surface route needs the transposed W1p
    assert bwd(params=L.DecoderParams(*([None] * 11))) == E_NULL
    assert bwd(n=0) == E_DIM and bwd(T=0) == E_DIM and bwd(cap=448) == E_DIM and bwd(stride=449) == E_DIM and bwd(stride=-1) == E_DIM
    for kw in (dict(h=200), dict(h=4160), dict(k=4), dict(m=11), dict(n=830, T=600, cap=830 * 512, h=64, stride=1800),
               dict(n=1, T=1 << 22, cap=512, h=1024, stride=3 << 22)):      # the last: g1 [2^22, 1024] beyond the 32-bit byte offsets
        assert bwd(**kw) == E_UNSUPPORTED, kw


class _Params:
    """what _resolve and _prepare read of a DPDistParams, without a device"""
    flat, KP, H, k, compute_dtype = torch.zeros(1), FC.KP, FC.H_DEC, FC.K_WIN, "f32"


def test_backward_keyword():
    from dpdist_amd import DPDistField
    assert DPDistField(_Params()).backward == "rows" and DPDistField(_Params(), backward="slots").backward == "slots"
    for bad in ("nonsense", None, True, "Slots"):
        with pytest.raises(ValueError, match="backward"):
            DPDistField(_Params(), backward=bad)
    S, Q = torch.tensor(FC.surfaces()), torch.tensor(FC.queries()).requires_grad_(True)
    with pytest.raises(ValueError, match="GPU"):             # the checks of the forward come first, in both modes
        DPDistField(_Params(), backward="slots")(S, Q)

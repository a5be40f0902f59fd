"""Host side of the live-row descriptor (dpd_live_rows): the carve-up, its refusals and the entries' argument checks.  No GPU calls."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def lib():
    from dpdist_amd import build, lib as L
    build.build(verbose=False)
    return L.load()


def test_carve_lays_the_members_out_in_order_without_overlap(lib):
    from dpdist_amd import lib as L
    Qb, KP, H = 256, 2528, 1024
    n = lib.dpd_live_rows_bytes(Qb, KP, H)
    assert n % 256 == 0 and n >= 4 * (4 + 3 * Qb + 3 * Qb * H + Qb * KP)
    base = 1 << 20        # (host pointer arithmetic only: nothing is dereferenced)
    lv = L.LiveRows()
    assert lib.dpd_live_rows_carve(ctypes.c_void_p(base), n, Qb, KP, H, lv) == 0
    assert (lv.Qb, lv.KP, lv.H) == (Qb, KP, H) and lv.X is None and lv.ssq is None
    sizes = [("cnt", 16), ("idx", 4 * Qb), ("pos", 4 * Qb), ("rowflag", 4 * Qb), ("g3c", 4 * Qb * H), ("h1c", 4 * Qb * H), ("h2c", 4 * Qb * H),
             ("Xc", 4 * Qb * KP)]
    end = base
    for name, size in sizes:
        p = getattr(lv, name)
        assert p % 256 == 0 and p >= end, name
        end = p + size
    assert end <= base + n


def test_carve_and_entries_refuse_what_they_do_not_take(lib):
    from dpdist_amd import lib as L
    lv = L.LiveRows()
    n = lib.dpd_live_rows_bytes(64, 64, 64)
    assert lib.dpd_live_rows_bytes(0, 64, 64) == 0
    assert lib.dpd_live_rows_carve(None, n, 64, 64, 64, lv) == -1
    assert lib.dpd_live_rows_carve(ctypes.c_void_p(1 << 20), n, 0, 64, 64, lv) == -2
    assert lib.dpd_live_rows_carve(ctypes.c_void_p((1 << 20) + 16), n, 64, 64, 64, lv) == -3      # alignment
    assert lib.dpd_live_rows_carve(ctypes.c_void_p(1 << 20), n, 48, 64, 64, lv) == -3             # whole 32-row tiles
    assert lib.dpd_live_rows_carve(ctypes.c_void_p(1 << 20), n - 1, 64, 64, 64, lv) == -4
    assert lib.dpd_live_rows_carve(ctypes.c_void_p(1 << 20), n, 64, 64, 64, lv) == 0
    one = ctypes.c_void_p(1 << 21)
    # weight gradients: a plane compute type, a bias gradient without the partial sums, rows other than the descriptor's
    assert lib.dpd_decoder_bwd_weights_live(1, None, 64, one, 64, 64, 64, 2, one, None, None, 0, None, None, lv, None) == -3
    assert lib.dpd_decoder_bwd_weights_live(1, None, 64, one, 64, 64, 64, 0, one, one, None, 0, None, None, lv, None) == -3
    assert lib.dpd_decoder_bwd_weights_live(1, None, 64, one, 96, 64, 64, 0, one, None, None, 0, None, None, lv, None) == -2
    assert lib.dpd_decoder_bwd_weights_live(4, None, 64, one, 64, 64, 64, 0, one, None, None, 0, None, None, lv, None) == -2
    assert lib.dpd_decoder_bwd_weights_pair_live(None, None, one, None, None, one, 64, 64, 64, 64, 0, None, 0, None, None, None, lv, None) == -1
    assert lib.dpd_decoder_bwd_weights_pair_live(None, one, one, None, None, one, 64, 64, 64, 64, 0, None, 0, None, one, None, lv, None) == -3
    # plan entries of the live launches: the two 32-row wave tiles only
    assert lib.dpd_set_gemm_plan(9, 30, 1) < 0 and lib.dpd_set_gemm_plan(11, 32, 1) == 0 and lib.dpd_set_gemm_plan(11, 33, 1) == 0
    assert lib.dpd_prof_enabled() == 0

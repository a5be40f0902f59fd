"""The encoder over tiles of points, what can be said without a GPU: the new entries are declared and exported, dpd_mfv3d_fits states the
plain entries' LDS caps as tests/mfv_cases.py restates them, the library's default tile is a multiple of 8 that fits 64 KiB, the tiled
entries refuse bad sizes and tiles on the host, and every case of tests/mfv_tiled_cases.py passes the admission of tests/mfv_cases.py
(float32 oracle within 3e-6 of float64, no sign change below 1e-6), with the float32 oracle as a stand-in passing the checkers."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from . import mfv_cases as M
from . import mfv_tiled_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dpd_mfv3d_fits", "dpd_mfv3d_fwd_tiled", "dpd_mfv3d_bwd_tiled")


@pytest.fixture(scope="module")
def lib():
    from dpdist_amd import build, lib as L
    build.build(verbose=False)
    return L.load()


def _id(case):
    return "%s-C%d-N%d-m%d-s%g" % case


def test_new_entries_are_declared_and_exported(lib):
    from dpdist_amd import lib as L
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dpdist_capi.h")).read(), flags=re.S)
    for n in NEW + ("dpd_mfv3d_tile",):
        assert re.search(r"\b%s\s*\(" % n, txt), "%s is not declared in include/dpdist_capi.h" % n
        assert hasattr(lib, n) and n in L.SIGNATURES, n


def test_fits_states_the_plain_caps(lib):
    """the table of the header's comments: forward from its formula (tests/mfv_cases.fwd_lds_bytes against LDS_CAP), backward from the
    host's bwd_lds_bytes / bwd_sliced_lds_bytes as restated there: one launch 400 N + 2736 <= 163840 <=> N <= 402; sliced
    400 n + 16 <= 163840 <=> n = ceil(N / 4) <= 409 <=> N <= 1636 (m = 8)"""
    FWD, ONE, SLICED = 0, 1, 2
    table = ((FWD, 8, 705, 706), (FWD, 8, 704, 712), (FWD, 10, 538, 539), (ONE, 8, 402, 403), (SLICED, 8, 1636, 1637))
    for which, m, fits, refused in table:
        assert lib.dpd_mfv3d_fits(fits, m, which) == 1 and lib.dpd_mfv3d_fits(refused, m, which) == 0, (which, m, fits, refused)
    assert M.bwd_lds_bytes(402, 8) <= M.LDS_CAP < M.bwd_lds_bytes(403, 8)
    assert M.bwd_sliced_lds_bytes(1636, 8)[1] <= M.LDS_CAP < M.bwd_sliced_lds_bytes(1637, 8)[1]
    for m in range(1, 11):          # every boundary, from the restated formulas
        for N in (1, 7, 8, 9, 64, 400, 402, 403, 536, 538, 539, 704, 705, 706, 712, 1636, 1637, 2048, 3397, 3398, 4096):
            assert lib.dpd_mfv3d_fits(N, m, FWD) == int(M.fwd_lds_bytes(N, m) <= M.LDS_CAP), (N, m)
            one = m <= 8 and M.bwd_lds_bytes(N, m) <= M.LDS_CAP
            sliced = m <= 8 and (M.bwd_sliced_lds_bytes(N, m)[1] <= M.LDS_CAP if M.takes_sliced(N) else one)
            assert lib.dpd_mfv3d_fits(N, m, ONE) == int(one) and lib.dpd_mfv3d_fits(N, m, SLICED) == int(sliced), (N, m)
    # sizes no entry takes, and a `which` there is none of
    for N, m, which in ((0, 8, 0), (4097, 8, 0), (64, 0, 0), (64, 11, 0), (64, 9, 1), (64, 9, 2), (64, 8, 3), (64, 8, -1)):
        assert lib.dpd_mfv3d_fits(N, m, which) == 0, (N, m, which)


def test_default_tile_is_a_multiple_of_8_that_fits(lib):
    for m in range(1, 11):
        t = lib.dpd_mfv3d_tile(m, 0)
        assert t >= 8 and t % 8 == 0 and T.fwd_tiled_lds_bytes(t, m) <= M.LDS_OPT_IN < T.fwd_tiled_lds_bytes(t + 8, m), (m, t)
        tb = lib.dpd_mfv3d_tile(m, 1)
        if m <= 8:
            assert tb >= 8 and tb % 8 == 0 and T.bwd_tiled_lds_bytes(tb, m) <= M.LDS_OPT_IN < T.bwd_tiled_lds_bytes(tb + 8, m), (m, tb)
        else:
            assert tb == 0
    assert (lib.dpd_mfv3d_tile(8, 0), lib.dpd_mfv3d_tile(10, 0), lib.dpd_mfv3d_tile(8, 1)) == (248, 168, 160)
    assert lib.dpd_mfv3d_tile(0, 0) == 0 and lib.dpd_mfv3d_tile(11, 0) == 0


def test_tiled_entries_refuse_on_the_host(lib):
    """argument checks come before any HIP call: the pointers below are host memory that a launch would fault on, and nothing touches them"""
    buf = (ctypes.c_float * 64)(*([7.0] * 64))
    p = ctypes.cast(buf, ctypes.c_void_p)
    ws_ok = 1 << 30
    for N, m, sigma, tile, C, want in ((0, 8, 0.125, 0, 1, T.E_UNSUPPORTED), (4097, 8, 0.125, 0, 1, T.E_UNSUPPORTED),
                                       (64, 8, 0.125, 12, 1, T.E_UNSUPPORTED), (64, 8, 0.125, 4, 1, T.E_UNSUPPORTED),
                                       (64, 8, 0.125, -8, 1, T.E_UNSUPPORTED), (64, 11, 0.125, 0, 1, T.E_UNSUPPORTED),
                                       (64, 0, 0.125, 0, 1, T.E_UNSUPPORTED), (64, 8, 0.0, 0, 1, T.E_DIM),
                                       (64, 8, float("nan"), 0, 1, T.E_DIM), (64, 8, 0.125, 0, 0, T.E_DIM)):
        assert lib.dpd_mfv3d_fwd_tiled(p, C, N, m, sigma, tile, p, None) == want, ("forward", N, m, sigma, tile, C)
        assert lib.dpd_mfv3d_bwd_tiled(p, p, C, N, m, sigma, tile, p, p, ws_ok, None) == want, ("backward", N, m, sigma, tile, C)
    # a tile whose tables do not fit 160 KiB (forward 4 (54 t + 2692) at m = 8: t <= 704; backward 400 t + 16: t <= 408)
    assert T.fwd_tiled_lds_bytes(704, 8) <= M.LDS_CAP < T.fwd_tiled_lds_bytes(712, 8)
    assert T.bwd_tiled_lds_bytes(408, 8) <= M.LDS_CAP < T.bwd_tiled_lds_bytes(416, 8)
    assert lib.dpd_mfv3d_fwd_tiled(p, 1, 64, 8, 0.125, 712, p, None) == T.E_UNSUPPORTED
    assert lib.dpd_mfv3d_bwd_tiled(p, p, 1, 64, 8, 0.125, 416, p, p, ws_ok, None) == T.E_UNSUPPORTED
    # the backward keeps one Gaussian per lane pair (m = 9: refused), and needs its workspace
    assert lib.dpd_mfv3d_bwd_tiled(p, p, 1, 64, 9, 0.125, 0, p, p, ws_ok, None) == T.E_UNSUPPORTED
    need = lib.dpd_mfv3d_bwd_workspace_bytes(2, 8)
    assert lib.dpd_mfv3d_bwd_tiled(p, p, 2, 64, 8, 0.125, 0, p, p, need - 1, None) == T.E_WORKSPACE
    assert lib.dpd_mfv3d_bwd_tiled(p, p, 2, 64, 8, 0.125, 0, p, None, need, None) == T.E_WORKSPACE
    assert lib.dpd_mfv3d_fwd_tiled(None, 1, 64, 8, 0.125, 0, p, None) == -1 and lib.dpd_mfv3d_bwd_tiled(p, None, 1, 64, 8, 0.125, 0, p, p, ws_ok, None) == -1
    assert list(buf) == [7.0] * 64


def test_python_routing_follows_fits(lib):
    from dpdist_amd import ops
    assert not ops.encoder_tiled(64, 8) and not ops.encoder_tiled(705, 8) and ops.encoder_tiled(706, 8) and ops.encoder_tiled(4096, 8)
    assert not ops.encoder_tiled(538, 10) and ops.encoder_tiled(539, 10)
    assert not ops.encoder_tiled(1636, 8, ops.FITS_BWD_SLICED) and ops.encoder_tiled(1637, 8, ops.FITS_BWD_SLICED)
    assert not ops.encoder_tiled(402, 8, ops.FITS_BWD_ONE) and ops.encoder_tiled(403, 8, ops.FITS_BWD_ONE)
    # sizes nothing takes stay with the plain entry, which states the refusal
    assert not ops.encoder_tiled(0, 8) and not ops.encoder_tiled(4097, 8) and not ops.encoder_tiled(64, 11) and not ops.encoder_tiled(64, 0)


def test_tie_clouds_put_every_copy_in_another_tile():
    for case in T.TIE_CASES:
        kind, _, N, m, _ = case
        idx, pos = T.tie_partner(kind, N), np.arange(N)
        copies = idx != pos
        assert copies.any() and np.array_equal(T.points(case)[:, idx], T.points(case))
        assert (idx[copies] // 8 != pos[copies] // 8).all()                         # forward: tiles of 8 points of the cloud
        ns = (N + M.SLICES - 1) // M.SLICES                                         # backward: tiles of 8 points of a slice of ns
        where = lambda i: (i // ns, (i % ns) // 8)                                  # noqa: E731
        assert all(where(a) != where(b) for a, b in zip(idx[copies], pos[copies]))
        if kind == "t3":                                                            # ... of the SAME slice
            assert (idx[copies] // ns == pos[copies] // ns).all()


@pytest.mark.parametrize("case", T.ALL_FWD, ids=_id)
def test_forward_case_is_admitted_and_the_standin_passes(case):
    ref = T.forward_ref(case)
    M.check_conditioning(ref, case)
    p = T.points(case)
    assert p.dtype == np.float32 and p.shape == case[1:3] + (3,) and np.abs(p).max() <= 0.8 + 1e-6
    assert ref.bar == max(3e-6, 4 * ref.d32) and ref.bar < 1.3e-5
    view, band = M.banded_flat(ref.fv64.size)
    view.copy_(torch.as_tensor(ref.fv32).reshape(-1))
    assert M.check_forward(view.view(ref.fv64.shape), band, ref, case[3], case) == ref.d32


@pytest.mark.parametrize("case", T.ALL_BWD, ids=_id)
def test_backward_case_is_admitted_and_the_standin_passes(case):
    ref = T.backward_ref(case)
    assert np.isfinite(ref.g64).all() and (ref.err32 <= ref.bar).all() and (np.abs(ref.g64).reshape(case[1], -1).max(1) > 0).all()
    assert (ref.dfv != 0).mean() > 0.5, "the upstream gradient is mostly masked"
    view, band = M.banded_flat(ref.g64.size)
    view.copy_(torch.as_tensor(ref.g32, dtype=torch.float32).reshape(-1))
    M.check_backward(view.view(ref.g64.shape), band, ref, case)
    if case[0][0] == "t":           # float64 autograd gives the copies of a point the same gradient
        idx = T.tie_partner(case[0], case[2])
        assert np.array_equal(ref.g64[:, idx], ref.g64)

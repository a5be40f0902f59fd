"""Differentiable all-pairs DPDist, the host side: argument checks of DPDistMatrix and of the new C entries (before any HIP call), the
workspace report of a backward chunk and Python's carve-up of it."""
import ctypes
import os
import re

import pytest
import torch

KP = 2528
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dpd_cross_bwd_workspace_bytes", "dpd_cross_invert", "dpd_decoder_fwd_cross_keep", "dpd_cross_slot_sum", "dpd_cross_scatter",
       "dpd_cross_bwd", "dpd_cross_carve")


@pytest.fixture(scope="module")
def lib():
    from dpdist_amd import build, lib as L
    build.build(verbose=False)
    return L.load()


def _params(**kw):
    from dpdist_amd.model import DPDistParams
    return DPDistParams(k=5, mlp=(64, 64, 64), device="cpu", **kw)


def test_module_is_exported_and_declared(lib):
    import dpdist_amd
    from dpdist_amd import lib as L, pairwise
    assert dpdist_amd.DPDistMatrix is pairwise.DPDistMatrix and issubclass(pairwise.DPDistMatrix, torch.nn.Module)
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dpdist_capi.h")).read(), flags=re.S)
    for name in NEW:
        assert hasattr(lib, name) and name in L.SIGNATURES and re.search(r"\b%s\s*\(" % name, header), name


def test_module_refuses_bad_arguments(lib):
    from dpdist_amd import DPDistMatrix
    a = torch.zeros(2, 64, 3)
    mod = DPDistMatrix(_params())
    assert mod.max_rows == 16384
    with pytest.raises(ValueError, match="same number of points"):
        mod(a, torch.zeros(3, 36, 3))
    with pytest.raises(ValueError, match="GPU"):
        mod(a, a)
    with pytest.raises(ValueError, match="GPU"):
        mod(a.clone().requires_grad_(True))
    with pytest.raises(ValueError, match=r"\[C, N, 3\]"):
        mod(torch.zeros(64, 3))
    with pytest.raises(ValueError, match="fp32"):
        DPDistMatrix(_params(compute_dtype="bf16"))
    with pytest.raises(ValueError, match="fp32"):
        DPDistMatrix(_params(compute_dtype="f32x3"))
    with pytest.raises(ValueError, match="perfect cube"):
        DPDistMatrix(_params(), Embedding_Size=500)
    with pytest.raises(ValueError, match="max_rows"):
        DPDistMatrix(_params(), max_rows=0)


def test_backward_workspace_report(lib):
    wb, fwd = lib.dpd_cross_bwd_workspace_bytes, lib.dpd_cross_workspace_bytes
    # what the forward refuses, the backward refuses
    assert wb(3, 2, 64, 8, 4, KP, 256) == 0 and wb(3, 2, 64, 11, 5, KP, 256) == 0
    assert wb(3, 2, 64, 8, 5, KP - 32, 256) == 0 and wb(3, 2, 64, 8, 5, KP, 200) == 0 and wb(0, 2, 64, 8, 5, KP, 256) == 0
    assert wb(3, 2, 64, 8, 5, KP, 4096) > 0 and wb(3, 2, 64, 8, 5, KP, 4160) == 0 and fwd(3, 2, 64, 8, 5, KP, 4160) > 0     # one wave per 256 columns
    sizes = [wb(c, 2, 64, 8, 5, KP, 256) for c in (1, 2, 3, 8)]
    assert sizes[0] > 0 and all(a < b for a, b in zip(sizes, sizes[1:]))
    # what the report is made of (every member rounded up to 256 bytes): (Ca, Cb, N) = (2, 3, 36) has pad rows
    al = lambda b: (b + 255) // 256 * 256      # noqa: E731
    rows_p, c, H = 224, 224, 256
    want = (al((KP - 32) * c * 4) + al(rows_p * 128) + 2 * al(rows_p * 4) + 256 + al(c * H * 4) + 3 * al(rows_p * H * 4) + 2 * al(rows_p * 12) +
            2 * al(rows_p * 12) + 2 * al(rows_p * H * 4) + al(rows_p * 12) + al(c * H * 4) + al(c * KP * 4) + al(2 * 512 * 20 * 4))
    assert wb(2, 3, 36, 8, 5, KP, H) == want
    # the default max_rows at the benchmark shape: five [16384, 1024] buffers of 64 MB
    assert wb(8, 32, 64, 8, 5, KP, 1024) >= 5 * 16384 * 1024 * 4 + 2 * 4096 * KP * 4


def test_python_layout_matches_the_report(lib):
    """dpdist_amd.pairwise has the library carve one allocation (dpd_cross_carve): every member at the running sum of the sizes that
    test_backward_workspace_report spells out, so two equal-sized members swapped on either side are caught"""
    from dpdist_amd import pairwise

    class _P:
        k, KP, H = 5, KP, 256

    ck = pairwise._Chunk(lib, 2, 3, 36, 8, _P, "cpu", backward=True)
    base = ck.arena.data_ptr()
    assert ck.cap == 224 and ck.ptr["Xu"] == base and all((v - base) % 256 == 0 for v in ck.ptr.values())
    order = ["Xu", "Xt", "uid", "maskr", "cnt", "Pu", "h1", "h2", "h3", "y", "pred", "dpred", "dy", "ga", "gb", "dq", "gs", "dXs", "dfv"]
    assert [n for n, _ in sorted(ck.ptr.items(), key=lambda kv: kv[1])] == order
    al = lambda b: (b + 255) // 256 * 256      # noqa: E731
    rows_p, c, H = 224, 224, 256
    act, row3 = al(rows_p * H * 4), al(rows_p * 12)
    sizes = [al((KP - 32) * c * 4), al(rows_p * 128), al(rows_p * 4), al(rows_p * 4), 256, al(c * H * 4), act, act, act, row3, row3,
             row3, row3, act, act, row3, al(c * H * 4), al(c * KP * 4), al(2 * 512 * 20 * 4)]
    off = 0
    for name, size in zip(order, sizes):
        assert ck.ptr[name] - base == off, name
        off += size
    assert off == ck.arena.numel() == lib.dpd_cross_bwd_workspace_bytes(2, 3, 36, 8, 5, KP, 256)
    assert ck.ptr["dfv"] + 2 * 512 * 20 * 4 <= base + ck.arena.numel()
    with pytest.raises(ValueError, match="not supported"):
        pairwise._Chunk(lib, 2, 3, 36, 11, _P, "cpu", backward=True)


def test_chunks_beyond_the_gemms_32_bit_offsets_are_refused(lib):
    """the slot product dXs [slots, KP] must stay below 4 GiB: 830 surface clouds x 512 slots x 2528 floats is beyond, 829 fit; the forward
    alone takes both.  Checked through the workspace report: nothing is allocated, nothing launched."""
    from dpdist_amd import pairwise
    wb, fwd = lib.dpd_cross_bwd_workspace_bytes, lib.dpd_cross_workspace_bytes
    assert fwd(830, 32, 64, 8, 5, KP, 64) > 0 and wb(830, 32, 64, 8, 5, KP, 64) == 0 and wb(829, 32, 64, 8, 5, KP, 64) > 0
    assert wb(512, 32, 64, 8, 5, KP, 1024) == 0 and wb(511, 32, 64, 8, 5, KP, 1024) > 0        # the activations, as in the forward

    class _P:
        k, KP, H = 5, KP, 64

    big = 1 << 30
    pairwise.check_chunks(lib, "dpd_cross_workspace_bytes", _P, 8, 830, 32, 64, big)
    with pytest.raises(ValueError, match="not supported"):
        pairwise.check_chunks(lib, "dpd_cross_bwd_workspace_bytes", _P, 8, 830, 32, 64, big)
    pairwise.check_chunks(lib, "dpd_cross_bwd_workspace_bytes", _P, 8, 830, 32, 64, 829 * 2048)     # 829 + 1 clouds: both chunks fit
    with pytest.raises(ValueError, match="not supported"):
        pairwise.check_chunks(lib, "dpd_cross_bwd_workspace_bytes", _P, 8, 830, None, 64, 1 << 40)  # a set against itself
    # the entries refuse the same chunk before any HIP call
    p = ctypes.c_void_p(1 << 30)
    from dpdist_amd import lib as L
    cp = L.DecoderParams(*([1 << 30] * 11))
    bwd = lambda ca, cap: lib.dpd_cross_bwd(p, p, p, p, p, p, p, p, p, p, ca, 32, 64, 8, 5, KP, 64, cap, cp, p, p, p, p, p, p, p, p, p, None)   # noqa: E731
    assert bwd(830, 830 * 512) == -3
    assert lib.dpd_cross_slot_sum(p, p, p, p, p, 830, 32, 64, 8, 5, KP, 64, 830 * 512, p, p, None) == -3
    assert lib.dpd_cross_scatter(p, p, p, 830, 32, 64, 8, 5, KP, p, None) == -3


def test_new_entries_refuse_before_any_hip_call(lib):
    p = ctypes.c_void_p(1 << 30)
    from dpdist_amd import lib as L
    cp = L.DecoderParams(*([1 << 30] * 11))
    assert lib.dpd_cross_invert(None, p, p, 2, 64, 8, p, p, p, None) == -1 and lib.dpd_cross_invert(p, p, p, 2, 64, 8, p, None, p, None) == -1
    assert lib.dpd_cross_invert(p, p, p, 2, 64, 11, p, p, p, None) == -3 and lib.dpd_cross_invert(p, p, p, 0, 64, 8, p, p, p, None) == -2
    keep = lambda h1=p, h2=ctypes.c_void_p(2 << 30), h3=ctypes.c_void_p(3 << 30), h=256, cap=384, ldu=384, params=cp: lib.dpd_decoder_fwd_cross_keep(   # noqa: E731
        p, ldu, cap, p, p, p, p, p, 6, 64, KP, h, params, h1, h2, h3, p, p, None, None)
    assert keep(h1=None) == -1 and keep(params=None) == -1 and keep(params=L.DecoderParams()) == -1
    assert keep(h2=p) == -2                                     # the three activations are kept: distinct buffers
    assert keep(h=200) == -3 and keep(cap=386, ldu=388) == -3 and keep(cap=384, ldu=256) == -2
    ssum = lambda gs=p, dq=p, w=p, cap=384, h=256, k=5, m=8: lib.dpd_cross_slot_sum(p, p, p, p, w, 3, 2, 64, m, k, KP, h, cap, gs, dq, None)   # noqa: E731
    assert ssum(gs=None, dq=None) == -1 and ssum(w=None) == -1 and ssum(cap=352) == -2
    assert ssum(h=200) == -3 and ssum(k=4) == -3 and ssum(m=11) == -3
    scat = lambda dfv=p, k=5, m=8: lib.dpd_cross_scatter(p, p, p, 3, 2, 64, m, k, KP, dfv, None)   # noqa: E731
    assert scat(dfv=None) == -1 and scat(k=4) == -3 and scat(m=11) == -3
    bwd = lambda dfv=p, gQ=p, gs=p, dq=p, params=cp, cap=384, h=256: lib.dpd_cross_bwd(   # noqa: E731
        p, p, p, p, p, p, p, p, p, p, 3, 2, 64, 8, 5, KP, h, cap, params, p, p, p, p, dq, gs, p, dfv, gQ, None)
    assert bwd(dfv=None, gQ=None) == -1 and bwd(gs=None) == -1 and bwd(dq=None) == -1 and bwd(params=None) == -1
    assert bwd(params=L.DecoderParams(*([1 << 30] * 8 + [None] * 3))) == -1      # the surface route needs the transposed W1p
    assert bwd(cap=352) == -2 and bwd(h=200) == -3

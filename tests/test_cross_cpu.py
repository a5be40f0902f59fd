"""All-pairs DPDist, the host side: argument checks of dpdist_matrix and of the C entries (before any HIP call), the workspace report."""
import ctypes

import pytest
import torch

KP = 2528


@pytest.fixture(scope="module")
def lib():
    from dpdist_amd import build, lib as L
    build.build(verbose=False)
    return L.load()


def _params(**kw):
    from dpdist_amd.model import DPDistParams
    return DPDistParams(k=5, mlp=(64, 64, 64), device="cpu", **kw)


def test_matrix_is_exported():
    import dpdist_amd
    from dpdist_amd import pairwise
    assert dpdist_amd.dpdist_matrix is pairwise.dpdist_matrix


def test_matrix_refuses_bad_arguments(lib):
    from dpdist_amd import dpdist_matrix
    a = torch.zeros(2, 64, 3)
    with pytest.raises(ValueError, match="same number of points"):
        dpdist_matrix(_params(), a, torch.zeros(3, 36, 3))
    with pytest.raises(ValueError, match="GPU"):
        dpdist_matrix(_params(), a, a)
    with pytest.raises(ValueError, match="GPU"):
        dpdist_matrix(_params(), a)
    with pytest.raises(ValueError, match=r"\[C, N, 3\]"):
        dpdist_matrix(_params(), torch.zeros(64, 3))
    with pytest.raises(ValueError, match="fp32"):
        dpdist_matrix(_params(compute_dtype="bf16"), a)
    with pytest.raises(ValueError, match="fp32"):
        dpdist_matrix(_params(compute_dtype="f32x3"), a)
    with pytest.raises(ValueError, match="perfect cube"):
        dpdist_matrix(_params(), a, Embedding_Size=500)


def test_chunks_hold_whole_clouds():
    from dpdist_amd.pairwise import chunk_clouds
    assert chunk_clouds(32, 2048, 16384) == 8
    assert chunk_clouds(3, 128, 1) == 1                  # at least one surface cloud
    assert chunk_clouds(3, 128, 1 << 20) == 3
    assert chunk_clouds(5, 108, 250) == 2


def test_cross_entries_refuse_before_any_hip_call(lib):
    """null pointers, an even window, a grid beyond 10 cells: DPD_E_NULL / DPD_E_UNSUPPORTED without touching a device"""
    p = ctypes.c_void_p(1 << 30)                          # any non-null "device address": nothing is dereferenced
    from dpdist_amd import lib as L
    cp = L.DecoderParams(*([1 << 30] * 8 + [None] * 3))
    assert lib.dpd_cross_index(None, 2, 64, 8, None, None, None, None, None) == -1
    assert lib.dpd_cross_index(p, 2, 64, 8, p, p, p, None, None) == -1
    assert lib.dpd_cross_index(p, 2, 64, 11, p, p, p, p, None) == -3
    assert lib.dpd_cross_index(p, 0, 64, 8, p, p, p, p, None) == -2
    gather = lambda k, m, kp, ldu=4096, xu=p: lib.dpd_cross_gather(p, p, p, p, p, p, None, 3, 2, 64, m, k, kp, xu, ldu, p, p, p, p, None)   # noqa: E731
    assert gather(5, 8, KP, xu=None) == -1
    assert lib.dpd_cross_gather(None, None, None, None, None, None, None, 3, 2, 64, 8, 5, KP, None, 4096, None, None, None, None, None) == -1
    assert gather(4, 8, KP) == -3 and gather(4, 8, lib.dpd_padded_width(4)) == -3
    assert gather(5, 11, KP) == -3
    assert gather(1, 8, lib.dpd_padded_width(1)) == -3    # k >= 3: the last 32 columns must hold everything that differs between rows
    assert gather(5, 8, KP - 32) == -3                    # KP == dpd_padded_width(k)
    assert gather(5, 8, KP, ldu=64) == -2                 # Xu narrower than the slot capacity
    dec = lambda xu=p, h=256, cap=384, ldu=384, params=cp: lib.dpd_decoder_fwd_cross(xu, ldu, cap, p, p, p, p, p, 6, 64, KP, h, params, p, p, p, p, p, None)   # noqa: E731
    assert dec(xu=None) == -1 and dec(params=None) == -1
    assert dec(params=L.DecoderParams()) == -1
    assert dec(h=200) == -3 and dec(cap=386, ldu=388) == -3
    assert dec(cap=384, ldu=256) == -2


def test_cross_workspace_report(lib):
    wb, cap = lib.dpd_cross_workspace_bytes, lib.dpd_cross_slot_capacity
    assert wb(3, 2, 64, 8, 4, KP, 256) == 0 and wb(3, 2, 64, 11, 5, KP, 256) == 0
    assert wb(3, 2, 64, 8, 5, KP - 32, 256) == 0 and wb(3, 2, 64, 8, 5, KP, 200) == 0 and wb(0, 2, 64, 8, 5, KP, 256) == 0
    assert cap(3, 2, 64, 8) == 384 and cap(2, 3, 36, 8) == 224 and cap(32, 32, 64, 8) == 32 * 512 and cap(3, 2, 64, 11) == 0
    sizes = [wb(c, 2, 64, 8, 5, KP, 256) for c in (1, 2, 3, 8)]
    assert sizes[0] > 0 and all(a < b for a, b in zip(sizes, sizes[1:]))
    # what the report is made of (every member rounded up to 256 bytes): (Ca, Cb, N) = (2, 3, 36) has pad rows
    al = lambda b: (b + 255) // 256 * 256      # noqa: E731
    rows_p, c, H = 224, 224, 256
    want = al((KP - 32) * c * 4) + al(rows_p * 128) + 2 * al(rows_p * 4) + 256 + al(c * H * 4) + 2 * al(rows_p * H * 4) + 2 * al(rows_p * 12) + al(6 * 4)
    assert wb(2, 3, 36, 8, 5, KP, H) == want
    # the benchmark shape in chunks of 16384 rows: two activation buffers of 64 MB at H = 1024
    assert wb(8, 32, 64, 8, 5, KP, 1024) >= 2 * 16384 * 1024 * 4 + (KP - 32) * 4096 * 4


def test_python_layout_matches_the_report(lib):
    """dpdist_amd.pairwise has the library carve one allocation (dpd_cross_carve): every member at the running sum of the sizes that
    test_cross_workspace_report spells out, so two equal-sized members swapped on either side are caught"""
    from dpdist_amd import pairwise

    class _P:
        k, KP, H = 5, KP, 256

    ck = pairwise._Chunk(lib, 2, 3, 36, 8, _P, "cpu", backward=False)
    base = ck.arena.data_ptr()
    assert ck.cap == 224 and ck.ptr["Xu"] == base and all((v - base) % 256 == 0 for v in ck.ptr.values())
    order = ["Xu", "Xt", "uid", "maskr", "cnt", "Pu", "act0", "act1", "y", "pred", "Dd"]
    assert [n for n, _ in sorted(ck.ptr.items(), key=lambda kv: kv[1])] == order
    al = lambda b: (b + 255) // 256 * 256      # noqa: E731
    rows_p, c, H = 224, 224, 256
    sizes = [al((KP - 32) * c * 4), al(rows_p * 128), al(rows_p * 4), al(rows_p * 4), 256, al(c * H * 4), al(rows_p * H * 4), al(rows_p * H * 4),
             al(rows_p * 12), al(rows_p * 12), al(6 * 4)]
    off = 0
    for name, size in zip(order, sizes):
        assert ck.ptr[name] - base == off, name
        off += size
    assert off == ck.arena.numel() == lib.dpd_cross_workspace_bytes(2, 3, 36, 8, 5, KP, 256)
    assert ck.Dd(6).numel() == 6 and ck.Dd(6).data_ptr() == ck.ptr["Dd"]
    with pytest.raises(ValueError, match="not supported"):
        pairwise._Chunk(lib, 2, 3, 36, 11, _P, "cpu")


SHAPES = [(2, 3, 36, 8, 5, KP, 256), (3, 2, 64, 8, 5, KP, 256), (1, 1, 1, 8, 5, KP, 64), (8, 32, 64, 8, 5, KP, 1024)]
FORWARD_ONLY, BACKWARD_ONLY = ("act0", "act1", "Dd"), ("h1", "h2", "h3", "dpred", "dy", "ga", "gb", "dq", "gs", "dXs", "dfv")
BASE = (1 << 30) + 16                                     # a fake, unaligned "device address": nothing is dereferenced


def _carve(lib, shape, backward, nbytes=None, base=BASE):
    from dpdist_amd import lib as L
    ck = L.CrossChunk()
    for n in L.CrossChunk.BUFFERS:                        # stale pointers: a refusal must leave none
        setattr(ck, n, 1 << 20)
    report = lib.dpd_cross_bwd_workspace_bytes if backward else lib.dpd_cross_workspace_bytes
    rc = lib.dpd_cross_carve(ctypes.c_void_p(base), report(*shape) if nbytes is None else nbytes, *shape, backward, ck)
    return rc, ck, {n: getattr(ck, n) for n in L.CrossChunk.BUFFERS if getattr(ck, n) is not None}


@pytest.mark.parametrize("backward", [0, 1])
@pytest.mark.parametrize("shape", SHAPES)
def test_carve_ends_at_the_report(lib, shape, backward):
    """both forms: offsets are multiples of 256 from an unaligned base, the members the form lacks are NULL, the last member's offset
    plus its padded size is the matching report, and the struct carries the shape, the slot capacity and rows_p"""
    Ca, Cb, N, m, k, kp, H = shape
    rc, ck, ptr = _carve(lib, shape, backward)
    assert rc == 0
    assert set(ptr) == set(ck.BUFFERS) - set(FORWARD_ONLY if backward else BACKWARD_ONLY)
    assert min(ptr.values()) == ptr["Xu"] == BASE and all((v - BASE) % 256 == 0 for v in ptr.values())
    report = (lib.dpd_cross_bwd_workspace_bytes if backward else lib.dpd_cross_workspace_bytes)(*shape)
    last, last_bytes = ("dfv", Ca * m ** 3 * 20 * 4) if backward else ("Dd", Ca * Cb * 4)
    assert max(ptr, key=ptr.get) == last and ptr[last] - BASE + (last_bytes + 255) // 256 * 256 == report == ck.bytes
    assert (ck.Ca_chunk, ck.Cb, ck.N, ck.m, ck.k, ck.KP, ck.H) == shape
    assert ck.slot_cap == lib.dpd_cross_slot_capacity(Ca, Cb, N, m) and ck.rows_p == (Ca * Cb * N + 31) // 32 * 32


REFUSED = [(3, 2, 64, 8, 4, KP, 256), (3, 2, 64, 11, 5, KP, 256), (3, 2, 64, 8, 5, KP - 32, 256), (3, 2, 64, 8, 5, KP, 200),
           (0, 2, 64, 8, 5, KP, 256), (512, 32, 64, 8, 5, KP, 1024), (841, 32, 64, 8, 5, KP, 64)]


@pytest.mark.parametrize("backward", [0, 1])
def test_carve_refuses_what_the_reports_refuse(lib, backward):
    """DPD_E_UNSUPPORTED exactly where the matching report returns 0, and no pointer left set; the neighbours that fit are carved"""
    report = lib.dpd_cross_bwd_workspace_bytes if backward else lib.dpd_cross_workspace_bytes
    refused = REFUSED + ([(830, 32, 64, 8, 5, KP, 64), (3, 2, 64, 8, 5, KP, 4160)] if backward else [])
    for shape in refused:
        assert report(*shape) == 0, shape
        rc, ck, ptr = _carve(lib, shape, backward, nbytes=1 << 62)
        assert rc == -3 and not ptr and ck.bytes == 0, shape
    fits = [(511, 32, 64, 8, 5, KP, 1024), (829 if backward else 840, 32, 64, 8, 5, KP, 64)]
    for shape in fits + ([] if backward else [(830, 32, 64, 8, 5, KP, 64), (3, 2, 64, 8, 5, KP, 4160)]):
        rc, ck, ptr = _carve(lib, shape, backward)
        assert rc == 0 and ck.bytes == report(*shape) > 0, shape
    if not backward:
        assert _carve(lib, (840, 32, 64, 8, 5, KP, 64), 1)[0] == -3      # the backward's limit is 829 clouds


@pytest.mark.parametrize("backward", [0, 1])
def test_carve_checks_its_arguments(lib, backward):
    from dpdist_amd import lib as L
    shape = SHAPES[0]
    report = (lib.dpd_cross_bwd_workspace_bytes if backward else lib.dpd_cross_workspace_bytes)(*shape)
    rc, ck, ptr = _carve(lib, shape, backward, nbytes=report - 1)
    assert rc == -4 and not ptr
    assert _carve(lib, shape, backward, nbytes=report)[0] == 0
    assert lib.dpd_cross_carve(None, report, *shape, backward, L.CrossChunk()) == -1
    assert lib.dpd_cross_carve(ctypes.c_void_p(BASE), report, *shape, backward, None) == -1


def test_shapes_beyond_the_gemms_32_bit_offsets_are_refused(lib):
    """the GEMM kernels address a matrix with 32-bit byte offsets: Xu [KP - 32, slots], Pu [slots, H] and the activations [rows, H] must
    each stay below 4 GiB -- refused by the workspace report and by both entries, not computed wrongly"""
    wb = lib.dpd_cross_workspace_bytes
    p = ctypes.c_void_p(1 << 30)
    from dpdist_amd import lib as L
    cp = L.DecoderParams(*([1 << 30] * 8 + [None] * 3))
    # activations: 512 surface clouds x 32 x 64 queries = 2^20 rows of 1024 floats = 4 GiB exactly; one cloud less fits
    assert wb(512, 32, 64, 8, 5, KP, 1024) == 0 and wb(511, 32, 64, 8, 5, KP, 1024) > 0
    # Xu: 2496 x (Ca * 512) floats; 4 GiB at 430 185 slots
    assert wb(841, 32, 64, 8, 5, KP, 64) == 0 and wb(840, 32, 64, 8, 5, KP, 64) > 0
    gather = lambda ca, ldu: lib.dpd_cross_gather(p, p, p, p, p, p, None, ca, 32, 64, 8, 5, KP, p, ldu, p, p, p, p, None)   # noqa: E731
    assert gather(841, 841 * 512) == -3
    assert gather(8, 430208) == -3                        # a row stride of Xu beyond the limit, whatever the chunk
    dec = lambda pairs, h, cap, ldu: lib.dpd_decoder_fwd_cross(p, ldu, cap, p, p, p, p, p, pairs, 64, KP, h, cp, p, p, p, p, p, None)   # noqa: E731
    assert dec(16384, 1024, 4096, 4096) == -3             # 2^20 rows x 1024
    assert dec(128, 1024, 1 << 20, 1 << 20) == -3         # Pu (and Xu) beyond 4 GiB
    assert dec(128, 64, 4096, 430208) == -3               # Xu's stride alone


def test_matrix_maps_refusals_to_value_errors(lib):
    from dpdist_amd import pairwise
    with pytest.raises(ValueError, match="refuses this shape"):
        pairwise._check(-3, "dpd_cross_gather")
    with pytest.raises(ValueError, match="refuses this shape"):
        pairwise._check(-2, "dpd_cross_index")
    with pytest.raises(RuntimeError):
        pairwise._check(-1, "dpd_cross_index")
    with pytest.raises(RuntimeError):
        pairwise._check(700, "dpd_cross_index")
    pairwise._check(0, "dpd_cross_index")

    class _M:                                             # what dpdist_matrix reads of a DPDistModel
        params_, Embedding_Size, sigma = _params(), 512, 0.125

    with pytest.raises(ValueError, match="contradicts"):
        pairwise._resolve(_M, 1000, None)
    with pytest.raises(ValueError, match="contradicts"):
        pairwise._resolve(_M, None, 0.25)
    assert pairwise._resolve(_M, 512, None)[1:] == (8, 0.125) and pairwise._resolve(_params(), None, None)[1:] == (8, 0.125)
    assert pairwise._resolve(_params(), 1000, 0.1)[1:] == (10, 0.1)

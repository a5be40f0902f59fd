"""Exact-integer, stride, split-K and guard-band tests of the GEMM building blocks (gemm_f32.hip, gemm_rs.h, gemm_x3.hip, gemm_p8.hip,
host dispatch in gemm_host.h) through the C entries dpd_gemm_f32, dpd_split_planes and dpd_gemm_planes.

Operands are small integers (tests/gemm_cases.py holds the builders, their exactness bounds and the case tables), so every result
must equal the int64 product bit for bit: every comparison here is torch.equal or an integer return code, there is no tolerance.
Every operand sits in a buffer wider than its logical width with NaN in the padding columns and in 256 guard rows before and
after (an operand element outside [M,K] / [K,N] that reaches the result poisons it); every output and every split-K workspace
starts filled with a NaN of a known bit pattern and its guard band must keep its bits (a store outside C[0:M, 0:N] is seen, and
stays inside memory the test owns).

Forms that do not exist are not generated (gemm_cases.x3_has_form), nothing is skipped at run time:
  np = 3 on tile 13 (a three-plane BK = 64 stage does not fit the LDS); np = 3 on tiles 21 / 23 and np = 1 on tile 24 (the
  phase-staggered tiles take one plane resp. three); the transpose-read TN form ("TNr") on tiles 4, 13, 21, 23, 24.
Tile 13 takes whole 64-deep K-tiles: its K is the table's K rounded up to a multiple of 64 (544 -> 576).
"""
import ctypes

import numpy as np
import pytest
import torch

from dpdist_amd import lib as L

from . import gemm_cases as G

pytestmark = pytest.mark.gpu

OK, E_NULL, E_DIM, E_UNSUPPORTED, E_WORKSPACE = 0, -1, -2, -3, -4


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible")
    L.load()     # raises if the HIP extension is missing -- never fall back
    return torch.device("cuda:0")


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _id(v):
    return "x".join(str(x) for x in v) if isinstance(v, tuple) else str(v)


# ------------------------------------------------------------------------------------------------ dpd_gemm_f32
class F32Operands:
    """A [M,K] and B [K,N] stored as `mode` wants them (NN: A [M,K], B [K,N]; NT: B as [N,K]; TN: A as [K,M]), row strides wider
    than the rows by pa / pb, NaN around"""

    def __init__(self, A, B, mode, pa, pb, dev):
        a = np.ascontiguousarray(A.T) if mode == "TN" else A
        b = np.ascontiguousarray(B.T) if mode == "NT" else B
        self.M, self.K, self.N = A.shape[0], A.shape[1], B.shape[1]
        self.ta, self.tb = int(mode == "TN"), int(mode == "NT")
        self.lda, self.ldb = a.shape[1] + pa, b.shape[1] + pb
        self.a, self.chk_a = G.put(a, self.lda, dev)
        self.b, self.chk_b = G.put(b, self.ldb, dev)

    def gemm(self, C, ldc, bias=None, gate=None, epilogue=0, split_k=1, tile=0, ws=None, ws_bytes=0):
        return L.load().dpd_gemm_f32(self.ta, self.tb, self.M, self.N, self.K, P(self.a), self.lda, P(self.b), self.ldb, P(C), ldc,
                                     P(bias), P(gate), epilogue, split_k, tile, P(ws), ws_bytes, L.cur_stream())

    def inputs_intact(self):
        self.chk_a()
        self.chk_b()


def _epilogue_operands(bias, gate, ldc, dev):
    """bias [N] (NaN after it) and the gate laid out with row stride ldc, as the entry reads it"""
    bias_v, chk_bias = G.put(bias[None, :], len(bias), dev)
    gate_v, chk_gate = G.put(gate, ldc, dev)
    return bias_v, gate_v, lambda: (chk_bias(), chk_gate())


@pytest.mark.parametrize("tile,mode,shape,pad", G.f32_cases(), ids=_id)
def test_gemm_f32_exact(dev, tile, mode, shape, pad):
    """every tile, mode and epilogue on ragged M, N, K and wide lda / ldb / ldc: equal to the int64 product, nothing written outside
    C[0:M, 0:N], nothing read from outside the operands.  K % 32 != 0, M < 4 and N = 4 send tiles 8, 9, 30-33 to tile 3."""
    M, N, K = shape
    A, B, bias, gate, ref = G.small_case(M, N, K)
    ops = F32Operands(A, B, mode, pad[0], pad[1], dev)
    ldc = N + pad[2]
    bias_v, gate_v, chk_epi = _epilogue_operands(bias, gate, ldc, dev)
    for epilogue in (0, 1, 2, 3):
        C, band = G.banded((M, N), ldc, device=dev)
        rc = ops.gemm(C, ldc, bias_v if epilogue in (1, 2) else None, gate_v if epilogue == 3 else None, epilogue, 1, tile)
        assert rc == OK, (epilogue, rc)
        G.check_exact(C, band, ref, epilogue, bias, gate)
    ops.inputs_intact()
    chk_epi()


@pytest.mark.parametrize("K,split", G.SPLITK_PAIRS, ids=_id)
@pytest.mark.parametrize("mode", G.F32_MODES)
@pytest.mark.parametrize("tile", G.F32_TILES)
def test_gemm_f32_split_k_exact(dev, tile, mode, K, split):
    """split-K into an uninitialised (NaN) workspace of exactly split_k * M * N floats: every slab is written whole, a slab whose K
    slice is empty is written as zeros, the epilogue is applied after the reduction, C keeps its stride"""
    M, N = G.SPLITK_MN
    A, B, bias, gate, ref = G.small_case(M, N, K)
    ops = F32Operands(A, B, mode, 4, 12, dev)
    ldc = N + 36
    bias_v, gate_v, chk_epi = _epilogue_operands(bias, gate, ldc, dev)
    chunk = G.splitk_chunk(K, split)
    for epilogue in G.SPLITK_EPILOGUES:
        C, band = G.banded((M, N), ldc, device=dev)
        ws, ws_band = G.banded_flat(split * M * N, device=dev)
        rc = ops.gemm(C, ldc, bias_v if epilogue == 2 else None, gate_v if epilogue == 3 else None, epilogue, split, tile, ws, 4 * ws.numel())
        assert rc == OK, (epilogue, rc)
        G.check_exact(C, band, ref, epilogue, bias, gate)
        ws_band()
        slabs = ws.view(split, M, N).cpu()
        for z in range(split):
            lo, hi = min(K, z * chunk), min(K, (z + 1) * chunk)
            want = G.product(A[:, lo:hi], B[lo:hi]).float() if hi > lo else torch.zeros(M, N)
            assert torch.equal(slabs[z], want), ("slab", z, lo, hi)
    ops.inputs_intact()
    chk_epi()


@pytest.mark.parametrize("tile", G.F32_TILES)
def test_gemm_f32_split_k_workspace_one_byte_short(dev, tile):
    M, N, K, split = 132, 68, 96, 2
    A, B, _, _, ref = G.small_case(M, N, K)
    ops = F32Operands(A, B, "NN", 4, 12, dev)
    C, band = G.banded((M, N), N + 36, device=dev)
    ws, ws_band = G.banded_flat(split * M * N, device=dev)
    assert ops.gemm(C, N + 36, split_k=split, tile=tile, ws=ws, ws_bytes=4 * ws.numel() - 1) == E_WORKSPACE
    assert ops.gemm(C, N + 36, split_k=split, tile=tile, ws=None, ws_bytes=4 * ws.numel()) == E_WORKSPACE
    torch.cuda.synchronize()
    assert G.untouched(C) and G.untouched(ws)
    band()
    ws_band()
    assert ops.gemm(C, N + 36, split_k=split, tile=tile, ws=ws, ws_bytes=4 * ws.numel()) == OK
    G.check_exact(C, band, ref)
    ws_band()


@pytest.mark.parametrize("tile,mode,shape,applies", G.TAIL_CASES, ids=_id)
def test_gemm_f32_tail_split_exact(dev, tile, mode, shape, applies):
    """split_k = 0 on the register-streamed tiles with ws >= 3 M N floats and no epilogue: where the tail split applies (more
    workgroup tiles than CUs, a last round less than 3/4 full, K pieces of at least 256) the tiles of the last tile row are cut
    along K into slabs in ws; where it does not, the call is silently a plain launch and ws stays untouched.  Exact either way."""
    M, N, K = shape
    plan = G.tail_split_plan(tile, M, N, K, torch.cuda.get_device_properties(dev).multi_processor_count)
    assert (plan is not None) == applies, "the table assumes the 256 CUs the kernel plans for"
    A, B, _, _, ref = G.small_case(M, N, K)
    ops = F32Operands(A, B, mode, 4, 12, dev)
    ldc = N + 36
    C, band = G.banded((M, N), ldc, device=dev)
    ws, ws_band = G.banded_flat(3 * M * N, device=dev)
    assert ops.gemm(C, ldc, split_k=0, tile=tile, ws=ws, ws_bytes=4 * ws.numel()) == OK
    G.check_exact(C, band, ref)
    ws_band()
    ops.inputs_intact()
    slabs = ws.view(3, M, N)
    if applies:
        row0, pieces = plan
        assert G.untouched(slabs[:, :row0]), "slab rows of whole-K tiles were written"
        assert not G.untouched(slabs[:pieces - 1, row0:]) and bool(torch.isfinite(slabs[:pieces - 1, row0:]).all())
        assert G.untouched(slabs[pieces - 1:])
        # one float less of workspace: not a tail split any more, and still right
        C2, band2 = G.banded((M, N), ldc, device=dev)
        ws2, ws2_band = G.banded_flat(3 * M * N, device=dev)
        assert ops.gemm(C2, ldc, split_k=0, tile=tile, ws=ws2, ws_bytes=4 * ws2.numel() - 4) == OK
        G.check_exact(C2, band2, ref)
        assert G.untouched(ws2)
        ws2_band()
    else:
        assert G.untouched(ws)


@pytest.mark.parametrize("swap", [False, True], ids=["wideA", "wideB"])
@pytest.mark.parametrize("mode", G.F32_MODES)
@pytest.mark.parametrize("tile", G.F32_TILES)
def test_gemm_f32_keeps_the_whole_mantissa(dev, tile, mode, swap):
    """a 12-bit operand against {-1, 0, 1}: an operand rounded to bf16 (8 bits) or a reduced-precision MFMA is off by integers"""
    M, N, K = G.MANTISSA_SHAPE
    A, B, ref = G.mantissa_case(M, N, K, swap)
    ops = F32Operands(A, B, mode, 4, 12, dev)
    C, band = G.banded((M, N), N + 36, device=dev)
    assert ops.gemm(C, N + 36, tile=tile) == OK
    G.check_exact(C, band, ref)
    ops.inputs_intact()


REFUSALS = {
    # name: (overrides of the base call, expected code)
    "K%4": (dict(K=6), E_UNSUPPORTED),
    "N%4": (dict(N=6), E_UNSUPPORTED),
    "lda%4": (dict(lda=18), E_UNSUPPORTED),
    "ldb%4": (dict(ldb=18), E_UNSUPPORTED),
    "ldc%4": (dict(ldc=18), E_UNSUPPORTED),
    "TN_M%4": (dict(ta=1, M=6), E_UNSUPPORTED),
    "transA_and_transB": (dict(ta=1, tb=1), E_UNSUPPORTED),
    "epilogue1_no_bias": (dict(epilogue=1, bias=False), E_NULL),
    "epilogue2_no_bias": (dict(epilogue=2, bias=False), E_NULL),
    "epilogue3_no_gate": (dict(epilogue=3, gate=False), E_NULL),
    "epilogue4": (dict(epilogue=4), E_UNSUPPORTED),
    "epilogue-1": (dict(epilogue=-1), E_UNSUPPORTED),
    "split_k-1": (dict(split_k=-1), E_DIM),
    "tile7": (dict(tile=7), E_UNSUPPORTED),
    "tile7_split2": (dict(tile=7, split_k=2), E_UNSUPPORTED),
    "tile29": (dict(tile=29), E_UNSUPPORTED),
    "tile34": (dict(tile=34), E_UNSUPPORTED),
    "M0": (dict(M=0), E_DIM),
    "A_null": (dict(a=False), E_NULL),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_gemm_f32_refusals(dev, name):
    """every documented refusal returns its code before anything is launched: C, its band and the workspace keep their bits"""
    over, code = REFUSALS[name]
    c = dict(ta=0, tb=0, M=8, N=8, K=8, lda=16, ldb=16, ldc=16, epilogue=0, split_k=1, tile=0, bias=True, gate=True, a=True)
    A, B, bias, gate, _ = G.small_case(16, 16, 16)
    a, _ = G.put(A, 16, dev)
    b, _ = G.put(B, 16, dev)
    bias_v, _ = G.put(bias[None, :], 16, dev)
    gate_v, _ = G.put(gate, 16, dev)
    C, band = G.banded((16, 16), 16, device=dev)
    ws, ws_band = G.banded_flat(2 * 16 * 16, device=dev)

    def call(c):
        return L.load().dpd_gemm_f32(c["ta"], c["tb"], c["M"], c["N"], c["K"], P(a) if c["a"] else None, c["lda"], P(b), c["ldb"], P(C),
                                     c["ldc"], P(bias_v) if c["bias"] else None, P(gate_v) if c["gate"] else None, c["epilogue"],
                                     c["split_k"], c["tile"], P(ws), 4 * ws.numel(), L.cur_stream())

    assert call(dict(c, **over)) == code
    torch.cuda.synchronize()
    assert G.untouched(C) and G.untouched(ws)
    band()
    ws_band()
    assert call(c) == OK            # the base call itself is fine: each refusal is due to its one override
    assert not G.untouched(C[:8, :8]) and G.untouched(C[8:]) and G.untouched(C[:, 8:])


# ------------------------------------------------------------------------------------------------ dpd_split_planes
def _bf16_bits(x):
    """bf16 bit patterns (int16) of integers that bf16 holds exactly"""
    t = torch.from_numpy(np.asarray(x, dtype=np.float32))
    assert torch.equal(t.bfloat16().float(), t)
    return (t.view(torch.int32) >> 16).to(torch.int16)


def _r8_as_rc(r8, R, C):
    """[np][R/8][C*8] (= [np][R/8][C][8]) -> [np][R][C]"""
    return r8.reshape(r8.shape[0], R // 8, C, 8).permute(0, 1, 3, 2).reshape(r8.shape[0], R, C)


def split_planes(src, R, C, ld, np_, dev, rc_pad=None, r8_extra=None, want_rc=True, want_r8=True):
    """dpd_split_planes of the fp32 view src into banded plane buffers: RC planes with row stride C + rc_pad and two spare rows
    between planes, R8 planes with r8_extra spare k-group rows between planes.  Returns dicts for rc / r8 (view, check, ld, plane)."""
    rc = r8 = None
    if want_rc:
        ld_rc = C + rc_pad
        v, chk = G.banded((R, C), ld_rc, G.NAN_OUT16, torch.int16, dev, planes=np_, plane_rows=R + 2)
        rc = dict(view=v, check=chk, ld=ld_rc, plane=(R + 2) * ld_rc)
    if want_r8:
        v, chk = G.banded((R // 8, C * 8), C * 8, G.NAN_OUT16, torch.int16, dev, planes=np_, plane_rows=R // 8 + r8_extra)
        r8 = dict(view=v, check=chk, ld=C, plane=(R // 8 + r8_extra) * C * 8)
    code = L.load().dpd_split_planes(P(src), R, C, ld, np_, P(rc["view"]) if rc else None, rc["ld"] if rc else 0, rc["plane"] if rc else 0,
                                     P(r8["view"]) if r8 else None, r8["plane"] if r8 else 0, L.cur_stream())
    assert code == OK, code
    return rc, r8


@pytest.mark.parametrize("shape", G.SPLIT_PLANES_SHAPES, ids=_id)
@pytest.mark.parametrize("np_", [1, 3])
def test_split_planes_exact(dev, np_, shape):
    """ld > C, ld_rc > C, plane strides larger than a plane: integers that bf16 holds land in the hi plane, the other planes are
    zero, RC and R8 agree element for element, nothing outside the planes is written and no padding of the source is read"""
    R, C = shape
    x = G.wide_int(np.random.default_rng([R, C]), (R, C), 9)
    src, chk_src = G.put(x, C + 12, dev)
    rc, r8 = split_planes(src, R, C, C + 12, np_, dev, rc_pad=24, r8_extra=3)
    got_rc, got_r8 = rc["view"].cpu(), _r8_as_rc(r8["view"].cpu(), R, C)
    assert torch.equal(got_rc[0], _bf16_bits(x))
    assert not got_rc[1:].any()
    assert torch.equal(got_r8, got_rc)
    rc["check"](), r8["check"](), chk_src()
    only_rc, _ = split_planes(src, R, C, C + 12, np_, dev, rc_pad=8, want_r8=False)
    _, only_r8 = split_planes(src, R, C, C + 12, np_, dev, r8_extra=0, want_rc=False)
    assert torch.equal(only_rc["view"].cpu(), got_rc) and torch.equal(_r8_as_rc(only_r8["view"].cpu(), R, C), got_rc)
    only_rc["check"](), only_r8["check"]()


# ------------------------------------------------------------------------------------------------ dpd_gemm_planes
class X3Operands:
    """the planes of A [M,K] and B [K,N] in the layouts of `fmt`, made by dpd_split_planes from NaN-padded fp32 sources.
    RC operands get a row stride wider than their rows by pa / pb with NaN (bf16) in the padding; R8 operands have no row stride
    (lda = M, ldb = N)."""

    def __init__(self, A, B, fmt, np_, pa, pb, dev):
        self.M, self.K, self.N = A.shape[0], A.shape[1], B.shape[1]
        self.np, (self.a_fmt, self.b_fmt) = np_, G.X3_FORMATS[fmt]
        a_store = A if self.a_fmt == 0 else np.ascontiguousarray(A.T)          # RC of [M,K] | R8 / RC of [K,M]
        b_store = np.ascontiguousarray(B.T) if self.b_fmt == 0 else B          # RC of [N,K] | R8 / RC of [K,N]
        self.a = self._planes(a_store, self.a_fmt != 1, pa, dev)
        self.b = self._planes(b_store, self.b_fmt != 1, pb, dev)

    def _planes(self, x, as_rc, pad, dev):
        R, C = x.shape
        src, chk = G.put(x, C + 4, dev)
        rc, r8 = split_planes(src, R, C, C + 4, self.np, dev, rc_pad=pad, r8_extra=1, want_rc=as_rc, want_r8=not as_rc)
        chk()
        return rc if as_rc else r8

    def gemm(self, C, ldc, bias=None, gate=None, epilogue=0, tile=0, out_rc=None, out_r8=None, r8_rows=0):
        a, b = self.a, self.b
        return L.load().dpd_gemm_planes(self.np, self.a_fmt, self.b_fmt, self.M, self.N, self.K, P(a["view"]), a["ld"], a["plane"],
                                        P(b["view"]), b["ld"], b["plane"], P(C), ldc, P(bias), P(gate), epilogue, tile, P(out_rc),
                                        P(out_r8), r8_rows, L.cur_stream())

    def inputs_intact(self):
        self.a["check"]()
        self.b["check"]()


@pytest.mark.parametrize("tile,np_,fmt,shape,pad", G.x3_cases(), ids=_id)
def test_gemm_planes_exact(dev, tile, np_, fmt, shape, pad):
    """one and three planes of small integers (exact in the hi plane) on every tile and format: equal to the int64 product with
    every epilogue, wide lda / ldb on RC operands, ldc > N, the gate with stride ldc"""
    M, N, K = shape
    A, B, bias, gate, ref = G.small_case(M, N, K)
    ops = X3Operands(A, B, fmt, np_, pad[0], pad[1], dev)
    ldc = N + pad[2]
    bias_v, gate_v, chk_epi = _epilogue_operands(bias, gate, ldc, dev)
    for epilogue in (0, 1, 2, 3):
        C, band = G.banded((M, N), ldc, device=dev)
        rc = ops.gemm(C, ldc, bias_v if epilogue in (1, 2) else None, gate_v if epilogue == 3 else None, epilogue, tile)
        assert rc == OK, (epilogue, rc)
        G.check_exact(C, band, ref, epilogue, bias, gate)
    ops.inputs_intact()
    chk_epi()


@pytest.mark.parametrize("tile,fmt,shape", G.x3_wide_cases(), ids=_id)
def test_gemm_planes_three_planes_wide_exact(dev, tile, fmt, shape):
    """two 10-bit operands: a value needs its hi and mid planes, so the product needs hi*hi, hi*mid, mid*hi and mid*mid right"""
    M, N, K = shape
    A, B, ref = G.wide_case(M, N, K)
    ops = X3Operands(A, B, fmt, 3, 8, 24, dev)
    C, band = G.banded((M, N), N + 12, device=dev)
    assert ops.gemm(C, N + 12, tile=tile) == OK
    G.check_exact(C, band, ref)
    ops.inputs_intact()


X3_OUT_CASES = [(tile, np_) for tile in G.X3_TILES for np_ in (1, 3) if G.x3_has_form(tile, np_, "NN")]


@pytest.mark.parametrize("tile,np_", X3_OUT_CASES, ids=_id)
def test_gemm_planes_plane_outputs_exact(dev, tile, np_):
    """out_rc / out_r8 with and without C: bit-identical to dpd_split_planes of the exact result (relu(A B + bias): integers up to
    11 bits, so hi and mid planes carry bits), rows >= r8_rows and everything past M untouched"""
    M, N, K, R8 = 200, 328, G.x3_k(tile, 96), 96
    A, B, bias, gate, ref = G.small_case(M, N, K)
    want = G.expected(ref, 2, bias)
    ops = X3Operands(A, B, "NN", np_, 8, 0, dev)
    bias_v, _, chk_epi = _epilogue_operands(bias, gate, N, dev)
    want_dev = want.to(dev)
    want_rc = torch.empty(np_, M, N, dtype=torch.int16, device=dev)
    want_r8 = torch.empty(np_, R8 // 8, N * 8, dtype=torch.int16, device=dev)
    assert L.load().dpd_split_planes(P(want_dev), M, N, N, np_, P(want_rc), N, M * N, None, 0, L.cur_stream()) == OK
    assert L.load().dpd_split_planes(P(want_dev), R8, N, N, np_, None, 0, 0, P(want_r8), R8 * N, L.cur_stream()) == OK
    assert torch.equal(_r8_as_rc(want_r8, R8, N), want_rc[:, :R8])           # the reference planes agree with each other
    for with_c in (True, False):
        C, band = G.banded((M, N), N + 12, device=dev)
        rc, rc_band = G.banded_flat(np_ * M * N, G.NAN_OUT16, torch.int16, dev)
        r8, r8_band = G.banded_flat(np_ * R8 * N, G.NAN_OUT16, torch.int16, dev)
        code = ops.gemm(C if with_c else None, N + 12, bias_v, None, 2, tile, rc, r8, R8)
        assert code == OK, (with_c, code)
        assert torch.equal(rc.view(np_, M, N), want_rc), with_c
        assert torch.equal(r8.view(np_, R8 // 8, N * 8), want_r8), with_c
        rc_band(), r8_band()
        if with_c:
            G.check_exact(C, band, ref, 2, bias)
        else:
            assert G.untouched(C)
            band()
    ops.inputs_intact()
    chk_epi()

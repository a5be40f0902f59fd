"""Exact-integer GEMM cases: operand builders with their exactness bounds, guard-banded buffers, the checker and the case tables
of tests/test_gemm_edges_gpu.py (tests/test_gemm_edges_cpu.py proves on the CPU that the checker has teeth and that every table
entry keeps its bound).  Not a test module and not a conftest.

The method: with small integer operands every partial sum of a dot product, in ANY order, with or without FMA, over any split of
K, is an integer of magnitude <= sum_k |a_k| |b_k|.  While that bound stays below 2^24 every such partial sum is exactly
representable in fp32, so an fp32 (or bf16-plane) GEMM must reproduce the int64 product bit for bit.  Each builder states the
closed-form bound of its value range and asserts it; `product` additionally asserts the bound on the operands it is given.
"""
import functools

import numpy as np
import torch

EXACT = 1 << 24            # integers of magnitude <= 2^24 are exact in fp32
BAND_ROWS = 256            # guard rows before and after a matrix: a whole 256-row tile written or read past an edge stays in the buffer
FLAT_BAND = 1 << 16        # guard elements on either side of a flat buffer (a 256 x 128 fp32 tile is 2^15 floats)
NAN_IN = 0x7FC00000        # input padding: a quiet NaN, so a padding element that reaches a result poisons it
NAN_OUT = 0x7FC0BEEF       # output / workspace fill: a NaN with a payload, so that "untouched" is a bit pattern, not a value
NAN_OUT16 = 0x7FC1         # the same for bf16 plane buffers


# ------------------------------------------------------------------------------------------------ operand builders
def small_int(rng, shape, K):
    """integers in [-4, 4].  Bound: |a b| <= 16, a bias in [-8, 8] on top: 16 K + 8 < 2^24 (K <= 1048575; the decoder's K is 2528)"""
    assert 16 * K + 8 < EXACT, ("small_int is not exact at this K", K)
    return rng.integers(-4, 5, size=shape).astype(np.int64)


def small_bias(rng, n):
    """integers in [-8, 8] (the + 8 of small_int's bound)"""
    return rng.integers(-8, 9, size=n).astype(np.int64)


def wide_int(rng, shape, bits):
    """integers with |x| < 2^(bits-1): `bits` significant bits including the sign"""
    assert 2 <= bits <= 24
    lim = 1 << (bits - 1)
    return rng.integers(-lim + 1, lim, size=shape).astype(np.int64)


def pm1(rng, shape):
    """values in {-1, 0, 1}"""
    return rng.integers(-1, 2, size=shape).astype(np.int64)


def gate_int(rng, shape):
    """gate values in [-2, 2]: negative, zero (closed: gate > 0 is false) and positive"""
    return rng.integers(-2, 3, size=shape).astype(np.int64)


def assert_wide_pm1(bits, K):
    """a `bits`-bit operand against pm1: |a b| < 2^(bits-1), so 2^(bits-1) K < 2^24 (12 bits: 2^11 K < 2^24, K < 8192)"""
    assert (1 << (bits - 1)) * K < EXACT, ("a %d-bit operand against pm1 is not exact at this K" % bits, K)


def assert_wide_wide(bits, K):
    """two `bits`-bit operands.  |a|, |b| <= 2^(bits-1) - 1, so K (2^(bits-1) - 1)^2 < 2^24; for 10 bits that is K <= 64 (the round
    figure 2^18 K < 2^24 stops one short of K = 64, which the value range still admits: 64 * 511^2 = 16 711 744 < 16 777 216).
    The bf16 planes of such a value (hi = 512, mid = -1 for 511) are bounded by `plane_bound` on the data itself."""
    assert K * ((1 << (bits - 1)) - 1) ** 2 < EXACT, ("two %d-bit operands are not exact at this K" % bits, K)


def bf16_planes(x):
    """hi, mid, lo bf16 planes of integer matrix x as float64 (round to nearest even, the hardware conversion)"""
    t = torch.from_numpy(np.asarray(x, dtype=np.float64)).float()
    hi = t.bfloat16().float()
    mid = (t - hi).bfloat16().float()
    lo = (t - hi - mid).bfloat16().float()
    return hi.double().numpy(), mid.double().numpy(), lo.double().numpy()


def plane_bound(A, B):
    """sum_k (|hi| + |mid| + |lo|)_A (|hi| + |mid| + |lo|)_B: bounds every partial sum of the plane products in any order"""
    a = sum(np.abs(p) for p in bf16_planes(A))
    b = sum(np.abs(p) for p in bf16_planes(B))
    return float((a @ b).max())


def product(A, B, planes=False):
    """int64 A @ B for integer A [M,K], B [K,N], with the exactness condition asserted on these operands: sum_k |a| |b| < 2^24
    (planes = True: on the bf16 planes of the operands).  Computed in float64, which is exact far beyond that bound."""
    A, B = np.asarray(A), np.asarray(B)
    assert A.dtype == np.int64 and B.dtype == np.int64 and A.shape[1] == B.shape[0]
    bound = plane_bound(A, B) if planes else float((np.abs(A).astype(np.float64) @ np.abs(B).astype(np.float64)).max())
    assert bound < EXACT, ("operands break the exactness bound", bound)
    p = A.astype(np.float64) @ B.astype(np.float64)
    return torch.from_numpy(np.rint(p).astype(np.int64))


# ------------------------------------------------------------------------------------------------ guard-banded buffers
_INT = {torch.float32: torch.int32, torch.int32: torch.int32, torch.int16: torch.int16}


class _Band:
    def __init__(self, raw, interior):
        self.raw, self.interior = raw, interior
        self.snap = self._masked()

    def _masked(self):
        now = self.raw.clone()
        self.interior(now).zero_()
        return now

    def __call__(self):
        now = self._masked()
        if not torch.equal(now, self.snap):
            bad = (now != self.snap).nonzero().flatten()
            raise AssertionError("guard band changed at %d raw elements, first at offset %d" % (bad.numel(), int(bad[0])))


def banded(shape, ld, fill=NAN_OUT, dtype=torch.float32, device="cpu", planes=None, plane_rows=None):
    """A [rows, cols] matrix of row stride ld (>= cols) inside a larger buffer filled with the bit pattern `fill`.
    Returns (view, check): view = the [rows, :cols] window (planes given: [planes, rows, :cols], plane stride plane_rows * ld);
    check() raises unless every element outside the window -- the ld - cols padding columns of every row, the rows between planes,
    and BAND_ROWS rows of ld elements before and after -- has the bits it had when the buffer was made."""
    rows, cols = shape
    plane_rows = rows if plane_rows is None else plane_rows
    assert ld >= cols and plane_rows >= rows
    it = _INT[dtype]
    flat2d = planes is None
    planes = 1 if flat2d else planes
    body = planes * plane_rows * ld
    guard = BAND_ROWS * ld
    if it == torch.int16:
        fill = fill - (1 << 16) if fill >= (1 << 15) else fill
    raw = torch.full((guard + body + guard,), fill, dtype=it, device=device)

    def window(r):
        w = r[guard:guard + body].view(planes, plane_rows, ld)[:, :rows, :cols]
        return w[0] if flat2d else w

    view = window(raw.view(dtype) if dtype != it else raw)
    return view, _Band(raw, window)


def banded_flat(n, fill=NAN_OUT, dtype=torch.float32, device="cpu"):
    """n contiguous elements between two guard bands of FLAT_BAND elements; returns (view, check)"""
    it = _INT[dtype]
    if it == torch.int16:
        fill = fill - (1 << 16) if fill >= (1 << 15) else fill
    raw = torch.full((FLAT_BAND + n + FLAT_BAND,), fill, dtype=it, device=device)

    def window(r):
        return r[FLAT_BAND:FLAT_BAND + n]

    view = window(raw.view(dtype) if dtype != it else raw)
    return view, _Band(raw, window)


def untouched(view, fill=NAN_OUT):
    """True when every element of a float32 / int16 view still has the fill pattern"""
    it = _INT[view.dtype]
    if it == torch.int16 and fill >= (1 << 15):
        fill -= 1 << 16
    return bool((view.contiguous().view(it) == fill).all())


def put(x, ld, device="cpu", fill=NAN_IN):
    """integer matrix x as a float32 operand of row stride ld, NaN around it; returns (view, check)"""
    x = np.asarray(x)
    view, check = banded(x.shape, ld, fill, torch.float32, device)
    view.copy_(torch.from_numpy(x.astype(np.float32)))
    return view, check


# ------------------------------------------------------------------------------------------------ the checker
def expected(ref_int64, epilogue=0, bias=None, gate=None):
    """epilogue (0 none, 1 + bias[n], 2 relu(+ bias[n]), 3 multiply by (gate[m,n] > 0)) of an int64 product, in float64 -> float32"""
    x = ref_int64.double()
    if epilogue in (1, 2):
        x = x + torch.as_tensor(bias).double()[None, :]
    if epilogue == 2:
        x = torch.clamp(x, min=0.0)
    if epilogue == 3:
        x = torch.where(torch.as_tensor(gate).double() > 0, x, torch.zeros_like(x))
    assert epilogue in (0, 1, 2, 3)
    assert float(x.abs().max()) <= EXACT
    return x.float()


def check_exact(C_view, band_check, ref_int64, epilogue=0, bias=None, gate=None):
    """C_view must equal the expected result bit for bit (as float32 values) and its guard band must be intact"""
    want = expected(ref_int64, epilogue, bias, gate)
    got = C_view.detach().cpu()
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(want.shape), (got.dtype, got.shape, want.shape)
    if not torch.equal(got, want):
        bad = ~(got == want)
        idx = bad.nonzero()
        r, c = int(idx[0, 0]), int(idx[0, 1])
        raise AssertionError("%d of %d elements differ; first at [%d, %d]: got %r, want %r; rows %s"
                             % (int(bad.sum()), bad.numel(), r, c, float(got[r, c]), float(want[r, c]),
                                sorted(set(idx[:, 0].tolist()))[:8]))
    band_check()


# ------------------------------------------------------------------------------------------------ case tables
F32_TILES = (0, 3, 8, 9, 30, 31, 32, 33)
F32_MODES = ("NN", "NT", "TN")
# extra leading dimension of (A, B, C): one contiguous case per tile and mode, every operand at +4, +12 and +36
F32_PADS = ((0, 0, 0), (4, 12, 36), (12, 36, 4), (36, 4, 12))
# (M, N, K): N = 4 and one K-step; ragged M, N, K below one tile; exact tiles; ragged above one 64-tile; two / one-and-a-half
# 128-tiles with K % 32 == 0; three / two 128-tiles with K % 32 != 0; the decoder's K
F32_SHAPES = ((4, 4, 4), (60, 68, 36), (64, 64, 32), (68, 60, 64), (132, 196, 96), (260, 132, 100), (132, 64, 2528))
# NN / NT only (TN needs M % 4 == 0): M below 4 (tile-3 fall-back), odd M, M one short of a tile
F32_SMALL_M = ((1, 8, 32), (1, 68, 36), (3, 8, 36), (3, 68, 32), (5, 8, 32), (5, 68, 36), (63, 8, 36), (63, 68, 32))


def f32_cases():
    """(tile, mode, (M, N, K), pad): every tile meets ragged M, N, K, every wide ld, a contiguous case and K = 2528 in every mode;
    each case runs epilogues 0-3"""
    out = []
    for tile in F32_TILES:
        for mi, mode in enumerate(F32_MODES):
            for si, shape in enumerate(F32_SHAPES):
                out.append((tile, mode, shape, F32_PADS[(si + mi) % 4]))
            if mode != "TN":
                for si, shape in enumerate(F32_SMALL_M):
                    out.append((tile, mode, shape, F32_PADS[(si + mi + 1) % 4]))
    return out


# (K, split_k): (32,2) and (64,3) leave the last 32-rounded slice empty, (36,3), (4,5), (100,7) have K % 32 != 0 -- all five send a
# DMA / register-streamed tile back to tile 3 and give tile 3 itself at least one slab that covers no K at all;
# (96,2), (2528,3), (2528,5) keep the whole-K-tile kernels
SPLITK_PAIRS = ((32, 2), (36, 3), (64, 3), (4, 5), (96, 2), (100, 7), (2528, 3), (2528, 5))
SPLITK_MN = (132, 68)
SPLITK_EPILOGUES = (0, 2, 3)


def splitk_chunk(K, split):
    """K range of one split-K slice as gemm_f32() plans it (whole 32-deep K-tiles)"""
    return ((K + split - 1) // split + 31) // 32 * 32


def splitk_has_empty_slice(K, split):
    return splitk_chunk(K, split) * (split - 1) >= K


RS_TILE_DIMS = {30: (128, 128), 31: (128, 64), 32: (64, 128), 33: (64, 64)}   # workgroup tiles of the register-streamed kernels


def tail_split_plan(tile, M, N, K, cus=256):
    """the tail split of gemm_rs.h: None when it does not apply, else (first_tail_row, pieces)"""
    bm, bn = RS_TILE_DIMS[tile]
    tm, tn = (M + bm - 1) // bm, (N + bn - 1) // bn
    T = tm * tn
    r = T % cus
    if not (T > cus and 0 < r < 192):
        return None
    pieces = min(4, (cus + r // 2) // r)
    first = ((T - r) // tn) * tn
    chunk = ((K // 32 + pieces - 1) // pieces) * 32
    if pieces >= 2 and first > 0 and chunk >= 256 and chunk * (pieces - 1) < K:
        return (first // tn) * bm, pieces
    return None


def tail_shape(tile, K=1024):
    """17 x 16 workgroup tiles (one round of 256 and a last round of 16), the last tile row and column ragged"""
    bm, bn = RS_TILE_DIMS[tile]
    return 16 * bm + 36, 16 * bn - 4, K


# (tile, mode, (M, N, K), applies)
TAIL_CASES = tuple([(t, "NN", tail_shape(t), True) for t in (30, 31, 32)] +
                   [(33, m, tail_shape(33), True) for m in F32_MODES] +
                   [(33, "NN", tail_shape(33, 512), False)] +                   # pieces of 128 < 256 deep: not worth a split
                   [(t, "NN", (260, 132, 512), False) for t in (30, 31, 32, 33)])   # fewer tiles than CUs

MANTISSA_SHAPE = (132, 68, 96)
MANTISSA_BITS = 12

X3_TILES = (1, 2, 3, 4, 5, 13, 21, 23, 24, 0)
X3_FORMATS = {"NN": (0, 1), "NT": (0, 0), "TN": (1, 1), "TNr": (2, 2)}
X3_SHAPES = ((200, 328, 32), (200, 328, 96), (72, 136, 160), (600, 328, 544), (8, 8, 32))
X3_PADS = ((8, 8, 4), (24, 40, 12), (40, 8, 36), (8, 24, 4))     # extra lda, ldb (multiples of 8: 16-byte chunks), ldc


def x3_has_form(tile, np_, fmt):
    """forms that exist: tile 13 and 21 / 23 one plane only, 24 three planes only; TNr on tiles 0 (= 1), 1, 2, 3, 5"""
    if tile == 13 and np_ != 1:
        return False
    if tile in (21, 23) and np_ != 1:
        return False
    if tile == 24 and np_ != 3:
        return False
    if fmt == "TNr" and tile not in (0, 1, 2, 3, 5):
        return False
    return True


def x3_k(tile, K):
    """tile 13 takes whole 64-deep K-tiles: its K is the next multiple of 64 (544 -> 576)"""
    return (K + 63) // 64 * 64 if tile == 13 else K


def x3_cases():
    """(tile, np, fmt, (M, N, K), pad) for every form that exists; each case runs epilogues 0-3"""
    out = []
    for tile in X3_TILES:
        for np_ in (1, 3):
            for fi, fmt in enumerate(X3_FORMATS):
                if not x3_has_form(tile, np_, fmt):
                    continue
                for si, (M, N, K) in enumerate(X3_SHAPES):
                    out.append((tile, np_, fmt, (M, N, x3_k(tile, K)), X3_PADS[(si + fi) % 4]))
    return out


def x3_wide_cases():
    """(tile, fmt, (M, N, K)): two 10-bit operands in three planes"""
    return [(tile, fmt, (72, 136, K)) for tile in X3_TILES for fmt in X3_FORMATS if x3_has_form(tile, 3, fmt) for K in (32, 64)]


X3_WIDE_BITS = 10
SPLIT_PLANES_SHAPES = ((8, 8), (64, 264), (72, 40))


@functools.lru_cache(maxsize=None)
def small_case(M, N, K, seed=0):
    """A [M,K], B [K,N], bias [N], gate [M,N] (int64 numpy) and the int64 product, shared by the tests that use the shape"""
    rng = np.random.default_rng([seed, M, N, K])
    A, B = small_int(rng, (M, K), K), small_int(rng, (K, N), K)
    for x in (A, B):
        x.setflags(write=False)
    return A, B, small_bias(rng, N), gate_int(rng, (M, N)), product(A, B)


@functools.lru_cache(maxsize=None)
def mantissa_case(M, N, K, swap, bits=MANTISSA_BITS):
    """a `bits`-bit operand against pm1 (swap: which of A, B is the wide one)"""
    assert_wide_pm1(bits, K)
    rng = np.random.default_rng([bits, M, N, K, int(swap)])
    wide_shape, one_shape = ((K, N), (M, K)) if swap else ((M, K), (K, N))
    W, P = wide_int(rng, wide_shape, bits), pm1(rng, one_shape)
    A, B = (P, W) if swap else (W, P)
    return A, B, product(A, B)


@functools.lru_cache(maxsize=None)
def wide_case(M, N, K, bits=X3_WIDE_BITS):
    """two `bits`-bit operands; the bound is asserted on their bf16 planes as well"""
    assert_wide_wide(bits, K)
    rng = np.random.default_rng([bits, M, N, K])
    A, B = wide_int(rng, (M, K), bits), wide_int(rng, (K, N), bits)
    return A, B, product(A, B, planes=True)

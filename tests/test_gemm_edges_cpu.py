"""The exact-integer GEMM checker of tests/gemm_cases.py has teeth: check_exact passes a float64 stand-in "kernel" that writes into
the guard-banded view, and raises for every corruption a GEMM kernel or its dispatch can commit without a tolerance test noticing.
Also: every shape of the GPU tables (tests/test_gemm_edges_gpu.py) keeps the exactness bound of its builder, and a case beyond a
bound fails in the builder.  Runs without a GPU."""
import numpy as np
import pytest
import torch

from . import gemm_cases as G

M, N, K = 60, 68, 36
LDA, LDB, LDC = K + 4, N + 12, N + 36


class Case:
    """operands, gate and output as the GPU tests lay them out: every matrix wider than its logical width, NaN around it"""

    def __init__(self):
        A, B, bias, gate, self.ref = G.small_case(M, N, K)
        self.A, self.chkA = G.put(A, LDA)
        self.B, self.chkB = G.put(B, LDB)
        self.gate, self.chk_gate = G.put(gate, LDC)
        self.bias = torch.from_numpy(bias)
        self.bias_f = self.bias.double()
        self.C, self.band = G.banded((M, N), LDC)

    def raw_offset(self, r, c):
        return G.BAND_ROWS * LDC + r * LDC + c

    def check(self, epilogue=0):
        G.check_exact(self.C, self.band, self.ref, epilogue, self.bias, self.gate)


def standin(c, epilogue=0, A=None, B=None, gate=None):
    """the reference "kernel": float64 matmul + epilogue, written into the banded view"""
    A = c.A if A is None else A
    B = c.B if B is None else B
    x = A.double() @ B.double()
    if epilogue in (1, 2):
        x = x + c.bias_f[None, :]
    if epilogue == 2:
        x = torch.relu(x)
    if epilogue == 3:
        g = c.gate if gate is None else gate
        x = torch.where(g > 0, x, torch.zeros_like(x))
    c.C.copy_(x.float())


@pytest.mark.parametrize("epilogue", [0, 1, 2, 3])
def test_standin_passes(epilogue):
    c = Case()
    assert c.C.stride() == (LDC, 1) and c.A.stride() == (LDA, 1) and G.untouched(c.C)
    standin(c, epilogue)
    c.check(epilogue)
    c.chkA(), c.chkB(), c.chk_gate()


def test_unwritten_output_raises():
    c = Case()
    with pytest.raises(AssertionError):
        c.check()


def test_one_element_off_by_one_raises():
    c = Case()
    standin(c)
    c.C[17, 5] += 1.0
    with pytest.raises(AssertionError, match=r"1 of 4080 elements differ; first at \[17, 5\]"):
        c.check()


@pytest.mark.parametrize("where", ["padding_column", "last_padding_column", "row_before", "row_after", "first_element", "last_element"])
def test_band_element_overwritten_raises(where):
    c = Case()
    standin(c)
    raw = c.band.raw
    off = {"padding_column": c.raw_offset(9, N), "last_padding_column": c.raw_offset(M - 1, LDC - 1),
           "row_before": c.raw_offset(-1, 3), "row_after": c.raw_offset(M, 0), "first_element": 0,
           "last_element": raw.numel() - 1}[where]
    raw[off] = 0                       # a stray store of 0.0f
    with pytest.raises(AssertionError, match="guard band changed at 1 raw elements, first at offset %d" % off):
        c.check()
    raw[off] = G.NAN_OUT
    c.check()
    raw.view(torch.float32)[off] = float("nan")        # a NaN of another bit pattern is a change too
    with pytest.raises(AssertionError, match="guard band"):
        c.check()


@pytest.mark.parametrize("row", [10, M - 1])
def test_row_written_one_too_low_raises(row):
    c = Case()
    standin(c)
    good = c.C[row].clone()
    c.band.raw.view(torch.float32)[c.raw_offset(row + 1, 0):c.raw_offset(row + 1, N)] = good
    c.band.raw[c.raw_offset(row, 0):c.raw_offset(row, N)] = G.NAN_OUT
    with pytest.raises(AssertionError):
        c.check()


def test_padding_column_of_an_operand_reaches_the_result():
    c = Case()
    A_wide = c.A.as_strided((M, K + 1), (LDA, 1))                  # one padding column of A ...
    B_wide = torch.cat([c.B, torch.ones(1, N)])                    # ... against a finite row
    standin(c, A=A_wide, B=B_wide)
    assert torch.isnan(c.C).all()
    with pytest.raises(AssertionError):
        c.check()
    c = Case()
    B_wide = c.B.as_strided((K, N + 1), (LDB, 1))[:, 1:]           # B's columns shifted by one: the last comes from the padding
    standin(c, B=B_wide)
    with pytest.raises(AssertionError):
        c.check()


def test_missing_k_tail_raises():
    c = Case()
    standin(c, A=c.A[:, :K - 4], B=c.B[:K - 4])
    with pytest.raises(AssertionError):
        c.check()


def test_split_k_sum_with_an_uninitialised_slab_raises():
    c = Case()
    ws, ws_band = G.banded_flat(3 * M * N)
    slabs = ws.view(3, M, N)
    slabs[0] = (c.A[:, :32].double() @ c.B[:32].double()).float()
    slabs[1] = (c.A[:, 32:].double() @ c.B[32:].double()).float()
    c.C.copy_(slabs[0] + slabs[1])                                 # the empty third slice left out: right
    c.check()
    ws_band()
    assert G.untouched(slabs[2]) and not G.untouched(slabs[1])
    c.C.copy_(slabs.sum(0))                                        # the third slab never written: NaN
    with pytest.raises(AssertionError):
        c.check()


def test_gate_read_with_stride_n_raises():
    c = Case()
    standin(c, 3)
    c.check(3)
    standin(c, 3, gate=c.gate.as_strided((M, N), (N, 1)))          # stride N where ldc was meant
    with pytest.raises(AssertionError):
        c.check(3)


def test_wrong_epilogue_raises():
    c = Case()
    standin(c, 1)
    with pytest.raises(AssertionError):
        c.check(2)


def test_banded_planes_and_flat():
    v, chk = G.banded((8, 16), 24, G.NAN_OUT16, torch.int16, planes=3, plane_rows=11)
    assert v.shape == (3, 8, 16) and v.stride() == (11 * 24, 24, 1) and G.untouched(v, G.NAN_OUT16)
    v.zero_()
    chk()
    base = G.BAND_ROWS * 24
    for off in (base + 16, base + 8 * 24, base + 11 * 24 - 1, base - 1, base + 3 * 11 * 24):   # padding, between planes, before, after
        chk.raw[off] = 0
        with pytest.raises(AssertionError):
            chk()
        chk.raw[off] = G.NAN_OUT16 - (1 << 16) if G.NAN_OUT16 >= (1 << 15) else G.NAN_OUT16
        chk()
    f, fchk = G.banded_flat(100)
    f.zero_()
    fchk()
    fchk.raw[G.FLAT_BAND + 100] = 0
    with pytest.raises(AssertionError):
        fchk()


# ------------------------------------------------------------------------------------------------ bounds
def test_builders_refuse_what_is_not_exact():
    rng = np.random.default_rng(0)
    with pytest.raises(AssertionError):
        G.small_int(rng, (4, 4), 1 << 20)              # 16 K + 8 = 2^24 + 8
    G.small_int(rng, (4, 4), (1 << 20) - 1)
    with pytest.raises(AssertionError):
        G.assert_wide_pm1(12, 8192)                    # 2^11 * 2^13 = 2^24
    G.assert_wide_pm1(12, 8191)
    with pytest.raises(AssertionError):
        G.assert_wide_wide(10, 65)
    G.assert_wide_wide(10, 64)
    big = np.full((2, 8), 2048, dtype=np.int64)
    with pytest.raises(AssertionError):
        G.product(big, big.T.copy())                   # 8 * 2^22 = 2^25
    with pytest.raises(AssertionError):
        G.mantissa_case(4, 4, 8192, False)
    with pytest.raises(AssertionError):
        G.wide_case(8, 8, 96)
    x = G.wide_int(rng, (64, 64), 10)
    assert np.abs(x).max() < 512 and np.abs(G.wide_int(rng, (64, 64), 12)).max() < 2048
    assert set(np.unique(G.pm1(rng, (64, 64)))) == {-1, 0, 1}
    assert np.abs(G.small_int(rng, (64, 64), 32)).max() == 4 and np.abs(G.small_bias(rng, 4096)).max() == 8
    hi, mid, lo = G.bf16_planes(np.array([[511, -3, 256, 0]]))
    assert hi.tolist() == [[512, -3, 256, 0]] and mid.tolist() == [[-1, 0, 0, 0]] and not lo.any()


def _small_enough(M_, N_, K_):
    return M_ * N_ * K_ <= 1e8


def test_every_gpu_case_keeps_its_bound():
    rng = np.random.default_rng(1)
    f32 = G.f32_cases()
    assert 200 <= len(f32) <= 400
    shapes = {s for _, _, s, _ in f32} | {(G.SPLITK_MN[0], G.SPLITK_MN[1], k) for k, _ in G.SPLITK_PAIRS} | {s for _, _, s, _ in G.TAIL_CASES}
    x3 = G.x3_cases()
    assert 200 <= len(x3) <= 400
    shapes |= {s for _, _, _, s, _ in x3}
    for (M_, N_, K_) in sorted(shapes):
        G.small_int(rng, (1, 1), K_)                   # the closed-form bound 16 K + 8 < 2^24
        if _small_enough(M_, N_, K_):
            ref = G.small_case(M_, N_, K_)[4]          # and the bound on the data (asserted in product)
            assert int(ref.abs().max()) + 8 < G.EXACT
    # every tile meets every kind of shape, every pad and the decoder's K
    for tile in G.F32_TILES:
        mine = [(m, s, p) for t, m, s, p in f32 if t == tile]
        assert {p for _, _, p in mine} == set(G.F32_PADS)
        for mode in G.F32_MODES:
            ss = [s for m, s, _ in mine if m == mode]
            assert any(s[2] == 2528 for s in ss) and any(s[2] % 32 for s in ss) and any(s[0] % 64 for s in ss) and any(s[1] % 64 for s in ss)
            assert (mode == "TN") or any(s[0] < 4 for s in ss)
    G.assert_wide_pm1(G.MANTISSA_BITS, G.MANTISSA_SHAPE[2])
    for swap in (False, True):
        G.mantissa_case(*G.MANTISSA_SHAPE, swap)
    for _, _, (M_, N_, K_) in G.x3_wide_cases():
        G.wide_case(M_, N_, K_)


def test_split_k_table_reaches_the_fallback_and_the_empty_slice():
    empty = {(k, s) for k, s in G.SPLITK_PAIRS if G.splitk_has_empty_slice(k, s)}
    assert empty == {(32, 2), (36, 3), (64, 3), (4, 5), (100, 7)}
    assert {(k, s) for k, s in G.SPLITK_PAIRS if k % 32} == {(36, 3), (4, 5), (100, 7)}
    for k, s in set(G.SPLITK_PAIRS) - empty:           # the pairs that stay on the whole-K-tile kernels: every slice whole K-tiles
        assert k % 32 == 0 and G.splitk_chunk(k, s) % 32 == 0


def test_tail_split_table_has_both_outcomes():
    for tile, _, (M_, N_, K_), applies in G.TAIL_CASES:
        plan = G.tail_split_plan(tile, M_, N_, K_)
        assert (plan is not None) == applies, (tile, M_, N_, K_, plan)
        if applies:
            row0, pieces = plan
            assert pieces == 4 and 0 < row0 < M_ and M_ % 4 == 0 and N_ % 4 == 0
    assert {t for t, _, _, a in G.TAIL_CASES if a} == {30, 31, 32, 33} == {t for t, _, _, a in G.TAIL_CASES if not a}

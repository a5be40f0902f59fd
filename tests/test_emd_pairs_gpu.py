"""Per-pair Earth Mover's distance on the GPU (dpd_emd_pairs_fwd / _bwd, dpdist_amd.emd: emd_pairs / EMDPairs) against the all-pairs entry
and EMDMatrix on each pair alone (bit for bit) and the float64 oracle composed in tests/baseline_pairs_cases.py (at 8 x the recorded
floors).  Outputs, gradients and the workspace of the C entries sit in NaN-payload guard bands, input padding holds a quiet NaN."""
import functools

import numpy as np
import pytest
import torch

from tests import baseline_cases as BC
from tests import baseline_pairs_cases as PC
from tests import gemm_cases as G

pytestmark = pytest.mark.gpu
DEV = "cuda"


def lib_():
    from dpdist_amd import build, lib as L
    build.build(verbose=False)
    return L.load()


@pytest.fixture(scope="module")
def lib():
    return lib_()


def bits(x):
    x = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    return np.ascontiguousarray(x, np.float32).view(np.int32)


def same(x, y):
    return np.array_equal(bits(x), bits(y))


def dev_set(X, counts, width=None, fill_bits=0x7FC00000):
    width = X.shape[1] if width is None else width
    return torch.from_numpy(BC.padded(X, counts, width, fill_bits)).to(DEV), torch.tensor(counts, dtype=torch.int32, device=DEV)


def entry(lib, A, cA, B, cB, W=None, form=0, wA=None, wB=None, counts=True, fill_bits=0x7FC00000, sides=(True, True), outs=(True, True)):
    """dpd_emd_pairs_fwd and, with W, dpd_emd_pairs_bwd into guard-banded outputs, gradients and workspace
    -> {"cost", "dist" [P], "dA", "dB"} as numpy (None when skipped); every band is checked"""
    from dpdist_amd import lib as L
    a, ac = dev_set(A, cA, wA, fill_bits)
    b, bc = dev_set(B, cB, wB, fill_bits)
    P, Wa, Wb = len(cA), a.shape[1], b.shape[1]
    pa, pb = (L.ptr(ac), L.ptr(bc)) if counts else (None, None)
    need = lib.dpd_emd_pairs_workspace_bytes(P, Wa, Wb)
    assert need == P * (3 * Wa + 2 * Wb) * 4
    ws, ck_ws = G.banded_flat(need // 4, device=DEV)
    (cost, ck_c), (dist, ck_d) = G.banded_flat(P, device=DEV), G.banded_flat(P, device=DEV)
    rc = lib.dpd_emd_pairs_fwd(L.ptr(a), pa, Wa, L.ptr(b), pb, Wb, P, form, L.ptr(cost) if outs[0] else None, L.ptr(dist) if outs[1] else None,
                               L.ptr(ws), need, L.cur_stream())
    assert rc == 0
    torch.cuda.synchronize()
    ck_ws(), ck_c(), ck_d()
    res = {"cost": cost.cpu().numpy().copy() if outs[0] else None, "dist": dist.cpu().numpy().copy() if outs[1] else None}
    for x, used in ((cost, outs[0]), (dist, outs[1])):
        assert used or G.untouched(x)
    if W is not None:
        w = torch.from_numpy(np.array(W, np.float32)).to(DEV)
        (da, ck_a), (db, ck_b) = G.banded_flat(a.numel(), device=DEV), G.banded_flat(b.numel(), device=DEV)
        rc = lib.dpd_emd_pairs_bwd(L.ptr(a), pa, Wa, L.ptr(b), pb, Wb, P, form, L.ptr(w), L.ptr(da) if sides[0] else None,
                                   L.ptr(db) if sides[1] else None, L.ptr(ws), need, L.cur_stream())
        assert rc == 0
        torch.cuda.synchronize()
        ck_ws(), ck_a(), ck_b()
        for x, used in ((da, sides[0]), (db, sides[1])):
            assert used or G.untouched(x)
        res["dA"] = da.cpu().view(a.shape).numpy().copy() if sides[0] else None
        res["dB"] = db.cpu().view(b.shape).numpy().copy() if sides[1] else None
    return res


@functools.lru_cache(maxsize=None)
def batch(name, form=0):
    """a case through the C entries under the case's W, computed once and shared"""
    A, B, cA, cB, W = PC.emd_make(name)
    return entry(lib_(), A, cA, B, cB, W, form)


@functools.lru_cache(maxsize=None)
def matrix_pair(name, b):
    """dpd_emd_matrix_fwd / _bwd on pair b alone (Ca = Cb = 1, the pair's counts, upstream W[b]) -> (cost, dist, dA [Wa,3], dB [Wb,3])"""
    from dpdist_amd import lib as L
    A, B, cA, cB, W = PC.emd_make(name)
    lib = lib_()
    a, ac = dev_set(A[b:b + 1], cA[b:b + 1])
    q, qc = dev_set(B[b:b + 1], cB[b:b + 1])
    out = torch.empty(2, device=DEV)
    assert lib.dpd_emd_matrix_fwd(L.ptr(a), L.ptr(ac), 1, a.shape[1], L.ptr(q), L.ptr(qc), 1, q.shape[1], L.ptr(out[0:]), L.ptr(out[1:]),
                                  L.cur_stream()) == 0
    need = lib.dpd_emd_matrix_workspace_bytes(1, a.shape[1], 1, q.shape[1])
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    w = torch.from_numpy(np.array(W[b:b + 1], np.float32)).to(DEV)
    da, dq = torch.empty_like(a), torch.empty_like(q)
    assert lib.dpd_emd_matrix_bwd(L.ptr(a), L.ptr(ac), 1, a.shape[1], L.ptr(q), L.ptr(qc), 1, q.shape[1], L.ptr(w), L.ptr(da), L.ptr(dq), 0,
                                  L.ptr(ws), need, L.cur_stream()) == 0
    o = out.cpu().numpy()
    return o[0], o[1], da.cpu().numpy()[0], dq.cpu().numpy()[0]


def assert_padding_is_plus_zero(g, counts):
    x = bits(g)
    for c, n in enumerate(counts):
        assert not x[c, n:].any(), c


@pytest.mark.parametrize("name", PC.EMD_CASES)
def test_values_and_gradients_are_the_matrix_entrys_on_the_pair_alone_bit_for_bit(lib, name):
    A, B, cA, cB, W = PC.emd_make(name)
    got = batch(name)
    for b in range(len(cA)):
        cost, dist, dA, dB = matrix_pair(name, b)
        assert bits(got["cost"][b]) == bits(cost) and bits(got["dist"][b]) == bits(dist), (b, got["cost"][b], cost)
        assert same(got["dA"][b], dA) and same(got["dB"][b], dB), b
    assert same(got["dist"], got["cost"] / np.asarray(cA, np.float32))
    assert_padding_is_plus_zero(got["dA"], cA), assert_padding_is_plus_zero(got["dB"], cB)
    assert same(entry(lib, A, cA, B, cB, outs=(True, False))["cost"], got["cost"])
    assert same(entry(lib, A, cA, B, cB, outs=(False, True))["dist"], got["dist"])


@pytest.mark.parametrize("name", PC.EMD_ORACLE_CASES)
def test_oracle_bars(name):
    """dist, dA and dB under the case's W within GPU_FACTOR x the recorded float32 floors of the float64 oracle"""
    A, B, cA, cB, W = PC.emd_make(name)
    got = batch(name)
    dev = PC.emd_deviation({"dist": got["dist"], "dA": np.nan_to_num(got["dA"], nan=np.inf), "dB": np.nan_to_num(got["dB"], nan=np.inf)},
                           PC.emd_oracle(name))
    print(name, {q: "%.3g (bar %.3g)" % (v, PC.GPU_FACTOR * PC.EMD_FLOOR[q]) for q, v in dev.items()})
    for q, v in dev.items():
        assert v <= PC.GPU_FACTOR * PC.EMD_FLOOR[q], (q, v)


@pytest.mark.parametrize("name", ["tiles", "wide", "cap"])
def test_the_two_forms_give_the_same_bits(lib, name):
    """form 1 (one launch) and form 2 (per pass), forward and gradients: a case below the switch, one above it and the cap"""
    one, two = batch(name, 1), batch(name, 2)
    for k in ("cost", "dist", "dA", "dB"):
        assert same(one[k], two[k]) and same(one[k], batch(name)[k]), k


def test_the_switch_lies_between_the_form_cases():
    """the library's choice is by the padded width: `tiles` (130) is below the switch, `wide` (300) and `cap` (2048) are at or above it
    -- the named constant of csrc/emd_pairs.hip read from the source"""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dpdist_amd", "csrc", "emd_pairs.hip")).read()
    switch = int(re.search(r"#define DPD_EMD_PAIRS_PER_PASS_FROM (\d+)", src).group(1))
    assert 130 < switch <= 300


@pytest.mark.parametrize("name", ["tiny", "tiles", "wide"])
@pytest.mark.parametrize("form", [1, 2])
def test_invariance(lib, name, form):
    """a second call, wider padding with another NaN payload, the other pairs of the batch and full counts change no bit"""
    A, B, cA, cB, W = PC.emd_make(name)
    first = batch(name, form)
    again = entry(lib, A, cA, B, cB, W, form)
    for k in first:
        assert same(first[k], again[k]), k
    wA, wB = A.shape[1] + 29, B.shape[1] + 61
    wide = entry(lib, A, cA, B, cB, W, form, wA, wB, fill_bits=0xFFC12345)
    assert same(wide["cost"], first["cost"]) and same(wide["dist"], first["dist"])
    assert same(wide["dA"][:, :A.shape[1]], first["dA"]) and same(wide["dB"][:, :B.shape[1]], first["dB"])
    assert_padding_is_plus_zero(wide["dA"], cA), assert_padding_is_plus_zero(wide["dB"], cB)
    for b in range(len(cA)):                                          # each pair alone, P = 1, at its own width and without counts
        alone = entry(lib, A[b:b + 1, :cA[b]], cA[b:b + 1], B[b:b + 1, :cB[b]], cB[b:b + 1], W[b:b + 1], form, counts=False)
        assert same(alone["cost"][0], first["cost"][b]) and same(alone["dist"][0], first["dist"][b])
        assert same(alone["dA"][0], first["dA"][b, :cA[b]]) and same(alone["dB"][0], first["dB"][b, :cB[b]]), b


def test_full_counts_equal_no_counts(lib):
    A, B, cA, cB, W = PC.emd_make("dup_far")
    for form in (1, 2):
        x, y = batch("dup_far", form), entry(lib, A, cA, B, cB, W, form, counts=False)
        for k in x:
            assert same(x[k], y[k]), (form, k)


def test_more_pairs_than_workgroups_of_one_launch(lib):
    """2^20 + 3 pairs of 2 / 3 points, forward only, both forms: the kernels stride over their pairs; the first and last pairs against
    the all-pairs entry on those pairs alone"""
    from dpdist_amd import emd, emd_matrix
    P = (1 << 20) + 3
    rng = np.random.default_rng(6)
    A = torch.from_numpy(rng.uniform(-0.8, 0.8, (P, 2, 3)).astype(np.float32)).to(DEV)
    B = torch.from_numpy(rng.uniform(-0.8, 0.8, (P, 3, 3)).astype(np.float32)).to(DEV)
    D1, D2 = emd._pairs_forward(A, B, None, None, 1), emd._pairs_forward(A, B, None, None, 2)
    assert torch.equal(D1, D2)
    for b in (0, 1, P - 2, P - 1):
        assert torch.equal(emd_matrix(A[b:b + 1], B[b:b + 1])[0, 0], D1[b])
    head = emd.emd_forward(A[:1024].contiguous(), B[:1024].contiguous(), False, False)[0] / 2
    tail = emd.emd_forward(A[-1024:].contiguous(), B[-1024:].contiguous(), False, False)[0] / 2
    assert torch.equal(D1[:1024], head) and torch.equal(D1[-1024:], tail)


def test_skipped_sides(lib):
    A, B, cA, cB, W = PC.emd_make("tiles")
    for form in (1, 2):
        both = batch("tiles", form)
        only_a = entry(lib, A, cA, B, cB, W, form, sides=(True, False))
        only_b = entry(lib, A, cA, B, cB, W, form, sides=(False, True))
        assert only_a["dB"] is None and only_b["dA"] is None and same(only_a["dA"], both["dA"]) and same(only_b["dB"], both["dB"])


def test_refusals_leave_the_outputs_untouched(lib):
    from dpdist_amd import lib as L
    x = torch.zeros(2, 8, 3, device=DEV)
    out, check = G.banded_flat(2 * 8 * 3, device=DEV)
    ws, check_ws = G.banded_flat(1 << 12, device=DEV)
    p, s = L.ptr, L.cur_stream()
    need = lib.dpd_emd_pairs_workspace_bytes(2, 8, 8)
    fwd = lambda Wa, P, form, nb=need, c=out: lib.dpd_emd_pairs_fwd(p(x), None, Wa, p(x), None, 8, P, form, p(c), p(c), p(ws), nb, s)   # noqa: E731
    bwd = lambda Wa, P, form, nb=need, w=x: lib.dpd_emd_pairs_bwd(p(x), None, Wa, p(x), None, 8, P, form, p(w), p(out), p(out), p(ws), nb, s)   # noqa: E731
    assert fwd(8, 0, 0) == -2 and fwd(8, 2, 3) == -2 and fwd(2049, 2, 0) == -3 and fwd(8, 2, 0, need - 1) == -4 and fwd(8, 2, 1, c=None) == -1
    assert bwd(8, 0, 0) == -2 and bwd(8, 2, -1) == -2 and bwd(2049, 2, 0) == -3 and bwd(8, 2, 2, need - 1) == -4 and bwd(8, 2, 0, w=None) == -1
    torch.cuda.synchronize()
    check(), check_ws()
    assert G.untouched(out) and G.untouched(ws)


def module_grads(mod, A, cA, B, cB, W, needA=True, needB=True):
    """EMDPairs / EMDMatrix on NaN-padded device sets under the upstream W (of D's shape) -> (D, grad A | None, grad B | None)"""
    a, ac = dev_set(A, cA)
    b, bc = dev_set(B, cB)
    a.requires_grad_(needA), b.requires_grad_(needB)
    D = mod(a, b, countsA=ac, countsB=bc)
    (D * torch.from_numpy(np.array(W, np.float32)).to(DEV).reshape(D.shape)).sum().backward()
    return D.detach(), a.grad, b.grad


@pytest.mark.parametrize("name", ["tiny", "tiles", "dup_far", "wide"])
def test_module(name):
    """EMDPairs: the values of emd_pairs and of the C entry bit for bit, EMDMatrix's values and gradients on each pair alone; host counts are
    taken too; a set without requires_grad gets None and the other side's bits stay"""
    from dpdist_amd import EMDMatrix, EMDPairs, emd_pairs
    A, B, cA, cB, W = PC.emd_make(name)
    got = batch(name)
    D, gA, gB = module_grads(EMDPairs(), A, cA, B, cB, W)
    a, ac = dev_set(A, cA)
    b, _ = dev_set(B, cB)
    assert same(emd_pairs(a, b, countsA=ac, countsB=list(cB)), D) and same(D, got["dist"])
    assert same(gA, got["dA"]) and same(gB, got["dB"])
    for p in range(len(cA)):
        D1, gA1, gB1 = module_grads(EMDMatrix(), A[p:p + 1], cA[p:p + 1], B[p:p + 1], cB[p:p + 1], W[p:p + 1])
        assert same(D[p], D1[0, 0]) and same(gA[p], gA1[0]) and same(gB[p], gB1[0]), p
    Da, ga, none_b = module_grads(EMDPairs(), A, cA, B, cB, W, True, False)
    Db, none_a, gb = module_grads(EMDPairs(), A, cA, B, cB, W, False, True)
    assert none_a is None and none_b is None and same(Da, D) and same(Db, D) and same(ga, gA) and same(gb, gB)
    plain = EMDPairs()(a, b, countsA=ac, countsB=list(cB))
    assert not plain.requires_grad and same(plain, D)

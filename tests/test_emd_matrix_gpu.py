"""All-pairs Earth Mover's distance on the GPU (dpd_emd_matrix_fwd / _bwd, dpdist_amd.emd: emd_matrix / EMDMatrix) against the paired entry
dpd_emd_fwd on each pair alone (bit for bit) and the float64 oracle of tests/emd_matrix_cases.py (at 8 x the recorded floors).  Outputs
of the C entries sit in NaN-payload guard bands, input padding holds a quiet NaN: padding that reached a result would poison it."""
import functools

import numpy as np
import pytest
import torch

from tests import baseline_cases as BC
from tests import emd_matrix_cases as EC
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


def dev_set(X, counts, width=None, fill_bits=0x7FC00000):
    """the set on the device: cut to its counts, padded to `width` with a NaN; counts as an int32 device tensor"""
    width = X.shape[1] if width is None else width
    return torch.from_numpy(BC.padded(X, counts, width, fill_bits)).to(DEV), torch.tensor(counts, dtype=torch.int32, device=DEV)


def entry_fwd(lib, A, cA, B, cB, wA=None, wB=None, counts=True, fill_bits=0x7FC00000):
    """dpd_emd_matrix_fwd into guard-banded outputs -> (cost, dist) as numpy [Ca,Cb]; the bands are checked"""
    from dpdist_amd import lib as L
    a, ac = dev_set(A, cA, wA, fill_bits)
    b, bc = dev_set(B, cB, wB, fill_bits)
    Ca, Cb = len(cA), len(cB)
    outs = [G.banded_flat(Ca * Cb, device=DEV) for _ in range(2)]
    rc = lib.dpd_emd_matrix_fwd(L.ptr(a), L.ptr(ac) if counts else None, Ca, a.shape[1], L.ptr(b), L.ptr(bc) if counts else None, Cb, b.shape[1],
                                *[L.ptr(v) for v, _ in outs], L.cur_stream())
    assert rc == 0
    torch.cuda.synchronize()
    for _, check in outs:
        check()
    return [v.cpu().numpy().reshape(Ca, Cb).copy() for v, _ in outs]


def entry_bwd(lib, A, cA, B, cB, W, wA=None, wB=None, fill_bits=0x7FC00000, sides=(True, True)):
    """dpd_emd_matrix_bwd into guard-banded gradients and a guard-banded workspace -> (dA [Ca,wA,3] | None, dB [Cb,wB,3] | None) as numpy"""
    from dpdist_amd import lib as L
    a, ac = dev_set(A, cA, wA, fill_bits)
    b, bc = dev_set(B, cB, wB, fill_bits)
    w = torch.from_numpy(np.array(W, np.float32)).to(DEV)
    need = lib.dpd_emd_matrix_workspace_bytes(len(cA), a.shape[1], len(cB), b.shape[1])
    assert need == len(cA) * len(cB) * (a.shape[1] + b.shape[1]) * 12
    ws, ck_ws = G.banded_flat(need // 4, device=DEV)
    (da, ck_a), (db, ck_b) = G.banded_flat(a.numel(), device=DEV), G.banded_flat(b.numel(), device=DEV)
    rc = lib.dpd_emd_matrix_bwd(L.ptr(a), L.ptr(ac), len(cA), a.shape[1], L.ptr(b), L.ptr(bc), len(cB), b.shape[1], L.ptr(w),
                                L.ptr(da) if sides[0] else None, L.ptr(db) if sides[1] else None, 0, L.ptr(ws), need, L.cur_stream())
    assert rc == 0
    torch.cuda.synchronize()
    ck_ws(), ck_a(), ck_b()
    for x, used in ((da, sides[0]), (db, sides[1])):
        assert used or G.untouched(x)
    return (da.cpu().view(a.shape).numpy().copy() if sides[0] else None), (db.cpu().view(b.shape).numpy().copy() if sides[1] else None)


@functools.lru_cache(maxsize=None)
def paired(name, i, j):
    """dpd_emd_fwd on pair (i, j) of a case alone, widths cut to the counts, gscale = n_i so that the gradients leave unscaled
    -> (cost[0], grad1 [n,3], grad2 [m,3]) as numpy; computed once and shared"""
    from dpdist_amd import emd
    A, B, cA, cB, _ = EC.make(name)
    x1 = torch.from_numpy(A[i:i + 1, :cA[i]].copy()).to(DEV)
    x2 = torch.from_numpy(B[j:j + 1, :cB[j]].copy()).to(DEV)
    cost, _, g1, g2, _ = emd.emd_forward(x1, x2, True, True, False, gscale=float(cA[i]))
    return cost.cpu().numpy()[0], g1.cpu().numpy()[0], g2.cpu().numpy()[0]


@functools.lru_cache(maxsize=None)
def matrix(name):
    """(cost, dist, dA, dB) of a case through the C entries under the case's W, computed once and shared"""
    A, B, cA, cB, W = EC.make(name)
    cost, dist = entry_fwd(lib_(), A, cA, B, cB)
    dA, dB = entry_bwd(lib_(), A, cA, B, cB, W)
    return cost, dist, dA, dB


def assert_padding_is_plus_zero(g, counts):
    """rows at or beyond a cloud's count: the bit pattern of +0.0"""
    b = bits(g)
    for c, n in enumerate(counts):
        assert not b[c, n:].any(), c


@pytest.mark.parametrize("name", EC.CASES)
def test_cost_is_the_paired_entrys_bit_for_bit(lib, name):
    A, B, cA, cB, _ = EC.make(name)
    cost, dist = entry_fwd(lib, A, cA, B, cB)
    for i, n in enumerate(cA):
        for j in range(len(cB)):
            assert bits(cost[i, j]) == bits(paired(name, i, j)[0]), (i, j, cost[i, j], paired(name, i, j)[0])
    assert np.array_equal(bits(dist), bits(cost / np.asarray(cA, np.float32)[:, None]))
    only_cost = entry_fwd_one(lib, A, cA, B, cB, 0)
    only_dist = entry_fwd_one(lib, A, cA, B, cB, 1)
    assert np.array_equal(bits(only_cost), bits(cost)) and np.array_equal(bits(only_dist), bits(dist))


def entry_fwd_one(lib, A, cA, B, cB, which):
    """the forward entry with only one of its two outputs"""
    from dpdist_amd import lib as L
    a, ac = dev_set(A, cA)
    b, bc = dev_set(B, cB)
    out, check = G.banded_flat(len(cA) * len(cB), device=DEV)
    rc = lib.dpd_emd_matrix_fwd(L.ptr(a), L.ptr(ac), len(cA), a.shape[1], L.ptr(b), L.ptr(bc), len(cB), b.shape[1],
                                L.ptr(out) if which == 0 else None, L.ptr(out) if which == 1 else None, L.cur_stream())
    assert rc == 0
    torch.cuda.synchronize()
    check()
    return out.cpu().numpy().reshape(len(cA), len(cB)).copy()


@pytest.mark.parametrize("name", EC.ORACLE_CASES)
def test_oracle_bars(name):
    """dist, dA and dB under the case's random W within GPU_FACTOR x the recorded float32 floors of the float64 oracle"""
    A, B, cA, cB, W = EC.make(name)
    _, dist, dA, dB = matrix(name)
    dev = EC.deviation({"dist": dist, "dA": np.nan_to_num(dA, nan=np.inf), "dB": np.nan_to_num(dB, nan=np.inf)}, EC.oracle(name))
    print(name, {q: "%.3g (bar %.3g)" % (v, EC.GPU_FACTOR * EC.FLOOR[q]) for q, v in dev.items()})
    for q, v in dev.items():
        assert v <= EC.GPU_FACTOR * EC.FLOOR[q], (q, v)
    assert_padding_is_plus_zero(dA, cA), assert_padding_is_plus_zero(dB, cB)


@pytest.mark.parametrize("name", EC.CASES)
def test_one_hot_upstream_isolates_a_pair(lib, name):
    """W[i,j] = n_i and 0 elsewhere: dA[i] and dB[j] are grad1 / grad2 of dpd_emd_fwd(gscale = n_i, B = 1) on the pair alone, bit for
    bit in value (np.array_equal), and every other row is 0"""
    A, B, cA, cB, _ = EC.make(name)
    for i, n in enumerate(cA):
        for j, m in enumerate(cB):
            W = np.zeros((len(cA), len(cB)), np.float32)
            W[i, j] = n
            dA, dB = entry_bwd(lib, A, cA, B, cB, W)
            _, g1, g2 = paired(name, i, j)
            assert np.array_equal(dA[i, :n], g1) and np.array_equal(dB[j, :m], g2), (i, j)
            dA[i, :n] = 0
            dB[j, :m] = 0
            assert not dA.any() and not dB.any(), (i, j)


@pytest.mark.parametrize("name", ["tiny", "tiles", "wide"])
def test_invariance(lib, name):
    """a second call, wider padded widths, another padding pattern and other clouds around a pair change no bit of the pair's values"""
    A, B, cA, cB, W = EC.make(name)
    cost, dist, dA, dB = matrix(name)
    again = entry_fwd(lib, A, cA, B, cB) + list(entry_bwd(lib, A, cA, B, cB, W))
    for x, y in zip((cost, dist, dA, dB), again):
        assert np.array_equal(bits(x), bits(y))
    wA, wB = A.shape[1] + 29, B.shape[1] + 61                     # "wide": 329 / 318, still the same form of the kernel
    c2, d2 = entry_fwd(lib, A, cA, B, cB, wA, wB, fill_bits=0xFFC12345)
    dA2, dB2 = entry_bwd(lib, A, cA, B, cB, W, wA, wB, fill_bits=0xFFC12345)
    assert np.array_equal(bits(c2), bits(cost)) and np.array_equal(bits(d2), bits(dist))
    assert np.array_equal(bits(dA2[:, :A.shape[1]]), bits(dA)) and np.array_equal(bits(dB2[:, :B.shape[1]]), bits(dB))
    assert_padding_is_plus_zero(dA2, cA), assert_padding_is_plus_zero(dB2, cB)
    # the last cloud of each set alone, without counts and at its own width: the other clouds leave no trace in the pair's values
    i, j = len(cA) - 1, len(cB) - 1
    alone = entry_fwd(lib, A[i:, :cA[i]], [cA[i]], B[j:, :cB[j]], [cB[j]], counts=False)
    assert bits(alone[0][0, 0]) == bits(cost[i, j]) and bits(alone[1][0, 0]) == bits(dist[i, j])


def test_narrow_and_wide_forms_agree(lib):
    """one pair of 200 / 190 points at its own widths (below the width from which four owner tiles are in flight) and padded to 300 / 257
    (above it): the same bits from both forms of the kernel, forward and backward"""
    rng = np.random.default_rng(99)
    A, B = rng.uniform(-0.8, 0.8, (1, 200, 3)).astype(np.float32), rng.uniform(-0.8, 0.8, (1, 190, 3)).astype(np.float32)
    W = np.full((1, 1), 200, np.float32)
    narrow = entry_fwd(lib, A, [200], B, [190]) + list(entry_bwd(lib, A, [200], B, [190], W))
    wide = entry_fwd(lib, A, [200], B, [190], 300, 257) + list(entry_bwd(lib, A, [200], B, [190], W, 300, 257))
    for k, (x, y) in enumerate(zip(narrow, wide)):
        assert np.array_equal(bits(x), bits(y[:, :x.shape[1]] if k >= 2 else y)), k


def test_more_pairs_than_workgroups_of_one_launch(lib):
    """(2^20 + 1024) pairs of 2 / 3 points: the kernel strides; the first and the last row against the paired entry on those pairs"""
    from dpdist_amd import emd, emd_matrix
    rng = np.random.default_rng(5)
    A = torch.from_numpy(rng.uniform(-0.8, 0.8, (1025, 2, 3)).astype(np.float32)).to(DEV)
    B = torch.from_numpy(rng.uniform(-0.8, 0.8, (1024, 3, 3)).astype(np.float32)).to(DEV)
    D = emd_matrix(A, B)
    for i in (0, 1024):
        cost = emd.emd_forward(A[i:i + 1].expand(1024, 2, 3).contiguous(), B, False, False)[0]
        assert torch.equal(D[i], cost / 2)


def test_skipped_sides_and_accumulation(lib):
    """one side at a time gives the bits of both sides together and leaves the other pointer alone; rows of A sent one by one with
    accumulate_dB from the second on give the bits of one call"""
    from dpdist_amd import lib as L
    A, B, cA, cB, W = EC.make("tiles")
    _, _, dA, dB = matrix("tiles")
    assert np.array_equal(bits(entry_bwd(lib, A, cA, B, cB, W, sides=(True, False))[0]), bits(dA))
    assert np.array_equal(bits(entry_bwd(lib, A, cA, B, cB, W, sides=(False, True))[1]), bits(dB))
    a, ac = dev_set(A, cA)
    b, bc = dev_set(B, cB)
    w = torch.from_numpy(W.copy()).to(DEV)
    need = lib.dpd_emd_matrix_workspace_bytes(1, a.shape[1], len(cB), b.shape[1])
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    db, check = G.banded_flat(b.numel(), device=DEV)
    for i in range(len(cA)):
        assert lib.dpd_emd_matrix_bwd(L.ptr(a[i:]), L.ptr(ac[i:]), 1, a.shape[1], L.ptr(b), L.ptr(bc), len(cB), b.shape[1], L.ptr(w[i:]), None,
                                      L.ptr(db), int(i > 0), L.ptr(ws), need, L.cur_stream()) == 0
    torch.cuda.synchronize()
    check()
    assert np.array_equal(bits(db.view(b.shape)), bits(dB))


def test_refusals_leave_the_outputs_untouched(lib):
    from dpdist_amd import lib as L
    x = torch.zeros(2, 8, 3, device=DEV)
    out, check = G.banded_flat(2 * 8 * 3, device=DEV)
    ws = torch.empty(1 << 16, dtype=torch.uint8, device=DEV)
    p, s = L.ptr, L.cur_stream()
    assert lib.dpd_emd_matrix_fwd(p(x), None, 0, 8, p(x), None, 2, 8, p(out), p(out), s) == -2
    assert lib.dpd_emd_matrix_fwd(p(x), None, 2, 2049, p(x), None, 2, 8, p(out), p(out), s) == -3
    assert lib.dpd_emd_matrix_bwd(p(x), None, 2, 8, p(x), None, 2, 8, None, p(out), p(out), 0, p(ws), ws.numel(), s) == -1
    assert lib.dpd_emd_matrix_bwd(p(x), None, 2, 8, p(x), None, 2, 8, p(x), p(out), p(out), 0, p(ws), 2 * 2 * 16 * 12 - 1, s) == -4
    torch.cuda.synchronize()
    check()
    assert G.untouched(out)


def module_grads(A, B, cA, cB, W, needA=True, needB=True, **kw):
    """EMDMatrix on NaN-padded device sets under the upstream W -> (D, grad A | None, grad B | None) as device tensors"""
    from dpdist_amd import EMDMatrix
    a, ac = dev_set(A, cA)
    b, bc = dev_set(B, cB)
    a.requires_grad_(needA), b.requires_grad_(needB)
    D = EMDMatrix()(a, b, countsA=ac, countsB=bc, **kw)
    (D * torch.from_numpy(W.copy()).to(DEV)).sum().backward()
    return D.detach(), a.grad, b.grad


@pytest.mark.parametrize("name", ["tiny", "tiles"])
def test_module(name):
    """EMDMatrix: the values of emd_matrix and of the C entry bit for bit, the entries' gradients; host counts are taken too"""
    from dpdist_amd import emd_matrix
    A, B, cA, cB, W = EC.make(name)
    _, dist, dA, dB = matrix(name)
    D, gA, gB = module_grads(A, B, cA, cB, W)
    a, ac = dev_set(A, cA)
    b, _ = dev_set(B, cB)
    assert torch.equal(emd_matrix(a, b, countsA=ac, countsB=list(cB)), D) and np.array_equal(bits(D), bits(dist))
    assert np.array_equal(bits(gA), bits(dA)) and np.array_equal(bits(gB), bits(dB))


def test_chunked_backward_changes_no_bit(monkeypatch):
    """the workspace bound lowered to one row of A per chunk (3 chunks): the bits of the single chunk"""
    from dpdist_amd import emd
    rng = np.random.default_rng(11)
    A, B = rng.uniform(-0.8, 0.8, (3, 70, 3)).astype(np.float32), rng.uniform(-0.8, 0.8, (2, 33, 3)).astype(np.float32)
    cA, cB, W = (70, 9, 65), (33, 20), rng.standard_normal((3, 2)).astype(np.float32)
    assert emd.MAX_WS_BYTES >= 3 * 2 * (70 + 33) * 12
    D, gA, gB = module_grads(A, B, cA, cB, W)
    calls = []
    real = emd.L.load().dpd_emd_matrix_bwd
    monkeypatch.setattr(emd, "MAX_WS_BYTES", 2 * (70 + 33) * 12 + 5)
    monkeypatch.setattr(emd.L.load(), "dpd_emd_matrix_bwd", lambda *a: calls.append(a[2]) or real(*a))
    D2, gA2, gB2 = module_grads(A, B, cA, cB, W)
    assert calls == [1, 1, 1]
    assert torch.equal(D, D2) and np.array_equal(bits(gA), bits(gA2)) and np.array_equal(bits(gB), bits(gB2))


def test_a_set_against_itself():
    """EMDMatrix()(A) = EMDMatrix()(A, A.clone()) in D, and its gradient is the sum of the two-set gradients (test_oracle_bars holds the
    two routes of this case to the oracle)"""
    from dpdist_amd import EMDMatrix
    A, _, cA, _, W = EC.make("self")
    D2, gA2, gB2 = module_grads(A, A, cA, cA, W)
    a, ac = dev_set(A, cA)
    a.requires_grad_(True)
    D = EMDMatrix()(a, countsA=ac)
    (D * torch.from_numpy(W.copy()).to(DEV)).sum().backward()
    assert torch.equal(D, D2) and np.array_equal(bits(a.grad), bits(gA2 + gB2))
    assert_padding_is_plus_zero(a.grad, cA)


def test_skipped_routes():
    """requires_grad on one set only: None for the other, the same bits for the one; no gradient at all: a plain forward"""
    from dpdist_amd import EMDMatrix
    A, B, cA, cB, W = EC.make("tiles")
    D, gA, gB = module_grads(A, B, cA, cB, W)
    Da, ga, none_b = module_grads(A, B, cA, cB, W, True, False)
    Db, none_a, gb = module_grads(A, B, cA, cB, W, False, True)
    assert none_a is None and none_b is None
    assert torch.equal(Da, D) and torch.equal(Db, D) and np.array_equal(bits(ga), bits(gA)) and np.array_equal(bits(gb), bits(gB))
    a, ac = dev_set(A, cA)
    b, bc = dev_set(B, cB)
    plain = EMDMatrix()(a, b, countsA=ac, countsB=bc)
    assert not plain.requires_grad and torch.equal(plain, D)

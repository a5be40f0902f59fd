"""Per-pair Chamfer / Hausdorff on the GPU (dpd_chamfer_pairs_fwd / _bwd, dpdist_amd.baselines: chamfer_pairs / hausdorff_pairs /
ChamferPairs) against the all-pairs entry and ChamferMatrix on each pair alone (bit for bit) and the float64 oracle of
tests/baseline_cases.py (at its bars).  Outputs, argmin buffers and gradients of the C entries sit in NaN-payload guard bands, input
padding holds a quiet NaN: padding that reached a result would poison it."""
import functools

import numpy as np
import pytest
import torch

from tests import baseline_cases as BC
from tests import baseline_pairs_cases as PC
from tests import gemm_cases as G

pytestmark = pytest.mark.gpu
DEV = "cuda"
FORMS = (("squared", 0, 4), ("sqrt", 1, 8))                           # (name, the entries' form, grad_ok's c)


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
    """the set on the device: cut to its counts, padded to `width` with a NaN; counts as an int32 device tensor"""
    width = X.shape[1] if width is None else width
    return torch.from_numpy(BC.padded(X, counts, width, fill_bits)).to(DEV), torch.tensor(counts, dtype=torch.int32, device=DEV)


def dev_vec(g):
    return None if g is None else torch.from_numpy(np.array(g, np.float32)).to(DEV)


def entry(lib, A, cA, B, cB, form=None, Gab=None, Gba=None, wA=None, wB=None, counts=True, fill_bits=0x7FC00000, sides=(True, True)):
    """dpd_chamfer_pairs_fwd into guard-banded outputs and, with a form, dpd_chamfer_pairs_bwd on its argmins into guard-banded gradients
    -> dict of numpy arrays: min_ab / arg_ab [P,wB], min_ba / arg_ba [P,wA], mean_sq / mean_rt / max_sq [2,P], dA, dB (None when
    skipped).  Every band is checked; entries of min / arg at or beyond a count must still hold the fill."""
    from dpdist_amd import lib as L
    a, ac = dev_set(A, cA, wA, fill_bits)
    b, bc = dev_set(B, cB, wB, fill_bits)
    P, Wa, Wb = len(cA), a.shape[1], b.shape[1]
    pa, pb = (L.ptr(ac), L.ptr(bc)) if counts else (None, None)
    bufs = {"min_ab": G.banded_flat(P * Wb, device=DEV), "arg_ab": G.banded_flat(P * Wb, dtype=torch.int32, device=DEV),
            "min_ba": G.banded_flat(P * Wa, device=DEV), "arg_ba": G.banded_flat(P * Wa, dtype=torch.int32, device=DEV)}
    outs = {n: G.banded_flat(2 * P, device=DEV) for n in ("mean_sq", "mean_rt", "max_sq")}
    rc = lib.dpd_chamfer_pairs_fwd(L.ptr(a), pa, Wa, L.ptr(b), pb, Wb, P, *[L.ptr(bufs[n][0]) for n in ("min_ab", "arg_ab", "min_ba", "arg_ba")],
                                   *[L.ptr(outs[n][0]) for n in ("mean_sq", "mean_rt", "max_sq")], L.cur_stream())
    assert rc == 0
    res = {}
    if form is not None:
        grads = {"dA": G.banded_flat(a.numel(), device=DEV), "dB": G.banded_flat(b.numel(), device=DEV)}
        gab, gba = dev_vec(Gab), dev_vec(Gba)
        rc = lib.dpd_chamfer_pairs_bwd(L.ptr(a), pa, Wa, L.ptr(b), pb, Wb, P, form, L.ptr(bufs["arg_ab"][0]), L.ptr(bufs["arg_ba"][0]),
                                       L.ptr(gab), L.ptr(gba), L.ptr(grads["dA"][0]) if sides[0] else None,
                                       L.ptr(grads["dB"][0]) if sides[1] else None, L.cur_stream())
        assert rc == 0
        torch.cuda.synchronize()
        for (n, (v, check)), used, like in zip(grads.items(), sides, (a, b)):
            check()
            assert used or G.untouched(v)
            res[n] = v.cpu().view(like.shape).numpy().copy() if used else None
    torch.cuda.synchronize()
    for n, (v, check) in list(bufs.items()) + list(outs.items()):
        check()
    for n, (v, _) in bufs.items():
        W = Wb if n.endswith("ab") else Wa
        res[n] = v.cpu().numpy().reshape(P, W).copy()
        for p, cnt in enumerate(cB if n.endswith("ab") else cA):     # beyond the count: not written
            assert (res[n][p, cnt:].view(np.int32) == np.int32(G.NAN_OUT)).all(), (n, p)
    for n, (v, _) in outs.items():
        res[n] = v.cpu().numpy().reshape(2, P).copy()
    return res


@functools.lru_cache(maxsize=None)
def batch(name, form=None, which="all"):
    """a case through the C entries, computed once and shared; which: "D" (upstream on D alone: G/2 each way) or "all" (G/2 + G_ab, G/2 + G_ba)"""
    A, B, cA, cB = PC.chamfer_make(name)
    Gab, Gba = entry_upstreams(name, which)
    return entry(lib_(), A, cA, B, cB, form, Gab, Gba)


def entry_upstreams(name, which):
    """the two directed upstreams as ChamferMatrix forms them from (G, G_ab, G_ba): float32 torch arithmetic"""
    g, gab, gba = (torch.from_numpy(x.copy()) for x in PC.chamfer_upstreams(name))
    half = g / 2
    return (half.numpy(), half.numpy()) if which == "D" else ((half + gab).numpy(), (half + gba).numpy())


@functools.lru_cache(maxsize=None)
def matrix_pair(name, b):
    """dpd_chamfer_matrix_fwd on pair b alone (Cs = Cq = 1, the pair's counts), both directions -> {"mean_sq": (ab, ba), ...} as numpy scalars"""
    from dpdist_amd import lib as L
    A, B, cA, cB = PC.chamfer_make(name)
    a, ac = dev_set(A[b:b + 1], cA[b:b + 1])
    q, qc = dev_set(B[b:b + 1], cB[b:b + 1])
    res = {}
    for d, (S, sc, Q, qq) in enumerate(((a, ac, q, qc), (q, qc, a, ac))):
        out = torch.empty(3, device=DEV)
        assert lib_().dpd_chamfer_matrix_fwd(L.ptr(S), L.ptr(sc), 1, S.shape[1], L.ptr(Q), L.ptr(qq), 1, Q.shape[1], L.ptr(out[0:]), L.ptr(out[1:]),
                                             L.ptr(out[2:]), L.cur_stream()) == 0
        for k, n in enumerate(("mean_sq", "mean_rt", "max_sq")):
            res.setdefault(n, []).append(out.cpu().numpy()[k])
    return res


def module_grads(mod, A, cA, B, cB, ups, needA=True, needB=True, wA=None, wB=None):
    """ChamferPairs / ChamferMatrix on NaN-padded device sets under the upstreams (G, G_ab, G_ba) (None = absent), each of D's shape
    -> ((D, D_AB, D_BA), grad A | None, grad B | None)"""
    a, ac = dev_set(A, cA, wA)
    b, bc = dev_set(B, cB, wB)
    a.requires_grad_(needA), b.requires_grad_(needB)
    out = mod(a, b, True, countsA=ac, countsB=bc)
    sum((o * torch.from_numpy(np.array(u, np.float32)).to(DEV).reshape(o.shape)).sum() for o, u in zip(out, ups) if u is not None).backward()
    return tuple(o.detach() for o in out), a.grad, b.grad


def assert_padding_is_plus_zero(g, counts):
    x = bits(g)
    for c, n in enumerate(counts):
        assert not x[c, n:].any(), c


# ------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("name", PC.CHAMFER_CASES)
def test_forward_is_the_matrix_entrys_on_the_pair_alone_bit_for_bit(lib, name):
    A, B, cA, cB = PC.chamfer_make(name)
    got = batch(name)
    for b in range(len(cA)):
        ref = matrix_pair(name, b)
        for n in ("mean_sq", "mean_rt", "max_sq"):
            for d in range(2):
                assert bits(got[n][d, b]) == bits(ref[n][d]), (n, d, b, got[n][d, b], ref[n][d])
        # the minima and their lowest-index argmins are exact in the float32 restatement
        d_ab, d_ba = BC.d2_f32(B[b, :cB[b]], A[b, :cA[b]]), BC.d2_f32(A[b, :cA[b]], B[b, :cB[b]])
        assert same(got["min_ab"][b, :cB[b]], d_ab.min(1)) and np.array_equal(got["arg_ab"][b, :cB[b]].view(np.int32), d_ab.argmin(1))
        assert same(got["min_ba"][b, :cA[b]], d_ba.min(1)) and np.array_equal(got["arg_ba"][b, :cA[b]].view(np.int32), d_ba.argmin(1))
    if name == "full":
        assert not bits(got["mean_sq"][:, 0]).any() and not bits(got["mean_rt"][:, 0]).any() and not bits(got["max_sq"][:, 0]).any()


@pytest.mark.parametrize("name", PC.CHAMFER_CASES)
def test_means_against_float64(name):
    A, B, cA, cB = PC.chamfer_make(name)
    got, ref = batch(name), PC.chamfer_fwd_oracle(name)
    for b in range(len(cA)):
        for d, key in enumerate(("ab", "ba")):
            r = ref[key][b]
            assert bits(got["max_sq"][d, b]) == bits(r["max_sq"][0, 0])
            for n in ("mean_sq", "mean_rt"):
                ok, ratio = BC.mean_ok(got[n][d, b], r[n][0, 0], r["n"][0, 0])
                print(name, b, key, n, "error / bar %.3g" % ratio)
                assert ok, (n, key, b, ratio)


@pytest.mark.parametrize("name", ["full", "ragged", "chunks"])
@pytest.mark.parametrize("form", ["squared", "sqrt"])
def test_functions_and_module_forward(name, form):
    """chamfer_pairs / hausdorff_pairs / ChamferPairs: the entry's bits, D = (D_AB + D_BA) / 2 at its bar, hausdorff_matrix of each pair"""
    from dpdist_amd import ChamferPairs, chamfer_pairs, hausdorff_matrix, hausdorff_pairs
    A, B, cA, cB = PC.chamfer_make(name)
    got, ref = batch(name), PC.chamfer_fwd_oracle(name)
    a, ac = dev_set(A, cA)
    b, bc = dev_set(B, cB)
    key = "mean_sq" if form == "squared" else "mean_rt"
    D, Dab, Dba = chamfer_pairs(a, b, form, True, countsA=ac, countsB=list(cB))
    assert same(Dab, got[key][0]) and same(Dba, got[key][1]) and same(D, (Dab + Dba) / 2)
    assert same(chamfer_pairs(a, b, form, countsA=list(cA), countsB=bc), D)
    for p in range(len(cA)):
        r_ab, r_ba = ref["ab"][p], ref["ba"][p]
        ok, ratio = BC.mean_ok(D[p].item(), (r_ab[key][0, 0] + r_ba[key][0, 0]) / 2, max(cA[p], cB[p]), extra=3)
        assert ok, (p, ratio)
    mod = ChamferPairs(form)
    for x, y in zip(mod(a, b, True, countsA=ac, countsB=bc), (D, Dab, Dba)):
        assert same(x, y)
    a.requires_grad_(True)
    for x, y in zip(mod(a, b, True, countsA=ac, countsB=bc), (D, Dab, Dba)):
        assert x.requires_grad and same(x, y)
    a.requires_grad_(False)
    H, Hab, Hba = hausdorff_pairs(a, b, True, countsA=ac, countsB=bc)
    assert same(Hab, np.sqrt(got["max_sq"][0])) and same(Hba, np.sqrt(got["max_sq"][1])) and same(hausdorff_pairs(a, b, countsA=ac, countsB=bc), H)
    for p in range(len(cA)):
        one = hausdorff_matrix(a[p:p + 1], b[p:p + 1], True, countsA=ac[p:p + 1], countsB=bc[p:p + 1])
        assert same(H[p], one[0][0, 0]) and same(Hab[p], one[1][0, 0]) and same(Hba[p], one[2][0, 0])


def test_more_pairs_than_workgroups_of_one_launch():
    """2^20 + 3 pairs of one point each, forward only: the kernels stride over their units; every value is the exact float32 d2"""
    from dpdist_amd import chamfer_pairs, hausdorff_pairs
    A, B = PC.chamfer_make_many()
    d = (B[:, 0] - A[:, 0]).astype(np.float32)                          # d2_f32's operations on the diagonal alone (its grid would be P^2)
    d2 = ((d[:, 0] * d[:, 0]).astype(np.float32) + (d[:, 1] * d[:, 1]).astype(np.float32)).astype(np.float32) + (d[:, 2] * d[:, 2]).astype(np.float32)
    a, b = torch.from_numpy(A).to(DEV), torch.from_numpy(B).to(DEV)
    D, Dab, Dba = chamfer_pairs(a, b, "squared", True)
    assert same(Dab, d2) and same(Dba, d2) and same(D, d2)
    R = chamfer_pairs(a, b, "sqrt")
    H = hausdorff_pairs(a, b)
    assert same(R, np.sqrt(d2)) and same(H, np.sqrt(d2))


# ------------------------------------------------------------------------------------------------ backward
@pytest.mark.parametrize("name", PC.CHAMFER_CASES)
@pytest.mark.parametrize("form", FORMS, ids=[f[0] for f in FORMS])
@pytest.mark.parametrize("which", ["D", "all"])
def test_gradients_are_chamfer_matrix_on_the_pair_alone_and_within_the_oracles_bars(name, form, which):
    from dpdist_amd import ChamferMatrix, ChamferPairs
    fname, f, c = form
    A, B, cA, cB = PC.chamfer_make(name)
    g, gab, gba = PC.chamfer_upstreams(name)
    ups = (g, None, None) if which == "D" else (g, gab, gba)
    out, gA, gB = module_grads(ChamferPairs(fname), A, cA, B, cB, ups)
    assert_padding_is_plus_zero(gA, cA), assert_padding_is_plus_zero(gB, cB)
    got = batch(name, f, which)                                      # the C entry under the same directed upstreams: the module's bits
    assert same(gA, got["dA"]) and same(gB, got["dB"])
    oracle = PC.chamfer_bwd_oracle(name, f, *ups)
    for b in range(len(cA)):
        one = tuple(None if u is None else u[b:b + 1].reshape(1, 1) for u in ups)
        (D1, Dab1, Dba1), gA1, gB1 = module_grads(ChamferMatrix(fname), A[b:b + 1], cA[b:b + 1], B[b:b + 1], cB[b:b + 1], one)
        assert same(out[0][b], D1[0, 0]) and same(out[1][b], Dab1[0, 0]) and same(out[2][b], Dba1[0, 0])
        assert same(gA[b], gA1[0]) and same(gB[b], gB1[0]), b
        for x, ref, side in ((gA[b:b + 1], oracle[b][0], "A"), (gB[b:b + 1], oracle[b][1], "B")):
            ok, ratio = BC.grad_ok(x.cpu().numpy(), ref, c)
            print(name, fname, which, b, side, "error / bar %.3g" % ratio)
            assert ok, (b, side, ratio)


def test_one_directed_upstream_alone_skips_the_other_directions_routes():
    """an upstream on D_AB only: the bits of ChamferMatrix on each pair (which runs that direction alone), through a NULL G_ba"""
    from dpdist_amd import ChamferMatrix, ChamferPairs
    A, B, cA, cB = PC.chamfer_make("ragged")
    _, gab, gba = PC.chamfer_upstreams("ragged")
    for ups in ((None, gab, None), (None, None, gba)):
        for fname, f, c in FORMS:
            _, gA, gB = module_grads(ChamferPairs(fname), A, cA, B, cB, ups)
            for b in range(len(cA)):
                one = tuple(None if u is None else u[b:b + 1].reshape(1, 1) for u in ups)
                _, gA1, gB1 = module_grads(ChamferMatrix(fname), A[b:b + 1], cA[b:b + 1], B[b:b + 1], cB[b:b + 1], one)
                assert same(gA[b], gA1[0]) and same(gB[b], gB1[0]), (fname, b)


# ------------------------------------------------------------------------------------------------ invariance, skipped routes, refusals
@pytest.mark.parametrize("name", ["ragged", "chunks"])
def test_invariance(lib, name):
    """a second call, wider padding with another NaN payload, and the other pairs of the batch change no bit"""
    A, B, cA, cB = PC.chamfer_make(name)
    Gab, Gba = entry_upstreams(name, "all")
    keys = ("mean_sq", "mean_rt", "max_sq", "dA", "dB")
    for f in (0, 1):
        first = batch(name, f, "all")
        again = entry(lib, A, cA, B, cB, f, Gab, Gba)
        for k in keys + ("min_ab", "arg_ab", "min_ba", "arg_ba"):
            assert same(first[k], again[k]), k
        wA, wB = A.shape[1] + 29, B.shape[1] + 261                    # wider: more chunks, some wholly in the padding
        wide = entry(lib, A, cA, B, cB, f, Gab, Gba, wA, wB, fill_bits=0xFFC12345)
        for k in keys[:3]:
            assert same(first[k], wide[k]), k
        assert same(wide["dA"][:, :A.shape[1]], first["dA"]) and same(wide["dB"][:, :B.shape[1]], first["dB"])
        assert_padding_is_plus_zero(wide["dA"], cA), assert_padding_is_plus_zero(wide["dB"], cB)
        for b in range(len(cA)):                                      # each pair alone, P = 1, at its own width and without counts
            alone = entry(lib, A[b:b + 1, :cA[b]], cA[b:b + 1], B[b:b + 1, :cB[b]], cB[b:b + 1], f, Gab[b:b + 1], Gba[b:b + 1], counts=False)
            for k in keys[:3]:
                assert same(alone[k][:, 0], first[k][:, b]), (k, b)
            assert same(alone["dA"][0], first["dA"][b, :cA[b]]) and same(alone["dB"][0], first["dB"][b, :cB[b]]), b


def test_full_counts_equal_no_counts(lib):
    A, B, cA, cB = PC.chamfer_make("full")
    Gab, Gba = entry_upstreams("full", "all")
    for f in (0, 1):
        x, y = batch("full", f, "all"), entry(lib, A, cA, B, cB, f, Gab, Gba, counts=False)
        for k in x:
            assert same(x[k], y[k]), k


def test_skipped_routes(lib):
    """dA or dB NULL at the entry, or a set without requires_grad at the module: nothing for that side, the other side's bits unchanged"""
    from dpdist_amd import ChamferPairs
    A, B, cA, cB = PC.chamfer_make("chunks")
    Gab, Gba = entry_upstreams("chunks", "all")
    ups = PC.chamfer_upstreams("chunks")
    for fname, f, _ in FORMS:
        both = batch("chunks", f, "all")
        only_a = entry(lib, A, cA, B, cB, f, Gab, Gba, sides=(True, False))
        only_b = entry(lib, A, cA, B, cB, f, Gab, Gba, sides=(False, True))
        assert only_a["dB"] is None and only_b["dA"] is None and same(only_a["dA"], both["dA"]) and same(only_b["dB"], both["dB"])
        out, gA, none_b = module_grads(ChamferPairs(fname), A, cA, B, cB, ups, True, False)
        out2, none_a, gB = module_grads(ChamferPairs(fname), A, cA, B, cB, ups, False, True)
        assert none_a is None and none_b is None and same(gA, both["dA"]) and same(gB, both["dB"])
        assert all(same(x, y) for x, y in zip(out, out2))


def test_refusals_leave_the_outputs_untouched(lib):
    from dpdist_amd import lib as L
    x = torch.zeros(2, 8, 3, device=DEV)
    out, check = G.banded_flat(2 * 8 * 3, device=DEV)
    arg, check_arg = G.banded_flat(2 * 8, dtype=torch.int32, device=DEV)
    p, s = L.ptr, L.cur_stream()
    fwd = lambda Wa, P, mn=out: lib.dpd_chamfer_pairs_fwd(p(x), None, Wa, p(x), None, 8, P, p(mn), p(arg), p(out), p(arg), p(out), p(out), p(out), s)   # noqa: E731
    bwd = lambda Wa, P, form, g=x: lib.dpd_chamfer_pairs_bwd(p(x), None, Wa, p(x), None, 8, P, form, p(arg), p(arg), p(g), p(g), p(out), p(out), s)   # noqa: E731
    assert fwd(8, 0) == -2 and fwd(4097, 2) == -3 and fwd(0, 2) == -3 and fwd(8, 2, None) == -1
    assert bwd(8, 0, 0) == -2 and bwd(8, 2, 2) == -2 and bwd(4097, 2, 0) == -3 and bwd(8, 2, 0, None) == -1
    torch.cuda.synchronize()
    check(), check_arg()
    assert G.untouched(out) and bool((arg == arg[0]).all())

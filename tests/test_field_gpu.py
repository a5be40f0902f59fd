"""Per-point DPDist field (dpd_field_index + dpd_field_gather + dpd_decoder_fwd_field, dpdist_amd.field.dpdist_field / DPDistField).

Every cloud of a chunk against T queries of its own (or of one shared set): the index is taken per cloud and layer 1 runs over the sum of
the clouds' occupied voxels.  Data movement is a bit-for-bit statement against the plain gather on the same rows, the decoder against
dpd_decoder_fwd on those rows, the field and its gradients against the float64 oracle of tests/field_cases.py.  Every output of an entry
sits in a NaN-filled guard-banded buffer (tests/gemm_cases.py).
"""
import functools

import numpy as np
import pytest
import torch

from tests import field_cases as FC
from tests import gemm_cases as G
from tests import pairs_cases as PC
from tests import ragged_cases as RC
from tests import test_cross_gpu as X

pytestmark = pytest.mark.gpu

M_GRID, K_WIN, H_DEC, KP, KW, NG = FC.M_GRID, FC.K_WIN, FC.H_DEC, FC.KP, FC.KW, FC.NG
CASES = [c[0] for c in FC.ENTRY_CASES]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible")
    from dpdist_amd import lib
    lib.load()
    return torch.device("cuda:0")


_bits = X._bits


def _cu(t, dev, grad=False):
    return torch.tensor(np.ascontiguousarray(t), device=dev).requires_grad_(grad)


class _Field:
    """dpd_field_index + dpd_field_gather of one entry case into guard-banded buffers, next to the plain gather on the same rows"""

    def __init__(self, name, shared, integer):
        from dpdist_amd import lib as L
        lib, s = L.load(), L.cur_stream()
        dev = torch.device("cuda:0")
        _, n, T, _, qcounts, t0 = next(c for c in FC.ENTRY_CASES if c[0] == name)
        self.n, self.T, self.t0, self.qcounts, self.shared = n, T, t0, qcounts, shared
        self.rows = rows = n * T
        self.rows_p = rows_p = (rows + 31) // 32 * 32
        self.cap = cap = lib.dpd_field_slot_capacity(n, T, M_GRID)
        assert cap == (n * min(NG, T) + 31) // 32 * 32 and lib.dpd_padded_width(K_WIN) == KP
        f32, i32 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int32, device=dev)
        q_all = FC.entry_queries(name)                                   # [n, M, 3]
        M = q_all.shape[1]
        assert t0 + T <= M
        self.q_all = torch.tensor(q_all[0] if shared else q_all, device=dev)
        q = self.q_all[t0:] if shared else self.q_all[:, t0:]
        stride = 0 if shared else 3 * M
        # the chunk's queries as a tensor of their own [n, T, 3], for the plain gather and the numpy references
        self.q_chunk = (q[None, :T].expand(n, -1, -1) if shared else q[:, :T]).contiguous()
        fv = G.small_int(np.random.default_rng(9), (n, NG, 20), KP).astype(np.float32) if integer else X._fv(n)
        self.fv = torch.tensor(fv, device=dev)
        self.qc = None if qcounts is None else torch.tensor(qcounts, **i32)
        self.mask, self.mask_band = G.banded_flat(rows, **f32)
        self.vox, self.vox_band = G.banded_flat(rows, **i32)
        self.slot, self.slot_band = G.banded_flat(n * NG, **i32)
        self.ucount, self.ucount_band = G.banded_flat(n, **i32)
        self.Xu, self.Xu_band = G.banded((KW, cap), cap, **f32)                  # k-major: [column of X, slot]
        self.Xt, self.Xt_band = G.banded((rows_p, 32), 32, **f32)
        self.uid, self.uid_band = G.banded_flat(rows_p, **i32)
        self.maskr, self.maskr_band = G.banded_flat(rows_p, **f32)
        self.cnt, self.cnt_band = G.banded_flat(4, **i32)
        L.check(lib.dpd_field_index(L.ptr(q), stride, L.ptr(self.qc), t0, n, T, M_GRID, L.ptr(self.mask), L.ptr(self.vox), L.ptr(self.slot),
                                    L.ptr(self.ucount), s), "dpd_field_index")
        L.check(lib.dpd_field_gather(L.ptr(q), stride, L.ptr(self.vox), L.ptr(self.mask), L.ptr(self.slot), L.ptr(self.ucount), L.ptr(self.fv),
                                     n, T, M_GRID, K_WIN, KP, L.ptr(self.Xu), cap, L.ptr(self.Xt), L.ptr(self.uid), L.ptr(self.maskr),
                                     L.ptr(self.cnt), s), "dpd_field_gather")
        # the plain gather on the same rows (every query taken as real)
        self.X_ref = torch.empty(rows, KP, **f32)
        self.mask_ref, self.vox_ref = torch.empty(rows, **f32), torch.empty(rows, **i32)
        L.check(lib.dpd_patch_rows_fwd(L.ptr(self.q_chunk), L.ptr(self.fv), n, T, M_GRID, K_WIN, KP, L.ptr(self.X_ref), L.ptr(self.mask_ref),
                                       L.ptr(self.vox_ref), None, s), "dpd_patch_rows_fwd")
        # a masked query of voxel 0 per cloud: the window a padded query shares
        out = torch.tensor([[[-1.0, 0.0, 0.0]]], **f32).expand(n, 1, 3).contiguous()
        self.X_out = torch.empty(n, KP, **f32)
        L.check(lib.dpd_patch_rows_fwd(L.ptr(out), L.ptr(self.fv), n, 1, M_GRID, K_WIN, KP, L.ptr(self.X_out), L.ptr(torch.empty(n, **f32)),
                                       L.ptr(torch.empty(n, **i32)), None, s), "dpd_patch_rows_fwd")
        torch.cuda.synchronize()
        # real[c, t]: row (c, t) is no padding
        real = np.ones((n, T), dtype=bool)
        if qcounts is not None:
            for c, k in enumerate(qcounts):
                real[c, max(0, k - t0):] = False
        self.real = real
        # the plain rows with every padded row replaced by what the contract states for it: voxel 0's window, q - centre of voxel 0
        self.X_want = self.X_ref.clone().view(n, T, KP)
        cen0 = np.float32(X._centres()[0])
        for c in range(n):
            pad = torch.tensor(~real[c], device=dev)
            if bool(pad.any()):
                rows_c = self.X_out[c].expand(int(pad.sum()), KP).clone()
                rows_c[:, FC.E:FC.E + 3] = torch.tensor(self.q_chunk[c].cpu().numpy()[~real[c]] - cen0, device=dev)
                self.X_want[c, pad] = rows_c
        self.X_want = self.X_want.view(rows, KP)
        self.U = [int(u) for u in self.ucount.cpu()]

    def bands(self):
        for b in (self.mask_band, self.vox_band, self.slot_band, self.ucount_band, self.Xu_band, self.Xt_band, self.uid_band, self.maskr_band,
                  self.cnt_band):
            b()


@functools.lru_cache(maxsize=None)
def _field(name, shared, integer):
    """one index + gather per case, shared by the tests that read it (nothing below writes into it)"""
    return _Field(name, shared, integer)


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("name", CASES)
def test_field_index(dev, name, shared):
    """vox, mask bit for bit those of the plain gather on the real queries, mask 0 and voxel 0 on the padded ones; slot_of_vox and ucount
    are np.unique per cloud; guard bands intact"""
    x = _field(name, shared, False)
    n, T = x.n, x.T
    real = torch.tensor(x.real.reshape(-1), device=dev)
    want_mask = torch.where(real, x.mask_ref, torch.zeros_like(x.mask_ref))
    want_vox = torch.where(real, x.vox_ref, torch.zeros_like(x.vox_ref))
    assert torch.equal(_bits(x.mask), _bits(want_mask)) and torch.equal(x.vox, want_vox)
    vox = want_vox.cpu().numpy().reshape(n, T)
    slot = x.slot.cpu().numpy().reshape(n, NG)
    for c in range(n):
        occ = np.unique(vox[c])
        want = np.full(NG, -1, dtype=np.int32)
        want[occ] = np.arange(len(occ))
        assert np.array_equal(slot[c], want) and x.U[c] == len(occ), (name, c)
    if name == "distinct":
        assert x.U == [T] * n
    if name == "capacity":
        assert T > NG and x.U[0] == NG and x.cap == NG                          # every voxel occupied: the capacity binds
    if name == "one_voxel":
        assert x.U == [1] * n
    if name == "tile":
        assert x.real.sum(1).tolist() == [86, 33, 0] and x.U[2] == 1        # a cloud of padded rows only occupies voxel 0
    if name in ("outside", "reference"):
        assert bool((want_mask == 0).any()) and bool((want_mask == 1).any())
    x.bands()


@pytest.mark.parametrize("integer", [True, False])
@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("name", CASES)
def test_field_gather(dev, name, shared, integer):
    """Xu column uid[r] and Xt[r] bit for bit the plain gather's row r; uid = base_c + slot; cnt; pad rows; nothing beyond the live columns"""
    x = _field(name, shared, integer)
    n, T, rows, rows_p = x.n, x.T, x.rows, x.rows_p
    total = sum(x.U)
    assert x.cnt.tolist() == [n, total, 0, 0] and total <= x.cap
    uid = x.uid[:rows].long()
    base = np.concatenate([[0], np.cumsum(x.U)[:-1]])
    vox = torch.where(torch.tensor(x.real.reshape(-1), device=dev), x.vox_ref, torch.zeros_like(x.vox_ref)).view(n, T)
    slot = x.slot.view(n, NG)
    for c in range(n):
        want = int(base[c]) + slot[c][vox[c].long()]
        assert torch.equal(x.uid[c * T:(c + 1) * T], want.to(torch.int32)), (name, c)
        assert int(want.min()) >= base[c] and int(want.max()) < base[c] + x.U[c]
    assert torch.equal(_bits(x.Xu.t()[uid]), _bits(x.X_want[:, :KW]))
    assert torch.equal(_bits(x.Xt[:rows]), _bits(x.X_want[:, KW:]))
    assert torch.equal(_bits(x.maskr[:rows]), _bits(x.mask))
    assert not _bits(x.Xt[rows:]).any() and not x.uid[rows:].any() and not _bits(x.maskr[rows:]).any()
    assert G.untouched(x.Xu[:, total:]) and not bool(torch.isnan(x.Xu[:, :total]).any())
    x.bands()


@pytest.mark.parametrize("name", ["reference", "smallest"])
def test_decoder_fwd_field_is_bitwise_the_plain_decoder(dev, name):
    """y and pred of dpd_decoder_fwd_field equal dpd_decoder_fwd's on the plain rows.  The plain rows are handed to dpd_decoder_fwd with the
    zero pad rows the field's own buffers have (rows_p of them): below 4 rows dpd_decoder_fwd leaves its default GEMM kernels for the
    register-staged fallback, whose summation order is another (measured at the single row of `smallest`: y1 = 36.7503 there against
    36.7504 on the default kernels), so the statement is about the default kernels, which every row of a call of 4 rows or more gets."""
    from dpdist_amd import lib as L
    lib, s = L.load(), L.cur_stream()
    x = _field(name, False, False)
    P = X._params(dev)
    cp = P.cparams()
    f32 = dict(dtype=torch.float32, device=dev)
    rows, rows_p, H = x.rows, x.rows_p, H_DEC
    Pu, a0, a1 = torch.empty(x.cap, H, **f32), torch.empty(rows_p, H, **f32), torch.empty(rows_p, H, **f32)
    y, y_band = G.banded((rows_p, 3), 3, **f32)
    pred, pred_band = G.banded((rows_p, 3), 3, **f32)
    L.check(lib.dpd_decoder_fwd_field(L.ptr(x.Xu), x.cap, x.cap, L.ptr(x.Xt), L.ptr(x.uid), L.ptr(x.cnt), L.ptr(Pu), L.ptr(x.maskr), rows, KP, H,
                                      cp, L.ptr(a0), L.ptr(a1), L.ptr(y), L.ptr(pred), s), "dpd_decoder_fwd_field")
    X_plain, mask_plain = torch.zeros(rows_p, KP, **f32), torch.zeros(rows_p, **f32)
    X_plain[:rows], mask_plain[:rows] = x.X_want, x.mask
    h = [torch.empty(rows_p, H, **f32) for _ in range(3)]
    y_ref, pred_ref = torch.empty(rows_p, 3, **f32), torch.empty(rows_p, 3, **f32)
    L.check(lib.dpd_decoder_fwd(L.ptr(X_plain), L.ptr(mask_plain), rows_p, KP, H, cp, 0, L.ptr(h[0]), L.ptr(h[1]), L.ptr(h[2]),
                                L.ptr(y_ref), L.ptr(pred_ref), None, 0, None, s), "dpd_decoder_fwd")
    torch.cuda.synchronize()
    assert torch.equal(y[:rows], y_ref[:rows]) and torch.equal(pred, pred_ref)      # (y of a pad row continues slot 0: not compared)
    assert float(y_ref[:rows].abs().max()) > 0 and (name == "smallest" or float(pred_ref.max()) > 0) and not pred[rows:].any()
    y_band()
    pred_band()
    x.bands()


def _inputs(dev, shared, pad=None, grad=(False, False)):
    S, Q = FC.surfaces(), FC.queries()
    if pad is not None:
        S, Q = RC.with_padding(S, FC.COUNTS, pad), RC.with_padding(Q, FC.QCOUNTS, pad)
    return _cu(S, dev, grad[0]), _cu(Q[0] if shared else Q, dev, grad[1])


@pytest.mark.parametrize("shared", [False, True])
def test_field_against_the_oracle(dev, shared):
    """pred within 1e-4 absolute of the float64 oracle composed per cloud on the truncated clouds (the oracle's own float32 run leaves
    2.6e-6); the mask is the oracle's; counts as a list, a CPU tensor and a device tensor are the same call; DPDistField gives the same bits"""
    from dpdist_amd import DPDistField, dpdist_field
    P = X._params(dev)
    s, q = _inputs(dev, shared)
    pred, mask = dpdist_field(P, s, q, counts=FC.COUNTS, query_counts=list(FC.QCOUNTS), return_mask=True)
    want, want_mask = FC.oracle(torch.float64, shared)
    err = float(np.abs(pred.double().cpu().numpy() - want).max())
    print("shared %s: pred vs the composed float64 oracle: %.3e" % (shared, err))
    assert pred.shape == (3, FC.T_REF, 3) and mask.shape == (3, FC.T_REF) and err <= FC.FWD_BAR
    assert np.array_equal(mask.cpu().numpy(), want_mask)
    for c, k in enumerate(FC.QCOUNTS):
        assert not _bits(pred[c, k:]).any() and not _bits(mask[c, k:]).any()
    on_dev = dpdist_field(P, s, q, RC.counts_dev(FC.COUNTS, dev), RC.counts_dev(FC.QCOUNTS, dev))
    cpu = dpdist_field(P, s, q, torch.tensor(FC.COUNTS), torch.tensor(FC.QCOUNTS, dtype=torch.int64))
    mod = DPDistField(P)(s, q, counts=FC.COUNTS, query_counts=FC.QCOUNTS)
    assert all(torch.equal(_bits(t), _bits(pred)) for t in (on_dev, cpu, mod))


def test_chunking_and_padding_change_no_bit(dev):
    """max_rows in {4096, 150, 64, 1} (whole clouds; one cloud per chunk; tiles of 64 queries; one row per chunk) and the padding values of
    tests/ragged_cases.py: the same bits; pred and mask 0 at the padded queries"""
    from dpdist_amd import dpdist_field
    P = X._params(dev)
    for shared in (False, True):
        s, q = _inputs(dev, shared, 0.0)
        ref = dpdist_field(P, s, q, FC.COUNTS, FC.QCOUNTS, return_mask=True, max_rows=4096)
        for max_rows, pad in ((150, 0.37), (64, 5.0), (1, 0.37)):
            s, q = _inputs(dev, shared, pad)
            got = dpdist_field(P, s, q, FC.COUNTS, FC.QCOUNTS, return_mask=True, max_rows=max_rows)
            assert torch.equal(_bits(got[0]), _bits(ref[0])) and torch.equal(_bits(got[1]), _bits(ref[1])), (shared, max_rows, pad)
        for c, k in enumerate(FC.QCOUNTS):
            assert not ref[0][c, k:].any() and not ref[1][c, k:].any()
        assert float(ref[0].max()) == 2.0 and float(ref[0][:, :, 0].max()) > 0


def test_pairs_are_the_means_of_the_field(dev):
    """D_AB[b] of dpdist_pairs against the float64 mean of the field of surface A_b at the real queries of B_b"""
    from dpdist_amd import dpdist_field, dpdist_pairs
    P = X._params(dev)
    A, B = (_cu(t, dev) for t in PC.sets())
    d_ab = dpdist_pairs(P, A, B, PC.COUNTS_A, PC.COUNTS_B, return_directed=True)[1]
    pred = dpdist_field(P, A, B, PC.COUNTS_A, PC.COUNTS_B)
    for b, k in enumerate(PC.COUNTS_B):
        want = float(pred[b, :k, 0].double().mean())
        print("pair %d: D_AB %.6f, mean of the field %.6f" % (b, float(d_ab[b]), want))
        assert abs(float(d_ab[b]) - want) <= PC.DD_BAR
    assert float(d_ab.max()) > 0.1


def _grads(dev, shared, max_rows=4096, need=(True, True), pad=None):
    from dpdist_amd import DPDistField
    s, q = _inputs(dev, shared, pad, need)
    pred = DPDistField(X._params(dev), max_rows=max_rows)(s, q, counts=FC.COUNTS, query_counts=FC.QCOUNTS)
    loss = (pred * _cu(FC.upstream(), dev)).sum()
    g = iter(torch.autograd.grad(loss, [t for t, w in zip((s, q), need) if w]))
    return pred, [next(g) if w else None for w in need]


@pytest.mark.parametrize("shared", [False, True])
def test_gradients_against_the_oracle(dev, shared):
    """gradients of (upstream * pred).sum() w.r.t. surfaces and queries against float64 autograd through the composed oracle, bars formed
    as tests/ragged_cases.py forms them; 0 on the padding; max_rows in {4096, 150} give the same bits; an input that needs no gradient
    changes nothing for the other"""
    pred, (gS, gQ) = _grads(dev, shared)
    for name, got, (ref, bar) in zip(("surfaces", "queries"), (gS, gQ), FC.grad_bars(shared)):
        err = np.abs(got.double().cpu().numpy() - ref).max()
        print("shared %s: g %s vs the composed float64 oracle: %.3e (bar %.3e, max|ref| %.3e)" % (shared, name, err, bar, np.abs(ref).max()))
        assert np.abs(ref).max() > 20 * bar, "a reference gradient without structure makes the bar vacuous"
        assert got.shape == ref.shape and err <= bar, name
    for c, k in enumerate(FC.COUNTS):
        assert not gS[c, k:].any() and float(gS[c, :k].abs().max()) > 0
    if not shared:
        for c, k in enumerate(FC.QCOUNTS):
            assert not gQ[c, k:].any()
        assert not gQ[:, 8].any()
    pred2, (gS2, gQ2) = _grads(dev, shared, max_rows=150, pad=5.0)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in ((pred, pred2), (gS, gS2), (gQ, gQ2)))
    _, (gS3, none_q) = _grads(dev, shared, need=(True, False))
    _, (none_s, gQ3) = _grads(dev, shared, need=(False, True))
    assert none_q is None and none_s is None and torch.equal(_bits(gS3), _bits(gS)) and torch.equal(_bits(gQ3), _bits(gQ))


def test_backward_takes_whole_clouds(dev):
    from dpdist_amd import DPDistField
    s, q = _inputs(dev, False, grad=(True, True))
    mod = DPDistField(X._params(dev), max_rows=149)
    with pytest.raises(ValueError, match="max_rows"):
        mod(s, q)
    assert mod(s.detach(), q.detach()).shape == (3, FC.T_REF, 3)      # the forward has no such limit


def test_errors_before_any_launch(dev):
    from dpdist_amd import DPDistField, dpdist_field
    P = X._params(dev)
    s, q = _inputs(dev, False)
    with pytest.raises(ValueError, match="GPU"):
        dpdist_field(P, s.cpu(), q)
    with pytest.raises(ValueError, match="GPU"):
        dpdist_field(P, s, q.cpu())
    with pytest.raises(ValueError, match="one set per cloud"):
        dpdist_field(P, s, q[:2].contiguous())
    with pytest.raises(ValueError, match="must be a"):
        dpdist_field(P, s, q[..., :2].contiguous())
    with pytest.raises(ValueError, match="counts must lie"):
        dpdist_field(P, s, q, counts=(64, 65, 5))
    with pytest.raises(ValueError, match="query_counts must lie"):
        dpdist_field(P, s, q, query_counts=(150, 0, 1))
    with pytest.raises(ValueError, match="one count per cloud"):
        DPDistField(P)(s, q, query_counts=(150, 97))
    with pytest.raises(ValueError, match="fp32"):
        dpdist_field(X._params(dev, compute_dtype="bf16"), s, q)
    with pytest.raises(ValueError, match="float32"):
        dpdist_field(P, s, q.double())
    with pytest.raises(ValueError, match="max_rows"):
        dpdist_field(P, s, q, max_rows=0)
    with pytest.raises(ValueError, match="not supported"):
        dpdist_field(P, torch.zeros(1, 4097, 3, device=dev), q[:1].contiguous())

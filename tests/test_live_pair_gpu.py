"""Pair launches of the live-row backward (gemm_rs_pair_kernel: dpd_gemm_f32_pair, dpd_decoder_bwd_pair_live,
dpd_decoder_bwd_chain_live, trainer option `live_pair`).

A pair launch runs a live dH product and the weight gradient that does not wait for it as two parts of one grid.  Each part is the wave
body of its own launch over the same operands in the same k order, so every statement here is a statement about BITS: the pair entry
against the two separate live launches, the chain entry against the five-launch live form (and, up to the sign of a zero, the dense
entries), the trainer with the option on against off.  Operands are random floats (an order change is invisible to integers); every
output sits in a NaN-filled guard-banded buffer (tests/gemm_cases.py), so a workgroup that runs the wrong part or the wrong tile shows.
Shapes: Qb in {64, 128, 256} x H in {64, 192, 256} -- the dH part has 1 .. 16 workgroup tiles of 64x64 at the capacity (fewer live),
the dW part 1, 9 and 16: neither count is a multiple of the 8 XCDs in some case.
"""
import functools

import numpy as np
import pytest
import torch

from dpdist_amd import synth
from tests import gemm_cases as G
from tests.test_live_rows_gpu import _bits, _eq, restate

pytestmark = pytest.mark.gpu

KP = 96            # layer-1 width of the chain cases: two 64-row workgroup tiles of dW1, the second one ragged
QBS, HS = (64, 128, 256), (64, 192, 256)
KINDS = ("none", "one", "L31", "L32", "L33", "quarter", "all", "flag_and_dy")
TILES = (33, 32)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible")
    from dpdist_amd import lib
    lib.load()
    return torch.device("cuda:0")


def _pattern(kind, Qb):
    """rows whose dy is not zero, and the clouds (of 2 * Qb / 32 clouds of 32 rows) whose encoder sums are NaN"""
    rng = np.random.default_rng([Qb, len(kind), ord(kind[-1])])
    live, nan_clouds = np.zeros(Qb, dtype=bool), ()
    if kind == "all":
        live[:] = True
    elif kind == "one":
        live[37] = True
    elif kind in ("L31", "L32", "L33"):
        live[rng.permutation(Qb)[:int(kind[1:])]] = True
    elif kind == "quarter":
        live[rng.permutation(Qb)[:Qb // 4 + 5]] = True
    elif kind == "flag_and_dy":
        live[rng.permutation(Qb)[:9]] = True
        nan_clouds = (Qb // 32 - 1,)
    else:
        assert kind == "none"
    return live, nan_clouds


class _Ops:
    """Random-float operands of one backward behind the output layer at (Qb, H); dead rows have dpred = 0 exactly."""
    ROWS = 32      # rows per cloud

    def __init__(self, dev, Qb, H, kind):
        from dpdist_amd import lib as L
        self.dev, self.Qb, self.H, self.C = dev, Qb, H, 2 * Qb // self.ROWS
        want, self.nan_clouds = _pattern(kind, Qb)
        rng = np.random.default_rng([7, Qb, H])
        t = lambda a: torch.tensor(np.ascontiguousarray(a, dtype=np.float32), device=dev)      # noqa: E731
        relu = lambda *s: np.maximum(rng.standard_normal(s), 0.0)                              # noqa: E731
        self.X, self.h1, self.h2, self.h3 = t(rng.standard_normal((Qb, KP)) * 0.5), t(relu(Qb, H)), t(relu(Qb, H)), t(relu(Qb, H))
        self.y, self.mask = t(rng.uniform(0.5, 5.5, size=(Qb, 3))), torch.ones(Qb, device=dev)
        dpred = rng.standard_normal((Qb, 3))
        dpred[np.abs(dpred) < 1e-3] = 0.5
        self.dpred = t(dpred * want[:, None])
        w = [rng.standard_normal(s) * 0.05 for s in ((KP, H), (H,), (H, H), (H,), (H, H), (H,), (H, 3), (3,))]
        self.w = [t(x) for x in w] + [t(w[2].T), t(w[4].T)]
        self.params = L.make_params(*self.w, None)
        ssq = np.abs(rng.standard_normal((self.C, 4, 20))) + 0.1
        for c in self.nan_clouds:
            ssq[c, 2, 7] = np.nan
        self.ssq = t(ssq)
        self.ws = torch.empty(L.load().dpd_workspace_bytes(2 * Qb, KP, H, 0) // 4 + 1, device=dev)
        self.part = torch.empty(((Qb + 7) // 8) * (4 * H + 8), device=dev)
        self.live = want.copy()
        for c in self.nan_clouds:
            r0 = (c % (self.C // 2)) * self.ROWS
            self.live[r0:r0 + self.ROWS] = True

    def descriptor(self):
        from dpdist_amd import lib as L
        lib = L.load()
        nbytes = lib.dpd_live_rows_bytes(self.Qb, KP, self.H)
        mem, band = G.banded_flat(nbytes // 4, device=self.dev)
        lv = L.LiveRows()
        L.check(lib.dpd_live_rows_carve(L.ptr(mem), nbytes, self.Qb, KP, self.H, lv), "dpd_live_rows_carve")
        lv.X, lv.ldx = self.X.data_ptr(), KP
        lv.ssq, lv.clouds, lv.rows_per_cloud = self.ssq.data_ptr(), self.C, self.ROWS
        cnt = mem[(lv.cnt - mem.data_ptr()) // 4:][:4].view(torch.int32)
        return lv, cnt, band

    def buffers(self):
        """every output of a backward, NaN-filled and guard-banded; returns (dict, check of all bands)"""
        Qb, H, out, bands = self.Qb, self.H, {}, []
        for name, shape in (("dy", (Qb, 3)), ("g3", (Qb, H)), ("g2", (Qb, H)), ("g1", (Qb, H)), ("dW1", (KP, H)), ("dW2", (H, H)),
                            ("dW3", (H, H)), ("db1", (1, H)), ("db2", (1, H)), ("db3", (1, H)), ("dW4", (H, 3)), ("db4", (1, 3)),
                            ("dbp", (2 * (Qb // 32), H))):
            out[name], b = G.banded(shape, shape[1], device=self.dev)
            bands.append(b)
        return out, lambda: [b() for b in bands]

    def data(self, o, lv, phases, partials=True):
        from dpdist_amd import lib as L
        sg = L.make_small_grads(None, None, o["db3"], o["dW4"], o["db4"], self.part, db_partials=o["dbp"] if partials else None)
        L.check(L.load().dpd_decoder_bwd_data_live(L.ptr(self.dpred), L.ptr(self.mask), L.ptr(self.y), L.ptr(self.h1), L.ptr(self.h2),
                                                   L.ptr(self.h3), self.Qb, KP, self.H, self.params, 0, L.ptr(o["dy"]), L.ptr(o["g3"]),
                                                   L.ptr(o["g2"]), L.ptr(o["g1"]), None, sg, L.ptr(self.ws), self.ws.numel() * 4, None, phases,
                                                   lv, L.cur_stream()), "dpd_decoder_bwd_data_live(%d)" % phases)

    def weights(self, o, lv, layer, db=None):
        from dpdist_amd import lib as L
        act, g, kin = {1: (self.X, o["g1"], KP), 2: (self.h1, o["g2"], self.H), 3: (self.h2, o["g3"], self.H)}[layer]
        L.check(L.load().dpd_decoder_bwd_weights_live(layer, L.ptr(act), kin, L.ptr(g), self.Qb, kin, self.H, 0, L.ptr(o["dW%d" % layer]),
                                                      L.ptr(db), L.ptr(self.ws), self.ws.numel() * 4, None, L.ptr(o["dbp"]) if db is not None else None,
                                                      lv, L.cur_stream()), "dpd_decoder_bwd_weights_live(%d)" % layer)

    def five(self, lv):
        """the five-launch form behind the output layer: data chain, dW1 (+ db1), dW2 + dW3 grouped (+ db2); lv = None: the dense form"""
        from dpdist_amd import lib as L
        o, check = self.buffers()
        self.data(o, lv, 7)
        self.weights(o, lv, 1, o["db1"])
        L.check(L.load().dpd_decoder_bwd_weights_pair_live(L.ptr(self.h1), L.ptr(o["g2"]), L.ptr(o["dW2"]), L.ptr(self.h2), L.ptr(o["g3"]),
                                                           L.ptr(o["dW3"]), self.H, self.Qb, self.H, self.H, 0, L.ptr(self.ws), self.ws.numel() * 4,
                                                           None, L.ptr(o["db2"]), L.ptr(o["dbp"]), lv, L.cur_stream()), "dpd_decoder_bwd_weights_pair_live")
        torch.cuda.synchronize()
        check()
        return o


@functools.lru_cache(maxsize=None)
def _ops(dev, Qb, H, kind):
    return _Ops(dev, Qb, H, kind)


@functools.lru_cache(maxsize=None)
def _reference(dev, Qb, H, kind):
    """computed once per case at the default tiles (both tiles give the same bits: tests/test_live_rows_gpu.py) and left unchanged:
    the five-launch live form and the dense form"""
    ops = _ops(dev, Qb, H, kind)
    lv, cnt, band = ops.descriptor()
    live5 = ops.five(lv)
    band()
    return live5, ops.five(None), cnt.cpu().tolist()


class _plan:
    """tiles of the live dH part (op 9), of the separate dW launches (10, 11) and of the pair's dW part (12) for the time of a case"""

    def __init__(self, tile):
        self.tile = tile

    def __enter__(self):
        from dpdist_amd import lib as L
        for op in (9, 10, 11, 12):
            assert L.load().dpd_set_gemm_plan(op, self.tile, 1) == 0

    def __exit__(self, *exc):
        from dpdist_amd import lib as L
        for op in (9, 10, 11, 12):
            assert L.load().dpd_set_gemm_plan(op, 33, 1) == 0


# ------------------------------------------------------------------------------------------------ 1. the pair entry
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("H", HS)
@pytest.mark.parametrize("Qb", QBS)
def test_pair_entry_equals_the_two_separate_live_launches(dev, Qb, H, kind, tile):
    """{g2 | dW3} and {g1 | dW2} as pair launches against phase 2, dW3, phase 4, dW2 as launches of their own, behind the same
    compaction: the same bits in every element, rows from Lp on untouched, guard bands intact.  none: every dH workgroup leaves and the
    dW part stores zero tiles; one / L31 / L32: one ragged row tile; L33: a padded second K-tile; all: the capacity."""
    from dpdist_amd import lib as L
    lib, ops = L.load(), _ops(dev, Qb, H, kind)
    lv, cnt, band = ops.descriptor()
    sep, check_sep = ops.buffers()
    pair, check_pair = ops.buffers()
    with _plan(tile):
        ops.data(sep, lv, 1)
        ops.data(sep, lv, 2, partials=False)
        ops.weights(sep, lv, 3)
        ops.data(sep, lv, 4, partials=False)
        ops.weights(sep, lv, 2)
        L.check(lib.dpd_decoder_bwd_pair_live(3, None, L.ptr(pair["g2"]), L.ptr(pair["dW3"]), Qb, H, ops.params, lv, L.cur_stream()), "pair(3)")
        L.check(lib.dpd_decoder_bwd_pair_live(2, L.ptr(pair["g2"]), L.ptr(pair["g1"]), L.ptr(pair["dW2"]), Qb, H, ops.params, lv, L.cur_stream()),
                "pair(2)")
        torch.cuda.synchronize()
    check_sep(), check_pair(), band()
    L_, Lp, idx, pos = restate(ops.live)
    assert cnt.cpu().tolist() == [L_, Lp, 0, 0]
    for name in ("g2", "g1", "dW3", "dW2"):
        assert torch.equal(_bits(pair[name]), _bits(sep[name])), name
    for name in ("g2", "g1"):
        assert G.untouched(pair[name][Lp:]), name
        assert not torch.isnan(pair[name][:Lp]).any() or kind == "flag_and_dy", name
    if kind == "none":
        assert not _bits(pair["dW3"]).any() and not _bits(pair["dW2"]).any()      # zero tiles, stored
    else:
        assert pair["dW3"].any() and pair["g2"][:Lp].any()


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("L_dev", [0, 33, 64])
def test_pair_gemm_bias_epilogue_runs_whatever_the_live_count(dev, L_dev, tile):
    """dpd_gemm_f32_pair with the second step of a bias gradient in its TN part: the block-order sum of the partials is stored whatever
    the device words say (0: every dH workgroup leaves, the dW part stores zeros and still finishes the bias)."""
    from dpdist_amd import lib as L
    lib, M, H, nparts = L.load(), 64, 192, 5
    rng = np.random.default_rng(L_dev)
    t = lambda a: torch.tensor(np.ascontiguousarray(a, dtype=np.float32), device=dev)      # noqa: E731
    A, W, act, parts = t(rng.standard_normal((M, H))), t(rng.standard_normal((H, H))), t(rng.standard_normal((M, H))), t(rng.standard_normal((nparts, H)))
    Lp = (L_dev + 31) // 32 * 32
    word = torch.tensor([Lp], dtype=torch.int32, device=dev)
    (C, bC), (D, bD), (bias, bB) = G.banded((M, H), H, device=dev), G.banded((H, H), H, device=dev), G.banded((1, H), H, device=dev)
    a, b = L.GemmPairPart(), L.GemmPairPart()
    a.transA, a.transB, a.M, a.N, a.K = 0, 0, M, H, H
    a.A, a.lda, a.B, a.ldb, a.C, a.ldc, a.gate = A.data_ptr(), H, W.data_ptr(), H, C.data_ptr(), H, act.data_ptr()
    a.epilogue, a.split_k, a.tile, a.M_dev = 3, 1, tile, word.data_ptr()
    b.transA, b.transB, b.M, b.N, b.K = 1, 0, H, H, M
    b.A, b.lda, b.B, b.ldb, b.C, b.ldc = act.data_ptr(), H, A.data_ptr(), H, D.data_ptr(), H
    b.epilogue, b.split_k, b.tile, b.K_dev = 0, 1, tile, word.data_ptr()
    b.bias_parts, b.bias_out, b.bias_nparts = parts.data_ptr(), bias.data_ptr(), nparts
    L.check(lib.dpd_gemm_f32_pair(a, b, L.cur_stream()), "dpd_gemm_f32_pair")
    torch.cuda.synchronize()
    bC(), bD(), bB()
    want = torch.zeros(H, device=dev)
    for p in range(nparts):          # the kernel's order: 0 + p0 + p1 + ...
        want = want + parts[p]
    assert torch.equal(_bits(bias[0]), _bits(want))
    assert G.untouched(C[Lp:])
    if L_dev == 0:
        assert not _bits(D).any()
    else:      # exact fp32 chains in another order than torch's: loose value check only (the bits are test 1's business)
        ref_C = (A[:Lp].double() @ W.double()) * (act[:Lp] > 0)
        ref_D = act[:Lp].double().T @ A[:Lp].double()
        assert (C[:Lp].double() - ref_C).abs().max() <= 1e-4 * ref_C.abs().max()
        assert (D.double() - ref_D).abs().max() <= 1e-4 * ref_D.abs().max()


# ------------------------------------------------------------------------------------------------ 2. the chain entry
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("H", HS)
@pytest.mark.parametrize("Qb", QBS)
def test_chain_entry_equals_the_five_launch_form_and_the_dense_entries(dev, Qb, H, kind, tile):
    """dpd_decoder_bwd_chain_live: g2, g1 (compact rows), dW1, dW2, dW3, db1, db2 and the partial sums have the bits of the five-launch
    live form (db2 is finished by dW1's waves here, by dW2's there: the same block-order sum) and == the dense entries' values."""
    from dpdist_amd import lib as L
    lib, ops = L.load(), _ops(dev, Qb, H, kind)
    live5, dense, cnt5 = _reference(dev, Qb, H, kind)
    lv, cnt, band = ops.descriptor()
    o, check = ops.buffers()
    sg = L.make_small_grads(None, None, o["db3"], o["dW4"], o["db4"], ops.part, db_partials=o["dbp"])
    with _plan(tile):
        L.check(lib.dpd_decoder_bwd_chain_live(L.ptr(ops.dpred), L.ptr(ops.mask), L.ptr(ops.y), L.ptr(ops.h1), L.ptr(ops.h2), L.ptr(ops.h3), Qb, KP, H,
                                               ops.params, L.ptr(o["dy"]), L.ptr(o["g3"]), L.ptr(o["g2"]), L.ptr(o["g1"]), sg, L.ptr(ops.ws),
                                               ops.ws.numel() * 4, 0, L.ptr(o["dW1"]), L.ptr(o["dW2"]), L.ptr(o["dW3"]), L.ptr(o["db1"]),
                                               L.ptr(o["db2"]), lv, L.cur_stream()), "dpd_decoder_bwd_chain_live")
        torch.cuda.synchronize()
    check(), band()
    L_, Lp, idx, pos = restate(ops.live)
    assert cnt.cpu().tolist() == [L_, Lp, 0, 0] == cnt5
    for name in ("dy", "g3", "g2", "g1", "dW1", "dW2", "dW3", "db1", "db2", "dbp"):
        assert torch.equal(_bits(o[name]), _bits(live5[name])), name
    live_pos = torch.tensor(sorted(idx), dtype=torch.long, device=dev)
    rows = torch.tensor([idx[p] for p in sorted(idx)], dtype=torch.long, device=dev)
    for name in ("g2", "g1"):
        assert _eq(o[name][live_pos], dense[name][rows]), name
        assert G.untouched(o[name][Lp:]), name
    for name in ("dW1", "dW2", "dW3", "db1", "db2", "dbp"):
        assert _eq(o[name], dense[name]), name
    if kind == "none":
        assert not o["dW1"].any() and not o["dW2"].any() and not o["dW3"].any() and not o["db1"].any() and not o["db2"].any()
    else:
        assert dense["dW1"].any() and dense["dW3"].any() and dense["db1"].any() and dense["db2"].any()


# ------------------------------------------------------------------------------------------------ 3. trainer
@pytest.mark.parametrize("B", [2, 4])
def test_trainer_with_pair_launches_equals_the_five_launch_trainer(dev, B):
    """five steps, two batches in turn, `live_pair` on against off: loss, pred, the gradient and the parameters bit for bit after every
    step.  (The library keeps no record of its launches, so the launch count -- one less per backward -- is not asserted here.)"""
    from dpdist_amd.model import DPDistParams
    from dpdist_amd.trainer import DPDistTrainer
    cu = lambda a: torch.tensor(a, device=dev)      # noqa: E731
    batches = [tuple(cu(x) for x in synth.s2_modelnet_shaped(B, 64, 100 + i)) for i in range(2)]
    runs = {}
    for on in (True, False):
        P = DPDistParams(device=dev)
        P.load_tf_state_dict(synth.make_weights("wide"))
        tr = DPDistTrainer(P, B, base_lr=1e-4, distributed=False, options={"live_pair": on})
        assert tr.live_rows and tr.live_pair == on
        snaps = []
        for bi in (0, 1, 0, 1, 0):
            tr.step(*batches[bi])
            torch.cuda.synchronize()
            snaps.append({k: getattr(tr, k).clone() for k in ("loss", "pred", "grad")})
            snaps[-1]["params"] = P.flat.detach().clone()
            snaps[-1]["count"] = tr.live_count.clone()
        runs[on] = snaps
    for t, (x, y) in enumerate(zip(runs[True], runs[False])):
        for k in x:
            assert torch.equal(_bits(x[k]), _bits(y[k])), (t, k)
    assert any(int(s["count"][0]) > 0 for s in runs[True])


# ------------------------------------------------------------------------------------------------ 4. argument errors
def test_pair_call_argument_errors_launch_nothing(dev):
    """split-K, a tile that is not register-streamed, a dW part with K < 32, a NULL part or operand: the negative code, and every output
    keeps its fill pattern"""
    from dpdist_amd import lib as L
    lib, M, H = L.load(), 64, 64
    t = lambda *s: torch.ones(*s, device=dev)      # noqa: E731
    A, W, act = t(M, H), t(H, H), t(M, H)
    word = torch.tensor([M], dtype=torch.int32, device=dev)
    (C, bC), (D, bD) = G.banded((M, H), H, device=dev), G.banded((H, H), H, device=dev)
    ws = torch.empty(4 * M * H, device=dev)

    def parts(**kw):
        a, b = L.GemmPairPart(), L.GemmPairPart()
        a.transA, a.transB, a.M, a.N, a.K = 0, 0, M, H, H
        a.A, a.lda, a.B, a.ldb, a.C, a.ldc, a.gate = A.data_ptr(), H, W.data_ptr(), H, C.data_ptr(), H, act.data_ptr()
        a.epilogue, a.split_k, a.tile, a.M_dev = 3, 1, 33, word.data_ptr()
        b.transA, b.transB, b.M, b.N, b.K = 1, 0, H, H, M
        b.A, b.lda, b.B, b.ldb, b.C, b.ldc = act.data_ptr(), H, A.data_ptr(), H, D.data_ptr(), H
        b.epilogue, b.split_k, b.tile, b.K_dev = 0, 1, 33, word.data_ptr()
        for k, v in kw.items():
            setattr(a if k[0] == "a" else b, k[2:], v)
        return a, b
    s = L.cur_stream()
    E_NULL, E_UNSUPPORTED = -1, -3
    assert lib.dpd_gemm_f32_pair(None, parts()[1], s) == E_NULL
    assert lib.dpd_gemm_f32_pair(parts()[0], None, s) == E_NULL
    assert lib.dpd_gemm_f32_pair(*parts(a_A=None), s) == E_NULL
    assert lib.dpd_gemm_f32_pair(*parts(b_C=None), s) == E_NULL
    assert lib.dpd_gemm_f32_pair(*parts(a_gate=None), s) == E_NULL
    for kw in (dict(a_split_k=2), dict(b_split_k=2), dict(a_split_k=0), dict(b_split_k=0),      # split-K, the tail split
               dict(a_tile=8), dict(b_tile=9), dict(a_tile=0), dict(b_tile=3), dict(a_tile=30), dict(b_tile=31),      # other kernels
               dict(b_K=16), dict(b_K=28), dict(b_K=48),                                      # K < 32, K not whole K-tiles
               dict(a_M_dev=None), dict(b_K_dev=None), dict(a_epilogue=0), dict(b_epilogue=3, b_gate=act.data_ptr()),
               dict(a_transB=1), dict(b_transA=0)):
        assert lib.dpd_gemm_f32_pair(*parts(**kw), s) == E_UNSUPPORTED, kw
    torch.cuda.synchronize()
    bC(), bD()
    assert G.untouched(C) and G.untouched(D)
    del ws
    # the entry: a layer it does not have, a descriptor of another shape, missing transposed weights
    ops = _ops(dev, 64, 64, "one")
    lv, cnt, band = ops.descriptor()
    g = torch.zeros(64, 64, device=dev)
    assert lib.dpd_decoder_bwd_pair_live(1, L.ptr(g), L.ptr(g), L.ptr(g), 64, 64, ops.params, lv, s) == -2
    assert lib.dpd_decoder_bwd_pair_live(2, None, L.ptr(g), L.ptr(g), 64, 64, ops.params, lv, s) == E_NULL
    assert lib.dpd_decoder_bwd_pair_live(3, None, L.ptr(g), L.ptr(g), 128, 64, ops.params, lv, s) == -2
    assert lib.dpd_decoder_bwd_pair_live(3, None, L.ptr(g), L.ptr(g), 64, 64, L.make_params(*ops.w[:8]), lv, s) == E_UNSUPPORTED
    band()

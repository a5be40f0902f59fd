"""Live rows of the exact-fp32 backward (dpd_live_rows, the `_live` entries, trainer option `live_rows`).

A row whose dy is zero adds exact zeros to every gradient behind the output layer, so the dH and dW GEMMs run over the other rows
only, compacted to the front of copies of their operands.  The statements here are `==` statements (the sign of a zero is the one
freedom the form has): the index against a numpy restatement of the kernel's visit order, the copies bit for bit, every gradient of
the live entries against the dense entries on the same data, the training step against the same trainer with the option off, and
the NaN pattern of a cloud the encoder turned to NaN.  Operands are random floats (an order change is invisible to integers);
outputs sit in NaN-filled guard-banded buffers (tests/gemm_cases.py).
"""
import functools

import numpy as np
import pytest
import torch

from dpdist_amd import synth
from tests import gemm_cases as G

pytestmark = pytest.mark.gpu

N_PTS, H, KP = 64, 1024, 2528


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible")
    from dpdist_amd import lib
    lib.load()
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------ numpy restatement
def visit_rank(i):
    """gemm_rs_kernel reaches row k = 32 t + 16 half + 4 b + s of a K-tile at step (b, s), half 0 before half 1"""
    return 2 * (i & 15) + (i >> 4)


def position(j):
    """the compact position whose visit rank inside its K-tile is j % 32"""
    return (j & ~31) + 16 * (j & 1) + ((j & 31) >> 1)


def restate(live):
    """live [Qb] bool -> L, Lp, idx {position: row} of the live positions, pos [Qb]"""
    Qb = len(live)
    order = sorted(range(Qb), key=lambda r: (r >> 5, visit_rank(r & 31)))
    rows = [r for r in order if live[r]]
    L = len(rows)
    pos = np.full(Qb, -1, dtype=np.int64)
    idx = {}
    for j, r in enumerate(rows):
        pos[r] = position(j)
        idx[position(j)] = r
    return L, (L + 31) // 32 * 32, idx, pos


def test_restatement_is_a_permutation_of_every_tile():
    assert sorted(visit_rank(i) for i in range(32)) == list(range(32))
    assert sorted(position(j) for j in range(96)) == list(range(96))
    assert all(visit_rank(position(j) & 31) == j & 31 for j in range(64))


# ------------------------------------------------------------------------------------------------ inputs
def _pattern(kind, B):
    """intended liveness from dy, and the clouds whose encoder sums are NaN"""
    Qb = B * N_PTS
    rng = np.random.default_rng([B, len(kind), ord(kind[-1])])
    live, nan_clouds = np.zeros(Qb, dtype=bool), ()
    if kind == "all":
        live[:] = True
    elif kind == "one":
        live[77] = True
    elif kind in ("L31", "L32", "L33"):
        live[rng.permutation(Qb)[:int(kind[1:])]] = True
    elif kind == "one_cloud":
        live[N_PTS:2 * N_PTS] = True
    elif kind == "quarter":
        live[rng.permutation(Qb)[:Qb // 4 + 5]] = True
    elif kind == "flag_fv":          # the cloud whose Fisher vectors rows 0 .. N gather
        nan_clouds = (0,)
    elif kind == "flag_query":       # the cloud the query points of rows N .. 2N belong to
        nan_clouds = (B + 1,)
    elif kind == "flag_and_dy":
        live[rng.permutation(Qb)[:40]] = True
        nan_clouds = (B - 1,)
    else:
        assert kind == "none"
    return live, nan_clouds


class _Chain:
    """Random-float operands of one backward behind the output layer; dead rows have dpred = 0 exactly."""

    def __init__(self, dev, B, kind, use_ssq=True, seed=3):
        from dpdist_amd import lib as L
        self.dev, self.B, self.Qb, self.C = dev, B, B * N_PTS, 2 * B
        Qb = self.Qb
        self.want_live, self.nan_clouds = _pattern(kind, B)
        rng = np.random.default_rng(seed)
        t = lambda a: torch.tensor(np.ascontiguousarray(a, dtype=np.float32), device=dev)      # noqa: E731
        relu = lambda *s: np.maximum(rng.standard_normal(s), 0.0)                              # noqa: E731
        self.X, self.h1, self.h2, self.h3 = t(rng.standard_normal((Qb, KP)) * 0.5), t(relu(Qb, H)), t(relu(Qb, H)), t(relu(Qb, H))
        self.y, self.mask = t(rng.uniform(0.5, 5.5, size=(Qb, 3))), torch.ones(Qb, device=dev)
        dpred = rng.standard_normal((Qb, 3))
        dpred[np.abs(dpred) < 1e-3] = 0.5
        self.dpred = t(dpred * self.want_live[:, None])
        w = [rng.standard_normal(s) * 0.05 for s in ((KP, H), (H,), (H, H), (H,), (H, H), (H,), (H, 3), (3,))]
        self.w = [t(x) for x in w] + [t(w[2].T), t(w[4].T)]
        self.params = L.make_params(*self.w, None)
        ssq = np.abs(rng.standard_normal((self.C, 4, 20))) + 0.1
        for c in self.nan_clouds:
            ssq[c, 2, 7] = np.nan
        self.ssq = t(ssq) if use_ssq else None
        if not use_ssq:      # the same clouds through the rows of X: one non-finite value per row of the flagged clouds
            for c in self.nan_clouds:
                r0 = (c % B) * N_PTS
                self.X[r0:r0 + N_PTS, 2527 - c] = float("inf")
        lib = L.load()
        self.ws = torch.empty(lib.dpd_workspace_bytes(2 * Qb, KP, H, 0) // 4 + 1, device=dev)
        self.live = self.want_live.copy()
        for c in self.nan_clouds:
            r0 = (c % B) * N_PTS
            self.live[r0:r0 + N_PTS] = True

    def descriptor(self):
        from dpdist_amd import lib as L
        lib = L.load()
        nbytes = lib.dpd_live_rows_bytes(self.Qb, KP, H)
        assert nbytes % 256 == 0
        mem, band = G.banded_flat(nbytes // 4, device=self.dev)
        lv = L.LiveRows()
        L.check(lib.dpd_live_rows_carve(L.ptr(mem), nbytes, self.Qb, KP, H, lv), "dpd_live_rows_carve")
        lv.X, lv.ldx = self.X.data_ptr(), KP
        if self.ssq is not None:
            lv.ssq, lv.clouds, lv.rows_per_cloud = self.ssq.data_ptr(), self.C, N_PTS

        def member(name, shape, integer=False):
            off = (getattr(lv, name) - mem.data_ptr()) // 4
            v = mem[off:off + int(np.prod(shape))]
            return (v.view(torch.int32) if integer else v).view(*shape)
        views = {"cnt": member("cnt", (4,), True), "idx": member("idx", (self.Qb,), True), "pos": member("pos", (self.Qb,), True),
                 "g3c": member("g3c", (self.Qb, H)), "h1c": member("h1c", (self.Qb, H)), "h2c": member("h2c", (self.Qb, H)),
                 "Xc": member("Xc", (self.Qb, KP))}
        return lv, views, band

    def run(self, lv, phases=7, weights=True):
        """the data chain and the weight gradients through the `_live` entries (lv = None: the dense form)"""
        from dpdist_amd import lib as L
        lib, s, Qb, dev = L.load(), L.cur_stream(), self.Qb, self.dev
        out, bands = {}, []

        def buf(name, shape):
            v, b = G.banded(shape, shape[1], device=dev)
            out[name] = v
            bands.append(b)
            return v
        dy, g3, g2, g1 = buf("dy", (Qb, 3)), buf("g3", (Qb, H)), buf("g2", (Qb, H)), buf("g1", (Qb, H))
        dW1, dW2, dW3 = buf("dW1", (KP, H)), buf("dW2", (H, H)), buf("dW3", (H, H))
        db1, db2, db3, dW4, db4 = buf("db1", (1, H)), buf("db2", (1, H)), buf("db3", (1, H)), buf("dW4", (H, 3)), buf("db4", (1, 3))
        dbp = buf("db_partials", (2 * (Qb // 32), H))
        part = torch.empty(((Qb + 7) // 8) * (4 * H + 8), device=dev)
        sg = L.make_small_grads(None, None, db3, dW4, db4, part, db_partials=dbp)
        wsb = self.ws.numel() * 4
        L.check(lib.dpd_decoder_bwd_data_live(L.ptr(self.dpred), L.ptr(self.mask), L.ptr(self.y), L.ptr(self.h1), L.ptr(self.h2), L.ptr(self.h3),
                                              Qb, KP, H, self.params, 0, L.ptr(dy), L.ptr(g3), L.ptr(g2), L.ptr(g1), None, sg, L.ptr(self.ws), wsb,
                                              None, phases, lv, s), "dpd_decoder_bwd_data_live")
        if weights:
            L.check(lib.dpd_decoder_bwd_weights_live(1, L.ptr(self.X), KP, L.ptr(g1), Qb, KP, H, 0, L.ptr(dW1), L.ptr(db1), L.ptr(self.ws), wsb, None,
                                                     L.ptr(dbp), lv, s), "dpd_decoder_bwd_weights_live(1)")
            L.check(lib.dpd_decoder_bwd_weights_pair_live(L.ptr(self.h1), L.ptr(g2), L.ptr(dW2), L.ptr(self.h2), L.ptr(g3), L.ptr(dW3), H, Qb, H, H, 0,
                                                          L.ptr(self.ws), wsb, None, L.ptr(db2), L.ptr(dbp), lv, s), "dpd_decoder_bwd_weights_pair_live")
            # layers 2 and 3 one at a time (layer 2 finishes db2 once more, into its own buffer)
            dW2s, dW3s, db2s = buf("dW2s", (H, H)), buf("dW3s", (H, H)), buf("db2s", (1, H))
            L.check(lib.dpd_decoder_bwd_weights_live(2, L.ptr(self.h1), H, L.ptr(g2), Qb, H, H, 0, L.ptr(dW2s), L.ptr(db2s), L.ptr(self.ws), wsb, None,
                                                     L.ptr(dbp), lv, s), "dpd_decoder_bwd_weights_live(2)")
            L.check(lib.dpd_decoder_bwd_weights_live(3, L.ptr(self.h2), H, L.ptr(g3), Qb, H, H, 0, L.ptr(dW3s), None, L.ptr(self.ws), wsb, None,
                                                     None, lv, s), "dpd_decoder_bwd_weights_live(3)")
        torch.cuda.synchronize()
        for b in bands:
            b()
        return out


def _bits(x):
    return x.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------ 1. compaction
@pytest.mark.parametrize("use_ssq", [True, False])
@pytest.mark.parametrize("kind", ["none", "all", "one", "L31", "L32", "L33", "one_cloud", "flag_fv", "flag_query", "flag_and_dy"])
@pytest.mark.parametrize("B", [2, 4])
def test_compaction_against_numpy(dev, B, kind, use_ssq):
    """idx, {L, Lp}, pos, zero pad rows and bit-equal copies; nothing beyond position Lp is written.  Liveness comes from dy, from the
    encoder sums of the row's two clouds (use_ssq) or from the rows of X themselves."""
    ch = _Chain(dev, B, kind, use_ssq=use_ssq)
    lv, v, band = ch.descriptor()
    out = ch.run(lv, phases=1, weights=False)
    band()
    dy = out["dy"].cpu().numpy()
    from_dy = ~(dy == 0).all(axis=1)
    assert np.array_equal(from_dy, ch.want_live)                 # the inputs do what the pattern says
    L, Lp, idx, pos = restate(ch.live)
    assert {"none": L == 0, "all": L == ch.Qb, "one": L == 1, "L31": L == 31, "L32": L == 32, "L33": L == 33, "one_cloud": L == N_PTS,
            "flag_fv": L == N_PTS, "flag_query": L == N_PTS, "flag_and_dy": N_PTS < L <= N_PTS + 40}[kind]
    assert v["cnt"].cpu().tolist() == [L, Lp, 0, 0]
    assert np.array_equal(v["pos"].cpu().numpy(), pos)
    got_idx = v["idx"].cpu().numpy()
    live_pos = np.array(sorted(idx), dtype=np.int64)
    pad_pos = np.array(sorted(set(range(Lp)) - set(idx)), dtype=np.int64)
    assert len(pad_pos) == Lp - L
    assert np.array_equal(got_idx[live_pos], np.array([idx[p] for p in live_pos], dtype=np.int64))
    assert ((got_idx[pad_pos] >= 0) & (got_idx[pad_pos] < ch.Qb)).all()
    assert G.untouched(v["idx"][Lp:].view(torch.float32))
    rows = torch.tensor([idx[p] for p in live_pos], dtype=torch.long, device=dev)
    lp_t, pp_t = torch.tensor(live_pos, device=dev), torch.tensor(pad_pos, device=dev)
    for name, src in (("g3c", out["g3"]), ("h1c", ch.h1), ("h2c", ch.h2), ("Xc", ch.X)):
        assert torch.equal(_bits(v[name][lp_t]), _bits(src[rows])), name
        assert not _bits(v[name][pp_t]).any(), name                # pad rows: +0.0 everywhere
        assert G.untouched(v[name][Lp:]), name


# ------------------------------------------------------------------------------------------------ 2. GEMM level
@functools.lru_cache(maxsize=None)
def _dense(dev, B, kind):
    ch = _Chain(dev, B, kind)
    return ch, ch.run(None)


def _eq(a, b):
    """== with equal NaN patterns (the sign of a zero is free)"""
    na, nb = torch.isnan(a), torch.isnan(b)
    return torch.equal(na, nb) and torch.equal(torch.where(na, torch.zeros_like(a), a), torch.where(nb, torch.zeros_like(b), b))


@pytest.mark.parametrize("tile", [33, 32])
@pytest.mark.parametrize("kind", ["none", "one", "L32", "L33", "quarter", "all", "flag_and_dy"])
@pytest.mark.parametrize("B", [2, 4])
def test_live_entries_equal_the_dense_entries(dev, B, kind, tile):
    """dH (compact rows against the dense rows), dW1, dW2 + dW3 (grouped and one at a time), the 32-row partial sums and db1 / db2:
    == the dense entries on the same data.  none: M_dev = K_dev = 0 (zero gradients, not stale ones); one / L32: one K-tile and a
    ragged 64-row workgroup tile; L33: a padded second tile; all: the capacity.  Both wave tiles of the plan."""
    from dpdist_amd import lib as L
    lib = L.load()
    ch, want = _dense(dev, B, kind)
    lv, v, band = ch.descriptor()
    try:
        for op in (9, 10, 11):
            assert lib.dpd_set_gemm_plan(op, tile, 1) == 0
        got = ch.run(lv)
    finally:
        for op in (9, 10, 11):
            assert lib.dpd_set_gemm_plan(op, 33, 1) == 0
    band()
    L_, Lp, idx, pos = restate(ch.live)
    assert v["cnt"].cpu().tolist() == [L_, Lp, 0, 0]
    assert (L_ == 0) == (kind == "none") and (L_ == ch.Qb) == (kind == "all")
    for name in ("dy", "g3", "db3", "dW4", "db4"):          # the output layer is untouched by the form
        assert torch.equal(_bits(got[name]), _bits(want[name])), name
    live_pos = torch.tensor(sorted(idx), dtype=torch.long, device=dev)
    rows = torch.tensor([idx[p] for p in sorted(idx)], dtype=torch.long, device=dev)
    dead = torch.tensor(np.nonzero(~ch.live)[0], dtype=torch.long, device=dev)
    for name in ("g2", "g1"):
        assert _eq(got[name][live_pos], want[name][rows]), name
        assert not want[name][dead].any(), name                  # what the form leaves out is zero rows
        assert not got[name][:Lp][torch.tensor(sorted(set(range(Lp)) - set(idx)), dtype=torch.long, device=dev)].any(), name
        assert G.untouched(got[name][Lp:]), name
    for name in ("dW1", "dW2", "dW3", "dW2s", "dW3s", "db_partials", "db1", "db2", "db2s"):
        assert _eq(got[name], want[name]), name
    if kind == "none":
        assert not got["dW1"].any() and not got["dW2"].any() and not got["dW3"].any() and not got["db1"].any()
    else:
        assert want["dW1"].any() and want["dW3"].any() and want["db1"].any()


def test_live_entries_argument_errors(dev):
    """what the descriptor form does not take is an error, not another form"""
    from dpdist_amd import lib as L
    lib, s = L.load(), L.cur_stream()
    ch = _Chain(dev, 2, "one")
    lv, v, band = ch.descriptor()
    g = torch.zeros(ch.Qb, H, device=dev)
    dW = torch.zeros(KP, H, device=dev)
    args = (L.ptr(ch.X), KP, L.ptr(g), ch.Qb, KP, H)
    assert lib.dpd_decoder_bwd_weights_live(1, *args, 2, L.ptr(dW), None, None, 0, None, None, lv, s) == -3        # plane compute type
    assert lib.dpd_decoder_bwd_weights_live(1, *args, 0, L.ptr(dW), L.ptr(g), None, 0, None, None, lv, s) == -3    # db without the partials
    assert lib.dpd_decoder_bwd_weights_live(1, L.ptr(ch.X), KP, L.ptr(g), ch.Qb - 32, KP, H, 0, L.ptr(dW), None, None, 0, None, None, lv, s) == -2
    assert lib.dpd_set_gemm_plan(9, 30, 1) < 0
    band()


# ------------------------------------------------------------------------------------------------ 3. trainer
def _trainer(dev, B, W0, **kw):
    from dpdist_amd.model import DPDistParams
    from dpdist_amd.trainer import DPDistTrainer
    P = DPDistParams(device=dev)
    P.load_tf_state_dict(W0)
    return P, DPDistTrainer(P, B, base_lr=1e-4, distributed=False, **kw)      # (the benchmark's learning rate)


def _run_trainer(dev, batches, order, **kw):
    P, tr = _trainer(dev, 4, synth.make_weights("wide"), **kw)
    snaps, counts = [], []
    for bi in order:
        a, b, l = batches[bi]
        tr.step(a, b, l)
        torch.cuda.synchronize()
        snaps.append({k: getattr(tr, k).clone() for k in ("loss", "pred", "grad")})
        snaps[-1]["params"] = P.flat.detach().clone()
        counts.append(tr.live_count.cpu().tolist() if tr.live_count is not None else None)
    return tr, snaps, counts


@pytest.mark.parametrize("unique_l1", [None, False])
def test_trainer_equals_the_dense_trainer(dev, unique_l1):
    """B = 4, two batches in turn, five steps: loss, pred, every gradient and the weights == the option-off trainer's after every step.
    The live count (read back here only) covers most rows (more than half of the 256), a handful (1 .. 16) and none at all within
    the run: 143, 3, 0, 0, 0 on this input as it is (b4 of make_weights("wide") not shifted)."""
    cu = lambda a: torch.tensor(a, device=dev)      # noqa: E731
    batches = [tuple(cu(x) for x in synth.s2_modelnet_shaped(4, 64, 100 + i)) for i in range(2)]
    order = [0, 1, 0, 1, 0]
    opts = {} if unique_l1 is None else {"unique_l1": False}
    tr_on, on, counts = _run_trainer(dev, batches, order, options=dict(opts))
    tr_off, off, none = _run_trainer(dev, batches, order, options=dict(opts, live_rows=False))
    assert tr_on.live_rows and not tr_off.live_rows and none == [None] * 5
    assert tr_on.unique_l1 == (unique_l1 is None)
    print("live rows per step:", counts)
    for t, (x, y) in enumerate(zip(on, off)):
        for k in x:
            assert _eq(x[k], y[k]), (t, k)
    Ls = [c[0] for c in counts]
    assert all(c[1] == (c[0] + 31) // 32 * 32 and 0 <= c[0] <= tr_on.BN for c in counts)
    assert max(Ls) > tr_on.BN // 2, Ls
    assert any(0 < n <= 16 for n in Ls), Ls
    assert min(Ls) == 0, Ls


# ------------------------------------------------------------------------------------------------ 4. NaN cloud
@pytest.mark.parametrize("front2", [True, False])
@pytest.mark.parametrize("side", ["A", "B"])
def test_nan_cloud_keeps_the_dense_nan_pattern(dev, side, front2):
    """One far point (it underflows every Gaussian: the reference's 0/0) in one cloud of pcA / pcB: the gradient of the first step has
    the dense form's NaN pattern and its values elsewhere.  front2 = False: no encoder sums, the rows of X are looked at."""
    B = 2
    a, b, l = (torch.tensor(x, device=dev) for x in synth.s2_modelnet_shaped(B, 64, 7))
    (a if side == "A" else b)[1, 5] = torch.tensor([40.0, -35.0, 50.0], device=dev)
    runs = {}
    for name, opt in (("on", {}), ("off", {"live_rows": False})):
        from dpdist_amd.model import DPDistParams
        from dpdist_amd.trainer import DPDistTrainer
        P = DPDistParams(device=dev)
        P.load_tf_state_dict(synth.make_weights("wide"))
        tr = DPDistTrainer(P, B, base_lr=1e-3, distributed=False, options=dict(opt, front2=front2))
        tr.step(a, b, l)
        torch.cuda.synchronize()
        runs[name] = {k: getattr(tr, k).clone() for k in ("loss", "pred", "grad")}
        if name == "on":
            assert tr.live_rows and tr.live_count[0].item() >= N_PTS
    # pcA's cloud feeds the Fisher vectors the gradient rows gather: NaN in the dense gradient.  pcB's feeds the other direction's rows
    # only (its far point is a masked query here): the flag makes the cloud's rows live and the gradient stays what it was, NaN-free
    assert bool(torch.isnan(runs["off"]["grad"]).any()) == (side == "A")
    for k in runs["on"]:
        assert _eq(runs["on"][k], runs["off"][k]), k

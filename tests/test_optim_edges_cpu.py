"""The exact-value optimizer / loss checker of tests/optim_cases.py has teeth: a numpy stand-in "kernel" that writes into the
guard-banded buffers passes every case of the GPU tables (tests/test_optim_edges_gpu.py), and check_fused raises for every corruption
the fused optimizer launch or its host side can commit without a loss-curve test noticing.  Also: the float32 restatement stays inside
its float64 rounding bound, the exact family is exact, every table entry keeps the entry's own rules, and every validation rule of
dpd_adam_tf_fused / dpd_adam_tf / dpd_adam_tf_dev / dpd_l1_loss returns the code the source gives it.  Runs without a GPU."""
import ctypes

import numpy as np
import pytest
import torch

from . import optim_cases as O
from .gemm_cases import FLAT_BAND, NAN_OUT, NAN_OUT16

CASES = O.fused_cases()


def _ids(cases):
    return [c.id for c in cases]


# ------------------------------------------------------------------------------------------------ the stand-in
def _adam(p, g, m, v, lr_t, c, corrupt=None):
    lr_t, b1, b2, eps, gscale = (O.F32(x) for x in (lr_t,) + tuple(c[1:]))
    if corrupt == "swap_b":
        b1, b2 = b2, b1
    if corrupt == "no_gscale":
        gscale = O.F32(1.0)
    if corrupt == "eps_in_sqrt":
        gs = g * gscale
        m2 = b1 * m + (O.F32(1) - b1) * gs
        v2 = b2 * v + ((O.F32(1) - b2) * gs) * gs
        return p - (lr_t * m2) / np.sqrt(v2 + eps), m2, v2
    return O.adam_f32(p, g, m, v, lr_t, b1, b2, eps, gscale)


def _first_changed(a, b, lo=0):
    return lo + int(np.flatnonzero(O.bits(a)[lo:] != O.bits(b)[lo:])[0])


def standin(run, lr_t, corrupt=None):
    """the reference "kernel": adam_f32 over the live elements, the tail's gradient and the loss from the records, the copies from the
    new p -- written into the run's banded buffers.  `corrupt` names one deliberate mistake."""
    case, c = run.case, run.consts
    p, g, m, v = (x.numpy() for x in (run.p, run.g, run.m, run.v))         # share the banded memory
    live = case.n - (case.tail.pad if case.tail is not None else 0)
    if run.partials is not None:
        t, off, T = case.tail, O.tail_off(case), O.tail_len(case.tail)
        recs = run.partials.numpy().reshape(t.nparts, t.rec).astype(np.float64)
        if corrupt == "tail_short":
            recs = recs[:-1]
        g[off:off + T] = recs[:, :T].sum(0).astype(np.float32)
        if run.loss is not None:
            run.loss.copy_(torch.from_numpy(O.tail_loss(recs[:, T + 1:T + 4].sum(0), t.nparts if corrupt == "loss_nparts" else O.tail_qb(t))))
    p0, m0, v0 = p.copy(), m.copy(), v.copy()
    m_in = m0.copy()
    if corrupt == "neighbour_m":
        k = int(np.flatnonzero(m0[:live - 1] != m0[1:live])[0])
        m_in[k] = m0[k + 1]
    p[:live], m[:live], v[:live] = _adam(p0[:live], g[:live], m_in[:live], v0[:live], lr_t, c, corrupt)
    if corrupt == "skipped":
        k = _first_changed(p, p0, 7)
        p[k], m[k], v[k] = p0[k], m0[k], v0[k]
    if corrupt == "twice":
        again = _adam(p[:live], g[:live], m[:live], v[:live], lr_t, c)
        k = _first_changed(again[0], p[:live], 7)
        p[k], m[k], v[k] = (x[k] for x in again)
    if corrupt == "padding_written":
        assert live < case.n
        p[case.n - 1] = 1.0
    for i, mt in enumerate(case.mats):
        cnt = mt.rows * mt.cols
        w = p[mt.off:mt.off + cnt].reshape(mt.rows, mt.cols)
        if mt.wt:
            run.WT[i].view(mt.cols, mt.rows).copy_(torch.from_numpy(np.ascontiguousarray(w.T)))
            if corrupt == "wt_stale_rows":
                assert mt.rows % 64
                run.WT[i].view(torch.int32).view(mt.cols, mt.rows)[:, mt.rows // 64 * 64:] = NAN_OUT
        if not (case.np and O.is_listed(case, mt)):
            continue
        src = p0[mt.off:mt.off + cnt].reshape(mt.rows, mt.cols) if corrupt == "planes_of_old_p" else w
        np_w = 2 if corrupt == "second_plane" else case.np
        rc, r8 = (x[:np_w] for x in O.planes_of(src, 3 if corrupt == "second_plane" else case.np))
        if corrupt == "r8_as_rc":
            r8 = rc
        for buf, x in ((run.rc[i], rc), (run.r8[i], r8)):
            if buf is not None:
                buf[:np_w * cnt].copy_(torch.from_numpy(np.ascontiguousarray(x)).reshape(-1))
    if corrupt == "guard_written":
        run.checks[0].raw[FLAT_BAND - 1] = 0                                # a stray store of 0.0f right before p


def plain_standin(run, lr_t):
    p, g, m, v = (x.numpy() for x in (run.p, run.g, run.m, run.v))
    p[:], m[:], v[:] = O.adam_f32(p.copy(), g, m.copy(), v.copy(), lr_t, *run.consts[1:])


def _run(cid, family, corrupt=None, lr_ts=None):
    return O.run_fused_case(O.case_by_id(cid), family, lambda r, lr: standin(r, lr, corrupt), lr_ts=lr_ts)


# ------------------------------------------------------------------------------------------------ the stand-in passes
@pytest.mark.parametrize("family", list(O.FAMILIES))
@pytest.mark.parametrize("case", [c for c in CASES if c.n < 100000], ids=_ids([c for c in CASES if c.n < 100000]))
def test_standin_passes_every_case(case, family):
    run = O.run_fused_case(case, family, standin)
    O.check_fused(run)
    # the header's promise "same arithmetic, element for element, as dpd_adam_tf": the plain form on the same state
    plain = O.run_fused_case(O.vector_form(case), family, plain_standin, prefill_tail=True, state=run.state)
    O.check_fused(plain, tail_role=False)
    for a, b in ((run.p, plain.p), (run.m, plain.m), (run.v, plain.v)):
        O.same_bits(a, b, "fused against plain")


def test_standin_passes_the_capped_length():
    run = O.run_fused_case(O.case_by_id("V-%d" % O.CAPPED_N), "real_t1", standin)
    O.check_fused(run)
    assert run.case.n // 4 > 256 * 2048 and run.case.n % 4 == 3


@pytest.mark.parametrize("cid", O.TWO_STEP_CASES)
def test_standin_passes_two_steps(cid):
    run = _run(cid, "real_t1", lr_ts=(O.lr_t_of(1), O.lr_t_of(2)))
    O.check_fused(run)
    one = _run(cid, "real_t1")
    assert not np.array_equal(O.bits(run.p), O.bits(one.p))


def test_unwritten_outputs_raise():
    for cid in ("M1", "D1-np3", "T1-17-pad0"):
        run = O.run_fused_case(O.case_by_id(cid), "exact", lambda r, lr: None)
        with pytest.raises(AssertionError):
            O.check_fused(run)


# ------------------------------------------------------------------------------------------------ one test per corruption
def _raises(cid, family, corrupt, match):
    O.check_fused(_run(cid, family))
    with pytest.raises(AssertionError, match=match):
        O.check_fused(_run(cid, family, corrupt))


def test_element_skipped_raises():
    _raises("M3", "exact", "skipped", r"^p: 1 of 13342 elements differ")


def test_element_updated_twice_raises():
    _raises("M3", "exact", "twice", r"^p: 1 of 13342 elements differ")


def test_m_of_the_neighbour_raises():
    _raises("M3", "exact", "neighbour_m", r"^p: 1 of 13342 elements differ")


def test_eps_inside_the_square_root_raises():
    _raises("M2", "real_t1", "eps_in_sqrt", r"^p: \d+ of 8717 elements differ")


def test_b1_and_b2_swapped_raises():
    _raises("M2", "real_t1000", "swap_b", r"^p: \d+ of 8717 elements differ")


def test_gscale_dropped_raises():
    _raises("M2", "exact", "no_gscale", r"^p: \d+ of 8717 elements differ")
    _raises("M2", "real_t1", "no_gscale", r"^p: \d+ of 8717 elements differ")


def test_wt_stale_for_the_last_partial_row_tile_raises():
    _raises("M2", "exact", "wt_stale_rows", r"^WT\[0\]: 512 of 8704 elements differ; first at \[0, 64\]")


def test_r8_written_with_rc_layout_raises():
    for cid in ("D2-both-np3", "L1b-np1"):
        _raises(cid, "exact", "r8_as_rc", r"^W_r8\[0\]")


def test_planes_of_the_old_p_raise():
    for cid in ("D1-np1", "L2-np3"):
        _raises(cid, "exact", "planes_of_old_p", r"^W_rc\[0\]")


def test_np1_writing_a_second_plane_raises():
    _raises("D1-np1", "real_t1", "second_plane", r"W_rc\[0\]: a plane beyond np = 1 was written")


def test_tail_summed_over_one_record_less_raises():
    for cid in ("T1-17-pad0", "T3"):
        _raises(cid, "exact", "tail_short", r"^p: ")


def test_loss_divided_by_nparts_raises():
    _raises("T1-16-pad3", "exact", "loss_nparts", r"^loss: ")


def test_padding_element_written_raises():
    _raises("T1-40-pad3", "exact", "padding_written", r"^p: 1 of 22 elements differ; first at \[21\]")


def test_guard_element_written_raises():
    _raises("V-5", "exact", "guard_written", "guard band changed at 1 raw elements, first at offset %d" % (FLAT_BAND - 1))


def test_plane_buffers_ignored_at_np0_must_stay_untouched():
    run = _run("M4", "exact")
    O.check_fused(run)
    assert run.WT[1] is None and O.untouched(run.rc[1], NAN_OUT16)
    run.r8[1][5] = 0
    with pytest.raises(AssertionError, match=r"W_r8\[1\] written although np = 0"):
        O.check_fused(run)


# ------------------------------------------------------------------------------------------------ references and builders
def test_restatement_stays_inside_its_float64_bound(record_property):
    """200 000 log-uniform elements at t = 1, 10, 1000: err / tol of adam_f32 against adam_f64 is at most 1 for p, m and v (0.55 when this
    was written: 0.53).  The bound still has teeth: eps inside the square root changes the step by more than a rounding only where
    v' is within a few decades of eps = 1e-8 .. 1e-2 of the 1e-6 .. 10 range (a third of the elements; a quarter is asserted), a dropped
    gscale doubles g' wherever the gradient is not negligible beside m and v (about 0.78; a half is asserted).  The bitwise comparison
    of check_fused catches both on every run; these shares say what the float64 bound alone would still see."""
    rng = np.random.default_rng(11)
    n = 200000
    worst = 0.0
    for t in (1, 10, 1000):
        c = O.real_consts(t)
        st = O.real_state(rng, n, c)
        worst = max(worst, O.bound_ratio(*st, c))
        tol_p = O.adam_bound(*st, *c)[0]
        want_p = O.adam_f64(*st, *c)[0]
        for corrupt, share in (("eps_in_sqrt", 0.25), ("no_gscale", 0.5)):
            bad_p = _adam(*st, c.lr_t, c, corrupt)[0].astype(np.float64)
            caught = float((np.abs(bad_p - want_p) > tol_p).mean())
            print("t = %d: %s leaves the bound on %.3f of the elements" % (t, corrupt, caught))
            assert caught >= share, (t, corrupt, caught)
    record_property("largest_err_over_tol", worst)
    print("largest err/tol of the float32 restatement: %.3f" % worst)
    assert worst <= 1.0


def test_exact_family_is_exact_and_varied():
    rng = np.random.default_rng(5)
    p, g, m, v = O.exact_state(rng, 200000)                 # asserts adam_f32 == adam_f64 == the closed form
    out = O.adam_f32(p, g, m, v, *O.EXACT_CONSTS)
    triples = np.unique(np.stack([O.bits(x) for x in out], 1), axis=0)
    assert len(triples) >= 50000                            # a neighbour's value is seen
    frozen = (g == 0) & (m == 0) & (v == 0)
    assert 0.2 < frozen.mean() < 0.3
    for x in (p, g, m, v) + out:
        assert np.isfinite(x).all() and (np.abs(x[x != 0]) >= 2.0 ** -8).all()


def test_real_state_has_no_denormals_and_refuses_them():
    rng = np.random.default_rng(6)
    for t in (1, 1000):
        p, g, m, v = O.real_state(rng, 50000, O.real_consts(t))
        assert 0.03 < (g == 0).mean() < 0.07 and (v > 0).all()
    with pytest.raises(AssertionError):
        O.assert_no_tiny(p, g * O.F32(1e-20), m, v, O.real_consts(1))


def test_planes_of_layouts():
    x = np.arange(16 * 64, dtype=np.float32).reshape(16, 64) + np.float32(0.00390625)
    rc, r8 = O.planes_of(x, 3)
    assert rc.shape == (3, 16, 64) and r8.shape == (3, 2, 64, 8) and rc.dtype == np.int16
    back = sum(torch.from_numpy(rc[q]).view(torch.bfloat16).double() for q in range(3)).numpy()
    assert np.array_equal(back, x.astype(np.float64))       # 18 significant bits: three planes hold them all
    for q, rg, c, j in ((0, 0, 0, 0), (1, 1, 63, 7), (2, 1, 5, 3), (0, 0, 17, 6)):
        assert r8[q, rg, c, j] == rc[q, 8 * rg + j, c]
    rc1, r81 = O.planes_of(x, 1)
    assert np.array_equal(rc1[0], rc[0]) and np.array_equal(r81[0], r8[0]) and rc1.shape[0] == 1


def test_tail_partials_sum_exactly_and_hold_nan_where_nothing_reads():
    rng = np.random.default_rng(7)
    H = 12
    T = 4 * H + 3
    g_tail = rng.integers(-18, 19, size=T).astype(np.float32)
    for nparts in (1, 16, 17):
        for rec, sums in ((T + 1, None), (T + 5, None), (T + 9, (5, -7, 130))):
            rp = O.tail_partials(rng, g_tail, sums, nparts, rec)
            assert rp.shape == (nparts, rec) and rp.dtype == np.float32
            s, ls = O.partial_sums(rp, T, sums is not None)
            assert np.array_equal(s, g_tail) and (sums is None or ls.tolist() == list(sums))
            holes = np.ones(rec, bool)
            holes[:T] = False
            if sums is not None:
                holes[T + 1:T + 4] = False
            assert (O.bits(rp)[:, holes] == O.NAN_IN).all() and np.isfinite(rp[:, ~holes]).all()
    with pytest.raises(AssertionError):
        O.tail_partials(rng, g_tail + np.float32(0.5), None, 4, T + 1)
    with pytest.raises(AssertionError):
        O.tail_partials(rng, g_tail, (1, 2, 3), 4, T + 4)


def test_every_table_entry_keeps_the_entrys_rules():
    assert len({c.id for c in CASES}) == len(CASES) == 40
    for c in CASES:
        O.case_rules(c)
    by = {c.id: c for c in CASES}
    assert {c.tail.nparts for c in CASES if c.id.startswith("T1")} == {1, 15, 16, 17, 40}
    assert O.tail_off(by["T3"]) % 4 == 1 and by["T3"].tail.H == 256
    assert O.tail_off(by["T4"]) == by["T4"].mats[0].off + 24 * 256
    assert by["M1"].n == 4 * 64 and by["M2"].mats[0].rows % 64 == 4
    assert {c.np for c in CASES if c.id[0] in "DL"} == {1, 3}
    with pytest.raises(AssertionError):
        O.case_rules(by["M2"]._replace(mats=(O.Mat(8, 68, 96, True, False, False),)))
    with pytest.raises(AssertionError):
        O.case_rules(by["D1-np1"]._replace(mats=(O.Mat(0, 12, 128, False, True, True),)))
    with pytest.raises(AssertionError):
        O.case_rules(by["M3"]._replace(mats=by["M3"].mats[::-1]))
    with pytest.raises(AssertionError):
        O.case_rules(by["T2-rec52"]._replace(tail=O.Tail(6, 17, 52, False, 2)))


# ------------------------------------------------------------------------------------------------ L1 loss
def l1_standin(run, sign0=0.0):
    pred, lab, BN = run.pred.numpy(), run.labels.numpy(), run.BN
    inv = O.F32(1) / O.F32(BN)
    d = pred[:BN, 0] - lab
    run.loss[0] = float(O.F32(np.abs(d).astype(np.float64).sum()) * inv)
    run.loss[1] = float((O.F32(pred[:BN, 0].astype(np.float64).sum()) * inv + O.F32(pred[BN:, 0].astype(np.float64).sum()) * inv) / O.F32(2))
    if run.mode == 1:
        sg = np.where(d > 0, 1.0, np.where(d < 0, -1.0, sign0)).astype(np.float32)
        run.dpred[:BN] = torch.from_numpy(np.stack([sg * inv * O.F32(run.gscale), np.zeros(BN, np.float32), np.zeros(BN, np.float32)], 1))
    if run.mode == 2:
        run.dpred[:] = torch.tensor([float(O.F32(0.5) * inv * O.F32(run.gscale)), 0.0, 0.0])


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("BN", O.L1_BN)
def test_l1_standin_passes(BN, mode):
    for gscale in O.L1_GSCALE:
        run = O.L1Run(BN, mode, gscale)
        assert torch.isnan(run.pred[:, 1:]).all() and (run.pred[:BN, 0] == run.labels).sum() * 10 >= BN
        l1_standin(run)
        run.check()


def test_l1_checker_has_teeth():
    run = O.L1Run(257, 1, 0.25)
    l1_standin(run, sign0=1.0)                              # sign(0) taken as +1
    with pytest.raises(AssertionError, match="^dpred"):
        run.check()
    run = O.L1Run(257, 1, 1.0)
    l1_standin(run)
    run.dpred[257, 0] = 0.0                                 # mode 1 writing a row of the BA half
    with pytest.raises(AssertionError, match="beyond the mode's"):
        run.check()
    run = O.L1Run(255, 0, 1.0)
    l1_standin(run)
    run.dpred[0, 1] = 0.0                                   # mode 0 writing a gradient
    with pytest.raises(AssertionError, match="beyond the mode's"):
        run.check()
    run = O.L1Run(1000, 2, 1.0)
    l1_standin(run)
    run.loss[1] = float(run.loss[1]) * 2                    # the mean of the two means not halved
    with pytest.raises(AssertionError, match="^loss"):
        run.check()


# ------------------------------------------------------------------------------------------------ validation codes
@pytest.fixture(scope="module")
def lib():
    from dpdist_amd import build, lib as L
    build.build(verbose=False)          # hipcc cross-compiles gfx950 without a GPU
    return L.load()


ADDR = 1 << 30                          # any 16-byte aligned non-NULL "device address": nothing is dereferenced
E_NULL, E_DIM, E_UNSUPPORTED = -1, -2, -3


def _fuse(mats=(), np_=0, tail=None):
    """mats: (off, rows, cols, WT, rc, r8) addresses or None; tail: dict(partials, nparts, rec, H, Qb, tail_off, loss)"""
    from dpdist_amd import lib as L
    f = L.AdamFuse()
    for i, (off, rows, cols, wt, rc, r8) in enumerate(mats):
        f.w_off[i], f.w_rows[i], f.w_cols[i], f.WT[i], f.W_rc[i], f.W_r8[i] = off, rows, cols, wt, rc, r8
    f.np = np_
    for k, x in (tail or {}).items():
        setattr(f, k, x)
    return f


def _fused(lib, f, n=8192, p=ADDR, g=ADDR, m=ADDR, v=ADDR):
    P = ctypes.c_void_p
    return lib.dpd_adam_tf_fused(P(p), P(g), P(m), P(v), n, 1e-3, 0.9, 0.999, 1e-8, 1.0, None if f is None else ctypes.byref(f), None)


def _tail(n, H=4, **kw):
    t = dict(partials=ADDR, nparts=2, rec=4 * H + 8, H=H, Qb=13, tail_off=n - (4 * H + 3), loss=ADDR)
    t.update(kw)
    return t


def test_fused_entry_null_dim_and_alignment(lib):
    ok = _fuse([(0, 64, 64, ADDR, None, None)])
    for name in "pgmv":
        assert _fused(lib, ok, **{name: None}) == E_NULL, name
    assert _fused(lib, None) == E_NULL
    assert _fused(lib, ok, n=0) == E_DIM
    for name in "pgmv":
        assert _fused(lib, ok, **{name: ADDR + 4}) == E_UNSUPPORTED, name


def test_fused_entry_matrix_rules(lib):
    assert _fused(lib, _fuse([(0, 64, 64, None, ADDR, ADDR)], np_=2)) == E_UNSUPPORTED
    assert _fused(lib, _fuse([(0, 64, 96, ADDR, None, None)])) == E_UNSUPPORTED              # cols % 64
    assert _fused(lib, _fuse([(0, 6, 64, ADDR, None, None)])) == E_UNSUPPORTED               # rows % 4
    assert _fused(lib, _fuse([(0, 12, 64, None, ADDR, ADDR)], np_=3)) == E_UNSUPPORTED       # rows % 8 with planes
    assert _fused(lib, _fuse([(0, 12, 64, ADDR, ADDR, None)], np_=1)) == E_UNSUPPORTED
    assert _fused(lib, _fuse([(6, 64, 64, ADDR, None, None)])) == E_UNSUPPORTED              # w_off % 4
    assert _fused(lib, _fuse([(-4, 64, 64, ADDR, None, None)])) == E_UNSUPPORTED             # negative w_off
    assert _fused(lib, _fuse([(4, 64, 64, ADDR, None, None)]), n=4096) == E_UNSUPPORTED      # the matrix ends beyond n
    assert _fused(lib, _fuse([(0, 0, 64, ADDR, None, None)])) == E_UNSUPPORTED
    assert _fused(lib, _fuse([(0, 64, 64, ADDR + 4, None, None)])) == E_UNSUPPORTED          # misaligned WT
    assert _fused(lib, _fuse([(0, 64, 64, None, ADDR + 8, ADDR)], np_=3)) == E_UNSUPPORTED   # misaligned plane pointers
    assert _fused(lib, _fuse([(0, 64, 64, None, ADDR, ADDR + 2)], np_=1)) == E_UNSUPPORTED
    assert _fused(lib, _fuse([(4096, 64, 64, ADDR, None, None), (0, 64, 64, ADDR, None, None)])) == E_DIM      # descending offsets
    assert _fused(lib, _fuse([(0, 64, 64, ADDR, None, None), (4092, 4, 64, ADDR, None, None)])) == E_DIM       # overlapping by 4


def test_fused_entry_tail_rules(lib):
    n = 8192
    assert _fused(lib, _fuse(tail=_tail(n, nparts=0)), n) == E_DIM
    assert _fused(lib, _fuse(tail=_tail(n, H=0)), n) == E_DIM
    assert _fused(lib, _fuse(tail=_tail(n, rec=4 * 4 + 3, loss=None)), n) == E_DIM
    assert _fused(lib, _fuse(tail=_tail(n, tail_off=n - 18)), n) == E_DIM                    # the tail ends beyond n
    assert _fused(lib, _fuse(tail=_tail(n, tail_off=-1)), n) == E_DIM
    assert _fused(lib, _fuse(tail=_tail(n, tail_off=n - 19 - 4)), n) == E_DIM                # more than 3 elements behind the tail
    assert _fused(lib, _fuse([(0, 64, 64, ADDR, None, None)], tail=_tail(4096 + 13)), 4096 + 13) == E_DIM      # overlaps the matrix
    assert _fused(lib, _fuse(tail=_tail(n, rec=4 * 4 + 7)), n) == E_DIM                      # a loss needs the sums in the record
    assert _fused(lib, _fuse(tail=_tail(n, Qb=0)), n) == E_DIM
    assert _fused(lib, _fuse(tail=_tail(n, H=6, loss=None)), n) == E_UNSUPPORTED


def test_plain_entries_and_l1_validation(lib):
    P = ctypes.c_void_p
    a, bad = P(ADDR), P(ADDR + 4)
    tail = (0.9, 0.999, 1e-8, 1.0, None)
    assert lib.dpd_adam_tf_dev(a, a, a, a, 8, None, *tail) == E_NULL
    for k in range(4):
        ptrs = [a] * 4
        ptrs[k] = None
        assert lib.dpd_adam_tf_dev(*ptrs, 8, a, *tail) == E_NULL
        assert lib.dpd_adam_tf(*ptrs, 8, 1e-3, *tail) == E_NULL
        ptrs[k] = bad
        assert lib.dpd_adam_tf_dev(*ptrs, 8, a, *tail) == E_UNSUPPORTED
        assert lib.dpd_adam_tf(*ptrs, 8, 1e-3, *tail) == E_UNSUPPORTED
    assert lib.dpd_adam_tf_dev(a, a, a, a, 0, a, *tail) == E_DIM
    assert lib.dpd_adam_tf(a, a, a, a, 0, 1e-3, *tail) == E_DIM
    # dpd_l1_loss(pred, labels, BN, mode, gscale, loss, dpred, stream)
    assert lib.dpd_l1_loss(None, a, 4, 0, 1.0, a, None, None) == E_NULL
    assert lib.dpd_l1_loss(a, None, 4, 0, 1.0, a, None, None) == E_NULL
    assert lib.dpd_l1_loss(a, a, 4, 0, 1.0, None, None, None) == E_NULL
    assert lib.dpd_l1_loss(a, a, 4, 1, 1.0, a, None, None) == E_NULL                        # a gradient mode needs dpred
    assert lib.dpd_l1_loss(a, a, 4, 2, 1.0, a, None, None) == E_NULL
    assert lib.dpd_l1_loss(a, a, 0, 0, 1.0, a, None, None) == E_DIM
    assert lib.dpd_l1_loss(a, a, 4, 3, 1.0, a, a, None) == E_DIM
    assert lib.dpd_l1_loss(a, a, 4, -1, 1.0, a, a, None) == E_DIM

"""The exact-value window-gather cases of tests/window_cases.py, checked without a GPU: the numpy references are bit-equal to the
oracle (oracle/restate.py: voxel_lookup, local_window) on the face-adjacent queries of every m in 2 .. 10 and k in {1, 3, 5, 7}; the
float32 cell faces leave gaps for m in {6, 7, 9, 10} and none elsewhere; the forward table reaches the kernel form written next to each
entry (a Python restatement of the host's dispatch); a numpy stand-in "kernel" passes every entry of every table and each deliberate
corruption of it makes the checker raise; every validation rule of the entries returns the code the source gives it."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import restate as R

from . import window_cases as W
from .gemm_cases import FLAT_BAND, NAN_OUT

FWD = W.fwd_cases()
BWD = W.bwd_cases()
GAPPED, TIGHT = (6, 7, 9, 10), (2, 3, 4, 5, 8)


# ------------------------------------------------------------------------------------------------ references against the oracle
@pytest.mark.parametrize("m", range(2, 11))
def test_references_equal_the_oracle_on_the_faces(m):
    """lookup against voxel_lookup and rows against local_window gathered at the voxel, in float32, bit for bit, on every face with its
    float32 neighbours and on the specials"""
    q = W.edge_pool(m)
    lk = W.lookup(q, m)
    v, mask, local = R.voxel_lookup(torch.from_numpy(q)[None], m)
    assert local.dtype == torch.float32
    assert np.array_equal(v[0].numpy(), lk.vox)
    W.same_bits(mask[0], lk.mask, "mask")
    W.same_bits(local[0], lk.local, "local", nan_any=True)
    c, half = W.axis(m)
    assert np.array_equal(R.grid_axis(m).astype(np.float32), c)
    fv = np.random.default_rng(m).standard_normal((1, m ** 3, W.F)).astype(np.float32)
    for k in (1, 3, 5, 7):
        win = R.local_window(torch.from_numpy(fv), m, k)[0][v[0]]
        X = W.rows(q, fv, None, m, k, W.padded_width(k))
        E = W.E_of(k)
        W.same_bits(X[:, :E], win.numpy(), "window k = %d" % k)
        W.same_bits(X[:, E:E + 3], lk.local, "local columns", nan_any=True)
        assert not W.bits(X[:, E + 3:]).any()


def test_axis_of_one_cell_is_library_defined():
    c, half = W.axis(1)
    assert c.tolist() == [0.0] and half == 1.0
    lk = W.lookup(np.array([[1.0, 0.0, -0.0], [-1.0, 0, 0], [np.nextafter(np.float32(1), np.float32(2)), 0, 0]], np.float32), 1)
    assert lk.mask.tolist() == [1.0, 0.0, 0.0] and lk.vox.tolist() == [0, 0, 0]


# ------------------------------------------------------------------------------------------------ gap facts
def _interior(m):
    """face-adjacent values strictly between the outer faces, and whether each lies in a cell"""
    c, half = W.axis(m)
    v = W.face_values(m)
    v = v[(v > c[0] - half) & (v <= c[-1] + half)]
    q = np.stack([v, np.full_like(v, c[0]), np.full_like(v, c[0])], 1)
    return v, W.lookup(q, m).mask


def test_gapped_axes_mask_interior_queries_and_tight_axes_do_not():
    for m in GAPPED:
        v, mask = _interior(m)
        assert (mask == 0).any(), m
    for m in TIGHT:
        v, mask = _interior(m)
        assert len(v) > 4 * m and mask.all(), m
    for m in (6, 10):
        z = np.array([[0.0, 0.5, 0.5], [-0.0, 0.5, 0.5], [0.5, 0.5, 0.5]], np.float32)
        assert W.lookup(z, m).mask.tolist() == [0.0, 0.0, 1.0], m
    for m in range(1, 11):      # cells never overlap: the first matching cell is the only one, whatever the query
        c, half = W.axis(m)
        assert ((c + half)[:-1] <= (c - half)[1:]).all(), m


def test_specials_are_masked_into_voxel_zero():
    for m in range(1, 11):
        c, _ = W.axis(m)
        q = W.specials(m)
        lk = W.lookup(q, m)
        out = ~(np.abs(q) <= 1).all(1)                    # a coordinate of +-1.5, +-inf or NaN
        assert out.sum() >= 20 and not lk.mask[out].any() and not lk.vox[out].any()
        W.same_bits(lk.local[out], q[out] - c[0], "local of a masked row", nan_any=True)
        assert not lk.mask[(q == -1).any(1)].any()        # the open lower face of cell 0


# ------------------------------------------------------------------------------------------------ the tables
def test_forward_table_reaches_the_form_written_next_to_each_entry():
    assert len({c.id for c in FWD}) == len(FWD)
    count = dict.fromkeys(W.FORMS, 0)
    for c in FWD:
        assert W.dispatch(c) == c.form, c.id
        assert c.C > 0 and c.N > 0 and 1 <= c.m <= 10 and c.k in (1, 3, 5, 7) and W.kp(c) >= W.E_of(c.k) + 3 and W.kp(c) % 4 == 0
        if c.form.startswith("planes"):
            assert 0 <= c.Qb <= c.C * c.N
        if c.form in count:
            count[c.form] += 1
    assert min(count.values()) >= 4, count
    for form in ("row", "lds"):
        got = {(c.m, c.k) for c in FWD if c.form == form and c.C <= 3 and c.N <= 16 and c.dKP == 0}
        assert got >= {(m, k) for m in range(1, 11) for k in (1, 3, 5, 7)}
        assert {c.ssq for c in FWD if c.form == form} == {None, "random", "pow4", "clamp"}
    for form in W.FORMS:
        assert {c.ssq is None for c in FWD if c.form == form} == {True, False}, form
    by = {c.id: c for c in FWD}
    big = by["R-lds-too-large"]
    assert big.N % 8 == 0 and W.dispatch(big._replace(dKP=big.dKP - 32)) == "lds" and big.dKP % 32 == 0
    assert W.dispatch(by["L-largest"]) == "lds" and by["L-largest"].dKP == 0
    c = by["PL-m9k7-np3"]
    assert 0 <= W.LDS_LIMIT - (3 * 9 ** 3 * W.F * 2 + W.kp(c) // 4 * 8) < 1200
    assert by["R-wide"].dKP == 4 and by["L-wide"].dKP == 32
    assert by["P3-8x12-qb32-np3"].N % 8 and by["P3-8x12-qb64-np1"].x is False
    for m in GAPPED:                                                  # every face query of a gapped m runs through both fp32 forms
        for cid in ("R-faces-m%d" % m, "L-faces-m%d" % m):
            assert by[cid].N >= W.n_faces(m) and (W.fwd_ref(by[cid]).look.mask == 0).sum() > 20


def test_backward_table_covers_the_shapes():
    assert len({c.id for c in BWD}) == len(BWD)
    mix = [c for c in BWD if c.voxf == "mix" and c.dKP == 0 and c.dq and c.dfv]
    assert {(c.C, c.N) for c in mix} >= {(C, N) for C in W.BWD_C for N in W.BWD_N}
    assert {c.m for c in mix} == {1, 2, 5, 8, 9, 10} and {c.k for c in mix} == {1, 3, 5, 7}
    assert {(c.m, c.k) for c in mix} >= {(1, 7), (10, 7), (9, 3)}
    for C, N in ((C, N) for C in W.BWD_C for N in W.BWD_N):
        assert {c.val for c in mix if (c.C, c.N) == (C, N)} == {"int", "f32"}
    cap = W.bwd_case("B-cap")
    assert (cap.N, cap.k, W.kp(cap), cap.m, cap.val) == (8192, 1, 24, 2, "int")
    d = W.bwd_data(W.bwd_case("B-masked-f32"))
    assert np.abs(d.dX[d.look.mask == 0][:, :W.E_of(3)]).min() > 0          # masked rows carry gradient
    assert W.PADDED_WIDTHS == {k: W.padded_width(k) for k in (1, 3, 5, 7, 9)}


# ------------------------------------------------------------------------------------------------ the stand-in
def _scale(ssq, cloud, corrupt):
    ss = np.float32(0)
    for sl in range(W.SLICES):
        ss = ss + ssq[cloud, sl]
    if corrupt == "clamp_after_sqrt":
        return np.float32(1) / np.maximum(np.sqrt(ss), np.float32(1e-12))
    return np.float32(1) / np.sqrt(np.maximum(ss, np.float32(1e-12)))


def standin_fwd(run, corrupt=None):
    """the entry as a row-by-row numpy loop, written into the run's banded buffers; returns the code.  `corrupt` names one mistake."""
    case, d = run.case, run.data
    form = W.dispatch(case)
    if form in ("null", "refused"):
        return W.return_code(case)
    C, N, m, k, KP, Q = case.C, case.N, case.m, case.k, run.KP, run.Q
    E, h = W.E_of(k), (k - 1) // 2
    c, half = W.axis(m)
    lo, hi = c - half, c + half
    X = np.zeros((Q, KP), np.float32)
    mask, vox = np.zeros(Q, np.float32), np.zeros(Q, np.int32)
    dd = np.arange(k) - h
    with np.errstate(invalid="ignore"):
        for r in range(Q):
            cell = []
            for v in d.q[r]:
                hit = np.flatnonzero(((v >= lo) if corrupt == "closed_lower" else (v > lo)) & (v <= hi))
                cell.append(-1 if len(hit) == 0 else int(hit[-1 if corrupt == "last_cell" else 0]))
            valid = min(cell) >= 0
            ix, iy, iz = cell if valid else (0, 0, 0)
            mask[r] = valid
            vox[r] = (ix * m + iy) * m + iz if corrupt == "swap_xy" else (iy * m + ix) * m + iz
            cloud = r // N
            g = d.fv[cloud].reshape(m, m, m, W.F)
            if d.ssq is not None:
                sc_cloud = (8 * (r // 8)) // N if corrupt == "neighbour_scale" else cloud
                g = g * _scale(d.ssq, sc_cloud, corrupt)
            a = [(ix if corrupt == "axis_order" else iy) + dd, (iy if corrupt == "axis_order" else ix) + dd, iz + dd]
            ok = [(x >= 0) & (x < m) for x in a]
            a = [np.clip(x, 0, m - 1) for x in a]
            if corrupt == "clamp":
                ok = [np.ones(k, bool)] * 3
            win = np.where((ok[0][:, None, None] & ok[1][None, :, None] & ok[2][None, None, :])[..., None], g[np.ix_(*a)], np.float32(0))
            X[r, :E] = win.reshape(-1)
            X[r, E:E + 3] = d.q[r] - c[[ix, iy, iz]]
    if corrupt == "padding":
        X[Q - 1, KP - 1] = 1.0
    taken = form.startswith("planes")
    outs = [(run.mask, mask), (run.vox, vox)]
    if run.X is not None:
        outs.append((run.X, X))
    if taken:
        qb = case.Qb + 8 if corrupt == "r8_rows" else case.Qb
        rc, r8 = W.planes(X, case.np, qb)
        if run.rc is not None:
            outs.append((run.rc[:rc.size], rc))
        if run.r8 is not None:
            if corrupt == "r8_rows":          # plane p still starts at p Qb KP: the extra row group lands on the next plane or behind the last
                for p in range(case.np):
                    run.r8[p * case.Qb * KP:][:r8[p].size].copy_(torch.from_numpy(r8[p].reshape(-1)))
            else:
                outs.append((run.r8[:r8.size], r8))
    if corrupt == "bad_remap":                # block b works on the remapped row group although the cloud count is no multiple of 8
        assert form in ("lds", "planes_lds1", "planes_lds3") and C % 8
        rgpc = N // 8
        hit = {((b // 8 // rgpc) * 8 + b % 8) * rgpc + (b // 8) % rgpc for b in range(Q // 8)}
        keep = np.repeat(np.array([rg in hit for rg in range(Q // 8)]), 8)
        mask, vox = np.where(keep, mask, np.int32(NAN_OUT).view(np.float32)), np.where(keep, vox, NAN_OUT).astype(np.int32)
        X[~keep] = np.int32(NAN_OUT).view(np.float32)
        outs = [(run.mask, mask), (run.vox, vox)] + ([(run.X, X)] if run.X is not None else [])
    for buf, x in outs:
        buf.copy_(torch.from_numpy(np.ascontiguousarray(x).reshape(-1)))
    if corrupt == "guard":
        run.checks[-1].raw[FLAT_BAND - 1] = 0
    return 0


def _fwd(cid, corrupt=None):
    run = W.FwdRun(W.fwd_case(cid))
    return run, standin_fwd(run, corrupt)


@pytest.mark.parametrize("case", FWD, ids=[c.id for c in FWD])
def test_forward_standin_passes_every_case(case):
    run = W.FwdRun(case)
    W.check_fwd(run, standin_fwd(run))


def _fwd_raises(cid, corrupt, match):
    W.check_fwd(*_fwd(cid))
    with pytest.raises(AssertionError, match=match):
        W.check_fwd(*_fwd(cid, corrupt))


def test_unwritten_forward_outputs_raise():
    for cid in ("R-1x1", "L-1x8", "PL-4x8-qb32-np1", "P3-4x8-np3"):
        run = W.FwdRun(W.fwd_case(cid))
        with pytest.raises(AssertionError):
            W.check_fwd(run, 0)


def test_closed_lower_face_raises():
    for m in (1, 8, 10):
        _fwd_raises("R-faces-m%d" % m, "closed_lower", "^mask")
        _fwd_raises("L-faces-m%d" % m, "closed_lower", "^mask")


def test_last_matching_cell_cannot_differ_from_the_first():
    """the float32 cells of m = 1 .. 10 never overlap (asserted in the gap test), so "the last matching cell instead of the first" is the
    same function on every float and no output can tell them apart: the stand-in with that change still passes -- the one listed
    corruption that is not observable.  A closed lower face, which does make neighbouring cells share a float, is caught above."""
    for m in (7, 8, 10):
        W.check_fwd(*_fwd("R-faces-m%d" % m, "last_cell"))


def test_x_and_y_swapped_in_vox_raises():
    _fwd_raises("R-3x5", "swap_xy", "^vox")
    _fwd_raises("PL-4x8-qb32-np1", "swap_xy", "^vox")


def test_window_axis_order_raises():
    _fwd_raises("L-3x16", "axis_order", "^X:")
    _fwd_raises("PL-4x8-qb0-np3", "axis_order", "^X_rc")


def test_clamped_instead_of_zero_clipping_raises():
    _fwd_raises("R-m10k7", "clamp", "^X:")
    _fwd_raises("L-m2k5", "clamp", "^X:")


def test_scale_of_the_neighbouring_cloud_in_a_straddling_group_raises():
    for cid in ("P3-8x12-qb32-np1", "P3-8x12-qb64-np3"):
        _fwd_raises(cid, "neighbour_scale", "^X")


def test_clamp_after_the_square_root_raises():
    _fwd_raises("L-16x24", "clamp_after_sqrt", "^X:")
    _fwd_raises("PL-8x8-qb32-np1", "clamp_after_sqrt", "^X_rc")


def test_r8_written_for_eight_rows_more_raises():
    _fwd_raises("PL-8x8-qb32-np3", "r8_rows", "^X_r8")
    _fwd_raises("P3-8x12-qb32-np1", "r8_rows", "X_r8 written beyond its Qb = 32 rows")


def test_nonzero_padding_column_raises():
    _fwd_raises("R-wide", "padding", r"^X: 1 of \d+ elements differ")
    _fwd_raises("L-wide", "padding", r"^X: 1 of \d+ elements differ")


def test_remap_with_a_cloud_count_that_is_no_multiple_of_8_raises():
    _fwd_raises("L-3x16", "bad_remap", "^mask")
    _fwd_raises("PL-k7-np1", "bad_remap", "^mask")


def test_guard_element_written_raises():
    _fwd_raises("R-3x5", "guard", "guard band changed at 1 raw elements, first at offset %d" % (FLAT_BAND - 1))


def test_planes_not_taken_must_stay_untouched_and_refusals_write_nothing():
    run, code = _fwd("NT-qb")
    W.check_fwd(run, code)
    run.rc[7] = 0
    with pytest.raises(AssertionError, match="X_rc written although the planes were not taken"):
        W.check_fwd(run, code)
    run, code = _fwd("P3-k7-r8-np3")
    assert code == W.E_UNSUPPORTED
    W.check_fwd(run, code)
    run.mask[0] = 0.0
    with pytest.raises(AssertionError, match="mask written although the entry refused"):
        W.check_fwd(run, code)
    with pytest.raises(AssertionError, match="return code"):
        W.check_fwd(*_fwd("NT-q-null")[:1], 0)


def test_planes_reference_layouts_and_nonfinite_values():
    x = (np.arange(16 * 32, dtype=np.float32).reshape(16, 32) + np.float32(0.00390625)) * np.float32(1.0001)
    x[3, 5], x[4, 6], x[5, 7] = np.inf, -np.inf, np.nan
    rc, r8 = W.planes(x, 3, 8)
    assert rc.shape == (3, 16, 32) and r8.shape == (3, 1, 32, 8) and rc.dtype == np.int16
    back = sum(torch.from_numpy(rc[p]).view(torch.bfloat16).double() for p in range(3)).numpy()
    fin = np.isfinite(x)
    assert (np.abs(back[fin] - x[fin]) <= np.abs(x)[fin] * 2.0 ** -24).all()
    assert back[3, 5] == np.inf and back[4, 6] == -np.inf and np.isnan(back[5, 7])
    assert not rc[1:, ~fin].any()
    for p, c, j in ((0, 0, 0), (1, 31, 7), (2, 5, 3)):
        assert r8[p, 0, c, j] == rc[p, j, c]
    rc1, _ = W.planes(x, 1)
    assert np.array_equal(rc1[0], rc[0])


# ---- backward, combine, stack
def standin_bwd(run, corrupt=None):
    case, d = run.case, run.data
    dX, vox = run.dX_np, d.look.vox
    if corrupt == "descending":
        order = np.concatenate([np.arange(c * case.N, (c + 1) * case.N)[::-1] for c in range(case.C)])
        dfv, _ = W.bwd(dX[order], vox[order], case.C, case.N, case.m, case.k)
    elif corrupt == "skip_masked":
        dfv, _ = W.bwd(np.where(d.look.mask[:, None] > 0, dX, np.float32(0)), vox, case.C, case.N, case.m, case.k)
    else:
        dfv, _ = W.bwd(dX, vox, case.C, case.N, case.m, case.k)
    E = W.E_of(case.k)
    if run.dfv is not None:
        run.dfv.copy_(torch.from_numpy(dfv.reshape(-1)))
    if run.dq is not None:
        run.dq.copy_(torch.from_numpy(dX[:, E:E + 3].reshape(-1).copy()))


@pytest.mark.parametrize("case", BWD, ids=[c.id for c in BWD])
def test_backward_standin_passes_every_case(case):
    run = W.BwdRun(case)
    standin_bwd(run)
    W.check_bwd(run)


def _bwd_raises(cid, corrupt, match):
    run = W.BwdRun(W.bwd_case(cid))
    standin_bwd(run, corrupt)
    with pytest.raises(AssertionError, match=match):
        W.check_bwd(run)


def test_backward_summed_in_descending_order_raises():
    _bwd_raises("B-one-64-m8k5-f32", "descending", "^dfv")
    _bwd_raises("B-3x130-m1k1-f32", "descending", "^dfv")


def test_backward_ignoring_masked_rows_raises():
    for val in ("int", "f32"):
        _bwd_raises("B-masked-" + val, "skip_masked", "^dfv")


def test_unwritten_backward_outputs_raise():
    for cid in ("B-dq-alone", "B-dfv-alone"):
        with pytest.raises(AssertionError):
            W.check_bwd(W.BwdRun(W.bwd_case(cid)))


def test_onehot_adjoint_columns_are_what_the_forward_reads():
    """the (cell, channel) that onehot_columns names for a column is where `rows` reads that column from: a Fisher vector that is one at
    that element alone gives X[row, column] = 1, and a clipped column reads nothing"""
    clipped = 0
    for cid, rws in W.ONEHOT_CASES:
        case = W.bwd_case(cid)
        d = W.bwd_data(case)
        for row in rws:
            cols = W.onehot_columns(case, row)
            assert {0, W.E_of(case.k) - 1} <= {c for c, _ in cols}
            for col, src in cols:
                fv = np.zeros((case.C, case.m ** 3, W.F), np.float32)
                if src is None:
                    clipped += 1
                    fv[:] = 1.0
                    assert W.rows(d.q, fv, None, case.m, case.k, W.kp(case))[row, col] == 0.0
                else:
                    fv[row // case.N, src[0], src[1]] = 1.0
                    X = W.rows(d.q, fv, None, case.m, case.k, W.kp(case))
                    assert X[row, col] == 1.0 and X[row, :W.E_of(case.k)].sum() == 1.0
    assert clipped >= 8


def _combine_standin(run, swap=False):
    gA, gB = W.combine(run.dpts_np, run.dX_np, run.case.scale, run.BN, run.case.k)
    if swap:
        gA, gB = W.combine(run.dpts_np, np.concatenate([run.dX_np[run.BN:], run.dX_np[:run.BN]]), run.case.scale, run.BN, run.case.k)
    run.gA.copy_(torch.from_numpy(gA.reshape(-1)))
    run.gB.copy_(torch.from_numpy(gB.reshape(-1)))


def test_combine_and_stack_standins_pass_and_swapped_halves_raise():
    for case in W.combine_cases():
        run = W.CombineRun(case)
        _combine_standin(run)
        run.check()
        run = W.CombineRun(case)
        _combine_standin(run, swap=True)
        with pytest.raises(AssertionError, match="^gA"):
            run.check()
    assert 2 * 2 * 43 * 3 == 516 > 2 * 256
    for B, N in W.COMBINE_SHAPES:
        for noise in (False, True):
            run = W.StackRun(B, N, noise)
            pts, q = W.stack(run.a_np, run.b_np, run.noise_np)
            run.pts.copy_(torch.from_numpy(pts))
            run.q.copy_(torch.from_numpy(q))
            run.check()
            run.q[:run.n], run.q[run.n:] = run.q[run.n:].clone(), run.q[:run.n].clone()
            with pytest.raises(AssertionError, match="^q"):
                run.check()


# ------------------------------------------------------------------------------------------------ validation codes
@pytest.fixture(scope="module")
def lib():
    from dpdist_amd import build, lib as L
    build.build(verbose=False)          # hipcc cross-compiles gfx950 without a GPU
    return L.load()


ADDR = 1 << 30                          # any 16-byte aligned non-NULL "device address": nothing is dereferenced
P = ctypes.c_void_p


def _fwd_call(lib, q=ADDR, fv=ADDR, C=4, N=8, m=8, k=5, KP=2528, X=ADDR, mask=ADDR, vox=ADDR, pl=None, scaled=True):
    args = (C, N, m, k, KP, P(X), P(mask), P(vox), None if pl is None else ctypes.byref(pl), None)
    if scaled:
        return lib.dpd_patch_rows_fwd_scaled(P(q), P(fv), P(ADDR), *args)
    return lib.dpd_patch_rows_fwd(P(q), P(fv), *args)


def _desc(np_=3, Q=32, Qb=32, rc=ADDR, r8=ADDR):
    from dpdist_amd import lib as L
    pl = L.Planes()
    pl.np, pl.Q, pl.Qb, pl.X_rc, pl.X_r8 = np_, Q, Qb, rc, r8
    return pl


def test_forward_entry_validation(lib):
    for scaled in (True, False):
        for name in ("q", "fv", "mask", "vox", "X"):
            assert _fwd_call(lib, scaled=scaled, **{name: None}) == W.E_NULL, name
        assert _fwd_call(lib, scaled=scaled, C=0) == W.E_DIM and _fwd_call(lib, scaled=scaled, N=0) == W.E_DIM
        assert _fwd_call(lib, scaled=scaled, C=-1) == W.E_DIM and _fwd_call(lib, scaled=scaled, N=-8) == W.E_DIM
        for m in (0, 11):
            assert _fwd_call(lib, scaled=scaled, m=m) == W.E_UNSUPPORTED
        for k in (0, 2, 9):
            assert _fwd_call(lib, scaled=scaled, k=k, KP=W.padded_width(9)) == W.E_UNSUPPORTED
        assert _fwd_call(lib, scaled=scaled, KP=2502) == W.E_DIM            # KP < E + 3
        assert _fwd_call(lib, scaled=scaled, KP=2504 + 2) == W.E_DIM        # KP & 3
    assert _fwd_call(lib, pl=_desc(np_=2)) == W.E_DIM
    assert _fwd_call(lib, pl=_desc(Q=24)) == W.E_DIM
    assert _fwd_call(lib, pl=_desc(Qb=64)) == W.E_DIM                       # Qb > Q
    assert _fwd_call(lib, pl=_desc(Qb=-32)) == W.E_DIM
    assert _fwd_call(lib, X=None, pl=_desc(rc=None, r8=None)) == W.E_NULL   # a descriptor without plane buffers writes nothing
    assert _fwd_call(lib, X=None, pl=_desc(Qb=8)) == W.E_NULL               # planes not taken (Qb % 32) and no fp32 rows
    assert _fwd_call(lib, X=None, KP=2532, pl=_desc()) == W.E_NULL          # ... (KP % 32)
    assert _fwd_call(lib, X=None, C=3, N=5, pl=_desc(Q=15, Qb=0)) == W.E_NULL
    assert _fwd_call(lib, k=7, KP=6880, pl=_desc()) == W.E_UNSUPPORTED      # three row images at k = 7 exceed the LDS


def test_backward_combine_and_stack_validation(lib):
    def bwd(dX=ADDR, vox=ADDR, C=2, N=8, m=8, k=5, KP=2528):
        return lib.dpd_patch_rows_bwd(P(dX), P(vox), C, N, m, k, KP, P(ADDR), P(ADDR), None)
    assert bwd(dX=None) == W.E_NULL and bwd(vox=None) == W.E_NULL
    assert bwd(C=0) == W.E_DIM and bwd(N=0) == W.E_DIM
    assert bwd(N=W.BWD_CAP + 1) == W.E_UNSUPPORTED
    for m in (0, 11):
        assert bwd(m=m) == W.E_UNSUPPORTED
    for k in (0, 2, 9):
        assert bwd(k=k, KP=W.padded_width(9)) == W.E_UNSUPPORTED
    assert bwd(KP=2502) == W.E_DIM and bwd(KP=2506) == W.E_DIM
    assert lib.dpd_patch_rows_bwd(P(ADDR), P(ADDR), 2, 8, 8, 5, 2528, None, None, None) == 0      # nothing requested: nothing launched

    def comb(dpts=ADDR, dX=ADDR, B=2, N=8, k=5, KP=2528, gA=ADDR, gB=ADDR):
        return lib.dpd_asloss_combine(P(dpts), P(dX), None, B, N, k, KP, P(gA), P(gB), None)
    for name in ("dpts", "dX", "gA", "gB"):
        assert comb(**{name: None}) == W.E_NULL, name
    assert comb(B=0) == W.E_DIM and comb(N=0) == W.E_DIM and comb(KP=2502) == W.E_DIM
    for k in (0, 2, 9):
        assert comb(k=k, KP=W.padded_width(9)) == W.E_UNSUPPORTED

    def stk(pcA=ADDR, pcB=ADDR, B=2, N=8, pts=ADDR, q=ADDR):
        return lib.dpd_stack_clouds(P(pcA), P(pcB), None, B, N, P(pts), P(q), None)
    for name in ("pcA", "pcB", "pts", "q"):
        assert stk(**{name: None}) == W.E_NULL, name
    assert stk(B=0) == W.E_DIM and stk(N=-1) == W.E_DIM
    for k, w in W.PADDED_WIDTHS.items():
        assert lib.dpd_padded_width(k) == w

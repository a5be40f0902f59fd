"""Exact-value cases of the window gather (csrc/patch_rows.hip, patch_rows_bwd.h): numpy references, query / Fisher-vector / ssq
builders, guard-banded runs, the checkers and the case tables of tests/test_window_edges_gpu.py (tests/test_window_edges_cpu.py
holds the references to oracle/restate.py, proves that the checkers have teeth and that every table entry reaches the kernel form
written next to it).  Not a test module and not a conftest.  Nothing here calls the library.

The method.  The gather only compares, copies, multiplies once (x * scale) and subtracts once (q - centre) in float32, and the
library is compiled with -ffp-contract=off, so every output -- mask, voxel id, the fp32 rows, the bf16 RC / R8 planes -- must equal
its numpy-float32 restatement BIT FOR BIT.  The backward adds the window columns of a cloud's queries in ascending query order
(patch_rows_bwd.h states it as an invariant), so its float32 restatement in that order is bitwise too; with small-integer dX the
sums are exact in any order and are compared with an int64 reference.  Every buffer sits between guard bands
(gemm_cases.banded_flat); outputs start as a NaN of a known bit pattern; input elements nothing may read hold a quiet NaN.

m = 1 is library-defined: the reference cannot form `half` from one centre (oracle/restate.py: voxel_lookup indexes centre 1), the
library takes half = 1, one cell (-1, 1].  `axis` restates that; the oracle comparison covers m = 2 .. 10.
"""
import functools
import zlib
from collections import namedtuple

import numpy as np
import torch

from .gemm_cases import NAN_IN, NAN_OUT, NAN_OUT16, banded_flat, bf16_planes, small_int, untouched

F32 = np.float32
F = 20                         # DPD_FV_CHANNELS
SLICES = 4                     # DPD_MFV_SLICES
E_NULL, E_DIM, E_UNSUPPORTED = -1, -2, -3
LDS_LIMIT = 100 * 1024         # the host's bound of the LDS forms
PLANES3_LIMIT = 150 * 1024     # ... of the row-image form


def E_of(k):
    return k * k * k * F


def padded_width(k):
    """the formula of dpd_padded_width: window + 3, rounded up to 32 columns"""
    return (E_of(k) + 3 + 31) // 32 * 32


# ------------------------------------------------------------------------------------------------ bit comparisons
def bits(x):
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().contiguous().numpy()
    x = np.ascontiguousarray(x)
    return x.view(np.int32) if x.dtype == np.float32 else x


def _isnan_bits(b):
    if b.dtype == np.int16:
        return (b & 0x7FFF) > 0x7F80
    return (b & 0x7FFFFFFF) > 0x7F800000


def same_bits(got, want, what, nan_any=False):
    """bitwise equality (so that -0 is not +0).  nan_any: where `want` is a NaN, `got` must be a NaN of any payload; everything else
    bit for bit (float32 as int32, bf16 planes as int16)."""
    g, w = bits(got), bits(want)
    assert g.dtype == w.dtype and g.shape == w.shape, (what, g.dtype, g.shape, w.dtype, w.shape)
    ne = g != w
    if nan_any:
        ne &= ~(_isnan_bits(g) & _isnan_bits(w))
    if ne.any():
        bad = np.argwhere(ne)
        first = tuple(int(i) for i in bad[0])
        raise AssertionError("%s: %d of %d elements differ; first at %s: got bits 0x%x, want 0x%x"
                             % (what, len(bad), g.size, list(first), int(g[first]) & 0xFFFFFFFF, int(w[first]) & 0xFFFFFFFF))


# ------------------------------------------------------------------------------------------------ references
def axis(m):
    """make_axis (csrc/common.h) in numpy: centres (i (2/m) + (-1)) + 1/m in float64, cast to float32; half = |c0 - c1| / 2 in float32,
    1 for m = 1.  Returns (c [m] float32, half float32)."""
    i = np.arange(m, dtype=np.float64)
    c = ((i * (2.0 / m) + (-1.0)) + 1.0 / m).astype(np.float32)
    half = np.abs(c[0] - c[1]) / F32(2.0) if m > 1 else F32(1.0)
    assert c.dtype == np.float32 and np.asarray(half).dtype == np.float32
    return c, F32(half)


Look = namedtuple("Look", "mask vox local idx")      # idx [Q, 3]: (ix, iy, iz) of the coordinates (x, y, z)


def lookup(q, m):
    """q [Q, 3] float32 -> Look.  Per coordinate the FIRST cell i with q > c[i] - half && q <= c[i] + half, both bounds rounded to
    float32 before the comparison; a row with a coordinate in no cell is masked and takes cell (0, 0, 0).
    vox = (iy m + ix) m + iz, local = q - c[idx] in float32."""
    q = np.asarray(q)
    assert q.dtype == np.float32 and q.ndim == 2 and q.shape[1] == 3
    c, half = axis(m)
    lo, hi = c - half, c + half
    assert lo.dtype == np.float32 and hi.dtype == np.float32
    with np.errstate(invalid="ignore"):
        inside = (q[:, :, None] > lo) & (q[:, :, None] <= hi)           # [Q, 3, m]
    valid = inside.any(-1).all(-1)
    idx = np.where(valid[:, None], inside.argmax(-1), 0)
    ix, iy, iz = idx[:, 0], idx[:, 1], idx[:, 2]
    vox = ((iy * m + ix) * m + iz).astype(np.int32)
    with np.errstate(invalid="ignore"):
        local = q - c[idx]
    assert local.dtype == np.float32
    return Look(valid.astype(np.float32), vox, local, idx)


def scale_of(ssq):
    """ssq [C, SLICES, F] float32 -> scale [C, F]: the slices added in order in float32, then 1 / sqrt(max(ss, 1e-12f))"""
    ssq = np.asarray(ssq)
    assert ssq.dtype == np.float32 and ssq.shape[1:] == (SLICES, F)
    ss = np.zeros((ssq.shape[0], F), dtype=np.float32)
    for sl in range(SLICES):
        ss = ss + ssq[:, sl]
    sc = F32(1.0) / np.sqrt(np.maximum(ss, F32(1e-12)))
    assert sc.dtype == np.float32
    return sc


def rows(q, fv, ssq, m, k, KP):
    """X [Q, KP] float32 of q [Q, 3], fv [C, m^3, F], ssq [C, SLICES, F] or None: column ((d0 k + d1) k + d2) F + ch is channel ch
    of grid cell (iy + d0 - h, ix + d1 - h, iz + d2 - h) of the row's cloud (zero outside the grid), times scale[cloud, ch] with
    ssq (one float32 multiply); columns [E, E + 3) hold local; the rest is zero."""
    q, fv = np.asarray(q), np.asarray(fv)
    C, Q, E, h = fv.shape[0], q.shape[0], E_of(k), (k - 1) // 2
    assert fv.dtype == np.float32 and fv.shape == (C, m ** 3, F) and Q % C == 0 and KP >= E + 3
    lk = lookup(q, m)
    g = fv.reshape(C, m, m, m, F)
    if ssq is not None:
        g = g * scale_of(ssq)[:, None, None, None, :]
        assert g.dtype == np.float32
    pad = np.zeros((C,) + (m + 2 * h,) * 3 + (F,), dtype=np.float32)
    pad[:, h:h + m, h:h + m, h:h + m] = g
    d = np.arange(k)
    cloud = np.arange(Q) // (Q // C)
    a0, a1, a2 = (lk.idx[:, j][:, None] + d for j in (1, 0, 2))           # slowest first: (y, x, z)
    win = pad[cloud[:, None, None, None], a0[:, :, None, None], a1[:, None, :, None], a2[:, None, None, :]]       # [Q, k, k, k, F]
    X = np.zeros((Q, KP), dtype=np.float32)
    X[:, :E] = win.reshape(Q, E)
    X[:, E:E + 3] = lk.local
    return X


def _bf16(x):
    return torch.from_numpy(np.array(x)).float().bfloat16().view(torch.int16).numpy()


def planes(X, np_, Qb=None):
    """bf16 bit patterns (int16) of the operand planes of X [Q, KP]: (RC [np, Q, KP], R8 [np, Qb/8, KP, 8] of the first Qb rows, where
    R8[p][rg][c][j] = plane p of row 8 rg + j, column c).  np = 1: X rounded to bf16 (nearest even); np = 3: hi, mid, lo of
    gemm_cases.bf16_planes; an inf or NaN lives in the hi plane alone (mid = lo = +0, as split3 in gemm_shared.h)."""
    X = np.asarray(X)
    assert X.dtype == np.float32 and X.ndim == 2 and np_ in (1, 3)
    Q, KP = X.shape
    Qb = Q if Qb is None else Qb
    assert Q % 8 == 0 and Qb % 8 == 0 and 0 <= Qb <= Q
    fin = np.isfinite(X)
    pl = [_bf16(X)]
    if np_ == 3:
        _, mid, lo = bf16_planes(np.where(fin, X, F32(0.0)))
        pl += [np.where(fin, _bf16(mid), np.int16(0)), np.where(fin, _bf16(lo), np.int16(0))]
    rc = np.stack(pl).astype(np.int16)
    r8 = np.ascontiguousarray(rc[:, :Qb].reshape(np_, Qb // 8, 8, KP).transpose(0, 1, 3, 2))
    return rc, r8


def bwd(dX, vox, C, N, m, k, dtype=np.float32):
    """dfv [C, m^3, F]: dfv[c, g, ch] = the sum, n ascending, of dX[c N + n, ((g0 - p0 + h) k + (g1 - p1 + h)) k + (g2 - p2 + h)) F + ch]
    over the queries whose window covers g (p = the query's cell; a masked query's is cell 0: the exact transpose of what the forward
    gathered), accumulated in `dtype`.  Returns (dfv, dq), dq = a copy of columns [E, E + 3)."""
    dX, vox = np.asarray(dX), np.asarray(vox).reshape(C, N).astype(np.int64)
    E, h = E_of(k), (k - 1) // 2
    assert dX.shape[0] == C * N and dX.shape[1] >= E + 3 and ((0 <= vox) & (vox < m ** 3)).all()
    p0, p1, p2 = vox // (m * m), (vox // m) % m, vox % m
    pad = np.zeros((C,) + (m + 2 * h,) * 3 + (F,), dtype=dtype)
    win = dX[:, :E].astype(dtype).reshape(C, N, k, k, k, F)
    for n in range(N):
        for c in range(C):
            a, b, d = p0[c, n], p1[c, n], p2[c, n]
            pad[c, a:a + k, b:b + k, d:d + k] += win[c, n]
    dfv = np.ascontiguousarray(pad[:, h:h + m, h:h + m, h:h + m]).reshape(C, m ** 3, F)
    assert dfv.dtype == dtype
    return dfv, dX[:, E:E + 3].copy()


def bwd_int(dX, vox, C, N, m, k):
    """the same for integer-valued dX in int64: exact whatever the order"""
    dXi = np.rint(dX[:, :E_of(k)]).astype(np.int64)
    assert np.array_equal(dXi.astype(np.float32), dX[:, :E_of(k)])
    dfv, _ = bwd(np.concatenate([dXi, np.zeros((len(dXi), 3), np.int64)], 1), vox, C, N, m, k, np.int64)
    assert int(np.abs(dfv).max(initial=0)) < (1 << 24)
    return dfv


def combine(dpts, dX, scale, BN, k):
    """(gA, gB) [BN, 3]: (dpts[which, r, c] + dX[qrow, E + c]) * scale in float32; qrow = BN + r for gA (which = 0), r for gB"""
    E = E_of(k)
    dpts = np.asarray(dpts).reshape(2, BN, 3)
    sc = F32(1.0) if scale is None else F32(scale)
    gA = (dpts[0] + dX[BN:2 * BN, E:E + 3]) * sc
    gB = (dpts[1] + dX[:BN, E:E + 3]) * sc
    assert gA.dtype == np.float32 and gB.dtype == np.float32
    return gA, gB


def stack(pcA, pcB, noise):
    """pts = [pcA + noise ; pcB], q = [pcB ; pcA]"""
    a = pcA if noise is None else pcA + noise
    assert a.dtype == np.float32
    return np.concatenate([a, pcB]), np.concatenate([pcB, pcA])


# ------------------------------------------------------------------------------------------------ query families
def face_values(m):
    """every rounded cell face fl32(c[i] - half), fl32(c[i] + half) with its two float32 neighbours on each side"""
    c, half = axis(m)
    out = []
    for f in np.concatenate([c - half, c + half]):
        dn1, up1 = np.nextafter(f, F32(-np.inf)), np.nextafter(f, F32(np.inf))
        out += [np.nextafter(dn1, F32(-np.inf)), dn1, f, up1, np.nextafter(up1, F32(np.inf))]
    return np.array(out, dtype=np.float32)


SPECIAL_VALUES = np.array([1.0, -1.0, 1.5, -1.5, np.nan, np.inf, -np.inf, 0.0, -0.0], dtype=np.float32)


def _placed(values, m):
    """each value in one coordinate at a time (the other two at a cell centre, which is inside its cell) and in all three at once"""
    c, _ = axis(m)
    out = []
    for j, v in enumerate(values):
        b = c[j % m]
        out += [(v, b, b), (b, v, b), (b, b, v), (v, v, v)]
    return np.array(out, dtype=np.float32)


def faces(m):
    return _placed(face_values(m), m)


def specials(m):
    return _placed(SPECIAL_VALUES, m)


def edge_pool(m):
    return np.concatenate([faces(m), specials(m)])


def in_cell(rng, m, i, n):
    """n queries strictly inside cell (i, i, i)"""
    c, half = axis(m)
    q = (c[i] + rng.uniform(-0.9, 0.9, size=(n, 3)) * float(half)).astype(np.float32)
    lk = lookup(q, m)
    assert lk.mask.all() and (lk.idx == i).all()
    return q


def family(rng, name, m, n):
    """n queries of one family: faces (the whole edge pool, cycled), specials, corner0 / cornerL (one voxel: the first / the last, whose
    window is clipped on three sides), random (uniform(-1.1, 1.1)), mix (half edge pool, half random)"""
    if name == "faces":
        pool = edge_pool(m)
        return pool[np.arange(n) % len(pool)]
    if name == "specials":
        pool = specials(m)
        return pool[rng.permutation(len(pool))[np.arange(n) % len(pool)]]
    if name == "corner0":
        return in_cell(rng, m, 0, n)
    if name == "cornerL":
        return in_cell(rng, m, m - 1, n)
    if name == "random":
        return rng.uniform(-1.1, 1.1, size=(n, 3)).astype(np.float32)
    assert name == "mix", name
    pool = edge_pool(m)
    take = min(len(pool), n // 2)
    return np.concatenate([pool[rng.permutation(len(pool))[:take]], family(rng, "random", m, n - take)])


def n_faces(m, mult=1):
    """rows of the whole edge pool, rounded up to a multiple of `mult`"""
    return (len(edge_pool(m)) + mult - 1) // mult * mult


def make_ssq(rng, C, fam):
    """[C, SLICES, F] float32 or None.  random: ss in [0.1, 2]; pow4: ss = 4^e split 1/2, 1/4, 1/8, 1/8 over the slices (every partial
    sum exact, scale = 2^-e exactly); clamp: per (cloud, channel) in turn ss = 0, just below 1e-12f, just above, exactly 1e-12f, random"""
    if fam is None:
        return None
    s = rng.uniform(0.025, 0.5, size=(C, SLICES, F)).astype(np.float32)
    if fam == "pow4":
        e = rng.integers(-3, 4, size=(C, 1, F))
        s = (4.0 ** e * np.array([0.5, 0.25, 0.125, 0.125])[None, :, None]).astype(np.float32)
        assert np.array_equal(scale_of(s).astype(np.float64), 2.0 ** -e[:, 0].astype(np.float64))
    elif fam == "clamp":
        t = F32(1e-12)
        for c in range(C):
            for ch in range(F):
                kind = (c * F + ch) % 5
                if kind < 4:
                    s[c, :, ch] = 0.0
                    s[c, ch % SLICES, ch] = (F32(0.0), np.nextafter(t, F32(0.0)), np.nextafter(t, F32(1.0)), t)[kind]
    else:
        assert fam == "random", fam
    return s


def _rng(case, salt=0):
    return np.random.default_rng([zlib.crc32(repr(case).encode()), salt])


def _frozen(*xs):
    for x in xs:
        if x is not None:
            x.setflags(write=False)
    return xs


# ------------------------------------------------------------------------------------------------ forward cases
# form: the kernel form the host must pick (asserted against `dispatch` on the CPU); dKP: columns beyond dpd_padded_width(k);
# ssq: family or None; x: fp32 rows requested; np: planes of the descriptor (0: no descriptor); rc / r8: which plane buffers are offered;
# qf: query family of cloud c = qf[c % len(qf)]
FwdCase = namedtuple("FwdCase", "id form C N m k dKP ssq x np Qb rc r8 qf")
FORMS = ("row", "lds", "planes_lds1", "planes_lds3", "planes3_1", "planes3_3")
MIX = ("mix", "corner0", "cornerL")


def kp(case):
    return padded_width(case.k) + case.dKP


def dispatch(case):
    """Python restatement of the host's choice in dpd_patch_rows_fwd_scaled: one of FORMS, "null" (DPD_E_NULL: neither rows nor
    planes to write) or "refused" (DPD_E_UNSUPPORTED: the row images of three planes at k = 7 exceed the LDS)"""
    Q, KP, G = case.C * case.N, kp(case), case.m ** 3
    offered = case.np != 0 and (case.rc or case.r8)
    taken = offered and Q % 8 == 0 and case.Qb % 32 == 0 and KP % 32 == 0
    if not case.x and not taken:
        return "null"
    tab = KP // 4 * 8
    if taken:
        if not case.x and case.N % 8 == 0 and case.np * G * F * 2 + tab <= LDS_LIMIT:
            return "planes_lds%d" % case.np
        if (case.np * 8 * KP * 2 if case.r8 else 0) + tab > PLANES3_LIMIT:
            return "refused"
        return "planes3_%d" % case.np
    if case.N % 8 == 0 and Q % 8 == 0 and G * F * 4 + tab <= LDS_LIMIT:
        return "lds"
    return "row"


def return_code(case):
    return {"null": E_NULL, "refused": E_UNSUPPORTED}.get(case.form, 0)


def _kp_beyond_lds(m, k):
    """the first width, in steps of 32 above the padded one, at which the host's inequality for the LDS form fails"""
    d = 0
    while m ** 3 * F * 4 + (padded_width(k) + d) // 4 * 8 <= LDS_LIMIT:
        d += 32
    return d


_SSQ = (None, "random", "pow4", "clamp")


def _fc(id, form, C, N, m=8, k=5, dKP=0, ssq=None, x=True, np=0, Qb=0, rc=False, r8=False, qf=MIX):
    return FwdCase(id, form, C, N, m, k, dKP, ssq, x, np, Qb, rc, r8, qf)


@functools.lru_cache(maxsize=None)
def fwd_cases():
    out = []
    # ---- patch_rows_fwd_kernel (two rows per workgroup): one row; odd Q (the second half-workgroup of the last block idle); Q % 8 == 0
    # but N % 8 != 0; N % 8 == 0 but the LDS form beyond 100 KiB; four extra columns
    out.append(_fc("R-1x1", "row", 1, 1, ssq="random", qf=("random",)))
    out.append(_fc("R-3x5", "row", 3, 5, ssq="pow4"))
    out.append(_fc("R-2x12", "row", 2, 12, m=5, k=3))
    out.append(_fc("R-lds-too-large", "row", 1, 8, m=10, k=7, dKP=_kp_beyond_lds(10, 7), ssq="pow4"))
    out.append(_fc("R-wide", "row", 3, 5, k=3, dKP=4, ssq="clamp"))
    # ---- patch_rows_fwd_lds_kernel: one row group; 3 clouds (no remap); 8 clouds x 1 row group and 16 clouds x 3 row groups (remap);
    # the largest LDS that still takes this form; 32 extra columns
    out.append(_fc("L-1x8", "lds", 1, 8, ssq="random"))
    out.append(_fc("L-3x16", "lds", 3, 16))
    out.append(_fc("L-8x8", "lds", 8, 8, ssq="random"))
    out.append(_fc("L-16x24", "lds", 16, 24, ssq="clamp"))
    out.append(_fc("L-largest", "lds", 2, 8, m=10, k=7, ssq="random"))
    out.append(_fc("L-wide", "lds", 3, 16, k=3, dKP=32, ssq="pow4"))
    # ---- the sweep: every m and k through both forms, with and without ssq in turn
    for m in range(1, 11):
        for k in (1, 3, 5, 7):
            s = _SSQ[(m + (k - 1) // 2) % 4]
            out.append(_fc("R-m%dk%d" % (m, k), "row", 3, 13, m=m, k=k, ssq=s))
            out.append(_fc("L-m%dk%d" % (m, k), "lds", 3, 16, m=m, k=k, ssq=_SSQ[(m + (k - 1) // 2 + 2) % 4]))
    # ---- every face of every m with its float32 neighbours, and the specials, through both forms (k = 1: 32 columns)
    for m in range(1, 11):
        out.append(_fc("R-faces-m%d" % m, "row", 1, n_faces(m) | 1, m=m, k=1, qf=("faces",)))
        out.append(_fc("L-faces-m%d" % m, "lds", 1, n_faces(m, 8), m=m, k=1, ssq="random", qf=("faces",)))
    for np_ in (1, 3):
        t = "-np%d" % np_
        pl, p3 = "planes_lds%d" % np_, "planes3_%d" % np_
        # ---- patch_rows_planes_lds_kernel<np> (no fp32 rows, N % 8 == 0)
        out.append(_fc("PL-4x8-qb0" + t, pl, 4, 8, x=False, np=np_, Qb=0, rc=True, r8=True, ssq="random"))
        out.append(_fc("PL-4x8-qb32" + t, pl, 4, 8, x=False, np=np_, Qb=32, rc=True, r8=True))
        out.append(_fc("PL-8x8-qb32" + t, pl, 8, 8, x=False, np=np_, Qb=32, rc=True, r8=True, ssq="clamp"))      # remap, R8 for half the rows
        out.append(_fc("PL-16x16-qb128" + t, pl, 16, 16, x=False, np=np_, Qb=128, rc=True, r8=True, ssq="random"))
        out.append(_fc("PL-rc-only" + t, pl, 4, 8, x=False, np=np_, Qb=32, rc=True, ssq="pow4"))
        out.append(_fc("PL-r8-only" + t, pl, 4, 8, x=False, np=np_, Qb=32, r8=True, ssq="random"))
        out.append(_fc("PL-k1" + t, pl, 3, 16, m=2, k=1, x=False, np=np_, Qb=32, rc=True, r8=True, ssq="random"))
        out.append(_fc("PL-k3-m1" + t, pl, 3, 16, m=1, k=3, x=False, np=np_, Qb=32, rc=True, r8=True))
        out.append(_fc("PL-k7" + t, pl, 3, 16, m=5, k=7, x=False, np=np_, Qb=32, rc=True, r8=True, ssq="random"))
        # ---- patch_rows_planes3_kernel<np>: planes and fp32 rows together; row groups that straddle clouds (N = 12: the scale changes
        # inside a group), with and without fp32 rows; k = 7
        out.append(_fc("P3-4x8" + t, p3, 4, 8, np=np_, Qb=32, rc=True, r8=True, ssq="random"))
        out.append(_fc("P3-8x12-qb32" + t, p3, 8, 12, np=np_, Qb=32, rc=True, r8=True, ssq="random"))
        out.append(_fc("P3-8x12-qb64" + t, p3, 8, 12, x=False, np=np_, Qb=64, rc=True, r8=True, ssq="clamp"))
        out.append(_fc("P3-rc-only" + t, p3, 4, 8, k=3, np=np_, Qb=0, rc=True))
        out.append(_fc("P3-r8-only" + t, p3, 4, 8, k=3, np=np_, Qb=32, r8=True, ssq="pow4"))
        out.append(_fc("P3-k1" + t, p3, 8, 12, m=3, k=1, np=np_, Qb=64, rc=True, r8=True))
        out.append(_fc("P3-k7-rc" + t, p3, 4, 8, m=6, k=7, np=np_, Qb=32, rc=True, ssq="random"))
    # the three-plane LDS form within 1 KiB of the limit; the staging loop beyond five float4 per thread (m = 10, one plane)
    out.append(_fc("PL-m9k7-np3", "planes_lds3", 4, 8, m=9, k=7, x=False, np=3, Qb=32, rc=True, r8=True, ssq="random"))
    out.append(_fc("PL-m10-np1", "planes_lds1", 4, 8, m=10, k=3, x=False, np=1, Qb=32, rc=True, r8=True, ssq="random"))
    # three planes of m = 10 exceed the LDS form although no fp32 rows are wanted; k = 7 with row images: one plane fits, three are refused
    out.append(_fc("P3-m10-np3", "planes3_3", 4, 8, m=10, k=3, x=False, np=3, Qb=32, rc=True, r8=True, ssq="random"))
    out.append(_fc("P3-k7-r8-np1", "planes3_1", 4, 8, k=7, np=1, Qb=32, rc=True, r8=True, ssq="random"))
    out.append(_fc("P3-k7-r8-np3", "refused", 4, 8, k=7, np=3, Qb=32, rc=True, r8=True))
    # the faces through the plane forms: the gapped m
    out.append(_fc("PL-faces-m6-np1", "planes_lds1", 1, n_faces(6, 32), m=6, k=1, x=False, np=1, Qb=n_faces(6, 32) - 32, rc=True, r8=True, qf=("faces",)))
    out.append(_fc("PL-faces-m10-np1", "planes_lds1", 1, n_faces(10, 32), m=10, k=1, x=False, np=1, Qb=32, rc=True, r8=True, qf=("faces",)))
    out.append(_fc("PL-faces-m7-np3", "planes_lds3", 1, n_faces(7, 32), m=7, k=1, x=False, np=3, Qb=n_faces(7, 32), rc=True, r8=True, qf=("faces",)))
    out.append(_fc("PL-faces-m9-np3", "planes_lds3", 1, n_faces(9, 32), m=9, k=1, x=False, np=3, Qb=32, rc=True, r8=True, qf=("faces",)))
    out.append(_fc("P3-faces-m10-np3", "planes3_3", 1, n_faces(10, 32), m=10, k=1, x=False, np=3, Qb=n_faces(10, 32), rc=True, r8=True, qf=("faces",)))
    out.append(_fc("P3-faces-m6-np1", "planes3_1", 1, n_faces(6, 32), m=6, k=1, np=1, Qb=32, rc=True, r8=True, ssq="random", qf=("faces",)))
    # ---- planes offered but not taken (Q % 8, Qb % 32, KP % 32): the fp32 forms run and the plane buffers keep their fill;
    # without fp32 rows there is nothing to write: DPD_E_NULL
    for name, C, N, Qb, dKP, form in (("q", 3, 5, 0, 0, "row"), ("qb", 4, 8, 8, 0, "lds"), ("kp", 4, 8, 32, 4, "lds")):
        out.append(_fc("NT-" + name, form, C, N, dKP=dKP, np=3, Qb=Qb, rc=True, r8=True, ssq="random"))
        out.append(_fc("NT-%s-null" % name, "null", C, N, dKP=dKP, x=False, np=3, Qb=Qb, rc=True, r8=True))
    return tuple(out)


def fwd_case(cid):
    return next(c for c in fwd_cases() if c.id == cid)


FwdData = namedtuple("FwdData", "q fv ssq")
FwdRef = namedtuple("FwdRef", "look X")


@functools.lru_cache(maxsize=8)
def fwd_data(case):
    rng = _rng(case)
    q = np.concatenate([family(rng, case.qf[c % len(case.qf)], case.m, case.N) for c in range(case.C)])
    fv = rng.standard_normal((case.C, case.m ** 3, F)).astype(np.float32)
    return FwdData(*_frozen(q, fv, make_ssq(rng, case.C, case.ssq)))


@functools.lru_cache(maxsize=8)
def fwd_ref(case):
    d = fwd_data(case)
    return FwdRef(lookup(d.q, case.m), rowsref(case, d))


def rowsref(case, d):
    X = rows(d.q, d.fv, d.ssq, case.m, case.k, kp(case))
    X.setflags(write=False)
    return X


def _flat(x, device, dtype=torch.float32, fill=NAN_IN):
    view, chk = banded_flat(x.size, fill, dtype, device)
    view.copy_(torch.from_numpy(np.array(x).reshape(-1)))          # a copy: the shared data is read-only
    return view, chk


class _Run:
    def __init__(self):
        self.checks = []

    def _add(self, view_chk):
        self.checks.append(view_chk[1])
        return view_chk[0]

    def guards(self):
        for chk in self.checks:
            chk()


class FwdRun(_Run):
    """every buffer of one dpd_patch_rows_fwd_scaled call in its own guard-banded allocation: q [Q 3], fv, ssq (inputs, NaN around
    them); X [Q KP] (None when the case wants no fp32 rows), mask [Q], vox [Q] int32 (NAN_OUT); rc / r8 int16 [np Q KP] (NAN_OUT16)
    where offered -- r8 sized for ALL Q rows, so that a row group beyond Qb lands inside the buffer and is seen"""

    def __init__(self, case, device="cpu"):
        super().__init__()
        self.case, self.device = case, device
        self.data = d = fwd_data(case)
        Q, KP = case.C * case.N, kp(case)
        self.Q, self.KP = Q, KP
        self.q = self._add(_flat(d.q, device))
        self.fv = self._add(_flat(d.fv, device))
        self.ssq = None if d.ssq is None else self._add(_flat(d.ssq, device))
        self.X = self._add(banded_flat(Q * KP, device=device)) if case.x else None
        self.mask = self._add(banded_flat(Q, device=device))
        self.vox = self._add(banded_flat(Q, NAN_OUT, torch.int32, device))
        n16 = max(case.np, 1) * Q * KP
        self.rc = self._add(banded_flat(n16, NAN_OUT16, torch.int16, device)) if case.np and case.rc else None
        self.r8 = self._add(banded_flat(n16, NAN_OUT16, torch.int16, device)) if case.np and case.r8 else None

    def descriptor(self):
        """the hand-filled dpd_planes of the case (None without one)"""
        from dpdist_amd import lib as L
        if not self.case.np:
            return None
        pl = L.Planes()
        pl.np, pl.Q, pl.Qb = self.case.np, self.Q, self.case.Qb
        pl.X_rc = None if self.rc is None else self.rc.data_ptr()
        pl.X_r8 = None if self.r8 is None else self.r8.data_ptr()
        return pl


def check_fwd(run, code):
    """everything one forward call must leave behind; raises AssertionError otherwise"""
    case, d = run.case, run.data
    assert code == return_code(case), ("return code", code, return_code(case))
    outs = [("X", run.X, NAN_OUT), ("mask", run.mask, NAN_OUT), ("vox", run.vox, NAN_OUT), ("X_rc", run.rc, NAN_OUT16), ("X_r8", run.r8, NAN_OUT16)]
    if code != 0:
        for name, buf, fill in outs:
            assert buf is None or untouched(buf, fill), "%s written although the entry refused" % name
        run.guards()
        return
    ref = fwd_ref(case)
    Q, KP, np_, Qb = run.Q, run.KP, case.np, case.Qb
    same_bits(run.mask, ref.look.mask, "mask")
    same_bits(run.vox, ref.look.vox, "vox")
    if run.X is not None:
        same_bits(run.X.view(Q, KP), ref.X, "X", nan_any=True)
    if case.form.startswith("planes"):
        rc, r8 = planes(ref.X, np_, Qb)
        if run.rc is not None:
            same_bits(run.rc.view(np_, Q, KP), rc, "X_rc", nan_any=True)
        if run.r8 is not None:
            n = np_ * Qb * KP
            same_bits(run.r8[:n].view(np_, Qb // 8, KP, 8), r8, "X_r8", nan_any=True)
            assert untouched(run.r8[n:], NAN_OUT16), "X_r8 written beyond its Qb = %d rows" % Qb
    else:
        for name, buf in (("X_rc", run.rc), ("X_r8", run.r8)):
            assert buf is None or untouched(buf, NAN_OUT16), "%s written although the planes were not taken" % name
    same_bits(run.q, d.q.reshape(-1), "q (input)")
    same_bits(run.fv, d.fv.reshape(-1), "fv (input)")
    run.guards()


# ------------------------------------------------------------------------------------------------ backward cases
# voxf: where the voxel ids come from -- "mix" (the reference lookup of the mixed family: faces, specials, corners, random), "one" (every
# query in one voxel), "masked" (mostly masked queries, whose rows still carry dX); val: "int" (small integers, int64 reference) or
# "f32" (normals, n-ascending float32 reference); dq / dfv: which outputs are requested
BwdCase = namedtuple("BwdCase", "id C N m k dKP voxf val dq dfv")
BWD_N = (1, 8, 17, 64, 65, 130)
BWD_C = (1, 3)
_MK = ((1, 7), (10, 7), (9, 3), (2, 1), (5, 5), (8, 5), (8, 3), (10, 1), (2, 3), (5, 7), (9, 5), (1, 1))
BWD_CAP = 8192


@functools.lru_cache(maxsize=None)
def bwd_cases():
    out = []
    i = 0
    for N in BWD_N:
        for C in BWD_C:
            m, k = _MK[i % len(_MK)]
            i += 1
            for val in ("int", "f32"):
                out.append(BwdCase("B-%dx%d-m%dk%d-%s" % (C, N, m, k, val), C, N, m, k, 0, "mix", val, True, True))
    for val in ("int", "f32"):
        # every query in one voxel: 17 / 64 hits per 64-query block (more than one round of sixteen, a ragged last round)
        for N, m, k in ((17, 8, 5), (64, 8, 5), (64, 2, 7), (17, 10, 3)):
            out.append(BwdCase("B-one-%d-m%dk%d-%s" % (N, m, k, val), 2, N, m, k, 0, "one", val, True, True))
        out.append(BwdCase("B-masked-" + val, 3, 17, 5, 3, 0, "masked", val, True, True))
        out.append(BwdCase("B-wide-" + val, 3, 17, 8, 3, 36, "mix", val, True, True))
    out.append(BwdCase("B-dq-alone", 3, 17, 8, 5, 0, "mix", "f32", True, False))
    out.append(BwdCase("B-dfv-alone", 3, 17, 8, 5, 0, "mix", "f32", False, True))
    out.append(BwdCase("B-cap", 1, BWD_CAP, 2, 1, 24 - padded_width(1), "mix", "int", True, True))
    return tuple(out)


def bwd_case(cid):
    return next(c for c in bwd_cases() if c.id == cid)


BwdData = namedtuple("BwdData", "q look dX")


@functools.lru_cache(maxsize=8)
def bwd_data(case):
    """q (and its reference lookup) and dX [Q, KP]: the window columns and the three dq columns hold values, every column behind them a
    quiet NaN that nothing may read"""
    rng = _rng(case)
    C, N, m, KP, E = case.C, case.N, case.m, kp(case), E_of(case.k)
    if case.voxf == "one":
        q = np.concatenate([in_cell(rng, m, (0, m // 2, m - 1)[c % 3 + (1 if C == 2 else 0)], N) for c in range(C)])
    elif case.voxf == "masked":
        q = np.concatenate([family(rng, "specials", m, N - 2), family(rng, "random", m, 2)] * C)
    else:
        q = np.concatenate([family(rng, MIX[c % 3] if N >= 8 else "mix", m, N) for c in range(C)])
    look = lookup(q, m)
    if case.voxf == "masked":
        assert (look.mask == 0).sum() * 2 > len(q)
    dX = np.full((C * N, KP), NAN_IN, dtype=np.int32).view(np.float32)
    if case.val == "int":
        dX[:, :E + 3] = small_int(rng, (C * N, E + 3), N).astype(np.float32)
    else:
        dX[:, :E + 3] = rng.standard_normal((C * N, E + 3)).astype(np.float32)
    _frozen(q, dX)
    return BwdData(q, look, dX)


@functools.lru_cache(maxsize=8)
def bwd_ref(case):
    d = bwd_data(case)
    dfv, dq = bwd(d.dX, d.look.vox, case.C, case.N, case.m, case.k)
    if case.val == "int":
        exact = bwd_int(d.dX, d.look.vox, case.C, case.N, case.m, case.k)
        assert np.array_equal(dfv.astype(np.int64), exact)          # the float32 form is exact on this family
        dfv = exact.astype(np.float32)
    return dfv, dq


class BwdRun(_Run):
    """dX [Q KP], vox [Q] (inputs), dq [Q 3] and dfv [C m^3 F] (NAN_OUT; None when not requested), each between guard bands.
    dX / dq: another gradient on the case's queries / whether dq is requested, instead of the case's own"""

    def __init__(self, case, device="cpu", dX=None, dq=None):
        super().__init__()
        self.data = d = bwd_data(case)
        self.case = case = case if dq is None else case._replace(dq=dq)
        self.dX_np = d.dX if dX is None else dX
        self.dX = self._add(_flat(self.dX_np, device))
        self.vox = self._add(_flat(d.look.vox, device, torch.int32, NAN_OUT))
        self.dq = self._add(banded_flat(case.C * case.N * 3, device=device)) if case.dq else None
        self.dfv = self._add(banded_flat(case.C * case.m ** 3 * F, device=device)) if case.dfv else None


def check_bwd(run, ref=None):
    case = run.case
    dfv, dq = bwd_ref(case) if ref is None else ref
    if run.dfv is not None:
        same_bits(run.dfv.view(dfv.shape), dfv, "dfv")
    if run.dq is not None:
        same_bits(run.dq.view(dq.shape), dq, "dq")
    same_bits(run.dX, run.dX_np.reshape(-1), "dX (input)", nan_any=True)
    same_bits(run.vox, run.data.look.vox, "vox (input)")
    run.guards()


def onehot_columns(case, row):
    """columns of the one-hot adjoint of `row`: the first and the last window column, the centre of the window, one column of every corner
    neighbour (clipped for a query in a corner voxel) -- with the (cloud cell, channel) the forward reads each from, or None when
    the neighbour lies outside the grid"""
    d = bwd_data(case)
    m, k, h = case.m, case.k, (case.k - 1) // 2
    ix, iy, iz = (int(x) for x in d.look.idx[row])
    nbs = {(a, b, c) for a in (0, k - 1) for b in (0, k - 1) for c in (0, k - 1)} | {(h, h, h)}
    cols = {0, E_of(k) - 1} | {((a * k + b) * k + c) * F + (3 * a + 5 * b + 7 * c) % F for a, b, c in nbs}
    out = []
    for col in sorted(cols):
        nb, ch = divmod(col, F)
        d0, d1, d2 = nb // (k * k), (nb // k) % k, nb % k
        g = (iy + d0 - h, ix + d1 - h, iz + d2 - h)
        inside = all(0 <= x < m for x in g)
        out.append((col, ((g[0] * m + g[1]) * m + g[2], ch) if inside else None))
    return out


ONEHOT_CASES = (("B-3x17-m8k5-f32", (0, 20, 40)), ("B-1x8-m9k3-f32", (0, 7)), ("B-one-64-m2k7-f32", (64, 127)))


# ------------------------------------------------------------------------------------------------ combine and stack
CombineCase = namedtuple("CombineCase", "id B N k dKP scale")
COMBINE_SHAPES = ((1, 1), (3, 5), (2, 43))       # 2 B N 3 = 516: just above two workgroups of 256


def combine_cases():
    out = []
    for B, N in COMBINE_SHAPES:
        for k, dKP in ((1, 0), (5, 0), (5, 36)):
            for scale in (None, 0.375):
                out.append(CombineCase("C-%dx%d-k%d+%d-%s" % (B, N, k, dKP, "scaled" if scale else "plain"), B, N, k, dKP, scale))
    return tuple(out)


class CombineRun(_Run):
    """dpts [2 BN 3], dX [2 BN, KP] (only columns [E, E + 3) hold values, the rest a quiet NaN), scale [1] or None; gA, gB [BN 3]"""

    def __init__(self, case, device="cpu"):
        super().__init__()
        self.case = case
        rng = _rng(case)
        BN, KP, E = case.B * case.N, kp(case), E_of(case.k)
        self.BN = BN
        self.dpts_np = rng.standard_normal((2, BN, 3)).astype(np.float32)
        self.dX_np = np.full((2 * BN, KP), NAN_IN, dtype=np.int32).view(np.float32)
        self.dX_np[:, E:E + 3] = rng.standard_normal((2 * BN, 3)).astype(np.float32)
        self.dpts = self._add(_flat(self.dpts_np, device))
        self.dX = self._add(_flat(self.dX_np, device))
        self.scale = None if case.scale is None else self._add(_flat(np.array([case.scale], np.float32), device))
        self.gA = self._add(banded_flat(BN * 3, device=device))
        self.gB = self._add(banded_flat(BN * 3, device=device))

    def check(self):
        gA, gB = combine(self.dpts_np, self.dX_np, self.case.scale, self.BN, self.case.k)
        same_bits(self.gA.view(self.BN, 3), gA, "gA")
        same_bits(self.gB.view(self.BN, 3), gB, "gB")
        same_bits(self.dpts, self.dpts_np.reshape(-1), "dpts (input)")
        self.guards()


class StackRun(_Run):
    """pcA, pcB, noise [B N 3] (noise None without); pts, q [2 B N 3]"""

    def __init__(self, B, N, noise, device="cpu"):
        super().__init__()
        rng = np.random.default_rng([B, N, int(noise)])
        n = B * N * 3
        self.n = n
        self.a_np, self.b_np = (rng.uniform(-1, 1, size=n).astype(np.float32) for _ in range(2))
        self.noise_np = (rng.standard_normal(n) * 0.01).astype(np.float32) if noise else None
        self.pcA, self.pcB = self._add(_flat(self.a_np, device)), self._add(_flat(self.b_np, device))
        self.noise = self._add(_flat(self.noise_np, device)) if noise else None
        self.pts = self._add(banded_flat(2 * n, device=device))
        self.q = self._add(banded_flat(2 * n, device=device))

    def check(self):
        pts, q = stack(self.a_np, self.b_np, self.noise_np)
        same_bits(self.pts, pts, "pts")
        same_bits(self.q, q, "q")
        self.guards()


PADDED_WIDTHS = {1: 32, 3: 544, 5: 2528, 7: 6880, 9: 14592}

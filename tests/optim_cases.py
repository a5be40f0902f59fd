"""Exact-value cases of the optimizer and loss kernels (csrc/loss_adam.hip): references, state builders, guard-banded runs, the
checker and the case tables of tests/test_optim_edges_gpu.py (tests/test_optim_edges_cpu.py proves on the CPU that the checker has
teeth and that every table entry keeps the entry's own rules).  Not a test module and not a conftest.

The method.  The library is compiled with -ffp-contract=off and HIP's float32 division and square root are correctly rounded, so
`adam_f32`, a numpy-float32 restatement of adam_one in the same operation order, must agree with every Adam kernel BIT FOR BIT; it is
itself held to the first-order rounding bound `adam_bound` of the float64 statement `adam_f64`.  Two families of state:
  exact  b1 = b2 = 0.5, eps = 1, lr_t = 2^-3, gscale = 0.5 and integer-derived p, g, m, v for which every intermediate of one step is
         exactly representable (`exact_state`): float32, float64 and the closed form agree exactly, so "every element updated exactly
         once, from its own g, m, v" is an equality whatever the rounding;
  real   b1 = 0.9, b2 = 0.999, eps = 1e-8, gscale = 0.5, log-uniform magnitudes 1e-6 .. 10, 5 % zero gradients (`real_state`).
Every buffer a kernel reads or writes sits between guard bands (gemm_cases.banded_flat); outputs start as a NaN of a known bit pattern.
"""
import functools
import math
import zlib
from collections import namedtuple

import numpy as np
import torch

from .gemm_cases import NAN_IN, NAN_OUT, NAN_OUT16, banded, banded_flat, bf16_planes, untouched

EXACT = 1 << 24
U = 2.0 ** -24                     # unit round-off of float32
F32 = np.float32
CAPPED_N = 4 * 256 * 2048 + 4 * 256 * 3 + 3      # beyond the 2048-block cap: some threads take a second trip, then the scalar leftover

Consts = namedtuple("Consts", "lr_t b1 b2 eps gscale")
EXACT_CONSTS = Consts(F32(0.125), F32(0.5), F32(0.5), F32(1.0), F32(0.5))


def lr_t_of(t, lr=1e-3, b1=0.9, b2=0.999):
    """the caller's lr_t = lr sqrt(1 - b2^t) / (1 - b1^t), as a float32"""
    return F32(lr * math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t))


def real_consts(t):
    return Consts(lr_t_of(t), F32(0.9), F32(0.999), F32(1e-8), F32(0.5))


FAMILIES = {"exact": EXACT_CONSTS, "real_t1": real_consts(1), "real_t1000": real_consts(1000)}


def bits(x):
    """int32 / int16 bit patterns of a float32 / int16 numpy array or tensor (on the host)"""
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().contiguous().numpy()
    x = np.ascontiguousarray(x)
    return x.view(np.int32) if x.dtype == np.float32 else x


def same_bits(got, want, what):
    """bitwise equality of two arrays (so that -0 is not +0 and a NaN is compared by its payload)"""
    g, w = bits(got), bits(want)
    assert g.dtype == w.dtype and g.shape == w.shape, (what, g.dtype, g.shape, w.dtype, w.shape)
    if not np.array_equal(g, w):
        bad = np.argwhere(g != w)
        first = tuple(int(i) for i in bad[0])
        gf = np.asarray(got.cpu() if isinstance(got, torch.Tensor) else got)[first]
        raise AssertionError("%s: %d of %d elements differ; first at %s: got %r, want %r"
                             % (what, len(bad), g.size, list(first), gf, np.asarray(want)[first]))


# ------------------------------------------------------------------------------------------------ Adam references
def _c32(c):
    return tuple(F32(x) for x in c)


def adam_f32(p, g, m, v, lr_t, b1, b2, eps, gscale):
    """One step in numpy float32, in the operation order of adam_one / adam_tf_kernel:
         g' = g * gscale;  m = b1 m + (1 - b1) g';  v = b2 v + ((1 - b2) g') g';  p = p - (lr_t m) / (sqrt(v) + eps)
    every constant a float32, 1 - b1 computed in float32.  Returns (p, m, v)."""
    p, g, m, v = (np.asarray(x) for x in (p, g, m, v))
    assert all(x.dtype == np.float32 for x in (p, g, m, v))
    lr_t, b1, b2, eps, gscale = _c32((lr_t, b1, b2, eps, gscale))
    one = F32(1.0)
    gs = g * gscale
    m2 = b1 * m + (one - b1) * gs
    v2 = b2 * v + ((one - b2) * gs) * gs
    p2 = p - (lr_t * m2) / (np.sqrt(v2) + eps)
    assert all(x.dtype == np.float32 for x in (gs, m2, v2, p2))
    return p2, m2, v2


def _c64(lr_t, b1, b2, eps, gscale):
    """the float32 constants as float64; 1 - b is the float32 difference (exact for 0.5 <= b <= 1, asserted)"""
    lr_t, b1, b2, eps, gscale = _c32((lr_t, b1, b2, eps, gscale))
    o1, o2 = F32(1.0) - b1, F32(1.0) - b2
    assert np.float64(o1) == 1.0 - np.float64(b1) and np.float64(o2) == 1.0 - np.float64(b2)
    return tuple(np.float64(x) for x in (lr_t, b1, b2, eps, gscale, o1, o2))


def adam_f64(p, g, m, v, lr_t, b1, b2, eps, gscale):
    """the same step in float64 arithmetic on the same float32 inputs and constants.  Returns float64 (p, m, v)."""
    p, g, m, v = (np.asarray(x) for x in (p, g, m, v))
    assert all(x.dtype == np.float32 for x in (p, g, m, v))
    p, g, m, v = (x.astype(np.float64) for x in (p, g, m, v))
    lr_t, b1, b2, eps, gscale, o1, o2 = _c64(lr_t, b1, b2, eps, gscale)
    gs = g * gscale
    m2 = b1 * m + o1 * gs
    v2 = b2 * v + (o2 * gs) * gs
    p2 = p - (lr_t * m2) / (np.sqrt(v2) + eps)
    return p2, m2, v2


def adam_bound(p, g, m, v, lr_t, b1, b2, eps, gscale):
    """First-order bound of the float32 rounding error of one step against adam_f64, u = 2^-24.  With g' = g gscale, m', Vr = v', p' the
    float64 results, den = sqrt(Vr) + eps and D = lr_t m' / den the step:
        tol_m   = 4u (|b1 m| + |(1-b1) g'|)          roundings: g', each product, the sum -- at most 3 per term, 4 allowed
        tol_v   = 5u (b2 v + (1-b2) g'^2)            roundings: g' (twice in the second term), two products, the sum -- at most 4 per term
        tol_den = tol_v / (2 sqrt(Vr)) + 2u den      the error of v' through the square root, the root's and the sum's rounding
        tol_p   = 2u max(|p|, |p'|) + lr_t (tol_m / den + |m'| tol_den / den^2) + 4u |D|
                                                     the final difference's rounding; the errors of m' and den carried into the step; the
                                                     roundings of lr_t m', of the quotient (and second-order slack)
    Returns (tol_p, tol_m, tol_v)."""
    p64, m2, v2 = adam_f64(p, g, m, v, lr_t, b1, b2, eps, gscale)
    p, g, m, v = (np.asarray(x).astype(np.float64) for x in (p, g, m, v))
    lr_t, b1, b2, eps, gscale, o1, o2 = _c64(lr_t, b1, b2, eps, gscale)
    gs = g * gscale
    tol_m = 4 * U * (np.abs(b1 * m) + np.abs(o1 * gs))
    tol_v = 5 * U * (b2 * v + o2 * gs * gs)
    root = np.sqrt(v2)
    den = root + eps
    with np.errstate(divide="ignore", invalid="ignore"):
        through_root = np.where(root > 0, tol_v / (2 * root), 0.0)
    tol_den = through_root + 2 * U * den
    step = lr_t * m2 / den
    tol_p = 2 * U * np.maximum(np.abs(p), np.abs(p64)) + lr_t * (tol_m / den + np.abs(m2) * tol_den / den ** 2) + 4 * U * np.abs(step)
    return tol_p, tol_m, tol_v


def bound_ratio(p, g, m, v, consts):
    """largest err / tol of adam_f32 against adam_f64 over (p, m, v); 0 / 0 (an exact zero with a zero bound) counts as 0"""
    got = adam_f32(p, g, m, v, *consts)
    return ratio_to_bound(got, p, g, m, v, consts)


def ratio_to_bound(got, p, g, m, v, consts):
    want = adam_f64(p, g, m, v, *consts)
    tol = adam_bound(p, g, m, v, *consts)
    worst = 0.0
    for a, b, t in zip(got, want, tol):
        err = np.abs(np.asarray(a).astype(np.float64) - b)
        assert np.isfinite(err).all() and np.isfinite(t).all()
        assert not ((t == 0) & (err > 0)).any()
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(t > 0, err / t, 0.0)
        worst = max(worst, float(r.max()))
    return worst


# ------------------------------------------------------------------------------------------------ states
def exact_state(rng, n):
    """p, g, m, v (float32) of the exact family.  Per element: s in {0, 1, 3, 7}; g' an integer with |g'| <= floor(sqrt(2) s); g = 2 g';
    v = 2 s^2 - g'^2 (>= 0); m an even integer in [-16, 16]; p a multiple of 2^-8 in [-2, 2].  Then with EXACT_CONSTS
        m' = m/2 + g'/2,   v' = s^2,   sqrt(v') + eps = s + 1 (a power of two),   p' = p - m' / (8 (s + 1))
    and every intermediate is exactly representable (m' a multiple of 1/2 below 13, lr_t m' a multiple of 2^-4, the quotient a multiple of
    2^-7, p' a multiple of 2^-8 below 4): asserted here as adam_f32 == adam_f64 == the closed form.  s = 0 is the frozen / padding
    element: g = m = v = 0, p stays, m and v stay +0."""
    s = rng.choice(np.array([0, 1, 3, 7]), size=n)
    lim = np.floor(math.sqrt(2.0) * s).astype(np.int64)
    gp = rng.integers(-lim, lim + 1)
    v = 2 * s * s - gp * gp
    assert (v >= 0).all()
    m = 2 * rng.integers(-8, 9, size=n) * (s > 0)
    p = rng.integers(-512, 513, size=n) / 256.0
    st = tuple(x.astype(np.float32) for x in (p, 2 * gp, m, v))
    m2 = m / 2.0 + gp / 2.0
    closed = (p - m2 / (8.0 * (s + 1)), m2, (s * s).astype(np.float64))
    f32, f64 = adam_f32(*st, *EXACT_CONSTS), adam_f64(*st, *EXACT_CONSTS)
    for a, b, c in zip(f32, f64, closed):
        assert np.array_equal(a.astype(np.float64), b) and np.array_equal(b, c)
    frozen = s == 0
    for x in (f32[1], f32[2]):
        assert not bits(x)[frozen].any()                      # +0, not -0
    assert np.array_equal(bits(f32[0])[frozen], bits(st[0])[frozen])
    return st


TINY = 2.0 ** -60


def _log_uniform(rng, n, signed=True):
    x = np.exp(rng.uniform(math.log(1e-6), math.log(10.0), size=n))
    return (x * rng.choice(np.array([-1.0, 1.0]), size=n) if signed else x).astype(np.float32)


def real_state(rng, n, consts=None):
    """p, g, m (signed) and v (positive) log-uniform in magnitude over 1e-6 .. 10, 5 % of the gradients exactly zero.  With `consts`
    given, asserts that one step meets no denormal: no non-zero intermediate below 2^-60."""
    p, g, m = (_log_uniform(rng, n) for _ in range(3))
    v = _log_uniform(rng, n, signed=False)
    g[rng.random(n) < 0.05] = 0.0
    if consts is not None:
        assert_no_tiny(p, g, m, v, consts)
    return p, g, m, v


def assert_no_tiny(p, g, m, v, consts):
    lr_t, b1, b2, eps, gscale = _c32(consts)
    one = F32(1.0)
    gs = g * gscale
    p2, m2, v2 = adam_f32(p, g, m, v, *consts)
    mids = (gs, b1 * m, (one - b1) * gs, (one - b2) * gs, ((one - b2) * gs) * gs, b2 * v, m2, v2, lr_t * m2, np.sqrt(v2) + eps,
            (lr_t * m2) / (np.sqrt(v2) + eps), p2)
    for x in mids:
        a = np.abs(x[x != 0])
        assert np.isfinite(x).all() and (a.size == 0 or a.min() >= TINY)


# ------------------------------------------------------------------------------------------------ derived copies
def planes_of(p2d, np_):
    """Expected int16 bits of the operand planes of a float32 matrix [rows, cols]: (RC [np][rows][cols], R8 [np][rows/8][cols][8], where
    R8[q][rg][c][j] = plane q of row 8 rg + j, column c).  The planes are gemm_cases.bf16_planes (hi, mid, lo; round to nearest even)
    of the float32 values, as bfloat16 bit patterns; np = 1 is plane 0 alone."""
    p2d = np.asarray(p2d)
    assert p2d.dtype == np.float32 and p2d.ndim == 2 and p2d.shape[0] % 8 == 0 and np_ in (1, 3)
    rows, cols = p2d.shape
    pl = [torch.from_numpy(x).float() for x in bf16_planes(p2d)[:np_]]
    for x in pl:
        assert torch.equal(x.bfloat16().float(), x)
    rc = torch.stack([x.bfloat16().view(torch.int16) for x in pl])
    r8 = rc.view(np_, rows // 8, 8, cols).permute(0, 1, 3, 2).contiguous()
    return rc.numpy(), r8.numpy()


def tail_partials(rng, g_tail, loss_sums, nparts, rec):
    """Block partials [nparts][rec] (float32) whose column sums over the records are exactly g_tail (elements i < 4H+3) and, with
    loss_sums given (rec >= 4H+8), the three loss sums (elements 4H+4 .. 4H+6).  Records are random integers in [-4, 4], the last one
    fixes the sum; every partial sum in any order is bounded by sum_k |record_k| < 2^24 (asserted), so the 16-way strided sum is exact.
    Element 4H+3 and everything from 4H+7 on (without loss_sums: from 4H+4 on) holds NAN_IN."""
    g_tail = np.asarray(g_tail)
    T = len(g_tail)
    assert (T - 3) % 4 == 0 and rec >= T + 1 and nparts >= 1 and np.array_equal(g_tail, np.rint(g_tail))
    want = [g_tail.astype(np.int64)]
    cols = [np.arange(T)]
    if loss_sums is not None:
        assert rec >= T + 5 and len(loss_sums) == 3
        want.append(np.asarray(loss_sums, dtype=np.int64))
        cols.append(np.arange(T + 1, T + 4))
    want, cols = np.concatenate(want), np.concatenate(cols)
    recs = rng.integers(-4, 5, size=(nparts, len(cols)))
    recs[-1] = want - recs[:-1].sum(0)
    assert np.array_equal(recs.sum(0), want) and int(np.abs(recs).sum(0).max()) < EXACT
    out = np.full((nparts, rec), NAN_IN, dtype=np.int32).view(np.float32)
    out[:, cols] = recs.astype(np.float32)
    return out


def partial_sums(partials, T, with_loss):
    """exact column sums of the records (float64 of integers): the reduced gradient [T] and the three loss sums or None"""
    x = np.asarray(partials, dtype=np.float64)
    s = x[:, :T].sum(0)
    assert np.array_equal(s, np.rint(s)) and np.abs(x[:, :T]).sum(0).max() < EXACT
    return s.astype(np.float32), (x[:, T + 1:T + 4].sum(0) if with_loss else None)


def tail_loss(loss_sums, Qb):
    """float32 restatement of the tail block's loss: inv = 1 / Qb; loss[0] = s0 inv; loss[1] = (s1 inv + s2 inv) / 2"""
    s = np.asarray(loss_sums).astype(np.float32)
    inv = F32(1.0) / F32(Qb)
    return np.array([s[0] * inv, (s[1] * inv + s[2] * inv) / F32(2.0)], dtype=np.float32)


# ------------------------------------------------------------------------------------------------ L1 loss
def l1_case(BN, seed=0):
    """pred [2 BN, 3] and labels [BN] (float32): channel 0 and the labels multiples of 1/8 in [-4, 4] -- |pred - label| is a multiple of
    1/8 up to 8, so each of the three sums is an integer number of eighths below 64 BN < 2^24 (asserted) and exact in any order --
    channels 1 and 2 NAN_IN (never read); at least 10 % of the rows (and always row 0) have pred_AB == label."""
    assert 64 * BN < EXACT
    rng = np.random.default_rng([seed, BN])
    pred = np.full((2 * BN, 3), NAN_IN, dtype=np.int32).view(np.float32)
    pred[:, 0] = rng.integers(-32, 33, size=2 * BN) / 8.0
    labels = (rng.integers(-32, 33, size=BN) / 8.0).astype(np.float32)
    eq = rng.random(BN) < 0.15
    eq[0] = True
    eq[rng.permutation(BN)[:(BN + 9) // 10]] = True
    labels[eq] = pred[:BN, 0][eq]
    assert eq.sum() * 10 >= BN
    for x in (pred, labels):
        x.setflags(write=False)
    return pred, labels


def l1_ref(pred, labels, BN, mode, gscale):
    """float32 restatement of l1_loss_kernel: (loss [2], dpred or None).  inv = 1 / BN; loss[0] = sum |pab - label| inv;
    loss[1] = (sum pab inv + sum pba inv) / 2 (the sums are exact, see l1_case); dpred: mode 1 [BN, 3] = (sign(d) inv gscale, 0, 0),
    mode 2 [2 BN, 3] = (0.5 inv gscale, 0, 0)."""
    pab, pba = pred[:BN, 0].astype(np.float64), pred[BN:, 0].astype(np.float64)
    d = pab - labels.astype(np.float64)
    sl, sab, sba = (F32(x) for x in (np.abs(d).sum(), pab.sum(), pba.sum()))
    for x, y in ((sl, np.abs(d).sum()), (sab, pab.sum()), (sba, pba.sum())):
        assert np.float64(x) == y
    inv, gscale = F32(1.0) / F32(BN), F32(gscale)
    loss = np.array([sl * inv, (sab * inv + sba * inv) / F32(2.0)], dtype=np.float32)
    if mode == 0:
        return loss, None
    if mode == 1:
        dp = np.zeros((BN, 3), dtype=np.float32)
        dp[:, 0] = np.sign(d).astype(np.float32) * inv * gscale
    else:
        dp = np.zeros((2 * BN, 3), dtype=np.float32)
        dp[:, 0] = F32(0.5) * inv * gscale
    return loss, dp


L1_BN = (1, 2, 255, 256, 257, 1000)
L1_GSCALE = (1.0, 0.25)


class L1Run:
    """pred, labels, loss [2] and a dpred buffer of 2 BN rows, each between guard bands; `dpred_fn(run)` is the kernel"""

    def __init__(self, BN, mode, gscale, device="cpu", seed=0):
        self.BN, self.mode, self.gscale = BN, mode, gscale
        self.pred_np, self.labels_np = l1_case(BN, seed)
        self.pred, self.chk_pred = banded((2 * BN, 3), 3, NAN_IN, device=device)
        self.pred.copy_(torch.from_numpy(self.pred_np.copy()))
        self.labels, self.chk_labels = banded_flat(BN, NAN_IN, device=device)
        self.labels.copy_(torch.from_numpy(self.labels_np.copy()))
        self.loss, self.chk_loss = banded_flat(2, device=device)
        self.dpred, self.chk_dpred = banded((2 * BN, 3), 3, device=device)

    def check(self, dpred_given=True):
        loss, dp = l1_ref(self.pred_np, self.labels_np, self.BN, self.mode, self.gscale)
        same_bits(self.loss, loss, "loss")
        written = 0 if dp is None else dp.shape[0]
        if written:
            assert dpred_given
            same_bits(self.dpred[:written], dp, "dpred")
        assert untouched(self.dpred[written:]), "dpred rows beyond the mode's were written"
        same_bits(self.pred, self.pred_np, "pred (input)")
        same_bits(self.labels, self.labels_np, "labels (input)")
        for chk in (self.chk_pred, self.chk_labels, self.chk_loss, self.chk_dpred):
            chk()


# ------------------------------------------------------------------------------------------------ fused cases
Mat = namedtuple("Mat", "off rows cols wt rc r8")      # wt / rc / r8: whether that copy's buffer is passed
Tail = namedtuple("Tail", "H nparts rec loss pad")     # loss: whether `loss` is passed; pad: zero elements behind the tail (0 .. 3)
FusedCase = namedtuple("FusedCase", "id n mats np tail")


def tail_len(t):
    return 4 * t.H + 3


def tail_off(case):
    return case.n - case.tail.pad - tail_len(case.tail)


def tail_qb(t):
    return 8 * t.nparts - 3


def is_listed(case, mat):
    """the entry treats a matrix as a matrix when it has a transposed copy or (np != 0) a plane buffer; else it is vector elements"""
    return mat.wt or (case.np != 0 and (mat.rc or mat.r8))


def case_rules(case):
    """the entry's own rules (dpd_adam_tf_fused), asserted on a table entry"""
    at = 0
    assert case.n > 0 and case.np in (0, 1, 3) and len(case.mats) <= 3
    for mt in case.mats:
        if not is_listed(case, mt):
            assert case.np == 0
            continue
        assert mt.rows > 0 and mt.cols > 0 and mt.cols % 64 == 0 and mt.rows % 4 == 0 and mt.off % 4 == 0
        if case.np and (mt.rc or mt.r8):
            assert mt.rows % 8 == 0
        assert mt.off >= at, "offsets ascend"
        at = mt.off + mt.rows * mt.cols
        assert at <= case.n
    if case.tail is not None:
        t = case.tail
        assert t.H > 0 and t.H % 4 == 0 and t.nparts > 0 and 0 <= t.pad <= 3 and t.rec >= 4 * t.H + 4
        assert tail_off(case) >= at, "the tail lies behind the last matrix and ends the buffer"
        if t.loss:
            assert t.rec >= 4 * t.H + 8 and tail_qb(t) > 0
    gaps = 0
    at = 0
    for mt in case.mats:
        if is_listed(case, mt):
            gaps += mt.off > at
            at = mt.off + mt.rows * mt.cols
    end = tail_off(case) if case.tail is not None else case.n
    gaps += end > at
    assert gaps <= 5


def _vec(n):
    return FusedCase("V-%d" % n, n, (), 0, None)


PLAIN_N = (1, 3, 4, 5, 1023, 1024, 1028, CAPPED_N)          # dpd_adam_tf / dpd_adam_tf_dev
_M3 = (Mat(4, 64, 64, True, False, False), Mat(4112, 4, 192, True, False, False), Mat(4892, 132, 64, True, False, False))
_D2 = 12 + 24 * 256
_T2 = ((4 * 12 + 4, False, 2), (4 * 12 + 8, False, 0), (4 * 12 + 12, True, 1))      # (rec, loss given, padding)


def fused_cases():
    """the table of the issue: the smallest shapes that reach each branch of adam_fused_kernel and of its host side"""
    out = [_vec(n) for n in (1, 3, 4, 5, 1028, CAPPED_N)]
    # one tile block and no vector block; 4 of the 64 tile rows live
    out.append(FusedCase("M1", 256, (Mat(0, 4, 64, True, False, False),), 0, None))
    # partial last row tile, a leading and a trailing range, scalar leftover
    out.append(FusedCase("M2", 8 + 68 * 128 + 5, (Mat(8, 68, 128, True, False, False),), 0, None))
    # three matrices, four vector ranges, tile indexing across tile_end
    out.append(FusedCase("M3", 4892 + 132 * 64 + 2, _M3, 0, None))
    # the middle matrix has no copy (its plane pointers are passed, but np = 0 ignores them): it falls to the vector role
    out.append(FusedCase("M4", 4892 + 132 * 64 + 2, (_M3[0], Mat(4112, 4, 192, False, True, True), _M3[2]), 0, None))
    for np_ in (1, 3):
        # direct path, one unit: three waves leave early
        out.append(FusedCase("D1-np%d" % np_, 1024, (Mat(0, 8, 128, False, True, True),), np_, None))
        # six units over two blocks, the permlane32_swap R8 store, either layout absent
        for name, rc, r8 in (("both", True, True), ("rc", True, False), ("r8", False, True)):
            out.append(FusedCase("D2-%s-np%d" % (name, np_), _D2 + 3, (Mat(12, 24, 256, False, rc, r8),), np_, None))
        # LDS-tile plane path (cols % 128 != 0), partial row tile
        out.append(FusedCase("L1a-np%d" % np_, 512, (Mat(0, 8, 64, False, True, True),), np_, None))
        out.append(FusedCase("L1b-np%d" % np_, 72 * 192, (Mat(0, 72, 192, False, True, True),), np_, None))
        # a transposed copy and planes together
        out.append(FusedCase("L2-np%d" % np_, 4 + 72 * 128, (Mat(4, 72, 128, True, True, True),), np_, None))
    # the three block forms in one grid, gaps of 4
    out.append(FusedCase("X", 7180, (Mat(0, 8, 128, False, True, True), Mat(1028, 8, 192, False, True, True),
                                     Mat(2568, 72, 64, True, True, True)), 3, None))
    # the tail role alone: the loss block is block 1; the 16-way strided sum around 16 records
    for nparts in (1, 15, 16, 17, 40):
        for pad in (0, 3):
            out.append(FusedCase("T1-%d-pad%d" % (nparts, pad), 19 + pad, (), 0, Tail(4, nparts, 24, True, pad)))
    # the record forms: 4H+4 (no loss sums), 4H+8 without a loss, 4H+12 with one
    for rec, loss, pad in _T2:
        out.append(FusedCase("T2-rec%d" % rec, 51 + pad, (), 0, Tail(12, 17, rec, loss, pad)))
    # matrices, a 5-element gap (so tail_off % 4 != 0) and the tail, at the trainer's smallest fused H
    out.append(FusedCase("T3", 4 + 68 * 64 + 5 + 1027 + 1, (Mat(4, 68, 64, True, False, False),), 0, Tail(256, 40, 1032, True, 1)))
    # planes and the tail in one launch, the tail right behind the matrix
    out.append(FusedCase("T4", _D2 + 51 + 3, (Mat(12, 24, 256, False, True, True),), 3, Tail(12, 17, 56, True, 3)))
    return out


def case_by_id(cid):
    return next(c for c in fused_cases() if c.id == cid)


TWO_STEP_CASES = ("M3", "T3")


# ------------------------------------------------------------------------------------------------ state of a case
State = namedtuple("State", "p g m v partials loss_sums")      # g: the gradient the update sees (the tail holds the exact column sums)


@functools.lru_cache(maxsize=4)
def make_state(case, family):
    """the shared, read-only state of (case, family): p, g, m, v [n]; with a tail, its gradient is integer-valued (it is a sum of integer
    records) and `partials` are the records; the padding elements behind the tail are zero in all four"""
    consts = FAMILIES[family]
    rng = np.random.default_rng([zlib.crc32(repr(case).encode()), zlib.crc32(family.encode())])
    p, g, m, v = exact_state(rng, case.n) if family == "exact" else real_state(rng, case.n)
    partials = loss_sums = None
    if case.tail is not None:
        t, off, T = case.tail, tail_off(case), tail_len(case.tail)
        if family != "exact":
            g[off:off + T] = rng.integers(-9, 10, size=T)
        for x in (p, g, m, v):
            x[off + T:] = 0.0
        with_sums = t.rec >= 4 * t.H + 8 and t.loss
        loss_sums = rng.integers(-4 * tail_qb(t), 4 * tail_qb(t) + 1, size=3) if with_sums else None
        partials = tail_partials(rng, g[off:off + T], loss_sums, t.nparts, t.rec)
    if family != "exact":
        assert_no_tiny(p, g, m, v, consts)
    for x in (p, g, m, v, partials):
        if x is not None:
            x.setflags(write=False)
    return State(p, g, m, v, partials, loss_sums)


def _flat(x, device, fill=NAN_IN):
    view, chk = banded_flat(len(x), fill, device=device)
    view.copy_(torch.from_numpy(np.array(x)))          # a copy: the shared state is read-only
    return view, chk


class FusedRun:
    """every buffer of one dpd_adam_tf_fused call, each in its own guard-banded allocation:
      p, g, m, v [n]; WT[i] [cols*rows] float32 (NAN_OUT), rc[i] / r8[i] [3*rows*cols] int16 (NAN_OUT16) where the case passes them,
      else None; partials [nparts*rec] and loss [2] (NAN_OUT) with a tail.  Before a fused call the tail of g holds NAN_IN (the kernel
      writes it without reading it); `prefill_tail` puts the exact sums there instead (for the entries without a tail role)."""

    def __init__(self, case, family, device="cpu", lr_ts=None, prefill_tail=False, state=None):
        self.case, self.family, self.consts, self.device = case, family, FAMILIES[family], device
        self.state = st = make_state(case, family) if state is None else state
        assert len(st.p) == case.n
        self.lr_ts = tuple(F32(x) for x in (lr_ts if lr_ts is not None else (self.consts.lr_t,)))
        self.prefill_tail = prefill_tail
        self.checks = []
        g0 = st.g.copy()
        if case.tail is not None and not prefill_tail:
            g0[tail_off(case):tail_off(case) + tail_len(case.tail)].view(np.int32)[:] = NAN_IN
        self.p, self.g, self.m, self.v = (self._add(_flat(x, device)) for x in (st.p, g0, st.m, st.v))
        self.WT, self.rc, self.r8 = [], [], []
        for mt in case.mats:
            cnt = mt.rows * mt.cols
            self.WT.append(self._add(banded_flat(cnt, NAN_OUT, device=device)) if mt.wt else None)
            self.rc.append(self._add(banded_flat(3 * cnt, NAN_OUT16, torch.int16, device)) if mt.rc else None)
            self.r8.append(self._add(banded_flat(3 * cnt, NAN_OUT16, torch.int16, device)) if mt.r8 else None)
        self.partials = self.loss = None
        if case.tail is not None and not prefill_tail:
            self.partials = self._add(_flat(st.partials.reshape(-1), device))
            if case.tail.loss:
                self.loss = self._add(banded_flat(2, NAN_OUT, device=device))

    def _add(self, view_chk):
        self.checks.append(view_chk[1])
        return view_chk[0]


def vector_form(case):
    """the same flat buffer with no matrix listed and the tail's gradient already reduced: what dpd_adam_tf sees of the case"""
    return case._replace(id=case.id + "-plain", mats=(), np=0)


def run_fused_case(case, family, step_fn, device="cpu", lr_ts=None, prefill_tail=False, state=None):
    """lay the case out, call step_fn(run, lr_t) once per lr_t (on the GPU: the C entry; on the CPU: a stand-in), return the run"""
    run = FusedRun(case, family, device, lr_ts, prefill_tail, state)
    for lr_t in run.lr_ts:
        step_fn(run, lr_t)
    return run


def expected_state(run):
    """p, m, v after the run's steps: adam_f32 over all of [0, n), the tail's g being the exact column sums of the records"""
    st, c = run.state, run.consts
    p, m, v = st.p, st.m, st.v
    for lr_t in run.lr_ts:
        p, m, v = adam_f32(p, st.g, m, v, lr_t, *c[1:])
    return p, m, v


def check_fused(run, tail_role=True):
    """Everything one fused call (or a plain entry on a vector-only case) must leave behind; raises AssertionError otherwise.
    tail_role = False: the entry has no tail role (the plain entries on a pre-filled gradient): no partials, no loss."""
    case, st, c = run.case, run.state, run.consts
    has_tail = case.tail is not None and tail_role and not run.prefill_tail
    p, m, v = expected_state(run)
    if case.tail is not None:
        off, T = tail_off(case), tail_len(case.tail)
        sums, lsum = partial_sums(st.partials[:, :], T, st.loss_sums is not None)      # independent of the builder: from the records
        same_bits(st.g[off:off + T], sums, "column sums of the records against the state's tail gradient")
    got = [x.detach().cpu().numpy() for x in (run.p, run.m, run.v)]
    for name, a, b in zip("pmv", got, (p, m, v)):
        same_bits(a, b, name)
    if run.family != "exact" and len(run.lr_ts) == 1:
        r = ratio_to_bound(got, st.p, st.g, st.m, st.v, c)
        assert r <= 1.0, ("beyond the float64 rounding bound", r)
    same_bits(run.g, st.g, "g (unchanged outside the tail, the exact column sums inside it)")
    if case.tail is not None:
        for name, a in zip("pmv", got):
            assert not bits(a)[off + T:].any(), "padding element of %s behind the tail is no longer +0" % name
    for i, mt in enumerate(case.mats):
        cnt = mt.rows * mt.cols
        w = p[mt.off:mt.off + cnt].reshape(mt.rows, mt.cols)
        listed = is_listed(case, mt)
        if mt.wt:
            same_bits(run.WT[i].view(mt.cols, mt.rows), np.ascontiguousarray(w.T), "WT[%d]" % i)
        for name, buf, k in (("W_rc", run.rc[i], 0), ("W_r8", run.r8[i], 1)):
            if buf is None:
                continue
            if not (listed and case.np):
                assert untouched(buf, NAN_OUT16), "%s[%d] written although np = 0" % (name, i)
                continue
            want = planes_of(w, case.np)[k]
            same_bits(buf[:case.np * cnt].view(want.shape), want, "%s[%d]" % (name, i))
            assert untouched(buf[case.np * cnt:], NAN_OUT16), "%s[%d]: a plane beyond np = %d was written" % (name, i, case.np)
    if has_tail:
        same_bits(run.partials, st.partials.reshape(-1), "partials (input)")
        if run.loss is not None:
            assert lsum is not None
            same_bits(run.loss, tail_loss(lsum, tail_qb(case.tail)), "loss")
    for chk in run.checks:
        chk()

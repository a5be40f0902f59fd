"""Cases, float32 restatement and float64 oracle of the all-pairs Chamfer / Hausdorff matrices (dpd_chamfer_matrix_fwd / _bwd,
dpdist_amd/baselines.py), shared by tests/test_baseline_matrix_cpu.py and tests/test_baseline_matrix_gpu.py.  Not a test module.

The restatement: d2 = (dx*dx + dy*dy) + dz*dz with d? = q? - s? in numpy float32 is the kernel's arithmetic operation by operation (no
fusion on either side), so d2, its minima, max_sq and sqrtf (correctly rounded on both sides) are BIT-EXACT references.  The oracle:
means and gradients in float64 over the float32 minima / argmins (np.argmin: the lowest index, the kernel's tie rule), exact-zero
minima skipped in the sqrt form.  The bars (u = 2^-24):
  directed mean over n real queries   |got - ref| <= (n + 2) u ref      fp32 sum of n non-negative terms in any order (n - 1) u, sqrtf
                                                                        u/2, the division u, margin u/2
  D = (D_AB + D_BA) / 2               (max(n_ab, n_ba) + 3) u ref       one more rounding for the sum of the two (the halving is exact)
  gradient element                    (T + c) u S, exactly 0 if S = 0   T terms summed into the element, S the float64 sum of their
                                                                        absolute values; c = 4 (squared: the difference, the product
                                                                        with 2, the weight's division and product), c = 8 (sqrt: d2's
                                                                        roundings and the hardware reciprocal square root on top)
"""
import numpy as np

U = 2.0 ** -24
F = np.float32

# (seed, Ca, Cb, N, M, countsA, countsB)
CASES = {
    "full": (0, 3, 2, 64, 64, None, None),
    "ragged": (1, 3, 2, 37, 70, [37, 5, 1], [70, 33]),
    "chunks": (2, 2, 3, 300, 257, [300, 256], [257, 1, 129]),       # more than one 256-point chunk, a partial last one, a one-point cloud
    "cap": (3, 1, 1, 4096, 64, None, None),
}
MANY = (4, 2, 65537, 2, 1)                                          # more clouds than a grid's y / z dimension holds
SELF = (5, 4, 40)                                                   # a set against itself
# the query route keeps 4, 2 or 1 queries per thread, whichever still gives 512 workgroups: (seed, Cs, Ns, Cq, Nq) run on all 512 query
# clouds (4 per thread), on the first 300 (2) and on the first 100 (1); the counts leave waves with 4, 3, 2 and 1 live queries
QUERIES = (6, 2, 7, 512, 1024)
QUERIES_COUNTS_S = [7, 5]
QUERIES_COUNTS_Q = [1024, 700, 513, 300, 1, 769, 256, 257]          # repeated over the 512 clouds
QUERIES_SUBSETS = (512, 300, 100)
STRIDE = (7, (1 << 20) + 3, 1, 1, 1)                                # more clouds than workgroups of one launch: the kernels stride
CAPS = (8, 1, 1, 4096, 4096)                                        # both widths at the cap: the surface route's 64 KB of LDS


def d2_f32(x, y):
    """x [n,3], y [m,3] float32 -> [n,m] float32: |x_i - y_j|^2 in the kernel's order, every operation rounded to float32"""
    d = (x[:, None, :] - y[None, :, :]).astype(F)
    return ((d[..., 0] * d[..., 0]).astype(F) + (d[..., 1] * d[..., 1]).astype(F)).astype(F) + (d[..., 2] * d[..., 2]).astype(F)


def draw(seed, Ca, Cb, N, M):
    r = np.random.default_rng(seed)
    A = r.uniform(-0.9, 0.9, (Ca, N, 3)).astype(F)
    B = r.uniform(-0.9, 0.9, (Cb, M, 3)).astype(F)
    return A, B


def make(name):
    """-> (A, B, countsA, countsB) with the planted edges; counts are lists (a full set: its width per cloud)"""
    seed, Ca, Cb, N, M, cA, cB = CASES[name]
    A, B = draw(seed, Ca, Cb, N, M)
    A[0, 1] = A[0, 0]                                               # a duplicate surface point: every tie goes to index 0
    if name == "full":
        B[0] = A[0]                                                 # minima exactly 0: D_AB[0,0] = D_BA[0,0] = 0, sqrt-form gradient 0
    return A, B, list(cA or [N] * Ca), list(cB or [M] * Cb)


def make_many():
    seed, Ca, Cb, N, M = MANY
    return draw(seed, Ca, Cb, N, M)


def make_queries():
    """-> (S, Q, countsS, countsQ) of the QUERIES case"""
    seed, Cs, Ns, Cq, Nq = QUERIES
    S, Q = draw(seed, Cs, Cq, Ns, Nq)
    return S, Q, list(QUERIES_COUNTS_S), (QUERIES_COUNTS_Q * (Cq // len(QUERIES_COUNTS_Q) + 1))[:Cq]


def make_self():
    seed, C, N = SELF
    return draw(seed, C, 1, N, 1)[0]


def ties(S, Q):
    """queries of Q [nq,3] whose fp32 minimum over S [ns,3] is attained by two points with DIFFERENT coordinates (a duplicated point is
    one point twice: np.argmin and the kernel both take its lowest index)"""
    d = d2_f32(Q, S)
    hit = d == d.min(1, keepdims=True)
    first = S[d.argmin(1)]                                          # [nq,3]
    other = (S[None, :, :] != first[:, None, :]).any(-1)            # [nq,ns]: a point that is not a copy of the argmin point
    return int((hit & other).any(1).sum())


def directed_fwd(S, cS, Q, cQ):
    """-> dict of [Cs,Cq] arrays: max_sq (float32, exact), mean_sq / mean_rt (float64 oracle), n (real queries per pair)"""
    Cs, Cq = len(cS), len(cQ)
    out = {"max_sq": np.zeros((Cs, Cq), F), "mean_sq": np.zeros((Cs, Cq)), "mean_rt": np.zeros((Cs, Cq)), "n": np.zeros((Cs, Cq), int)}
    for i in range(Cs):
        for j in range(Cq):
            mn = d2_f32(Q[j, :cQ[j]], S[i, :cS[i]]).min(1)
            out["max_sq"][i, j] = mn.max()
            out["mean_sq"][i, j] = mn.astype(np.float64).mean()
            out["mean_rt"][i, j] = np.sqrt(mn.astype(np.float64)).mean()
            out["n"][i, j] = cQ[j]
    return out


class Grad:
    """a float64 gradient [C,N,3] with, per element, the number of terms T [C,N,1] and the sum of their absolute values S [C,N,3]"""

    def __init__(self, shape):
        self.g, self.S, self.T = np.zeros(shape), np.zeros(shape), np.zeros(shape[:2] + (1,))

    def __add__(self, o):
        r = Grad(self.g.shape)
        r.g, r.S, r.T = self.g + o.g, self.S + o.S, self.T + o.T
        return r


def directed_bwd(S, cS, Q, cQ, form, W):
    """float64 oracle of dpd_chamfer_matrix_bwd -> (surface route, query route) as Grad; form 0 squared, 1 sqrt; W [Cs,Cq]"""
    gS, gQ = Grad(S.shape), Grad(Q.shape)
    for i in range(len(cS)):
        for j in range(len(cQ)):
            s, q = S[i, :cS[i]], Q[j, :cQ[j]]
            d = d2_f32(q, s)
            arg, mn = d.argmin(1), d.min(1)
            diff = q.astype(np.float64) - s[arg].astype(np.float64)                     # [nq,3]
            if form == 0:
                t = 2.0 * diff
                live = np.ones(len(q), bool)
            else:
                live = mn != 0
                norm = np.sqrt((diff ** 2).sum(1, keepdims=True))
                t = np.where(live[:, None], diff / np.where(norm == 0, 1.0, norm), 0.0)
            t = t * (float(W[i, j]) / cQ[j])
            gQ.g[j, :cQ[j]] += t
            gQ.S[j, :cQ[j]] += np.abs(t)
            gQ.T[j, :cQ[j], 0] += live
            np.add.at(gS.g[i], arg, -t)
            np.add.at(gS.S[i], arg, np.abs(t))
            np.add.at(gS.T[i, :, 0], arg, live.astype(np.float64))
    return gS, gQ


def _full_scan(S, Q):
    """full sets, all pairs at once (for many tiny clouds): d2 [Cs,Cq,Nq,Ns] float32 in the kernel's order"""
    d = (Q[None, :, :, None, :] - S[:, None, None, :, :]).astype(F)
    return ((d[..., 0] * d[..., 0]).astype(F) + (d[..., 1] * d[..., 1]).astype(F)).astype(F) + (d[..., 2] * d[..., 2]).astype(F)


def full_fwd(S, Q):
    """directed_fwd for full sets, vectorised over the pairs"""
    mn = _full_scan(S, Q).min(3)                                                        # [Cs,Cq,Nq]
    return {"max_sq": mn.max(2), "mean_sq": mn.astype(np.float64).mean(2), "mean_rt": np.sqrt(mn.astype(np.float64)).mean(2),
            "n": np.full(mn.shape[:2], Q.shape[1])}


def full_bwd(S, Q, form, W):
    """directed_bwd for full sets, vectorised over the pairs"""
    d = _full_scan(S, Q)
    arg, mn = d.argmin(3), d.min(3)                                                     # [Cs,Cq,Nq]
    i = np.arange(S.shape[0])[:, None, None]
    diff = Q[None].astype(np.float64) - S[i, arg].astype(np.float64)                   # [Cs,Cq,Nq,3]
    if form == 0:
        t, live = 2.0 * diff, np.ones(mn.shape, bool)
    else:
        live = mn != 0
        norm = np.sqrt((diff ** 2).sum(-1, keepdims=True))
        t = np.where(live[..., None], diff / np.where(norm == 0, 1.0, norm), 0.0)
    t = t * (W[:, :, None, None].astype(np.float64) / Q.shape[1])
    gS, gQ = Grad(S.shape), Grad(Q.shape)
    gQ.g, gQ.S, gQ.T = t.sum(0), np.abs(t).sum(0), live.sum(0)[..., None].astype(np.float64)
    ii = np.broadcast_to(i, arg.shape)
    np.add.at(gS.g, (ii, arg), -t)
    np.add.at(gS.S, (ii, arg), np.abs(t))
    np.add.at(gS.T[..., 0], (ii, arg), live.astype(np.float64))
    return gS, gQ


def matrix_bwd(A, cA, B, cB, form, G=None, Gab=None, Gba=None):
    """float64 oracle of ChamferMatrix's backward under upstreams on D, D_AB, D_BA ([Ca,Cb] each, None = absent) -> (Grad A, Grad B)"""
    z = np.zeros((len(cA), len(cB)))
    Wab = (z if G is None else G / 2.0) + (z if Gab is None else Gab)
    Wba = ((z if G is None else G / 2.0) + (z if Gba is None else Gba)).T
    sA, qB = directed_bwd(A, cA, B, cB, form, Wab)
    sB, qA = directed_bwd(B, cB, A, cA, form, Wba)
    return sA + qA, qB + sB


def mean_ok(got, ref, n, extra=2, scale=1.0):
    """the bar of a mean: elementwise |got - ref| <= scale (n + extra) u ref -> (ok, worst error / bar)"""
    bar = scale * (np.asarray(n, np.float64) + extra) * U * ref
    err = np.abs(np.asarray(got, np.float64) - ref)
    ratio = float(np.max(np.where(bar > 0, err / np.where(bar > 0, bar, 1.0), np.where(err == 0, 0.0, np.inf))))
    return bool((err <= bar).all()), ratio


def grad_ok(got, ref, c):
    """the bar of a gradient: |got - ref.g| <= (T + c) u S, and exactly 0 where S = 0 -> (ok, worst error / bar)"""
    bar = (ref.T + c) * U * ref.S
    err = np.abs(np.asarray(got, np.float64) - ref.g)
    zero = ref.S == 0
    ok = bool((err[~zero] <= bar[~zero]).all()) and bool((np.asarray(got)[zero] == 0).all())
    ratio = float((err[~zero] / bar[~zero]).max()) if (~zero).any() else 0.0
    return ok, ratio


def padded(X, counts, width, fill_bits=0x7FC00000):
    """X [C,N,3] cut to counts and re-padded to `width` columns with a quiet NaN (the kernels never read padding)"""
    out = np.full((X.shape[0], width, 3), np.uint32(fill_bits).view(F), F)
    out.view(np.uint32)[:] = fill_bits
    for c, n in enumerate(counts):
        out[c, :n] = X[c, :n]
    return out

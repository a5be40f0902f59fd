"""The paired Chamfer entries (csrc/chamfer.hip: dpd_chamfer_fwd / _bwd, dpd_chamfer_sqrt_fwd / _bwd) restated in numpy float32, in the
kernels' own order of operations, so that a test can compare bit patterns:

    pair distance   (dx dx + dy dy) + dz dz, every operation rounded to float32 (the library is built without contraction)
    minimum         an ascending scan with a strict <: the lowest index among equal distances
    loss            thread t of 256 sums the elements t, t + 256, ... in that order from 0, the 256 partial sums go through a halving
                    tree (slot t += slot t + o for o = 128, 64, ..., 1), then (sum_a / na + sum_b / nb) / 2
    gradient        w_x = gscale / (2 B n_x); the query route (the point's own nearest neighbour) first, then every point of the other
                    cloud whose nearest neighbour this point is, in ascending order
                      squared form   the query route is ASSIGNED (w_x 2) (x - y), a hit adds (w_y 2) (x - y)
                      sqrt form      both are added to 0: (w / sqrt(d)) (x - y) with the IEEE square root and division, nothing where d is 0

The inputs lie on a dyadic grid (multiples of 2^-6, or of 2^-2 for the coarse case, in [-1, 1]): every squared distance is exact, and equal
distances, duplicated points and coincident pairs occur.  A case with `plant` holds, in every pair, one point shared by both clouds
that is no other point's nearest neighbour (checked here): its squared-form gradient is a signed zero, which pins the assignment."""
import functools

import numpy as np

F = np.float32
FORMS = ("squared", "sqrt")
#        name: (B, N, M, grid step, plant a coincident pair)
CASES = {"b1_1_1": (1, 1, 1, 2.0 ** -6, False),
         "b2_5_3": (2, 5, 3, 2.0 ** -6, True),
         "b2_64_64_coarse": (2, 64, 64, 2.0 ** -2, False),
         "b2_257_300": (2, 257, 300, 2.0 ** -6, True),          # two chunks each way, tail lanes
         "b1_513_40": (1, 513, 40, 2.0 ** -6, False)}           # three chunks against one
GSCALES = (1.0, -1.5)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(a [B,N,3], b [B,M,3]) float32, read-only"""
    B, N, M, step, plant = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name) + 11)
    k = int(round(1.0 / step))
    if plant:        # the clouds in [-1, 0]^3 and the shared point at (1, 1, 1): farther from every other point than those are from each other
        a = (rng.integers(-k, 1, (B, N, 3)) * step).astype(F)
        b = (rng.integers(-k, 1, (B, M, 3)) * step).astype(F)
        a[:, N // 2] = 1.0
        b[:, M - 1] = 1.0
        if M >= 3:
            a[:, 0] = a[:, 1]                                   # a duplicated point: a tie for whoever it is nearest to
    else:
        a = (rng.integers(-k, k + 1, (B, N, 3)) * step).astype(F)
        b = (rng.integers(-k, k + 1, (B, M, 3)) * step).astype(F)
    a.setflags(write=False), b.setflags(write=False)
    return a, b


def pair_sq(x, y):
    """|x - y|^2 of x [..., 3] and y [..., 3] in the kernels' order"""
    d = (x - y).astype(F)
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def _sum256(v):
    """the loss kernel's sum of a flat float32 array: stride-256 partial sums, then the halving tree"""
    pad = np.zeros((-len(v)) % 256, F)                          # a thread without a further element adds nothing; + 0.0 changes no bit of a sum >= +0
    rows = np.concatenate([v, pad]).reshape(-1, 256)
    red = np.zeros(256, F)
    for r in rows:
        red = red + r
    o = 128
    while o > 0:
        red[:o] = red[:o] + red[o:2 * o]
        o >>= 1
    return red[0]


def _grad(x, y, arg_x, arg_y, form, gscale, B):
    """d loss / d x of one cloud x [nx,3] against y [ny,3]"""
    nx, ny = len(x), len(y)
    wx = F(gscale) / (F(2.0) * F(B) * F(nx))
    wy = F(gscale) / (F(2.0) * F(B) * F(ny))
    if form == "squared":
        g = ((wx * F(2.0)) * (x - y[arg_x])).astype(F)
        for j in range(ny):
            i = arg_y[j]
            g[i] = g[i] + (wy * F(2.0)) * (x[i] - y[j])
        return g
    g = np.zeros((nx, 3), F)
    d = pair_sq(x, y[arg_x])
    live = d > 0
    s = wx / np.sqrt(d[live])
    g[live] = g[live] + s[:, None] * (x[live] - y[arg_x][live])
    for j in range(ny):
        i = arg_y[j]
        dj = pair_sq(x[i], y[j])
        if dj > 0:
            g[i] = g[i] + (wy / np.sqrt(dj)) * (x[i] - y[j])
    return g


@functools.lru_cache(maxsize=None)
def forward(name, form):
    """{min_a [B,N], arg_a [B,N] int32, min_b [B,M], arg_b [B,M] int32, loss [1]} of the case"""
    a, b = inputs(name)
    B, N, M, _, plant = CASES[name]
    with np.errstate(all="raise"):
        D = pair_sq(a[:, :, None, :], b[:, None, :, :])         # [B,N,M]
        out = {"min_a": D.min(2), "arg_a": D.argmin(2).astype(np.int32), "min_b": D.min(1), "arg_b": D.argmin(1).astype(np.int32)}
        root = np.sqrt if form == "sqrt" else (lambda v: v)
        sa, sb = _sum256(root(out["min_a"].reshape(-1))), _sum256(root(out["min_b"].reshape(-1)))
        out["loss"] = np.array([(sa / F(B * N) + sb / F(B * M)) / F(2.0)], F)
    if plant:        # the shared point is its partner's nearest neighbour (distance 0) and nobody else's
        assert (out["min_a"][:, N // 2] == 0).all() and (out["arg_a"][:, N // 2] == M - 1).all()
        assert ((out["arg_a"] == M - 1).sum(1) == 1).all() and ((out["arg_b"] == N // 2).sum(1) == 1).all()
    assert all(v.dtype in (F, np.int32) for v in out.values())
    return out


@functools.lru_cache(maxsize=None)
def backward(name, form, gscale):
    """(da [B,N,3], db [B,M,3]) of the case under the entry's gscale"""
    a, b = inputs(name)
    f = forward(name, form)
    B = a.shape[0]
    with np.errstate(over="raise", invalid="raise", divide="raise"):
        da = np.stack([_grad(a[c], b[c], f["arg_a"][c], f["arg_b"][c], form, gscale, B) for c in range(B)])
        db = np.stack([_grad(b[c], a[c], f["arg_b"][c], f["arg_a"][c], form, gscale, B) for c in range(B)])
    assert da.dtype == F and db.dtype == F
    return da, db

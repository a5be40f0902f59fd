"""Farthest-point sampling: the definition of include/dpdist_capi.h (dpd_fps_order) restated in numpy, and the clouds the tests run it on.

fps_reference evaluates the definition term by term in the dtype asked for: numpy does not fuse a*b + c, `(dx*dx + dy*dy) + dz*dz` keeps
its order, and np.argmax returns the FIRST maximum, which is the lowest-index tie rule.  In float32 it is the bit-exact statement of what
the kernel computes; in float64 it is the same algorithm without rounding, which agrees with float32 wherever every distance is exact:
on lattice clouds (coordinates k/8 in [-1, 1]: differences are multiples of 1/8 up to 2, squares multiples of 1/64 up to 4, sums up to 12,
all far inside 24 bits).  Those clouds carry massive exact ties -- 17^3 = 4913 distinct positions and few distinct distances -- so they
decide whether every merge compares (dmin, index).
"""
import numpy as np


def fps_reference(points, K, start=0, dtype=np.float32):
    """-> (order [K] int32, radius [K] dtype): -1 / 0 past min(K, n)"""
    p = np.asarray(points).astype(dtype)
    n = len(p)
    order = np.full(K, -1, np.int32)
    radius = np.zeros(K, dtype)
    dmin = np.full(n, np.inf, dtype)
    taken = np.zeros(n, bool)
    cur = int(start)
    for k in range(min(K, n)):
        order[k] = cur
        radius[k] = np.inf if k == 0 else np.sqrt(dmin[cur])
        taken[cur] = True
        dx, dy, dz = p[:, 0] - p[cur, 0], p[:, 1] - p[cur, 1], p[:, 2] - p[cur, 2]
        d = (dx * dx + dy * dy) + dz * dz
        assert d.dtype == dtype
        dmin = np.where(d < dmin, d, dmin)
        cur = int(np.argmax(np.where(taken, dtype(-1), dmin)))
    return order, radius


def fps_orders(points_list, K):
    """resample_tree's order_fn on the float32 restatement (row 0 first)"""
    return [fps_reference(p, K)[0][:min(K, len(p))] for p in points_list]


def random_cloud(n, seed):
    return np.random.default_rng([seed, n]).uniform(-1.0, 1.0, (n, 3)).astype(np.float32)


def lattice_cloud(n, seed):
    return (np.random.default_rng([seed, n, 1]).integers(-8, 9, (n, 3)) / 8.0).astype(np.float32)


def lattice_cloud_with_duplicates(n, seed):
    """a lattice cloud whose last tenth repeats earlier points: the copy of point s sits at a higher index, which for n > 64 another lane,
    and for n > 1024 another wave or the same thread's later round, owns"""
    p = lattice_cloud(n, seed)
    m = n // 10
    if m:
        src = np.random.default_rng([seed, n, 2]).integers(0, n - m, m)
        p[n - m:] = p[src]
    return p


def ulp_distance(a, b):
    """largest difference of two float32 arrays in units of the last place (finite or equal infinities)"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return int(np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64)).max()) if a.size else 0


def check_properties(order, radius, n):
    """the consequences of the definition that hold for ANY cloud: a prefix of a permutation, -1 / 0 behind it, radius[1:] non-increasing"""
    K = len(order)
    kn = min(K, n)
    assert sorted(set(order[:kn].tolist())) == sorted(order[:kn].tolist()) and order[:kn].min() >= 0 and order[:kn].max() < n
    assert (order[kn:] == -1).all() and (radius[kn:] == 0).all()
    assert np.isposinf(radius[0])
    r = radius[1:kn]
    assert (r[1:] <= r[:-1]).all() and (r >= 0).all()

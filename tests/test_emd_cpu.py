"""Earth Mover's distance (csrc/emd.hip, dpdist_amd/emd.py) without a GPU: a numpy restatement of the contract in
include/dpdist_capi.h (dpd_emd_fwd), its own checks, the inputs and tolerances of tests/test_emd_gpu.py, and the argument errors of the
C entries.  The restatement is the oracle of both files; it is written from the contract, not from the kernel.

Tolerances of the GPU test.  The restatement runs in float64 (the oracle) and in float32 (every array and constant float32, numpy's exp
and pairwise sums).  FLOOR[q] is the worst deviation of the float32 run from the float64 run over all CASES, measured here on the CPU:
absolute for `match`, relative to the case's largest float64 magnitude for cost, loss and the two gradients.  The GPU bar is
GPU_FACTOR = 8 times that: the device's exponential and summation order differ from numpy's; the algorithm is continuous in its inputs,
so the device's roundings are passed on the way numpy's are.  test_recorded_floors_are_the_measured_ones recomputes the floors, so the
constants cannot drift from the measurement.

    measured floors (numpy float32 vs float64)     match 1.22e-4   cost 7.5e-7   loss 7.5e-7   grad1 2.00e-4   grad2 1.89e-4
    recorded (rounded up)                          match 1.3e-4    cost 8.0e-7   loss 8.0e-7   grad1 2.1e-4    grad2 2.0e-4
    GPU bars (8 x recorded)                        match 1.04e-3   cost 6.4e-6   loss 6.4e-6   grad1 1.68e-3   grad2 1.6e-3
The worst cases are b2_64 and b1_2048 (the others stay below 3e-6): at the sharp levels exp(level d2) has |level d2| of order 10 to 100, so
one rounding of d2 moves a weight by 1e-6 to 1e-5 relative, and where a point's mass hangs on few such weights the clamps
min(., 1) and max(0, .) pass that on to single match entries.  Cost and loss average over the entries and stay at 1e-6.
"""
import ctypes
import functools

import numpy as np
import pytest

LEVELS = [-(4.0 ** j) for j in range(7, -2, -1)] + [0.0]          # j = 7 ... -1, then level 0 at j = -2
GPU_FACTOR = 8.0
# recorded from floors() below (rounded up); see the module docstring
FLOOR = {"match": 1.3e-4, "cost": 8.0e-7, "loss": 8.0e-7, "grad1": 2.1e-4, "grad2": 2.0e-4}
# minimum over CASES of sum(match) / max(n, m) in the float64 restatement (test_transported_mass_of_the_gpu_inputs)
MASS_FLOOR = 0.99


def d2_matrix(x1, x2):
    """[n,m,3] differences xyz1[k] - xyz2[l] and d2(k,l) = (dx*dx + dy*dy) + dz*dz, in the arrays' dtype"""
    d = x1[:, None, :] - x2[None, :, :]
    return d, (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def approx_match_pair(x1, x2, dtype=np.float64):
    """match [m,n] of one pair, the contract's three steps per level"""
    T = dtype
    x1, x2 = x1.astype(T), x2.astype(T)
    n, m = len(x1), len(x2)
    _, d2 = d2_matrix(x1, x2)                                      # [n,m] = (k,l)
    big = T(max(n, m))
    remainL, remainR = np.full(n, big / T(n), T), np.full(m, big / T(m), T)
    match = np.zeros((m, n), T)
    eps, zero, one = T(1e-9), T(0), T(1)
    for level in LEVELS:
        e = np.exp(T(level) * d2)
        ratioL = remainL / (eps + (e * remainR[None, :]).sum(1))
        s = remainR * (e * ratioL[:, None]).sum(0)
        ratioR = np.minimum(remainR / (s + eps), one) * remainR
        remainR = np.maximum(zero, remainR - s)
        w = e * ratioL[:, None] * ratioR[None, :]
        match += w.T
        remainL = np.maximum(zero, remainL - w.sum(1))
    assert match.dtype == T
    return match


def match_cost_pair(x1, x2, match, dtype=np.float64):
    """cost and d cost / d xyz1 [n,3], d cost / d xyz2 [m,3] of one pair for a given (constant) match [m,n]"""
    T = dtype
    x1, x2, mt = x1.astype(T), x2.astype(T), match.astype(T).T      # mt [n,m]
    d, d2 = d2_matrix(x1, x2)
    cost = (mt * np.sqrt(d2)).sum()
    t = (mt / np.sqrt(np.maximum(d2, T(1e-20))))[..., None] * d
    return cost, t.sum(1), -t.sum(0)


def emd_restate(xyz1, xyz2, dtype=np.float64, upstream=1.0):
    """The whole contract for a batch: match [B,m,n], cost [B], loss, grad1 [B,n,3], grad2 [B,m,3] (gradients of the loss times upstream)"""
    B, n = xyz1.shape[0], xyz1.shape[1]
    out = {"match": [], "cost": [], "grad1": [], "grad2": []}
    for b in range(B):
        mt = approx_match_pair(xyz1[b], xyz2[b], dtype)
        c, g1, g2 = match_cost_pair(xyz1[b], xyz2[b], mt, dtype)
        scale = dtype(upstream) / dtype(B * n)
        for k, v in zip(("match", "cost", "grad1", "grad2"), (mt, c, g1 * scale, g2 * scale)):
            out[k].append(v)
    out = {k: np.stack(v) for k, v in out.items()}
    out["loss"] = (out["cost"] / dtype(n)).mean(dtype=dtype)
    return out


# ---- the inputs of the GPU test: uniform in [-0.8, 0.8]^3, fixed seeds -----------------------------------------------------------------
SHAPES = {"one": (1, 1, 1), "b2_64": (2, 64, 64), "b3_65_130": (3, 65, 130), "b2_257_64": (2, 257, 64), "b1_2048": (1, 2048, 2048),
          "dup": (2, 96, 80), "far": (2, 33, 47)}
CASES = list(SHAPES)


@functools.lru_cache(maxsize=None)
def inputs(name):
    B, n, m = SHAPES[name]
    rng = np.random.default_rng(4200 + CASES.index(name))
    x1 = rng.uniform(-0.8, 0.8, (B, n, 3)).astype(np.float32)
    x2 = rng.uniform(-0.8, 0.8, (B, m, 3)).astype(np.float32)
    if name == "dup":                       # a third of each cloud repeats earlier points, and the clouds share points (d2 = 0 exactly)
        x1[:, 64:] = x1[:, :32]
        x2[:, 48:] = x2[:, :32]
        x2[:, :16] = x1[:, 40:56]
    if name == "far":                       # |dx| >= 38.4: exp(-0.25 d2) < 1e-160, exactly 0 in fp32: nothing moves before level 0
        x2[..., 0] += np.float32(40.0)
    for a in (x1, x2):
        a.setflags(write=False)
    return x1, x2


@functools.lru_cache(maxsize=None)
def oracle(name):
    """float64 restatement of a case, computed once per process and read-only"""
    out = emd_restate(*inputs(name))
    for a in out.values():
        a.setflags(write=False)
    return out


def deviation(got, want):
    """{quantity: deviation of `got` from the float64 `want`}: absolute for match, relative to the largest magnitude for the rest"""
    dev = {}
    for q in FLOOR:
        err = np.abs(np.asarray(got[q], np.float64) - want[q]).max()
        dev[q] = err if q == "match" else err / np.abs(want[q]).max()
    return dev


def floors():
    worst = dict.fromkeys(FLOOR, 0.0)
    for name in CASES:
        dev = deviation(emd_restate(*inputs(name), dtype=np.float32), oracle(name))
        print(name, {q: "%.3g" % v for q, v in dev.items()})
        worst = {q: max(worst[q], dev[q]) for q in worst}
    return worst


# ---- the restatement's own checks ------------------------------------------------------------------------------------------------------
def test_recorded_floors_are_the_measured_ones():
    """FLOOR is the float32 restatement's worst deviation from float64 on CASES as measured when the test was written.  numpy's exp and
    pairwise sums differ by an ulp between CPUs (SIMD width) and the worst entry is a tail event, so the recomputed floor may move: it
    has to stay within a factor of four of the recorded one, either way."""
    worst = floors()
    print("measured floors:", {q: "%.3g" % v for q, v in worst.items()})
    for q, v in worst.items():
        assert FLOOR[q] / 4 <= v <= FLOOR[q] * 4, (q, v, FLOOR[q])


def test_gradient_formula_is_the_derivative_of_the_cost_with_the_match_frozen():
    rng = np.random.default_rng(1)
    x1, x2 = rng.uniform(-0.8, 0.8, (7, 3)), rng.uniform(-0.8, 0.8, (9, 3))
    mt = approx_match_pair(x1, x2)
    _, g1, g2 = match_cost_pair(x1, x2, mt)
    h = 1e-6
    for x, g, which in ((x1, g1, 0), (x2, g2, 1)):
        for i in range(len(x)):
            for c in range(3):
                p, q = x.copy(), x.copy()
                p[i, c] += h
                q[i, c] -= h
                fd = (match_cost_pair(*((p, x2) if which == 0 else (x1, p)), mt)[0] -
                      match_cost_pair(*((q, x2) if which == 0 else (x1, q)), mt)[0]) / (2 * h)
                assert abs(fd - g[i, c]) <= 1e-8 + 1e-7 * abs(g[i, c]), (which, i, c, fd, g[i, c])


def test_permutation_of_a_well_separated_cloud_is_matched_to_itself():
    """points on a grid of pitch 0.4: the first level (exp(-16384 * 0.16) = 0 off the diagonal) already moves everything"""
    g = np.stack(np.meshgrid(*[np.arange(3) * 0.4 - 0.4] * 3, indexing="ij"), -1).reshape(-1, 3)
    perm = np.random.default_rng(2).permutation(len(g))
    x2 = g[perm]                                                   # xyz2[l] = xyz1[perm[l]]
    mt = approx_match_pair(g, x2)
    want = np.zeros_like(mt)
    want[np.arange(len(g)), perm] = 1.0
    assert np.abs(mt - want).max() <= 1e-8
    assert match_cost_pair(g, x2, mt)[0] < 1e-6


@pytest.mark.parametrize("name", [c for c in CASES if c != "b1_2048"])
def test_row_and_column_sums_stay_within_the_initial_remain(name):
    B, n, m = SHAPES[name]
    mt = oracle(name)["match"]
    assert (mt >= 0).all()
    assert mt.sum(1).max() <= max(n, m) / n * (1 + 1e-12)          # over l: what point k of xyz1 gave away
    assert mt.sum(2).max() <= max(n, m) / m * (1 + 1e-12)          # over k: what point l of xyz2 received


def test_transported_mass_of_the_gpu_inputs():
    """sum(match) / max(n, m) per pair: the restatement moves at least MASS_FLOOR of the mass on every input of the GPU test (the
    minimum measured here is 1 - 2e-9: level 0 hands out whatever is left); tests/test_emd_gpu.py asserts the same floor for the kernel."""
    worst = 1.0
    for name in CASES:
        B, n, m = SHAPES[name]
        mass = oracle(name)["match"].sum((1, 2)) / max(n, m)
        print(name, "transported mass", mass)
        worst = min(worst, mass.min())
    assert worst >= MASS_FLOOR


def test_far_clouds_are_matched_uniformly():
    B, n, m = SHAPES["far"]
    assert np.abs(oracle("far")["match"] - max(n, m) / (n * m)).max() <= 1e-8


# ---- the C entries' argument checks, no device -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from dpdist_amd import build, lib as L
    build.build(verbose=False)
    return L.load()


def test_exports_and_header_agree(lib):
    import os
    from dpdist_amd import lib as L
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dpdist_capi.h")).read()
    for name in ("dpd_emd_fwd", "dpd_emd_match_cost", "dpd_emd_workspace_bytes"):
        assert hasattr(lib, name) and name in L.SIGNATURES and name + "(" in header
    assert "#define DPD_EMD_MAX_POINTS 2048" in header


def test_argument_errors_without_a_device(lib):
    p = ctypes.c_void_p(1 << 30)                                  # any non-NULL "device address": nothing is dereferenced
    E_NULL, E_DIM, E_UNSUPPORTED, E_WORKSPACE = -1, -2, -3, -4
    ok = lib.dpd_emd_workspace_bytes(2, 64, 65)
    assert ok == (2 * 64 * 3 + 2 * 65 * 2) * 4
    fwd = lambda x1, x2, B, n, m, cost, loss, ws, nb: lib.dpd_emd_fwd(x1, x2, B, n, m, 1.0, cost, loss, None, None, None, ws, nb, None)   # noqa: E731
    for args in ((None, p, p, p, p), (p, None, p, p, p), (p, p, None, p, p), (p, p, p, None, p), (p, p, p, p, None)):
        x1, x2, cost, loss, ws = args
        assert fwd(x1, x2, 2, 64, 65, cost, loss, ws, ok) == E_NULL
    assert fwd(p, p, 0, 64, 65, p, p, p, ok) == E_DIM
    assert fwd(p, p, 2, 0, 65, p, p, p, ok) == E_DIM and fwd(p, p, 2, 64, -1, p, p, p, ok) == E_DIM
    assert fwd(p, p, 2, 2049, 65, p, p, p, 1 << 30) == E_UNSUPPORTED and fwd(p, p, 2, 64, 2049, p, p, p, 1 << 30) == E_UNSUPPORTED
    assert fwd(p, p, 2, 64, 65, p, p, p, ok - 1) == E_WORKSPACE
    assert lib.dpd_emd_workspace_bytes(1, 2049, 1) == 0 and lib.dpd_emd_workspace_bytes(0, 1, 1) == 0
    assert lib.dpd_emd_workspace_bytes(1, 2048, 2048) == (2048 * 5) * 4
    mc = lambda match, B, n: lib.dpd_emd_match_cost(p, p, B, n, 65, match, 1.0, p, p, None, None, p, ok, None)   # noqa: E731
    assert mc(None, 2, 64) == E_NULL and mc(p, 0, 64) == E_DIM and mc(p, 2, 2049) == E_UNSUPPORTED


def test_wrappers_refuse_cpu_tensors(lib):
    import torch
    from dpdist_amd import emd
    a, b = torch.zeros(1, 8, 3), torch.zeros(1, 9, 3)
    for call in (lambda: emd.earth_mover(a, b), lambda: emd.approx_match(a, b), lambda: emd.match_cost(a, b, torch.zeros(1, 9, 8))):
        with pytest.raises(RuntimeError, match="GPU"):
            call()

"""dpd_emd_fwd / dpd_emd_match_cost (csrc/emd.hip) and dpdist_amd/emd.py on the GPU against the float64 restatement of
tests/test_emd_cpu.py, which also holds the inputs (CASES) and the tolerances: the bar of a quantity is GPU_FACTOR = 8 times the
float32 restatement's worst deviation from float64 on these inputs (FLOOR, measured on the CPU, never from the kernel):

    quantity   floor (numpy fp32 vs fp64)   GPU bar        measure
    match      1.3e-4                       1.04e-3        absolute
    cost       8.0e-7                       6.4e-6         relative to the largest |cost| of the case
    loss       8.0e-7                       6.4e-6         relative
    grad1      2.1e-4                       1.68e-3        relative to the largest |grad1| entry of the case
    grad2      2.0e-4                       1.6e-3         relative to the largest |grad2| entry of the case
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from dpdist_amd import emd
from dpdist_amd import lib as L

from . import test_emd_cpu as E

pytestmark = pytest.mark.gpu

BAR = {q: E.GPU_FACTOR * v for q, v in E.FLOOR.items()}
G, SENT = 1024, -7.0            # guard band (floats) on either side of every output, and its fill


def cu(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()      # a copy: the cached inputs are read-only


class Banded:
    """an output buffer of `shape` between two guard bands"""

    def __init__(self, *shape):
        self.n = int(np.prod(shape))
        self.shape = shape
        self.buf = torch.full((self.n + 2 * G,), SENT, device="cuda")
        self.ptr = ctypes.c_void_p(self.buf.data_ptr() + 4 * G)

    def get(self):
        assert (self.buf[:G] == SENT).all() and (self.buf[G + self.n:] == SENT).all(), "guard band overwritten"
        return self.buf[G:G + self.n].view(*self.shape).clone()


def run_entry(x1, x2, with_match, gscale=1.0, grads=(True, True)):
    """dpd_emd_fwd through the C ABI with guard bands around every output: {quantity: tensor}"""
    lib = L.load()
    B, n, m = x1.shape[0], x1.shape[1], x2.shape[1]
    out = {"cost": Banded(B), "loss": Banded(1)}
    if grads[0]:
        out["grad1"] = Banded(B, n, 3)
    if grads[1]:
        out["grad2"] = Banded(B, m, 3)
    if with_match:
        out["match"] = Banded(B, m, n)
    ws = Banded(lib.dpd_emd_workspace_bytes(B, n, m) // 4)
    p = lambda q: out[q].ptr if q in out else None      # noqa: E731
    L.check(lib.dpd_emd_fwd(L.ptr(x1), L.ptr(x2), B, n, m, gscale, p("cost"), p("loss"), p("grad1"), p("grad2"), p("match"), ws.ptr,
                            ws.n * 4, L.cur_stream()), "dpd_emd_fwd")
    ws.get()
    res = {q: b.get() for q, b in out.items()}
    res["loss"] = res["loss"][0]
    return res


@functools.lru_cache(maxsize=None)
def gpu_result(name):
    x1, x2 = (cu(a) for a in E.inputs(name))
    return x1, x2, run_entry(x1, x2, True)


def check_against_oracle(name, got):
    want = E.oracle(name)
    dev = E.deviation({q: (got[q].cpu().numpy() if q in got else want[q]) for q in E.FLOOR}, want)
    print(name, {q: "%.3g (bar %.3g)" % (dev[q], BAR[q]) for q in dev if q in got})
    for q in got:
        assert torch.isfinite(got[q]).all(), q
        assert dev[q] <= BAR[q], (name, q, dev[q], BAR[q])


@pytest.mark.parametrize("name", E.CASES)
def test_entry_with_the_match_written_against_the_restatement(name):
    x1, x2, got = gpu_result(name)
    check_against_oracle(name, got)
    B, n, m = E.SHAPES[name]
    mass = got["match"].double().sum((1, 2)) / max(n, m)
    print(name, "transported mass", mass.cpu().numpy())
    assert mass.min().item() >= E.MASS_FLOOR
    assert (got["match"] >= 0).all()


@pytest.mark.parametrize("name", E.CASES)
def test_fused_path_gives_the_same_cost_and_gradients(name):
    """match = NULL (the training path: no [B,m,n] array) against the path with the match written: within the bar of the restatement, and
    in fact the same bits, since both accumulate cost and gradients from the same registers in the same order"""
    x1, x2, full = gpu_result(name)
    fused = run_entry(x1, x2, False)
    assert "match" not in fused
    check_against_oracle(name, fused)
    for q in ("cost", "loss", "grad1", "grad2"):
        assert torch.equal(fused[q], full[q]), q
    only1, only2 = run_entry(x1, x2, False, grads=(True, False)), run_entry(x1, x2, False, grads=(False, True))   # either gradient alone
    assert torch.equal(only1["grad1"], full["grad1"]) and torch.equal(only2["grad2"], full["grad2"])
    assert torch.equal(only1["cost"], full["cost"]) and torch.equal(only2["loss"], full["loss"])


@pytest.mark.parametrize("name", E.CASES)
def test_two_runs_are_bitwise_equal(name):
    x1, x2, full = gpu_result(name)
    again = run_entry(x1, x2, True)
    for q in full:
        assert torch.equal(again[q].view(torch.int32), full[q].view(torch.int32)), q


@pytest.mark.parametrize("name", E.CASES)
def test_autograd_function_agrees_with_the_entry_and_scales_with_the_upstream_gradient(name):
    x1, x2, full = gpu_result(name)
    a, b = x1.clone().requires_grad_(), x2.clone().requires_grad_()
    loss = emd.earth_mover(a, b)
    assert loss.shape == () and torch.equal(loss.detach(), full["loss"])
    loss.backward()
    assert torch.equal(a.grad, full["grad1"]) and torch.equal(b.grad, full["grad2"])
    a2, b2 = x1.clone().requires_grad_(), x2.clone().requires_grad_()
    (emd.earth_mover(a2, b2) * -2.5).backward()                    # a non-unit upstream gradient
    assert torch.equal(a2.grad, full["grad1"] * -2.5) and torch.equal(b2.grad, full["grad2"] * -2.5)
    want = E.oracle(name)
    for g, q in ((a2.grad, "grad1"), (b2.grad, "grad2")):
        ref = -2.5 * want[q]
        assert np.abs(g.cpu().numpy() - ref).max() / np.abs(ref).max() <= BAR[q]
    a3 = x1.clone().requires_grad_()                               # a gradient to one input only
    emd.earth_mover(a3, x2).backward()
    assert torch.equal(a3.grad, full["grad1"])
    b3 = x2.clone().requires_grad_()
    emd.earth_mover(x1, b3).backward()
    assert torch.equal(b3.grad, full["grad2"])
    scaled = run_entry(x1, x2, False, gscale=-2.5)                 # the entry's own gscale
    for q in ("grad1", "grad2"):
        ref = -2.5 * want[q]
        assert np.abs(scaled[q].cpu().numpy() - ref).max() / np.abs(ref).max() <= BAR[q]


@pytest.mark.parametrize("n,m", [(70, 130), (130, 70)])
def test_a_batch_is_its_pairs_one_by_one(n, m):
    """the batch plumbing of the entry (two to three owner tiles, tail lanes, uneven quarters): cost, grad1, grad2 and match of a batch of
    three are, bit for bit, those of three calls with one pair each and a third of the gscale (3 / (3 n) and 1 / n are the same float),
    with either gradient left out too; loss is the fixed-order float32 mean of cost[b] / n"""
    rng = np.random.default_rng(n)
    x1, x2 = cu(rng.uniform(-1, 1, (3, n, 3)).astype(np.float32)), cu(rng.uniform(-1, 1, (3, m, 3)).astype(np.float32))
    batch = run_entry(x1, x2, True, gscale=3.0)
    ones = [run_entry(x1[b:b + 1].contiguous(), x2[b:b + 1].contiguous(), True, gscale=1.0) for b in range(3)]
    same = lambda u, v: torch.equal(u.view(torch.int32), v.view(torch.int32))      # noqa: E731
    for q in ("cost", "grad1", "grad2", "match"):
        assert same(batch[q], torch.cat([o[q] for o in ones])), q
    tot = np.float32(0)
    for c in batch["cost"].cpu().numpy():
        tot = tot + c / np.float32(n)
    assert batch["loss"].cpu().numpy().view(np.int32) == (tot / np.float32(3)).view(np.int32)
    only1, only2 = run_entry(x1, x2, False, gscale=3.0, grads=(True, False)), run_entry(x1, x2, False, gscale=3.0, grads=(False, True))
    assert "grad2" not in only1 and "grad1" not in only2
    assert same(only1["grad1"], batch["grad1"]) and same(only2["grad2"], batch["grad2"])
    for o in (only1, only2):
        assert same(o["cost"], batch["cost"]) and same(o["loss"], batch["loss"])


def test_far_clouds_get_the_uniform_match():
    """no exponential survives before level 0 (|dx| >= 38: exp(-0.25 d2) = 0 in fp32), so every pair receives max(n,m) / (n m)"""
    B, n, m = E.SHAPES["far"]
    got = gpu_result("far")[2]["match"]
    assert (got - max(n, m) / (n * m)).abs().max().item() <= BAR["match"] * max(n, m) / (n * m)


def test_duplicated_points_give_finite_gradients_and_zero_distance_pairs_no_direction():
    x1, x2, got = gpu_result("dup")
    assert torch.isfinite(got["grad1"]).all() and torch.isfinite(got["grad2"]).all()
    assert torch.equal(x2[:, :16], x1[:, 40:56])                   # shared points: d2 = 0 exactly


@pytest.mark.parametrize("name", ["b3_65_130", "dup"])
def test_the_ops_original_names(name):
    """approx_match / match_cost (the op's names): the match of the entry, and cost [B] with its gradients for a GIVEN match"""
    x1, x2, full = gpu_result(name)
    B, n, m = E.SHAPES[name]
    mt = emd.approx_match(x1, x2)
    assert mt.shape == (B, m, n) and torch.equal(mt, full["match"]) and not mt.requires_grad
    rng = np.random.default_rng(5)
    given = rng.uniform(0, 1, (B, m, n)).astype(np.float32)        # any match, not the optimal one
    up = rng.uniform(-1, 1, B)
    a, b = x1.clone().requires_grad_(), x2.clone().requires_grad_()
    cost = emd.match_cost(a, b, cu(given))
    (cost * cu(up.astype(np.float32))).sum().backward()
    x1n, x2n = E.inputs(name)
    for i in range(B):
        c, g1, g2 = E.match_cost_pair(x1n[i], x2n[i], given[i])
        assert abs(cost[i].item() - c) <= 1e-5 * abs(c)
        assert np.abs(a.grad[i].cpu().numpy() - up[i] * g1).max() <= 1e-5 * np.abs(g1).max()
        assert np.abs(b.grad[i].cpu().numpy() - up[i] * g2).max() <= 1e-5 * np.abs(g2).max()


def test_errors_name_the_entry_and_bad_inputs_are_refused():
    with pytest.raises(RuntimeError, match="dpd_emd_fwd.*DPD_E_UNSUPPORTED"):
        emd.earth_mover(torch.zeros(1, 2049, 3, device="cuda"), torch.zeros(1, 4, 3, device="cuda"))
    with pytest.raises(RuntimeError, match="float32"):
        emd.earth_mover(torch.zeros(1, 4, 3, device="cuda").double(), torch.zeros(1, 4, 3, device="cuda").double())
    with pytest.raises(RuntimeError, match="same number of clouds"):
        emd.earth_mover(torch.zeros(2, 4, 3, device="cuda"), torch.zeros(1, 4, 3, device="cuda"))
    with pytest.raises(RuntimeError, match="match must have shape"):
        emd.match_cost(torch.zeros(1, 4, 3, device="cuda"), torch.zeros(1, 5, 3, device="cuda"), torch.zeros(1, 4, 5, device="cuda"))

"""Exact-value edge tests of the pose network's units through their C entries: dpd_pose_point_fwd_train / dpd_pose_point_bwd (shared MLP,
max pool, tie words, the ten gradients), dpd_pose_head_fwd_train / dpd_pose_head_bwd, dpd_pose_refine (first loop) and
dpd_pose_apply_fwd / dpd_pose_apply_bwd.

tests/pose_cases.py holds the integer networks, the float64 references, the checker and the case tables (tests/test_pose_edges_cpu.py
proves on the CPU that every entry keeps the exactness condition and that the checker has teeth).  On the integer network every fp32
operation of the forward and the backward is exact, so every comparison of the exact families is an equality of values (-0 equals +0,
a NaN never matches) or an integer return code.  Every output and every workspace -- at exactly the size its `*_workspace_bytes` entry
reports -- is pre-filled with a NaN pattern and sits between guard bands that must keep their bits; every input sits between NaNs, so
an element read past an edge poisons a result.  Nothing the reference can supply is taken from the library: the backward entries are
given the reference's activations and tie words, and df = cnt * k with the reference's own tie count.

The only tolerances are those of the real-valued pose algebra (2e-6 forward, 2e-5 max(1, |grad|) backward) and of the moved cloud and
transform after the first refinement loop (5e-5): the bars tests/test_registration.py already applies to the same kernels."""
import ctypes

import numpy as np
import pytest
import torch

from dpdist_amd import lib as L

from . import pose_cases as P
from .gemm_cases import NAN_IN, NAN_OUT, banded_flat

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible")
    L.load()     # raises if the HIP extension is missing -- never fall back
    return torch.device("cuda:0")


def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def ptrs(ts):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


class Buffers:
    """the banded buffers of one call: inputs between NaNs, outputs filled with NAN_OUT; `check()` runs every band check"""

    def __init__(self, dev):
        self.dev, self.checks = dev, []

    def put(self, x):
        """a float32 input holding the (integer or real) array x"""
        x = np.ascontiguousarray(x, dtype=np.float32)
        view, chk = banded_flat(x.size, NAN_IN, device=self.dev)
        view.copy_(torch.from_numpy(x.reshape(-1)))
        self.checks.append(chk)
        return view

    def put_words(self, w):
        """uint64 tie words as an input"""
        w = np.array(w, dtype=np.uint64)                 # (a copy: the reference's arrays are read-only)
        view, chk = banded_flat(2 * w.size, NAN_IN, dtype=torch.int32, device=self.dev)
        view.view(torch.int64).copy_(torch.from_numpy(w.reshape(-1).view(np.int64)))
        self.checks.append(chk)
        return view

    def out(self, n, dtype=torch.float32):
        view, chk = banded_flat(n, NAN_OUT, dtype=dtype, device=self.dev)
        self.checks.append(chk)
        return view

    def check(self):
        torch.cuda.synchronize()
        for chk in self.checks:
            chk()


def host(t, *shape):
    return t.detach().cpu().numpy().reshape(*shape)


_NETS = {}


def device_net(dev, point="plain"):
    """dpd_pose_net of an integer shared MLP and the integer head (uploaded once per variant, between NaNs)"""
    if point not in _NETS:
        bufs = Buffers(dev)
        pn, hn = P.point_net(point), P.head_net()
        w = L.PoseNetW()
        for i in range(5):
            w.Wp[i], w.bp[i] = bufs.put(pn.W[i]).data_ptr(), bufs.put(pn.b[i]).data_ptr()
        for i in range(4):
            w.Wh[i], w.bh[i] = bufs.put(hn.W[i]).data_ptr(), bufs.put(hn.b[i]).data_ptr()
        w.out_features = P.OUT
        _NETS[point] = (w, bufs)
    return _NETS[point][0]


# ------------------------------------------------------------------------------------------------ 1. shared MLP, max pool and backward
@pytest.mark.parametrize("case", P.POINT_CASES, ids=[c.id for c in P.POINT_CASES])
def test_point_case(dev, case):
    """forward: f, h1 .. h4 and every tie word (C * ceil(N / 64) * 1024 of them, no bit at or beyond N) equal the reference; backward, given
    the reference's activations, tie words and df = cnt * k: all ten gradients equal the reference"""
    lib = L.load()
    net = device_net(dev, case.net)
    _, bwd, want = P.point_reference(case)
    A, B = P.point_clouds(case)
    nA, nB, N, C = case.nA, case.nB, case.N, case.nA + case.nB
    NW = lib.dpd_pose_point_tie_words(N)
    assert NW == (N + 63) // 64
    widths = (64, 64, 64, 128)
    bufs = Buffers(dev)
    a, b = bufs.put(A), (bufs.put(B) if nB else None)
    f, h = bufs.out(C * P.OUT), [bufs.out(C * N * w) for w in widths]
    ties = bufs.out(2 * C * NW * 1024, torch.int32)
    rc = lib.dpd_pose_point_fwd_train(ctypes.byref(net), ptr(a), ptr(b), nA, nB, N, ptr(f), ptr(h[0]), ptr(h[1]), ptr(h[2]), ptr(h[3]), ptr(ties),
                                      L.cur_stream())
    assert rc == 0, rc
    bufs.check()
    got = {"f": host(f, C, P.OUT), "ties": host(ties.view(torch.int64), C, NW, 1024)}
    got.update({"h%d" % (i + 1): host(h[i], C * N, w) for i, w in enumerate(widths)})
    P.check(got, want, P.POINT_NAMES[:6])

    bufs = Buffers(dev)
    a, b = bufs.put(A), (bufs.put(B) if nB else None)
    hin = [bufs.put(want["h%d" % (i + 1)]) for i in range(4)]
    tin, df = bufs.put_words(want["ties"]), bufs.put(bwd["df"])
    nbytes = lib.dpd_pose_point_bwd_workspace_bytes_n(C, N)
    assert nbytes > 0 and nbytes % 4 == 0
    ws = bufs.out(nbytes // 4)
    dW = [bufs.out(o * i) for i, o in P.POINT_WIDTHS]
    db = [bufs.out(o) for _, o in P.POINT_WIDTHS]
    rc = lib.dpd_pose_point_bwd(ctypes.byref(net), ptr(a), ptr(b), nA, nB, N, ptr(df), ptr(hin[0]), ptr(hin[1]), ptr(hin[2]), ptr(hin[3]), ptr(tin),
                                ptrs(dW), ptrs(db), ptr(ws), nbytes, L.cur_stream())
    assert rc == 0, rc
    bufs.check()
    got = {"dW%d" % (l + 1): host(dW[l], o, i) for l, (i, o) in enumerate(P.POINT_WIDTHS)}
    got.update({"db%d" % (l + 1): host(db[l], o) for l, (_, o) in enumerate(P.POINT_WIDTHS)})
    P.check(got, want, P.POINT_NAMES[6:])


# ------------------------------------------------------------------------------------------------ 2. head
@pytest.mark.parametrize("case", P.HEAD_CASES, ids=[c.id for c in P.HEAD_CASES])
def test_head_case(dev, case):
    """h1, h2, h3 (dropout mask in {0, 2} applied) and pred; then, given the reference's activations, the eight gradients and df [2B, 1024]"""
    lib = L.load()
    net = device_net(dev)
    _, _, want = P.head_reference(case)
    fin, mask, dpred = P.head_inputs(case)
    B = case.B
    bufs = Buffers(dev)
    f = bufs.put(fin)
    m = None if mask is None else bufs.put(mask)
    outs = [bufs.out(B * w) for w in (1024, 512, 256, 7)]
    rc = lib.dpd_pose_head_fwd_train(ctypes.byref(net), ptr(f), B, ptr(m), ptr(outs[0]), ptr(outs[1]), ptr(outs[2]), ptr(outs[3]), L.cur_stream())
    assert rc == 0, rc
    bufs.check()
    got = {n: host(t, B, w) for n, t, w in zip(("h1", "h2", "h3", "pred"), outs, (1024, 512, 256, 7))}
    P.check(got, want, P.HEAD_NAMES[:4])

    bufs = Buffers(dev)
    f = bufs.put(fin)
    m = None if mask is None else bufs.put(mask)
    hin = [bufs.put(want[n]) for n in ("h1", "h2", "h3")]
    dp = bufs.put(dpred)
    nbytes = lib.dpd_pose_head_bwd_workspace_bytes(B)
    assert nbytes == B * (256 + 512 + 1024) * 4
    ws = bufs.out(nbytes // 4)
    dW = [bufs.out(o * i) for i, o in P.HEAD_WIDTHS]
    db = [bufs.out(o) for _, o in P.HEAD_WIDTHS]
    df = bufs.out(2 * B * P.OUT)
    rc = lib.dpd_pose_head_bwd(ctypes.byref(net), ptr(f), B, ptr(m), ptr(hin[0]), ptr(hin[1]), ptr(hin[2]), ptr(dp), ptrs(dW), ptrs(db), ptr(df),
                               ptr(ws), nbytes, L.cur_stream())
    assert rc == 0, rc
    bufs.check()
    got = {"dW%d" % (l + 1): host(dW[l], o, i) for l, (i, o) in enumerate(P.HEAD_WIDTHS)}
    got.update({"db%d" % (l + 1): host(db[l], o) for l, (_, o) in enumerate(P.HEAD_WIDTHS)})
    got["df"] = host(df, 2 * B, P.OUT)
    P.check(got, want, P.HEAD_NAMES[4:])


# ------------------------------------------------------------------------------------------------ 3. refinement, first loop
def _pose_reference(pred, src, T, lim, mode):
    """float64 torch algebra of dpdist_amd/registration.py: (pred leaf, pose, moved, T_out); T None: composed onto the identity"""
    from dpdist_amd.registration import compose, predicted_pose_applied, quat_normalize, transformation_quat_tensor, unit_quat_pose
    p = torch.as_tensor(np.asarray(pred, dtype=np.float64)).requires_grad_(True)
    s = torch.as_tensor(np.asarray(src, dtype=np.float64))
    T = torch.eye(4, dtype=torch.float64).repeat(len(p), 1, 1) if T is None else torch.as_tensor(np.asarray(T, dtype=np.float64))
    pose = quat_normalize(p, lim) if lim else p
    pc = unit_quat_pose(pose)
    moved = transformation_quat_tensor(s, pc[:, 3:7], pc[:, :3]) if mode == 0 else predicted_pose_applied(s, pose)
    return p, pose, moved, compose(T, pc)


@pytest.mark.parametrize("case", P.REFINE_CASES, ids=[c.id for c in P.REFINE_CASES])
def test_refine_first_loop(dev, case):
    """dpd_pose_refine with loops = 1 on the integer network: pred_out equals the reference exactly (the template half of fc1 as a
    separate `rowbias` sum, fc4 as the apply kernel's prologue); moved and T_out follow the float64 algebra of that pose to 5e-5"""
    lib = L.load()
    net = device_net(dev)
    src, tmpl, mask = P.refine_inputs(case)
    want, _ = P.refine_reference(case)
    B, N = case.B, case.N
    bufs = Buffers(dev)
    s, t = bufs.put(src), bufs.put(tmpl)
    m = None if mask is None else bufs.put(mask)
    nbytes = lib.dpd_pose_refine_workspace_bytes(B, N, P.OUT)
    assert nbytes > 0 and nbytes % 4 == 0
    ws, moved, T_out, pred = bufs.out(nbytes // 4), bufs.out(B * N * 3), bufs.out(B * 16), bufs.out(B * 7)
    rc = lib.dpd_pose_refine(ctypes.byref(net), ptr(s), ptr(t), B, N, 1, P.REFINE_LIM, ptr(m), ptr(ws), nbytes, ptr(moved), ptr(T_out), ptr(pred),
                             L.cur_stream())
    assert rc == 0, rc
    bufs.check()
    P.same_values(host(pred, B, 7), want, "pred_out")
    _, _, moved64, T64 = _pose_reference(want, src, None, P.REFINE_LIM, 0)
    em = np.abs(host(moved, B, N, 3).astype(np.float64) - moved64.detach().numpy()).max()
    eT = np.abs(host(T_out, B, 4, 4).astype(np.float64) - T64.detach().numpy()).max()
    print("%s: |moved - float64| = %.3e, |T - float64| = %.3e" % (case.id, em, eT))
    assert em <= 5e-5 and eT <= 5e-5          # (a NaN fails both)
    assert np.abs(moved64.detach().numpy() - src).max() > 1e-2          # the pose did move the cloud


# ------------------------------------------------------------------------------------------------ 4. pose algebra
def _apply_fwd(dev, pred, src, T, N, lim, mode, want_pose=True, want_moved=True, want_T=True):
    """one dpd_pose_apply_fwd call on banded buffers -> (pose, moved, T_out) as numpy (None for an output not asked for)"""
    B = len(pred)
    bufs = Buffers(dev)
    p = bufs.put(pred)
    s = bufs.put(src) if want_moved else None
    t = None if T is None else bufs.put(T)
    pose = bufs.out(B * 7) if want_pose else None
    moved = bufs.out(B * N * 3) if want_moved else None
    T_out = bufs.out(B * 16) if want_T else None
    rc = L.load().dpd_pose_apply_fwd(ptr(p), ptr(s), ptr(t), B, N, float(lim), mode, ptr(pose), ptr(moved), ptr(T_out), L.cur_stream())
    assert rc == 0, rc
    bufs.check()
    return (None if pose is None else host(pose, B, 7), None if moved is None else host(moved, B, N, 3),
            None if T_out is None else host(T_out, B, 4, 4))


@pytest.mark.parametrize("N", P.APPLY_N)
@pytest.mark.parametrize("B", P.APPLY_B)
def test_apply_exact_family(dev, B, N):
    """lim = 0, mode 0, quaternions of norm 1 or 2, integer source, translation and T_in: the rotation is a signed permutation, so pose,
    moved and T_out EQUAL the reference -- a misindexed or dropped point beyond lane 63 is a mismatch.  Also without T_in (composed onto
    the identity), without pose, without moved and without T_out: what is asked for stays equal."""
    pred, src, T, moved, T_out, M = P.apply_exact_case(B, N)
    got = _apply_fwd(dev, pred, src, T, N, 0.0, 0)
    for name, g, w in zip(("pose", "moved", "T_out"), got, (pred, moved, T_out)):
        P.same_values(g, w, name)
    q_eye = _apply_fwd(dev, pred, src, None, N, 0.0, 0, want_pose=False)
    assert q_eye[0] is None
    P.same_values(q_eye[1], moved, "moved (no T_in, no pose)")
    P.same_values(q_eye[2], M, "T_out (no T_in)")
    no_moved = _apply_fwd(dev, pred, src, T, N, 0.0, 0, want_moved=False)
    assert no_moved[1] is None
    P.same_values(no_moved[0], pred, "pose (no moved)")
    P.same_values(no_moved[2], T_out, "T_out (no moved)")
    no_T = _apply_fwd(dev, pred, src, None, N, 0.0, 0, want_T=False)
    assert no_T[2] is None
    P.same_values(no_T[0], pred, "pose (no T_out)")
    P.same_values(no_T[1], moved, "moved (no T_out)")


def _real_rows(B, N, lim):
    """row kinds of a real-valued batch: over the (B, N) grid every limit meets a regular row, a zero axis and a saturated tanh
    (lim != 0: p0..3 = +-20, the three translations and the angle), or a zero quaternion (lim = 0)"""
    kinds = ("regular", "zero_axis", "saturated") if lim else ("regular", "zero_quat")
    if B == 1:
        return [kinds[P.APPLY_N.index(N) % len(kinds)]]
    return [kinds[b % len(kinds)] for b in range(B)]


def _real_case(B, N, lim):
    g = torch.Generator().manual_seed(6000 + 10 * N + B + int(lim))
    pred = torch.randn(B, 7, generator=g) * torch.tensor([2.0, 2.0, 2.0, 1.5, 1.0, 1.0, 1.0])
    if lim == 0.0:
        pred[:, 3:] = torch.nn.functional.normalize(pred[:, 3:], dim=1) * (1 + 0.3 * torch.rand(B, 1, generator=g))
    kinds = _real_rows(B, N, lim)
    for b, kind in enumerate(kinds):
        if kind == "zero_axis":
            pred[b, 4:] = 0.0
        if kind == "saturated":
            pred[b, :4] = torch.tensor([20.0, -20.0, 20.0, -20.0])
        if kind == "zero_quat":
            pred[b, 3:] = 0.0
    assert float(pred.abs().max()) <= 30.0               # the fp32 squares do not overflow
    src = torch.rand(B, N, 3, generator=g) * 2 - 1
    T = torch.eye(4).repeat(B, 1, 1) + 0.1 * torch.randn(B, 4, 4, generator=g)
    T[:, 3] = torch.tensor([0.0, 0.0, 0.0, 1.0])
    w = torch.randn(B, N, 3, generator=g)
    return pred.numpy(), src.numpy(), T.numpy(), w.numpy(), kinds


@pytest.mark.parametrize("lim", [45.0, 10.0, 0.0])
@pytest.mark.parametrize("N", P.APPLY_N)
@pytest.mark.parametrize("B", P.APPLY_B)
def test_apply_real_family(dev, B, N, lim):
    """both modes against the float64 torch algebra within 2e-6; the backward of the training evaluation against float64 autograd within
    2e-5 max(1, |grad|) of the row.  Degenerate rows: a zero axis; a zero quaternion at lim = 0 (moved IS t, no gradient reaches q,
    everything finite); saturated tanh (|p| = 20: that gradient is exactly 0)."""
    pred, src, T, w, kinds = _real_case(B, N, lim)
    for mode in (0, 1):
        _, pose, moved, Tn = _pose_reference(pred, src, T, lim, mode)
        got = _apply_fwd(dev, pred, src, T, N, lim, mode)
        for name, x, y in zip(("pose", "moved", "T"), got, (pose, moved, Tn)):
            assert np.isfinite(x).all(), (mode, name)
            err = np.abs(x.astype(np.float64) - y.detach().numpy()).max()
            assert err <= 2e-6, (mode, name, err)
        for b, kind in enumerate(kinds):
            if kind == "zero_quat":
                P.same_values(got[1][b], np.broadcast_to(pred[b, :3], (N, 3)), "moved of a zero quaternion")
    # backward of the training evaluation (mode 1)
    p64, _, moved, _ = _pose_reference(pred, src, None, lim, 1)
    (moved * torch.as_tensor(w, dtype=torch.float64)).sum().backward()
    ref = p64.grad.numpy().copy()
    for b, kind in enumerate(kinds):
        if kind == "zero_quat":      # (autograd differentiates sqrt at 0: NaN; the chain's own value there: dt = sum of d moved, dq = 0)
            ref[b] = np.concatenate([w[b].astype(np.float64).sum(0), np.zeros(4)])
    assert np.isfinite(ref).all()
    bufs = Buffers(dev)
    dpred = bufs.out(B * 7)
    rc = L.load().dpd_pose_apply_bwd(ptr(bufs.put(pred)), ptr(bufs.put(src)), ptr(bufs.put(w)), B, N, float(lim), ptr(dpred), L.cur_stream())
    assert rc == 0, rc
    bufs.check()
    got = host(dpred, B, 7)
    assert np.isfinite(got).all()
    for b, kind in enumerate(kinds):
        err = np.abs(got[b].astype(np.float64) - ref[b]).max()
        bar = 2e-5 * max(1.0, np.abs(ref[b]).max())
        print("B=%d N=%d lim=%g row %d (%s): gradient error %.3e, bar %.3e" % (B, N, lim, b, kind, err, bar))
        assert err <= bar, (b, kind, err, bar)
        if kind == "saturated":
            P.same_values(got[b, :4], np.zeros(4), "gradient through a saturated tanh")
        if kind == "zero_quat":
            P.same_values(got[b, 3:], np.zeros(4), "gradient of a zero quaternion")

"""The average-pool pose encoder (`--pn_pool avg`, models/ipcr_model.py:236-271) on the GPU, through the `_pool` entries of
include/dpdist_capi.h and through the Python harness.

1. exact values on the integer network (tests/pose_avg_cases.py: f = float32(S / N), gate words, all ten gradients), every output and an
   exact-size workspace NaN-filled between guard bands;  2. DPD_POOL_MAX through the new entries is the old entries bit for bit;
3. the forward-only refinement;  4. real values against float64 torch autograd of the mean-pool network at the bars of
tests/test_registration_points.py;  5. the module and the harness;  6. determinism;  7. refusals.

On 3: dpd_pose_refine adds the two halves of the head's first layer in another order than dpd_pose_head_fwd_train (the template's half
once per call as a row bias; the training head contracts all 2048 inputs in one pass) -- both max-pool forms of before, not touched
here.  The composition dpd_pose_point_fwd_train_pool -> dpd_pose_head_fwd_train -> dpd_pose_apply_fwd can therefore equal the refinement
BIT FOR BIT only where every sum of the head is exact, i.e. where the pooled features are exactly representable small numbers: the
integer network with clouds whose S / N is a dyadic rational -- N = 64: any cloud (S / 64); N = 200: eight distinct points, 25 copies of
each (S / 200 = S8 / 8); N = 65: one point, 65 copies (S / 65 = a5, an integer).  A row left out, a padded row summed or another cloud
read breaks S / N all the same.  That the forward-only form makes the FEATURE bits of the training form on real clouds, with and without
its pose-move prologue, is checked on the features themselves (the first 2 B 1024 floats of the refinement's workspace, csrc/pose.hip
`refine_ws`)."""
from ctypes import byref

import numpy as np
import pytest
import torch

from dpdist_amd import lib as L
from dpdist_amd import synth
from dpdist_amd.registration import PoseNet, compose, quat_normalize, transformation_quat_tensor

from . import pose_avg_cases as A
from . import pose_cases as P
from .gemm_cases import EXACT, NAN_OUT, untouched
from .test_pose_edges_gpu import Buffers, device_net, host, ptr, ptrs

pytestmark = pytest.mark.gpu

MAX, AVG = 0, 1
WIDTHS = (64, 64, 64, 128)
E_NULL, E_DIM, E_UNSUPPORTED, E_WORKSPACE = -1, -2, -3, -4


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible")
    L.load()     # raises if the HIP extension is missing -- never fall back
    return torch.device("cuda:0")


def _case(cid):
    return next(c for c in P.POINT_CASES if c.id == cid)


def forward(dev, net, a_np, b_np, N, pool, old=False):
    """dpd_pose_point_fwd_train_pool (old: dpd_pose_point_fwd_train) on banded buffers -> dict of numpy arrays f, h1 .. h4, words"""
    lib = L.load()
    nA, nB = len(a_np), len(b_np)
    C, NW = nA + nB, (N + 63) // 64
    bufs = Buffers(dev)
    a, b = bufs.put(a_np), (bufs.put(b_np) if nB else None)
    f, h = bufs.out(C * P.OUT), [bufs.out(C * N * w) for w in WIDTHS]
    words = bufs.out(2 * C * NW * P.OUT, torch.int32)
    if old:
        rc = lib.dpd_pose_point_fwd_train(byref(net), ptr(a), ptr(b), nA, nB, N, ptr(f), ptr(h[0]), ptr(h[1]), ptr(h[2]), ptr(h[3]), ptr(words),
                                          L.cur_stream())
    else:
        rc = lib.dpd_pose_point_fwd_train_pool(byref(net), ptr(a), ptr(b), nA, nB, N, pool, ptr(f), ptr(h[0]), ptr(h[1]), ptr(h[2]), ptr(h[3]),
                                               ptr(words), L.cur_stream())
    assert rc == 0, rc
    bufs.check()
    got = {"f": host(f, C, P.OUT), "words": host(words.view(torch.int64), C, NW, P.OUT).view(np.uint64)}
    got.update({"h%d" % (i + 1): host(h[i], C * N, w) for i, w in enumerate(WIDTHS)})
    return got


def backward(dev, net, a_np, b_np, N, pool, df, hs, words, old=False):
    """dpd_pose_point_bwd_pool (old: dpd_pose_point_bwd) on banded buffers, the workspace at exactly its reported size -> dW1 .. db5"""
    lib = L.load()
    nA, nB = len(a_np), len(b_np)
    C = nA + nB
    bufs = Buffers(dev)
    a, b = bufs.put(a_np), (bufs.put(b_np) if nB else None)
    hin = [bufs.put(x) for x in hs]
    win, dfin = bufs.put_words(words), bufs.put(df)
    nbytes = lib.dpd_pose_point_bwd_workspace_bytes_n(C, N) if old else lib.dpd_pose_point_bwd_workspace_bytes_pool(C, N, pool)
    assert nbytes > 0 and nbytes % 4 == 0
    ws = bufs.out(nbytes // 4)
    dW = [bufs.out(o * i) for i, o in P.POINT_WIDTHS]
    db = [bufs.out(o) for _, o in P.POINT_WIDTHS]
    if old:
        rc = lib.dpd_pose_point_bwd(byref(net), ptr(a), ptr(b), nA, nB, N, ptr(dfin), ptr(hin[0]), ptr(hin[1]), ptr(hin[2]), ptr(hin[3]), ptr(win),
                                    ptrs(dW), ptrs(db), ptr(ws), nbytes, L.cur_stream())
    else:
        rc = lib.dpd_pose_point_bwd_pool(byref(net), ptr(a), ptr(b), nA, nB, N, pool, ptr(dfin), ptr(hin[0]), ptr(hin[1]), ptr(hin[2]), ptr(hin[3]),
                                         ptr(win), ptrs(dW), ptrs(db), ptr(ws), nbytes, L.cur_stream())
    assert rc == 0, rc
    bufs.check()
    got = {"dW%d" % (l + 1): host(dW[l], o, i) for l, (i, o) in enumerate(P.POINT_WIDTHS)}
    got.update({"db%d" % (l + 1): host(db[l], o) for l, (_, o) in enumerate(P.POINT_WIDTHS)})
    return got


def same_bits(x, y):
    return x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes()


# ------------------------------------------------------------------------------------------------ 1. exact values
def avg_case(dev, case):
    """forward, then the backward on the reference's activations, gate words and df = N k: dict of every array of A.AVG_NAMES"""
    net = device_net(dev, case.net)
    _, bwd, want = A.avg_reference(case)
    a, b = P.point_clouds(case)
    got = forward(dev, net, a, b, case.N, AVG)
    got.update(backward(dev, net, a, b, case.N, AVG, bwd["df"], [want["h%d" % i] for i in range(1, 5)], want["words"]))
    return got


@pytest.mark.parametrize("case", P.POINT_CASES, ids=[c.id for c in P.POINT_CASES])
def test_avg_point_case(dev, case):
    """f = float32(S / N), h1 .. h4, every gate word (no bit at or beyond N) and all ten gradients equal the float64 reference"""
    _, _, want = A.avg_reference(case)
    got = avg_case(dev, case)
    P.check(got, want, A.AVG_NAMES)


# ------------------------------------------------------------------------------------------------ 2. max through the new entries
@pytest.mark.parametrize("cid", ["plain-plain-N33-C2+1", "plain-plain-N129-C2+1", "plain-plain-N2048-C1+1"])
def test_max_pool_through_the_pool_entries_is_the_old_entries(dev, cid):
    case = _case(cid)
    net = device_net(dev, case.net)
    _, bwd, want = P.point_reference(case)
    a, b = P.point_clouds(case)
    lib = L.load()
    C = case.nA + case.nB
    assert lib.dpd_pose_point_bwd_workspace_bytes_pool(C, case.N, MAX) == lib.dpd_pose_point_bwd_workspace_bytes_n(C, case.N)
    new, old = forward(dev, net, a, b, case.N, MAX), forward(dev, net, a, b, case.N, MAX, old=True)
    hs = [want["h%d" % i] for i in range(1, 5)]
    new.update(backward(dev, net, a, b, case.N, MAX, bwd["df"], hs, want["ties"]))
    old.update(backward(dev, net, a, b, case.N, MAX, bwd["df"], hs, want["ties"], old=True))
    for n in new:
        assert same_bits(new[n], old[n]), n
    assert np.array_equal(new["words"], want["ties"])                      # ... and they are the max pool's tie words, not gate words


# ------------------------------------------------------------------------------------------------ 3. refinement
def _refine(dev, net, src, tmpl, loops, pool, mask=None, lim=P.REFINE_LIM, old=False, keep_ws=False):
    """dpd_pose_refine_pool on banded buffers -> pred [loops, B, 7], moved, T_out (numpy) [, the workspace tensor]"""
    lib = L.load()
    B, N = src.shape[:2]
    bufs = Buffers(dev)
    s, t = bufs.put(src), bufs.put(tmpl)
    m = None if mask is None else bufs.put(mask)
    nbytes = lib.dpd_pose_refine_workspace_bytes(B, N, P.OUT)
    ws, moved, T_out, pred = bufs.out(nbytes // 4), bufs.out(B * N * 3), bufs.out(B * 16), bufs.out(loops * B * 7)
    if old:
        rc = lib.dpd_pose_refine(byref(net), ptr(s), ptr(t), B, N, loops, lim, ptr(m), ptr(ws), nbytes, ptr(moved), ptr(T_out), ptr(pred), L.cur_stream())
    else:
        rc = lib.dpd_pose_refine_pool(byref(net), ptr(s), ptr(t), B, N, loops, lim, pool, ptr(m), ptr(ws), nbytes, ptr(moved), ptr(T_out), ptr(pred),
                                      L.cur_stream())
    assert rc == 0, rc
    bufs.check()
    out = (host(pred, loops, B, 7), host(moved, B, N, 3), host(T_out, B, 4, 4))
    return out + (ws,) if keep_ws else out


def _dyadic_clouds(rng, C, N):
    """integer clouds [C, N, 3] whose average-pooled features are exact (module docstring): m distinct points, N / m copies of each in
    shuffled order (the copies spread over the 64-point passes), m = the largest power of two that divides N (at most 64)"""
    m = min(N & -N, 64)
    pts = np.repeat(rng.integers(-4, 5, size=(C, m, 3)).astype(np.int64), N // m, axis=1)
    for c in range(C):
        pts[c] = pts[c, rng.permutation(N)]
    return pts, m


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("N", [64, 65, 200])
@pytest.mark.parametrize("B", [1, 16, 17])
def test_avg_refinement_first_loop_is_the_composition_of_the_training_entries(dev, B, N, masked):
    """loops = 1: pred_out, moved and T_out of dpd_pose_refine_pool have the bits of dpd_pose_point_fwd_train_pool ->
    dpd_pose_head_fwd_train -> dpd_pose_apply_fwd (integer network, clouds with exactly representable features: module docstring);
    the features are not integers and the pose moves the cloud"""
    lib = L.load()
    net = device_net(dev)
    rng = np.random.default_rng(7000 + 100 * B + N)
    (src, m), (tmpl, _) = _dyadic_clouds(rng, B, N), _dyadic_clouds(rng, B, N)
    mask = 2 * rng.integers(0, 2, size=(1, B, 256)).astype(np.int64) if masked else None
    pred, moved, T_out = _refine(dev, net, src, tmpl, 1, AVG, mask)
    fwd = forward(dev, net, src, tmpl, N, AVG)
    ref = A.avg_forward(P.point_net("plain"), np.concatenate([src, tmpl]))
    P.same_values(fwd["f"], ref["f"], "f")
    assert np.array_equal(ref["f"] * m, np.rint(ref["f"] * m))             # multiples of 1 / m ...
    if m > 1:
        assert (ref["f"] != np.rint(ref["f"])).mean() > 0.2                  # ... and not integers
    head = P.head_forward(P.head_net(), ref["f"], None if mask is None else mask[0])
    print("B=%d N=%d: features in units of 1/%d, the head's largest sum of absolute terms %.3e" % (B, N, m, head["bound"]))
    assert head["bound"] * m < EXACT                                         # every sum of the head is exact in fp32, in any order
    P.same_values(pred[0], head["pred"], "pred_out")
    bufs = Buffers(dev)
    f = bufs.put(fwd["f"])
    dm = None if mask is None else bufs.put(mask[0])
    outs = [bufs.out(B * w) for w in (1024, 512, 256, 7)]
    rc = lib.dpd_pose_head_fwd_train(byref(net), ptr(f), B, ptr(dm), ptr(outs[0]), ptr(outs[1]), ptr(outs[2]), ptr(outs[3]), L.cur_stream())
    assert rc == 0, rc
    s = bufs.put(src)
    mv, T = bufs.out(B * N * 3), bufs.out(B * 16)
    rc = lib.dpd_pose_apply_fwd(ptr(outs[3]), ptr(s), None, B, N, P.REFINE_LIM, 0, None, ptr(mv), ptr(T), L.cur_stream())
    assert rc == 0, rc
    bufs.check()
    assert same_bits(pred[0], host(outs[3], B, 7)), "pred_out"
    assert same_bits(moved, host(mv, B, N, 3)), "moved"
    assert same_bits(T_out, host(T, B, 4, 4)), "T_out"
    assert np.abs(moved.astype(np.float64) - src).max() > 1e-2
    pmax, _, _ = _refine(dev, net, src, tmpl, 1, MAX, mask)
    assert same_bits(pmax, pred) == (m == 1)                                 # (the mean of 65 copies of one point IS its maximum)


def _real_net(dev, seed=11, pool="avg"):
    """a pose network with biases that are not all zero and a head that actually moves the cloud (tests/test_registration.py)"""
    torch.manual_seed(seed)
    net = PoseNet(pool=pool).to(dev)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.Linear):
                m.bias.normal_(0.0, 0.05)
        net.head[-1].bias.copy_(torch.tensor([0.3, -0.2, 0.1, 0.25, 0.4, -0.3, 0.8], device=dev))
    return net


def _struct(net):
    from dpdist_amd.registration import _pose_net_struct, _weights
    wb = _weights(net.point, net.head)
    return _pose_net_struct(wb), wb


@pytest.mark.parametrize("B,N", [(3, 100), (16, 64)])
def test_forward_only_form_makes_the_training_forms_feature_bits(dev, B, N):
    """real weights and clouds, two loops: the features the refinement leaves in its workspace (rows < B: the source as loop 2 saw it,
    moved by the prologue of the forward-only kernel; rows >= B: the template, from loop 1) have the bits of
    dpd_pose_point_fwd_train_pool on (the moved cloud of a one-loop call, the template)"""
    net = _real_net(dev)
    w, keep = _struct(net)
    src, tmpl, _ = synth.registration_pairs(B, N, seed=5)
    _, moved1, _ = _refine(dev, w, src, tmpl, 1, AVG, lim=net.lim_rot)
    _, _, _, ws = _refine(dev, w, src, tmpl, 2, AVG, lim=net.lim_rot, keep_ws=True)
    f_ws = host(ws[:2 * B * P.OUT], 2 * B, P.OUT)
    f_train = forward(dev, w, moved1, tmpl, N, AVG)["f"]
    assert same_bits(f_ws, f_train)
    assert not same_bits(f_ws[:B], forward(dev, w, src, tmpl, N, AVG)["f"][:B])          # the prologue did move the source
    del keep


@pytest.mark.parametrize("B,N,loops", [(16, 64, 3), (5, 50, 3), (3, 150, 3)])
def test_avg_refinement_matches_the_float64_network(B, N, loops, dev):
    """three loops with real weights against the float64 torch restatement with `.mean(1)`, at the bars of the max-pool refinement test
    of tests/test_registration.py: raw outputs 2e-5 relative, moved cloud and transform 5e-5; with and without a dropout mask"""
    from dpdist_amd.registration import pose_refine_native
    net = _real_net(dev)
    src, tmpl, _ = synth.registration_pairs(B, N, seed=5)
    src, tmpl = torch.tensor(src, device=dev), torch.tensor(tmpl, device=dev)
    g = torch.Generator(device="cpu").manual_seed(1)
    net64 = PoseNet(pool="avg").double().to(dev)
    net64.load_state_dict({k: v.double() for k, v in net.state_dict().items()})
    for mask in (None, (torch.rand(loops, B, 256, generator=g) < 0.7).float().div(0.7).to(dev)):
        moved, T, pred = pose_refine_native(net, src, tmpl, loops, mask, want_pred=True)
        s, t = src.double(), tmpl.double()
        Tr = torch.eye(4, device=dev, dtype=torch.float64).repeat(B, 1, 1)
        with torch.no_grad():
            for it in range(loops):
                f = net64.point(torch.cat([s, t], 0)).mean(1)
                h = net64.head[:6](torch.cat([f[:B], f[B:]], 1))
                if mask is not None:
                    h = h * mask[it].double()
                raw = net64.head[7](h)
                err = (pred[it].double() - raw).abs().max().item()
                print("B=%d N=%d loop %d: raw output error %.3e (scale %.3e)" % (B, N, it, err, raw.abs().max().item()))
                assert err <= 2e-5 * max(1.0, raw.abs().max().item()), (it, "raw output")
                pose = quat_normalize(raw, net.lim_rot)
                pose = torch.cat([pose[:, :3], pose[:, 3:7] / pose[:, 3:7].norm(dim=1, keepdim=True).clamp_min(1e-12)], 1)
                s = transformation_quat_tensor(s, pose[:, 3:7], pose[:, :3])
                Tr = compose(Tr, pose)
        assert (s - src.double()).abs().max().item() > 1e-2          # the loops did move the cloud
        em, eT = (moved.double() - s).abs().max().item(), (T.double() - Tr).abs().max().item()
        print("B=%d N=%d: |moved - float64| = %.3e, |T - float64| = %.3e" % (B, N, em, eT))
        assert em <= 5e-5 and eT <= 5e-5


# ------------------------------------------------------------------------------------------------ 4. real values
def _biased_net(dev, seed, pool="avg"):
    torch.manual_seed(seed)
    net = PoseNet(pool=pool).to(dev)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.Linear):
                m.bias.normal_(0.0, 0.05)
    return net


def _net64(net, dev):
    net64 = PoseNet(pool=net.pool).double().to(dev)
    net64.load_state_dict({k: v.double() for k, v in net.state_dict().items()})
    return net64


def _linear_params(net, head):
    seqs = (net.point, net.head) if head else (net.point,)
    return [t for seq in seqs for m in seq if isinstance(m, torch.nn.Linear) for t in (m.weight, m.bias)]


def point_evaluation(dev, C, N):
    """_PointFeaturesFn under the average pool on C clouds of N points: (features, the ten gradients) of the library, and the inputs"""
    net = _biased_net(dev, 3)
    src, tmpl, _ = synth.registration_pairs(max(1, C), N, seed=9)
    clouds = torch.tensor(np.concatenate([src, tmpl])[:C], device=dev)
    up = torch.randn(C, 1024, generator=torch.Generator().manual_seed(5)).to(dev)
    params = _linear_params(net, head=False)
    f = net._pooled(clouds)
    assert type(f.grad_fn).__name__ == "_PointFeaturesFnBackward"
    grads = torch.autograd.grad((f * up).sum(), params)
    return net, clouds, up, f.detach(), grads


@pytest.mark.parametrize("N", [64, 100, 1024])
@pytest.mark.parametrize("C", [3, 32])
def test_avg_training_evaluation_against_float64_autograd(dev, C, N):
    """features 2e-5 relative, every gradient 1e-3 of the tensor's largest entry: the bars of tests/test_registration_points.py.  The
    oracle is torch autograd of the same layers and `.mean(1)` in float64."""
    net, clouds, up, f, grads = point_evaluation(dev, C, N)
    net64 = _net64(net, dev)
    p64 = _linear_params(net64, head=False)
    f64 = net64.point(clouds.double()).mean(1)
    g64 = torch.autograd.grad((f64 * up.double()).sum(), p64)
    f_err, scale = (f.double() - f64).abs().max().item(), f64.abs().max().item()
    worst = [(n, (a.double() - r).abs().max().item() / max(1e-6, r.abs().max().item()))
             for n, a, r in zip(["W1", "b1", "W2", "b2", "W3", "b3", "W4", "b4", "W5", "b5"], grads, g64)]
    print("C=%d N=%d: feature error %.3e (scale %.3e); gradient errors / largest entry: %s"
          % (C, N, f_err, scale, " ".join("%s=%.2e" % w for w in worst)))
    assert f_err <= 2e-5 * max(1.0, scale)
    for name, rel in worst:
        assert rel <= 1e-3, (name, rel)


def raw_evaluation(dev, B, N):
    """_PoseNetRawFn under the average pool with a dropout mask: (raw output, the 18 gradients), and the inputs"""
    from dpdist_amd.registration import _PoseNetRawFn
    net = _biased_net(dev, 4)
    src, tmpl, _ = synth.registration_pairs(B, N, seed=3)
    clouds = torch.tensor(np.concatenate([src, tmpl]), device=dev)
    g = torch.Generator().manual_seed(7)
    mask = (torch.rand(B, 256, generator=g) < 0.7).float().div(0.7).to(dev)
    up = torch.randn(B, 7, generator=g).to(dev)
    params = _linear_params(net, head=True)
    pred = _PoseNetRawFn.apply(clouds[:B].contiguous(), clouds[B:].contiguous(), mask, None, *params, L.POOLS["avg"])
    grads = torch.autograd.grad((pred * up).sum(), params)
    return net, clouds, mask, up, pred.detach(), grads


@pytest.mark.parametrize("N", [64, 100, 1024])
@pytest.mark.parametrize("C", [3, 32])
def test_avg_one_node_evaluation_against_float64_autograd(dev, C, N):
    """the whole network as one node (B = ceil(C / 2) pairs, with a dropout mask): raw output 2e-5 relative, all 18 gradients 1e-3 of the
    tensor's largest entry"""
    B = (C + 1) // 2
    net, clouds, mask, up, pred, grads = raw_evaluation(dev, B, N)
    net64 = _net64(net, dev)
    p64 = _linear_params(net64, head=True)
    f = net64.point(clouds.double()).mean(1)
    h = net64.head[:6](torch.cat([f[:B], f[B:]], 1)) * mask.double()
    ref = net64.head[7](h)
    gref = torch.autograd.grad((ref * up.double()).sum(), p64)
    perr = (pred.double() - ref).abs().max().item()
    worst = [(a.double() - r).abs().max().item() / max(1e-6, r.abs().max().item()) for a, r in zip(grads, gref)]
    print("B=%d N=%d: output error %.3e (scale %.3e); gradient errors / largest entry: %s"
          % (B, N, perr, ref.abs().max().item(), " ".join("%.2e" % w for w in worst)))
    assert perr <= 2e-5 * max(1.0, ref.abs().max().item())
    for i, rel in enumerate(worst):
        assert rel <= 1e-3, (i, rel)


# ------------------------------------------------------------------------------------------------ 5. module and harness
class _Spy:
    """counts the calls of one library entry and keeps their `pool` argument (position 6 of the point entries)"""

    def __init__(self, name):
        self.name, self.lib, self.pools = name, L.load(), []
        self.orig = getattr(self.lib, name)

    def __enter__(self):
        def call(*args):
            self.pools.append(args[6])
            return self.orig(*args)
        setattr(self.lib, self.name, call)
        return self

    def __exit__(self, *exc):
        setattr(self.lib, self.name, self.orig)


@pytest.mark.parametrize("N", [64, 100])
def test_avg_module_takes_the_library_node(dev, N):
    net = _biased_net(dev, 4)
    src, tmpl, _ = synth.registration_pairs(4, N, seed=3)
    src, tmpl = torch.tensor(src, device=dev), torch.tensor(tmpl, device=dev)
    net.eval()
    with _Spy("dpd_pose_point_fwd_train_pool") as fw, _Spy("dpd_pose_point_bwd_pool") as bw:
        out_n = net.raw(src, tmpl)
        assert type(out_n.grad_fn).__name__ == "_PoseNetRawFnBackward"
        out_n.sum().backward()
        assert fw.pools == [AVG] and bw.pools == [AVG]
        f = net._pooled(torch.cat([src, tmpl], 0))
        assert type(f.grad_fn).__name__ == "_PointFeaturesFnBackward" and fw.pools == [AVG, AVG]
        assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in net.parameters())
        net.native_train = False
        try:
            out_t = net.raw(src, tmpl)
        finally:
            net.native_train = True
        assert fw.pools == [AVG, AVG]                                     # the torch form calls nothing
    assert type(out_t.grad_fn).__name__ != "_PoseNetRawFnBackward"
    assert (out_t - out_n).abs().max().item() <= 2e-5 * max(1.0, out_t.abs().max().item())
    with _Spy("dpd_pose_point_fwd_train_pool") as fw:                     # ... and the max-pool module goes through the same entry with MAX
        _biased_net(dev, 4, "max").raw(src, tmpl)
        assert fw.pools == [MAX]


def _registration_run(dev, graph, pool="avg", steps=2, B=4, N=100):
    from dpdist_amd.model import DPDistLoss, DPDistModel
    from dpdist_amd.registration import IterativeRegistration
    torch.manual_seed(0)
    model = DPDistModel(device=dev)
    model.load_tf_state_dict(synth.make_weights("wide"))
    net = PoseNet(pool=pool).to(dev)
    torch.manual_seed(1000)
    rng = np.random.default_rng(0)
    reg = IterativeRegistration(net, DPDistLoss(model), lr=1e-4, max_loops=3, distributed=False, graph=graph, graph_warmup=1)
    losses, Ts = [], []
    for _ in range(steps):
        src, tmpl, _ = synth.registration_pairs(B, N, rng=rng)
        loss, T = reg.train_step(torch.tensor(src, device=dev), torch.tensor(tmpl, device=dev))
        losses.append(loss.clone())
        Ts.append(T.clone())
    torch.cuda.synchronize()
    assert reg.graph_replays == (steps - 1 if graph else 0), reg.graph_replays
    w = torch.cat([p.detach().reshape(-1) for p in net.parameters()]).clone()
    reg.close()
    return w, torch.stack(Ts), torch.stack(losses)


def test_avg_registration_step_is_bitwise_graph_and_eager(dev):
    """IterativeRegistration with an average-pool network at B = 4, N = 100, three loops, two training steps (one eager, one captured
    and replayed): the same pose network, transforms and losses bit for bit as two eager steps; the library's `_pool` entries ran"""
    with _Spy("dpd_pose_point_bwd_pool") as bw:
        e = _registration_run(dev, False)
        assert bw.pools == [AVG, AVG]
        g = _registration_run(dev, True)
    for x, y, name in zip(g, e, ("weights", "transforms", "losses")):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), name
    assert torch.isfinite(e[0]).all() and torch.isfinite(e[2]).all()
    m = _registration_run(dev, False, pool="max", steps=1)
    assert not torch.equal(m[2][0], e[2][0])


def test_no_stop_test_runs_the_avg_network(dev):
    """regtest.no_stop_test on an average-pool network returns the final transforms of pose_refine_native bit for bit, and they are not
    the transforms the same weights give under the max pool"""
    from dpdist_amd import regtest
    from dpdist_amd.registration import pose_refine_native
    net = _real_net(dev).eval()
    src, tmpl, gt = synth.registration_pairs(5, 100, seed=3)
    res = regtest.no_stop_test(net, src, tmpl, gt, iterations=4, batch=16)
    s, t = torch.tensor(src, device=dev), torch.tensor(tmpl, device=dev)
    with torch.no_grad():
        _, T = pose_refine_native(net, s, t, 4)
        net.pool = "max"
        try:
            _, Tmax = pose_refine_native(net, s, t, 4)
        finally:
            net.pool = "avg"
    assert same_bits(res["T"], T.cpu().numpy())
    assert np.isfinite(res["T"]).all() and np.abs(res["T"] - Tmax.cpu().numpy()).max() > 1e-3


# ------------------------------------------------------------------------------------------------ 6. determinism
def test_two_runs_give_the_same_bytes(dev):
    case = _case("plain-plain-N200-C2+1")
    x, y = avg_case(dev, case), avg_case(dev, case)
    for n in x:
        assert same_bits(x[n], y[n]), n
    a, b = raw_evaluation(dev, 16, 1024), raw_evaluation(dev, 16, 1024)
    assert torch.equal(a[4].view(torch.int32), b[4].view(torch.int32))
    assert all(torch.equal(p.view(torch.int32), q.view(torch.int32)) for p, q in zip(a[5], b[5]))


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals_leave_the_outputs_untouched(dev):
    """pool = 2, N = 2049 on the training entries and a workspace one byte short: the documented codes, and not one output element
    written"""
    lib = L.load()
    net = device_net(dev)
    C, N = 2, 70
    NW = (N + 63) // 64
    bufs = Buffers(dev)
    pts = bufs.put(np.zeros((C, 2049, 3)))
    f, h = bufs.out(C * P.OUT), [bufs.out(C * 2049 * w) for w in WIDTHS]
    words = bufs.out(2 * C * 33 * P.OUT, torch.int32)
    nbytes = lib.dpd_pose_point_bwd_workspace_bytes_pool(C, N, AVG)
    ws = bufs.out(nbytes // 4)
    dW = [bufs.out(o * i) for i, o in P.POINT_WIDTHS]
    db = [bufs.out(o) for _, o in P.POINT_WIDTHS]
    outs = [f, words, ws] + h + dW + db

    def fwd(pool, n):
        return lib.dpd_pose_point_fwd_train_pool(byref(net), ptr(pts), None, C, 0, n, pool, ptr(f), ptr(h[0]), ptr(h[1]), ptr(h[2]), ptr(h[3]),
                                                 ptr(words), L.cur_stream())

    def bwd(pool, n, nb):
        return lib.dpd_pose_point_bwd_pool(byref(net), ptr(pts), None, C, 0, n, pool, ptr(f), ptr(h[0]), ptr(h[1]), ptr(h[2]), ptr(h[3]), ptr(words),
                                           ptrs(dW), ptrs(db), ptr(ws), nb, L.cur_stream())

    assert fwd(2, N) == E_UNSUPPORTED and fwd(-1, N) == E_UNSUPPORTED and bwd(2, N, nbytes) == E_UNSUPPORTED
    assert fwd(AVG, 2049) == E_UNSUPPORTED and bwd(AVG, 2049, nbytes) == E_UNSUPPORTED
    assert fwd(MAX, 2049) == E_UNSUPPORTED and bwd(MAX, 2049, nbytes) == E_UNSUPPORTED
    assert bwd(AVG, N, nbytes - 1) == E_WORKSPACE
    assert bwd(MAX, N, lib.dpd_pose_point_bwd_workspace_bytes_pool(C, N, MAX) - 1) == E_WORKSPACE
    assert lib.dpd_pose_point_bwd_workspace_bytes_pool(C, N, 2) == 0 and lib.dpd_pose_point_bwd_workspace_bytes_pool(C, 2049, AVG) == 0
    # the refinement: an unknown pool and a short workspace
    rb = lib.dpd_pose_refine_workspace_bytes(C, N, P.OUT)
    rws, moved, T_out = bufs.out(rb // 4), bufs.out(C * N * 3), bufs.out(C * 16)
    outs += [rws, moved, T_out]

    def refine(pool, nb):
        return lib.dpd_pose_refine_pool(byref(net), ptr(pts), ptr(pts), C, N, 1, 45.0, pool, None, ptr(rws), nb, ptr(moved), ptr(T_out), None,
                                        L.cur_stream())
    assert refine(2, rb) == E_UNSUPPORTED and refine(AVG, rb - 1) == E_WORKSPACE
    bufs.check()
    for t in outs:
        assert untouched(t, NAN_OUT)

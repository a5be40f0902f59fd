"""The pose network's training evaluation on the library above 64 points per cloud (csrc/pose.hip: the max pool's tie mask over several
64-point passes, the backward chunked per (cloud, 64 points)): the reference registers at 256 .. 2048 points, default 512
(pcrnet-registration/iterative_PCRNet_ours.py:40,103-104)."""
import numpy as np
import pytest
import torch

from dpdist_amd import synth
from dpdist_amd.registration import PoseNet


def _biased_net(dev, seed):
    torch.manual_seed(seed)
    net = PoseNet().to(dev)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.Linear):
                m.bias.normal_(0.0, 0.05)
    return net


def _net64(net, dev):
    net64 = PoseNet().double().to(dev)
    net64.load_state_dict({k: v.double() for k, v in net.state_dict().items()})
    return net64


def _native_pool_selection(net, clouds):
    """The max pool's selection as the LIBRARY's forward made it (dpd_pose_point_fwd_train's tie words, ties [C, W, 1024]: bit b of word w is
    point 64 w + b): sel [C,N,1024] float64 with 1 / (number of tied points) at the points that attain a column's positive maximum, the
    raw 0/1 bits, and the features.  A float64 reference pools with THIS selection (two points equal to fp32 rounding may be ordered
    differently by two fp32 forwards; the gradient of max is discontinuous there)."""
    from ctypes import byref
    from dpdist_amd import lib as L
    C, N, _ = clouds.shape
    lin = [m for m in net.point if isinstance(m, torch.nn.Linear)]
    w = L.PoseNetW()
    for i, m in enumerate(lin):
        w.Wp[i], w.bp[i] = m.weight.data_ptr(), m.bias.data_ptr()
    w.out_features = 1024
    dev = clouds.device
    lib = L.load()
    W = lib.dpd_pose_point_tie_words(N)
    assert W == (N + 63) // 64
    e = lambda *sh: torch.empty(*sh, device=dev)      # noqa: E731
    f, h = e(C, 1024), [e(C * N, k) for k in (64, 64, 64, 128)]
    ties = torch.full((C, W, 1024), -1, device=dev, dtype=torch.int64)
    L.check(lib.dpd_pose_point_fwd_train(byref(w), L.ptr(clouds.contiguous()), None, C, 0, N, L.ptr(f), L.ptr(h[0]), L.ptr(h[1]), L.ptr(h[2]),
                                         L.ptr(h[3]), ties.data_ptr(), L.cur_stream()), "dpd_pose_point_fwd_train")
    bits = torch.stack([(ties[:, p // 64] >> (p % 64)) & 1 for p in range(N)], 1).double()          # [C, N, 1024]
    if N % 64:                                       # no bit beyond the cloud's last point
        assert int((ties[:, W - 1] >> (N % 64)).ne(0).sum()) == 0
    return bits / bits.sum(1, keepdim=True).clamp_min(1.0), bits, f


@pytest.mark.gpu
@pytest.mark.parametrize("C,N,dup", [(32, 512, False), (3, 65, False), (4, 200, True), (2, 2048, False), (6, 128, True)])
def test_pose_point_network_training_evaluation_above_64_points(C, N, dup):
    """dpd_pose_point_fwd_train / dpd_pose_point_bwd at N > 64 against torch autograd of the same layers in float64, pooled with the
    library's own selection: features (2e-5 relative) and all ten gradients (1e-3 of the tensor's largest entry) -- the bars of the
    64-point test.  The selection attains the float64 maximum to 1e-5, the selected weights of every column with a positive maximum sum
    to 1, and two runs give equal bits.  `dup` repeats the first half of every cloud as its second half: the two copies of a point lie
    in DIFFERENT 64-point words, so a column's ties span words."""
    dev = torch.device("cuda:0")
    net = _biased_net(dev, 3)
    src, tmpl, _ = synth.registration_pairs(max(1, C), N, seed=9)
    clouds = torch.tensor(np.concatenate([src, tmpl])[:C], device=dev)
    if dup:
        clouds[:, N // 2:] = clouds[:, :N - N // 2]
        assert N // 2 >= 64                                          # a point and its copy never share a word
    g = torch.Generator().manual_seed(5)
    up = torch.randn(C, 1024, generator=g).to(dev)
    params = [p for m in net.point if isinstance(m, torch.nn.Linear) for p in (m.weight, m.bias)]

    def run(native):
        net.native_train = native
        for p in params:
            p.grad = None
        f = net._pooled(clouds)
        assert (type(f.grad_fn).__name__ == "_PointFeaturesFnBackward") == native
        (f * up).sum().backward()
        return f.detach().clone(), [p.grad.clone() for p in params]

    try:
        f_nat, g_nat = run(True)
        f_nat2, g_nat2 = run(True)
        f_t, g_t = run(False)
    finally:
        net.native_train = True
    assert torch.equal(f_nat, f_nat2) and all(torch.equal(a, b) for a, b in zip(g_nat, g_nat2))
    assert (f_nat - f_t).abs().max().item() <= 2e-5 * max(1.0, f_t.abs().max().item())
    net64 = _net64(net, dev)
    p64 = [p for m in net64.point if isinstance(m, torch.nn.Linear) for p in (m.weight, m.bias)]
    z64 = net64.point(clouds.double())
    sel, bits, f_sel = _native_pool_selection(net, clouds)
    assert torch.equal(f_sel, f_nat)
    f64 = (z64 * sel).sum(1)
    err_sel = (f64 - z64.amax(1)).abs().max().item()
    wsum = sel.sum(1)                                               # [C, 1024]
    pos = f_nat > 0
    f_err = (f_nat.double() - f64).abs().max().item()
    print("C=%d N=%d dup=%s: |selection - max| = %.3e, feature error = %.3e (scale %.3e)" % (C, N, dup, err_sel, f_err, f64.abs().max().item()))
    assert err_sel <= 1e-5
    assert float((wsum[pos] - 1.0).abs().max()) <= 1e-12 and float(wsum[~pos].abs().sum()) == 0.0
    if dup:
        cnt = bits.sum(1)
        assert float((cnt[pos] >= 2).double().mean()) == 1.0      # every positive maximum is attained by a point AND its copy in another word
        assert float(pos.float().mean()) > 0.05
    (f64 * up.double()).sum().backward()
    assert f_err <= 2e-5 * max(1.0, f64.abs().max().item())
    worst = []
    for name, a, r in zip(["W1", "b1", "W2", "b2", "W3", "b3", "W4", "b4", "W5", "b5"], g_nat, (p.grad for p in p64)):
        scale = max(1e-6, r.abs().max().item())
        worst.append((name, (a.double() - r).abs().max().item() / scale))
    print("gradient errors / largest entry:", " ".join("%s=%.2e" % w for w in worst))
    for name, rel in worst:
        assert rel <= 1e-3, (name, rel)


@pytest.mark.gpu
@pytest.mark.parametrize("B,N", [(16, 512), (5, 100), (33, 256)])
def test_pose_network_training_evaluation_is_one_node_above_64_points(B, N):
    """_PoseNetRawFn (shared MLP + max pool + head on csrc/pose.hip) at N > 64 against the same network in torch, float64, with the SAME
    dropout mask: raw output [B,7] (2e-5 relative) and all 18 gradients (1e-3 of the tensor's largest entry)."""
    from dpdist_amd.registration import _PoseNetRawFn
    dev = torch.device("cuda:0")
    net = _biased_net(dev, 4)
    src, tmpl, _ = synth.registration_pairs(B, N, seed=3)
    clouds = torch.tensor(np.concatenate([src, tmpl]), device=dev)
    g = torch.Generator().manual_seed(7)
    mask = (torch.rand(B, 256, generator=g) < 0.7).float().div(0.7).to(dev)
    up = torch.randn(B, 7, generator=g).to(dev)
    lin = [m for m in net.point if isinstance(m, torch.nn.Linear)] + [m for m in net.head if isinstance(m, torch.nn.Linear)]
    params = [t for m in lin for t in (m.weight, m.bias)]
    pred = _PoseNetRawFn.apply(clouds[:B].contiguous(), clouds[B:].contiguous(), mask, None, *params)
    grads = torch.autograd.grad((pred * up).sum(), params)
    pred2 = _PoseNetRawFn.apply(clouds[:B].contiguous(), clouds[B:].contiguous(), mask, None, *params)
    grads2 = torch.autograd.grad((pred2 * up).sum(), params)
    assert torch.equal(pred, pred2) and all(torch.equal(a, b) for a, b in zip(grads, grads2))
    net64 = _net64(net, dev)
    lin64 = [m for m in net64.point if isinstance(m, torch.nn.Linear)] + [m for m in net64.head if isinstance(m, torch.nn.Linear)]
    p64 = [t for m in lin64 for t in (m.weight, m.bias)]
    sel, _, _ = _native_pool_selection(net, clouds)
    f = (net64.point(clouds.double()) * sel).sum(1)
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


@pytest.mark.gpu
@pytest.mark.parametrize("N", [100, 512])
def test_pose_network_module_takes_the_library_node_above_64_points(N):
    """Through the module: `net.raw` at N > 64 is the library's node; with `native_train = False` it is torch, and the two agree (2e-5)."""
    dev = torch.device("cuda:0")
    net = _biased_net(dev, 4)
    src, tmpl, _ = synth.registration_pairs(4, N, seed=3)
    src, tmpl = torch.tensor(src, device=dev), torch.tensor(tmpl, device=dev)
    net.train()
    assert type(net.raw(src, tmpl).grad_fn).__name__ == "_PoseNetRawFnBackward"
    net.eval()
    out_n = net.raw(src, tmpl)
    assert type(out_n.grad_fn).__name__ == "_PoseNetRawFnBackward"
    net.native_train = False
    try:
        out_t = net.raw(src, tmpl)
    finally:
        net.native_train = True
    assert type(out_t.grad_fn).__name__ != "_PoseNetRawFnBackward"
    assert (out_t - out_n).abs().max().item() <= 2e-5 * max(1.0, out_t.abs().max().item())


@pytest.fixture(scope="module")
def lib():
    from dpdist_amd import build, lib as L
    build.build(verbose=False)
    return L.load()


def test_tie_words_and_workspace_entries(lib):
    """Host-only entries: the tie-word count of an N, and the backward's workspace for (clouds, N) -- the old entry's size at N <= 64,
    growing with the number of 64-point chunks, 0 for what the entries refuse."""
    assert [lib.dpd_pose_point_tie_words(n) for n in (1, 64, 65, 2048)] == [1, 1, 2, 32]
    for clouds in (1, 32, 66):
        old = lib.dpd_pose_point_bwd_workspace_bytes(clouds)
        assert old > 0 and all(lib.dpd_pose_point_bwd_workspace_bytes_n(clouds, n) == old for n in (1, 50, 64))
        sizes = [lib.dpd_pose_point_bwd_workspace_bytes_n(clouds, n) for n in (64, 65, 128, 129, 512, 2048)]
        assert sizes[1] == sizes[2] and all(a < b for a, b in zip([sizes[0]] + sizes[2:], sizes[2:]))
        assert sizes[5] >= 32 * old                                  # one partial record per (cloud, chunk)
    assert lib.dpd_pose_point_bwd_workspace_bytes_n(4, 2049) == 0 and lib.dpd_pose_point_bwd_workspace_bytes_n(0, 64) == 0
    assert lib.dpd_pose_point_bwd_workspace_bytes_n(4, 0) == 0


@pytest.mark.gpu
def test_point_entries_take_65_points_and_refuse_2049(lib):
    from ctypes import byref
    from dpdist_amd import lib as L
    dev = torch.device("cuda:0")
    net = _biased_net(dev, 0)
    lin = [m for m in net.point if isinstance(m, torch.nn.Linear)]
    w = L.PoseNetW()
    for i, m in enumerate(lin):
        w.Wp[i], w.bp[i] = m.weight.data_ptr(), m.bias.data_ptr()
    w.out_features = 1024
    for N, want in ((65, 0), (2049, -3)):
        pts = torch.rand(1, N, 3, device=dev)
        f, h = torch.empty(1, 1024, device=dev), [torch.empty(N, k, device=dev) for k in (64, 64, 64, 128)]
        ties = torch.empty(1, (N + 63) // 64, 1024, device=dev, dtype=torch.int64)
        rc = lib.dpd_pose_point_fwd_train(byref(w), L.ptr(pts), None, 1, 0, N, L.ptr(f), L.ptr(h[0]), L.ptr(h[1]), L.ptr(h[2]), L.ptr(h[3]),
                                          ties.data_ptr(), L.cur_stream())
        torch.cuda.synchronize()
        assert rc == want, (N, rc)
        dW = [torch.empty_like(m.weight) for m in lin]
        db = [torch.empty_like(m.bias) for m in lin]
        import ctypes
        vp = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])      # noqa: E731
        nb = max(lib.dpd_pose_point_bwd_workspace_bytes_n(1, N), 16)
        ws = torch.empty(nb // 4, device=dev)
        rc = lib.dpd_pose_point_bwd(byref(w), L.ptr(pts), None, 1, 0, N, L.ptr(torch.ones(1, 1024, device=dev)), L.ptr(h[0]), L.ptr(h[1]),
                                    L.ptr(h[2]), L.ptr(h[3]), ties.data_ptr(), vp(dW), vp(db), L.ptr(ws), nb, L.cur_stream())
        torch.cuda.synchronize()
        assert rc == want, (N, rc)


@pytest.mark.gpu
def test_registration_step_at_the_reference_point_count_is_bitwise_graph_and_eager():
    """IterativeRegistration at the reference's default cloud size (B = 8, N = 512, 3 loops; four training steps: two eager, one capture,
    two replays): the captured step and the eager step leave bit for bit the same pose network, transforms and losses, with the pose
    network's training evaluation on the library.  The torch pose network (`native_train = False`) agrees on the first step's loss to 1e-5
    relative; those two legs run without dropout (keep_prob 1), because the torch head draws its own mask where the library's node takes
    the one drawn with the refinements' masks."""
    from dpdist_amd import lib as L
    from dpdist_amd.model import DPDistLoss, DPDistModel
    from dpdist_amd.registration import IterativeRegistration, _PoseNetRawFn
    dev = torch.device("cuda:0")
    B, N = 8, 512
    taken = []
    orig = _PoseNetRawFn.forward

    def run(graph, native_train=True, steps=4, keep_prob=0.7):
        torch.manual_seed(0)
        model = DPDistModel(device=dev)
        model.load_tf_state_dict(synth.make_weights("wide"))
        P = model.params_
        assert L.load().dpd_asloss_bytes(B, N, 8, 5, P.H, L.DTYPES[P.compute_dtype]) != 0      # the as-loss engine takes the shape
        net = PoseNet(keep_prob=keep_prob).to(dev)
        net.native_train = native_train
        torch.manual_seed(1000)
        rng = np.random.default_rng(0)
        reg = IterativeRegistration(net, DPDistLoss(model), lr=1e-4, max_loops=3, distributed=False, graph=graph)
        losses, Ts = [], []
        for _ in range(steps):
            src, tmpl, _ = synth.registration_pairs(B, N, rng=rng)
            loss, T = reg.train_step(torch.tensor(src, device=dev), torch.tensor(tmpl, device=dev))
            losses.append(loss.clone())
            Ts.append(T.clone())
        torch.cuda.synchronize()
        assert reg.graph_replays == (steps - 2 if graph else 0), reg.graph_replays
        w = torch.cat([p.detach().reshape(-1) for p in net.parameters()]).clone()
        reg.close()
        return w, torch.stack(Ts), torch.stack(losses)

    def counting(ctx, source, *rest):
        taken.append(tuple(source.shape))
        return orig(ctx, source, *rest)
    _PoseNetRawFn.forward = staticmethod(counting)
    try:
        g = run(True)
        n_graph = len(taken)
        e = run(False)
        n_eager = len(taken) - n_graph
        n1 = run(False, steps=1, keep_prob=1.0)
        n_first = len(taken) - n_graph - n_eager
        t = run(False, native_train=False, steps=1, keep_prob=1.0)
        n_torch = len(taken) - n_graph - n_eager - n_first
    finally:
        _PoseNetRawFn.forward = staticmethod(orig)
    assert all(s == (B, N, 3) for s in taken)
    # the library's node was taken: two eager steps + one capture | four eager steps | one | never by the torch leg
    assert (n_graph, n_eager, n_first, n_torch) == (3, 4, 1, 0), (n_graph, n_eager, n_first, n_torch)
    assert all(bool(torch.isfinite(x).all()) for x in g)
    assert all(torch.equal(a, b) for a, b in zip(g, e)), [(a - b).abs().max().item() for a, b in zip(g, e)]
    l_nat, l_t = n1[2][0].item(), t[2][0].item()
    print("first loss: library %.8f torch %.8f" % (l_nat, l_t))
    assert abs(l_nat - l_t) <= 1e-5 * abs(l_t)

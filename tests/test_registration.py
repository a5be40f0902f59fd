"""Row f2 (registration harness): the pose math, the pose network and the error metric against goldens produced by the
reference's own functions (tests/golden/pose_cases.npz, oracle/gen_goldens.py:fx_pose runs helper.transformation_quat_tensor,
ipcr_model.quat_normalize / get_model / get_pose, results_itrPCRNet_no_stop.find_errors, helper.transformation_quat2mat /
find_final_pose under the stubs), plus scipy cross-checks; GPU: gradients reach the pose network through DPDist."""
import os
import math

import numpy as np
import pytest
import torch
from scipy.spatial.transform import Rotation

from dpdist_amd import synth
from dpdist_amd.registration import (PoseNet, compose, find_errors, find_final_pose, pose_errors, quat_normalize, quat_to_mat,
                                     transformation_quat2mat, transformation_quat_tensor)


@pytest.fixture(scope="module")
def pose(golden_dir):
    return np.load(os.path.join(golden_dir, "pose_cases.npz"))


def test_transformation_quat_tensor_golden(pose):
    """helper.py:539-570 run by the generator; unit AND un-normalised quaternions (no normalisation inside)."""
    for dt, tag, tol in ((torch.float32, "f32", 2e-6), (torch.float64, "f64", 1e-12)):
        got = transformation_quat_tensor(torch.tensor(pose["data"], dtype=dt), torch.tensor(pose["quat"], dtype=dt),
                                         torch.tensor(pose["trans"], dtype=dt)).numpy()
        assert np.abs(got - pose["transformed_" + tag]).max() <= tol


@pytest.mark.parametrize("lim", [45, 10])
def test_quat_normalize_golden(pose, lim):
    """models/ipcr_model.py:285-294."""
    got = quat_normalize(torch.tensor(pose["raw7"], dtype=torch.float64), rot_lim=float(lim)).numpy()
    assert np.abs(got - pose["quat_normalize%d_f64" % lim]).max() <= 1e-12
    got32 = quat_normalize(torch.tensor(pose["raw7"]), rot_lim=float(lim)).numpy()
    assert np.abs(got32 - pose["quat_normalize%d_f32" % lim]).max() <= 1e-6


def test_pose_network_golden(pose):
    """ipcr_model.pointnet + get_pose (inference branch of the dropout) with the seeded weights of synth.pose_net_spec."""
    net = PoseNet(out_features=1024, lim_rot=0).double().eval()
    net.load_tf_state_dict(synth.make_named_weights(synth.pose_net_spec(1024), seed=int(pose["weights_seed"])))
    src, tmpl = torch.tensor(pose["source"], dtype=torch.float64), torch.tensor(pose["template"], dtype=torch.float64)
    with torch.no_grad():
        fs, ft = net.features(src, tmpl)
        raw = net(src, tmpl)
        net.lim_rot = 45.0
        lim = net(src, tmpl)
    assert np.abs(fs.numpy() - pose["feat_source_f64"]).max() <= 1e-10
    assert np.abs(ft.numpy() - pose["feat_template_f64"]).max() <= 1e-10
    assert np.abs(raw.numpy() - pose["pose_raw_f64"]).max() <= 1e-10
    assert np.abs(lim.numpy() - pose["pose_lim45_f64"]).max() <= 1e-10
    assert np.abs(raw.numpy() - pose["pose_raw_f32"]).max() <= 1e-4        # the float32 run of the same graph


def test_find_errors_golden(pose):
    """results_itrPCRNet_no_stop.py:112-133 (same signature) against its own output."""
    for i in range(len(pose["err_gt_pose"])):
        te, re = find_errors(pose["err_gt_pose"][i], pose["err_final_pose"][i])
        assert abs(te - pose["err_translation"][i]) <= 1e-12
        assert abs(re - pose["err_rotation_deg"][i]) <= 1e-8
    te, re = find_errors(pose["err_gt_pose"][0], pose["err_gt_pose"][0])
    assert te == 0.0 and re <= 1e-5


def test_quat2mat_and_final_pose_golden(pose):
    """helper.transformation_quat2mat (:309-329) and find_final_pose (:331-345)."""
    B = pose["quat"].shape[0]
    poses = np.concatenate([pose["trans"], pose["quat"]], 1).astype(np.float64)
    T, moved = transformation_quat2mat(poses.reshape(1, B, 7), np.tile(np.eye(4), (B, 1, 1)), pose["data"].astype(np.float64).copy())
    assert np.abs(T - pose["quat2mat_T"]).max() <= 1e-12
    assert np.abs(moved - pose["quat2mat_data"]).max() <= 1e-12
    assert np.abs(find_final_pose(T) - pose["final_pose"]).max() <= 1e-12


def test_quat_to_mat_matches_scipy():
    rng = np.random.default_rng(0)
    q = rng.standard_normal((16, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    R = quat_to_mat(torch.tensor(q)).numpy()
    ref = Rotation.from_quat(q[:, [1, 2, 3, 0]]).as_matrix()      # scipy is (x,y,z,w); the reference is (q0=w,q1,q2,q3)
    assert np.abs(R - ref).max() < 1e-12


def test_transformation_and_compose_are_consistent():
    rng = np.random.default_rng(1)
    data = torch.tensor(rng.standard_normal((4, 10, 3)))
    T = torch.eye(4, dtype=torch.float64).repeat(4, 1, 1)
    cur = data
    for _ in range(3):
        pose = quat_normalize(torch.tensor(rng.standard_normal((4, 7))))
        cur = transformation_quat_tensor(cur, pose[:, 3:7], pose[:, :3])
        T = compose(T, pose)
    via_T = data @ T[:, :3, :3].transpose(1, 2) + T[:, None, :3, 3]
    assert (cur - via_T).abs().max() < 1e-12


def test_quat_normalize_limits():
    p = quat_normalize(torch.randn(64, 7) * 10, rot_lim=45.0)
    assert (p[:, :3].abs() <= 0.1 + 1e-6).all()
    assert ((p[:, 3:7].norm(dim=-1) - 1).abs() < 1e-5).all()
    ang = 2 * torch.rad2deg(torch.acos(p[:, 3].clamp(-1, 1)))
    assert (ang <= 45.0 + 1e-3).all()


def test_pose_errors_on_matrices():
    find_errors = pose_errors
    ang = math.radians(30.0)
    Rg = torch.tensor(Rotation.from_rotvec([0, 0, ang]).as_matrix())[None]
    tg = torch.tensor([[0.05, -0.02, 0.01]], dtype=torch.float64)
    T_perfect = torch.eye(4, dtype=torch.float64)[None].clone()
    T_perfect[:, :3, :3] = Rg.transpose(1, 2)
    T_perfect[:, :3, 3] = -(Rg.transpose(1, 2) @ tg[:, :, None])[:, :, 0]
    te, re = find_errors(T_perfect, Rg, tg)
    assert te.item() < 1e-12 and re.item() < 1e-5
    te, re = find_errors(torch.eye(4, dtype=torch.float64)[None], Rg, tg)
    assert abs(re.item() - 30.0) < 1e-6


def _gpu_harness(dev, max_loops=8, keep_prob=0.7, weights="wide"):
    from dpdist_amd.model import DPDistLoss, DPDistModel
    from dpdist_amd.registration import IterativeRegistration
    model = DPDistModel(device=dev)
    model.load_tf_state_dict(synth.make_weights(weights))
    return model, IterativeRegistration(PoseNet(keep_prob=keep_prob).to(dev), DPDistLoss(model), lr=1e-4, max_loops=max_loops)


@pytest.mark.gpu
def test_dpdist_loss_trains_the_pose_network():
    """Gradients flow source -> transformed source -> (HIP) DPDist backward-to-input -> pose network; the update is the
    library's TF-form Adam (one flat buffer), DPDist stays frozen."""
    from dpdist_amd.optim import TFAdam
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model, reg = _gpu_harness(dev, max_loops=3)
    assert isinstance(reg.opt, TFAdam)
    src, tmpl, _ = synth.registration_pairs(8, 64, seed=100)
    src, tmpl = torch.tensor(src, device=dev), torch.tensor(tmpl, device=dev)
    before = [p.detach().clone() for p in reg.net.parameters()]
    loss, T = reg.train_step(src, tmpl)
    assert torch.isfinite(loss) and T.shape == (8, 4, 4)
    changed = sum(float((p.detach() - b).abs().max()) > 0 for p, b in zip(reg.net.parameters(), before))
    assert changed >= len(before) - 1          # every layer received a gradient
    assert all(not p.requires_grad for p in model.parameters())      # DPDist stays frozen
    # all parameters still live in the optimizer's flat buffer
    lo, hi = reg.opt.flat.data_ptr(), reg.opt.flat.data_ptr() + reg.opt.flat.numel() * 4
    assert all(lo <= p.data_ptr() < hi for p in reg.net.parameters())


@pytest.mark.gpu
def test_registration_step_gradients_vs_oracle():
    """ONE training step of config 5's workload (B=16, 64 points, 8 loops: run_train_and_eval_PCRNet.bash:17-32,
    iterative_PCRNet_ours.py:410-470) -- the pose-network gradients that come back through the HIP as-loss path
    (d loss_pred / d input1) against the oracle: float64 autograd through the pose network -> quaternion normalisation
    (:213-221) -> transformation_quat_tensor -> oracle get_model -> loss_pred (:248-251).  Dropout is switched off so that
    both sides see the same network; the seven no-gradient refinements run on the GPU and their result feeds both."""
    from oracle import restate as R
    from dpdist_amd.registration import predicted_pose_applied
    dev = torch.device("cuda:0")
    torch.manual_seed(3)
    model, reg = _gpu_harness(dev, max_loops=8, keep_prob=1.0)
    with torch.no_grad():                      # a pose head that actually moves the cloud (Xavier init predicts ~identity)
        reg.net.head[-1].bias.copy_(torch.tensor([0.3, -0.2, 0.1, 0.25, 0.4, -0.3, 0.8], device=dev))
    src, tmpl, _ = synth.registration_pairs(16, 64, seed=5)
    src, tmpl = torch.tensor(src, device=dev), torch.tensor(tmpl, device=dev)
    reg.net.train()
    refined, T = reg.refine(src, tmpl, reg.max_loops - 1)
    assert (refined - src).abs().max() > 1e-2                         # the refinements did move the source
    loss, pose = reg.loss_and_gradients(refined, tmpl)
    got = {n: p.grad.detach().double().cpu() for n, p in reg.net.named_parameters()}

    def oracle(dtype):
        net = PoseNet(keep_prob=1.0).to(dtype)
        net.load_state_dict({k: v.detach().cpu().to(dtype) for k, v in reg.net.state_dict().items()})
        net.train()
        W = R.as_torch_weights(synth.make_weights("wide"), dtype)
        s, t = refined.detach().cpu().to(dtype), tmpl.cpu().to(dtype)
        moved = predicted_pose_applied(s, net(s, t))
        ps, _ = R.get_model(moved, t, W)
        _, lp = R.get_loss(ps, torch.ones(16, 64, dtype=dtype))      # labels12 is fed with ones and unused (:422)
        lp.backward()
        return lp.item(), {n: p.grad.double() for n, p in net.named_parameters()}

    l64, ref = oracle(torch.float64)
    l32, ref32 = oracle(torch.float32)
    assert abs(loss.item() - l64) <= 2e-5
    gmax = max(float(g.abs().max()) for g in ref.values())
    assert gmax > 1e-4                                                # a real gradient, not a saturated zero
    report, bad = [], []
    num = den = 0.0
    for n, g in ref.items():
        # Same bar as the input-gradient goldens (tests/test_gpu_parity.py::test_losses_and_input_gradients_golden): the loss is
        # piecewise smooth (ReLU gates, relu6 clip, max/min statistics, sqrt|x| power normalisation), so float32 evaluations
        # in a different summation order differ by more than round-off on a few entries.  Per layer: max error <= 4x the gap of
        # the oracle's own float32 run, or 2 % of the layer's largest gradient entry; whole gradient: 1 % in the L2 norm.
        bar = max(4.0 * float((ref32[n] - g).abs().max()), 2e-2 * float(g.abs().max()), 1e-7)
        err = float((got[n] - g).abs().max())
        num += float((got[n] - g).square().sum())
        den += float(g.square().sum())
        report.append((n, err, float(g.abs().max())))
        if err > bar:
            bad.append((n, err, bar))
    rel = math.sqrt(num / den)
    print("registration step gradients vs oracle: relative L2 error %.2e; per layer (name, max err, max |g|): %s" % (rel, report))
    assert not bad, bad
    assert rel <= 1e-2, rel


@pytest.mark.gpu
def test_tf_adam_optimizer_matches_the_oracle_update():
    """optim.TFAdam (what the f2 / f4 consumers now use instead of torch.optim.Adam) == tf.train.AdamOptimizer's update as the
    oracle restates it (epsilon OUTSIDE the bias correction), over several steps and parameters of ragged sizes."""
    from oracle import restate as R
    from dpdist_amd.optim import TFAdam
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    shapes = [(7, 5), (5,), (3, 11), (1,)]
    ps = [torch.nn.Parameter(torch.tensor(rng.standard_normal(s).astype(np.float32), device=dev)) for s in shapes]
    ref = [p.detach().cpu().numpy().astype(np.float64) for p in ps]
    ms, vs = [np.zeros_like(r) for r in ref], [np.zeros_like(r) for r in ref]
    opt = TFAdam(ps, lr=1e-2)
    for t in range(1, 6):
        opt.zero_grad()
        gs = [rng.standard_normal(s).astype(np.float32) * (1e-4 if t == 3 else 1.0) for s in shapes]   # tiny |g|: epsilon matters
        loss = sum((p * torch.tensor(g, device=dev)).sum() for p, g in zip(ps, gs))
        loss.backward()
        opt.step()
        for i, g in enumerate(gs):
            R.adam_tf_step(ref[i], g.astype(np.float64), ms[i], vs[i], t, 1e-2)        # in place
        for p, r in zip(ps, ref):
            assert np.abs(p.detach().cpu().numpy() - r).max() <= 2e-6
    with pytest.raises(RuntimeError):
        TFAdam([torch.nn.Parameter(torch.zeros(3))])                 # CPU parameters: no fallback


# ---------------------------------------------------------------------------------------------------------------- synthetic chairs
def test_chair_surface_samples_and_exact_distance():
    """synth.make_chair / BoxUnion (the rotation-observable stand-in for ModelNet40 'chair'): inside the radius-0.8 ball
    (dataset_sample_with_gt.py:82), samples lie ON the union's surface and outside every other box, and dist() is the exact
    point-to-surface distance for outside points (against 60 k brute-force surface samples)."""
    rng = np.random.default_rng(0)
    for _ in range(3):
        ch = synth.make_chair(rng)
        assert len(ch.c) in (6, 10)                                    # seat + back + 4 legs (+ 2 x 2 arm-rest boxes)
        S = ch.sample(rng, 60000)
        assert np.linalg.norm(S, axis=1).max() <= 0.8 + 1e-9
        sd = ch.sdf_each(S)
        assert np.abs(sd).min(axis=1).max() <= 1e-9                    # on the surface of (at least) one box
        assert (sd > -1e-9).all()                                      # and not buried in another one
        q = rng.uniform(-0.85, 0.85, (300, 3))
        q = q[ch.outside(q)]
        brute = np.sqrt(((q[:, None] - S[None]) ** 2).sum(-1)).min(1)
        assert np.abs(ch.dist(q) - brute).max() <= 1.2e-2             # sampling density of the brute force (dist <= brute always)
        assert (ch.dist(q) <= brute + 1e-9).all()


def test_chair_batches_follow_the_trainers_recipe():
    """s2_modelnet_shaped(shapes='chair') = the recipe of train_multi_gpu_pc_compare_dist.py:747-766 on chairs: 32 surface labels of 0,
    16 near (0.001 .. 0.1) and 16 far (> 0.1) exact distances; the default analytic stream is untouched by the new option."""
    pcA, pcB, lab = synth.s2_modelnet_shaped(6, 64, 7, shapes="chair")
    assert pcA.shape == (6, 64, 3) and pcB.shape == (6, 64, 3) and lab.shape == (6, 64)
    assert (lab[:, :32] == 0).all() and (lab[:, 32:48] > 0.001).all() and (lab[:, 32:48] < 0.1).all() and (lab[:, 48:] > 0.1).all()
    assert np.abs(pcA).max() <= 0.8 + 0.1 + 1e-6                      # radius 0.8 + the +-0.1 shift
    a = synth.s2_modelnet_shaped(3, 64, 100)
    b = synth.s2_modelnet_shaped(3, 64, 100, shapes="analytic")
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    t = synth.s2_modelnet_shaped(2, 64, 7, shapes="chair", tilt_deg=20.0)
    assert np.isfinite(t[0]).all() and not np.array_equal(t[0], synth.s2_modelnet_shaped(2, 64, 7, shapes="chair")[0])


def test_registration_pairs_follow_the_reference_recipe():
    """helper.split_template_source + generate_poses_ours.py: different samples of one surface, source = R_x R_y R_z p + t with
    Euler angles in +-45 deg and |t| <= 0.01; the metric of results_itrPCRNet_no_stop.py reads 0 for the true transform and the
    rotation angle of the pose for the identity."""
    from dpdist_amd.registration import find_final_pose_inv
    src, tmpl, gt = synth.registration_pairs(8, 64, seed=3)
    assert src.shape == tmpl.shape == (8, 64, 3) and gt.shape == (8, 6)
    assert np.abs(gt[:, :3]).max() <= 0.01 and np.abs(gt[:, 3:]).max() <= np.pi / 4 + 1e-12
    assert not np.allclose(src, tmpl)
    for b in range(8):
        R = synth.euler_rotation(*gt[b, 3:])
        back = (src[b].astype(np.float64) - gt[b, :3]) @ R                    # R^T (s - t): the source's samples in the template frame
        assert np.abs(np.linalg.norm(back, axis=1)).max() <= 0.8 + 1e-5       # a rotation about the origin: still inside the ball
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = R.T, -R.T @ gt[b, :3]                            # the transform a perfect registration would compose
        te, re = find_errors(gt[b], find_final_pose_inv(T[None])[0])
        assert te <= 1e-12 and re <= 1e-5
        te0, re0 = find_errors(gt[b], np.zeros(6))
        ang = np.degrees(np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1)))
        assert abs(re0 - ang) <= 1e-6


def test_gpu_only_helpers_refuse_the_cpu():
    """optim.TFAdam / hipevents are bindings to the GPU library and the HIP runtime: no CPU form, loud failure."""
    from dpdist_amd.optim import TFAdam
    with pytest.raises(RuntimeError):
        TFAdam([torch.nn.Parameter(torch.zeros(3))])
    if not torch.cuda.is_available():
        from dpdist_amd import hipevents
        with pytest.raises(RuntimeError):
            hipevents.LightEvent()


# ---- BASELINE config 5's data-parallel leg: the pose network's gradient is the one thing that travels -------------------------
def _torch_chamfer(a, b):
    d = torch.cdist(a, b)
    return d.min(2)[0].mean() + d.min(1)[0].mean()


def _reg_dp_worker(rank, world, port, out):
    import torch.distributed as dist
    from dpdist_amd.ddp import shard_range
    from dpdist_amd.registration import IterativeRegistration
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(2)
    GB = 8
    src, tmpl, _ = synth.registration_pairs(GB, 64, seed=5)
    src, tmpl = torch.tensor(src), torch.tensor(tmpl)
    lo, hi = shard_range(GB, rank, world)

    def harness(distributed):
        torch.manual_seed(0)                                   # replicated variables: the same pose network on every rank
        net = PoseNet(keep_prob=1.0)                           # (no dropout: the full-batch comparison needs the same function)
        return IterativeRegistration(net, _torch_chamfer, optimizer=torch.optim.SGD(net.parameters(), lr=1e-2), max_loops=3,
                                     distributed=distributed)

    reg = harness(True)
    assert reg.reducer is not None and reg.reducer.active and reg.reducer.mode == "allreduce" and reg.reducer.crosscheck["ok"]
    refined, _ = reg.refine(src[lo:hi], tmpl[lo:hi], 2)
    reg.loss_and_gradients(refined, tmpl[lo:hi])               # all-reduced and scaled by 1 / world
    g_dp = reg._flat_grad.clone()
    for _ in range(2):                                         # two optimizer steps: replicas must stay bit-identical
        loss, T = reg.train_step(src[lo:hi], tmpl[lo:hi])
    w = torch.cat([p.detach().reshape(-1) for p in reg.net.parameters()])
    ws = [torch.empty_like(w) for _ in range(world)]
    dist.all_gather(ws, w)
    if rank == 0:
        full = harness(False)
        assert full.reducer is None
        refined, _ = full.refine(src, tmpl, 2)
        full.loss_and_gradients(refined, tmpl)
        g_full = torch.cat([p.grad.reshape(-1) for p in full.net.parameters()])
        out.put({"err": float((g_dp[:g_full.numel()] - g_full).abs().max()), "scale": float(g_full.abs().max()),
                 "same": bool(all(torch.equal(ws[0], x) for x in ws[1:])), "moved": float((w - torch.cat([p.detach().reshape(-1) for p in harness(False).net.parameters()])).abs().max()),
                 "wire": reg.reducer.wire_bytes_per_step, "n": int(g_full.numel())})
    dist.barrier()
    dist.destroy_process_group()


def test_registration_data_parallel_step_on_gloo():
    """BASELINE config 5's data-parallel leg (registration.IterativeRegistration(distributed=True); world size 2 over gloo, a torch
    Chamfer distance standing in for the GPU-only DPDist loss, SGD for the GPU-only TFAdam): the mean over the ranks of the pose
    network's shard gradients equals the full-batch gradient, two optimizer steps leave the replicas bit-identical, and the only
    bytes on the wire are the pose network's flat gradient (DPDist is frozen: no DPDist collective)."""
    import socket
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_reg_dp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = q.get(timeout=300)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert res["err"] <= 1e-6 * max(1.0, res["scale"]), res
    assert res["same"] and res["moved"] > 0
    assert res["wire"] == 4 * ((res["n"] + 3) // 4 * 4)          # 2 (P-1)/P x 4 B x parameters at P = 2


def test_centroid_residual_separates_lever_arm_from_misregistration():
    """registration.centroid_residual: a pure rotation error about the origin moves an off-centre cloud although the translation
    vector is exact; the ideal transform leaves no residual."""
    from dpdist_amd.registration import centroid_residual, euler_to_mat
    rng = np.random.default_rng(0)
    src = rng.normal(size=(4, 64, 3)) * 0.05 + np.array([0.3, 0.0, 0.0])
    gt = np.concatenate([rng.uniform(-0.01, 0.01, (4, 3)), np.radians(rng.uniform(-45, 45, (4, 3)))], 1)
    ideal = np.tile(np.eye(4), (4, 1, 1))
    for i in range(4):
        R = euler_to_mat(*gt[i, 3:])
        ideal[i, :3, :3] = R.T
        ideal[i, :3, 3] = -R.T @ gt[i, :3]
    assert centroid_residual(ideal, gt, src).max() < 1e-12
    off = ideal.copy()
    d = np.radians(2.0)
    Rz = np.array([[math.cos(d), -math.sin(d), 0], [math.sin(d), math.cos(d), 0], [0, 0, 1]])
    for i in range(4):
        off[i, :3, :3] = Rz @ ideal[i, :3, :3]                 # 2 degrees of rotation error, translation vector untouched
    r = centroid_residual(off, gt, src)
    assert 0.005 < r.min() and r.max() < 0.02                  # ~ 0.035 rad x 0.3 lever arm


@pytest.mark.gpu
@pytest.mark.parametrize("backend", ["rccl", "torch"])
def test_registration_step_on_a_single_rank_group_is_the_plain_step(backend, monkeypatch):
    """The data-parallel registration step through RCCL on one GPU (single-rank group, DPD_FORCE_DIST=1: the all-reduce is a copy, the
    scale 1): config 5's B = 16 / 8-loop step gives bit for bit the pose-network gradients and the update of the plain step (whose
    gradients test_registration_step_gradients_vs_oracle pins to the oracle); the reducer passed its start-up cross-check."""
    import torch.distributed as dist
    monkeypatch.setenv("DPD_DP_BACKEND", backend)
    monkeypatch.setenv("DPD_FORCE_DIST", "1")
    dev = torch.device("cuda:0")
    own = not dist.is_initialized()
    if own:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29661")
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        src, tmpl, _ = synth.registration_pairs(16, 64, seed=5)
        src, tmpl = torch.tensor(src, device=dev), torch.tensor(tmpl, device=dev)
        res = {}
        for mode in ("plain", "dp"):
            from dpdist_amd.model import DPDistLoss, DPDistModel
            from dpdist_amd.registration import IterativeRegistration
            torch.manual_seed(3)
            model = DPDistModel(device=dev)
            model.load_tf_state_dict(synth.make_weights("wide"))
            reg = IterativeRegistration(PoseNet(keep_prob=1.0).to(dev), DPDistLoss(model), lr=1e-4, max_loops=8, distributed=(mode == "dp"))
            if mode == "dp":
                assert reg.reducer.active and reg.reducer.backend == backend and reg.reducer.crosscheck["ok"] and reg.reducer.nranks == 1
            else:
                assert reg.reducer is None
            refined, _ = reg.refine(src, tmpl, 7)
            reg.loss_and_gradients(refined, tmpl)
            g = reg.opt.grad.clone()
            for _ in range(5):                     # two eager steps, then the captured form (with a reducer: two graphs around the collective)
                loss, T = reg.train_step(src, tmpl)
            torch.cuda.synchronize()
            assert reg.graph_replays == 3 and (next(iter(reg._graphs.values())).g2 is not None) == (mode == "dp")
            res[mode] = (g, reg.opt.flat.clone(), loss.clone(), T.clone())
            reg.close()
        for a, b in zip(res["plain"], res["dp"]):
            assert torch.equal(a, b)
        assert float(res["plain"][0].abs().max()) > 0
    finally:
        if own:
            dist.destroy_process_group()


@pytest.mark.gpu
def test_registration_training_is_bitwise_with_and_without_the_as_loss_engine(monkeypatch):
    """Twelve training steps of the iterative registration at the reference's workload (batch 16, 8 loops, dropout on: 7 forward-only
    pose refinements, then ONE DPDist forward + backward per step, iterative_PCRNet_ours.py:414-470) --
      * with DPDist evaluated through the as-loss engine (dpd_asloss_forward / _backward) and through the entry-by-entry autograd node,
      * with the whole step replayed as a hipGraph (two eager steps, one capture, ten replays) and launched eagerly:
    the pose network ends up bit for bit the same in all four combinations, and the same again on a second run.  The captured step runs
    the same kernels on the same inputs, dropout included (torch's graph-safe Philox offsets), Adam's lr_t comes from device memory."""
    import hashlib
    from dpdist_amd.model import DPDistLoss, DPDistModel
    from dpdist_amd.registration import IterativeRegistration
    dev = torch.device("cuda:0")

    def run(engine, graph, fused="1", native="1", concat=True):
        monkeypatch.setattr("dpdist_amd.asloss.ENGINE", engine == "1")
        torch.manual_seed(0)
        model = DPDistModel(device=dev)
        model.load_tf_state_dict(synth.make_weights("wide"))
        net = PoseNet().to(dev)
        torch.manual_seed(1000)
        rng = np.random.default_rng(0)
        reg = IterativeRegistration(net, DPDistLoss(model), lr=1e-4, max_loops=8, distributed=False, graph=(graph == "1"),
                                    fused_pose=(fused == "1"), native_refine=(native == "1"), concat_grads=concat)
        losses = []
        for _ in range(12):
            src, tmpl, _ = synth.registration_pairs(16, 64, rng=rng)
            loss, T = reg.train_step(torch.tensor(src, device=dev), torch.tensor(tmpl, device=dev))
            losses.append(loss)
        es, et, _ = synth.registration_pairs(16, 64, seed=77)
        for _ in range(4):                                   # evaluation: eager twice, then its own graph
            el, eT = reg.evaluate(torch.tensor(es, device=dev), torch.tensor(et, device=dev))
        torch.cuda.synchronize()
        w = torch.cat([p.detach().reshape(-1) for p in net.parameters()])
        used = bool(getattr(model.params_, "_asloss_engines", None))
        assert reg.graph_replays == (12 if graph == "1" else 0), reg.graph_replays
        assert reg.opt.t == 12
        reg.close()
        h = hashlib.sha1()
        for x in (w, T, eT):
            h.update(x.cpu().numpy().tobytes())
        return h.hexdigest(), tuple(l.item() for l in losses) + (el.item(),), used

    a, b, c, d, e = run("1", "1"), run("1", "1"), run("1", "0"), run("0", "0"), run("0", "1")
    # gradients accumulated into 18 views of a zeroed flat buffer (autograd's default) instead of written by one concatenation: 0 + g == g
    acc = run("1", "1", concat=False)
    assert acc[:2] == a[:2], (acc, a)
    assert a[2] and c[2] and not d[2] and not e[2]      # the engine really ran where it should and not where it should not
    assert a[:2] == b[:2] == c[:2] == d[:2] == e[:2], (a, b, c, d, e)
    # the torch pose algebra (~115 launches per loop) instead of csrc/pose.hip (1): the same step up to fp32 rounding of the pose chain
    # (first loss: 6e-8 apart on the box of round 6) -- after that the two trainings drift like any two fp32 summation orders do through
    # ReLU gates and relu6 clips (3e-2 in the loss after 12 steps on the 'wide' weights), so only the first step is pinned here; the
    # kernels themselves are pinned to the torch algebra by test_fused_pose_kernels_match_the_torch_algebra
    g, h = run("1", "1", native="0"), run("1", "0", native="0")      # torch pose network + csrc/pose.hip algebra: graph == eager again
    assert g[:2] == h[:2], (g, h)
    f = run("1", "0", fused="0")
    assert abs(f[1][0] - g[1][0]) <= 1e-5 and max(abs(x - y) for x, y in zip(f[1], g[1])) <= 0.1, (f[1], g[1])


@pytest.mark.gpu
@pytest.mark.parametrize("B,N,loops", [(16, 64, 3), (5, 50, 2), (3, 150, 2), (33, 64, 1)])
def test_native_pose_refinement_matches_the_torch_network(B, N, loops):
    """dpd_pose_refine (pose network + quat_normalize + cloud move + T composition on the library, four launches per loop + one per call) against the torch
    PoseNet driven through the torch algebra: raw network outputs of every loop, the moved source and the accumulated transform; ragged
    batches (more than 16 rows: two row groups in the head) and point counts (more than one 64-point pass of the shared MLP); with an
    explicit dropout mask against the same mask applied in torch."""
    from dpdist_amd.registration import pose_refine_native
    dev = torch.device("cuda:0")
    torch.manual_seed(11)
    net = PoseNet().to(dev)
    with torch.no_grad():                      # a head that actually moves the cloud, biases that are not all zero
        for m in net.modules():
            if isinstance(m, torch.nn.Linear):
                m.bias.normal_(0.0, 0.05)
        net.head[-1].bias.copy_(torch.tensor([0.3, -0.2, 0.1, 0.25, 0.4, -0.3, 0.8], device=dev))
    src, tmpl, _ = synth.registration_pairs(B, N, seed=5)
    src, tmpl = torch.tensor(src, device=dev), torch.tensor(tmpl, device=dev)
    g = torch.Generator(device="cpu").manual_seed(1)
    for mask in (None, (torch.rand(loops, B, 256, generator=g) < 0.7).float().div(0.7).to(dev)):
        moved, T, pred = pose_refine_native(net, src, tmpl, loops, mask, want_pred=True)
        # torch, loop by loop, in float64 (the reference arithmetic both fp32 forms approximate)
        net64 = PoseNet().double().to(dev)
        net64.load_state_dict({k: v.double() for k, v in net.state_dict().items()})
        s, t = src.double(), tmpl.double()
        Tr = torch.eye(4, device=dev, dtype=torch.float64).repeat(B, 1, 1)
        with torch.no_grad():
            for it in range(loops):
                f = net64.point(torch.cat([s, t], 0)).amax(1)
                h = net64.head[:6](torch.cat([f[:B], f[B:]], 1))
                if mask is not None:
                    h = h * mask[it].double()
                raw = net64.head[7](h)
                assert (pred[it].double() - raw).abs().max().item() <= 2e-5 * max(1.0, raw.abs().max().item()), (it, "raw output")
                pose = quat_normalize(raw, net.lim_rot)
                pose = torch.cat([pose[:, :3], pose[:, 3:7] / pose[:, 3:7].norm(dim=1, keepdim=True).clamp_min(1e-12)], 1)
                s = transformation_quat_tensor(s, pose[:, 3:7], pose[:, :3])
                Tr = compose(Tr, pose)
        assert (s - src.double()).abs().max().item() > 1e-2          # the loops did move the cloud
        assert (moved.double() - s).abs().max().item() <= 5e-5 and (T.double() - Tr).abs().max().item() <= 5e-5


@pytest.mark.gpu
@pytest.mark.parametrize("lim", [45.0, 10.0, 0.0])
def test_fused_pose_kernels_match_the_torch_algebra(lim):
    """csrc/pose.hip (one launch for quat_normalize -> normalisation -> Besl-McKay R -> moved cloud -> T composition, one for its
    backward) against the torch functions above, which tests at the top of this file pin to the reference's goldens: forward in both
    modes (refinement / training evaluation) to fp32 round-off, backward against float64 autograd of the torch chain."""
    from dpdist_amd.registration import compose, pose_apply, predicted_pose_applied
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(5)
    B, N = 16, 64
    pred = torch.randn(B, 7, generator=g) * torch.tensor([2.0, 2.0, 2.0, 1.5, 1.0, 1.0, 1.0])
    if lim == 0.0:
        pred[:, 3:] = torch.nn.functional.normalize(pred[:, 3:], dim=1) * (1 + 0.3 * torch.rand(B, 1, generator=g))
    src = torch.rand(B, N, 3, generator=g) * 2 - 1
    T = torch.eye(4).repeat(B, 1, 1) + 0.1 * torch.randn(B, 4, 4, generator=g)
    T[:, 3] = torch.tensor([0.0, 0.0, 0.0, 1.0])
    qn = (lambda p: quat_normalize(p, lim)) if lim else (lambda p: p)

    def ref(dtype, mode):
        p = pred.to(dtype).requires_grad_(True)
        pose = qn(p)
        pc = torch.cat([pose[:, :3], pose[:, 3:7] / pose[:, 3:7].norm(dim=1, keepdim=True).clamp_min(1e-12)], 1)
        if mode == 0:
            moved = transformation_quat_tensor(src.to(dtype), pc[:, 3:7], pc[:, :3])
        else:
            moved = predicted_pose_applied(src.to(dtype), pose)
        return p, pose, moved, compose(T.to(dtype), pc)

    for mode in (0, 1):
        _, pose, moved, Tn = ref(torch.float64, mode)
        got = pose_apply(pred.to(dev), src.to(dev), T.to(dev), lim, mode)
        for name, x, y in zip(("pose", "moved", "T"), got, (pose, moved, Tn)):
            assert (x.double().cpu() - y.detach()).abs().max().item() <= 2e-6, (mode, name)
        got2 = pose_apply(pred.to(dev), src.to(dev), None, lim, mode)       # without a transform to compose
        assert len(got2) == 2 and torch.equal(got2[0], got[0]) and torch.equal(got2[1], got[1])
    # backward of the training evaluation
    w = torch.randn(B, N, 3, generator=g)
    p64, _, moved, _ = ref(torch.float64, 1)
    (moved * w.double()).sum().backward()
    pg = pred.to(dev).requires_grad_(True)
    out = pose_apply(pg, src.to(dev), None, lim, 1)
    (out[1] * w.to(dev)).sum().backward()
    err = (pg.grad.double().cpu() - p64.grad).abs().max().item()
    assert err <= 2e-5 * max(1.0, p64.grad.abs().max().item()), err
    assert float(p64.grad.abs().min()) > 0 or lim == 0.0
    with pytest.raises(RuntimeError, match="forward-only"):
        pg2 = pred.to(dev).requires_grad_(True)
        pose_apply(pg2, src.to(dev), None, lim, 0)[1].sum().backward()


def _native_pool_selection(net, clouds):
    """The max pool's selection as the LIBRARY's forward made it: sel [C,N,1024] float64 with 1 / (number of tied points) at the points that
    attain a column's positive maximum (dpd_pose_point_fwd_train's tie masks).  A float64 reference must pool with THIS selection: where two
    points of a cloud are equal to fp32 rounding, the library's fp32-MFMA forward and torch's GEMM may each call a different one the
    maximum (seen: 1 column of 18765) -- both are right for their own values, and the gradient of max is discontinuous there."""
    from ctypes import byref
    from dpdist_amd import lib as L
    C, N, _ = clouds.shape
    lin = [m for m in net.point if isinstance(m, torch.nn.Linear)]
    w = L.PoseNetW()
    for i, m in enumerate(lin):
        w.Wp[i], w.bp[i] = m.weight.data_ptr(), m.bias.data_ptr()
    w.out_features = 1024
    dev = clouds.device
    e = lambda *sh: torch.empty(*sh, device=dev)      # noqa: E731
    f, h = e(C, 1024), [e(C * N, k) for k in (64, 64, 64, 128)]
    ties = torch.empty(C, 1024, device=dev, dtype=torch.int64)
    L.check(L.load().dpd_pose_point_fwd_train(byref(w), L.ptr(clouds.contiguous()), None, C, 0, N, L.ptr(f), L.ptr(h[0]), L.ptr(h[1]), L.ptr(h[2]),
                                              L.ptr(h[3]), ties.data_ptr(), L.cur_stream()), "dpd_pose_point_fwd_train")
    bits = torch.stack([(ties >> b) & 1 for b in range(N)], 1).double()          # [C, N, 1024]
    return bits / bits.sum(1, keepdim=True).clamp_min(1.0), f


@pytest.mark.gpu
@pytest.mark.parametrize("C,N,dup", [(32, 64, False), (5, 50, False), (6, 64, True), (1, 8, False)])
def test_pose_point_network_training_evaluation_on_the_library(C, N, dup):
    """dpd_pose_point_fwd_train / dpd_pose_point_bwd (the pose network's shared MLP + max pool with its weight gradients: one launch forward,
    three backward) against torch autograd of the same layers in float64: features and all ten gradients; `dup` duplicates points inside
    the clouds, so that several points attain a column's maximum and the max pool's gradient must be SHARED among them (tf.reduce_max /
    torch.amax); and two calls give the same bits (every sum has a fixed order)."""
    dev = torch.device("cuda:0")
    torch.manual_seed(3)
    net = PoseNet().to(dev)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.Linear):
                m.bias.normal_(0.0, 0.05)
    src, tmpl, _ = synth.registration_pairs(max(1, C), N, seed=9)
    clouds = torch.tensor(np.concatenate([src, tmpl])[:C], device=dev)
    if dup:
        clouds[:, N // 2:] = clouds[:, :N - N // 2]              # every point twice: every positive maximum is attained (at least) twice
    g = torch.Generator().manual_seed(5)
    up = torch.randn(C, 1024, generator=g).to(dev)
    params = [p for m in net.point if isinstance(m, torch.nn.Linear) for p in (m.weight, m.bias)]

    def run(native):
        net.native_train = native
        for p in params:
            p.grad = None
        f = net._pooled(clouds)
        (f * up).sum().backward()
        return f.detach().clone(), [p.grad.clone() for p in params]

    f_nat, g_nat = run(True)
    f_nat2, g_nat2 = run(True)
    assert torch.equal(f_nat, f_nat2) and all(torch.equal(a, b) for a, b in zip(g_nat, g_nat2))
    f_t, g_t = run(False)
    assert (f_nat - f_t).abs().max().item() <= 2e-5 * max(1.0, f_t.abs().max().item())
    # float64 reference
    net64 = PoseNet().double().to(dev)
    net64.load_state_dict({k: v.double() for k, v in net.state_dict().items()})
    p64 = [p for m in net64.point if isinstance(m, torch.nn.Linear) for p in (m.weight, m.bias)]
    z64 = net64.point(clouds.double())
    sel, _ = _native_pool_selection(net, clouds)
    f64 = (z64 * sel).sum(1)                                     # the max pool with the library's selection (see the helper)
    assert (f64 - z64.amax(1)).abs().max().item() <= 1e-5        # ... which IS the maximum up to fp32 rounding
    (f64 * up.double()).sum().backward()
    assert (f_nat.double() - f64).abs().max().item() <= 2e-5 * max(1.0, f64.abs().max().item())
    for name, a, r in zip(["W1", "b1", "W2", "b2", "W3", "b3", "W4", "b4", "W5", "b5"], g_nat, (p.grad for p in p64)):
        scale = max(1e-6, r.abs().max().item())
        # (a ReLU gate that is +-1e-8 in float64 and exactly 0 in fp32 can still move single entries: 1e-3 of the tensor's largest entry)
        assert (a.double() - r).abs().max().item() <= 1e-3 * scale, (name, (a.double() - r).abs().max().item(), scale)
    if dup:
        assert float((f_nat > 0).float().mean()) > 0.05          # positive maxima exist, i.e. ties really carried gradient
    net.native_train = True


@pytest.mark.gpu
@pytest.mark.parametrize("B,N,with_mask", [(16, 64, True), (16, 64, False), (5, 50, True), (33, 64, True)])
def test_pose_network_training_evaluation_is_one_node_on_the_library(B, N, with_mask):
    """_PoseNetRawFn (shared MLP + max pool + head, forward and weight gradients on csrc/pose.hip) against the same network in torch, float64,
    with the SAME dropout mask: raw output [B,7] and all 18 gradients; ragged batch / more than one row group of the head (B = 33)."""
    from dpdist_amd.registration import _PoseNetRawFn
    dev = torch.device("cuda:0")
    torch.manual_seed(4)
    net = PoseNet().to(dev)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.Linear):
                m.bias.normal_(0.0, 0.05)
    src, tmpl, _ = synth.registration_pairs(B, N, seed=3)
    clouds = torch.tensor(np.concatenate([src, tmpl]), device=dev)
    g = torch.Generator().manual_seed(7)
    mask = (torch.rand(B, 256, generator=g) < 0.7).float().div(0.7).to(dev) if with_mask else None
    up = torch.randn(B, 7, generator=g).to(dev)
    lin = [m for m in net.point if isinstance(m, torch.nn.Linear)] + [m for m in net.head if isinstance(m, torch.nn.Linear)]
    params = [t for m in lin for t in (m.weight, m.bias)]
    pred = _PoseNetRawFn.apply(clouds[:B].contiguous(), clouds[B:].contiguous(), mask, None, *params)
    grads = torch.autograd.grad((pred * up).sum(), params)
    # a second evaluation whose gradients are WRITTEN into caller storage (the optimizer's flat buffer in the registration step): the very
    # tensors come back from autograd, with the same bits (fixed summation orders)
    flat = torch.full((sum(p.numel() for p in params) + 3,), float("nan"), device=dev)
    sink, off = {}, 0
    for p in params:
        sink[id(p)] = flat[off:off + p.numel()].view_as(p)
        off += p.numel()
    pred2 = _PoseNetRawFn.apply(clouds[:B].contiguous(), clouds[B:].contiguous(), mask, sink, *params)
    grads2 = torch.autograd.grad((pred2 * up).sum(), params)
    assert torch.equal(pred, pred2) and all(torch.equal(a, b) for a, b in zip(grads, grads2))
    assert all(g.data_ptr() == sink[id(p)].data_ptr() for g, p in zip(grads2, params)) and bool(torch.isnan(flat[off:]).all())
    net64 = PoseNet().double().to(dev)
    net64.load_state_dict({k: v.double() for k, v in net.state_dict().items()})
    lin64 = [m for m in net64.point if isinstance(m, torch.nn.Linear)] + [m for m in net64.head if isinstance(m, torch.nn.Linear)]
    p64 = [t for m in lin64 for t in (m.weight, m.bias)]
    sel, _ = _native_pool_selection(net, clouds)
    f = (net64.point(clouds.double()) * sel).sum(1)             # the max pool with the library's selection (see the helper)
    h = net64.head[:6](torch.cat([f[:B], f[B:]], 1))
    if mask is not None:
        h = h * mask.double()
    ref = net64.head[7](h)
    gref = torch.autograd.grad((ref * up.double()).sum(), p64)
    assert (pred.double() - ref).abs().max().item() <= 2e-5 * max(1.0, ref.abs().max().item())
    for i, (a, r) in enumerate(zip(grads, gref)):
        scale = max(1e-6, r.abs().max().item())
        assert (a.double() - r).abs().max().item() <= 1e-3 * scale, (i, (a.double() - r).abs().max().item(), scale)
    # and through the module: train mode takes this node (a drawn mask), evaluation mode too (no mask); torch when switched off
    net.train()
    out = net.raw(clouds[:B], clouds[B:])
    assert type(out.grad_fn).__name__ == "_PoseNetRawFnBackward"
    net.native_train = False
    out_t = net.eval().raw(clouds[:B], clouds[B:])
    net.native_train = True
    out_n = net.raw(clouds[:B], clouds[B:])
    assert type(out_t.grad_fn).__name__ != "_PoseNetRawFnBackward" and (out_t - out_n).abs().max().item() <= 2e-5 * max(1.0, out_t.abs().max().item())


def test_the_library_takes_exactly_the_reference_pose_network():
    """`native_refine_supported` / `native_point_supported` are the one statement of what csrc/pose.hip implements: the network PoseNet()
    builds; another feature width, another head layer or another module are the torch path.  The point-only form reads the shared MLP alone."""
    from dpdist_amd.registration import native_point_supported, native_refine_supported
    assert native_refine_supported(PoseNet()) and native_point_supported(PoseNet())
    assert not native_refine_supported(PoseNet(out_features=512)) and not native_point_supported(PoseNet(out_features=512))
    net = PoseNet()
    net.head[0] = torch.nn.Linear(2048, 512)
    assert not native_refine_supported(net) and native_point_supported(net)
    assert not native_refine_supported(torch.nn.Linear(3, 7)) and not native_point_supported(torch.nn.Linear(3, 7))


def _tiny_registration(dev, net):
    """B = 2, N = 8, eager, a plain mean-square loss (no DPDist engine): the pairs, and the trainer around `net`."""
    from dpdist_amd.registration import IterativeRegistration
    src, tmpl, _ = synth.registration_pairs(2, 8, seed=1)
    reg = IterativeRegistration(net.to(dev), lambda a, b: (a - b).square().mean(), max_loops=3, distributed=False, graph=False)
    return torch.tensor(src, device=dev), torch.tensor(tmpl, device=dev), reg


@pytest.mark.gpu
def test_reference_pose_network_runs_on_the_library():
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    src, tmpl, reg = _tiny_registration(dev, PoseNet())
    assert reg.native_refine
    assert type(reg.net.raw(src, tmpl).grad_fn).__name__ == "_PoseNetRawFnBackward"
    assert type(reg.net._pooled(torch.cat([src, tmpl], 0)).grad_fn).__name__ == "_PointFeaturesFnBackward"
    loss, T = reg.train_step(src, tmpl)
    assert bool(torch.isfinite(loss)) and T.shape == (2, 4, 4)
    # a source that wants a gradient itself: the library's nodes give weight gradients only, so torch takes it
    out = reg.net.raw(src.clone().requires_grad_(True), tmpl)
    assert out.grad_fn is not None and type(out.grad_fn).__name__ != "_PoseNetRawFnBackward"
    reg.close()


@pytest.mark.gpu
def test_another_pose_network_stays_in_torch_everywhere():
    """out_features = 512 is not the library's network: `raw`, `_pooled` and the refinements all take torch (the pose algebra stays on
    csrc/pose.hip), and the step still trains."""
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    src, tmpl, reg = _tiny_registration(dev, PoseNet(out_features=512))
    assert not reg.native_refine
    out, f = reg.net.raw(src, tmpl), reg.net._pooled(torch.cat([src, tmpl], 0))
    assert out.grad_fn is not None and type(out.grad_fn).__name__ != "_PoseNetRawFnBackward"
    assert f.grad_fn is not None and type(f.grad_fn).__name__ != "_PointFeaturesFnBackward"
    loss, T = reg.train_step(src, tmpl)
    assert bool(torch.isfinite(loss)) and T.shape == (2, 4, 4)
    reg.close()

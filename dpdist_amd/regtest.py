"""The registration experiment's test protocol on the HIP kernels of csrc/regtest.hip (its baseline loss: csrc/chamfer.hip): what the reference's run script ends every leg
(EMD, Chamfer, ours) with, and what its paper reports.

Restates (relative to the reference's pcrnet-registration/):
    results_itrPCRNet_no_stop.py:256-258,321-378   the no-stop loop: TE, RE, CE [iterations + 1, pairs], row 0 = the identity
    results_itrPCRNet_no_stop.py:394-401           the nested success buckets 20 deg / 0.2, 10 / 0.1, 5 / 0.05, 2.5
    results_itrPCRNet_no_stop.py:433-462           plot_iter_graph: mean and std per iteration (the numbers, not the plot)
    results_itrPCRNet_no_stop.py:464-474           get_error: find_errors(gt, find_final_pose_inv(T) + centroid)
    helper.py:963-982                              add_occlusions (--add_occlusions)
    helper.py:464-470                              add_noise (the noise leg)
    helper.py:771-...                              log_test_results: test.txt
    utils/tf_util_loss.py:35-39                    chamfer: (mean sqrt d1 + mean sqrt d2) / 2, PCRNet's --loss_type chamf
The reference tests one pair per network evaluation; here a batch of pairs goes through dpd_pose_refine and ONE dpd_pose_trace launch
produces every pair's and every iteration's errors.  There is no torch fallback: a pose network the library does not implement raises.
"""
import os
import time

import numpy as np
import torch

from . import lib as L
from .baselines import _chamfer_paired

# (name, rotation bound in degrees, translation bound or None), outermost first: results_itrPCRNet_no_stop.py:394-401
BUCKETS = (("idxs_20_2", 20.0, 0.2), ("idxs_10_1", 10.0, 0.1), ("idxs_5_5", 5.0, 0.05), ("idxs_25_5", 2.5, None))


def _cloud(t, name):
    L.req(t, name=name)
    if t.dim() != 3 or t.shape[2] != 3:
        raise RuntimeError("%s must be [B,N,3], got %s" % (name, tuple(t.shape)))
    return t.shape[0], t.shape[1]


def occlude_with(source, seed_idx, order_key, drop, return_index=False):
    """One dpd_occlude call with the caller's draws: seed_idx [B] int32 (the point the hole grows around), order_key [B,N] float32 or None
    (the survivors' output order), drop = points removed per cloud.  Returns the occluded clouds [B,N,3] (and the source index of every
    output row, [B,N] int32)."""
    B, N = _cloud(source, "source")
    L.req(seed_idx, torch.int32, "seed_idx", shape=(B,))
    if order_key is not None:
        L.req(order_key, name="order_key", shape=(B, N))
    if B and (int(seed_idx.min()) < 0 or int(seed_idx.max()) >= N):
        raise RuntimeError("seed_idx must lie in [0, %d)" % N)
    out = torch.empty_like(source)
    kept = torch.empty(B, N, device=source.device, dtype=torch.int32) if return_index else None
    L.check(L.load().dpd_occlude(L.ptr(source), L.ptr(seed_idx), L.ptr(order_key), B, N, int(drop), L.ptr(out), L.ptr(kept),
                                 L.cur_stream()), "dpd_occlude")
    return (out, kept) if return_index else out


def occlude(source, fraction, generator=None):
    """helper.add_occlusions(source, fraction): per cloud, the int(fraction * N) points nearest a random point of the cloud are cut out
    and the survivors, in random order, are repeated up to N points.  The random point and the order are drawn with torch on the device."""
    B, N = _cloud(source, "source")
    seed_idx = torch.randint(0, N, (B,), device=source.device, dtype=torch.int32, generator=generator)
    key = torch.rand(B, N, device=source.device, generator=generator)
    return occlude_with(source, seed_idx, key, int(fraction * N))


def add_noise(source, generator=None):
    """helper.add_noise: per point sigma = 0.04 U(0,1), then + N(0, sigma) per coordinate.  Plain torch on the device."""
    B, N = _cloud(source, "source")
    sigma = 0.04 * torch.rand(B, N, 1, device=source.device, generator=generator)
    return source + sigma * torch.randn(B, N, 3, device=source.device, generator=generator)


def chamfer_sqrt(a, b):
    """chamfer(pcd1, pcd2) of utils/tf_util_loss.py:35-39: (mean sqrt(nearest squared distance a->b) + mean sqrt(... b->a)) / 2.
    A coincident pair contributes a zero gradient (the reference: NaN)."""
    return _chamfer_paired(a, b, "sqrt")


def pose_trace(pred, gt_pose, shift=None, lim_rot=45.0):
    """One dpd_pose_trace call: pred [L,B,7] (pose_refine_native's raw outputs), gt_pose [B,6] float32, shift [B,3] or None ->
    (T_all [L+1,B,4,4] float32, te, re, ce [L+1,B] float64), all on the device."""
    L.req(pred, name="pred")
    if pred.dim() != 3 or pred.shape[2] != 7:
        raise RuntimeError("pred must be [L,B,7], got %s" % (tuple(pred.shape),))
    loops, B = pred.shape[0], pred.shape[1]
    L.req(gt_pose, name="gt_pose", shape=(B, 6))
    if shift is not None:
        L.req(shift, name="shift", shape=(B, 3))
    dev = pred.device
    T_all = torch.empty(loops + 1, B, 4, 4, device=dev)
    te, re, ce = (torch.empty(loops + 1, B, device=dev, dtype=torch.float64) for _ in range(3))
    L.check(L.load().dpd_pose_trace(L.ptr(pred), loops, B, float(lim_rot or 0.0), L.ptr(gt_pose), L.ptr(shift), L.ptr(T_all), L.ptr(te),
                                    L.ptr(re), L.ptr(ce), L.cur_stream()), "dpd_pose_trace")
    return T_all, te, re, ce


def buckets(trans_err, rot_err):
    """The four index lists of results_itrPCRNet_no_stop.py:394-401, each inside the one before it."""
    trans_err, rot_err = np.asarray(trans_err), np.asarray(rot_err)
    ok = np.ones(len(rot_err), bool)
    out = {}
    for name, rot, trans in BUCKETS:
        ok = ok & (rot_err < rot) & (True if trans is None else trans_err < trans)
        out[name] = [int(i) for i in np.nonzero(ok)[0]]
    return out


def summarize(TE, RE, CE, seconds=0.0):
    """TE, RE, CE [iterations + 1, P] -> the result dictionary of no_stop_test (everything but the transforms)."""
    TE, RE, CE = (np.asarray(x, dtype=np.float64) for x in (TE, RE, CE))
    P = TE.shape[1]
    return {"TE": TE, "RE": RE, "CE": CE, "pairs": P, "iterations": TE.shape[0] - 1, "buckets": buckets(TE[-1], RE[-1]),
            "per_iteration": {"rot_mean": RE.mean(1), "rot_std": RE.std(1), "trans_mean": TE.mean(1), "trans_std": TE.std(1),
                              "conv_mean": CE.mean(1), "conv_std": CE.std(1)},
            "seconds": float(seconds), "pairs_per_s": P / seconds if seconds > 0 else 0.0}


def no_stop_test(net, sources, templates, gt_poses, iterations=8, batch=16, occlusions=0.0, noise=False, centroid_sub=False,
                 generator=None):
    """The no-stop test of results_itrPCRNet_no_stop.py over P pairs: sources, templates [P,N,3], gt_poses [P,6] (t, rx, ry, rz; radians).
    Per batch: centroid subtraction of the source (centroid_sub), add_noise (noise), occlude (occlusions > 0), `iterations` refinements
    of `net` in evaluation mode (no dropout) on the library, one trace launch.  Returns TE, RE, CE [iterations + 1, P] (float64 numpy:
    translation, rotation in degrees, convergence), T [P,4,4] (the final transforms of the -- centred -- sources, float32), `shift` [P,3]
    (the subtracted centroids, zeros without centroid_sub), `buckets` (four nested index lists),
    `per_iteration` (mean / std of every table row), `pairs_per_s`.  A last partial batch is evaluated at its own size."""
    from .registration import native_refine_supported, pose_refine_native
    if not native_refine_supported(net):
        raise RuntimeError("no_stop_test: the pose network is not the architecture csrc/pose.hip implements (there is no torch fallback)")
    dev = next(net.parameters()).device
    sources, templates = (torch.as_tensor(x, dtype=torch.float32, device=dev) for x in (sources, templates))
    gt = torch.as_tensor(gt_poses, dtype=torch.float32, device=dev).contiguous()      # the C entry takes the poses in float32
    P, N = _cloud(sources.contiguous(), "sources")
    if tuple(templates.shape) != (P, N, 3) or tuple(gt.shape) != (P, 6):
        raise RuntimeError("templates must be [%d,%d,3] and gt_poses [%d,6], got %s and %s" % (P, N, P, tuple(templates.shape), tuple(gt.shape)))
    if iterations < 1 or batch < 1 or P < 1:
        raise RuntimeError("no_stop_test needs iterations, batch and pairs >= 1")
    tabs, Ts, shifts = [], [], []
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    with torch.no_grad():
        for i in range(0, P, batch):
            src, tmpl = sources[i:i + batch].contiguous(), templates[i:i + batch].contiguous()
            shift = None
            if centroid_sub:
                shift = src.mean(1)
                src = src - shift[:, None, :]
            if noise:
                src = add_noise(src, generator)
            if occlusions > 0.0:
                src = occlude(src, occlusions, generator)
            _, _, pred = pose_refine_native(net, src, tmpl, iterations, None, want_pred=True)      # is_training = False: no dropout mask
            T_all, te, re, ce = pose_trace(pred, gt[i:i + batch], shift, net.lim_rot)
            tabs.append(torch.stack([te, re, ce]))
            Ts.append(T_all[iterations])
            shifts.append(shift if shift is not None else torch.zeros(src.shape[0], 3, device=dev))
        tab = torch.cat(tabs, 2).cpu().numpy()
        T = torch.cat(Ts, 0).cpu().numpy()
    res = summarize(tab[0], tab[1], tab[2], time.perf_counter() - t0)
    res["T"], res["shift"] = T, torch.cat(shifts, 0).cpu().numpy()
    return res


def write_results(log_dir, result, filename="test"):
    """log_data.npz (TE, RE, CE; stands in for the reference's log_data.h5) and <filename>.txt with the counts and means under the names
    helper.log_test_results gives them.  The reference's ITR is `iterations` for every pair (no-stop), its TIME the mean time per pair."""
    os.makedirs(log_dir, exist_ok=True)
    TE, RE, CE = (np.asarray(result[k], dtype=np.float64) for k in ("TE", "RE", "CE"))
    np.savez(os.path.join(log_dir, "log_data.npz"), TE=TE, RE=RE, CE=CE)
    trans, rot = TE[-1], RE[-1]
    P = len(rot)
    per_pair = float(result.get("seconds", 0.0)) / max(P, 1)
    idx = result.get("buckets") or buckets(trans, rot)
    with open(os.path.join(log_dir, filename + ".txt"), "w") as f:
        f.write("Mean of Time: {}\n".format(per_pair))
        f.write("Mean Translation Err: {}\n".format(np.mean(trans)))
        f.write("Var Translation Err: {}\n".format(np.var(trans)))
        f.write("Mean Rotation Err: {}\n".format(np.mean(rot)))
        f.write("Var Rotation Err: {}\n".format(np.var(rot)))
        for name, title in (("idxs_25_5", "2.5 Degree & 0.05 Units"), ("idxs_5_5", "5 Degree & 0.05 Units"),
                            ("idxs_10_1", "10 Degree & 0.1 Units"), ("idxs_20_2", "20 Degree & 0.2 Units")):
            sel = np.asarray(idx[name], dtype=np.int64)
            n = len(sel)
            f.write("\n###### {} ######\n".format(title))
            f.write("Count: {}\n".format(n))
            f.write("Accuray: {}%\n".format(100.0 * n / P))
            f.write("Mean rotational error: {}\n".format(rot[sel].mean() if n else 0))
            f.write("Mean translation error: {}\n".format(trans[sel].mean() if n else 0))
            f.write("Mean time: {}\n".format(per_pair if n else 0))
            f.write("Var translation error: {}\n".format(trans[sel].var() if n else 0))
            f.write("Var rotational error: {}\n".format(rot[sel].var() if n else 0))
            f.write("Mean Iterations: {}\n".format(TE.shape[0] - 1 if n else 0))
    return os.path.join(log_dir, "log_data.npz"), os.path.join(log_dir, filename + ".txt")


def read_results(log_dir):
    """TE, RE, CE of a write_results directory."""
    with np.load(os.path.join(log_dir, "log_data.npz")) as z:
        return z["TE"], z["RE"], z["CE"]

"""The registration test protocol at the demo's evaluation shape (128 held-out pairs of 64 points, batch 16, 8 iterations, untrained
pose network): wall time of the former per-pair host evaluation (IterativeRegistration.evaluate per batch, then find_final_pose_inv /
find_errors / centroid_residual per pair on the host: tools/registration_demo.py's evaluate() before the protocol ran on the device)
against regtest.no_stop_test, and the three kernels of csrc/regtest.hip by in-stream events.

    python tools/regtest_bench.py > profiles/regtest_bench.txt

Wall times: median of 5 after a warm-up, each bracketed by a device synchronisation.  Kernel times: event pairs around `reps`
back-to-back launches, 7 windows, median and best (tools/emd_bench.py's form)."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dpdist_amd import regtest, synth  # noqa: E402
from dpdist_amd import registration as R  # noqa: E402
from dpdist_amd.aue import chamfer_dist  # noqa: E402
from emd_bench import windows  # noqa: E402

PAIRS, N, BATCH, LOOPS = 128, 64, 16, 8


def wall(fn, n=5):
    fn()
    out = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out)), float(min(out))


def main():
    print("device: %s   %d pairs of %d points, batch %d, %d iterations" % (torch.cuda.get_device_name(0), PAIRS, N, BATCH, LOOPS))
    torch.manual_seed(0)
    net = R.PoseNet().cuda()
    src, tmpl, gt = synth.registration_pairs(PAIRS, N, seed=99)
    es, et = torch.from_numpy(src).cuda(), torch.from_numpy(tmpl).cuda()
    reg = R.IterativeRegistration(net, lambda m, t: chamfer_dist(m, t), max_loops=LOOPS, graph=False)

    def host_path():
        errs = []
        for i in range(0, PAIRS, BATCH):
            l, T = reg.evaluate(es[i:i + BATCH], et[i:i + BATCH])
            Tn = T.double().cpu().numpy()
            fp = R.find_final_pose_inv(Tn)
            cr = R.centroid_residual(Tn, gt[i:i + BATCH], src[i:i + BATCH])
            errs += [R.find_errors(gt[i + j], fp[j]) + (cr[j],) for j in range(fp.shape[0])]
            l.item()
        return np.array(errs)

    errs = host_path()
    res = regtest.no_stop_test(net, es, et, gt, iterations=LOOPS, batch=BATCH)
    print("last table row vs the host path (float64 poses there, float32 at the entry): max |d rot| %.3g deg   max |d trans| %.3g"
          % (np.abs(res["RE"][-1] - errs[:, 1]).max(), np.abs(res["TE"][-1] - errs[:, 0]).max()))
    hm, hb = wall(host_path)
    nm, nb = wall(lambda: regtest.no_stop_test(net, es, et, gt, iterations=LOOPS, batch=BATCH))
    om, ob = wall(lambda: regtest.no_stop_test(net, es, et, gt, iterations=LOOPS, batch=BATCH, occlusions=0.25, noise=True, centroid_sub=True))
    print("per-pair host evaluation (final transform only)          median %8.3f ms   best %8.3f ms" % (hm, hb))
    print("no_stop_test (all %d iterations' tables)                   median %8.3f ms   best %8.3f ms   (%.1f x)" % (LOOPS, nm, nb, hm / nm))
    print("no_stop_test + centroid_sub + noise + occlusions 0.25    median %8.3f ms   best %8.3f ms" % (om, ob))
    reg.close()

    g = torch.Generator(device="cuda")
    g.manual_seed(0)
    gt32 = torch.from_numpy(gt.astype(np.float32)).cuda()
    with torch.no_grad():
        _, _, pred = R.pose_refine_native(net, es[:BATCH], et[:BATCH], LOOPS, None, want_pred=True)
    print("kernels (in-stream events):")
    med, best = windows(lambda: regtest.pose_trace(pred, gt32[:BATCH], None, net.lim_rot), 200)
    print("  dpd_pose_trace      L = %d, B = %-4d          median %8.4f ms   best %8.4f ms" % (LOOPS, BATCH, med, best))
    for n in (64, 512, 2048):
        s, _, _ = synth.registration_pairs(BATCH, n, seed=5)
        s = torch.from_numpy(s).cuda()
        seed = torch.randint(0, n, (BATCH,), device="cuda", dtype=torch.int32, generator=g)
        key = torch.rand(BATCH, n, device="cuda", generator=g)
        out = torch.empty_like(s)
        lib = regtest.L.load()
        fn = lambda: regtest.L.check(lib.dpd_occlude(regtest.L.ptr(s), regtest.L.ptr(seed), regtest.L.ptr(key), BATCH, n, n // 4,      # noqa: E731
                                                     regtest.L.ptr(out), None, regtest.L.cur_stream()), "dpd_occlude")
        med, best = windows(fn, 200 if n < 2048 else 50)
        print("  dpd_occlude         B = %d, N = %-4d, drop N/4  median %8.4f ms   best %8.4f ms" % (BATCH, n, med, best))
        a = s.clone().requires_grad_(True)
        b = torch.from_numpy(synth.registration_pairs(BATCH, n, seed=6)[1]).cuda()

        def fb():
            torch.autograd.grad(regtest.chamfer_sqrt(a, b), [a])
        med, best = windows(fb, 100)
        print("  dpd_chamfer_sqrt    B = %d, N = M = %-4d fwd+bwd median %8.4f ms   best %8.4f ms" % (BATCH, n, med, best))


if __name__ == "__main__":
    main()

"""dpd_nn_dist at the label generator's shapes, against the exact-difference torch.cdist on the same GPU and scipy's cdist on the host.

    python tools/nn_dist_bench.py [--no-scipy] > profiles/nn_dist_bench.txt

Timing: in-stream event pairs around `reps` back-to-back launches (every shape warmed first; reps sized so that a window lasts tens of
milliseconds at least), 7 windows, median and best reported.  The yardstick is
torch.cdist(q, p, compute_mode="donot_use_mm_for_euclid_dist").min(-1): the exact-difference form (the mm form does not meet the accuracy
contract of the labels), over QCHUNK queries at a time.  In one call at M = 50 000, P = 10 000 it returned distances off by up to 0.58 on
MI355X (torch 2.x ROCm; it launches one workgroup per matrix element, 5e8 of them), so the yardstick runs in chunks, at which its result
matches dpd_nn_dist to 6e-8; the tool checks that before it times anything.  The scipy line is what the reference's generator pays per draw
(dataset_sample_with_gt.py:90-91)."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dpdist_amd import dataset as D  # noqa: E402

P, M = 10000, 50000
QCHUNK = 1600          # queries per torch.cdist call: 1600 x 10 000 matrix elements


def windows(fn, reps, n=7):
    for _ in range(max(3, reps // 4)):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / reps)
    return float(np.median(out)), float(min(out))


def main():
    rng = np.random.default_rng(0)
    print("device: %s   P = %d reference points, M = %d queries per shape" % (torch.cuda.get_device_name(0), P, M))
    for S in (1, 16):
        g = rng.standard_normal((S, P, 3))
        p = torch.from_numpy((0.6 * g / np.linalg.norm(g, axis=2, keepdims=True)).astype(np.float32)).cuda()
        g = rng.standard_normal((S, 5, M))
        q = torch.from_numpy(np.ascontiguousarray((g[:, 2:5] / np.sqrt((g * g).sum(1, keepdims=True))).transpose(0, 2, 1)).astype(np.float32)).cuda()
        ours = lambda: D.nn_distance(p, q)                                                                  # noqa: E731
        ref = lambda: torch.cat([torch.cdist(q[s:s + 1, i:i + QCHUNK], p[s:s + 1], compute_mode="donot_use_mm_for_euclid_dist").min(-1).values   # noqa: E731
                                 for s in range(S) for i in range(0, M, QCHUNK)], 1).view(S, M)
        d0, d1 = ours(), ref()
        err = (d0 - d1).abs().max().item()
        print("S = %2d   max |dpd_nn_dist - torch.cdist.min| = %.3g" % (S, err))
        assert err <= 1e-6, "the yardstick does not compute the same thing"
        med, best = windows(ours, 200 if S == 1 else 20)
        pairs = S * P * M
        print("S = %2d   dpd_nn_dist                     median %9.4f ms   best %9.4f ms   (%.2f T pairs/s)" % (S, med, best, pairs / med / 1e9))
        rmed, rbest = windows(ref, 4 if S == 1 else 1, n=5)
        print("S = %2d   torch.cdist(exact diff).min(-1)  median %9.4f ms   best %9.4f ms   (dpd_nn_dist is %.1f x faster)" % (S, rmed, rbest, rmed / med))
        del d0, d1
        if S == 1 and "--no-scipy" not in sys.argv:
            from scipy.spatial.distance import cdist
            pn, qn = p[0].cpu().numpy(), q[0].cpu().numpy()
            t0 = time.perf_counter()
            dh = cdist(pn, qn).min(0)
            t = time.perf_counter() - t0
            print("S =  1   scipy cdist(P x M float64).min(0) on the host: %.2f s per draw   max |dpd_nn_dist - scipy| = %.3g"
                  % (t, np.abs(ours()[0].cpu().numpy() - dh).max()))


if __name__ == "__main__":
    main()

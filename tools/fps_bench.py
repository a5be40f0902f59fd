"""dpd_fps_order (csrc/fps.hip) at the registration's and the resampler's shapes, against the same loop written in torch ops on the same GPU.

    python tools/fps_bench.py > profiles/fps_bench.txt

(S, N, K): (16, 2048, 64) and (16, 2048, 1024) are template clouds of the registration (register-resident form); (1, 50000, 10000) and
(16, 50000, 10000) are resample_tree's launches on 50 000-row shape files (streamed form; one cloud occupies one CU).  The yardstick is
the definition's loop in torch element-wise ops -- (dx*dx + dy*dy) + dz*dz as separate kernels, torch.minimum, argmax -- K dependent
rounds of ~12 launches with no host synchronisation in between; on random clouds (no exact ties) it must give the SAME order, which the
tool asserts before it times anything.  Timing: in-stream event pairs around `reps` back-to-back calls after a warm-up, 5 windows (3 for
the yardstick's long runs), median and best; "us / iteration" is the median over K."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dpdist_amd import farthest_point_order  # noqa: E402

SHAPES = [(16, 2048, 64, 50, 2), (16, 2048, 1024, 10, 1), (1, 50000, 10000, 2, 1), (16, 50000, 10000, 1, 1)]   # S, N, K, reps, yardstick reps


def torch_fps(p, K):
    S, N, _ = p.shape
    x, y, z = (p[..., c].contiguous() for c in range(3))
    dmin = torch.full((S, N), float("inf"), device=p.device)
    cur = torch.zeros(S, 1, dtype=torch.long, device=p.device)
    order = torch.empty(S, K, dtype=torch.long, device=p.device)
    for k in range(K):
        order[:, k:k + 1] = cur
        dx, dy, dz = x - x.gather(1, cur), y - y.gather(1, cur), z - z.gather(1, cur)
        dmin = torch.minimum(dmin, (dx * dx + dy * dy) + dz * dz)
        dmin.scatter_(1, cur, -1.0)
        cur = dmin.argmax(1, keepdim=True)
    return order


def windows(fn, reps, n):
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
    print("device: %s" % torch.cuda.get_device_name(0))
    for S, N, K, reps, yreps in SHAPES:
        p = torch.from_numpy(np.random.default_rng([S, N]).uniform(-1, 1, (S, N, 3)).astype(np.float32)).cuda()
        ours = lambda: farthest_point_order(p, K)          # noqa: E731
        ref = lambda: torch_fps(p, K)                      # noqa: E731
        same = bool((ours().long() == ref()).all())
        print("S = %2d  N = %5d  K = %5d   orders equal to the torch loop: %s" % (S, N, K, same))
        assert same, "the yardstick does not compute the same order"
        med, best = windows(ours, reps, 5)
        print("S = %2d  N = %5d  K = %5d   dpd_fps_order   median %10.3f ms   best %10.3f ms   %8.2f us / iteration" % (S, N, K, med, best, 1e3 * med / K))
        rmed, rbest = windows(ref, yreps, 3)
        print("S = %2d  N = %5d  K = %5d   torch loop      median %10.3f ms   best %10.3f ms   %8.2f us / iteration   (dpd_fps_order is %.1f x faster)"
              % (S, N, K, rmed, rbest, 1e3 * rmed / K, rmed / med))


if __name__ == "__main__":
    main()

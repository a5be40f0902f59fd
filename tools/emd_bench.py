"""dpd_emd_fwd (forward with both gradients, the fused form: no [B,m,n] array) against a torch implementation of the same contract
(include/dpdist_capi.h) on the same GPU, at B = 16 and n = m = 64 / 512 / 2048.

    python tools/emd_bench.py > profiles/emd_bench.txt

Timing: in-stream event pairs around `reps` back-to-back evaluations (warmed first), 7 windows, median and best.  The yardstick keeps d2
and its square root from one level to the next and uses batched matrix-vector products for the sums, i.e. it is the fast way to write
this in torch, not the slow one; it still materialises [B,n,m] arrays about 40 times per evaluation.  It is verified against the kernel
before anything is timed: cost to 1e-5 relative, each gradient to 1e-3 in relative L2 norm.  Both sides are fp32 with different
exponentials and summation orders, and single gradient entries of two fp32 runs differ by up to 1e-3 of the largest entry (the clamps
pass a rounding of a sharp level on to single match entries; tests/test_emd_cpu.py measures the same between numpy fp32 and fp64), so the
largest entry-wise difference is printed, not asserted."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dpdist_amd import emd  # noqa: E402

B = 16
LEVELS = [-(4.0 ** j) for j in range(7, -2, -1)] + [0.0]


def torch_emd(x1, x2):
    """cost [B], loss, grad1, grad2 of the contract, fp32 torch ops"""
    Bn, n, m = x1.shape[0], x1.shape[1], x2.shape[1]
    d = x1[:, :, None, :] - x2[:, None, :, :]                                       # [B,n,m,3]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]    # [B,n,m]
    big = float(max(n, m))
    remainL = torch.full((Bn, n), big / n, device=x1.device)
    remainR = torch.full((Bn, m), big / m, device=x1.device)
    match = torch.zeros_like(d2)                                                    # [B,n,m] = match[l][k] transposed
    for level in LEVELS:
        e = torch.exp(level * d2)
        ratioL = remainL / (1e-9 + torch.bmm(e, remainR[:, :, None])[:, :, 0])
        s = remainR * torch.bmm(ratioL[:, None, :], e)[:, 0, :]
        ratioR = torch.clamp(remainR / (s + 1e-9), max=1.0) * remainR
        remainR = torch.clamp(remainR - s, min=0.0)
        e.mul_(ratioL[:, :, None]).mul_(ratioR[:, None, :])
        match.add_(e)
        remainL = torch.clamp(remainL - e.sum(2), min=0.0)
    cost = (match * torch.sqrt(d2)).sum((1, 2))
    t = match * torch.rsqrt(torch.clamp(d2, min=1e-20))
    scale = 1.0 / (Bn * n)
    g1 = torch.einsum("bnm,bnmc->bnc", t, d) * scale
    g2 = torch.einsum("bnm,bnmc->bmc", t, d) * -scale
    return cost, (cost / n).mean(), g1, g2


def windows(fn, reps, n=7):
    for _ in range(max(2, reps // 4)):
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
    print("device: %s   B = %d, forward with both gradients, fused form (no match array)" % (torch.cuda.get_device_name(0), B))
    rng = np.random.default_rng(0)
    slower = []
    for N, reps, rreps in ((64, 200, 20), (512, 50, 5), (2048, 10, 1)):
        x1 = torch.from_numpy(rng.uniform(-0.8, 0.8, (B, N, 3)).astype(np.float32)).cuda()
        x2 = torch.from_numpy(rng.uniform(-0.8, 0.8, (B, N, 3)).astype(np.float32)).cuda()
        ours = lambda: emd.emd_forward(x1, x2)                      # noqa: E731
        ref = lambda: torch_emd(x1, x2)                             # noqa: E731
        c0, l0, a0, b0, _ = ours()
        c1, l1, a1, b1 = ref()
        rel = lambda u, v: ((u - v).abs().max() / v.abs().max()).item()     # noqa: E731
        l2 = lambda u, v: ((u - v).norm() / v.norm()).item()                # noqa: E731
        print("n = m = %4d   yardstick vs kernel: cost %.2g   grad1 L2 %.2g (max entry %.2g)   grad2 L2 %.2g (max entry %.2g)   loss %.6f / %.6f"
              % (N, rel(c0, c1), l2(a0, a1), rel(a0, a1), l2(b0, b1), rel(b0, b1), l0.item(), l1.item()))
        assert rel(c0, c1) <= 1e-5 and max(l2(a0, a1), l2(b0, b1)) <= 1e-3, "the yardstick does not compute the same thing"
        del c1, l1, a1, b1
        med, best = windows(ours, reps)
        rmed, rbest = windows(ref, rreps, n=5)
        print("n = m = %4d   dpd_emd_fwd  median %9.4f ms   best %9.4f ms   |   torch  median %9.4f ms   best %9.4f ms   (kernel is %.1f x faster)"
              % (N, med, best, rmed, rbest, rmed / med))
        if med > rmed:
            slower.append(N)
    assert not slower, "dpd_emd_fwd is slower than the torch yardstick at n = m = %s" % slower


if __name__ == "__main__":
    main()

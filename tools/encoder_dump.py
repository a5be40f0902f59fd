#!/usr/bin/env python3
"""Every 3DmFV encoder entry of the library of one tree on fixed seeded inputs, every output (and the backward's workspace) saved to
one .npz -- two trees computed the same when their files hold the same bytes array by array.  GPU only.

    python tools/encoder_dump.py --root TREE --out FILE.npz          # imports dpdist_amd from TREE (its built library)
    python tools/encoder_dump.py --compare A.npz B.npz               # names of the arrays that differ; exit status 1 if any

Shapes (C = 3): m = 8, N = 64 (packed forward with its DPP table path, sliced backward, stacked forward with and without noise and with
ssq, and once at N = 12 on the eight-group kernel); m = 8, N = 72 (packed forward without whole table passes); m = 5, N = 13 (eight-group forward, sliced backward with a short last
slice); m = 5, N = 5 and m = 8, N = 50 without a workspace (one-launch backward); m = 8, N = 712 (tiled at the default tiles, ragged last
tile); m = 10, N = 170 forward only (two batches of Gaussians, two tiles); m = 8, N = 300 with counts (1, 7, 300); dpd_asloss_tail at
B = 2, N = 64, k = 3.  The upstream gradient is zeroed where |fv| < 2e-3, as in the tests.
"""
import argparse
import os
import sys

import numpy as np


def compare(a, b):
    A, B = np.load(a), np.load(b)
    bad = [n for n in sorted(set(A.files) | set(B.files))
           if n not in A.files or n not in B.files or A[n].shape != B[n].shape or A[n].tobytes() != B[n].tobytes()]
    print("%d arrays, %d differ%s" % (len(A.files), len(bad), ": " + ", ".join(bad) if bad else ""))
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2)
    a = ap.parse_args()
    if a.compare:
        raise SystemExit(compare(*a.compare))
    sys.path.insert(0, os.path.abspath(a.root))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("encoder_dump needs a GPU")
    from dpdist_amd import lib as L, ops
    assert os.path.abspath(L.__file__).startswith(os.path.abspath(a.root)), L.__file__
    lib, dev, s = L.load(), torch.device("cuda:0"), L.cur_stream()
    C, sigma, out = 3, 0.125, {}
    cu = lambda x, dt=torch.float32: torch.tensor(np.ascontiguousarray(x), dtype=dt, device=dev)      # noqa: E731
    nanf = lambda *sh: torch.full(sh, float("nan"), device=dev)                                        # noqa: E731

    def keep(name, t):
        torch.cuda.synchronize()
        out[name] = t.detach().cpu().numpy().copy()

    def clouds(N, m):
        rng = np.random.default_rng([41, N, m])
        return cu(rng.uniform(-0.8, 0.8, size=(C, N, 3)).astype(np.float32)), rng

    def upstream(rng, fv):
        return cu(rng.standard_normal(tuple(fv.shape)).astype(np.float32)) * (fv.abs() > 2e-3).float()

    def workspace(m):
        n = lib.dpd_mfv3d_bwd_workspace_bytes(C, m) // 4
        return nanf(n), n * 4

    def fwd(tag, pts, N, m):
        fv = nanf(C, m ** 3, 20)
        L.check(lib.dpd_mfv3d_fwd(L.ptr(pts), C, N, m, sigma, L.ptr(fv), s), "dpd_mfv3d_fwd")
        keep(tag + "/fwd", fv)
        return fv

    def bwd(tag, pts, dfv, N, m, sliced):
        g = nanf(C, N, 3)
        ws, nb = workspace(m) if sliced else (None, 0)
        L.check(lib.dpd_mfv3d_bwd(L.ptr(pts), L.ptr(dfv), C, N, m, sigma, L.ptr(g), L.ptr(ws), nb, s), "dpd_mfv3d_bwd")
        keep(tag + ("/bwd_sliced" if sliced else "/bwd_one"), g)
        if sliced:
            keep(tag + "/bwd_sliced_ws", ws)

    # ---- plain entries
    for N, m, forms in ((64, 8, (True, False)), (72, 8, ()), (13, 5, (True, False)), (5, 5, (True,)), (50, 8, (False,))):
        tag = "m%d_N%d" % (m, N)
        pts, rng = clouds(N, m)
        fv = fwd(tag, pts, N, m)
        dfv = upstream(rng, fv)
        for sliced in forms:          # N = 5 with a workspace: the entry runs the one-launch kernel (N < 2 slices)
            bwd(tag, pts, dfv, N, m, sliced)
    # ---- stacked forward: B = 2 -> 4 clouds of 64 points
    B, N, m = 2, 64, 8
    rng = np.random.default_rng([42, N, m])
    pcA, pcB = (cu(rng.uniform(-0.8, 0.8, size=(B, N, 3)).astype(np.float32)) for _ in range(2))
    noise = cu((0.01 * rng.standard_normal((B, N, 3))).astype(np.float32))
    for tag, nz, want_ssq in (("plain", None, False), ("noise", noise, False), ("noise_ssq", noise, True), ("ssq", None, True)):
        pts, q, fv = nanf(2 * B, N, 3), nanf(2 * B, N, 3), nanf(2 * B, m ** 3, 20)
        ssq = nanf(2 * B, 4, 20) if want_ssq else None
        L.check(lib.dpd_mfv3d_fwd_stacked(L.ptr(pcA), L.ptr(pcB), L.ptr(nz), B, N, m, sigma, L.ptr(pts), L.ptr(q), L.ptr(fv), L.ptr(ssq), s), "stacked")
        for n, t in (("pts", pts), ("q", q), ("fv", fv)) + ((("ssq", ssq),) if want_ssq else ()):
            keep("stacked_%s/%s" % (tag, n), t)
    # ---- the same on the eight-group kernel (N = 12)
    pA, pB, nz12 = pcA[:, :12].contiguous(), pcB[:, :12].contiguous(), noise[:, :12].contiguous()
    pts, q, fv, ssq = nanf(2 * B, 12, 3), nanf(2 * B, 12, 3), nanf(2 * B, m ** 3, 20), nanf(2 * B, 4, 20)
    L.check(lib.dpd_mfv3d_fwd_stacked(L.ptr(pA), L.ptr(pB), L.ptr(nz12), B, 12, m, sigma, L.ptr(pts), L.ptr(q), L.ptr(fv), L.ptr(ssq), s), "stacked")
    for n, t in (("pts", pts), ("q", q), ("fv", fv), ("ssq", ssq)):
        keep("stacked_N12_noise_ssq/%s" % n, t)
    # ---- tiled entries at the default tiles
    for N, m, back in ((712, 8, True), (170, 10, False)):
        tag = "m%d_N%d" % (m, N)
        pts, rng = clouds(N, m)
        fv = nanf(C, m ** 3, 20)
        L.check(lib.dpd_mfv3d_fwd_tiled(L.ptr(pts), C, N, m, sigma, 0, L.ptr(fv), s), "dpd_mfv3d_fwd_tiled")
        keep(tag + "/fwd_tiled", fv)
        if back:
            dfv, g = upstream(rng, fv), nanf(C, N, 3)
            ws, nb = workspace(m)
            L.check(lib.dpd_mfv3d_bwd_tiled(L.ptr(pts), L.ptr(dfv), C, N, m, sigma, 0, L.ptr(g), L.ptr(ws), nb, s), "dpd_mfv3d_bwd_tiled")
            keep(tag + "/bwd_tiled", g)
            keep(tag + "/bwd_tiled_ws", ws)
    # ---- ragged sets
    N, m = 300, 8
    pts, rng = clouds(N, m)
    counts = cu([1, 7, 300], torch.int32)
    fv, g = nanf(C, m ** 3, 20), nanf(C, N, 3)
    L.check(lib.dpd_mfv3d_fwd_counts(L.ptr(pts), L.ptr(counts), C, N, m, sigma, 0, L.ptr(fv), s), "dpd_mfv3d_fwd_counts")
    keep("counts/fwd", fv)
    dfv = upstream(rng, fv)
    ws, nb = workspace(m)
    L.check(lib.dpd_mfv3d_bwd_counts(L.ptr(pts), L.ptr(counts), L.ptr(dfv), C, N, m, sigma, 0, L.ptr(g), L.ptr(ws), nb, s), "dpd_mfv3d_bwd_counts")
    keep("counts/bwd", g)
    keep("counts/bwd_ws", ws)
    # ---- the as-loss tail
    B, N, m, k = 2, 64, 8, 3
    KP = ops.padded_width(k)
    pts = torch.cat([pcA, pcB])
    fv = ops.mfv3d_fwd(pts, m, sigma)
    X, mask, vox = ops.patch_rows_fwd(torch.cat([pcB, pcA]), fv, m, k)
    dX = cu((1e-3 * rng.standard_normal((2 * B * N, KP))).astype(np.float32))
    dfv, gA, gB = nanf(2 * B, m ** 3, 20), nanf(B, N, 3), nanf(B, N, 3)
    n = lib.dpd_mfv3d_bwd_workspace_bytes(2 * B, m) // 4
    ws = nanf(n)
    L.check(lib.dpd_asloss_tail(L.ptr(dX), L.ptr(vox), L.ptr(pts), None, B, N, m, k, KP, sigma, L.ptr(dfv), L.ptr(ws), n * 4, L.ptr(gA), L.ptr(gB), s),
            "dpd_asloss_tail")
    for nme, t in (("dfv", dfv), ("gA", gA), ("gB", gB), ("ws", ws)):
        keep("asloss_tail/" + nme, t)
    np.savez(a.out, **out)
    print("%d arrays -> %s" % (len(out), a.out))


if __name__ == "__main__":
    main()

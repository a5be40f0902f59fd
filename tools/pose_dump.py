#!/usr/bin/env python3
"""Every pose entry of the library of one tree on fixed seeded inputs, one sha256 per output buffer (workspaces included) -- two trees
computed the same when their listings are equal line by line: these kernels have fixed summation orders and no atomics.  GPU only.

    python tools/pose_dump.py --root TREE > LISTING          # imports dpdist_amd from TREE (its built library)
    python tools/pose_dump.py --compare A B                  # the lines that differ; exit status 1 if any

Inputs from numpy.random.default_rng with fixed seeds, weights from a seeded PoseNet() (Xavier kernels; the zero biases are redrawn so that
every bias path carries a value).  Shapes: dpd_pose_apply_fwd in both modes at lim_rot 45 and 0, with and without T_in, at (B, N) =
(5, 50) and (3, 150), dpd_pose_apply_bwd at the same; dpd_pose_refine at (B, N, loops) = (5, 50, 2), (33, 64, 1), (3, 150, 2) with a dropout
mask and pred_out; dpd_pose_point_fwd_train + dpd_pose_point_bwd at (clouds, N) = (1, 8), (6, 64), (3, 65), (4, 200), (2, 2048), the second
and fourth with duplicated points (tied maxima); dpd_pose_head_fwd_train + dpd_pose_head_bwd at B = 5 and 33 with a mask and 16 without.
"""
import argparse
import ctypes
import hashlib
import os
import sys

import numpy as np


def compare(a, b):
    A, B = (dict(line.split() for line in open(p) if line.strip()) for p in (a, b))
    bad = [n for n in sorted(set(A) | set(B)) if A.get(n) != B.get(n)]
    print("%d buffers, %d differ%s" % (len(A), len(bad), ": " + ", ".join(bad) if bad else ""))
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--compare", nargs=2)
    a = ap.parse_args()
    if a.compare:
        raise SystemExit(compare(*a.compare))
    sys.path.insert(0, os.path.abspath(a.root))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("pose_dump needs a GPU")
    from dpdist_amd import lib as L, registration as reg
    assert os.path.abspath(L.__file__).startswith(os.path.abspath(a.root)), L.__file__
    lib, dev, s = L.load(), torch.device("cuda:0"), L.cur_stream()
    cu = lambda x, dt=torch.float32: torch.tensor(np.ascontiguousarray(x), dtype=dt, device=dev)      # noqa: E731
    nanf = lambda *sh: torch.full(sh, float("nan"), device=dev)                                        # noqa: E731
    normal = lambda rng, *sh: cu(rng.standard_normal(sh).astype(np.float32))                           # noqa: E731
    uniform = lambda rng, *sh: cu(rng.uniform(-0.8, 0.8, size=sh).astype(np.float32))                  # noqa: E731

    def keep(name, t):
        torch.cuda.synchronize()
        print("%-40s %s" % (name, hashlib.sha256(t.detach().cpu().numpy().tobytes()).hexdigest()), flush=True)

    torch.manual_seed(7)
    net = reg.PoseNet()
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.Linear):
                m.bias.normal_(0.0, 0.05)
    net = net.to(dev)
    wb = [t.detach().contiguous() for m in list(net.point) + list(net.head) if isinstance(m, torch.nn.Linear) for t in (m.weight, m.bias)]
    w = L.PoseNetW()
    for i in range(5):
        w.Wp[i], w.bp[i] = wb[2 * i].data_ptr(), wb[2 * i + 1].data_ptr()
    for i in range(4):
        w.Wh[i], w.bh[i] = wb[10 + 2 * i].data_ptr(), wb[11 + 2 * i].data_ptr()
    w.out_features = OUT = 1024
    net_p = ctypes.byref(w)
    keep_prob = 0.7
    drop = lambda rng, *sh: cu(((rng.random(sh) < keep_prob) / keep_prob).astype(np.float32))          # noqa: E731

    # ---- the quaternion chain
    for B, N in ((5, 50), (3, 150)):
        rng = np.random.default_rng([51, B, N])
        pred, src, T_in, dmoved = normal(rng, B, 7), uniform(rng, B, N, 3), normal(rng, B, 4, 4), normal(rng, B, N, 3)
        for lim in (45.0, 0.0):
            for mode in (0, 1):
                for T in (T_in, None):
                    tag = "apply_fwd/B%d_N%d_lim%d_mode%d_%s" % (B, N, lim, mode, "T" if T is not None else "I")
                    pose, moved, T_out = nanf(B, 7), nanf(B, N, 3), nanf(B, 4, 4)
                    L.check(lib.dpd_pose_apply_fwd(L.ptr(pred), L.ptr(src), L.ptr(T), B, N, lim, mode, L.ptr(pose), L.ptr(moved), L.ptr(T_out), s), tag)
                    for n, t in (("pose", pose), ("moved", moved), ("T_out", T_out)):
                        keep(tag + "/" + n, t)
            dpred = nanf(B, 7)
            L.check(lib.dpd_pose_apply_bwd(L.ptr(pred), L.ptr(src), L.ptr(dmoved), B, N, lim, L.ptr(dpred), s), "dpd_pose_apply_bwd")
            keep("apply_bwd/B%d_N%d_lim%d/dpred" % (B, N, lim), dpred)
    # ---- the forward-only refinement
    for B, N, loops in ((5, 50, 2), (33, 64, 1), (3, 150, 2)):
        rng = np.random.default_rng([52, B, N])
        src, tmpl, mask = uniform(rng, B, N, 3), uniform(rng, B, N, 3), drop(rng, loops, B, 256)
        nb = lib.dpd_pose_refine_workspace_bytes(B, N, OUT)
        ws, moved, T, pred = nanf(nb // 4), nanf(B, N, 3), nanf(B, 4, 4), nanf(loops, B, 7)
        L.check(lib.dpd_pose_refine(net_p, L.ptr(src), L.ptr(tmpl), B, N, loops, 45.0, L.ptr(mask), L.ptr(ws), nb, L.ptr(moved), L.ptr(T), L.ptr(pred), s),
                "dpd_pose_refine")
        for n, t in (("moved", moved), ("T", T), ("pred", pred), ("ws", ws)):
            keep("refine/B%d_N%d_loops%d/%s" % (B, N, loops, n), t)
    # ---- shared MLP, training evaluation and backward
    for C, N, dup in ((1, 8, 0), (6, 64, 20), (3, 65, 0), (4, 200, 60), (2, 2048, 0)):
        rng = np.random.default_rng([53, C, N])
        pts = rng.uniform(-0.8, 0.8, size=(C, N, 3)).astype(np.float32)
        pts[:, N - dup:] = pts[:, :dup]                    # the last `dup` points repeat the first: tied maxima
        nA = (C + 1) // 2
        nB = C - nA
        ptsA, ptsB = cu(pts[:nA]), (cu(pts[nA:]) if nB else None)
        NW = lib.dpd_pose_point_tie_words(N)
        f, h = nanf(C, OUT), [nanf(C * N, k) for k in (64, 64, 64, 128)]
        ties = torch.full((C, NW, OUT), -1, dtype=torch.int64, device=dev)
        L.check(lib.dpd_pose_point_fwd_train(net_p, L.ptr(ptsA), L.ptr(ptsB), nA, nB, N, L.ptr(f), L.ptr(h[0]), L.ptr(h[1]), L.ptr(h[2]), L.ptr(h[3]),
                                             ties.data_ptr(), s), "dpd_pose_point_fwd_train")
        tag = "point/C%d_N%d/" % (C, N)
        for n, t in (("f", f), ("h1", h[0]), ("h2", h[1]), ("h3", h[2]), ("h4", h[3]), ("ties", ties)):
            keep(tag + n, t)
        df = normal(rng, C, OUT)
        dW = [nanf(*wb[2 * i].shape) for i in range(5)]
        db = [nanf(*wb[2 * i + 1].shape) for i in range(5)]
        nb = lib.dpd_pose_point_bwd_workspace_bytes_n(C, N)
        ws = nanf(nb // 4)
        L.check(lib.dpd_pose_point_bwd(net_p, L.ptr(ptsA), L.ptr(ptsB), nA, nB, N, L.ptr(df), L.ptr(h[0]), L.ptr(h[1]), L.ptr(h[2]), L.ptr(h[3]),
                                       ties.data_ptr(), reg._ptr_array(dW), reg._ptr_array(db), L.ptr(ws), nb, s), "dpd_pose_point_bwd")
        for i in range(5):
            keep(tag + "dW%d" % (i + 1), dW[i])
            keep(tag + "db%d" % (i + 1), db[i])
        keep(tag + "bwd_ws", ws)
    # ---- head, training evaluation and backward
    for B, masked in ((5, True), (33, True), (16, False)):
        rng = np.random.default_rng([54, B])
        f = cu(np.abs(rng.standard_normal((2 * B, OUT))).astype(np.float32))      # pooled ReLU outputs: >= 0
        mask = drop(rng, B, 256) if masked else None
        h1, h2, h3, pred = nanf(B, 1024), nanf(B, 512), nanf(B, 256), nanf(B, 7)
        L.check(lib.dpd_pose_head_fwd_train(net_p, L.ptr(f), B, L.ptr(mask), L.ptr(h1), L.ptr(h2), L.ptr(h3), L.ptr(pred), s), "dpd_pose_head_fwd_train")
        tag = "head/B%d/" % B
        for n, t in (("h1", h1), ("h2", h2), ("h3", h3), ("pred", pred)):
            keep(tag + n, t)
        dpred = normal(rng, B, 7)
        dW = [nanf(*wb[10 + 2 * i].shape) for i in range(4)]
        db = [nanf(*wb[11 + 2 * i].shape) for i in range(4)]
        nb = lib.dpd_pose_head_bwd_workspace_bytes(B)
        ws, df = nanf(nb // 4), nanf(2 * B, OUT)
        L.check(lib.dpd_pose_head_bwd(net_p, L.ptr(f), B, L.ptr(mask), L.ptr(h1), L.ptr(h2), L.ptr(h3), L.ptr(dpred), reg._ptr_array(dW), reg._ptr_array(db),
                                      L.ptr(df), L.ptr(ws), nb, s), "dpd_pose_head_bwd")
        for i in range(4):
            keep(tag + "dW%d" % (i + 1), dW[i])
            keep(tag + "db%d" % (i + 1), db[i])
        keep(tag + "df", df)
        keep(tag + "bwd_ws", ws)


if __name__ == "__main__":
    main()

"""The all-pairs Chamfer matrix (dpdist_amd.chamfer_matrix / ChamferMatrix, squared form) against the only route there was before it:
the two sets expanded by hand into Ca * Cb explicit pairs, in batches of whole rows of the matrix, through the paired entries
dpd_chamfer_fwd / dpd_chamfer_bwd, with the per-pair means taken in torch.

    matrix     chamfer_matrix(A, B, countsA=, countsB=)                  forward+backward: ChamferMatrix, loss = (G * D).sum(), random G
    expanded   per batch: A_i repeated Cb times beside B tiled, dpd_chamfer_fwd (minima and argmins of every pair), means per pair in
               torch; backward, full sets: dpd_chamfer_bwd (one uniform weight) scaled per pair by G, then summed over the pairs of each
               cloud; backward, ragged sets: the paired entries have no per-cloud counts, so a ragged set is padded with copies of each
               cloud's first point (which changes no minimum), the means are masked in torch, and the gradient is gathered / scattered
               in torch through the stored argmins (dpd_chamfer_bwd weighs every pair by its padded width)

at   full     Ca = Cb = 64, N = M = 1024
     ragged   the same widths, counts uniform in [N / 4, N]

    python tools/baseline_matrix_bench.py [--out profiles/baseline_matrix_bench.txt]

The two routes alternate, `--rounds` calls after two warm-up calls, each timed with an in-stream device event pair.  Before anything is
timed both routes are held to the bars of tests/test_baseline_matrix_gpu.py against a float64 evaluation (on the device, through the
argmins the paired entry stored): D within twice the mean bar (max(n_ab, n_ba) + 3) u ref of each other, each gradient element within
(T + c) u S of float64 with c = 4 for the matrix and 8 for the expanded route (it rounds its weights differently); the tool refuses to
time otherwise.  No threshold is set on the times.

    python tools/baseline_matrix_bench.py --emd [--out profiles/emd_matrix_bench.txt]

times the all-pairs Earth Mover's distance instead (dpdist_amd.emd_matrix / EMDMatrix: one workgroup per pair, one launch) against the
route there was before it: the Ca * Cb pairs expanded into [Ca * Cb, n, 3] copies and sent through the paired entry dpd_emd_fwd (22
dependent launches over all pairs), the per-pair upstream applied and the pairs summed in torch.  Full sets (the paired entry has no
counts), at 32 x 32 clouds of 64 points, 16 x 16 of 256, 8 x 8 of 1024 and 4 x 4 of 2048.  The time of the copies is part of the
expanded route and is shown on its own as well.  Before a shape is timed D of the two routes has to be the same bits and every gradient
element within 4 (C + 4) u S of the other route's (C terms of absolute sum S, each rounded a few times differently)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dpdist_amd import ChamferMatrix, chamfer_matrix  # noqa: E402
from dpdist_amd import lib as L  # noqa: E402

U = 2.0 ** -24

# Not measured by this tool: read by hand from the gfx950 ISA of csrc/chamfer_matrix.hip (the scans' inner loops over four surface points)
# and written into the record as stated, so that a rerun keeps it.  Re-read it when cm_scan changes.
ISA_NOTE = """# VALU instructions per point-pair evaluation, read from the gfx950 ISA of csrc/chamfer_matrix.hip (a constant of the tool, not a measurement of this run):
#   forward, 4 queries per thread (cm_scan<4, false>):             113 VALU (32 packed) + 3 ds_read_b128 per 16 evaluations = 7.1
#   query route, 4 queries per thread, argmin (cm_scan<4, true>):  136 VALU (64 packed) + 3 ds_read_b128 per 16 evaluations = 8.5
#   surface route / 1 query per thread, argmin (cm_scan<1, true>):  45 VALU (8 packed)  + 3 ds_read_b128 per  4 evaluations = 11.3
# at 7.1 instructions per evaluation the device's 256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz = 39.3 T lane-instructions/s bound the forward at 5.5 T evaluations/s
"""


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def first_point_padding(X, counts):
    """rows at or beyond a cloud's count replaced by the cloud's first point: no minimum over the cloud changes, and an argmin tie with
    the copy goes to the original (the lowest index)"""
    keep = torch.arange(X.shape[1], device=X.device)[None, :] < counts[:, None]
    return torch.where(keep[..., None], X, X[:, :1].expand_as(X)).contiguous()


def _idx(arg):
    return arg.long()[..., None].expand(-1, -1, 3)


def terms(a, b, arg_a, arg_b, wa, wb, mask_a, mask_b, stats=False):
    """the gradient of sum_p ( wa_p sum_n mask_a min_a[p,n] + wb_p sum_m mask_b min_b[p,m] ) w.r.t. the expanded pairs a [P,N,3], b [P,M,3]
    through the argmins; stats: also the sum of the absolute terms and the number of terms per element (float64 evaluation)"""
    ta = 2 * wa[:, None, None] * (a - torch.gather(b, 1, _idx(arg_a))) * mask_a[..., None]
    tb = 2 * wb[:, None, None] * (b - torch.gather(a, 1, _idx(arg_b))) * mask_b[..., None]
    da = ta.clone().scatter_add_(1, _idx(arg_b), -tb)
    db = tb.clone().scatter_add_(1, _idx(arg_a), -ta)
    if not stats:
        return da, db
    Sa = ta.abs().scatter_add_(1, _idx(arg_b), tb.abs())
    Sb = tb.abs().scatter_add_(1, _idx(arg_a), ta.abs())
    ma, mb = mask_a.to(a.dtype), mask_b.to(a.dtype)
    Ta = ma.clone().scatter_add_(1, arg_b.long(), mb)
    Tb = mb.clone().scatter_add_(1, arg_a.long(), ma)
    return da, db, Sa, Sb, Ta, Tb


class Expanded:
    """the route of the parent commit; `rows` rows of the matrix (rows * Cb pairs) per call of the paired entry"""

    def __init__(self, A, B, cA, cB, rows=8):
        self.lib = L.load()
        self.ragged = cA is not None
        self.Ca, self.N, self.Cb, self.M = A.shape[0], A.shape[1], B.shape[0], B.shape[1]
        dev = A.device
        self.nA = torch.full((self.Ca,), self.N, device=dev, dtype=torch.int32) if cA is None else cA
        self.nB = torch.full((self.Cb,), self.M, device=dev, dtype=torch.int32) if cB is None else cB
        self.A = first_point_padding(A, self.nA) if self.ragged else A.contiguous()
        self.B = first_point_padding(B, self.nB) if self.ragged else B.contiguous()
        self.maskA = torch.arange(self.N, device=dev)[None, :] < self.nA[:, None]
        self.maskB = torch.arange(self.M, device=dev)[None, :] < self.nB[:, None]
        self.rows = rows

    def batches(self):
        for i0 in range(0, self.Ca, self.rows):
            r = min(self.rows, self.Ca - i0)
            P = r * self.Cb
            a = self.A[i0:i0 + r].repeat_interleave(self.Cb, 0)                  # the staging the matrix entry does away with
            b = self.B.repeat(r, 1, 1)
            dev = a.device
            min_a, min_b = torch.empty(P, self.N, device=dev), torch.empty(P, self.M, device=dev)
            arg_a, arg_b = torch.empty(P, self.N, device=dev, dtype=torch.int32), torch.empty(P, self.M, device=dev, dtype=torch.int32)
            loss = torch.empty(1, device=dev)
            L.check(self.lib.dpd_chamfer_fwd(L.ptr(a), L.ptr(b), P, self.N, self.M, L.ptr(min_a), L.ptr(arg_a), L.ptr(min_b), L.ptr(arg_b),
                                             L.ptr(loss), L.cur_stream()), "dpd_chamfer_fwd")
            mask_a = self.maskA[i0:i0 + r].repeat_interleave(self.Cb, 0)
            mask_b = self.maskB.repeat(r, 1)
            yield i0, r, P, a, b, min_a, min_b, arg_a, arg_b, mask_a, mask_b

    def means(self, i0, r, min_a, min_b, mask_a, mask_b, dtype=torch.float32):
        """(D_AB, D_BA) [r, Cb] of one batch: min_b belongs to the queries of B against surface A, min_a to the other direction"""
        nA = self.nA[i0:i0 + r].repeat_interleave(self.Cb).to(dtype)
        nB = self.nB.repeat(r).to(dtype)
        if self.ragged or dtype != torch.float32:
            d_ba = (min_a.to(dtype) * mask_a).sum(1) / nA
            d_ab = (min_b.to(dtype) * mask_b).sum(1) / nB
        else:
            d_ba, d_ab = min_a.mean(1), min_b.mean(1)
        return d_ab.view(r, self.Cb), d_ba.view(r, self.Cb)

    def forward(self):
        D = torch.empty(self.Ca, self.Cb, device=self.A.device)
        for i0, r, P, a, b, min_a, min_b, arg_a, arg_b, mask_a, mask_b in self.batches():
            d_ab, d_ba = self.means(i0, r, min_a, min_b, mask_a, mask_b)
            D[i0:i0 + r] = (d_ab + d_ba) / 2
        return D

    def forward_backward(self, G):
        """-> (D, dA, dB) under the upstream G on D"""
        D = torch.empty(self.Ca, self.Cb, device=self.A.device)
        dA, dB = torch.empty_like(self.A), torch.zeros_like(self.B)
        for i0, r, P, a, b, min_a, min_b, arg_a, arg_b, mask_a, mask_b in self.batches():
            d_ab, d_ba = self.means(i0, r, min_a, min_b, mask_a, mask_b)
            D[i0:i0 + r] = (d_ab + d_ba) / 2
            g = G[i0:i0 + r].reshape(P)
            if self.ragged:
                nA = self.nA[i0:i0 + r].repeat_interleave(self.Cb).float()
                da, db = terms(a, b, arg_a, arg_b, g / (2 * nA), g / (2 * self.nB.repeat(r).float()), mask_a, mask_b)
            else:
                da, db = torch.empty_like(a), torch.empty_like(b)
                L.check(self.lib.dpd_chamfer_bwd(L.ptr(a), L.ptr(b), P, self.N, self.M, L.ptr(arg_a), L.ptr(arg_b), 1.0, L.ptr(da), L.ptr(db),
                                                 L.cur_stream()), "dpd_chamfer_bwd")
                scale = (g * P)[:, None, None]              # the entry weighs every pair 1 / P; pair p's gradient touches pair p alone
                da, db = da * scale, db * scale
            dA[i0:i0 + r] = da.view(r, self.Cb, self.N, 3).sum(1)
            dB += db.view(r, self.Cb, self.M, 3).sum(0)
        return D, dA, dB

    def float64(self, G):
        """float64 on the device through the stored argmins -> D, n (the larger count of each pair), and per set (g, S, T)"""
        f = torch.float64
        D = torch.empty(self.Ca, self.Cb, device=self.A.device, dtype=f)
        sets = [[torch.zeros(*self.A.shape[:2], k, device=self.A.device, dtype=f) for k in (3, 3, 1)],
                [torch.zeros(*self.B.shape[:2], k, device=self.A.device, dtype=f) for k in (3, 3, 1)]]
        for i0, r, P, a, b, min_a, min_b, arg_a, arg_b, mask_a, mask_b in self.batches():
            d_ab, d_ba = self.means(i0, r, min_a, min_b, mask_a, mask_b, f)
            D[i0:i0 + r] = (d_ab + d_ba) / 2
            g = G[i0:i0 + r].reshape(P).to(f)
            nA = self.nA[i0:i0 + r].repeat_interleave(self.Cb).to(f)
            da, db, Sa, Sb, Ta, Tb = terms(a.to(f), b.to(f), arg_a, arg_b, g / (2 * nA), g / (2 * self.nB.repeat(r).to(f)), mask_a, mask_b, True)
            for k, (xa, xb) in enumerate(((da, db), (Sa, Sb), (Ta[..., None], Tb[..., None]))):
                sets[0][k][i0:i0 + r] = xa.view(r, self.Cb, self.N, -1).sum(1)
                sets[1][k] += xb.view(r, self.Cb, self.M, -1).sum(0)
        n = torch.maximum(self.nA[:, None], self.nB[None, :]).to(f)
        return D, n, sets


def check_grad(name, got, ref, c):
    g, S, T = ref
    bar = (T + c) * U * S
    err = (got.double() - g).abs()
    if not bool((err <= bar).all()) or not bool((got[(S == 0).expand_as(got)] == 0).all()):
        raise SystemExit("%s: a gradient element misses its bar (T + %d) u S: worst error / bar %.3f"
                         % (name, c, float((err / bar.clamp_min(1e-300)).max())))
    return float((err / bar.clamp_min(1e-300)).max())


EMD_SHAPES = ((32, 64), (16, 256), (8, 1024), (4, 2048))


class ExpandedEMD:
    """the route of the parent commit: every pair as a batch entry of dpd_emd_fwd"""

    def __init__(self, A, B):
        self.lib, self.A, self.B = L.load(), A, B
        self.C, self.N = A.shape[0], A.shape[1]
        self.P = self.C * self.C
        dev = A.device
        self.ws = torch.empty(self.lib.dpd_emd_workspace_bytes(self.P, self.N, self.N), device=dev, dtype=torch.uint8)
        self.cost, self.loss = torch.empty(self.P, device=dev), torch.empty(1, device=dev)
        self.copy_ms = []

    def copies(self):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        a = self.A.repeat_interleave(self.C, 0)
        b = self.B.repeat(self.C, 1, 1)
        e1.record()
        self.copy_ms.append((e0, e1))
        return a, b

    def run(self, a, b, g1, g2):
        # gscale = P N: the gradients of cost[p] itself, not of the batch mean
        L.check(self.lib.dpd_emd_fwd(L.ptr(a), L.ptr(b), self.P, self.N, self.N, float(self.P * self.N), L.ptr(self.cost), L.ptr(self.loss),
                                     L.ptr(g1), L.ptr(g2), None, L.ptr(self.ws), self.ws.numel(), L.cur_stream()), "dpd_emd_fwd")
        return (self.cost / self.N).view(self.C, self.C)

    def forward(self):
        a, b = self.copies()
        return self.run(a, b, None, None)

    def forward_backward(self, G, stats=False):
        a, b = self.copies()
        g1, g2 = torch.empty_like(a), torch.empty_like(b)
        D = self.run(a, b, g1, g2)
        w = (G / self.N)[:, :, None, None]
        t1, t2 = g1.view(self.C, self.C, self.N, 3) * w, g2.view(self.C, self.C, self.N, 3) * w
        if stats:
            return D, t1.sum(1), t2.sum(0), t1.abs().sum(1), t2.abs().sum(0)
        return D, t1.sum(1), t2.sum(0)

    def take_copy_ms(self):
        ms = [e0.elapsed_time(e1) for e0, e1 in self.copy_ms]
        self.copy_ms = []
        return ms


def emd_main(a):
    from dpdist_amd import EMDMatrix, emd_matrix
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(12)
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "shapes": {}}
    lines = ["# tools/baseline_matrix_bench.py --emd --rounds %d" % a.rounds,
             "# device: %s; Earth Mover's distance of every pair, full sets; ms per call (in-stream device event pairs), median [min .. max] of %d"
             % (res["device"], a.rounds),
             "# alternating calls after 2 warm-up calls.  matrix: emd_matrix / EMDMatrix (one launch, one workgroup per pair; forward+backward:",
             "# loss = (G * D).sum(), random G).  expanded: the pairs copied into [Ca * Cb, n, 3] batches and sent through dpd_emd_fwd; its time",
             "# includes the copies, whose share is shown as `copies`.", ""]
    mod = EMDMatrix()
    for C, N in EMD_SHAPES:
        A = torch.tensor(rng.uniform(-0.8, 0.8, (C, N, 3)).astype(np.float32), device=dev)
        B = torch.tensor(rng.uniform(-0.8, 0.8, (C, N, 3)).astype(np.float32), device=dev)
        G = torch.tensor(rng.standard_normal((C, C)).astype(np.float32), device=dev)
        ex = ExpandedEMD(A, B)

        def matrix_fb():
            x, y = A.detach().requires_grad_(True), B.detach().requires_grad_(True)
            D = mod(x, y)
            (G * D).sum().backward()
            return D.detach(), x.grad, y.grad

        f = {"matrix": (lambda: emd_matrix(A, B), matrix_fb), "expanded": (ex.forward, lambda: ex.forward_backward(G))}
        # agreement, before anything is timed
        Dm, gAm, gBm = matrix_fb()
        De, gAe, gBe, SA, SB = ex.forward_backward(G, stats=True)
        torch.cuda.synchronize()
        for label, D in (("matrix", Dm), ("matrix forward", f["matrix"][0]()), ("expanded forward", f["expanded"][0]())):
            if not torch.equal(D, De):
                raise SystemExit("%d x %d x %d: D of %s and of the expanded route differ in bits" % (C, C, N, label))
        worst = 0.0
        for label, got, ref, S in (("dA", gAm, gAe, SA), ("dB", gBm, gBe, SB)):
            bar = 4 * (C + 4) * U * S
            err = (got.double() - ref.double()).abs()
            if not bool((err <= bar).all()):
                raise SystemExit("%d x %d x %d: %s of the two routes differ by more than 4 (C + 4) u S" % (C, C, N, label))
            worst = max(worst, float((err / bar.clamp_min(1e-300)).max()))
        ex.take_copy_ms()
        name = "%dx%dx%d" % (C, C, N)
        lines.append("%s: Ca = Cb = %d, n = m = %d; D the same bits on both routes, gradients within %.3f of 4 (C + 4) u S of each other" % (name, C, N, worst))
        shape = res["shapes"][name] = {"grad_difference_over_bar": worst}
        for k, what in ((0, "forward"), (1, "forward+backward")):
            for _ in range(2):
                f["matrix"][k](), f["expanded"][k]()
            torch.cuda.synchronize()
            ex.take_copy_ms()
            t = {"matrix": [], "expanded": []}
            for _ in range(a.rounds):
                for route in ("matrix", "expanded"):
                    t[route].append(timed(f[route][k]))
            copies = float(np.median(ex.take_copy_ms()))
            med = {route: float(np.median(v)) for route, v in t.items()}
            ratio = med["expanded"] / med["matrix"]
            win = "matrix" if ratio > 1 else "expanded"
            shape[what] = {"matrix_ms": round(med["matrix"], 4), "expanded_ms": round(med["expanded"], 4), "expanded_copies_ms": round(copies, 4),
                           "expanded_over_matrix": round(ratio, 2), "winner": win}
            lines.append("    %-17s matrix %9.3f [%9.3f .. %9.3f]   expanded %9.3f [%9.3f .. %9.3f] (copies %7.3f)   expanded / matrix %6.2f   -> %s wins"
                         % (what, med["matrix"], min(t["matrix"]), max(t["matrix"]), med["expanded"], min(t["expanded"]), max(t["expanded"]), copies,
                            ratio, win))
        lines.append("")
    text = "\n".join(lines)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)
    print(text)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--emd", action="store_true", help="time the all-pairs Earth Mover's distance instead (see the module docstring)")
    ap.add_argument("--clouds", type=int, default=64)
    ap.add_argument("--points", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--rows", type=int, default=8, help="rows of the matrix per call of the paired entry (expanded route)")
    ap.add_argument("--out", default=None, help="the record; default profiles/baseline_matrix_bench.txt, with --emd profiles/emd_matrix_bench.txt")
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                             "emd_matrix_bench.txt" if a.emd else "baseline_matrix_bench.txt")
    if a.emd:
        return emd_main(a)
    dev = torch.device("cuda:0")
    C, N = a.clouds, a.points
    rng = np.random.default_rng(12)
    A = torch.tensor(rng.uniform(-0.9, 0.9, (C, N, 3)).astype(np.float32), device=dev)
    B = torch.tensor(rng.uniform(-0.9, 0.9, (C, N, 3)).astype(np.float32), device=dev)
    G = torch.tensor(rng.standard_normal((C, C)).astype(np.float32), device=dev)
    res = {"device": torch.cuda.get_device_name(0), "Ca": C, "Cb": C, "N": N, "M": N, "rounds": a.rounds, "rows_per_batch": a.rows, "shapes": {}}
    lines = ["# tools/baseline_matrix_bench.py --clouds %d --points %d --rounds %d --rows %d" % (C, N, a.rounds, a.rows),
             "# device: %s; squared Chamfer; ms per call (in-stream device event pairs), median [min .. max] of %d alternating calls after 2 warm-up calls"
             % (res["device"], a.rounds),
             "# Geval/s: point-pair evaluations of the FORWARD of both directions, 2 sum_ij nA_i nB_j, per second of the call (the matrix route's",
             "# backward scans every pair twice more, once per route; the expanded route scans its padded widths)", ""]
    mod = ChamferMatrix("squared")
    for name, ragged in (("full", False), ("ragged", True)):
        cA = cB = None
        if ragged:
            cA, cB = (torch.tensor(rng.integers(N // 4, N + 1, size=C), dtype=torch.int32, device=dev) for _ in range(2))
        ex = Expanded(A, B, cA, cB, a.rows)
        evals = 2.0 * float(ex.nA.double().sum() * ex.nB.double().sum())

        def matrix_fb():
            x, y = A.detach().requires_grad_(True), B.detach().requires_grad_(True)
            D = mod(x, y, countsA=cA, countsB=cB)
            (G * D).sum().backward()
            return D.detach(), x.grad, y.grad

        f = {"matrix": (lambda: chamfer_matrix(A, B, countsA=cA, countsB=cB), matrix_fb), "expanded": (ex.forward, lambda: ex.forward_backward(G))}
        # agreement, before anything is timed
        D64, n, (refA, refB) = ex.float64(G)
        Dm, gAm, gBm = f["matrix"][1]()
        De, gAe, gBe = f["expanded"][1]()
        torch.cuda.synchronize()
        for label, D in (("matrix", Dm), ("expanded", De), ("matrix forward", f["matrix"][0]()), ("expanded forward", f["expanded"][0]())):
            if not bool(((D.double() - D64).abs() <= (n + 3) * U * D64).all()):
                raise SystemExit("%s, %s: D misses its bar against float64" % (name, label))
        if not bool(((Dm.double() - De.double()).abs() <= 2 * (n + 3) * U * D64).all()):
            raise SystemExit("%s: the two routes disagree on D" % name)
        keepA, keepB = ex.maskA[..., None], ex.maskB[..., None]
        worst = {"matrix": max(check_grad(name + ", matrix dA", gAm, refA, 4), check_grad(name + ", matrix dB", gBm, refB, 4)),
                 "expanded": max(check_grad(name + ", expanded dA", gAe * keepA, refA, 8), check_grad(name + ", expanded dB", gBe * keepB, refB, 8))}
        lines.append("%s: Ca = Cb = %d, N = M = %d%s; %.3f G evaluations per forward" % (
            name, C, N, ", counts uniform in [%d, %d] (mean %.1f, %.1f)" % (N // 4, N, float(ex.nA.float().mean()), float(ex.nB.float().mean()))
            if ragged else ", no counts", evals / 1e9))
        lines.append("    agreement: D of both routes within (max(n_ab, n_ba) + 3) u of float64; gradients, worst error / bar: matrix %.3f of (T + 4) u S, "
                     "expanded %.3f of (T + 8) u S" % (worst["matrix"], worst["expanded"]))
        shape = res["shapes"][name] = {"evaluations_per_forward": evals, "grad_error_over_bar": worst}
        for k, what in ((0, "forward"), (1, "forward+backward")):
            for _ in range(2):
                f["matrix"][k](), f["expanded"][k]()
            t = {"matrix": [], "expanded": []}
            for _ in range(a.rounds):
                for route in ("matrix", "expanded"):
                    t[route].append(timed(f[route][k]))
            med = {route: float(np.median(v)) for route, v in t.items()}
            ratio = med["expanded"] / med["matrix"]
            win = "matrix" if ratio > 1 else "expanded"
            shape[what] = {"matrix_ms": round(med["matrix"], 4), "expanded_ms": round(med["expanded"], 4), "expanded_over_matrix": round(ratio, 2),
                           "matrix_geval_per_s": round(evals / med["matrix"] / 1e6, 1), "expanded_geval_per_s": round(evals / med["expanded"] / 1e6, 1),
                           "winner": win}
            lines.append("    %-17s matrix %9.3f [%9.3f .. %9.3f] %8.1f Geval/s   expanded %9.3f [%9.3f .. %9.3f] %8.1f Geval/s   expanded / matrix %6.2f   -> %s wins"
                         % (what, med["matrix"], min(t["matrix"]), max(t["matrix"]), evals / med["matrix"] / 1e6, med["expanded"], min(t["expanded"]),
                            max(t["expanded"]), evals / med["expanded"] / 1e6, ratio, win))
        lines.append("")
    text = "\n".join(lines) + "\n" + ISA_NOTE
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)
    print(text)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The 3DmFV encoder's plain and tiled entries side by side (in-stream event pairs around every call, median over --reps calls after
--warmup; the forms of one shape alternate inside the timed loop).  GPU only.

    python tools/encoder_bench.py [--clouds 32] [--m 8] [--reps 200] [--warmup 20]

N = 704: dpd_mfv3d_fwd / dpd_mfv3d_bwd (sliced) against dpd_mfv3d_fwd_tiled / dpd_mfv3d_bwd_tiled at their default tile -- the plain
entry of the same process is the yardstick for what tiling costs.  N = 1024, 2048: tiled only (the plain forward refuses them).
Two more figures split a difference to the plain forward into "another kernel" and "rebuilding the tables per tile": N = 704 with
tile 704 (ONE tile: the tiled kernel without any rebuild), and N = 705, where the plain entry runs the eight-point-group kernel the
tiled one is built on (N = 704 runs the kernel that takes the points in pairs on the packed VALU).  Also the largest difference
between the forms' results (random clouds, not the admitted cases of the tests: an fv entry near 0 amplifies the last bits of its
statistic through the power-1/2 normalisation; the upstream gradient is zeroed where |fv| < 2e-3, as in the tests).  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, default=32)
    ap.add_argument("--m", type=int, default=8)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("encoder_bench needs a GPU")
    from dpdist_amd import lib as L
    lib, dev = L.load(), torch.device("cuda:0")
    C, m, sigma, G = a.clouds, a.m, 0.125, a.m ** 3
    s = L.cur_stream()
    ws = torch.empty(lib.dpd_mfv3d_bwd_workspace_bytes(C, m) // 4, device=dev)
    out = {"clouds": C, "m": m, "reps": a.reps, "tile_fwd": lib.dpd_mfv3d_tile(m, 0), "tile_bwd": lib.dpd_mfv3d_tile(m, 1), "shapes": {}}

    def timed(forms):
        """forms: {name: fn}; the forms alternate call by call; -> {name: median us}"""
        for _ in range(a.warmup):
            for fn in forms.values():
                fn()
        ev = {n: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.reps)] for n in forms}
        torch.cuda.synchronize()
        for r in range(a.reps):
            for n, fn in forms.items():
                e0, e1 = ev[n][r]
                e0.record()
                fn()
                e1.record()
        torch.cuda.synchronize()
        return {n: round(statistics.median(e0.elapsed_time(e1) for e0, e1 in ev[n]) * 1e3, 2) for n in forms}

    for N in (704, 705, 1024, 2048):
        rng = np.random.default_rng([3, N])
        pts = torch.tensor(rng.uniform(-0.8, 0.8, size=(C, N, 3)).astype(np.float32), device=dev)
        dfv = torch.tensor(rng.standard_normal((C, G, 20)).astype(np.float32), device=dev)
        fv = {n: torch.empty(C, G, 20, device=dev) for n in ("plain", "tiled", "one_tile")}
        g = {n: torch.empty(C, N, 3, device=dev) for n in ("plain", "tiled")}
        plain = bool(lib.dpd_mfv3d_fits(N, m, 0)) and bool(lib.dpd_mfv3d_fits(N, m, 2))

        def fwd_tiled(tile, o):
            return lambda: L.check(lib.dpd_mfv3d_fwd_tiled(L.ptr(pts), C, N, m, sigma, tile, L.ptr(o), s), "dpd_mfv3d_fwd_tiled")

        fwd = {"tiled": fwd_tiled(0, fv["tiled"])}
        bwd = {"tiled": lambda: L.check(lib.dpd_mfv3d_bwd_tiled(L.ptr(pts), L.ptr(dfv), C, N, m, sigma, 0, L.ptr(g["tiled"]), L.ptr(ws),
                                                                ws.numel() * 4, s), "dpd_mfv3d_bwd_tiled")}
        if plain:
            fwd["plain"] = lambda: L.check(lib.dpd_mfv3d_fwd(L.ptr(pts), C, N, m, sigma, L.ptr(fv["plain"]), s), "dpd_mfv3d_fwd")
            if N % 8 == 0:
                fwd["one_tile"] = fwd_tiled(N, fv["one_tile"])
            bwd["plain"] = lambda: L.check(lib.dpd_mfv3d_bwd(L.ptr(pts), L.ptr(dfv), C, N, m, sigma, L.ptr(g["plain"]), L.ptr(ws),
                                                             ws.numel() * 4, s), "dpd_mfv3d_bwd")
        rec = {"forward_us": timed(fwd)}
        dfv.mul_((fv["tiled"].abs() > 2e-3).float())      # as the tests do: the power-1/2 normalisation has no bounded gradient at fv = 0
        rec["backward_us"] = timed(bwd)
        if plain:
            rec["forward_max_abs_diff"] = float((fv["tiled"] - fv["plain"]).abs().max())
            rec["backward_max_abs_diff_over_scale"] = float((g["tiled"] - g["plain"]).abs().max() / max(1.0, float(g["plain"].abs().max())))
        out["shapes"][str(N)] = rec
    print(json.dumps(out))


if __name__ == "__main__":
    main()

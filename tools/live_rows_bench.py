"""Cross-over of the live-row backward (trainer option `live_rows`): the exact-fp32 training step with the option on and off,
alternating, on two inputs --
    bench      the recipe of bench.py (seed-1234 weights, lr 1e-4): after the warm-up about 30 % of the rows carry gradient;
    all_live   the same clouds with the output bias shifted to 3 (0 < y0 < 6 on every row) and the learning rate at its floor, so that
               every row inside the cube stays live: what the compaction launch, the partial-sum launch and the smaller dH tiles COST
               when there is nothing to leave out.
Each line: input, form, ms per step (host clock around `steps` steps that end in a synchronise) and the live count {L, Lp} read back
AFTER the timed window (the step itself never reads it).
--pair alternates the option `live_pair` instead (live rows on in both forms): the five-launch live backward against the one whose dH
products share a launch with a weight gradient; on all_live the dH part of a pair has all its workgroups.
    python tools/live_rows_bench.py [--batch 32] [--steps 200] [--warmup 220] [--reps 3] [--pair]"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dpdist_amd import synth                              # noqa: E402
from dpdist_amd.model import DPDistParams                 # noqa: E402
from dpdist_amd.trainer import DPDistTrainer              # noqa: E402


def run(dev, B, N, kind, on, steps, warmup, batch, pair=False):
    P = DPDistParams(k=5, mlp=(1024, 1024, 1024), device=dev, compute_dtype="f32")
    P.reset_parameters_tf(generator=torch.Generator().manual_seed(1234))
    lr = 1e-4
    if kind == "all_live":
        P.view("b4").add_(3.0)
        lr = 1e-7
    tr = DPDistTrainer(P, B, num_point=N, Embedding_Size=512, sigma3dmfv=0.125, base_lr=lr, distributed=False,
                       options={"live_pair": on} if pair else {"live_rows": None if on else False})
    assert (tr.live_pair if pair else tr.live_rows) == on
    for _ in range(warmup):
        tr.step(*batch)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        tr.step(*batch)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    count = tr.live_count.cpu().tolist() if (on or pair) else None
    return ms, count, float(tr.loss.cpu()[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=220)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--pair", action="store_true", help="alternate live_pair (live rows on) instead of live_rows")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("live_rows_bench needs a GPU")
    dev = torch.device("cuda:0")
    B, N = a.batch, 64
    batch = tuple(torch.tensor(x, device=dev) for x in synth.s2_modelnet_shaped(B, N, 100))
    for kind in ("bench", "all_live"):
        for rep in range(a.reps):
            for on in (False, True):
                ms, count, loss = run(dev, B, N, kind, on, a.steps, a.warmup, batch, a.pair)
                print("%-9s %s=%-5s rep %d  %.4f ms/step  live {L, Lp} = %s of %d  loss_samples %.6f"
                      % (kind, "live_pair" if a.pair else "live_rows", on, rep, ms, count, B * N, loss), flush=True)


if __name__ == "__main__":
    main()

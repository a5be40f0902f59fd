"""Fit the implicit surface on many labelled queries per cloud through the per-point field with decoder gradients
(dpdist_amd.DPDistField(backward="slots", decoder_grad=True)): what the label files of `python -m dpdist_amd.dataset` are for, with
more than the 64 queries per cloud of the reference's training step.

    python tools/field_fit_demo.py [--clouds 8] [--points 256] [--queries 1024] [--width 256] [--steps 50] [--lr 1e-4] [--log-every 5]

Synthetic shapes (dpdist_amd.synth.s2_modelnet_shaped: spheres and boxes), M queries per cloud uniform in the cube, labels = the nearest
distance to the cloud's points (dpdist_amd.dataset.nn_distance, on the GPU), loss = mean |pred[..., 0] - label| over the queries inside the
cube, TFAdam on model.params_.flat.  The decoder starts from the Xavier initialisation of the reference.  Writes ONE JSON line with the
L1 at every logged step."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dpdist_amd import DPDistField, synth  # noqa: E402
from dpdist_amd.dataset import nn_distance  # noqa: E402
from dpdist_amd.model import DPDistModel  # noqa: E402
from dpdist_amd.optim import TFAdam  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, default=8)
    ap.add_argument("--points", type=int, default=256)
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--width", type=int, default=256)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--log-every", type=int, default=5)
    ap.add_argument("--max-rows", type=int, default=16384)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    C, M, H = a.clouds, a.queries, a.width
    model = DPDistModel(Embedding_Size=512, k=5, localSNmlp=(H,) * 3, sigma3dmfv=0.125, device=dev)
    model.load_tf_state_dict(synth.make_weights("xavier_tf", mlp=(H,) * 3))
    S = torch.tensor(synth.s2_modelnet_shaped(C, a.points, 100 + a.seed)[0], device=dev)
    Q = torch.tensor(np.random.default_rng([a.seed, M]).uniform(-1.0, 1.0, (C, M, 3)).astype(np.float32), device=dev)
    labels = nn_distance(S, Q)                                                  # [C, M]
    field = DPDistField(model, max_rows=a.max_rows, backward="slots", decoder_grad=True)
    opt = TFAdam([model.params_.flat], lr=a.lr)
    log = []
    for step in range(a.steps + 1):
        opt.zero_grad()
        pred, mask = field(S, Q, return_mask=True)
        loss = ((pred[..., 0] - labels).abs() * mask).sum() / mask.sum()
        if step % a.log_every == 0 or step == a.steps:
            log.append({"step": step, "l1": round(float(loss.detach()), 6)})
        if step < a.steps:
            loss.backward()
            opt.step()
    print(json.dumps({"device": torch.cuda.get_device_name(0), "clouds": C, "points": a.points, "queries": M, "H": H, "lr": a.lr,
                      "max_rows": a.max_rows, "log": log}))


if __name__ == "__main__":
    main()

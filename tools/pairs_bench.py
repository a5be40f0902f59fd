"""The per-pair distances of two sets of clouds of different sizes (dpdist_amd.dpdist_pairs / DPDistPairs) against the only route there
was before them, the diagonal of the all-pairs matrix on the same inputs, at decoder width 1024 on synth.s2_modelnet_shaped clouds:

    pairs    dpdist_pairs: B (Wa + Wb) decoder rows                    forward+backward: DPDistPairs, loss = (G * D).sum()
    matrix   dpdist_matrix(...).diagonal(): B^2 (Wa + Wb) decoder rows    forward+backward: DPDistMatrix, the same loss on its diagonal

at two shapes:

    rectangular   B = 16, Wa = 1024, Wb = 64, no counts (the matrix takes two widths only with counts: it gets full ones)
    ragged        B = 16, Wa = Wb = 256, counts uniform in [64, 256]

    python tools/pairs_bench.py [--out profiles/pairs_bench.txt]

The two forms alternate, `--rounds` calls after two warm-up calls, each timed with an in-stream device event pair; the distances of the
two forms must agree within the fp32 forward bar of the tests (1e-4 absolute), the gradients within the input-gradient bar.  No threshold
is set on the times."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dpdist_amd import DPDistMatrix, DPDistPairs, dpdist_matrix, dpdist_pairs, synth  # noqa: E402
from dpdist_amd.model import DPDistModel  # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def forms(model, A, B, cA, cB, max_rows):
    """{name: (forward, forward + backward)} of the two routes; the matrix always gets counts (full ones where the set has none)"""
    dev = A.device
    nb = A.shape[0]
    G = torch.tensor(np.random.default_rng(7).standard_normal(nb).astype(np.float32), device=dev)
    full = lambda t: torch.full((nb,), t.shape[1], dtype=torch.int32, device=dev)   # noqa: E731
    mA, mB = (full(A) if cA is None else cA), (full(B) if cB is None else cB)
    pairs_mod, matrix_mod = DPDistPairs(model, max_rows=max_rows), DPDistMatrix(model, max_rows=max_rows)

    def grads(fn):
        a, b = A.detach().requires_grad_(True), B.detach().requires_grad_(True)
        (G * fn(a, b)).sum().backward()
        return a.grad, b.grad

    return {"pairs": (lambda: dpdist_pairs(model, A, B, cA, cB, max_rows=max_rows),
                      lambda: grads(lambda a, b: pairs_mod(a, b, countsA=cA, countsB=cB))),
            "matrix": (lambda: dpdist_matrix(model, A, B, max_rows=max_rows, countsA=mA, countsB=mB).diagonal(),
                       lambda: grads(lambda a, b: matrix_mod(a, b, countsA=mA, countsB=mB).diagonal()))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=16)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--max-rows", type=int, default=16384)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "pairs_bench.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    nb, H = a.pairs, a.width
    model = DPDistModel(Embedding_Size=512, k=5, localSNmlp=(H,) * 3, sigma3dmfv=0.125, device=dev)
    model.load_tf_state_dict(synth.make_weights("wide", mlp=(H,) * 3))
    for prm in model.parameters():
        prm.requires_grad_(False)
    rng = np.random.default_rng(9)
    res = {"device": torch.cuda.get_device_name(0), "H": H, "m": 8, "k": 5, "max_rows": a.max_rows, "rounds": a.rounds, "shapes": {}}
    lines = ["# tools/pairs_bench.py --pairs %d --width %d --rounds %d --max-rows %d" % (nb, H, a.rounds, a.max_rows),
             "# device: %s; exact fp32; ms per call (in-stream device event pairs), median [min .. max] of %d alternating calls after 2 warm-up calls"
             % (res["device"], a.rounds), ""]
    for name, Wa, Wb, ragged in (("rectangular", 1024, 64, False), ("ragged", 256, 256, True)):
        A = torch.tensor(synth.s2_modelnet_shaped(nb, Wa, 100)[0], device=dev)
        B = torch.tensor(synth.s2_modelnet_shaped(nb, Wb, 101)[1], device=dev)
        cA = cB = None
        if ragged:
            cA, cB = (torch.tensor(rng.integers(Wa // 4, Wa + 1, size=nb), dtype=torch.int32, device=dev) for _ in range(2))
        f = forms(model, A, B, cA, cB, a.max_rows)
        lines.append("%s: B = %d, Wa = %d, Wb = %d%s; decoder rows per call: pairs %d, matrix %d"
                     % (name, nb, Wa, Wb, ", counts uniform in [%d, %d] (mean %.1f, %.1f)" % (Wa // 4, Wa, float(cA.float().mean()), float(cB.float().mean()))
                        if ragged else ", no counts", nb * (Wa + Wb), nb * nb * (Wa + Wb)))
        shape = res["shapes"][name] = {"B": nb, "Wa": Wa, "Wb": Wb, "ragged": ragged}
        for k, what in ((0, "forward"), (1, "forward+backward")):
            got, want = f["pairs"][k](), f["matrix"][k]()
            torch.cuda.synchronize()
            outs = zip((got,), (want,)) if k == 0 else zip(got, want)
            err = [float((x.double() - y.double()).abs().max()) for x, y in outs]
            scale = 1.0 if k == 0 else max(1.0, max(float(x.abs().max()) for x in want))
            if max(err) > (1e-4 if k == 0 else 4e-4 * scale):
                raise SystemExit("%s, %s: the two routes disagree: %s" % (name, what, err))
            f["pairs"][k](), f["matrix"][k]()
            t = {"pairs": [], "matrix": []}
            for _ in range(a.rounds):
                for form in ("pairs", "matrix"):
                    t[form].append(timed(f[form][k]))
            med = {form: float(np.median(v)) for form, v in t.items()}
            ratio = med["matrix"] / med["pairs"]
            shape[what] = {"pairs_ms": round(med["pairs"], 4), "matrix_diagonal_ms": round(med["matrix"], 4), "ratio": round(ratio, 2),
                           "max_abs_diff": max(err)}
            lines.append("    %-17s pairs %9.3f [%9.3f .. %9.3f]   matrix diagonal %9.3f [%9.3f .. %9.3f]   ratio %6.2f   max |difference| %.2e"
                         % (what, med["pairs"], min(t["pairs"]), max(t["pairs"]), med["matrix"], min(t["matrix"]), max(t["matrix"]), ratio, max(err)))
        lines.append("")
    text = "\n".join(lines)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)
    print(text)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

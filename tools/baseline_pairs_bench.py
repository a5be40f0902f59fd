"""The baselines per pair on ragged batches (dpdist_amd.chamfer_pairs / ChamferPairs, emd_pairs / EMDPairs) against the two routes there
were before them:

    pairs    chamfer_pairs / emd_pairs(A, B, countsA=, countsB=)            forward+backward: ChamferPairs / EMDPairs, loss = (G * D).sum()
    diag     chamfer_matrix / emd_matrix(...).diagonal(), the same counts   forward+backward: ChamferMatrix / EMDMatrix, the same loss on the
             (P times the distance evaluations)                             diagonal
    paired   full sets only: aue.chamfer_dist (squared), regtest.chamfer_sqrt (sqrt), emd.earth_mover -- the batch mean, their own nodes;
             forward+backward: loss.backward()

and, for the Earth Mover's distance, the two forms of the library against each other: form 1 (one launch, a workgroup per pair) and form 2
(a launch per pass, a workgroup per 64-point tile of a pair); `pairs` is the library's choice between them.

    python tools/baseline_pairs_bench.py [--out profiles/baseline_pairs_bench.txt]

at P = 16 pairs of width 64, 256, 1024, 2048 (Chamfer also 4096), each width full (no counts) and ragged (counts uniform in [W / 4, W],
fixed seed).  The routes alternate, `--rounds` calls after two warm-up calls, each timed with an in-stream device event pair.  Before a
shape is timed `pairs` is held to the yardstick: D has to equal the diagonal of the matrix and both gradients those of the matrix
module under the same upstream on its diagonal, value for value (they are the same bits per pair; the matrix adds exact zeros for the
other pairs), the two EMD forms have to give the same bits, and on full sets the batch mean of D has to lie within 1e-6 relative of the
paired loss; the tool refuses to time otherwise.  No threshold is set on the times."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dpdist_amd import ChamferMatrix, ChamferPairs, EMDMatrix, EMDPairs, chamfer_matrix, chamfer_pairs, emd_matrix, emd_pairs  # noqa: E402
from dpdist_amd import aue, emd, regtest  # noqa: E402

PAIRS = 16
WIDTHS = {"chamfer": (64, 256, 1024, 2048, 4096), "chamfer_sqrt": (64, 256, 1024, 2048, 4096), "emd": (64, 256, 1024, 2048)}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def routes(kind, A, B, cA, cB, G):
    """{route: (forward, forward + backward)}; forward + backward returns (D or loss, grad A, grad B)"""
    def grads(fn, weigh=True):
        a, b = A.detach().requires_grad_(True), B.detach().requires_grad_(True)
        D = fn(a, b)
        ((G * D).sum() if weigh else D).backward()
        return D.detach(), a.grad, b.grad

    kw = {"countsA": cA, "countsB": cB}
    if kind == "emd":
        pm, mm = EMDPairs(), EMDMatrix()
        out = {"pairs": (lambda: emd_pairs(A, B, **kw), lambda: grads(lambda a, b: pm(a, b, **kw))),
               "diag": (lambda: emd_matrix(A, B, **kw).diagonal(), lambda: grads(lambda a, b: mm(a, b, **kw).diagonal()))}
        for form in (1, 2):
            out["form%d" % form] = (lambda form=form: emd._pairs_forward(A, B, cA, cB, form),
                                    lambda form=form: (emd._pairs_forward(A, B, cA, cB, form),) + emd._pairs_backward(A, B, cA, cB, G, True, True, form))
        paired = emd.earth_mover
    else:
        form = "squared" if kind == "chamfer" else "sqrt"
        pm, mm = ChamferPairs(form), ChamferMatrix(form)
        out = {"pairs": (lambda: chamfer_pairs(A, B, form, **kw), lambda: grads(lambda a, b: pm(a, b, **kw))),
               "diag": (lambda: chamfer_matrix(A, B, form, **kw).diagonal(), lambda: grads(lambda a, b: mm(a, b, **kw).diagonal()))}
        paired = aue.chamfer_dist if kind == "chamfer" else regtest.chamfer_sqrt
    if cA is None:
        out["paired"] = (lambda: paired(A, B), lambda: grads(paired, weigh=False))
    return out


def verify(name, f):
    """pairs against the yardsticks, before anything is timed"""
    Dp, gAp, gBp = f["pairs"][1]()
    Dd, gAd, gBd = f["diag"][1]()
    torch.cuda.synchronize()
    for label, x, y in (("D", Dp, Dd), ("forward D", f["pairs"][0](), f["diag"][0]()), ("dA", gAp, gAd), ("dB", gBp, gBd)):
        if not torch.equal(x, y):
            raise SystemExit("%s: %s of the pairs route and of the matrix diagonal differ" % (name, label))
    for form in ("form1", "form2"):
        if form in f:
            for label, x, y in zip(("D", "dA", "dB"), f[form][1](), (Dp, gAp, gBp)):
                if not np.array_equal(x.cpu().numpy().view(np.int32), y.cpu().numpy().view(np.int32)):
                    raise SystemExit("%s: %s of %s and of the library's choice differ in bits" % (name, label, form))
    if "paired" in f:
        loss = float(f["paired"][0]())
        if abs(float(Dp.double().mean()) - loss) > 1e-6 * abs(loss):
            raise SystemExit("%s: the mean of D (%.9g) and the paired loss (%.9g) differ" % (name, float(Dp.double().mean()), loss))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=PAIRS)
    ap.add_argument("--kinds", default="chamfer,chamfer_sqrt,emd")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "baseline_pairs_bench.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    P = a.pairs
    res = {"device": torch.cuda.get_device_name(0), "pairs": P, "rounds": a.rounds, "shapes": {}}
    lines = ["# tools/baseline_pairs_bench.py --pairs %d --rounds %d --kinds %s" % (P, a.rounds, a.kinds),
             "# device: %s; P = %d pairs; ms per call (in-stream device event pairs), median [min .. max] of %d alternating calls after 2 warm-up"
             % (res["device"], P, a.rounds),
             "# calls.  pairs: the new entries; diag: the diagonal of the all-pairs matrix with the same counts (P times the evaluations); paired: the",
             "# full-set losses with their own nodes (a batch mean); form1 / form2: the one-launch and the per-pass form of dpd_emd_pairs_*.", ""]
    for kind in a.kinds.split(","):
        for W in WIDTHS[kind]:
            for ragged in (False, True):
                rng = np.random.default_rng(12 + W)
                A = torch.tensor(rng.uniform(-0.8, 0.8, (P, W, 3)).astype(np.float32), device=dev)
                B = torch.tensor(rng.uniform(-0.8, 0.8, (P, W, 3)).astype(np.float32), device=dev)
                G = torch.tensor(rng.standard_normal(P).astype(np.float32), device=dev)
                cA = cB = None
                if ragged:
                    cA, cB = (torch.tensor(rng.integers(W // 4, W + 1, size=P), dtype=torch.int32, device=dev) for _ in range(2))
                name = "%s %dx%d %s" % (kind, P, W, "ragged" if ragged else "full")
                f = routes(kind, A, B, cA, cB, G)
                verify(name, f)
                lines.append("%s%s" % (name, ": counts uniform in [%d, %d] (mean %.1f, %.1f)" % (W // 4, W, float(cA.float().mean()), float(cB.float().mean()))
                                       if ragged else ": no counts"))
                shape = res["shapes"][name] = {}
                for k, what in ((0, "forward"), (1, "forward+backward")):
                    for _ in range(2):
                        for r in f:
                            f[r][k]()
                    torch.cuda.synchronize()
                    t = {r: [] for r in f}
                    for _ in range(a.rounds):
                        for r in f:
                            t[r].append(timed(f[r][k]))
                    med = {r: float(np.median(v)) for r, v in t.items()}
                    shape[what] = {r + "_ms": round(v, 4) for r, v in med.items()}
                    shape[what].update({r + "_over_pairs": round(med[r] / med["pairs"], 2) for r in med if r != "pairs"})
                    lines.append("    %-17s " % what + "   ".join("%s %8.3f [%8.3f .. %8.3f]" % (r, med[r], min(t[r]), max(t[r])) for r in f))
                    lines.append("    %-17s " % "" + "   ".join("%s / pairs %6.2f" % (r, med[r] / med["pairs"]) for r in f if r != "pairs"))
                lines.append("")
    text = "\n".join(lines)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)
    print(text)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

"""The all-pairs distance matrix against the same matrix through the pair path, at Ca = Cb = 32 clouds of 64 points, decoder width 1024,
on synth.s2_modelnet_shaped clouds:

    cross   dpdist_amd.dpdist_matrix (each set encoded once, layer 1 over Ca * U slots, no row matrix)
    pairs   DPDistModel.forward under no_grad on hand-tiled pairs, 128 pairs (16384 rows per launch) at a time, the mean over the
            points of pred_listAB / pred_listBA[..., 0]

    python tools/matrix_bench.py            # one JSON line
    python tools/matrix_bench.py --grad     # forward + backward under a random upstream matrix G, loss = (G * D).sum():
                                            #   cross   dpdist_amd.DPDistMatrix (one autograd node; the backward recomputes each chunk)
                                            #   pairs   the frozen model on the hand-tiled pairs, 128 pairs at a time, each pair weighted by G

    python tools/matrix_bench.py --ragged   # ragged sets (counts drawn uniformly in [N/4, N]): the counted matrix, forward and
                                            #   forward + backward, beside the full sets of the same padded width; then, at N = 2048
                                            #   (both calls encode over tiles: the same kernels), the counted call with all counts = N
                                            #   beside the un-counted call, three repetitions; written to profiles/ragged_matrix_bench.txt

The two forms alternate, five rounds after a warm-up, each timed with a device event pair; the two matrices must agree within the
fp32 forward bar of the tests (1e-4 absolute).  The per-kernel split comes from a further pass of each form under the library's in-stream
stage profiler (event pairs around every launch: dpd_prof_enable(2))."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dpdist_amd import DPDistMatrix, dpdist_matrix, synth  # noqa: E402
from dpdist_amd import lib as L  # noqa: E402
from dpdist_amd.model import DPDistModel  # noqa: E402

STAGES = {1: "encoder", 2: "index_and_gather", 3: "output_layer", 5: "pair_mean", 7: "layer1_finish"}
# --grad: the backward's launches record under the same tags (index + inverted index + gather + window scatter; pair means + upstream
# spread + slot sum / query route + query-route reduction)
STAGES_GRAD = {1: "encoder", 2: "index_gather_scatter", 3: "output_layer", 5: "spread_slotsum_reduce", 7: "layer1_finish"}


def pair_matrix(model, A, B, batch=128):
    """(D, D_AB, D_BA) through the pair path: pair p = i * Cb + j is (A_i, B_j)"""
    Ca, Cb, N = A.shape[0], B.shape[0], A.shape[1]
    a_t = A[:, None].expand(-1, Cb, -1, -1).reshape(Ca * Cb, N, 3)
    b_t = B[None].expand(Ca, -1, -1, -1).reshape(Ca * Cb, N, 3)
    ab, ba = [], []
    with torch.no_grad():
        for p0 in range(0, Ca * Cb, batch):
            ps = model(a_t[p0:p0 + batch].contiguous(), b_t[p0:p0 + batch].contiguous())
            ab.append(ps["pred_listAB"][:, :, 0, 0].mean(1))
            ba.append(ps["pred_listBA"][:, :, 0, 0].mean(1))
    d_ab, d_ba = torch.cat(ab).view(Ca, Cb), torch.cat(ba).view(Ca, Cb)
    return (d_ab + d_ba) / 2, d_ab, d_ba


def pair_grads(model, A, B, G, batch=128):
    """d (G * D).sum() / d (A, B) through the pair path in as-loss mode (frozen decoder): forward and backward per batch of pairs"""
    Ca, Cb, N = A.shape[0], B.shape[0], A.shape[1]
    a, b = A.detach().requires_grad_(True), B.detach().requires_grad_(True)
    a_t = a[:, None].expand(-1, Cb, -1, -1).reshape(Ca * Cb, N, 3)
    b_t = b[None].expand(Ca, -1, -1, -1).reshape(Ca * Cb, N, 3)
    g = G.reshape(-1)
    loss = None
    for p0 in range(0, Ca * Cb, batch):
        ps = model(a_t[p0:p0 + batch].contiguous(), b_t[p0:p0 + batch].contiguous())
        d = (ps["pred_listAB"][:, :, 0, 0].mean(1) + ps["pred_listBA"][:, :, 0, 0].mean(1)) / 2
        part = (g[p0:p0 + batch] * d).sum()
        part.backward()                     # per batch: the activations of one batch alive at a time, as in the forward
        loss = part.detach() if loss is None else loss + part.detach()
    return a.grad, b.grad, loss


def cross_grads(mod, A, B, G):
    a, b = A.detach().requires_grad_(True), B.detach().requires_grad_(True)
    loss = (G * mod(a, b)).sum()
    loss.backward()
    return a.grad, b.grad, loss.detach()


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def kernel_split(lib, fn, stages=None):
    """ms per call of `fn` by kind of launch, from the library's in-stream profiler"""
    torch.cuda.synchronize()
    lib.dpd_prof_enable(2)
    fn()
    torch.cuda.synchronize()
    out = {}
    ms, x = ctypes.c_double(0), ctypes.c_double(0)
    for form, name in ((0, "gemm_rows"), (1, "gemm_slots")):
        n = lib.dpd_prof_collect_form(form, ctypes.byref(ms), ctypes.byref(x))
        if n > 0:
            out[name] = {"launches": n, "ms": round(ms.value, 4)}
            if form == 0:       # (the slot product records its flops by the slot CAPACITY, not the live count)
                out[name]["tflops"] = round(x.value / (ms.value * 1e-3) / 1e12, 1)
    for tag, name in (stages or STAGES).items():
        n = lib.dpd_prof_collect_stage(tag, ctypes.byref(ms), ctypes.byref(x))
        if n > 0:
            out[name] = {"launches": n, "ms": round(ms.value, 4)}
    lib.dpd_prof_enable(0)
    out["sum_ms"] = round(sum(v["ms"] for v in out.values()), 4)
    return out


def ragged(a, dev, model):
    """--ragged: what per-cloud counts cost.  (1) counts uniform in [N/4, N] against the full sets of the same padded width (the padded
    rows still pay their GEMM work: the two should be close); (2) at N = 2048, counts all N against the call without counts, three
    repetitions of `rounds` calls each, alternating -- the spread of the un-counted medians is the yardstick"""
    C, N, H = a.clouds, a.points, a.width
    rng = np.random.default_rng(9)
    lines = ["# tools/matrix_bench.py --ragged --clouds %d --points %d --width %d --rounds %d --max-rows %d" % (C, N, H, a.rounds, a.max_rows),
             "# device: %s; exact fp32; times in ms per call (device event pairs), median [min .. max] of %d calls after 2 warm-up calls"
             % (torch.cuda.get_device_name(0), a.rounds), ""]
    mod = DPDistMatrix(model, max_rows=a.max_rows)

    def sets(c, n):
        return (torch.tensor(synth.s2_modelnet_shaped(c, n, 100)[0], device=dev), torch.tensor(synth.s2_modelnet_shaped(c, n, 101)[1], device=dev))

    def forms(A, B, cA, cB):
        kw = {} if cA is None else {"countsA": cA, "countsB": cB}
        G = torch.tensor(np.random.default_rng(7).standard_normal((A.shape[0], B.shape[0])).astype(np.float32), device=dev)

        def grad():
            x, y = A.detach().requires_grad_(True), B.detach().requires_grad_(True)
            (G * mod(x, y, **kw)).sum().backward()
        return (lambda: dpdist_matrix(model, A, B, max_rows=a.max_rows, **kw)), grad

    def med(fn):
        for _ in range(2):
            fn()
        v = [timed(fn) for _ in range(a.rounds)]
        return float(np.median(v)), "%9.3f [%9.3f .. %9.3f]" % (float(np.median(v)), min(v), max(v))

    # (1) ragged against full, same padded width
    A, B = sets(C, N)
    cA, cB = (torch.tensor(rng.integers(max(1, N // 4), N + 1, size=C), dtype=torch.int32, device=dev) for _ in range(2))
    lines.append("(1) Ca = Cb = %d, padded width N = %d, H = %d; counts uniform in [%d, %d]: mean %.1f (A), %.1f (B)"
                 % (C, N, H, max(1, N // 4), N, float(cA.float().mean()), float(cB.float().mean())))
    for name, (fwd, grad) in (("full sets, no counts", forms(A, B, None, None)), ("ragged sets, counts", forms(A, B, cA, cB))):
        lines.append("    %-24s forward %s   forward+backward %s" % (name, med(fwd)[1], med(grad)[1]))
    lines.append("    (the padded rows are not compacted out of the decoder GEMMs: a ragged set pays for its padded width)")
    # (2) counts == N against no counts where both encode over tiles
    N2, C2 = 2048, min(C, 8)
    A, B = sets(C2, N2)
    full = torch.full((C2,), N2, dtype=torch.int32, device=dev)
    lines += ["", "(2) Ca = Cb = %d, N = %d, H = %d: all counts = N beside the call without counts (both encode over tiles), 3 repetitions" % (C2, N2, H)]
    un, co = forms(A, B, None, None), forms(A, B, full, full)
    same = all(torch.equal(x, y) for x, y in zip(dpdist_matrix(model, A, B, return_directed=True, max_rows=a.max_rows),
                                                 dpdist_matrix(model, A, B, return_directed=True, max_rows=a.max_rows, countsA=full, countsB=full)))
    lines.append("    the two forward results are bit for bit equal: %s" % same)
    for k, what in ((0, "forward"), (1, "forward+backward")):
        m_un, m_co = [], []
        for rep_ in range(3):
            u, c = med(un[k]), med(co[k])
            m_un.append(u[0]), m_co.append(c[0])
            lines.append("    %-16s rep %d   no counts %s   counts = N %s" % (what, rep_, u[1], c[1]))
        spread = max(m_un) - min(m_un)
        diff = float(np.median(m_co)) - float(np.median(m_un))
        lines.append("    %-16s median of medians: no counts %.3f, counts = N %.3f; difference %+.3f ms; spread of the three un-counted medians %.3f ms"
                     " -> %s" % (what, float(np.median(m_un)), float(np.median(m_co)), diff, spread,
                                 "equal within that spread" if abs(diff) <= spread else "NOT within that spread"))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, default=32)
    ap.add_argument("--points", type=int, default=64)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--max-rows", type=int, default=16384)
    ap.add_argument("--grad", action="store_true", help="forward + backward under a random upstream matrix")
    ap.add_argument("--ragged", action="store_true", help="ragged sets: what per-cloud counts cost (writes --out)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "ragged_matrix_bench.txt"))
    a = ap.parse_args()
    C, N, H = a.clouds, a.points, a.width
    dev = torch.device("cuda:0")
    lib = L.load()
    A = torch.tensor(synth.s2_modelnet_shaped(C, N, 100)[0], device=dev)
    B = torch.tensor(synth.s2_modelnet_shaped(C, N, 101)[1], device=dev)
    model = DPDistModel(Embedding_Size=512, k=5, localSNmlp=(H,) * 3, sigma3dmfv=0.125, device=dev)
    model.load_tf_state_dict(synth.make_weights("wide", mlp=(H,) * 3))
    if a.ragged:
        for prm in model.parameters():
            prm.requires_grad_(False)
        return ragged(a, dev, model)
    if a.grad:
        for prm in model.parameters():
            prm.requires_grad_(False)       # as-loss mode: the decoder is frozen in both forms
        G = torch.tensor(np.random.default_rng(7).standard_normal((C, C)).astype(np.float32), device=dev)
        mod = DPDistMatrix(model, max_rows=a.max_rows)
        cross = lambda: cross_grads(mod, A, B, G)       # noqa: E731
        pairs = lambda: pair_grads(model, A, B, G)      # noqa: E731
    else:
        cross = lambda: dpdist_matrix(model, A, B, max_rows=a.max_rows, return_directed=True)   # noqa: E731
        pairs = lambda: pair_matrix(model, A, B)                                                # noqa: E731
    got, want = cross(), pairs()
    torch.cuda.synchronize()
    err = [float((x.double() - y.double()).abs().max()) for x, y in zip(got, want)]
    if a.grad:
        # both gradients sit within the input-gradient bar of the tests of the same float64 value: 2e-4 max(1, max|g|) each
        scale = max(1.0, max(float(x.abs().max()) for x in want[:2]))
        if max(err[:2]) > 4e-4 * scale or err[2] > 1e-4 * C * C:
            raise SystemExit("the two forms disagree: max |gA - gA_pairs|, gB, loss = %s" % err)
    elif max(err) > 1e-4:
        raise SystemExit("the two forms disagree: max |D - D_pairs|, AB, BA = %s" % err)
    for _ in range(2):
        cross(), pairs()
    t = {"cross": [], "pairs": []}
    for _ in range(a.rounds):
        t["cross"].append(timed(cross))
        t["pairs"].append(timed(pairs))
    slots = {}
    for name, q in (("AB", B), ("BA", A)):                      # the queries of direction AB are the clouds of B
        ix = [torch.empty(n, device=dev, dtype=dt) for n, dt in ((C * N, torch.float32), (C * N, torch.int32), (512, torch.int32), (1, torch.int32))]
        L.check(lib.dpd_cross_index(L.ptr(q), C, N, 8, *[L.ptr(x) for x in ix], L.cur_stream()), "dpd_cross_index")
        slots[name] = {"U": int(ix[3][0]), "slots": C * int(ix[3][0]), "rows": C * C * N}
    stat = lambda v: {"median_ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}   # noqa: E731
    names = ("gA", "gB", "loss") if a.grad else ("D", "D_AB", "D_BA")
    stages = STAGES_GRAD if a.grad else STAGES
    res = {"mode": "forward+backward" if a.grad else "forward", "shape": {"Ca": C, "Cb": C, "N": N, "H": H, "m": 8, "k": 5, "max_rows": a.max_rows, "pair_batch": 128},
           "device": torch.cuda.get_device_name(0), "rounds": a.rounds,
           "cross": stat(t["cross"]), "pairs": stat(t["pairs"]),
           "speedup_median": round(float(np.median(t["pairs"]) / np.median(t["cross"])), 3),
           "max_abs_diff": dict(zip(names, err)), "live_slots": slots,
           "kernels": {"cross": kernel_split(lib, cross, stages), "pairs": kernel_split(lib, pairs, stages)},
           "note": "kernels: one profiled call of each form (event pairs around every launch add ~2 us between launches); the pair path's "
                   "output layer and its torch glue (tiling, means) are not bracketed; --grad: nor are the encoder backward and the pair path's "
                   "window-gather backward"}
    print(json.dumps(res))


if __name__ == "__main__":
    main()

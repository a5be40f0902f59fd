"""The per-point field (dpdist_amd.dpdist_field: layer 1 once per occupied (cloud, voxel) window) against the same rows composed from the
plain entries (dpd_patch_rows_fwd + dpd_decoder_fwd: layer 1 once per row), in one process, at decoder width 1024 on
synth.s2_modelnet_shaped clouds, C = 8 clouds with M = 64, 1024, 10 000 queries each (uniform in the cube):

    field    dpdist_field(model, S, Q)                                  forward+backward: DPDistField, loss = (G * pred).sum(), with
                                                                        backward="rows" and backward="slots"
    rows     the encoder, then per chunk the plain gather and dpd_decoder_fwd on [rows, KP]

    python tools/field_bench.py [--out profiles/field_bench.txt]

The two forms have the same bits (checked with torch.equal before anything is timed) and walk the same chunks.  They alternate, `--rounds`
calls after two warm-up calls, each timed with an in-stream device event pair.  The backward leg has no plain twin: its two forms
alternate with each other.  Before they are timed each form is run twice and must give the same bits both times, and the two forms must
agree to 1e-3 of the largest gradient.  The rows backward takes whole clouds of at most 8192 queries, so at M = 10 000 only the slots
backward runs.  No threshold is set on the times.

--decoder-grad adds a leg per M: forward + backward with the DECODER's gradients alone (DPDistField(backward="slots", decoder_grad=True),
dpd_field_bwd_train: layer 1's weight gradient once per slot) against the same eight gradients composed over the same chunks from the
row entries (dpd_patch_rows_fwd, dpd_decoder_fwd, dpd_decoder_bwd_data with its small-gradient by-products, dpd_decoder_bwd_weights x 3
on the materialised [rows, KP] matrix).  Before they are timed the two must agree per variable within 2e-4 max(1, max |gradient|), the
relative bar of the tests.  A record, not a gate."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dpdist_amd import DPDistField, dpdist_field, synth  # noqa: E402
from dpdist_amd import lib as L  # noqa: E402
from dpdist_amd import ops  # noqa: E402
from dpdist_amd.field import MAX_BWD_QUERIES, plan_chunks  # noqa: E402
from dpdist_amd.model import DPDistModel  # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def plain_rows(model, S, Q, max_rows):
    """pred [C, M, 3] from the plain entries over the chunks of plan_chunks"""
    lib, s, P = L.load(), L.cur_stream(), model.params_
    C, M, dev = S.shape[0], Q.shape[1], S.device
    cp = P.cparams()
    fv = ops.mfv3d_fwd(S, 8, 0.125)
    out = torch.empty(C, M, 3, device=dev)
    buf = {}
    for c0, n, t0, T in plan_chunks(C, M, max_rows):
        rows = n * T
        if (n, T) not in buf:
            f = lambda *sh: torch.empty(*sh, device=dev)   # noqa: E731
            buf[n, T] = (f(rows, P.KP), f(rows), torch.empty(rows, device=dev, dtype=torch.int32), f(rows, P.H), f(rows, P.H), f(rows, 3), f(rows, 3))
        X, mask, vox, h1, h2, y, pred = buf[n, T]
        q = Q[c0:c0 + n, t0:t0 + T].contiguous()
        L.check(lib.dpd_patch_rows_fwd(L.ptr(q), L.ptr(fv[c0:]), n, T, 8, P.k, P.KP, L.ptr(X), L.ptr(mask), L.ptr(vox), None, s), "dpd_patch_rows_fwd")
        L.check(lib.dpd_decoder_fwd(L.ptr(X), L.ptr(mask), rows, P.KP, P.H, cp, 0, L.ptr(h1), L.ptr(h2), L.ptr(h1), L.ptr(y), L.ptr(pred), None, 0,
                                    None, s), "dpd_decoder_fwd")
        out[c0:c0 + n, t0:t0 + T].copy_(pred.view(n, T, 3))
    return out


def rows_weight_grads(model, S, Q, G, max_rows):
    """the eight decoder gradients of (G * pred).sum() composed from the row entries over the chunks of plan_chunks -> flat [numel]"""
    lib, s, P = L.load(), L.cur_stream(), model.params_
    C, M, dev = S.shape[0], Q.shape[1], S.device
    params, wT = P.views(), P.transposed()
    fv = ops.mfv3d_fwd(S, 8, 0.125)
    total, part = torch.zeros_like(P.flat), torch.zeros_like(P.flat)
    d = P.views(part)
    buf = {}
    for c0, n, t0, T in plan_chunks(C, M, max_rows):
        rows, rows_p = n * T, (n * T + 31) // 32 * 32
        if (n, T) not in buf:
            buf[n, T] = (torch.zeros(rows_p, P.KP, device=dev), torch.zeros(rows_p, device=dev), torch.empty(rows_p, device=dev, dtype=torch.int32),
                         torch.zeros(rows_p, 3, device=dev), ops.workspace(rows_p, P.KP, P.H, dev))
        X, mask, vox, dpred, ws = buf[n, T]
        q = Q[c0:c0 + n, t0:t0 + T].contiguous()
        L.check(lib.dpd_patch_rows_fwd(L.ptr(q), L.ptr(fv[c0:]), n, T, 8, P.k, P.KP, L.ptr(X), L.ptr(mask), L.ptr(vox), None, s), "dpd_patch_rows_fwd")
        h1, h2, h3, y, _ = ops.decoder_fwd(X, mask, params, P.H)
        dpred[:rows].copy_(G[c0:c0 + n, t0:t0 + T].reshape(rows, 3))
        dy, g3, g2, g1, _ = ops.decoder_bwd_data(dpred, mask, y, h1, h2, h3, params, P.KP, False, small_grads=(None, None, d[5], d[6], d[7]),
                                                 transposed=wT)
        ops.decoder_bwd_weights(1, X, g1, rows_p, d[0], d[1], ws)
        ops.decoder_bwd_weights(2, h1, g2, rows_p, d[2], d[3], ws)
        ops.decoder_bwd_weights(3, h2, g3, rows_p, d[4], None, ws)
        total.add_(part)
    return total


def decoder_grad_leg(a, model, S, Q, G, M, shape, lines):
    P = model.params_
    mod = DPDistField(model, max_rows=a.max_rows, backward="slots", decoder_grad=True)

    def slot_form():
        P.flat.grad = None
        (G * mod(S, Q)).sum().backward()
        return P.flat.grad

    P.flat.requires_grad_(True)
    try:
        forms = {"slots": slot_form, "rows": lambda: rows_weight_grads(model, S, Q, G, a.max_rows)}
        got, want = forms["slots"]().clone(), forms["rows"]()
        torch.cuda.synchronize()
        if not torch.equal(got, forms["slots"]()):
            raise SystemExit("M = %d: the decoder gradients are not reproducible" % M)
        for name in ("W1p", "b1", "W2", "b2", "W3", "b3", "W4", "b4"):
            x, y = P.view(name, got), P.view(name, want)
            if float((x - y).abs().max()) > 2e-4 * max(1.0, float(y.abs().max())):
                raise SystemExit("M = %d: the two forms of d%s differ by %.3e" % (M, name, float((x - y).abs().max())))
        forms["rows"]()
        t = {"slots": [], "rows": []}
        for _ in range(a.rounds):
            for form in ("slots", "rows"):
                t[form].append(timed(forms[form]))
    finally:
        P.flat.requires_grad_(False)
        P.flat.grad = None
    med = {form: float(np.median(v)) for form, v in t.items()}
    shape["decoder_grad_slots_ms"], shape["decoder_grad_rows_ms"] = round(med["slots"], 4), round(med["rows"], 4)
    lines.append("    decoder gradients  slots %9.3f [%9.3f .. %9.3f]   row entries %8.3f [%9.3f .. %9.3f]   ratio %6.2f"
                 % (med["slots"], min(t["slots"]), max(t["slots"]), med["rows"], min(t["rows"]), max(t["rows"]), med["rows"] / med["slots"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, default=8)
    ap.add_argument("--points", type=int, default=1024)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--queries", type=int, nargs="+", default=[64, 1024, 10000])
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--max-rows", type=int, default=16384)
    ap.add_argument("--decoder-grad", action="store_true", help="add the forward+backward leg with the decoder's gradients (see above)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "field_bench.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    C, H = a.clouds, a.width
    model = DPDistModel(Embedding_Size=512, k=5, localSNmlp=(H,) * 3, sigma3dmfv=0.125, device=dev)
    model.load_tf_state_dict(synth.make_weights("wide", mlp=(H,) * 3))
    for prm in model.parameters():
        prm.requires_grad_(False)
    S = torch.tensor(synth.s2_modelnet_shaped(C, a.points, 100)[0], device=dev)
    res = {"device": torch.cuda.get_device_name(0), "C": C, "W": a.points, "H": H, "m": 8, "k": 5, "max_rows": a.max_rows, "rounds": a.rounds,
           "shapes": {}}
    lines = ["# tools/field_bench.py --clouds %d --points %d --width %d --rounds %d --max-rows %d%s"
             % (C, a.points, H, a.rounds, a.max_rows, " --decoder-grad" if a.decoder_grad else ""),
             "# device: %s; exact fp32; ms per call (in-stream device event pairs), median [min .. max] of %d alternating calls after 2 warm-up calls"
             % (res["device"], a.rounds), ""]
    for M in a.queries:
        Q = torch.tensor(np.random.default_rng([9, M]).uniform(-1.0, 1.0, (C, M, 3)).astype(np.float32), device=dev)
        G = torch.tensor(np.random.default_rng(7).standard_normal((C, M, 3)).astype(np.float32), device=dev)
        f = {"field": lambda: dpdist_field(model, S, Q, max_rows=a.max_rows), "rows": lambda: plain_rows(model, S, Q, a.max_rows)}
        got, want = f["field"](), f["rows"]()
        torch.cuda.synchronize()
        if not torch.equal(got, want):
            raise SystemExit("M = %d: the two routes differ by %.3e" % (M, float((got - want).abs().max())))
        f["field"](), f["rows"]()
        t = {"field": [], "rows": []}
        for _ in range(a.rounds):
            for form in ("field", "rows"):
                t[form].append(timed(f[form]))
        med = {form: float(np.median(v)) for form, v in t.items()}
        shape = res["shapes"][str(M)] = {"field_ms": round(med["field"], 4), "rows_ms": round(med["rows"], 4),
                                        "ratio": round(med["rows"] / med["field"], 2)}
        lines.append("M = %d: %d decoder rows in %d chunk(s); same bits" % (M, C * M, len(plan_chunks(C, M, a.max_rows))))
        lines.append("    forward            field %9.3f [%9.3f .. %9.3f]   plain rows %9.3f [%9.3f .. %9.3f]   ratio %6.2f"
                     % (med["field"], min(t["field"]), max(t["field"]), med["rows"], min(t["rows"]), max(t["rows"]), med["rows"] / med["field"]))
        mods = {}
        if M <= min(a.max_rows, MAX_BWD_QUERIES):
            mods["rows"] = DPDistField(model, max_rows=a.max_rows)
        mods["slots"] = DPDistField(model, max_rows=a.max_rows, backward="slots")

        def both(mod):
            s, q = S.detach().requires_grad_(True), Q.detach().requires_grad_(True)
            (G * mod(s, q)).sum().backward()
            return s.grad, q.grad

        grads = {}
        for form, mod in mods.items():
            grads[form], again = both(mod), both(mod)
            torch.cuda.synchronize()
            if not all(torch.equal(x, y) for x, y in zip(grads[form], again)):
                raise SystemExit("M = %d: the %s backward is not reproducible" % (M, form))
        if "rows" in grads:
            for x, y in zip(grads["rows"], grads["slots"]):
                if float((x - y).abs().max()) > 1e-3 * float(x.abs().max()):
                    raise SystemExit("M = %d: the two backward forms differ by %.3e" % (M, float((x - y).abs().max())))
        tb = {form: [] for form in mods}
        for _ in range(a.rounds):
            for form, mod in mods.items():
                tb[form].append(timed(lambda: both(mod)))
        for form in ("rows", "slots"):
            if form in tb:
                shape["field_fwd_bwd_%s_ms" % form] = round(float(np.median(tb[form])), 4)
                lines.append("    forward+backward   %-5s %9.3f [%9.3f .. %9.3f]" % (form, float(np.median(tb[form])), min(tb[form]), max(tb[form])))
            else:
                shape["field_fwd_bwd_%s_ms" % form] = None
                lines.append("    forward+backward   rows  not supported (the rows backward takes whole clouds of at most %d queries)" % MAX_BWD_QUERIES)
        if a.decoder_grad:
            decoder_grad_leg(a, model, S, Q, G, M, shape, lines)
        lines.append("")
    text = "\n".join(lines)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)
    print(text)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

"""Per-point DPDist field: the decoder's answer at queries of the caller's choosing, not averaged (include/dpdist_capi.h:
dpd_field_index, dpd_field_gather, dpd_decoder_fwd_field).

    pred[c, t] = clip(y, 0, 6) / 3 * mask   of the decoder on the row built from query t and the Fisher vector of surface c

-- what `pred_listAB` of get_model holds for the partner cloud's points (utils/dpdist_util.py:434-544, 690-698), at any queries: the
labelled points of a shape, the residuals of a registration, a slice or a lattice of the field.  All three channels are returned;
channel 0 is the distance.  A cloud is encoded once and queries are never encoded.  `queries` is [C, M, 3] (cloud c's own queries) or
[M, 3] (one set evaluated against every cloud); M has no cap of its own.

A chunk is n consecutive clouds times T consecutive queries of each (plan_chunks), rows ordered (c, t).  Every chunk is independent: its
own index (one workgroup per cloud), its own slots -- the occupied (cloud, voxel) windows, at most min(m^3, T) per cloud -- and its own
slot product, so layer 1 contracts the window columns once per slot and never sees a [rows, KP] row matrix.  The bits are those of
dpd_patch_rows_fwd + dpd_decoder_fwd on the plain rows, whatever the chunking.  Exact fp32, on the current stream, without a host
synchronisation.  There is no fallback.

`dpdist_field` is the forward alone (no_grad).  `DPDistField` is the same as ONE autograd node in as-loss mode (the decoder is frozen,
gradients go to the surfaces and the queries), with two backward forms behind the `backward` keyword:

  "rows"   (the default) built from existing entries: dpd_decoder_fwd_cross_keep, dpd_decoder_bwd_data with dX [rows_p, KP],
           dpd_patch_rows_bwd and the encoder backward, per chunk of whole clouds (M <= max_rows, M <= 8192);
  "slots"  the slot-summed form (csrc/field_bwd.hip: dpd_field_invert, dpd_field_bwd): the g1 rows of the queries that share a slot are
           summed, layer 1's data gradient runs once per slot, and the tiles of one cloud accumulate into its Fisher-vector gradient.  It
           walks the forward's plan, tiles included, so M has no limit of its own, and it never holds a [rows_p, KP] matrix.
"""
import torch

from . import lib as L
from . import ops
from .pairs import MAX_WIDTH
from .pairwise import _check, _check_device, _check_shape, _host_counts, _resolve

F = 20
MAX_BWD_QUERIES = 8192      # dpd_patch_rows_bwd holds the voxels of a cloud's queries in LDS


def plan_chunks(C, M, max_rows):
    """the chunks of C clouds with M queries each -> [(first cloud, clouds, first query, queries)]: whole clouds while a cloud's queries fit
    into max_rows rows (at least one cloud), else one cloud and tiles of max_rows queries.  Pure host arithmetic."""
    C, M, max_rows = int(C), int(M), int(max_rows)
    if C < 1 or M < 1 or max_rows < 1:
        raise ValueError("plan_chunks needs C, M, max_rows >= 1")
    if M <= max_rows:
        per = max(1, max_rows // M)
        return [(c0, min(per, C - c0), 0, M) for c0 in range(0, C, per)]
    return [(c, 1, t0, min(max_rows, M - t0)) for c in range(C) for t0 in range(0, M, max_rows)]


BACKWARDS = ("rows", "slots")
MAX_SLOT_H = 4096           # dpd_field_slot_sum: one wave per 256 columns, at most 16 waves


def _prepare(model_or_params, surfaces, queries, counts, query_counts, max_rows, Embedding_Size, sigma3dmfv, backward=None):
    """every argument check, before anything is launched -> (P, m, sigma, S, Q, cS, cQ, shared): the counts as int32 device tensors | None.
    backward: None (forward only), "rows" or "slots": the backward form whose limits apply as well"""
    if backward not in (None,) + BACKWARDS:
        raise ValueError("backward must be one of %s" % (BACKWARDS,))
    rows_mode, slots_mode = backward == "rows", backward == "slots"
    P, m, sigma = _resolve(model_or_params, Embedding_Size, sigma3dmfv)
    _check_shape(surfaces, "surfaces")
    C = surfaces.shape[0]
    shared = torch.is_tensor(queries) and queries.dim() == 2
    if shared:
        if queries.shape[-1] != 3 or queries.shape[0] < 1:
            raise ValueError("queries must be a [C, M, 3] or [M, 3] tensor")
    else:
        _check_shape(queries, "queries")
        if queries.shape[0] != C:
            raise ValueError("dpdist_field evaluates cloud c at its own queries: queries must hold one set per cloud (%d != %d), or be one "
                             "shared [M, 3] set" % (queries.shape[0], C))
    M = queries.shape[-2]
    cS = _host_counts(counts, C, surfaces.shape[1], "counts")
    cQ = _host_counts(query_counts, C, M, "query_counts")
    S, Q = _check_device(surfaces, "surfaces"), _check_device(queries, "queries")
    if Q.device != S.device:
        raise ValueError("surfaces and queries must live on the same device")
    if int(max_rows) < 1:
        raise ValueError("max_rows must be positive")
    if P.flat.device != S.device:
        raise ValueError("the decoder weights and the clouds must live on the same device")
    for c, name in ((cS, "counts"), (cQ, "query_counts")):
        if c is not None and c.is_cuda and c.device != S.device:
            raise ValueError("%s and the clouds must live on the same device" % name)
    if rows_mode and M > int(max_rows):
        raise ValueError("DPDistField: the backward takes whole clouds: M = %d queries per cloud exceed max_rows = %d" % (M, int(max_rows)))
    if slots_mode and not (0 < P.H <= MAX_SLOT_H and P.H % 64 == 0):
        raise ValueError("DPDistField: the slots backward needs a decoder width H <= %d that is a multiple of 64, not %d" % (MAX_SLOT_H, P.H))
    # what the entries would refuse: the encoder's sizes (its backward: m <= 8), the window scatter's query count (rows backward), and a
    # chunk beyond the GEMMs' 32-bit byte offsets (the widest matrix: dX [rows_p, KP] of the rows backward, dXs [cap, KP] of the slots one)
    lib = L.load()
    ok = S.shape[1] <= MAX_WIDTH and 1 <= m <= (8 if backward else 10) and not (rows_mode and M > MAX_BWD_QUERIES)
    for n, T in {(n, T) for _, n, _, T in plan_chunks(C, M, max_rows)} if ok else ():
        cap, rows_p = lib.dpd_field_slot_capacity(n, T, m), (n * T + 31) // 32 * 32
        widest = max((P.KP - 32) * cap, cap * P.H, rows_p * (P.KP if rows_mode else P.H), cap * P.KP if slots_mode else 0)
        ok = ok and cap > 0 and widest * 4 < 1 << 32
    if not ok:
        raise ValueError("dpdist_field: shape not supported%s (%d clouds of width %d, %d queries each, m %d, k %d, H %d; max_rows %d)"
                         % (" by the backward" if backward else "", C, S.shape[1], M, m, P.k, P.H, max_rows))
    cS = None if cS is None else cS.to(S.device).contiguous()      # host counts: copied once
    cQ = None if cQ is None else cQ.to(S.device).contiguous()
    return P, m, sigma, S, Q, cS, cQ, shared


def _encode(lib, s, pts, m, sigma, counts):
    """pts [C,W,3] -> fv [C,m^3,20], once; a counted set through dpd_mfv3d_fwd_counts"""
    C, N, _ = pts.shape
    fv = torch.empty(C, m ** 3, F, device=pts.device, dtype=torch.float32)
    if counts is not None:
        _check(*ops.encode_counts(lib, L.ptr(pts), L.ptr(counts), C, N, m, sigma, L.ptr(fv), s))
    else:
        _check(*ops.encode(lib, L.ptr(pts), C, N, m, sigma, L.ptr(fv), s))
    return fv


class _Chunk:
    """the buffers of one chunk of n clouds times T queries.  Forward: index, slots (Xu, Pu over the slot capacity), the rows' tails, two
    ping-pong activations, y, pred.  Backward: three activations and two gradient buffers of [rows_p, H]; "rows" adds dX [rows_p, KP];
    "slots" adds gs [cap, H], dXs [cap, KP], dq [rows_p, 3] and the integer inverted index instead."""

    def __init__(self, lib, P, n, T, m, dev, backward):
        f = lambda *sh: torch.empty(*sh, device=dev, dtype=torch.float32)                  # noqa: E731
        i = lambda *sh: torch.empty(*sh, device=dev, dtype=torch.int32)                    # noqa: E731
        self.n, self.T, self.rows = n, T, n * T
        self.rows_p = rows_p = (n * T + 31) // 32 * 32
        self.cap = cap = lib.dpd_field_slot_capacity(n, T, m)
        self.mask, self.vox, self.slot, self.ucount = f(n * T), i(n * T), i(n, m ** 3), i(n)
        self.Xu, self.Xt, self.uid, self.maskr, self.cnt = f(P.KP - 32, cap), f(rows_p, 32), i(rows_p), f(rows_p), i(4)
        self.Pu, self.h1, self.h2 = f(cap, P.H), f(rows_p, P.H), f(rows_p, P.H)
        self.y, self.pred = f(rows_p, 3), f(rows_p, 3)
        if backward:
            self.h3, self.ga, self.gb = f(rows_p, P.H), f(rows_p, P.H), f(rows_p, P.H)
            self.dy, self.dpred = f(rows_p, 3), torch.zeros(rows_p, 3, device=dev, dtype=torch.float32)      # (the pad rows stay zero)
        if backward == "rows":
            self.dX, self.dq, self.dfv = f(rows_p, P.KP), f(n, T, 3), f(n, m ** 3, F)
        if backward == "slots":
            self.gs, self.dXs, self.dq = f(cap, P.H), f(cap, P.KP), f(rows_p, 3)
            self.slot_start, self.qlist, self.slot_vox, self.slot_cloud = i(cap + 1), i(n * T), i(cap), i(cap)


def _walk(lib, P, m, C, M, max_rows, dev, backward=None):
    """the chunks -> (first cloud, first query, the chunk's buffers: one set per shape)"""
    chunks = {}
    for c0, n, t0, T in plan_chunks(C, M, max_rows):
        ck = chunks.get((n, T))
        if ck is None:
            ck = chunks[n, T] = _Chunk(lib, P, n, T, m, dev, backward)
        yield c0, t0, ck


def _rows(lib, s, P, cp, m, ck, c0, t0, fv, Q, cQ, shared, keep):
    """index, gather and decoder chain of one chunk into its buffers"""
    n, T = ck.n, ck.T
    q = Q[t0:] if shared else Q[c0:, t0:]
    stride = 0 if shared else 3 * Q.shape[1]
    qc = None if cQ is None else L.ptr(cQ[c0:])
    _check(lib.dpd_field_index(L.ptr(q), stride, qc, t0, n, T, m, L.ptr(ck.mask), L.ptr(ck.vox), L.ptr(ck.slot), L.ptr(ck.ucount), s),
           "dpd_field_index")
    _check(lib.dpd_field_gather(L.ptr(q), stride, L.ptr(ck.vox), L.ptr(ck.mask), L.ptr(ck.slot), L.ptr(ck.ucount), L.ptr(fv[c0:]), n, T, m, P.k,
                                P.KP, L.ptr(ck.Xu), ck.cap, L.ptr(ck.Xt), L.ptr(ck.uid), L.ptr(ck.maskr), L.ptr(ck.cnt), s), "dpd_field_gather")
    head = (L.ptr(ck.Xu), ck.cap, ck.cap, L.ptr(ck.Xt), L.ptr(ck.uid), L.ptr(ck.cnt), L.ptr(ck.Pu), L.ptr(ck.maskr))
    if keep:
        _check(lib.dpd_decoder_fwd_cross_keep(*head, n, T, P.KP, P.H, cp, L.ptr(ck.h1), L.ptr(ck.h2), L.ptr(ck.h3), L.ptr(ck.y), L.ptr(ck.pred),
                                              None, s), "dpd_decoder_fwd_cross_keep")
    else:
        _check(lib.dpd_decoder_fwd_field(*head, ck.rows, P.KP, P.H, cp, L.ptr(ck.h1), L.ptr(ck.h2), L.ptr(ck.y), L.ptr(ck.pred), s),
               "dpd_decoder_fwd_field")


def _forward(P, m, sigma, S, Q, cS, cQ, shared, max_rows):
    """the launches of dpdist_field -> (pred [C, M, 3], mask [C, M])"""
    lib = L.load()
    C, M = S.shape[0], Q.shape[-2]
    with torch.cuda.device(S.device):
        s, cp = L.cur_stream(), P.cparams()
        fv = _encode(lib, s, S, m, sigma, cS)
        pred = torch.empty(C, M, 3, device=S.device, dtype=torch.float32)
        mask = torch.empty(C, M, device=S.device, dtype=torch.float32)
        for c0, t0, ck in _walk(lib, P, m, C, M, max_rows, S.device):
            _rows(lib, s, P, cp, m, ck, c0, t0, fv, Q, cQ, shared, False)
            pred[c0:c0 + ck.n, t0:t0 + ck.T].copy_(ck.pred[:ck.rows].view(ck.n, ck.T, 3))
            mask[c0:c0 + ck.n, t0:t0 + ck.T].copy_(ck.mask.view(ck.n, ck.T))
    return pred, mask


@torch.no_grad()
def dpdist_field(model_or_params, surfaces, queries, counts=None, query_counts=None, return_mask=False, max_rows=16384, Embedding_Size=None,
                 sigma3dmfv=None):
    """surfaces [C,W,3] (1 <= W <= 4096), queries [C,M,3] (cloud c's own) or [M,3] (one set against every cloud) -> pred [C,M,3], or
    (pred, mask [C,M]) with return_mask: pred[c,t] = clip(y, 0, 6) / 3 * mask of the decoder on the row of query t and surface c, channel 0
    the distance; mask is 0 for a query outside the cube.  counts (surface sizes) / query_counts: cloud c is its first counts[c] points, its
    queries are the first query_counts[c] (of a shared set too); the rest is finite padding that influences no bit, and pred and mask are 0
    at a padded query.  A sequence or a CPU integer tensor is checked (one count per cloud, each in [1, width], else ValueError) and copied
    to the device once; an int32 device tensor is used as it is, without a synchronisation, and the kernels clamp its values.
    model_or_params, Embedding_Size, sigma3dmfv: as dpdist_matrix.  max_rows bounds the decoder rows of one chunk (plan_chunks); the
    chunking changes no bit.  ValueError for a compute type other than exact fp32, CPU tensors, a query set per cloud of another length
    than the surfaces and shapes the C entries refuse.  Forward only: DPDistField is the differentiable form."""
    P, m, sigma, S, Q, cS, cQ, shared = _prepare(model_or_params, surfaces, queries, counts, query_counts, max_rows, Embedding_Size, sigma3dmfv)
    pred, mask = _forward(P, m, sigma, S, Q, cS, cQ, shared, max_rows)
    return (pred, mask) if return_mask else pred


class _FieldFn(torch.autograd.Function):
    """(pred, mask) of the surfaces at the queries as one autograd node"""

    @staticmethod
    def forward(ctx, surfaces, queries, P, m, sigma, max_rows, cS, cQ, mode, flat=None):
        # flat: P.flat as an input of the node (decoder_grad), else None: the decoder is frozen and the node is what it was
        ctx.cfg = (P, m, sigma, max_rows, mode)
        ctx.counts = (cS, cQ)                                           # int32 device tensors | None: no gradient exists w.r.t. counts
        ctx.set_materialize_grads(False)
        S, Q = surfaces.detach().contiguous(), queries.detach().contiguous()
        ctx.train = flat is not None
        ctx.save_for_backward(*((S, Q) if flat is None else (S, Q, flat)))      # activation checkpointing: the inputs only
        pred, mask = _forward(P, m, sigma, S, Q, cS, cQ, Q.dim() == 2, max_rows)
        ctx.mark_non_differentiable(mask)
        return pred, mask

    @staticmethod
    def backward(ctx, gpred, _gmask):
        P, m, sigma, max_rows, mode = ctx.cfg
        cS, cQ = ctx.counts
        S, Q = ctx.saved_tensors[:2]
        needS, needQ = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        needW = ctx.train and ctx.needs_input_grad[9]
        if gpred is None or not (needS or needQ or needW):
            return (None,) * (10 if ctx.train else 9)
        shared = Q.dim() == 2
        C, W, M, dev = S.shape[0], S.shape[1], Q.shape[-2], S.device
        lib = L.load()
        flat = ctx.saved_tensors[2] if ctx.train else P.flat
        with torch.cuda.device(dev), torch.no_grad():
            s = L.cur_stream()
            g = gpred.to(torch.float32).contiguous()
            if ctx.train:
                # an optimizer that writes through raw pointers bumps no version, so the cache of P.transposed would serve the weights of
                # the step before: with the decoder in training its transposed copies are derived afresh in every backward
                wT = [torch.empty(P.H, P.H, device=dev), torch.empty(P.H, P.H, device=dev), torch.empty(P.H, P.KP, device=dev)]
                _check(lib.dpd_weights_transpose(L.make_params(*P.views(flat)), P.KP, P.H, L.ptr(wT[0]), L.ptr(wT[1]), L.ptr(wT[2]), s),
                       "dpd_weights_transpose")
            else:
                wT = P.transposed(flat)
            cp = L.make_params(*P.views(flat), *wT)
            gW = torch.zeros_like(flat) if needW else None                  # the alignment gaps between the segments stay zero
            dW = [L.ptr(t) for t in P.views(gW)] if needW else None
            wws = None
            if needW:
                nbytes = max(lib.dpd_field_bwd_train_workspace_bytes(n, T, m, P.k, P.KP, P.H) for _, n, _, T in plan_chunks(C, M, max_rows))
                wws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
            first = [True]                                                  # the first chunk stores the weight gradients, the later ones add
            fv = _encode(lib, s, S, m, sigma, cS)
            gS = torch.empty_like(S) if needS else None
            gQ = (torch.zeros_like(Q) if shared else torch.empty_like(Q)) if needQ else None
            per = plan_chunks(C, M, max_rows)[0][1]
            ws = torch.empty(lib.dpd_mfv3d_bwd_workspace_bytes(per, m), device=dev, dtype=torch.uint8) if needS else None

            def encoder_bwd(c0, n, dfv):      # dfv [n, m^3, 20] of the clouds [c0, c0 + n) -> their rows of gS
                if cS is not None:
                    _check(*ops.encode_bwd_counts(lib, L.ptr(S[c0:c0 + n]), L.ptr(cS[c0:c0 + n]), L.ptr(dfv), n, W, m, sigma, L.ptr(gS[c0:c0 + n]),
                                                  L.ptr(ws), ws.numel(), s))
                else:
                    _check(*ops.encode_bwd(lib, L.ptr(S[c0:c0 + n]), L.ptr(dfv), n, W, m, sigma, L.ptr(gS[c0:c0 + n]), L.ptr(ws), ws.numel(), s))

            def rows_chunk(ck, c0, t0):      # whole clouds (t0 = 0, T = M) -> the chunk's dfv
                n = ck.n
                # g3 (ga) -> g2 (gb) -> g1 (ga) -> dX; a masked or padded query and the pad rows carry exact zeros through the mask
                _check(lib.dpd_decoder_bwd_data(L.ptr(ck.dpred), L.ptr(ck.maskr), L.ptr(ck.y), L.ptr(ck.h1), L.ptr(ck.h2), L.ptr(ck.h3), ck.rows_p,
                                                P.KP, P.H, cp, 0, L.ptr(ck.dy), L.ptr(ck.ga), L.ptr(ck.gb), L.ptr(ck.ga), L.ptr(ck.dX), None, None,
                                                0, None, 7, s), "dpd_decoder_bwd_data")
                dq = None if not needQ else (ck.dq if shared else gQ[c0:c0 + n])
                _check(lib.dpd_patch_rows_bwd(L.ptr(ck.dX), L.ptr(ck.vox), n, M, m, P.k, P.KP, L.ptr(dq), L.ptr(ck.dfv) if needS else None, s),
                       "dpd_patch_rows_bwd")
                if needQ and shared:
                    for i in range(n):      # ascending c, one chain across the chunks: a chunk boundary changes no bit
                        gQ.add_(ck.dq[i])
                return ck.dfv

            # slots mode: the tiles of one cloud come consecutively (plan_chunks: cloud outer, tile inner) and share one dfv: the first tile
            # stores it, the later ones continue the chain; a shared query set continues one chain in ascending cloud across chunks and tiles
            dfv_slots = torch.empty(per, m ** 3, F, device=dev, dtype=torch.float32) if needS and mode == "slots" else None

            def slots_chunk(ck, c0, t0):
                n, T = ck.n, ck.T
                _check(lib.dpd_field_invert(L.ptr(ck.vox), L.ptr(ck.slot), L.ptr(ck.ucount), n, T, m, ck.cap, L.ptr(ck.slot_start), L.ptr(ck.qlist),
                                            L.ptr(ck.slot_vox), L.ptr(ck.slot_cloud), s), "dpd_field_invert")
                gq = None if not needQ else (gQ[t0:] if shared else gQ[c0:, t0:])
                if needW:
                    _check(lib.dpd_field_bwd_train(L.ptr(ck.dpred), L.ptr(ck.maskr), L.ptr(ck.y), L.ptr(ck.h1), L.ptr(ck.h2), L.ptr(ck.h3),
                                                   L.ptr(ck.cnt), L.ptr(ck.ucount), L.ptr(ck.slot_start), L.ptr(ck.qlist), L.ptr(ck.slot_vox),
                                                   L.ptr(ck.slot_cloud), L.ptr(ck.Xu), ck.cap, L.ptr(ck.Xt), n, T, m, P.k, P.KP, P.H, ck.cap, cp,
                                                   L.ptr(ck.dy), L.ptr(ck.ga), L.ptr(ck.gb), L.ptr(ck.dq), L.ptr(ck.gs), L.ptr(ck.dXs),
                                                   L.ptr(dfv_slots), int(t0 > 0), L.ptr(gq), 0 if shared else 3 * M, *dW, int(not first[0]),
                                                   L.ptr(wws), wws.numel(), s), "dpd_field_bwd_train")
                    first[0] = False
                    return dfv_slots
                _check(lib.dpd_field_bwd(L.ptr(ck.dpred), L.ptr(ck.maskr), L.ptr(ck.y), L.ptr(ck.h1), L.ptr(ck.h2), L.ptr(ck.h3), L.ptr(ck.cnt),
                                         L.ptr(ck.ucount), L.ptr(ck.slot_start), L.ptr(ck.qlist), L.ptr(ck.slot_vox), L.ptr(ck.slot_cloud), n, T, m,
                                         P.k, P.KP, P.H, ck.cap, cp, L.ptr(ck.dy), L.ptr(ck.ga), L.ptr(ck.gb), L.ptr(ck.dq), L.ptr(ck.gs),
                                         L.ptr(ck.dXs), L.ptr(dfv_slots), int(t0 > 0), L.ptr(gq), 0 if shared else 3 * M, s), "dpd_field_bwd")
                return dfv_slots

            for c0, t0, ck in _walk(lib, P, m, C, M, max_rows, dev, backward=mode):
                _rows(lib, s, P, cp, m, ck, c0, t0, fv, Q, cQ, shared, True)
                ck.dpred[:ck.rows].copy_(g[c0:c0 + ck.n, t0:t0 + ck.T].reshape(ck.rows, 3))
                dfv = (slots_chunk if mode == "slots" else rows_chunk)(ck, c0, t0)
                if needS and t0 + ck.T == M:      # after the last tile of a cloud, or once per chunk of whole clouds
                    encoder_bwd(c0, ck.n, dfv)
            del cp
        return (gS, gQ) + (None,) * 7 + ((gW,) if ctx.train else ())


class DPDistField(torch.nn.Module):
    """dpdist_field as a differentiable module in as-loss mode: the decoder is frozen, gradients go to `surfaces` and `queries` only,
    under any upstream gradient of pred [C, M, 3].  Exact fp32; the forward values are bit for bit those of dpdist_field (the same
    launches).

    One autograd node over the library, on the current stream, without a host synchronisation.  The node saves the two inputs only and
    RECOMPUTES every chunk in the backward (as DPDistPairs does).  The gradient of a shared query set [M, 3] is the sum over the clouds
    in ascending order, one chain across the chunks (and tiles), so it does not depend on max_rows.

    backward="rows" (the default): layer 1's data gradient runs over the rows.  The backward takes whole clouds: M > max_rows raises a
    ValueError when an input requires a gradient (the forward has no such limit), and so does M > 8192 (the window scatter's LDS).  A
    backward chunk of rows_p rows holds three activation and two gradient buffers of [rows_p, H] and dX [rows_p, KP].  No gradient
    depends on max_rows.

    backward="slots": the slot-summed backward (dpd_field_invert, dpd_field_bwd).  The same forward launches and bits.  The g1 rows of the
    queries that share a (cloud, voxel) slot are summed, layer 1's data gradient is one product per slot, and the node walks the forward's
    plan, tiles included: M is bounded by neither max_rows nor 8192.  A chunk holds three activation and two gradient buffers of
    [rows_p, H], gs [cap, H], dXs [cap, KP], dq [rows_p, 3] and the integer index; never a [rows_p, KP] matrix.  The gradient at a query
    depends on its own row only, so the query gradients do not depend on max_rows.  The surface gradients do not either while a cloud's
    queries fit into one chunk (M <= max_rows).  With tiles (M > max_rows) a slot's sum is formed per tile and the tiles are added in
    ascending order, so the bits of the surface gradients depend on max_rows; for a given max_rows they are the same on every run, and
    they stay inside the oracle's bar.  Needs H % 64 == 0 and H <= 4096 (ValueError before any launch).  The values of the two forms
    differ by rounding only; their bits differ.

    decoder_grad=True (needs backward="slots"; with "rows" the constructor raises a ValueError): the decoder is no longer frozen.  When
    P.flat requires grad and grad is enabled, it is an input of the node and the backward returns its gradient in the flat segment layout
    (dpd_field_bwd_train), as the training node of DPDistModel does: after backward() P.flat.grad holds it, P.view(name, P.flat.grad) is a
    variable's block, P.tf_state_dict(P.flat.grad) has it under the TF names, and the alignment gaps between the segments are exact zeros.
    Layer 1's weight gradient contracts its window rows once per slot (Xu gs) and only its 32 tail columns over the rows; the chunks of the
    plan add up in ascending order.  Surfaces, queries and the decoder may need gradients in any combination; the share of an input that
    needs none is skipped.  The forward is unchanged (the launches and bits of dpdist_field).  For a given max_rows the weight gradients
    are the same bits on every run; across different max_rows they differ by rounding only, because chunks add in ascending order.  The
    surface and query gradients are bit for bit those of the frozen backward="slots" node.  The transposed weight copies are derived
    afresh in every backward, so an optimizer that updates P.flat through raw pointers (optim.TFAdam) needs no invalidate_derived() here.
    decoder_grad=False (the default): the node, its launches and every bit are those described above.

    counts / query_counts (keywords of forward): as dpdist_field.  The gradients at padded queries and padded surface points are 0; there
    is no gradient w.r.t. the counts.  An input that needs no gradient gets None and its share of the work is skipped.  Argument checks
    and errors as dpdist_field, before the first launch."""

    def __init__(self, model_or_params, max_rows=16384, Embedding_Size=None, sigma3dmfv=None, backward="rows", decoder_grad=False):
        super().__init__()
        if backward not in BACKWARDS:
            raise ValueError("backward must be one of %s, not %r" % (BACKWARDS, backward))
        if decoder_grad and backward != "slots":
            raise ValueError("decoder_grad=True needs backward=\"slots\" (the field never holds the rows that backward=%r would contract "
                             "the layer-1 weight gradient with)" % (backward,))
        self.backward = backward
        self.decoder_grad = bool(decoder_grad)
        self._src = (model_or_params, Embedding_Size, sigma3dmfv)
        _resolve(model_or_params, Embedding_Size, sigma3dmfv)
        if int(max_rows) < 1:
            raise ValueError("max_rows must be positive")
        self.max_rows = int(max_rows)

    def forward(self, surfaces, queries, return_mask=False, *, counts=None, query_counts=None):
        mp, es, sg = self._src
        flat = getattr(getattr(mp, "params_", mp), "flat", None)
        train = self.decoder_grad and torch.is_grad_enabled() and torch.is_tensor(flat) and flat.requires_grad
        want_grad = train or (torch.is_grad_enabled() and any(torch.is_tensor(t) and t.requires_grad for t in (surfaces, queries)))
        P, m, sigma, S, Q, cS, cQ, shared = _prepare(mp, surfaces, queries, counts, query_counts, self.max_rows, es, sg,
                                                     backward=self.backward if want_grad else None)
        if not want_grad:
            with torch.no_grad():
                pred, mask = _forward(P, m, sigma, S, Q, cS, cQ, shared, self.max_rows)
        elif train:
            pred, mask = _FieldFn.apply(surfaces, queries, P, m, sigma, self.max_rows, cS, cQ, self.backward, P.flat)
        else:
            pred, mask = _FieldFn.apply(surfaces, queries, P, m, sigma, self.max_rows, cS, cQ, self.backward)
        return (pred, mask) if return_mask else pred

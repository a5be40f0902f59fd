"""Paired DPDist for clouds of different sizes: the per-pair distances of two sets (include/dpdist_capi.h: dpd_patch_rows_fwd_counts,
dpd_decoder_out_pairs, dpd_pairs_combine).

    D_AB[b] = (1 / nB[b]) sum_{n < nB[b]} pred(surface A_b[:nA[b]] ; query B_b[n])[0]
    D_BA[b] = (1 / nA[b]) sum_{n < nA[b]} pred(surface B_b[:nB[b]] ; query A_b[n])[0]
    D[b]    = (D_AB[b] + D_BA[b]) / 2

which is `loss_pred` of the pair (A_b, B_b) at that pair's own sizes (models/dpdist_and_aue.py:56-69, utils/dpdist_util.py:494-511, 690-698,
976-977): the diagonal of dpdist_matrix(..., countsA, countsB) at B instead of B^2 decoder evaluations.  A set is a padded tensor
[B, W, 3] with optional counts [B] (pairwise.pad_clouds builds both from a list); the two widths may differ; a set without counts is
full.  Exact fp32, on the current stream, without a host synchronisation.

Each set is encoded once (dpd_mfv3d_fwd_counts for a counted set, else the route ops.mfv3d_fwd takes).  A chunk of P pairs is
Q = P (Wb + Wa) decoder rows, the AB half first (row b Wb + n: query B_b[n] against surface A_b), the BA half at P Wb: the window gather
runs once per half with the other set's Fisher vectors (a padded query is a zero row with mask 0), the decoder chain is dpd_decoder_fwd,
and dpd_decoder_out_pairs reduces pred[:, 0] per pair and direction.  Pairs are independent and every sum has one order (the pair means
are exact integer sums), so neither the chunking nor the other pairs of a batch change a bit.

`dpdist_pairs` is the forward alone.  `DPDistPairs` is the same as ONE autograd node in as-loss mode (the decoder is frozen, gradients go
to the two sets).  The backward runs the chain with unit upstream per directed distance -- everything between the output layer and the
inputs is linear in the two per-pair upstream scalars -- and dpd_pairs_combine applies G_ab = dL/dD_AB + dL/dD / 2 and
G_ba = dL/dD_BA + dL/dD / 2 once, at the end.
"""
import torch

from . import lib as L
from . import ops
from .pairwise import _check, _check_device, _check_shape, _host_counts, _resolve

F = 20
MAX_WIDTH = 4096        # the encoder's (include/dpdist_capi.h: dpd_mfv3d_fwd_tiled)


def chunk_pairs(B, rows_per_pair, max_rows):
    """whole pairs per chunk: at most max_rows rows, at least one pair"""
    return max(1, min(B, int(max_rows) // rows_per_pair))


def _prepare(model_or_params, cloudsA, cloudsB, countsA, countsB, max_rows, Embedding_Size, sigma3dmfv, backward=False):
    """every argument check, before anything is launched -> (P, m, sigma, A, B, cA, cB): the counts as int32 device tensors | None"""
    P, m, sigma = _resolve(model_or_params, Embedding_Size, sigma3dmfv)
    _check_shape(cloudsA, "cloudsA")
    _check_shape(cloudsB, "cloudsB")
    if cloudsA.shape[0] != cloudsB.shape[0]:
        raise ValueError("dpdist_pairs compares cloud b of one set with cloud b of the other: both sets must hold the same number of clouds "
                         "(%d != %d)" % (cloudsA.shape[0], cloudsB.shape[0]))
    cA = _host_counts(countsA, cloudsA.shape[0], cloudsA.shape[1], "countsA")
    cB = _host_counts(countsB, cloudsB.shape[0], cloudsB.shape[1], "countsB")
    A, B = _check_device(cloudsA, "cloudsA"), _check_device(cloudsB, "cloudsB")
    if B.device != A.device:
        raise ValueError("cloudsA and cloudsB must live on the same device")
    if int(max_rows) < 1:
        raise ValueError("max_rows must be positive")
    if P.flat.device != A.device:
        raise ValueError("the decoder weights and the clouds must live on the same device")
    for c, name in ((cA, "countsA"), (cB, "countsB")):
        if c is not None and c.is_cuda and c.device != A.device:
            raise ValueError("%s and the clouds must live on the same device" % name)
    Wa, Wb = A.shape[1], B.shape[1]
    per = chunk_pairs(A.shape[0], Wa + Wb, max_rows)
    # what the entries would refuse: the encoder's sizes (its backward: m <= 8), and a chunk beyond the GEMMs' 32-bit byte offsets
    if max(Wa, Wb) > MAX_WIDTH or not 1 <= m <= (8 if backward else 10) or per * (Wa + Wb) * max(P.KP, P.H) * 4 >= 1 << 32:
        raise ValueError("dpdist_pairs: shape not supported%s (%d pairs per chunk, widths %d and %d, m %d, k %d, H %d; max_rows %d)"
                         % (" by the backward" if backward else "", per, Wa, Wb, m, P.k, P.H, max_rows))
    cA = None if cA is None else cA.to(A.device).contiguous()      # host counts: copied once
    cB = None if cB is None else cB.to(A.device).contiguous()
    return P, m, sigma, A, B, cA, cB


def _encode(lib, s, pts, m, sigma, counts):
    """pts [B,W,3] -> fv [B,m^3,20], once per set; a counted set through dpd_mfv3d_fwd_counts"""
    C, N, _ = pts.shape
    fv = torch.empty(C, m ** 3, F, device=pts.device, dtype=torch.float32)
    if counts is not None:
        _check(*ops.encode_counts(lib, L.ptr(pts), L.ptr(counts), C, N, m, sigma, L.ptr(fv), s))
    else:
        _check(*ops.encode(lib, L.ptr(pts), C, N, m, sigma, L.ptr(fv), s))
    return fv


class _Chunk:
    """the buffers of one chunk of `n` pairs.  Forward: the rows, two ping-pong activations, y, pred, Dd.  Backward: three activations and
    two gradient buffers of [Q, H]; dX takes the place of the rows, which are dead after layer 1."""

    def __init__(self, P, n, Wa, Wb, m, dev, backward):
        Q = n * (Wa + Wb)
        f = lambda *sh: torch.empty(*sh, device=dev, dtype=torch.float32)   # noqa: E731
        self.n, self.Q = n, Q
        self.X, self.mask, self.vox = f(Q, P.KP), f(Q), torch.empty(Q, device=dev, dtype=torch.int32)
        self.h1, self.h2 = f(Q, P.H), f(Q, P.H)
        self.h3 = f(Q, P.H) if backward else self.h1
        self.y, self.pred, self.Dd = f(Q, 3), f(Q, 3), f(2, n)
        if backward:
            self.dy, self.ga, self.gb = f(Q, 3), f(Q, P.H), f(Q, P.H)
            self.dfv = f(n, m ** 3, F)


def _walk(P, m, A, B, max_rows, chunks, backward=False):
    """the chunks of whole pairs -> (first pair, the chunk's buffers: cached in `chunks` by size)"""
    nb, Wa, Wb = A.shape[0], A.shape[1], B.shape[1]
    per = chunk_pairs(nb, Wa + Wb, max_rows)
    for p0 in range(0, nb, per):
        n = min(per, nb - p0)
        ck = chunks.get(n)
        if ck is None:
            ck = chunks[n] = _Chunk(P, n, Wa, Wb, m, A.device, backward)
        yield p0, ck


def _part(t, p0, n):
    """pointer to the clouds [p0, p0 + n) of a per-cloud tensor (None stays None)"""
    return None if t is None else L.ptr(t[p0:p0 + n])


def _rows(lib, s, P, cp, m, ck, p0, A, B, fvA, fvB, cA, cB, backward):
    """gather of both halves, decoder chain and output layer of one chunk into its buffers"""
    n, Wa, Wb = ck.n, A.shape[1], B.shape[1]
    for q, qc, fv, W, r0 in ((B, cB, fvA, Wb, 0), (A, cA, fvB, Wa, n * Wb)):      # the AB half: queries B against surfaces A; then the BA half
        out = (L.ptr(ck.X[r0:]), L.ptr(ck.mask[r0:]), L.ptr(ck.vox[r0:]))
        if qc is None:
            _check(lib.dpd_patch_rows_fwd(_part(q, p0, n), _part(fv, p0, n), n, W, m, P.k, P.KP, *out, None, s), "dpd_patch_rows_fwd")
        else:
            _check(lib.dpd_patch_rows_fwd_counts(_part(q, p0, n), _part(qc, p0, n), _part(fv, p0, n), n, W, m, P.k, P.KP, *out, s),
                   "dpd_patch_rows_fwd_counts")
    _check(lib.dpd_decoder_fwd(L.ptr(ck.X), L.ptr(ck.mask), ck.Q, P.KP, P.H, cp, 0, L.ptr(ck.h1), L.ptr(ck.h2), L.ptr(ck.h3), None, None, None, 0,
                               None, s), "dpd_decoder_fwd")
    _check(lib.dpd_decoder_out_pairs(L.ptr(ck.h3), L.ptr(ck.mask), n, Wa, Wb, _part(cA, p0, n), _part(cB, p0, n), P.H, cp, L.ptr(ck.y),
                                     L.ptr(ck.pred), L.ptr(ck.Dd), L.ptr(ck.dy) if backward else None, L.ptr(ck.ga) if backward else None, s),
           "dpd_decoder_out_pairs")


def _forward(P, m, sigma, A, B, cA, cB, max_rows):
    """the launches of dpdist_pairs -> (D, D_AB, D_BA) [B]"""
    lib = L.load()
    with torch.cuda.device(A.device):
        s, cp = L.cur_stream(), P.cparams()
        fvA, fvB = _encode(lib, s, A, m, sigma, cA), _encode(lib, s, B, m, sigma, cB)
        d_ab, d_ba = (torch.empty(A.shape[0], device=A.device, dtype=torch.float32) for _ in range(2))
        for p0, ck in _walk(P, m, A, B, max_rows, {}):
            _rows(lib, s, P, cp, m, ck, p0, A, B, fvA, fvB, cA, cB, False)
            d_ab[p0:p0 + ck.n].copy_(ck.Dd[0])
            d_ba[p0:p0 + ck.n].copy_(ck.Dd[1])
        return (d_ab + d_ba) / 2, d_ab, d_ba


@torch.no_grad()
def dpdist_pairs(model_or_params, cloudsA, cloudsB, countsA=None, countsB=None, return_directed=False, max_rows=16384, Embedding_Size=None,
                 sigma3dmfv=None):
    """cloudsA [B,Wa,3], cloudsB [B,Wb,3] -> D [B], the distance of cloud b of one set to cloud b of the other, or (D, D_AB, D_BA) with
    return_directed.  Wa != Wb is allowed.  countsA / countsB: cloud b of a set is its first counts[b] points, the rest of its row is
    finite padding that influences no bit; a set without counts is full.  A sequence or a CPU integer tensor is checked (one count per
    cloud, each in [1, width], else ValueError) and copied to the device once; an int32 device tensor is used as it is, without a
    synchronisation, and the kernels clamp its values into [1, width].
    model_or_params, Embedding_Size, sigma3dmfv: as dpdist_matrix.  max_rows bounds the decoder rows B_chunk (Wa + Wb) of one chunk of
    whole pairs (a chunk holds at least one); the chunking changes no bit.  ValueError for a compute type other than exact fp32, CPU
    tensors, sets of different lengths and shapes the C entries refuse.  Forward only: DPDistPairs is the differentiable form."""
    P, m, sigma, A, B, cA, cB = _prepare(model_or_params, cloudsA, cloudsB, countsA, countsB, max_rows, Embedding_Size, sigma3dmfv)
    D, d_ab, d_ba = _forward(P, m, sigma, A, B, cA, cB, max_rows)
    return (D, d_ab, d_ba) if return_directed else D


class _PairsFn(torch.autograd.Function):
    """(D, D_AB, D_BA) [B] of two sets as one autograd node"""

    @staticmethod
    def forward(ctx, A, B, P, m, sigma, max_rows, cA, cB):
        ctx.cfg = (P, m, sigma, max_rows)
        ctx.counts = (cA, cB)                                           # int32 device tensors | None: no gradient exists w.r.t. counts
        ctx.set_materialize_grads(False)
        a, b = A.detach().contiguous(), B.detach().contiguous()
        ctx.save_for_backward(a, b)                                     # activation checkpointing: the clouds only
        return _forward(P, m, sigma, a, b, cA, cB, max_rows)

    @staticmethod
    def backward(ctx, gD, gAB, gBA):
        P, m, sigma, max_rows = ctx.cfg
        cA, cB = ctx.counts
        A, B = ctx.saved_tensors
        needA, needB = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if (gD is None and gAB is None and gBA is None) or not (needA or needB):
            return (None,) * 8
        nb, Wa, Wb = A.shape[0], A.shape[1], B.shape[1]
        dev = A.device

        def upstream(direct):
            """G of one direction [B]: its own upstream plus half of D's"""
            terms = [t.to(torch.float32) for t in (direct, None if gD is None else gD / 2) if t is not None]
            return sum(terms[1:], terms[0]).contiguous() if terms else torch.zeros(nb, device=dev, dtype=torch.float32)

        lib = L.load()
        flat = P.flat
        with torch.cuda.device(dev), torch.no_grad():
            s = L.cur_stream()
            g_ab, g_ba = upstream(gAB), upstream(gBA)
            cp = L.make_params(*P.views(flat), *P.transposed(flat))
            fvA, fvB = _encode(lib, s, A, m, sigma, cA), _encode(lib, s, B, m, sigma, cB)
            gA = torch.empty_like(A) if needA else None
            gB = torch.empty_like(B) if needB else None
            ws = torch.empty(lib.dpd_mfv3d_bwd_workspace_bytes(min(nb, chunk_pairs(nb, Wa + Wb, max_rows)), m), device=dev, dtype=torch.uint8)
            dpts = {True: torch.empty_like(A) if needA else None, False: torch.empty_like(B) if needB else None}
            for p0, ck in _walk(P, m, A, B, max_rows, {}, backward=True):
                n = ck.n
                _rows(lib, s, P, cp, m, ck, p0, A, B, fvA, fvB, cA, cB, True)
                # g3 (ga) -> g2 (gb) -> g1 (ga) -> dX, which overwrites the rows
                _check(lib.dpd_decoder_bwd_data(None, None, None, L.ptr(ck.h1), L.ptr(ck.h2), None, ck.Q, P.KP, P.H, cp, 0, None, L.ptr(ck.ga),
                                                L.ptr(ck.gb), L.ptr(ck.ga), L.ptr(ck.X), None, None, 0, None, 6, s), "dpd_decoder_bwd_data")
                # the encoder route of a set: the window scatter of the half whose SURFACE it is, then the encoder backward
                for isA, need, S, sc, W, r0 in ((True, needA, A, cA, Wb, 0), (False, needB, B, cB, Wa, n * Wb)):
                    if not need:
                        continue
                    _check(lib.dpd_patch_rows_bwd(L.ptr(ck.X[r0:]), L.ptr(ck.vox[r0:]), n, W, m, P.k, P.KP, None, L.ptr(ck.dfv), s),
                           "dpd_patch_rows_bwd")
                    out = _part(dpts[isA], p0, n)
                    if sc is not None:
                        _check(*ops.encode_bwd_counts(lib, _part(S, p0, n), _part(sc, p0, n), L.ptr(ck.dfv), n, S.shape[1], m, sigma, out,
                                                      L.ptr(ws), ws.numel(), s))
                    else:
                        _check(*ops.encode_bwd(lib, _part(S, p0, n), L.ptr(ck.dfv), n, S.shape[1], m, sigma, out, L.ptr(ws), ws.numel(), s))
                _check(lib.dpd_pairs_combine(_part(dpts[True], p0, n), _part(dpts[False], p0, n), L.ptr(ck.X), _part(g_ab, p0, n),
                                             _part(g_ba, p0, n), n, Wa, Wb, _part(cA, p0, n), _part(cB, p0, n), P.k, P.KP, _part(gA, p0, n),
                                             _part(gB, p0, n), s), "dpd_pairs_combine")
            del cp
        return gA, gB, None, None, None, None, None, None


class DPDistPairs(torch.nn.Module):
    """dpdist_pairs as a differentiable module in as-loss mode: the decoder is frozen, gradients go to cloudsA and cloudsB only (as in
    DPDistLoss), under any upstream gradient of D [B] and, with return_directed, of D_AB and D_BA.  Exact fp32; the forward values are
    bit for bit those of dpdist_pairs (the same launches).

    One autograd node over the library, on the current stream, without a host synchronisation.  The node saves the clouds only and
    RECOMPUTES every chunk in the backward (activation checkpointing, as DPDistMatrix does: a forward over many chunks cannot keep h1..h3
    of each).  A backward chunk of Q = B_chunk (Wa + Wb) rows holds the rows [Q, KP] (re-used for dX), three activation and two gradient
    buffers of [Q, H].  Neither values nor gradients depend on max_rows.

    countsA / countsB (keywords of forward): as dpdist_pairs.  The gradient at a padded point is exactly +0.0; there is no gradient w.r.t.
    the counts.  A set that needs no gradient gets None and its share of the work is skipped.  Argument checks and errors as
    dpdist_pairs, before the first launch."""

    def __init__(self, model_or_params, max_rows=16384, Embedding_Size=None, sigma3dmfv=None):
        super().__init__()
        self._src = (model_or_params, Embedding_Size, sigma3dmfv)
        _resolve(model_or_params, Embedding_Size, sigma3dmfv)
        if int(max_rows) < 1:
            raise ValueError("max_rows must be positive")
        self.max_rows = int(max_rows)

    def forward(self, cloudsA, cloudsB, return_directed=False, *, countsA=None, countsB=None):
        mp, es, sg = self._src
        want_grad = torch.is_grad_enabled() and any(torch.is_tensor(t) and t.requires_grad for t in (cloudsA, cloudsB))
        P, m, sigma, A, B, cA, cB = _prepare(mp, cloudsA, cloudsB, countsA, countsB, self.max_rows, es, sg, backward=want_grad)
        if not want_grad:
            with torch.no_grad():
                D, d_ab, d_ba = _forward(P, m, sigma, A, B, cA, cB, self.max_rows)
        else:
            D, d_ab, d_ba = _PairsFn.apply(cloudsA, cloudsB, P, m, sigma, self.max_rows, cA, cB)
        return (D, d_ab, d_ba) if return_directed else D

"""All-pairs DPDist: the distance matrix between two sets of clouds (include/dpdist_capi.h: dpd_cross_index, dpd_cross_gather,
dpd_decoder_fwd_cross).

    D_AB[i, j] = mean_n pred(surface A_i ; query B_j[n])[0]
    D_BA[i, j] = mean_n pred(surface B_j ; query A_i[n])[0]
    D          = (D_AB + D_BA) / 2

which is `loss_pred` of the pair (A_i, B_j) as DPDistLoss computes it (utils/dpdist_util.py:976-979), for every pair.  Each set is
encoded once; the queries of a set are indexed once per direction (their voxels do not depend on the surface cloud), so layer 1 of the
decoder contracts the window columns once per (surface cloud, occupied voxel) and never sees a [rows, KP] row matrix.  Exact fp32,
on the current stream, without a host synchronisation.  There is no fallback to the pair path.

`dpdist_matrix` is the forward alone (no_grad).  `DPDistMatrix` is the same matrix as ONE autograd node in as-loss mode (the decoder is
frozen, gradients go to the two cloud sets; dpd_cross_invert, dpd_decoder_fwd_cross_keep, dpd_cross_bwd): the node saves the clouds and
recomputes every chunk in the backward, where the gradient rows that share a (surface cloud, occupied voxel) slot are summed before the
layer-1 data gradient, the window scatter and the encoder backward.

RAGGED sets (countsA / countsB): a set is a padded tensor [C, N, 3] plus counts [C]; cloud c is its first counts[c] points (pad_clouds
builds both from a list of clouds).  The surface side of a counted set is encoded by dpd_mfv3d_fwd_counts / dpd_mfv3d_bwd_counts, its
query side indexed by dpd_cross_index_counts (a padded query is a masked query of voxel 0) and averaged over each cloud's own count
(dpd_decoder_fwd_cross_counts, dpd_cross_bwd_counts).  The padding must be finite; it influences no bit of any output or gradient, and
its gradient is exactly +0.0.  The padded rows still cost their share of the decoder GEMMs.
"""
import math

import torch

from . import lib as L
from . import ops

F = 20


def _check(rc, what):
    """a shape an entry refuses is the caller's ValueError; anything else stays the library's RuntimeError"""
    if rc in (-2, -3):
        raise ValueError("dpdist_matrix: %s refuses this shape: %s" % (what, L._ERR[rc]))
    L.check(rc, what)


def _resolve(model_or_params, Embedding_Size, sigma3dmfv):
    """-> (DPDistParams, m, sigma)"""
    P = getattr(model_or_params, "params_", model_or_params)
    if model_or_params is not P:                         # a DPDistModel carries its grid and sigma: a different one given here is a mistake
        for name, given, own in (("Embedding_Size", Embedding_Size, model_or_params.Embedding_Size), ("sigma3dmfv", sigma3dmfv, model_or_params.sigma)):
            if given is not None and given != own:
                raise ValueError("%s=%r contradicts the model's %r" % (name, given, own))
        Embedding_Size, sigma3dmfv = model_or_params.Embedding_Size, model_or_params.sigma
    Embedding_Size = 512 if Embedding_Size is None else Embedding_Size
    sigma3dmfv = 0.125 if sigma3dmfv is None else sigma3dmfv
    m = int(math.ceil(Embedding_Size ** (1 / 3) - 1e-9))
    if m ** 3 != Embedding_Size:
        raise ValueError("Embedding_Size must be a perfect cube")
    for attr in ("flat", "KP", "H", "k", "compute_dtype"):
        if not hasattr(P, attr):
            raise ValueError("dpdist_matrix needs a DPDistModel or DPDistParams, got %s" % type(model_or_params).__name__)
    if L.DTYPES.get(P.compute_dtype) != 0:
        raise ValueError("dpdist_matrix is exact fp32 only (compute type %r)" % (P.compute_dtype,))
    return P, m, float(sigma3dmfv)


def _check_shape(t, name):
    if not torch.is_tensor(t) or t.dim() != 3 or t.shape[-1] != 3 or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError("%s must be a [C, N, 3] tensor" % name)


def _check_device(t, name):
    if not t.is_cuda:
        raise ValueError("%s must live on the GPU (dpdist_amd has no CPU path)" % name)
    if t.dtype != torch.float32:
        raise ValueError("%s must be float32, got %s" % (name, t.dtype))
    return t.detach().contiguous()


def chunk_clouds(C, rows_per_cloud, max_rows):
    """whole surface clouds per chunk: at most max_rows rows, at least one cloud"""
    return max(1, min(C, int(max_rows) // rows_per_cloud))


class _Chunk:
    """the buffers of one chunk of `ca` surface clouds (backward: of one BACKWARD chunk): one allocation of the size the workspace report
    states, carved by the library (dpd_cross_carve) -- `ptr` holds the addresses of the members the form has, by name"""

    def __init__(self, lib, ca, Cb, N, m, P, dev, backward=False):
        shape = (ca, Cb, N, m, P.k, P.KP, P.H)
        nbytes = (lib.dpd_cross_bwd_workspace_bytes if backward else lib.dpd_cross_workspace_bytes)(*shape)
        if not nbytes:
            raise ValueError("dpdist_matrix: shape not supported%s (clouds per chunk %d x %d, N %d, m %d, k %d, H %d)"
                             % (" by the backward" if backward else "", ca, Cb, N, m, P.k, P.H))
        self.arena = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        self.c = L.CrossChunk()
        L.check(lib.dpd_cross_carve(L.ptr(self.arena), nbytes, *shape, int(backward), self.c), "dpd_cross_carve")
        self.ca, self.cap = ca, self.c.slot_cap
        self.ptr = {n: getattr(self.c, n) for n in L.CrossChunk.BUFFERS if getattr(self.c, n) is not None}

    def Dd(self, n):
        off = self.ptr["Dd"] - self.arena.data_ptr()
        return self.arena[off:off + 4 * n].view(torch.float32)


def _index(lib, s, Q, m, extra=0, qcounts=None):
    """the queries Q [Cq, N, 3] indexed once per direction (dpd_cross_index; dpd_cross_index_counts for a ragged set) -> mask [Cq N], then
    of one int32 allocation vox [Cq N], slot_of_vox [m^3] with the count behind it, the count alone, and `extra` words for the caller"""
    QN, G = Q.shape[0] * Q.shape[1], m ** 3
    mask = torch.empty(QN, device=Q.device, dtype=torch.float32)
    idx = torch.empty(QN + G + 1 + extra, device=Q.device, dtype=torch.int32)
    vox, slot, rest = idx[:QN], idx[QN:QN + G + 1], idx[QN + G + 1:]
    ucount = slot[G:]
    if qcounts is None:
        _check(lib.dpd_cross_index(L.ptr(Q), Q.shape[0], Q.shape[1], m, L.ptr(mask), L.ptr(vox), L.ptr(slot), L.ptr(ucount), s), "dpd_cross_index")
    else:
        _check(lib.dpd_cross_index_counts(L.ptr(Q), L.ptr(qcounts), Q.shape[0], Q.shape[1], m, L.ptr(mask), L.ptr(vox), L.ptr(slot),
                                          L.ptr(ucount), s), "dpd_cross_index_counts")
    return mask, vox, slot, ucount, rest


def _walk(lib, P, m, Cs, Q, max_rows, chunks, backward=False):
    """the chunks of whole surface clouds of one direction -> (first cloud, clouds, the chunk's buffers: cached in `chunks` by shape)"""
    Cq, N, _ = Q.shape
    per = chunk_clouds(Cs, Cq * N, max_rows)
    for i0 in range(0, Cs, per):
        ca = min(per, Cs - i0)
        ck = chunks.get((ca, Cq, N))
        if ck is None:
            ck = chunks[ca, Cq, N] = _Chunk(lib, ca, Cq, N, m, P, Q.device, backward)
        yield i0, ca, ck


def _encode(lib, s, pts, m, sigma, counts=None):
    """pts [C,N,3] -> fv [C,m^3,20], once per set; a ragged set (counts) always through dpd_mfv3d_fwd_counts"""
    C, N, _ = pts.shape
    fv = torch.empty(C, m ** 3, F, device=pts.device, dtype=torch.float32)
    if counts is not None:
        _check(*ops.encode_counts(lib, L.ptr(pts), L.ptr(counts), C, N, m, sigma, L.ptr(fv), s))
    else:
        _check(*ops.encode(lib, L.ptr(pts), C, N, m, sigma, L.ptr(fv), s))    # over tiles of points beyond the plain entry's LDS cap
    return fv


def _directed(lib, s, P, cp, m, fvS, Q, qcounts, max_rows, chunks):
    """[Cs, Cq]: every surface cloud (Fisher vectors fvS [Cs, m^3, 20]) against the queries Q [Cq, N, 3] (qcounts: their counts | None)"""
    Cs, (Cq, N, _) = fvS.shape[0], Q.shape
    mask, vox, slot, ucount, _ = _index(lib, s, Q, m, qcounts=qcounts)
    out = torch.empty(Cs, Cq, device=Q.device, dtype=torch.float32)
    for i0, ca, ck in _walk(lib, P, m, Cs, Q, max_rows, chunks):
        p = ck.ptr
        _check(lib.dpd_cross_gather(L.ptr(Q), L.ptr(vox), L.ptr(mask), L.ptr(slot), L.ptr(ucount), L.ptr(fvS[i0:i0 + ca]), None, ca, Cq, N, m,
                                     P.k, P.KP, p["Xu"], ck.cap, p["Xt"], p["uid"], p["maskr"], p["cnt"], s), "dpd_cross_gather")
        if qcounts is None:
            _check(lib.dpd_decoder_fwd_cross(p["Xu"], ck.cap, ck.cap, p["Xt"], p["uid"], p["cnt"], p["Pu"], p["maskr"], ca * Cq, N, P.KP, P.H, cp,
                                              p["act0"], p["act1"], p["y"], p["pred"], p["Dd"], s), "dpd_decoder_fwd_cross")
        else:
            _check(lib.dpd_decoder_fwd_cross_counts(p["Xu"], ck.cap, ck.cap, p["Xt"], p["uid"], p["cnt"], p["Pu"], p["maskr"], L.ptr(qcounts),
                                                     ca * Cq, Cq, N, P.KP, P.H, cp, p["act0"], p["act1"], p["y"], p["pred"], p["Dd"], s),
                   "dpd_decoder_fwd_cross_counts")
        out[i0:i0 + ca].copy_(ck.Dd(ca * Cq).view(ca, Cq))
    return out


def pad_clouds(clouds):
    """a list of clouds [n_i, 3] (n_i >= 1) -> (points [C, max n_i, 3], zero padded; counts [C] int32), both on the clouds' device: the
    ragged-set arguments of dpdist_matrix / DPDistMatrix"""
    clouds = list(clouds)
    if not clouds:
        raise ValueError("pad_clouds needs at least one cloud")
    for t in clouds:
        if not torch.is_tensor(t) or t.dim() != 2 or t.shape[1] != 3 or t.shape[0] < 1:
            raise ValueError("every cloud must be a [n, 3] tensor with n >= 1")
    if any(t.device != clouds[0].device or t.dtype != clouds[0].dtype for t in clouds):
        raise ValueError("the clouds must share one device and one dtype")
    pts = clouds[0].new_zeros(len(clouds), max(t.shape[0] for t in clouds), 3)
    for c, t in enumerate(clouds):
        pts[c, :t.shape[0]] = t.detach()
    return pts, torch.tensor([t.shape[0] for t in clouds], dtype=torch.int32, device=clouds[0].device)


def _host_counts(counts, C, width, name):
    """the checks of one counts argument that need no device: a device tensor is checked for type and length only (its values are clamped
    into [1, width] by the kernels, without a synchronisation); host data is checked value by value -> int32 tensor | None"""
    if counts is None:
        return None
    if torch.is_tensor(counts) and counts.is_cuda:
        if counts.dtype != torch.int32 or counts.dim() != 1:
            raise ValueError("%s on the device must be a one-dimensional int32 tensor" % name)
        t = counts
    else:
        t = torch.as_tensor(counts)
        if t.dim() != 1 or t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool:
            raise ValueError("%s must be a sequence of integers" % name)
    if t.numel() != C:
        raise ValueError("%s must hold one count per cloud (%d != %d)" % (name, t.numel(), C))
    if not t.is_cuda:
        if int(t.min()) < 1 or int(t.max()) > width:
            raise ValueError("%s must lie in [1, %d] (got %d .. %d)" % (name, width, int(t.min()), int(t.max())))
        t = t.to(torch.int32)
    return t


def _prepare(model_or_params, cloudsA, cloudsB, max_rows, Embedding_Size, sigma3dmfv, report="dpd_cross_workspace_bytes", countsA=None,
             countsB=None):
    """every argument check of the matrix, and every chunk shape of both directions against `report` before anything is launched
    -> (P, m, sigma, A, B, cA, cB): the counts as int32 device tensors (None: a full set; cB is None for a set against itself)"""
    P, m, sigma = _resolve(model_or_params, Embedding_Size, sigma3dmfv)
    _check_shape(cloudsA, "cloudsA")
    if cloudsB is not None:
        _check_shape(cloudsB, "cloudsB")
        if countsA is None and countsB is None and cloudsB.shape[1] != cloudsA.shape[1]:
            raise ValueError("the clouds of both sets must have the same number of points (%d != %d)" % (cloudsA.shape[1], cloudsB.shape[1]))
    elif countsB is not None:
        raise ValueError("countsB given without cloudsB (a set against itself takes countsA)")
    cA = _host_counts(countsA, cloudsA.shape[0], cloudsA.shape[1], "countsA")
    cB = None if cloudsB is None else _host_counts(countsB, cloudsB.shape[0], cloudsB.shape[1], "countsB")
    A = _check_device(cloudsA, "cloudsA")
    B = None if cloudsB is None else _check_device(cloudsB, "cloudsB")
    if B is not None and B.device != A.device:
        raise ValueError("cloudsA and cloudsB must live on the same device")
    if int(max_rows) < 1:
        raise ValueError("max_rows must be positive")
    if P.flat.device != A.device:
        raise ValueError("the decoder weights and the clouds must live on the same device")
    for c, name in ((cA, "countsA"), (cB, "countsB")):
        if c is not None and c.is_cuda and c.device != A.device:
            raise ValueError("%s and the clouds must live on the same device" % name)
    check_chunks(L.load(), report, P, m, A.shape[0], None if B is None else B.shape[0], A.shape[1], max_rows, None if B is None else B.shape[1])
    cA = None if cA is None else cA.to(A.device).contiguous()      # host counts: copied once
    cB = None if cB is None else cB.to(A.device).contiguous()
    return P, m, sigma, A, B, cA, cB


def check_chunks(lib, report, P, m, Ca, Cb, N, max_rows, Nb=None):
    """every chunk shape of both directions (Cb = None: a set against itself) against a workspace report, which allocates nothing: a
    chunk too large for the GEMMs' 32-bit offsets is refused here.  A direction is walked by its QUERY set's width: N is cloudsA's,
    Nb cloudsB's where it differs (ragged sets)"""
    for Cs, Cq, N in ((Ca, Ca, N),) if Cb is None else ((Ca, Cb, N if Nb is None else Nb), (Cb, Ca, N)):
        per = chunk_clouds(Cs, Cq * N, max_rows)
        for ca in {per, Cs % per} - {0}:
            if not getattr(lib, report)(ca, Cq, N, m, P.k, P.KP, P.H):
                raise ValueError("dpdist_matrix: shape not supported (%d x %d clouds per chunk, N %d, m %d, k %d, H %d; max_rows %d)"
                                 % (ca, Cq, N, m, P.k, P.H, max_rows))


def _forward(P, m, sigma, A, B, max_rows, cA=None, cB=None):
    """the launches of dpdist_matrix -> (D, D_AB, D_BA); cA / cB: the counts of a ragged set (int32, on the device) | None"""
    lib = L.load()
    with torch.cuda.device(A.device):
        s, cp = L.cur_stream(), P.cparams()
        chunks = {}
        fvA = _encode(lib, s, A, m, sigma, cA)
        if B is None:
            d_ab = _directed(lib, s, P, cp, m, fvA, A, cA, max_rows, chunks)
            d_ba = d_ab.t()
        else:
            fvB = _encode(lib, s, B, m, sigma, cB)
            d_ab = _directed(lib, s, P, cp, m, fvA, B, cB, max_rows, chunks)
            d_ba = _directed(lib, s, P, cp, m, fvB, A, cA, max_rows, chunks).t()      # the same code with the sets swapped
        D = (d_ab + d_ba) / 2
    return D, d_ab, d_ba.contiguous()


@torch.no_grad()
def dpdist_matrix(model_or_params, cloudsA, cloudsB=None, max_rows=16384, return_directed=False, Embedding_Size=None,
                  sigma3dmfv=None, *, countsA=None, countsB=None):
    """cloudsA [Ca,N,3], cloudsB [Cb,N,3] (None: cloudsA against itself, from one direction) -> D [Ca,Cb], or (D, D_AB, D_BA) with
    return_directed.  model_or_params: a DPDistModel, or a DPDistParams with the grid (Embedding_Size = m^3, default 512) and sigma3dmfv
    (default 0.125) given here; with a DPDistModel they are the model's, and different values given here raise.
    max_rows bounds the decoder rows of one chunk of whole surface clouds (a chunk holds at least one): 16384 rows are two activation
    buffers of 64 MB at H = 1024.  ValueError for a compute type other than exact fp32, CPU tensors, N differing between the sets and
    shapes the C entries refuse.  Forward only: DPDistMatrix is the differentiable form.
    countsA / countsB (keywords): ragged sets -- cloud c of a set is its first counts[c] points, the rest of its row is finite padding that
    influences no bit (pad_clouds builds both).  With at least one of them the padded widths of the two sets may differ; a set without
    counts is full; a set against itself takes countsA.  A sequence or a CPU integer tensor is checked (one count per cloud, each in
    [1, width], else ValueError) and copied to the device once; an int32 device tensor is used as it is, without a synchronisation, and
    the kernels clamp its values into [1, width]."""
    P, m, sigma, A, B, cA, cB = _prepare(model_or_params, cloudsA, cloudsB, max_rows, Embedding_Size, sigma3dmfv, countsA=countsA,
                                         countsB=countsB)
    D, d_ab, d_ba = _forward(P, m, sigma, A, B, max_rows, cA, cB)
    return (D, d_ab, d_ba) if return_directed else D


# ---- the differentiable form ----
def _directed_bwd(lib, s, P, cp, m, sigma, S, fvS, Q, Gd, need_s, need_q, max_rows, chunks, scounts=None, qcounts=None):
    """one direction of the backward: surface clouds S [Cs, Ns, 3] (Fisher vectors fvS), queries Q [Cq, N, 3], upstream Gd [Cs, Cq] of that
    direction's matrix -> (surface route [Cs, Ns, 3] | None, query route [Cq, N, 3] | None); scounts / qcounts: the counts of a ragged
    surface / query set (their padded rows get +0.0 on both routes)"""
    Cs, Ns, (Cq, N, _) = S.shape[0], S.shape[1], Q.shape
    dev = Q.device
    G = m ** 3
    mask, vox, slot, ucount, rest = _index(lib, s, Q, m, Cq * N + 2 * G + 1, qcounts)
    qlist, start, svox = rest[:Cq * N], rest[Cq * N:][:G + 1], rest[Cq * N + G + 1:]
    _check(lib.dpd_cross_invert(L.ptr(vox), L.ptr(slot), L.ptr(ucount), Cq, N, m, L.ptr(start), L.ptr(qlist), L.ptr(svox), s), "dpd_cross_invert")
    gS = torch.empty(Cs, Ns, 3, device=dev, dtype=torch.float32) if need_s else None
    gQ = torch.zeros(Cq, N, 3, device=dev, dtype=torch.float32) if need_q else None
    ws = torch.empty(lib.dpd_mfv3d_bwd_workspace_bytes(Cs, m), device=dev, dtype=torch.uint8) if need_s else None
    for i0, ca, ck in _walk(lib, P, m, Cs, Q, max_rows, chunks, backward=True):
        p = ck.ptr
        _check(lib.dpd_cross_gather(L.ptr(Q), L.ptr(vox), L.ptr(mask), L.ptr(slot), L.ptr(ucount), L.ptr(fvS[i0:i0 + ca]), None, ca, Cq, N, m,
                                     P.k, P.KP, p["Xu"], ck.cap, p["Xt"], p["uid"], p["maskr"], p["cnt"], s), "dpd_cross_gather")
        _check(lib.dpd_decoder_fwd_cross_keep(p["Xu"], ck.cap, ck.cap, p["Xt"], p["uid"], p["cnt"], p["Pu"], p["maskr"], ca * Cq, N, P.KP, P.H,
                                               cp, p["h1"], p["h2"], p["h3"], p["y"], p["pred"], None, s), "dpd_decoder_fwd_cross_keep")
        tail = (p["y"], p["h1"], p["h2"], p["h3"], p["cnt"], L.ptr(start), L.ptr(qlist), L.ptr(svox), ca, Cq, N, m, P.k, P.KP, P.H, ck.cap, cp,
                p["dpred"], p["dy"], p["ga"], p["gb"], p["dq"], p["gs"] if need_s else None, p["dXs"] if need_s else None,
                p["dfv"] if need_s else None, L.ptr(gQ), s)
        if qcounts is None:
            _check(lib.dpd_cross_bwd(L.ptr(Gd[i0:i0 + ca]), p["maskr"], *tail), "dpd_cross_bwd")
        else:
            _check(lib.dpd_cross_bwd_counts(L.ptr(Gd[i0:i0 + ca]), p["maskr"], L.ptr(qcounts), *tail), "dpd_cross_bwd_counts")
        if need_s and scounts is not None:
            _check(*ops.encode_bwd_counts(lib, L.ptr(S[i0:i0 + ca]), L.ptr(scounts[i0:i0 + ca]), p["dfv"], ca, Ns, m, sigma,
                                          L.ptr(gS[i0:i0 + ca]), L.ptr(ws), ws.numel(), s))
        elif need_s:
            _check(*ops.encode_bwd(lib, L.ptr(S[i0:i0 + ca]), p["dfv"], ca, Ns, m, sigma, L.ptr(gS[i0:i0 + ca]), L.ptr(ws), ws.numel(), s))
    return gS, gQ


class _MatrixFn(torch.autograd.Function):
    """(D, D_AB, D_BA) of two cloud sets as one autograd node; B is None for a set against itself"""

    @staticmethod
    def forward(ctx, A, B, P, m, sigma, max_rows, cA, cB):
        ctx.cfg = (P, m, sigma, max_rows, B is None)
        ctx.counts = (cA, cB)                                           # int32 device tensors | None: no gradient exists w.r.t. counts
        ctx.set_materialize_grads(False)
        a = A.detach().contiguous()
        b = None if B is None else B.detach().contiguous()
        ctx.save_for_backward(*((a,) if b is None else (a, b)))        # activation checkpointing: the clouds only
        return _forward(P, m, sigma, a, b, max_rows, cA, cB)

    @staticmethod
    def backward(ctx, gD, gAB, gBA):
        P, m, sigma, max_rows, self_matrix = ctx.cfg
        cA, cB = ctx.counts
        A = ctx.saved_tensors[0]
        B = A if self_matrix else ctx.saved_tensors[1]
        needA = ctx.needs_input_grad[0]
        needB = (not self_matrix) and ctx.needs_input_grad[1]
        if (gD is None and gAB is None and gBA is None) or not (needA or needB):
            return (None,) * 8

        def upstream(*terms):
            """the sum of the upstreams that exist, as a contiguous fp32 matrix (None: no upstream at all)"""
            terms = [t for t in terms if t is not None]
            return sum(terms[1:], terms[0]).to(torch.float32).contiguous() if terms else None

        # D = (D_AB + D_BA) / 2; D_BA is returned as [Ca, Cb], its direction's matrix (surface B, query A) is [Cb, Ca]
        half = None if gD is None else gD / 2
        half_t = None if gD is None else half.t()
        gBA_t = None if gBA is None else gBA.t()
        lib = L.load()
        flat = P.flat
        with torch.cuda.device(A.device), torch.no_grad():
            s = L.cur_stream()
            cp = L.make_params(*P.views(flat), *P.transposed(flat))
            chunks = {}
            gA = gB = None
            if self_matrix:
                # D_BA = D_AB^T: the matrix came from one direction, whose upstream is (G + G^T) / 2 plus the directed ones; both routes land in A
                g = upstream(half, half_t, gAB, gBA_t)
                fvA = _encode(lib, s, A, m, sigma, cA)
                gs_, gq_ = _directed_bwd(lib, s, P, cp, m, sigma, A, fvA, A, g, True, True, max_rows, chunks, cA, cA)
                gA = gs_ + gq_
            else:
                g_ab, g_ba = upstream(half, gAB), upstream(half_t, gBA_t)
                sA = qB = sB = qA = None
                if g_ab is not None:
                    fvA = _encode(lib, s, A, m, sigma, cA)
                    sA, qB = _directed_bwd(lib, s, P, cp, m, sigma, A, fvA, B, g_ab, needA, needB, max_rows, chunks, cA, cB)
                if g_ba is not None:
                    fvB = _encode(lib, s, B, m, sigma, cB)
                    sB, qA = _directed_bwd(lib, s, P, cp, m, sigma, B, fvB, A, g_ba, needB, needA, max_rows, chunks, cB, cA)
                both = lambda x, y: y if x is None else (x if y is None else x + y)   # noqa: E731  (a direction without upstream gave None)
                gA, gB = both(sA, qA), both(qB, sB)
            del cp
        return gA, gB, None, None, None, None, None, None


class DPDistMatrix(torch.nn.Module):
    """dpdist_matrix as a differentiable module in as-loss mode: the decoder is frozen, gradients go to cloudsA and cloudsB only (as in
    DPDistLoss), under any upstream gradient of D [Ca, Cb] and, with return_directed, of D_AB and D_BA.  Exact fp32; the forward values
    are bit for bit those of dpdist_matrix (the same launches on the same buffers).

    One autograd node over the library, on the current stream, without a host synchronisation.  The node saves the clouds only and
    recomputes every chunk in the backward (activation checkpointing: an all-pairs forward cannot keep h1..h3 of every chunk).  A backward
    chunk of `rows_p` decoder rows holds three activation buffers and two gradient buffers of [rows_p, H] and y, beside the slot buffers
    (Xu, Pu, gs, dXs over the slot capacity): the default max_rows = 16384 makes that five buffers of 64 MB at H = 1024.  The gradients do
    not depend on max_rows (chunks hold whole surface clouds and the query-route sum is one chain across the chunks).

    cloudsB = None: cloudsA against itself from one direction; its upstream is then (G + G^T) / 2 and both routes land in cloudsA.
    A set that needs no gradient gets None and its share of the work is skipped.  Argument checks and errors as dpdist_matrix; every chunk
    shape of forward and backward is checked before the first launch.

    countsA / countsB (keywords of forward): ragged sets as in dpdist_matrix.  The gradient at a padded point is exactly +0.0; there is no
    gradient w.r.t. the counts."""

    def __init__(self, model_or_params, max_rows=16384, Embedding_Size=None, sigma3dmfv=None):
        super().__init__()
        self._src = (model_or_params, Embedding_Size, sigma3dmfv)
        _resolve(model_or_params, Embedding_Size, sigma3dmfv)
        if int(max_rows) < 1:
            raise ValueError("max_rows must be positive")
        self.max_rows = int(max_rows)

    def forward(self, cloudsA, cloudsB=None, return_directed=False, *, countsA=None, countsB=None):
        mp, es, sg = self._src
        want_grad = torch.is_grad_enabled() and any(torch.is_tensor(t) and t.requires_grad for t in (cloudsA, cloudsB))
        P, m, sigma, A, B, cA, cB = _prepare(mp, cloudsA, cloudsB, self.max_rows, es, sg,
                                             "dpd_cross_bwd_workspace_bytes" if want_grad else "dpd_cross_workspace_bytes", countsA, countsB)
        if not want_grad:
            with torch.no_grad():
                D, d_ab, d_ba = _forward(P, m, sigma, A, B, self.max_rows, cA, cB)
        else:
            D, d_ab, d_ba = _MatrixFn.apply(cloudsA, cloudsB, P, m, sigma, self.max_rows, cA, cB)
        return (D, d_ab, d_ba) if return_directed else D

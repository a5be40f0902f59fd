"""All-pairs DPDist: the distance matrix between two sets of clouds (include/dpdist_capi.h: dpd_cross_index, dpd_cross_gather,
dpd_decoder_fwd_cross).

    D_AB[i, j] = mean_n pred(surface A_i ; query B_j[n])[0]
    D_BA[i, j] = mean_n pred(surface B_j ; query A_i[n])[0]
    D          = (D_AB + D_BA) / 2

which is `loss_pred` of the pair (A_i, B_j) as DPDistLoss computes it (utils/dpdist_util.py:976-979), for every pair.  Each set is
encoded once; the queries of a set are indexed once per direction (their voxels do not depend on the surface cloud), so layer 1 of the
decoder contracts the window columns once per (surface cloud, occupied voxel) and never sees a [rows, KP] row matrix.  Exact fp32,
forward only, on the current stream, without a host synchronisation.  There is no fallback to the pair path.
"""
import math

import torch

from . import lib as L

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
    """the buffers of one chunk of `ca` surface clouds, carved from one allocation in the order dpd_cross_workspace_bytes states"""

    def __init__(self, lib, ca, Cb, N, m, P, dev):
        nbytes = lib.dpd_cross_workspace_bytes(ca, Cb, N, m, P.k, P.KP, P.H)
        self.cap = lib.dpd_cross_slot_capacity(ca, Cb, N, m)
        if not nbytes or not self.cap:
            raise ValueError("dpdist_matrix: shape not supported (clouds per chunk %d x %d, N %d, m %d, k %d, H %d)" % (ca, Cb, N, m, P.k, P.H))
        self.ca = ca
        rows_p = (ca * Cb * N + 31) // 32 * 32
        self.arena = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        off = 0
        self.ptr = {}
        for name, size in (("Xu", (P.KP - 32) * self.cap * 4), ("Xt", rows_p * 32 * 4), ("uid", rows_p * 4), ("maskr", rows_p * 4), ("cnt", 16),
                           ("Pu", self.cap * P.H * 4), ("act0", rows_p * P.H * 4), ("act1", rows_p * P.H * 4), ("y", rows_p * 12),
                           ("pred", rows_p * 12), ("Dd", ca * Cb * 4)):
            self.ptr[name] = self.arena.data_ptr() + off
            off += (size + 255) // 256 * 256
        if off != nbytes:
            raise RuntimeError("dpd_cross_workspace_bytes and dpdist_amd.pairwise disagree on the layout (%d != %d)" % (off, nbytes))
        self.Dd_off = self.ptr["Dd"] - self.arena.data_ptr()

    def Dd(self, n):
        return self.arena[self.Dd_off:self.Dd_off + 4 * n].view(torch.float32)


def _encode(lib, s, pts, m, sigma):
    """pts [C,N,3] -> fv [C,m^3,20], once per set"""
    C, N, _ = pts.shape
    fv = torch.empty(C, m ** 3, F, device=pts.device, dtype=torch.float32)
    _check(lib.dpd_mfv3d_fwd(L.ptr(pts), C, N, m, sigma, L.ptr(fv), s), "dpd_mfv3d_fwd")
    return fv


def _directed(lib, s, P, cp, m, fvS, Q, max_rows, chunks):
    """[Cs, Cq]: every surface cloud (Fisher vectors fvS [Cs, m^3, 20]) against the queries Q [Cq, N, 3]"""
    Cs, (Cq, N, _) = fvS.shape[0], Q.shape
    dev = Q.device
    mask = torch.empty(Cq * N, device=dev, dtype=torch.float32)
    vox = torch.empty(Cq * N, device=dev, dtype=torch.int32)
    slot = torch.empty(m ** 3 + 1, device=dev, dtype=torch.int32)          # slot_of_vox, then the count
    ucount = slot[m ** 3:]
    _check(lib.dpd_cross_index(L.ptr(Q), Cq, N, m, L.ptr(mask), L.ptr(vox), L.ptr(slot), L.ptr(ucount), s), "dpd_cross_index")
    out = torch.empty(Cs, Cq, device=dev, dtype=torch.float32)
    per = chunk_clouds(Cs, Cq * N, max_rows)
    for i0 in range(0, Cs, per):
        ca = min(per, Cs - i0)
        key = (ca, Cq)
        ck = chunks.get(key)
        if ck is None:
            ck = chunks[key] = _Chunk(lib, ca, Cq, N, m, P, dev)
        p = ck.ptr
        _check(lib.dpd_cross_gather(L.ptr(Q), L.ptr(vox), L.ptr(mask), L.ptr(slot), L.ptr(ucount), L.ptr(fvS[i0:i0 + ca]), None, ca, Cq, N, m,
                                     P.k, P.KP, p["Xu"], ck.cap, p["Xt"], p["uid"], p["maskr"], p["cnt"], s), "dpd_cross_gather")
        _check(lib.dpd_decoder_fwd_cross(p["Xu"], ck.cap, ck.cap, p["Xt"], p["uid"], p["cnt"], p["Pu"], p["maskr"], ca * Cq, N, P.KP, P.H, cp,
                                          p["act0"], p["act1"], p["y"], p["pred"], p["Dd"], s), "dpd_decoder_fwd_cross")
        out[i0:i0 + ca].copy_(ck.Dd(ca * Cq).view(ca, Cq))
    return out


@torch.no_grad()
def dpdist_matrix(model_or_params, cloudsA, cloudsB=None, max_rows=16384, return_directed=False, Embedding_Size=None,
                  sigma3dmfv=None):
    """cloudsA [Ca,N,3], cloudsB [Cb,N,3] (None: cloudsA against itself, from one direction) -> D [Ca,Cb], or (D, D_AB, D_BA) with
    return_directed.  model_or_params: a DPDistModel, or a DPDistParams with the grid (Embedding_Size = m^3, default 512) and sigma3dmfv
    (default 0.125) given here; with a DPDistModel they are the model's, and different values given here raise.
    max_rows bounds the decoder rows of one chunk of whole surface clouds (a chunk holds at least one): 16384 rows are two activation
    buffers of 64 MB at H = 1024.  ValueError for a compute type other than exact fp32, CPU tensors, N differing between the sets and
    shapes the C entries refuse."""
    P, m, sigma = _resolve(model_or_params, Embedding_Size, sigma3dmfv)
    _check_shape(cloudsA, "cloudsA")
    if cloudsB is not None:
        _check_shape(cloudsB, "cloudsB")
        if cloudsB.shape[1] != cloudsA.shape[1]:
            raise ValueError("the clouds of both sets must have the same number of points (%d != %d)" % (cloudsA.shape[1], cloudsB.shape[1]))
    A = _check_device(cloudsA, "cloudsA")
    B = None if cloudsB is None else _check_device(cloudsB, "cloudsB")
    if B is not None and B.device != A.device:
        raise ValueError("cloudsA and cloudsB must live on the same device")
    if int(max_rows) < 1:
        raise ValueError("max_rows must be positive")
    if P.flat.device != A.device:
        raise ValueError("the decoder weights and the clouds must live on the same device")
    lib = L.load()
    # every chunk shape of both directions, before anything is launched (a chunk too large for the GEMMs' 32-bit offsets is refused here)
    for Cs, Cq in ((A.shape[0], A.shape[0]),) if B is None else ((A.shape[0], B.shape[0]), (B.shape[0], A.shape[0])):
        per = chunk_clouds(Cs, Cq * A.shape[1], max_rows)
        for ca in {per, Cs % per} - {0}:
            if not lib.dpd_cross_workspace_bytes(ca, Cq, A.shape[1], m, P.k, P.KP, P.H):
                raise ValueError("dpdist_matrix: shape not supported (%d x %d clouds per chunk, N %d, m %d, k %d, H %d; max_rows %d)"
                                 % (ca, Cq, A.shape[1], m, P.k, P.H, max_rows))
    with torch.cuda.device(A.device):
        s, cp = L.cur_stream(), P.cparams()
        chunks = {}
        fvA = _encode(lib, s, A, m, sigma)
        if B is None:
            d_ab = _directed(lib, s, P, cp, m, fvA, A, max_rows, chunks)
            d_ba = d_ab.t()
        else:
            fvB = _encode(lib, s, B, m, sigma)
            d_ab = _directed(lib, s, P, cp, m, fvA, B, max_rows, chunks)
            d_ba = _directed(lib, s, P, cp, m, fvB, A, max_rows, chunks).t()      # the same code with the sets swapped
        D = (d_ab + d_ba) / 2
    return (D, d_ab, d_ba.contiguous()) if return_directed else D

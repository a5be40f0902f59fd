"""Farthest-point sampling on the HIP library (csrc/fps.hip; the definition is the comment above dpd_fps_order in include/dpdist_capi.h).

    farthest_point_order    the order itself: order[c, 0] = start, order[c, k] = the not yet chosen point farthest from order[c, :k]
    farthest_point_sample   the first K points of that order (and the same rows of per-point features), differentiable in the values

The reference's readers take "the first npoints rows" of a shape file (modelnet_dataset.py:121-122,136) and get a well-spread cloud only
because modelnet40_normal_resampled was written in this order; dpdist_amd.dataset.resample_tree writes any tree that way.  Distances are
(dx*dx + dy*dy) + dz*dz in fp32, not fused, ties go to the lowest index and a chosen point is excluded: the order is defined bit for bit,
is a prefix of a permutation, and the order for K is a prefix of the order for any larger K.  Ragged sets follow the library's conventions
(`counts`, pad_clouds): cloud c is its first counts[c] rows, the padding is never read.  There is no torch fallback.
"""
import torch

from . import lib as L
from . import ops
from .pairwise import _host_counts

FPS_THREADS = 1024                 # include/dpdist_capi.h: DPD_FPS_THREADS, one workgroup per cloud
FPS_RESIDENT_POINTS = 16384        # DPD_FPS_RESIDENT_POINTS: clouds up to this width live in registers
FPS_MAX_POINTS = 1 << 20           # DPD_FPS_MAX_POINTS
FPS_MAX_CLOUDS = 65535             # DPD_FPS_MAX_CLOUDS


def _host_start(start, S, W, counts):
    """start: None, or one index per cloud as a list / numpy array / int32 tensor.  Host values are checked against [0, n - 1] (n from
    host counts, else W); a device tensor is checked for type and length only (the kernel clamps it) -> int32 tensor | None"""
    if start is None:
        return None
    if torch.is_tensor(start) and start.is_cuda:
        if start.dtype != torch.int32 or start.dim() != 1:
            raise ValueError("start on the device must be a one-dimensional int32 tensor")
        t = start
    else:
        t = torch.as_tensor(start)
        if t.dim() != 1 or t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool:
            raise ValueError("start must be a sequence of integers")
    if t.numel() != S:
        raise ValueError("start must hold one index per cloud (%d != %d)" % (t.numel(), S))
    if not t.is_cuda:
        n = counts.to(torch.int64) if counts is not None and not counts.is_cuda else torch.full((S,), W, dtype=torch.int64)
        if int(t.min()) < 0 or bool((t.to(torch.int64) >= n).any()):
            raise ValueError("start must lie in [0, n - 1] of its cloud")
        t = t.to(torch.int32)
    return t


def _prepare(clouds, K, counts, start):
    """every check that needs no device, then the boundary check of the tensors -> (pts [S,W,3], counts, start on the device, batched)"""
    if not torch.is_tensor(clouds) or clouds.dim() not in (2, 3) or clouds.shape[-1] != 3:
        raise ValueError("clouds must be a [S, W, 3] or [W, 3] tensor")
    batched = clouds.dim() == 3
    pts = clouds if batched else clouds[None]
    S, W = pts.shape[0], pts.shape[1]
    if S < 1 or W < 1:
        raise ValueError("clouds must hold at least one cloud of at least one point")
    if int(K) != K or not 1 <= int(K) <= W:
        raise ValueError("K must lie in [1, %d], got %s" % (W, K))
    c = _host_counts(counts, S, W, "counts")
    s = _host_start(start, S, W, c)
    L.req(pts, name="clouds")
    c = None if c is None else c.to(pts.device)
    s = None if s is None else s.to(pts.device)
    return pts, c, s, batched


def farthest_point_order(clouds, K, counts=None, start=None, return_radius=False):
    """clouds [S,W,3] (or one cloud [W,3]) -> order [S,K] int32 (or [K]): the farthest-point order of each cloud from row start[c] (0),
    -1 past min(K, counts[c]).  With return_radius also radius [S,K]: the distance of each chosen point to all earlier ones (+inf for
    the first, non-increasing after it, 0 past the valid part).  counts / start: lists, numpy arrays or int32 tensors with one entry per
    cloud; host values outside [1, W] / [0, n - 1] raise ValueError, device values are clamped by the kernel.  No gradient."""
    pts, c, s, batched = _prepare(clouds, K, counts, start)
    order, radius = ops.fps_order(pts.detach(), int(K), c, s, want_radius=return_radius)
    if not batched:
        order, radius = order[0], None if radius is None else radius[0]
    return (order, radius) if return_radius else order


class _Gather(torch.autograd.Function):
    """out[c,k,:] = src[c, order[c,k], :] (dpd_fps_gather_fwd); the adjoint writes the chosen rows and +0.0 elsewhere (dpd_fps_gather_bwd)"""

    @staticmethod
    def forward(ctx, src, order):
        ctx.save_for_backward(order)
        ctx.W = src.shape[1]
        return ops.fps_gather_fwd(src, order)

    @staticmethod
    def backward(ctx, dout):
        (order,) = ctx.saved_tensors
        return ops.fps_gather_bwd(dout.contiguous(), order, ctx.W), None


def farthest_point_sample(clouds, K, counts=None, start=None, features=None):
    """The first K points of the farthest-point order: (points [S,K,3], counts_out, order [S,K]), and with features [S,W,D] the same rows of
    them as a fourth value [S,K,D].  counts_out = min(K, counts) (int32 on the device; None without counts): rows past it are +0.0 and
    `order` is -1 there, so (points, counts_out) go straight into the counts arguments of dpdist_pairs, dpdist_matrix, chamfer_*, emd_*
    and DPDistLoss.  Gradients reach the chosen rows of clouds and features (exactly +0.0 elsewhere); the order carries none.
    One cloud [W,3] (features [W,D]) gives [K,3], [K] (and [K,D]); counts_out keeps its shape [1]."""
    feats = None
    if features is not None:                             # shape errors first: they need no device
        if not torch.is_tensor(clouds) or not torch.is_tensor(features) or features.dim() != clouds.dim() or features.dim() not in (2, 3):
            raise ValueError("features must be a [S, W, D] tensor (or [W, D] with one cloud [W, 3])")
        if features.shape[:-1] != clouds.shape[:-1] or features.shape[-1] < 1:
            raise ValueError("features must hold one row per point of clouds")
    pts, c, s, batched = _prepare(clouds, K, counts, start)
    if features is not None:
        feats = features if batched else features[None]
        L.req(feats, name="features")
    order, _ = ops.fps_order(pts.detach(), int(K), c, s)
    points = _Gather.apply(pts, order)
    counts_out = None if c is None else torch.clamp(c, 1, int(K))
    out_f = None if feats is None else _Gather.apply(feats, order)
    if not batched:
        points, order = points[0], order[0]
        out_f = None if out_f is None else out_f[0]
    return (points, counts_out, order) if feats is None else (points, counts_out, order, out_f)

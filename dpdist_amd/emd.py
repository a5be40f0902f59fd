"""Earth Mover's distance on the HIP kernels (csrc/emd.hip): the EMD loss of the registration baselines.

Restates (relative to /root/reference):
    utils/tf_util_loss.py:42-47        earth_mover(pcd1, pcd2): match = approx_match(pcd1, pcd2); cost = match_cost(pcd1, pcd2, match);
                                       mean(cost / num_points)
    models/ipcr_model.py:296-314       its use as the loss of the iterative PCRNet
The reference's CUDA op (pc_distance/tf_approxmatch) is not in its tree; the contract is the one in include/dpdist_capi.h (dpd_emd_fwd).
The match carries no gradient, like the op's.
"""
import torch

from . import lib as L


def _dims(pcd1, pcd2):
    L.req(pcd1, name="pcd1"), L.req(pcd2, name="pcd2")
    if pcd1.dim() != 3 or pcd2.dim() != 3 or pcd1.shape[2] != 3 or pcd2.shape[2] != 3 or pcd1.shape[0] != pcd2.shape[0]:
        raise RuntimeError("pcd1 [B,n,3] and pcd2 [B,m,3] must hold the same number of clouds, got %s and %s"
                           % (tuple(pcd1.shape), tuple(pcd2.shape)))
    return pcd1.shape[0], pcd1.shape[1], pcd2.shape[1]


def _workspace(lib, B, n, m, dev):
    return torch.empty(max(1, lib.dpd_emd_workspace_bytes(B, n, m)), device=dev, dtype=torch.uint8)


def emd_forward(pcd1, pcd2, want_grad1=True, want_grad2=True, want_match=False, gscale=1.0):
    """One dpd_emd_fwd call: (cost [B], loss [1], grad1 or None, grad2 or None, match [B,m,n] or None); the gradients are
    gscale * d loss / d pcd."""
    B, n, m = _dims(pcd1, pcd2)
    dev, lib = pcd1.device, L.load()
    cost, loss = torch.empty(B, device=dev), torch.empty(1, device=dev)
    g1 = torch.empty_like(pcd1) if want_grad1 else None
    g2 = torch.empty_like(pcd2) if want_grad2 else None
    match = torch.empty(B, m, n, device=dev) if want_match else None
    ws = _workspace(lib, B, n, m, dev)
    L.check(lib.dpd_emd_fwd(L.ptr(pcd1), L.ptr(pcd2), B, n, m, float(gscale), L.ptr(cost), L.ptr(loss), L.ptr(g1), L.ptr(g2), L.ptr(match),
                            L.ptr(ws), ws.numel(), L.cur_stream()), "dpd_emd_fwd")
    return cost, loss, g1, g2, match


class _EarthMoverFn(torch.autograd.Function):
    """forward = the fused launch sequence with the gradients saved (no [B,m,n] array); backward scales them on the device"""

    @staticmethod
    def forward(ctx, pcd1, pcd2):
        _, loss, g1, g2, _ = emd_forward(pcd1, pcd2, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        ctx.save_for_backward(g1, g2)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        g1, g2 = ctx.saved_tensors
        return (None if g1 is None else g1 * g), (None if g2 is None else g2 * g)


def earth_mover(pcd1, pcd2):
    """earth_mover(pcd1, pcd2) of utils/tf_util_loss.py:42-47: mean over the batch of cost / n, pcd1 [B,n,3], pcd2 [B,m,3]."""
    return _EarthMoverFn.apply(pcd1.contiguous(), pcd2.contiguous())


def approx_match(pcd1, pcd2):
    """The op's approx_match: match [B,m,n] (no gradient)."""
    with torch.no_grad():
        return emd_forward(pcd1.contiguous(), pcd2.contiguous(), False, False, True)[4]


class _MatchCostFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pcd1, pcd2, match):
        B, n, m = _dims(pcd1, pcd2)
        L.req(match, name="match", shape=(B, m, n))
        dev, lib = pcd1.device, L.load()
        cost, loss = torch.empty(B, device=dev), torch.empty(1, device=dev)
        g1 = torch.empty_like(pcd1) if ctx.needs_input_grad[0] else None
        g2 = torch.empty_like(pcd2) if ctx.needs_input_grad[1] else None
        ws = _workspace(lib, B, n, m, dev)
        # gscale = B n: the gradients of cost[b] itself, not of the mean
        L.check(lib.dpd_emd_match_cost(L.ptr(pcd1), L.ptr(pcd2), B, n, m, L.ptr(match), float(B * n), L.ptr(cost), L.ptr(loss), L.ptr(g1),
                                       L.ptr(g2), L.ptr(ws), ws.numel(), L.cur_stream()), "dpd_emd_match_cost")
        ctx.save_for_backward(g1, g2)
        return cost

    @staticmethod
    def backward(ctx, g):
        g1, g2 = ctx.saved_tensors
        return (None if g1 is None else g1 * g[:, None, None]), (None if g2 is None else g2 * g[:, None, None]), None


def match_cost(pcd1, pcd2, match):
    """The op's match_cost: cost [B] = sum_{k,l} match[l][k] |pcd1_k - pcd2_l| with gradients to both clouds, none to the match."""
    return _MatchCostFn.apply(pcd1.contiguous(), pcd2.contiguous(), match.contiguous())

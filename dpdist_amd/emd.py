"""Earth Mover's distance on the HIP kernels (csrc/emd.hip): the EMD loss of the registration baselines.

Restates (relative to /root/reference):
    utils/tf_util_loss.py:42-47        earth_mover(pcd1, pcd2): match = approx_match(pcd1, pcd2); cost = match_cost(pcd1, pcd2, match);
                                       mean(cost / num_points)
    models/ipcr_model.py:296-314       its use as the loss of the iterative PCRNet
The reference's CUDA op (pc_distance/tf_approxmatch) is not in its tree; the contract is the one in include/dpdist_capi.h (dpd_emd_fwd).
The match carries no gradient, like the op's.

All pairs of two sets of clouds: emd_matrix / EMDMatrix (csrc/emd_matrix.hip: dpd_emd_matrix_fwd / _bwd, one workgroup per pair), in the
conventions of dpdist_matrix and chamfer_matrix.  D[i, j] = earth_mover(A_i, B_j), bit for bit; nothing of size [Ca, Cb, N] exists in the
forward, and the backward's per-pair gradients pass through a workspace bounded by MAX_WS_BYTES.  There is no fallback to expanded pairs.

The pairs (A_b, B_b) alone, ragged: emd_pairs / EMDPairs (csrc/emd_pairs.hip: dpd_emd_pairs_fwd / _bwd), in the conventions of dpdist_pairs.
D[b] = earth_mover(A_b, B_b), bit for bit; the library runs a pair per workgroup in one launch at small widths and a launch per pass with
a workgroup per 64-point tile at large ones.
"""
import torch

from . import lib as L
from .baselines import _check, _prepare

MAX_POINTS = 2048                # DPD_EMD_MAX_POINTS: both clouds of a pair live in LDS
MAX_WS_BYTES = 1 << 30           # bound on the workspace of EMDMatrix's backward: above it the backward goes in chunks of rows of A


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


def _matrix_forward(A, B, cA, cB):
    """D [Ca,Cb] of prepared sets (B None: A against itself, all Ca^2 pairs -- the match is not symmetric)"""
    lib = L.load()
    Q, cQ = (A, cA) if B is None else (B, cB)
    D = torch.empty(A.shape[0], Q.shape[0], device=A.device, dtype=torch.float32)
    with torch.cuda.device(A.device):
        _check(lib.dpd_emd_matrix_fwd(L.ptr(A), L.ptr(cA), A.shape[0], A.shape[1], L.ptr(Q), L.ptr(cQ), Q.shape[0], Q.shape[1], None,
                                             L.ptr(D), L.cur_stream()), "dpd_emd_matrix_fwd")
    return D


def _matrix_backward(A, B, cA, cB, W, needA, needB):
    """(dA | None, dB | None) under the upstream W [Ca,Cb] of D.  Rows of A go in ascending chunks whose workspace stays within
    MAX_WS_BYTES (one row at least); dB is a left fold over the rows, continued from chunk to chunk, so chunking changes no bit."""
    lib = L.load()
    (Ca, Na), (Cb, Nb) = A.shape[:2], B.shape[:2]
    per_row = Cb * (Na + Nb) * 3 * 4
    rows = max(1, min(Ca, MAX_WS_BYTES // per_row))
    dA = torch.empty_like(A) if needA else None
    dB = torch.empty_like(B) if needB else None
    with torch.cuda.device(A.device):
        ws = torch.empty(rows * per_row, device=A.device, dtype=torch.uint8)
        s = L.cur_stream()
        for chunk, i0 in enumerate(range(0, Ca, rows)):
            r = min(rows, Ca - i0)
            _check(lib.dpd_emd_matrix_bwd(L.ptr(A[i0:]), L.ptr(None if cA is None else cA[i0:]), r, Na, L.ptr(B), L.ptr(cB), Cb, Nb,
                                                 L.ptr(W[i0:]), L.ptr(None if dA is None else dA[i0:]), L.ptr(dB), int(chunk > 0), L.ptr(ws),
                                                 ws.numel(), s), "dpd_emd_matrix_bwd")
    return dA, dB


@torch.no_grad()
def emd_matrix(cloudsA, cloudsB=None, *, countsA=None, countsB=None):
    """cloudsA [Ca,N,3], cloudsB [Cb,M,3] (None: cloudsA against itself) -> D [Ca,Cb], D[i,j] = earth_mover(A_i, B_j): the cost of the
    approximate matching of the pair over the number of points of A_i, bit for bit the paired entry's value.  The two sets may have
    different widths.  countsA / countsB (keywords): ragged sets as in dpdist_matrix -- a sequence or CPU integer tensor is checked (one
    count per cloud, each in [1, width]) and copied once, an int32 device tensor is used as it is and clamped by the kernels; padding is
    never read.  ValueError for CPU tensors, a dtype other than float32, sets on two devices, bad counts, countsB without cloudsB and
    more than 2048 points per cloud -- before anything is launched.  Forward only: EMDMatrix is differentiable."""
    return _matrix_forward(*_prepare(cloudsA, cloudsB, countsA, countsB, cap=MAX_POINTS))


class _EMDMatrixFn(torch.autograd.Function):
    """D of two cloud sets as one autograd node; B is None for a set against itself"""

    @staticmethod
    def forward(ctx, A, B, cA, cB):
        ctx.self_matrix = B is None
        ctx.counts = (cA, cB)
        ctx.set_materialize_grads(False)
        a = A.detach().contiguous()
        b = None if B is None else B.detach().contiguous()
        ctx.save_for_backward(*((a,) if b is None else (a, b)))        # the two sets only: the match is recomputed
        return _matrix_forward(a, b, cA, cB)

    @staticmethod
    def backward(ctx, gD):
        cA, cB = ctx.counts
        A = ctx.saved_tensors[0]
        needA = ctx.needs_input_grad[0]
        needB = (not ctx.self_matrix) and ctx.needs_input_grad[1]
        if gD is None or not (needA or needB):
            return (None,) * 4
        W = gD.to(torch.float32).contiguous()
        with torch.no_grad():
            if ctx.self_matrix:                                        # both routes of the one call land in A
                g1, g2 = _matrix_backward(A, A, cA, cA, W, True, True)
                return g1 + g2, None, None, None
            dA, dB = _matrix_backward(A, ctx.saved_tensors[1], cA, cB, W, needA, needB)
        return dA, dB, None, None


class EMDMatrix(torch.nn.Module):
    """emd_matrix as a differentiable module: gradients to cloudsA and cloudsB under any upstream gradient of D [Ca,Cb].  One autograd node
    over the library, on the current stream, without a host synchronisation; the forward values are bit for bit those of emd_matrix.  The
    match carries no gradient (as in earth_mover); the node saves the two sets only and the backward recomputes the match of every
    pair.  cloudsB = None: both routes of the one call land in cloudsA's gradient.  The gradient at a padded point is exactly +0.0; a set
    that needs no gradient gets None and its route is skipped.  Arguments and errors as emd_matrix."""

    def forward(self, cloudsA, cloudsB=None, *, countsA=None, countsB=None):
        want_grad = torch.is_grad_enabled() and any(torch.is_tensor(t) and t.requires_grad for t in (cloudsA, cloudsB))
        A, B, cA, cB = _prepare(cloudsA, cloudsB, countsA, countsB, cap=MAX_POINTS)
        if not want_grad:
            with torch.no_grad():
                return _matrix_forward(A, B, cA, cB)
        return _EMDMatrixFn.apply(cloudsA, cloudsB, cA, cB)


def _pairs_workspace(lib, A, B):
    return torch.empty(max(1, lib.dpd_emd_pairs_workspace_bytes(A.shape[0], A.shape[1], B.shape[1])), device=A.device, dtype=torch.uint8)


def _pairs_forward(A, B, cA, cB, form=0):
    """D [P] of prepared sets; form: 0 the library's choice, 1 one launch, 2 per pass (the same bits)"""
    lib = L.load()
    D = torch.empty(A.shape[0], device=A.device, dtype=torch.float32)
    with torch.cuda.device(A.device):
        ws = _pairs_workspace(lib, A, B)
        _check(lib.dpd_emd_pairs_fwd(L.ptr(A), L.ptr(cA), A.shape[1], L.ptr(B), L.ptr(cB), B.shape[1], A.shape[0], form, None, L.ptr(D),
                                            L.ptr(ws), ws.numel(), L.cur_stream()), "dpd_emd_pairs_fwd")
    return D


def _pairs_backward(A, B, cA, cB, W, needA, needB, form=0):
    """(dA | None, dB | None) under the upstream W [P] of D"""
    lib = L.load()
    dA = torch.empty_like(A) if needA else None
    dB = torch.empty_like(B) if needB else None
    with torch.cuda.device(A.device):
        ws = _pairs_workspace(lib, A, B)
        _check(lib.dpd_emd_pairs_bwd(L.ptr(A), L.ptr(cA), A.shape[1], L.ptr(B), L.ptr(cB), B.shape[1], A.shape[0], form, L.ptr(W),
                                            L.ptr(dA), L.ptr(dB), L.ptr(ws), ws.numel(), L.cur_stream()), "dpd_emd_pairs_bwd")
    return dA, dB


@torch.no_grad()
def emd_pairs(cloudsA, cloudsB, *, countsA=None, countsB=None):
    """cloudsA [P,N,3], cloudsB [P,M,3] -> D [P], D[b] = earth_mover(A_b, B_b): the cost of the approximate matching of the pair over the
    number of points of A_b, bit for bit the paired entry's value and emd_matrix's on the pair alone.  The two sets may have different
    widths.  countsA / countsB (keywords): ragged sets as in dpdist_pairs -- a sequence or CPU integer tensor is checked (one count per
    cloud, each in [1, width]) and copied once, an int32 device tensor is used as it is and clamped by the kernels; padding is never
    read.  ValueError for sets of different lengths, CPU tensors, a dtype other than float32, sets on two devices, bad counts and more
    than 2048 points per cloud -- before anything is launched.  Forward only: EMDPairs is differentiable."""
    return _pairs_forward(*_prepare(cloudsA, cloudsB, countsA, countsB, cap=MAX_POINTS, pairs=True))


class _EMDPairsFn(torch.autograd.Function):
    """D [P] of the pairs of two cloud sets as one autograd node"""

    @staticmethod
    def forward(ctx, A, B, cA, cB):
        ctx.counts = (cA, cB)
        ctx.set_materialize_grads(False)
        a, b = A.detach().contiguous(), B.detach().contiguous()
        ctx.save_for_backward(a, b)                                    # the two sets only: the match is recomputed
        return _pairs_forward(a, b, cA, cB)

    @staticmethod
    def backward(ctx, gD):
        cA, cB = ctx.counts
        A, B = ctx.saved_tensors
        needA, needB = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if gD is None or not (needA or needB):
            return (None,) * 4
        with torch.no_grad():
            dA, dB = _pairs_backward(A, B, cA, cB, gD.to(torch.float32).contiguous(), needA, needB)
        return dA, dB, None, None


class EMDPairs(torch.nn.Module):
    """emd_pairs as a differentiable module: gradients to cloudsA and cloudsB under any upstream gradient of D [P].  One autograd node
    over the library, on the current stream, without a host synchronisation; the forward values are bit for bit those of emd_pairs and
    the gradients those of EMDMatrix on each pair alone.  The match carries no gradient (as in earth_mover); the node saves the two sets
    only and the backward recomputes the match.  The gradient at a padded point is exactly +0.0; a set that needs no gradient gets None
    and its route is skipped.  Arguments and errors as emd_pairs."""

    def forward(self, cloudsA, cloudsB, *, countsA=None, countsB=None):
        want_grad = torch.is_grad_enabled() and any(torch.is_tensor(t) and t.requires_grad for t in (cloudsA, cloudsB))
        A, B, cA, cB = _prepare(cloudsA, cloudsB, countsA, countsB, cap=MAX_POINTS, pairs=True)
        if not want_grad:
            with torch.no_grad():
                return _pairs_forward(A, B, cA, cB)
        return _EMDPairsFn.apply(cloudsA, cloudsB, cA, cB)

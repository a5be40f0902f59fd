"""The baselines between two sets of clouds: the Chamfer and Hausdorff distance matrices of all pairs (include/dpdist_capi.h:
dpd_chamfer_matrix_fwd, dpd_chamfer_matrix_bwd), in the conventions of dpdist_matrix (dpdist_amd/pairwise.py), and the same distances
of the pairs (A_b, B_b) alone (dpd_chamfer_pairs_fwd, dpd_chamfer_pairs_bwd), in the conventions of dpdist_pairs.

    D_AB[i, j] = mean over the real points q of B_j of  min_p |q - A_i[p]|^2      (form "squared";  "sqrt": of the root of that minimum)
    D_BA[i, j] = mean over the real points q of A_i of  min_p |q - B_j[p]|^2
    D          = (D_AB + D_BA) / 2

so D[i, j] is aue.chamfer_dist(A_i, B_j) for the squared form and regtest.chamfer_sqrt(A_i, B_j) (PCRNet's form) for the sqrt form, and

    H[i, j]    = sqrt(max(max_AB[i, j], max_BA[i, j])),   max_AB[i, j] = max over the real points q of B_j of min_p |q - A_i[p]|^2

is the Hausdorff distance.  A is the surface of D_AB, as in dpdist_matrix.  Nothing of size [Ca, Cb, N] exists: a workgroup keeps one
surface cloud in LDS and walks query clouds past it.  Exact fp32, on the current stream, without a host synchronisation, no workspace.
Ragged sets (countsA / countsB) are those of dpdist_matrix: padding influences no bit and gets the gradient +0.0; here it is never read.
There is no fallback to expanded pairs.

chamfer_pairs / hausdorff_pairs / ChamferPairs: D[b] = D of the pair (A_b, B_b) with the definitions above, bit for bit the 1 x 1 matrix
of that pair, from kernels shaped for few, large pairs (a pair is spread over workgroups; the argmins [P, W] are kept for the backward).
"""
import torch

from . import lib as L
from .pairwise import _check_device, _check_shape, _host_counts

MAX_POINTS = 4096          # the C entries' cap: a surface cloud lives in LDS
FORMS = {"squared": 0, "sqrt": 1}


def _check(rc, what):
    if rc in (-2, -3):
        raise ValueError("%s refuses this shape: %s" % (what, L._ERR[rc]))
    L.check(rc, what)


def _form(form):
    if form not in FORMS:
        raise ValueError("form must be 'squared' or 'sqrt', got %r" % (form,))
    return FORMS[form]


class _ChamferPairedFn(torch.autograd.Function):
    """the batch-mean Chamfer loss of two full sets a [B,N,3], b [B,M,3] (dpd_chamfer_fwd / _bwd, or dpd_chamfer_sqrt_fwd / _bwd for the
    sqrt form) as one autograd node: the public names are aue.chamfer_dist and regtest.chamfer_sqrt"""

    @staticmethod
    def forward(ctx, a, b, form):
        for t, name in ((a, "a"), (b, "b")):
            L.req(t, name=name)
            if t.dim() != 3 or t.shape[2] != 3:
                raise RuntimeError("%s must be [B,N,3], got %s" % (name, tuple(t.shape)))
        if a.shape[0] != b.shape[0]:
            raise RuntimeError("a and b must hold the same number of clouds, got %d and %d" % (a.shape[0], b.shape[0]))
        ctx.entries = (("dpd_chamfer_fwd", "dpd_chamfer_bwd"), ("dpd_chamfer_sqrt_fwd", "dpd_chamfer_sqrt_bwd"))[_form(form)]
        B, N, M, dev = a.shape[0], a.shape[1], b.shape[1], a.device
        min_a, min_b = torch.empty(B, N, device=dev), torch.empty(B, M, device=dev)
        arg_a, arg_b = torch.empty(B, N, device=dev, dtype=torch.int32), torch.empty(B, M, device=dev, dtype=torch.int32)
        loss = torch.empty(1, device=dev)
        L.check(getattr(L.load(), ctx.entries[0])(L.ptr(a), L.ptr(b), B, N, M, L.ptr(min_a), L.ptr(arg_a), L.ptr(min_b), L.ptr(arg_b),
                                                  L.ptr(loss), L.cur_stream()), ctx.entries[0])
        ctx.save_for_backward(a, b, arg_a, arg_b)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        a, b, arg_a, arg_b = ctx.saved_tensors
        da = torch.empty_like(a) if ctx.needs_input_grad[0] else None
        db = torch.empty_like(b) if ctx.needs_input_grad[1] else None
        L.check(getattr(L.load(), ctx.entries[1])(L.ptr(a), L.ptr(b), a.shape[0], a.shape[1], b.shape[1], L.ptr(arg_a), L.ptr(arg_b), 1.0,
                                                  L.ptr(da), L.ptr(db), L.cur_stream()), ctx.entries[1])
        # the upstream gradient stays on the device (no host sync, any scalar-shaped g)
        return (None if da is None else da.mul_(g)), (None if db is None else db.mul_(g)), None


def _chamfer_paired(a, b, form):
    return _ChamferPairedFn.apply(a.contiguous(), b.contiguous(), form)


def _prepare(cloudsA, cloudsB, countsA, countsB, cap=MAX_POINTS, pairs=False):
    """every argument check, before anything is launched -> (A, B, cA, cB): contiguous fp32 sets and int32 device counts (None: a full
    set; B and cB are None for a set against itself); cap: the most points per cloud the caller's entries take; pairs: the sets are
    scored cloud by cloud (both are needed and must hold the same number of clouds) instead of all against all"""
    _check_shape(cloudsA, "cloudsA")
    if pairs:
        _check_shape(cloudsB, "cloudsB")
        if cloudsA.shape[0] != cloudsB.shape[0]:
            raise ValueError("cloudsA and cloudsB must hold the same number of clouds, got %d and %d" % (cloudsA.shape[0], cloudsB.shape[0]))
    elif cloudsB is not None:
        _check_shape(cloudsB, "cloudsB")
    elif countsB is not None:
        raise ValueError("countsB given without cloudsB (a set against itself takes countsA)")
    for t, name in ((cloudsA, "cloudsA"), (cloudsB, "cloudsB")):
        if t is not None and t.shape[1] > cap:
            raise ValueError("%s holds %d points per cloud, the cap is %d" % (name, t.shape[1], cap))
    if not pairs and cloudsA.shape[0] * (cloudsA if cloudsB is None else cloudsB).shape[0] >= 1 << 31:
        raise ValueError("the matrix must hold fewer than 2^31 pairs")
    cA = _host_counts(countsA, cloudsA.shape[0], cloudsA.shape[1], "countsA")
    cB = None if cloudsB is None else _host_counts(countsB, cloudsB.shape[0], cloudsB.shape[1], "countsB")
    A = _check_device(cloudsA, "cloudsA")
    B = None if cloudsB is None else _check_device(cloudsB, "cloudsB")
    if B is not None and B.device != A.device:
        raise ValueError("cloudsA and cloudsB must live on the same device")
    for c, name in ((cA, "countsA"), (cB, "countsB")):
        if c is not None and c.is_cuda and c.device != A.device:
            raise ValueError("%s and the clouds must live on the same device" % name)
    cA = None if cA is None else cA.to(A.device).contiguous()
    cB = None if cB is None else cB.to(A.device).contiguous()
    return A, B, cA, cB


def _directed(lib, s, S, cS, Q, cQ, want):
    """one launch: surface set S against query set Q -> the outputs named in `want` (of "mean_sq", "mean_rt", "max_sq"), each [Cs, Cq]"""
    out = {n: torch.empty(S.shape[0], Q.shape[0], device=S.device, dtype=torch.float32) for n in want}
    _check(lib.dpd_chamfer_matrix_fwd(L.ptr(S), L.ptr(cS), S.shape[0], S.shape[1], L.ptr(Q), L.ptr(cQ), Q.shape[0], Q.shape[1],
                                      L.ptr(out.get("mean_sq")), L.ptr(out.get("mean_rt")), L.ptr(out.get("max_sq")), s),
           "dpd_chamfer_matrix_fwd")
    return [out[n] for n in want]


def _both(A, B, cA, cB, name):
    """(X_AB, X_BA), both [Ca, Cb], of one output of the forward entry; a set against itself runs one direction"""
    lib = L.load()
    with torch.cuda.device(A.device):
        s = L.cur_stream()
        ab, = _directed(lib, s, A, cA, A if B is None else B, cA if B is None else cB, (name,))
        if B is None:
            return ab, ab.t().contiguous()
        ba, = _directed(lib, s, B, cB, A, cA, (name,))          # the same code with the sets swapped: [Cb, Ca]
        return ab, ba.t().contiguous()


def _chamfer_forward(A, B, cA, cB, form):
    d_ab, d_ba = _both(A, B, cA, cB, ("mean_sq", "mean_rt")[form])
    return (d_ab + d_ba) / 2, d_ab, d_ba


@torch.no_grad()
def chamfer_matrix(cloudsA, cloudsB=None, form="squared", return_directed=False, *, countsA=None, countsB=None):
    """cloudsA [Ca,N,3], cloudsB [Cb,M,3] (None: cloudsA against itself, from one direction) -> the Chamfer matrix D [Ca,Cb], or
    (D, D_AB, D_BA) with return_directed.  form "squared": mean squared nearest distances (aue.chamfer_dist of every pair); "sqrt": mean
    nearest distances (regtest.chamfer_sqrt, PCRNet's form).  D_AB[i,j] averages over the points of B_j their nearest distance to A_i.
    The two sets may have different widths.  countsA / countsB (keywords): ragged sets as in dpdist_matrix -- a sequence or CPU integer
    tensor is checked (one count per cloud, each in [1, width]) and copied once, an int32 device tensor is used as it is and clamped by
    the kernels; padding is never read.  ValueError for CPU tensors, a dtype other than float32, sets on two devices, bad counts, countsB
    without cloudsB and more than 4096 points per cloud -- before anything is launched.  Forward only: ChamferMatrix is differentiable."""
    f = _form(form)
    A, B, cA, cB = _prepare(cloudsA, cloudsB, countsA, countsB)
    D, d_ab, d_ba = _chamfer_forward(A, B, cA, cB, f)
    return (D, d_ab, d_ba) if return_directed else D


@torch.no_grad()
def hausdorff_matrix(cloudsA, cloudsB=None, return_directed=False, *, countsA=None, countsB=None):
    """The Hausdorff matrix H [Ca,Cb] = sqrt(max(max_AB, max_BA)), or (H, H_AB, H_BA) with return_directed, where H_AB[i,j] is the largest
    nearest distance to A_i of a point of B_j and H_BA[i,j] the largest nearest distance to B_j of a point of A_i (the directed
    Hausdorff distances, square roots of the entry's max_sq).  Arguments, ragged sets and errors as chamfer_matrix.  FORWARD ONLY: there
    is no differentiable form (the maximum's gradient reaches one point of a pair)."""
    A, B, cA, cB = _prepare(cloudsA, cloudsB, countsA, countsB)
    m_ab, m_ba = _both(A, B, cA, cB, "max_sq")
    H = torch.sqrt(torch.maximum(m_ab, m_ba))
    return (H, torch.sqrt(m_ab), torch.sqrt(m_ba)) if return_directed else H


def _directed_bwd(lib, s, S, cS, Q, cQ, form, W, need_s, need_q):
    """one direction of the backward: W [Cs, Cq] is the upstream of that direction's mean -> (surface route | None, query route | None)"""
    gS = torch.empty_like(S) if need_s else None
    gQ = torch.empty_like(Q) if need_q else None
    if need_s or need_q:
        _check(lib.dpd_chamfer_matrix_bwd(L.ptr(S), L.ptr(cS), S.shape[0], S.shape[1], L.ptr(Q), L.ptr(cQ), Q.shape[0], Q.shape[1], form,
                                          L.ptr(W), L.ptr(gS), L.ptr(gQ), s), "dpd_chamfer_matrix_bwd")
    return gS, gQ


class _ChamferMatrixFn(torch.autograd.Function):
    """(D, D_AB, D_BA) of two cloud sets as one autograd node; B is None for a set against itself"""

    @staticmethod
    def forward(ctx, A, B, form, cA, cB):
        ctx.cfg = (form, B is None)
        ctx.counts = (cA, cB)
        ctx.set_materialize_grads(False)
        a = A.detach().contiguous()
        b = None if B is None else B.detach().contiguous()
        ctx.save_for_backward(*((a,) if b is None else (a, b)))        # the two sets only: the argmins are recomputed
        return _chamfer_forward(a, b, cA, cB, form)

    @staticmethod
    def backward(ctx, gD, gAB, gBA):
        form, self_matrix = ctx.cfg
        cA, cB = ctx.counts
        A = ctx.saved_tensors[0]
        B = A if self_matrix else ctx.saved_tensors[1]
        needA = ctx.needs_input_grad[0]
        needB = (not self_matrix) and ctx.needs_input_grad[1]
        if (gD is None and gAB is None and gBA is None) or not (needA or needB):
            return (None,) * 5

        def upstream(*terms):
            terms = [t for t in terms if t is not None]
            return sum(terms[1:], terms[0]).to(torch.float32).contiguous() if terms else None

        # D = (D_AB + D_BA) / 2: W_ab = G / 2 + G_ab for the direction (surface A, query B), W_ba = (G / 2 + G_ba)^T for (surface B, query A)
        half = None if gD is None else gD / 2
        w_ab = upstream(half, gAB)
        w_ba = upstream(half, gBA)
        w_ba = None if w_ba is None else w_ba.t().contiguous()
        lib = L.load()
        with torch.cuda.device(A.device), torch.no_grad():
            s = L.cur_stream()
            both = lambda x, y: y if x is None else (x if y is None else x + y)   # noqa: E731
            if self_matrix:
                # D_BA = D_AB^T came from the one direction (surface A, query A): its upstream is W_ab + W_ba, both routes land in A
                gs_, gq_ = _directed_bwd(lib, s, A, cA, A, cA, form, both(w_ab, w_ba), True, True)
                return gs_ + gq_, None, None, None, None
            sA = qB = sB = qA = None
            if w_ab is not None:
                sA, qB = _directed_bwd(lib, s, A, cA, B, cB, form, w_ab, needA, needB)
            if w_ba is not None:
                sB, qA = _directed_bwd(lib, s, B, cB, A, cA, form, w_ba, needB, needA)
        return both(sA, qA), both(qB, sB), None, None, None


class ChamferMatrix(torch.nn.Module):
    """chamfer_matrix as a differentiable module: gradients to cloudsA and cloudsB under any upstream gradient of D [Ca, Cb] and, with
    return_directed, of D_AB and D_BA.  One autograd node over the library, on the current stream, without a host synchronisation; the
    forward values are bit for bit those of chamfer_matrix.  The node saves the two sets only and recomputes the argmins in the backward
    (ties go to the lowest index).  Each set's gradient is its surface route from one direction plus its query route from the other;
    cloudsB = None runs one direction whose upstream is G/2 + G_ab + (G/2 + G_ba)^T.  form "sqrt": a pair of coincident points
    contributes exactly zero (the reference's gradient is NaN there; regtest.chamfer_sqrt deviates in the same way).  The gradient at a
    padded point is exactly +0.0; a set that needs no gradient gets None and its route is skipped.  Arguments and errors as
    chamfer_matrix."""

    def __init__(self, form="squared"):
        super().__init__()
        self.form = form
        self._form = _form(form)

    def forward(self, cloudsA, cloudsB=None, return_directed=False, *, countsA=None, countsB=None):
        want_grad = torch.is_grad_enabled() and any(torch.is_tensor(t) and t.requires_grad for t in (cloudsA, cloudsB))
        A, B, cA, cB = _prepare(cloudsA, cloudsB, countsA, countsB)
        if not want_grad:
            with torch.no_grad():
                D, d_ab, d_ba = _chamfer_forward(A, B, cA, cB, self._form)
        else:
            D, d_ab, d_ba = _ChamferMatrixFn.apply(cloudsA, cloudsB, self._form, cA, cB)
        return (D, d_ab, d_ba) if return_directed else D


def _pairs_forward(A, B, cA, cB, want):
    """one dpd_chamfer_pairs_fwd call -> ({name: [2, P]} for the names in `want`, (arg_ab [P,Wb], arg_ba [P,Wa]))"""
    lib = L.load()
    P, Wa, Wb = A.shape[0], A.shape[1], B.shape[1]
    dev = A.device
    out = {n: torch.empty(2, P, device=dev, dtype=torch.float32) for n in want}
    min_ab, min_ba = torch.empty(P, Wb, device=dev, dtype=torch.float32), torch.empty(P, Wa, device=dev, dtype=torch.float32)
    arg_ab, arg_ba = torch.empty(P, Wb, device=dev, dtype=torch.int32), torch.empty(P, Wa, device=dev, dtype=torch.int32)
    with torch.cuda.device(dev):
        _check(lib.dpd_chamfer_pairs_fwd(L.ptr(A), L.ptr(cA), Wa, L.ptr(B), L.ptr(cB), Wb, P, L.ptr(min_ab), L.ptr(arg_ab), L.ptr(min_ba),
                                         L.ptr(arg_ba), L.ptr(out.get("mean_sq")), L.ptr(out.get("mean_rt")), L.ptr(out.get("max_sq")),
                                         L.cur_stream()), "dpd_chamfer_pairs_fwd")
    return out, (arg_ab, arg_ba)


def _chamfer_pairs_forward(A, B, cA, cB, form):
    out, args = _pairs_forward(A, B, cA, cB, (("mean_sq", "mean_rt")[form],))
    d = out[("mean_sq", "mean_rt")[form]]
    return ((d[0] + d[1]) / 2, d[0], d[1]), args


@torch.no_grad()
def chamfer_pairs(cloudsA, cloudsB, form="squared", return_directed=False, *, countsA=None, countsB=None):
    """cloudsA [P,N,3], cloudsB [P,M,3] -> the Chamfer distance D [P] of the pairs (A_b, B_b), or (D, D_AB, D_BA) with return_directed:
    D[b] is chamfer_matrix(A[b:b+1], B[b:b+1])[0, 0] with the same counts, bit for bit (form "squared": aue.chamfer_dist of the pair,
    "sqrt": regtest.chamfer_sqrt).  D_AB[b] averages over the real points of B_b their nearest distance to A_b.  The two sets may have
    different widths.  countsA / countsB (keywords): ragged sets as in dpdist_pairs -- a sequence or CPU integer tensor is checked (one
    count per cloud, each in [1, width]) and copied once, an int32 device tensor is used as it is and clamped by the kernels; padding is
    never read.  ValueError for sets of different lengths, CPU tensors, a dtype other than float32, sets on two devices, bad counts and
    more than 4096 points per cloud -- before anything is launched.  Forward only: ChamferPairs is differentiable."""
    f = _form(form)
    A, B, cA, cB = _prepare(cloudsA, cloudsB, countsA, countsB, pairs=True)
    (D, d_ab, d_ba), _ = _chamfer_pairs_forward(A, B, cA, cB, f)
    return (D, d_ab, d_ba) if return_directed else D


@torch.no_grad()
def hausdorff_pairs(cloudsA, cloudsB, return_directed=False, *, countsA=None, countsB=None):
    """The Hausdorff distance H [P] = sqrt(max(max_AB, max_BA)) of the pairs (A_b, B_b), or (H, H_AB, H_BA) with return_directed: bit for
    bit hausdorff_matrix of each pair alone.  Arguments, ragged sets and errors as chamfer_pairs.  FORWARD ONLY, as hausdorff_matrix."""
    A, B, cA, cB = _prepare(cloudsA, cloudsB, countsA, countsB, pairs=True)
    m = _pairs_forward(A, B, cA, cB, ("max_sq",))[0]["max_sq"]
    H = torch.sqrt(torch.maximum(m[0], m[1]))
    return (H, torch.sqrt(m[0]), torch.sqrt(m[1])) if return_directed else H


class _ChamferPairsFn(torch.autograd.Function):
    """(D, D_AB, D_BA) [P] of the pairs of two cloud sets as one autograd node"""

    @staticmethod
    def forward(ctx, A, B, form, cA, cB):
        ctx.form = form
        ctx.counts = (cA, cB)
        ctx.set_materialize_grads(False)
        a, b = A.detach().contiguous(), B.detach().contiguous()
        out, (arg_ab, arg_ba) = _chamfer_pairs_forward(a, b, cA, cB, form)
        ctx.save_for_backward(a, b, arg_ab, arg_ba)                    # the argmins are [P, W]: kept, not recomputed
        return out

    @staticmethod
    def backward(ctx, gD, gAB, gBA):
        cA, cB = ctx.counts
        A, B, arg_ab, arg_ba = ctx.saved_tensors
        needA, needB = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if (gD is None and gAB is None and gBA is None) or not (needA or needB):
            return (None,) * 5

        def upstream(*terms):
            terms = [t for t in terms if t is not None]
            return sum(terms[1:], terms[0]).to(torch.float32).contiguous() if terms else None

        # D = (D_AB + D_BA) / 2: G_ab = G / 2 + G_ab, G_ba = G / 2 + G_ba, as ChamferMatrix forms them
        half = None if gD is None else gD / 2
        g_ab, g_ba = upstream(half, gAB), upstream(half, gBA)
        lib = L.load()
        dA = torch.empty_like(A) if needA else None
        dB = torch.empty_like(B) if needB else None
        with torch.cuda.device(A.device), torch.no_grad():
            _check(lib.dpd_chamfer_pairs_bwd(L.ptr(A), L.ptr(cA), A.shape[1], L.ptr(B), L.ptr(cB), B.shape[1], A.shape[0], ctx.form,
                                             L.ptr(arg_ab), L.ptr(arg_ba), L.ptr(g_ab), L.ptr(g_ba), L.ptr(dA), L.ptr(dB), L.cur_stream()),
                   "dpd_chamfer_pairs_bwd")
        return dA, dB, None, None, None


class ChamferPairs(torch.nn.Module):
    """chamfer_pairs as a differentiable module: gradients to cloudsA and cloudsB under any upstream gradient of D [P] and, with
    return_directed, of D_AB and D_BA.  One autograd node over the library, on the current stream, without a host synchronisation; the
    forward values are bit for bit those of chamfer_pairs and the gradients those of ChamferMatrix on each pair alone.  The node saves
    the two sets and the argmins [P, W] of the forward (ties go to the lowest index).  Each set's gradient is its surface route from one
    direction plus its query route from the other, written by one kernel.  form "sqrt": a pair of coincident points contributes exactly
    zero, as in ChamferMatrix.  The gradient at a padded point is exactly +0.0; a set that needs no gradient gets None and its route is
    skipped.  Arguments and errors as chamfer_pairs."""

    def __init__(self, form="squared"):
        super().__init__()
        self.form = form
        self._form = _form(form)

    def forward(self, cloudsA, cloudsB, return_directed=False, *, countsA=None, countsB=None):
        want_grad = torch.is_grad_enabled() and any(torch.is_tensor(t) and t.requires_grad for t in (cloudsA, cloudsB))
        A, B, cA, cB = _prepare(cloudsA, cloudsB, countsA, countsB, pairs=True)
        if not want_grad:
            with torch.no_grad():
                D, d_ab, d_ba = _chamfer_pairs_forward(A, B, cA, cB, self._form)[0]
        else:
            D, d_ab, d_ba = _ChamferPairsFn.apply(cloudsA, cloudsB, self._form, cA, cB)
        return (D, d_ab, d_ba) if return_directed else D

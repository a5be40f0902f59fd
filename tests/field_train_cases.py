"""Decoder gradients of the per-point field (csrc/field_train.hip: dpd_field_bwd_train; DPDistField(backward="slots", decoder_grad=True)):
the float64 autograd oracle for the eight decoder variables in the flat layout of DPDistParams, its bars, the numpy restatement of the
slot form of layer 1's weight gradient, and the oracle's fitting trajectory, for tests/test_field_train_gpu.py;
tests/test_field_train_cpu.py runs the admissions here without a GPU.  The case, the decoder, the upstream gradient and the constants are
those of tests/field_cases.py (imported, not restated); the composition is its _field with weights that require grad.  Not a test module
and not a conftest.
"""
import functools

import numpy as np
import torch

from dpdist_amd import synth
from oracle import restate as R

from . import field_cases as FC
from . import field_slots_cases as FS

M_GRID, K_WIN, H_DEC, KP, NG, E = FC.M_GRID, FC.K_WIN, FC.H_DEC, FC.KP, FC.NG, FC.E
NAMES = ("W1p", "b1", "W2", "b2", "W3", "b3", "W4", "b4")
TF_NAME = "pc_compare/dpdist_local/mapper_conv%d/%s"
N_REAL = sum(FC.QCOUNTS)      # 248 real queries


def tf_weights():
    """the decoder of tests/test_cross_gpu.py under the TF names (numpy)"""
    return synth.make_weights("wide", mlp=(H_DEC,) * 3)


def to_flat_layout(sd):
    """TF name -> array (weights or gradients, any float type) -> the eight blocks of DPDistParams' flat layout as float64 numpy arrays, by
    the conventions of DPDistParams.load_tf_state_dict: W1p [KP, H] = window rows first, the three q - centre rows after, zero pad rows"""
    get = lambda l, t: np.asarray(sd[TF_NAME % (l, t)].detach().double().numpy() if torch.is_tensor(sd[TF_NAME % (l, t)])     # noqa: E731
                                  else sd[TF_NAME % (l, t)], dtype=np.float64)
    w1 = get(1, "weights").reshape(E + 3, H_DEC)
    W1p = np.zeros((KP, H_DEC))
    W1p[:E], W1p[E:E + 3] = w1[3:], w1[:3]
    return {"W1p": W1p, "b1": get(1, "biases"), "W2": get(2, "weights").reshape(H_DEC, H_DEC), "b2": get(2, "biases"),
            "W3": get(3, "weights").reshape(H_DEC, H_DEC), "b3": get(3, "biases"), "W4": get(4, "weights").reshape(H_DEC, 3),
            "b4": get(4, "biases")}


def _rows(dtype, shared):
    """the decoder's input rows of the reference case, built once per dtype as tests/field_cases.py: _field builds them (the rows do not
    depend on the decoder) -> (X [248, 3 + E] in the oracle's column order, mask [248], upstream [248, 3], labels [248])"""
    S, _, Q = FC._leaves(dtype, shared, False)
    up = torch.tensor(FC.upstream(), dtype=dtype)
    rows, masks, ups, labels = [], [], [], []
    with torch.no_grad():
        for c, (s, q) in enumerate(zip(S, Q)):
            emb = R.local_window(R.mfv3d(s[None], M_GRID, 0.125), M_GRID, K_WIN)[0]
            v, mask, loc = R.voxel_lookup(q[None], M_GRID)
            rows.append(torch.cat([loc[0], emb[v[0]]], -1))
            masks.append(mask[0])
            ups.append(up[c, :q.shape[0]])
            labels.append(torch.cdist(q.double(), s.double()).min(1).values.to(dtype))      # float64 nearest distance to the truncated cloud
    return torch.cat(rows), torch.cat(masks), torch.cat(ups), torch.cat(labels)


@functools.lru_cache(maxsize=None)
def rows(dtype, shared=False):
    return _rows(dtype, shared)


def pred_of(W, dtype, shared=False):
    """pred [248, 3] of the oracle at the weights W (TF name -> tensor), with its graph: tests/field_cases.py: _field, row for row"""
    X, mask, _, _ = rows(dtype, shared)
    y, _ = R.decoder(X, W)
    return y * mask[:, None]


def weight_grads(dtype, shared=False, weights=None):
    """gradients of (upstream * pred).sum() w.r.t. the eight variables, the oracle run in `dtype` at `weights` (TF name -> numpy; None:
    tf_weights()) -> name -> float64 numpy array in the flat layout"""
    W = R.as_torch_weights(tf_weights() if weights is None else weights, dtype, requires_grad=True)
    names = sorted(W)
    loss = (pred_of(W, dtype, shared) * rows(dtype, shared)[2]).sum()
    return to_flat_layout(dict(zip(names, torch.autograd.grad(loss, [W[n] for n in names]))))


@functools.lru_cache(maxsize=None)
def oracle_weight_grads(dtype, shared=False):
    return weight_grads(dtype, shared)


def weight_bars(shared=False, weights=None):
    """name -> (ref, bar), formed per variable as tests/field_cases.py: grad_bars forms them"""
    if weights is None:
        r64, r32 = oracle_weight_grads(torch.float64, shared), oracle_weight_grads(torch.float32, shared)
    else:
        r64, r32 = weight_grads(torch.float64, shared, weights), weight_grads(torch.float32, shared, weights)
    return {n: (r64[n], max(4.0 * np.abs(r32[n] - r64[n]).max(), 2e-4 * max(1.0, np.abs(r64[n]).max()))) for n in NAMES}


# ------------------------------------------------------------------------------------------------ the slot form of dW1, restated
def restated_dW1(tile=None):
    """dW1p [KP, H] of the reference case (own queries) as the library forms it, in float64 from the oracle's g1 rows: per cloud and per
    tile of `tile` queries (None: the whole cloud) the restated index of tests/field_slots_cases.py, gs = the slot sums, Xu [KP - 32, U] =
    the first KP - 32 window values of every slot, Xt [t, 32] = the window's last values, q - centre and the zero pad of every row;
    dW1p = [Xu gs ; Xt^T g1], the tiles and clouds added in ascending order"""
    S, _, Q = FC._leaves(torch.float64, False, True)
    up = torch.tensor(FC.upstream(), dtype=torch.float64)
    out = np.zeros((KP, H_DEC))
    for c, (s, q) in enumerate(zip(S, Q)):
        t_all = q.shape[0]
        vox, g1, _, fv = FS.oracle_rows(s, q.detach(), up[c, :t_all])
        emb = R.local_window(fv, M_GRID, K_WIN)[0].detach().numpy()                   # [m^3, E]
        loc = R.voxel_lookup(q.detach()[None], M_GRID)[2][0].numpy()                  # [t, 3] q - centre
        step = t_all if tile is None else tile
        for t0 in range(0, t_all, step):
            inv = FS.invert(vox[None, t0:t0 + step])
            g = g1[t0:t0 + step]
            gs = FS.slot_sum(g, inv)[:inv["total"]]
            win = emb[inv["slot_vox"][:inv["total"]]]                                 # [U, E]
            Xt = np.zeros((g.shape[0], 32))
            Xt[:, :E - (KP - 32)] = emb[vox[t0:t0 + step]][:, KP - 32:]
            Xt[:, E - (KP - 32):E + 3 - (KP - 32)] = loc[t0:t0 + step]
            out[:KP - 32] += win[:, :KP - 32].T @ gs
            out[KP - 32:] += Xt.T @ g
    return out


# ------------------------------------------------------------------------------------------------ fitting trajectory
STEPS, LR = 10, 1e-4


def trajectory(dtype, steps=STEPS, lr=LR):
    """`steps` TF-Adam steps (oracle.restate.adam_tf_step) on loss = mean |pred[:, 0] - label| over the 248 real queries, labels = the
    float64 nearest distance to the truncated cloud -> the loss before every step"""
    W = R.as_torch_weights(tf_weights(), dtype, requires_grad=True)
    names = sorted(W)
    label = rows(dtype)[3]
    m = {n: np.zeros(tuple(W[n].shape)) for n in names}
    v = {n: np.zeros(tuple(W[n].shape)) for n in names}
    out = []
    for t in range(1, steps + 1):
        loss = (pred_of(W, dtype)[:, 0] - label).abs().mean()
        out.append(float(loss.detach()))
        grads = torch.autograd.grad(loss, [W[n] for n in names])
        with torch.no_grad():
            for n, g in zip(names, grads):
                p = W[n].detach().double().numpy().copy()
                R.adam_tf_step(p, g.double().numpy(), m[n], v[n], t, lr)
                W[n].copy_(torch.tensor(p, dtype=dtype))
    return out


def labels_padded():
    """(labels [3, 150], real [3, 150]) as float32 numpy arrays: zeros on the padding"""
    lab, real = np.zeros((3, FC.T_REF), dtype=np.float32), np.zeros((3, FC.T_REF), dtype=np.float32)
    flat, o = rows(torch.float64)[3].numpy(), 0
    for c, n in enumerate(FC.QCOUNTS):
        lab[c, :n], real[c, :n] = flat[o:o + n], 1.0
        o += n
    return lab, real

"""Decoder gradients of the per-point field, the part that needs no GPU: the admission of the float32 oracle for the eight decoder
gradients (so that the bars of the GPU test are the project's 2e-4 relative ones), the numpy restatement of the slot form of layer 1's
weight gradient against the autograd oracle, the oracle's fitting trajectory, the exported symbols, every refusal of the new C entry
(none of which touches a device) and of the `decoder_grad` keyword.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from dpdist_amd import lib as L

from . import field_cases as FC
from . import field_train_cases as FT

E_NULL, E_DIM, E_UNSUPPORTED, E_WORKSPACE = -1, -2, -3, -4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dpd_field_bwd_train", "dpd_field_bwd_train_workspace_bytes")
KP = FC.KP


def test_composition_is_the_field_oracle():
    """the rows built once and run through the decoder are tests/field_cases.py: _field, cloud by cloud (one product over all 248 rows
    instead of one per cloud: the same values up to the blocking of the host's matrix product)"""
    for dtype, tol in ((torch.float64, 1e-12), (torch.float32, 1e-5)):
        W = FT.R.as_torch_weights(FT.tf_weights(), dtype)
        with torch.no_grad():
            got = FT.pred_of(W, dtype).double().numpy()
        want = np.concatenate([FC.oracle(dtype)[0][c, :n] for c, n in enumerate(FC.QCOUNTS)])
        assert got.shape == (FT.N_REAL, 3) and np.abs(got - want).max() <= tol and np.abs(want).max() > 1.0


@pytest.mark.parametrize("shared", [False, True])
def test_admission_of_the_weight_gradients(shared):
    """float32 autograd oracle within ADMIT_GRAD * max(1, max |g64|) of float64 for all eight gradients; gradients with structure; the zero
    pad rows of W1p get none"""
    r64, r32 = FT.oracle_weight_grads(torch.float64, shared), FT.oracle_weight_grads(torch.float32, shared)
    for n in FT.NAMES:
        err, top = np.abs(r32[n] - r64[n]).max(), np.abs(r64[n]).max()
        print("shared %s: g %s |g32 - g64| max %.3g at max |g64| %.3g (relative %.3g)" % (shared, n, err, top, err / max(1.0, top)))
        assert err <= FC.ADMIT_GRAD * max(1.0, top) and top > 1e-2, n
    for n, (ref, bar) in FT.weight_bars(shared).items():
        print("shared %s: bar of %s %.3g" % (shared, n, bar))
        assert np.abs(ref).max() > 20 * bar and 2e-4 <= bar <= 1e-2, n
    assert not r64["W1p"][FC.E + 3:].any() and r64["W1p"].shape == (KP, FC.H_DEC)


@pytest.mark.parametrize("tile", [None, 64])
def test_slot_form_of_dW1_reproduces_the_autograd_oracle(tile):
    """Xu gs + Xt^T g1 on the restated index, composed in float64 with the oracle's g1 rows, for whole clouds and for tiles of 64: the
    oracle's dW1 in the flat layout, to float64 rounding"""
    got, ref = FT.restated_dW1(tile), FT.oracle_weight_grads(torch.float64)["W1p"]
    err, top = np.abs(got - ref).max(), np.abs(ref).max()
    print("tile %s: dW1p restated vs autograd: %.3e at max |ref| %.3e" % (tile, err, top))
    assert got.shape == ref.shape and top > 1e-2 and err <= 1e-10 * max(1.0, top)
    assert not got[FC.E + 3:].any()


def test_trajectory_of_the_oracle():
    """ten TF-Adam steps at lr 1e-4: the float32 oracle stays within a thousandth of the forward bar of float64, and the loss falls by at
    least 0.006 per step, 60 times the bar the GPU test holds the library to"""
    a, b = FT.trajectory(torch.float64), FT.trajectory(torch.float32)
    print("float64", ["%.5f" % x for x in a])
    print("max |f32 - f64| %.3g" % max(abs(x - y) for x, y in zip(a, b)))
    assert len(a) == FT.STEPS and max(abs(x - y) for x, y in zip(a, b)) <= FC.FWD_BAR / 100
    assert all(x - y >= 0.006 for x, y in zip(a, a[1:])) and 0.4 < a[0] < 0.5


def test_new_symbols_are_exported_and_declared():
    from dpdist_amd import build
    build.build(verbose=False)
    lib = L.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dpdist_capi.h")).read(), flags=re.S)
    for name in NEW:
        assert hasattr(lib, name) and name in L.SIGNATURES and re.search(r"\b%s\s*\(" % name, header), name
    assert "field_train.hip" in build.SOURCES


def test_entry_refuses_bad_arguments_without_a_device():
    """every DPD_E_* path of dpd_field_bwd_train, before anything is launched: the pointers are never dereferenced"""
    lib = L.load()
    p = ctypes.c_void_p(1 << 30)
    cp = L.DecoderParams(*([1 << 30] * 11))
    wsb = lib.dpd_field_bwd_train_workspace_bytes
    need = wsb(3, 150, 8, 5, KP, 256)
    grads = (KP * 256 + 256 + 2 * (256 * 256 + 256) + 3 * 256 + 3) * 4
    assert need % 256 == 0 and grads < need < 3 * grads
    assert wsb(0, 150, 8, 5, KP, 256) == 0 and wsb(3, 150, 11, 5, KP, 256) == 0 and wsb(3, 150, 8, 4, KP, 256) == 0
    assert wsb(3, 150, 8, 5, KP, 200) == 0 and wsb(3, 150, 8, 5, KP, 4160) == 0 and wsb(3, 150, 8, 5, KP + 32, 256) == 0

    def call(dpred=p, dfv=p, gq=p, gs=p, dq=p, ucount=p, xu=p, xt=p, ldu=480, params=cp, n=3, T=150, cap=480, h=256, k=5, m=8, stride=450,
             w=(p,) * 8, ws=p, ws_bytes=need):
        return lib.dpd_field_bwd_train(dpred, p, p, p, p, p, p, ucount, p, p, p, p, xu, ldu, xt, n, T, m, k, KP, h, cap, params, p, p, p, dq, gs, p,
                                       dfv, 0, gq, stride, *w, 0, ws, ws_bytes, None)
    assert call(dpred=None) == E_NULL and call(params=None) == E_NULL and call(xu=None) == E_NULL and call(xt=None) == E_NULL
    assert call(gs=None) == E_NULL and call(gs=None, dfv=None) == E_NULL          # gs is formed for the weight gradient in any case
    assert call(ws=None) == E_NULL and call(ucount=None) == E_NULL and call(dq=None, stride=0) == E_NULL
    for i in range(8):                                                              # all eight outputs, or none
        assert call(w=(p,) * i + (None,) + (p,) * (7 - i)) == E_NULL, i
    assert call(w=(None,) * 8, dfv=None, gq=None) == E_NULL                         # nothing wanted at all (dpd_field_bwd's refusal)
    assert call(params=L.DecoderParams(*([1 << 30] * 8 + [None] * 3))) == E_NULL    # the surface route needs the transposed W1p
    assert call(params=L.DecoderParams(*([None] * 11))) == E_NULL
    assert call(n=0) == E_DIM and call(T=0) == E_DIM and call(cap=448) == E_DIM and call(cap=512) == E_DIM and call(h=0) == E_DIM
    assert call(stride=449) == E_DIM and call(stride=-1) == E_DIM and call(ldu=476) == E_DIM and call(ldu=0) == E_DIM
    for kw in (dict(h=200), dict(h=4160), dict(k=4), dict(m=11), dict(ldu=482), dict(n=830, T=600, cap=830 * 512, ldu=830 * 512, h=64, stride=1800),
               dict(n=1, T=1 << 22, cap=512, ldu=512, h=1024, stride=3 << 22)):
        assert call(**kw) == E_UNSUPPORTED, kw
    # Xu [KP - 32, ldu] beyond the GEMMs' 32-bit byte offsets through its row stride alone
    assert (KP - 32) * 430184 * 4 < 1 << 32 <= (KP - 32) * 430188 * 4 and call(ldu=430188) == E_UNSUPPORTED
    assert call(ws_bytes=need - 1) == E_WORKSPACE and call(ws_bytes=0) == E_WORKSPACE
    assert call(dfv=None, gq=None, ws_bytes=need - 1) == E_WORKSPACE               # the weights alone: checked the same way


class _Params:
    """what _resolve and _prepare read of a DPDistParams, without a device"""
    flat, KP, H, k, compute_dtype = torch.zeros(1), FC.KP, FC.H_DEC, FC.K_WIN, "f32"


def test_decoder_grad_keyword():
    from dpdist_amd import DPDistField
    assert DPDistField(_Params()).decoder_grad is False and DPDistField(_Params(), backward="slots").decoder_grad is False
    assert DPDistField(_Params(), backward="slots", decoder_grad=True).decoder_grad is True
    for kw in (dict(backward="rows"), dict()):
        with pytest.raises(ValueError, match="decoder_grad.*backward"):
            DPDistField(_Params(), decoder_grad=True, **kw)
    S, Q = torch.tensor(FC.surfaces()), torch.tensor(FC.queries())
    with pytest.raises(ValueError, match="GPU"):             # the checks of the forward come first
        DPDistField(_Params(), backward="slots", decoder_grad=True)(S, Q)

"""The four paired Chamfer entries (csrc/chamfer.hip) through the C ABI against the numpy float32 restatement of tests/chamfer_cases.py:
EQUAL BIT PATTERNS of min_*, arg_*, loss, da and db for both forms.  The restatement follows the kernels' order of operations and was
first run against the two separate implementations the entries had before they were merged; nothing here is a tolerance."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from dpdist_amd import lib as L

from . import chamfer_cases as C

pytestmark = pytest.mark.gpu

G = 256                        # guard band (elements) on either side of every output
ENTRY = {"squared": ("dpd_chamfer_fwd", "dpd_chamfer_bwd"), "sqrt": ("dpd_chamfer_sqrt_fwd", "dpd_chamfer_sqrt_bwd")}


class Banded:
    """an output buffer of `shape` between two guard bands, prefilled with a pattern no entry writes"""

    def __init__(self, shape, dtype=torch.float32):
        self.n, self.shape = int(np.prod(shape)), shape
        self.buf = torch.full((self.n + 2 * G,), -7, device="cuda", dtype=dtype)
        self.ptr = ctypes.c_void_p(self.buf.data_ptr() + 4 * G)

    def get(self):
        assert (self.buf[:G] == -7).all() and (self.buf[G + self.n:] == -7).all(), "guard band overwritten"
        return self.buf[G:G + self.n].view(*self.shape).cpu().numpy()

    def untouched(self):
        return bool((self.buf == -7).all())


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def same_bits(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    bad = np.argwhere(bits(got) != bits(want))
    assert len(bad) == 0, (what, len(bad), bad[:4].tolist(), [(got[tuple(i)], want[tuple(i)]) for i in bad[:4]])


@functools.lru_cache(maxsize=None)
def device_inputs(name):
    return tuple(torch.from_numpy(np.array(x)).cuda() for x in C.inputs(name))


@functools.lru_cache(maxsize=None)
def gpu_forward(name, form):
    a, b = device_inputs(name)
    B, N, M = C.CASES[name][:3]
    out = {"min_a": Banded((B, N)), "arg_a": Banded((B, N), torch.int32), "min_b": Banded((B, M)), "arg_b": Banded((B, M), torch.int32),
           "loss": Banded((1,))}
    L.check(getattr(L.load(), ENTRY[form][0])(L.ptr(a), L.ptr(b), B, N, M, out["min_a"].ptr, out["arg_a"].ptr, out["min_b"].ptr,
                                              out["arg_b"].ptr, out["loss"].ptr, L.cur_stream()), ENTRY[form][0])
    return {q: v.get() for q, v in out.items()}


def gpu_backward(name, form, gscale, want_a=True, want_b=True):
    """(da, db, their buffers): the backward entry on the argmins of the forward entry"""
    a, b = device_inputs(name)
    B, N, M = C.CASES[name][:3]
    f = gpu_forward(name, form)
    arg_a, arg_b = torch.from_numpy(f["arg_a"]).cuda(), torch.from_numpy(f["arg_b"]).cuda()
    da, db = Banded((B, N, 3)), Banded((B, M, 3))
    L.check(getattr(L.load(), ENTRY[form][1])(L.ptr(a), L.ptr(b), B, N, M, L.ptr(arg_a), L.ptr(arg_b), gscale, da.ptr if want_a else None,
                                              db.ptr if want_b else None, L.cur_stream()), ENTRY[form][1])
    torch.cuda.synchronize()
    return da, db


@pytest.mark.parametrize("form", C.FORMS)
@pytest.mark.parametrize("name", C.CASES)
def test_forward_bits(name, form):
    got, want = gpu_forward(name, form), C.forward(name, form)
    for q in ("min_a", "arg_a", "min_b", "arg_b", "loss"):
        same_bits(got[q], want[q], (name, form, q))


@pytest.mark.parametrize("form", C.FORMS)
def test_both_forms_store_the_same_minima(form):
    for name in C.CASES:
        for q in ("min_a", "arg_a", "min_b", "arg_b"):
            same_bits(gpu_forward(name, form)[q], gpu_forward(name, "squared")[q], (name, q))


@pytest.mark.parametrize("gscale", C.GSCALES)
@pytest.mark.parametrize("form", C.FORMS)
@pytest.mark.parametrize("name", C.CASES)
def test_backward_bits(name, form, gscale):
    da, db = gpu_backward(name, form, gscale)
    want_a, want_b = C.backward(name, form, gscale)
    same_bits(da.get(), want_a, (name, form, gscale, "da"))
    same_bits(db.get(), want_b, (name, form, gscale, "db"))


@pytest.mark.parametrize("form", C.FORMS)
def test_a_coincident_pair_gets_a_signed_zero_from_the_squared_form_and_plus_zero_from_the_sqrt_form(form):
    """the shared point of a planted case: the squared form ASSIGNS w 2 (x - y) = -0.0 under a negative gscale and adds -0.0 for the one
    hit; the sqrt form starts from +0.0 and adds nothing"""
    for name in (n for n, c in C.CASES.items() if c[4]):
        B, N, M = C.CASES[name][:3]
        for gscale in C.GSCALES:
            da, db = (x.get() for x in gpu_backward(name, form, gscale))
            zero = np.float32(-0.0 if (form == "squared" and gscale < 0) else 0.0)
            for g in (da[:, N // 2], db[:, M - 1]):
                same_bits(g, np.full_like(g, zero), (name, form, gscale))


@pytest.mark.parametrize("form", C.FORMS)
@pytest.mark.parametrize("name", ["b2_5_3", "b2_257_300"])
def test_a_skipped_side_is_not_written_and_the_other_keeps_its_bits(name, form):
    want_a, want_b = C.backward(name, form, -1.5)
    da, db = gpu_backward(name, form, -1.5, want_b=False)
    same_bits(da.get(), want_a, (name, form, "da alone"))
    assert db.untouched()
    da, db = gpu_backward(name, form, -1.5, want_a=False)
    same_bits(db.get(), want_b, (name, form, "db alone"))
    assert da.untouched()

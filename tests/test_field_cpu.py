"""Per-point DPDist field, the part that needs no GPU: the admission of the reference case of tests/field_cases.py (the float32 oracle
against float64, so that a later change of seed cannot hide behind the bars of tests/test_field_gpu.py), the chunk plan, the capacity
report, the argument checks of the three new C entries (none of which touches a device) and of the public functions.
"""
import ctypes

import numpy as np
import pytest
import torch

from dpdist_amd import field
from dpdist_amd import lib as L

from . import field_cases as FC

E_NULL, E_DIM, E_UNSUPPORTED = -1, -2, -3


def test_admission_of_the_reference_case():
    """float32 oracle within 2 ADMIT_FWD of float64 per point (pred lies in [0, 2]); both saturations and masked queries occur"""
    for shared in (False, True):
        p64, m64 = FC.oracle(torch.float64, shared)
        p32, m32 = FC.oracle(torch.float32, shared)
        assert np.array_equal(m64, m32)
        err = np.abs(p32 - p64).max()
        print("shared %s: |f32 - f64| max %.3g, masked per cloud %s, zeros %.3f, twos %.4f"
              % (shared, err, [int(n - m64[c, :n].sum()) for c, n in enumerate(FC.QCOUNTS)], (p64 == 0).mean(), (p64 == 2).mean()))
        assert err <= FC.ADMIT_FWD * 2
        assert (p64 == 0).any() and (p64 == 2).any() and ((p64 > 0) & (p64 < 2)).any()
    m = FC.oracle(torch.float64)[1]
    assert [int(n - m[c, :n].sum()) for c, n in enumerate(FC.QCOUNTS)] == [24, 15, 0]      # (23, 14, 0 of the draw, and query 8)
    assert m[0, 7] == 1 and m[0, 8] == 0                     # the closed upper face is inside, the open lower face is not
    for c, n in enumerate(FC.QCOUNTS):
        assert not FC.oracle(torch.float64)[0][c, n:].any()


@pytest.mark.parametrize("shared", [False, True])
def test_admission_of_the_gradients(shared):
    """float32 autograd oracle within ADMIT_GRAD * max(1, max |g64|) of float64, every gradient; every cloud's gradient has structure"""
    for g64, g32 in zip(FC.oracle_grads(torch.float64, shared), FC.oracle_grads(torch.float32, shared)):
        err, top = np.abs(g32 - g64).max(), np.abs(g64).max()
        print("shared %s: |g32 - g64| max %.3g at max |g64| %.3g" % (shared, err, top))
        assert err <= FC.ADMIT_GRAD * max(1.0, top)
        assert top > 1e-2
    gS, gQ = FC.oracle_grads(torch.float64, shared)
    for c, n in enumerate(FC.COUNTS):
        assert not gS[c, n:].any()
    if not shared:
        for c, n in enumerate(FC.QCOUNTS):
            assert not gQ[c, n:].any()
        assert not gQ[:, 8].any()                            # a masked query has no gradient


@pytest.mark.parametrize("C,M,max_rows", FC.PLAN_CASES)
def test_plan_chunks_covers_every_row_once(C, M, max_rows):
    seen = np.zeros((C, M), dtype=np.int64)
    for c0, n, t0, T in field.plan_chunks(C, M, max_rows):
        assert n >= 1 and T >= 1 and c0 + n <= C and t0 + T <= M
        assert n * T <= max_rows or (n == 1 and T == M)      # a chunk holds at least one cloud
        assert (t0 == 0 and T == M) or n == 1                # whole clouds, or tiles of one cloud
        seen[c0:c0 + n, t0:t0 + T] += 1
    assert (seen == 1).all()
    if M <= max_rows:
        assert all(n == min(max(1, max_rows // M), C - c0) for c0, n, _, _ in field.plan_chunks(C, M, max_rows))
    else:
        assert all(T == min(max_rows, M - t0) for _, _, t0, T in field.plan_chunks(C, M, max_rows))
    with pytest.raises(ValueError):
        field.plan_chunks(C, M, 0)


def test_slot_capacity():
    lib = L.load()
    for n, T, m in ((1, 1, 8), (3, 150, 8), (2, 40, 8), (1, 600, 8), (7, 513, 8), (5, 1000, 10), (4, 3, 1), (1, 1 << 30, 8), (1 << 20, 1 << 10, 8)):
        assert lib.dpd_field_slot_capacity(n, T, m) == (n * min(m ** 3, T) + 31) // 32 * 32
    for n, T, m in ((0, 8, 8), (8, 0, 8), (-1, 8, 8), (1, 8, 0), (1, 8, 11), (2, 1 << 30, 8), (1 << 16, 1 << 15, 8)):
        assert lib.dpd_field_slot_capacity(n, T, m) == 0


def test_entries_refuse_bad_arguments_without_a_device():
    """every refusal happens before anything is launched: the pointers are never dereferenced (host memory would do) and no device is needed"""
    lib = L.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    KP = FC.KP
    assert lib.dpd_padded_width(FC.K_WIN) == KP
    index = lambda q=p, stride=0, t0=0, n=1, T=1, m=8, mask=p: lib.dpd_field_index(q, stride, None, t0, n, T, m, mask, p, p, p, None)   # noqa: E731
    assert index(q=None) == E_NULL and index(mask=None) == E_NULL
    assert index(n=0) == E_DIM and index(T=0) == E_DIM and index(t0=-1) == E_DIM and index(stride=-3) == E_DIM
    assert index(m=11) == E_UNSUPPORTED and index(m=0) == E_UNSUPPORTED and index(n=2, T=1 << 30) == E_UNSUPPORTED
    gather = lambda q=p, n=1, T=1, m=8, k=5, KP=KP, ldu=32, cnt=p: lib.dpd_field_gather(q, 0, p, p, p, p, p, n, T, m, k, KP, p, ldu, p, p, p, cnt,   # noqa: E731
                                                                                        None)
    assert gather(q=None) == E_NULL and gather(cnt=None) == E_NULL
    assert gather(n=0) == E_DIM and gather(T=-1) == E_DIM and gather(ldu=31) == E_DIM and gather(n=3, T=150, ldu=448) == E_DIM
    for kw in (dict(k=1), dict(k=4), dict(k=9), dict(KP=KP + 32), dict(KP=KP - 4), dict(m=11), dict(n=2, T=1 << 30),
               dict(n=1 << 12, T=1 << 10, ldu=1 << 21)):      # the last: Xu [2496, 2^21] beyond the GEMMs' 32-bit byte offsets
        assert gather(**kw) == E_UNSUPPORTED, kw
    cp = L.DecoderParams(*([p.value] * 8 + [None] * 3))
    dec = lambda Xu=p, ldu=32, cap=32, rows=1, KP=KP, H=256, prm=cp, a0=p, a1=ctypes.c_void_p(p.value + 4): lib.dpd_decoder_fwd_field(   # noqa: E731
        Xu, ldu, cap, p, p, p, p, p, rows, KP, H, prm, a0, a1, p, p, None)
    assert dec(Xu=None) == E_NULL and dec(prm=None) == E_NULL and dec(a0=None) == E_NULL
    assert dec(prm=L.DecoderParams(*([None] * 11))) == E_NULL
    assert dec(rows=0) == E_DIM and dec(ldu=28) == E_DIM and dec(cap=0) == E_DIM and dec(a1=p) == E_DIM
    assert dec(H=100) == E_UNSUPPORTED and dec(KP=KP + 4) == E_UNSUPPORTED and dec(cap=30, ldu=32) == E_UNSUPPORTED
    assert dec(rows=1 << 22, H=1024) == E_UNSUPPORTED        # activations [2^22, 1024] beyond the 32-bit byte offsets


class _Params:
    """what _resolve reads of a DPDistParams, without a device"""
    flat, KP, H, k, compute_dtype = torch.zeros(1), FC.KP, FC.H_DEC, FC.K_WIN, "f32"


def test_public_functions_raise_on_cpu_tensors():
    from dpdist_amd import DPDistField, dpdist_field
    S, Q = torch.tensor(FC.surfaces()), torch.tensor(FC.queries())
    with pytest.raises(ValueError, match="GPU"):
        dpdist_field(_Params(), S, Q)
    with pytest.raises(ValueError, match="GPU"):
        DPDistField(_Params())(S, Q[0], counts=FC.COUNTS)
    with pytest.raises(ValueError, match="one set per cloud"):
        dpdist_field(_Params(), S, Q[:2])
    with pytest.raises(ValueError, match="query_counts"):
        dpdist_field(_Params(), S, Q, query_counts=(150, 151, 1))
    with pytest.raises(ValueError, match="fp32"):
        bad = _Params()
        bad.compute_dtype = "bf16"
        dpdist_field(bad, S, Q)

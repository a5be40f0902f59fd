"""Paired DPDist for clouds of different sizes, without a GPU: the admission of the cases of tests/pairs_cases.py (the float32 oracle
against the float64 one, distances and gradients with structure) and the argument errors of dpdist_pairs that need no device."""
import numpy as np
import pytest
import torch

from tests import pairs_cases as PC


def test_the_reference_case_is_admitted():
    """float32 oracle within ADMIT_FWD of float64 on every distance, within ADMIT_GRAD on every gradient entry and within a quarter of
    the bar the kernels are held to; D spreads over more than 0.05; every reference gradient clears 20 x its bar"""
    o64, o32 = PC.case_oracle("reference", torch.float64), PC.case_oracle("reference", torch.float32)
    d32 = max(np.abs(a - b).max() for a, b in zip(o64, o32))
    print("D_AB %s  D_BA %s  float32 vs float64: %.3e" % (np.round(o64[1], 3), np.round(o64[2], 3), d32))
    assert d32 <= PC.ADMIT_FWD <= 0.25 * PC.FWD_BAR
    assert o64[0].max() - o64[0].min() > 0.05
    assert np.allclose(o64[1], (0.358, 0.0, 0.293), atol=2e-3) and o64[1][1] == 0.0      # the single query of B_1 on the lower relu6 saturation
    assert np.allclose(o64[2], (0.354, 0.397, 0.592), atol=2e-3)
    assert np.array_equal(o64[0], (o64[1] + o64[2]) / 2)
    A, B = PC.sets()
    for name, (ref, bar), g32, counts in zip(("gA", "gB"), PC.grad_bars("reference"), PC.case_grads("reference", torch.float32),
                                             (PC.COUNTS_A, PC.COUNTS_B)):
        e32 = np.abs(g32 - ref).max()
        per_cloud = [np.abs(ref[c]).max() for c in range(3)]
        print("%s: max|ref| per cloud %s, float32 oracle within %.3e, bar %.3e" % (name, np.round(per_cloud, 4), e32, bar))
        assert e32 <= 0.25 * bar and e32 <= PC.ADMIT_GRAD * max(1.0, np.abs(ref).max()), name
        assert min(per_cloud) > 20 * bar, "a reference gradient without structure makes the bar vacuous"
        for c, n in enumerate(counts):
            assert not ref[c, n:].any() and np.abs(ref[c, :n]).max() > 0


@pytest.mark.parametrize("name", ["rect", PC.LARGE[0], PC.LARGE[1]], ids=str)
def test_the_other_cases_are_admitted(name):
    o64, o32 = PC.case_oracle(name, torch.float64), PC.case_oracle(name, torch.float32)
    d32 = max(np.abs(a - b).max() for a, b in zip(o64, o32))
    print("%s: D_AB %s  D_BA %s  float32 vs float64: %.3e" % (name, o64[1], o64[2], d32))
    assert d32 <= 0.25 * PC.FWD_BAR and min(o64[1].min(), o64[2].min()) > 0
    if name == "rect":
        return                                                      # forward only on the GPU
    for which, (ref, bar), g32 in zip(("gA", "gB"), PC.grad_bars(name), PC.case_grads(name, torch.float32)):
        e32 = np.abs(g32 - ref).max()
        print("%s %s: max|ref| %.3f, float32 oracle within %.3e, bar %.3e" % (name, which, np.abs(ref).max(), e32, bar))
        assert e32 <= 0.25 * bar and np.abs(ref).max() > 20 * bar


def test_the_row_layout():
    segs = PC.seg_rows(3, 64, 40, PC.COUNTS_A, PC.COUNTS_B)
    assert segs[:3] == [(0, 0, 0, 40, 40), (0, 1, 40, 40, 1), (0, 2, 80, 40, 23)]
    assert segs[3:] == [(1, 0, 120, 64, 64), (1, 1, 184, 64, 37), (1, 2, 248, 64, 5)]
    assert PC.seg_rows(2, 24, 64, None, None)[-1] == (1, 1, 2 * 64 + 24, 24, 24) and 2 * (24 + 64) == 176


class _P:
    """what dpdist_pairs asks of a parameter set before it touches a device"""
    k, KP, H, compute_dtype = 5, PC.KP, 64, "f32"
    flat = torch.zeros(1)


def test_argument_errors_that_need_no_device():
    import dpdist_amd
    from dpdist_amd import pairs
    assert dpdist_amd.dpdist_pairs is pairs.dpdist_pairs and dpdist_amd.DPDistPairs is pairs.DPDistPairs
    A, B = torch.zeros(3, 64, 3), torch.zeros(3, 40, 3)
    with pytest.raises(ValueError, match="same number of clouds"):
        pairs.dpdist_pairs(_P, A, B[:2])
    with pytest.raises(ValueError, match="one count per cloud"):
        pairs.dpdist_pairs(_P, A, B, countsA=[64, 37])
    with pytest.raises(ValueError, match=r"lie in \[1, 40\]"):
        pairs.dpdist_pairs(_P, A, B, countsB=[40, 41, 1])
    with pytest.raises(ValueError, match=r"lie in \[1, 64\]"):
        pairs.dpdist_pairs(_P, A, B, countsA=torch.tensor([64, 0, 5]))
    with pytest.raises(ValueError, match="sequence of integers"):
        pairs.dpdist_pairs(_P, A, B, countsA=torch.tensor([64.0, 37.0, 5.0]))
    with pytest.raises(ValueError, match=r"\[C, N, 3\]"):
        pairs.dpdist_pairs(_P, A, None)
    with pytest.raises(ValueError, match="fp32"):
        pairs.dpdist_pairs(type("Q", (_P,), {"compute_dtype": "bf16"}), A, B)
    with pytest.raises(ValueError, match="max_rows"):
        pairs.DPDistPairs(_P, max_rows=0)
    with pytest.raises(ValueError, match="GPU"):                    # everything above comes first: the clouds are CPU tensors here
        pairs.dpdist_pairs(_P, A, B, countsA=[64, 37, 5], countsB=[40, 1, 23])
    assert pairs.chunk_pairs(3, 104, 1) == 1 and pairs.chunk_pairs(3, 104, 208) == 2 and pairs.chunk_pairs(3, 104, 1 << 20) == 3

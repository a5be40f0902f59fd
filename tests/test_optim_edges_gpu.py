"""Exact-value edge tests of the optimizer and loss kernels (csrc/loss_adam.hip) through their C entries dpd_adam_tf, dpd_adam_tf_dev,
dpd_adam_tf_fused and dpd_l1_loss.

tests/optim_cases.py holds the references, the state builders, the checker and the case tables (tests/test_optim_edges_cpu.py proves
on the CPU that the checker has teeth).  Every Adam result must equal `adam_f32`, a numpy-float32 restatement of adam_one in the same
operation order, bit for bit -- the library is built with -ffp-contract=off and float32 division and square root are correctly
rounded -- and, for the real-valued family, lie inside the first-order float64 rounding bound `adam_bound`.  The exact family makes
"every element updated exactly once, from its own g, m, v" an equality whatever the rounding.  Every copy the fused launch derives
(transposed fp32, bf16 RC / R8 planes), the tail's reduced gradient and its two loss values are compared bit for bit with their
restatements; every buffer sits between guard bands that must keep their bits.  Every comparison is an equality of bit patterns or an
integer return code, except the float64 bound.  The fused table (optim_cases.fused_cases) holds the shapes DPDistTrainer never
builds: partial row tiles, cols % 128 != 0 with planes, one plane layout without the other, a transposed copy together with planes,
odd gaps, the tail role alone, record forms, the 2048-block cap of the vector role."""
import ctypes

import numpy as np
import pytest
import torch

from dpdist_amd import lib as L

from . import optim_cases as O
from .gemm_cases import NAN_IN, banded_flat

pytestmark = pytest.mark.gpu

CASES = O.fused_cases()
FAMILY_NAMES = list(O.FAMILIES)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible")
    L.load()     # raises if the HIP extension is missing -- never fall back
    return torch.device("cuda:0")


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _consts(run):
    return [float(x) for x in run.consts[1:]]


# ------------------------------------------------------------------------------------------------ the three entries as step functions
def plain_step(run, lr_t):
    rc = L.load().dpd_adam_tf(P(run.p), P(run.g), P(run.m), P(run.v), run.case.n, float(lr_t), *_consts(run), L.cur_stream())
    assert rc == 0, rc


class DevStep:
    """dpd_adam_tf_dev: lr_t in state[3] of a banded 8-float buffer whose other seven entries are NAN_IN"""

    def __init__(self, dev):
        self.state, self.chk = banded_flat(8, NAN_IN, device=dev)
        self.lr_t = None

    def __call__(self, run, lr_t):
        self.lr_t = np.float32(lr_t)
        self.state[3] = float(lr_t)
        rc = L.load().dpd_adam_tf_dev(P(run.p), P(run.g), P(run.m), P(run.v), run.case.n, P(self.state), *_consts(run), L.cur_stream())
        assert rc == 0, rc

    def check(self):
        want = np.full(8, NAN_IN, dtype=np.int32)
        want[3] = self.lr_t.view(np.int32)
        O.same_bits(self.state, want.view(np.float32), "state")
        self.chk()


def fused_step(run, lr_t):
    case = run.case
    f = L.AdamFuse()
    for i, mt in enumerate(case.mats):
        f.w_off[i], f.w_rows[i], f.w_cols[i] = mt.off, mt.rows, mt.cols
        for arr, buf in ((f.WT, run.WT[i]), (f.W_rc, run.rc[i]), (f.W_r8, run.r8[i])):
            arr[i] = None if buf is None else buf.data_ptr()
    f.np = case.np
    if case.tail is not None:
        t = case.tail
        f.partials, f.nparts, f.rec, f.H, f.Qb, f.tail_off = run.partials.data_ptr(), t.nparts, t.rec, t.H, O.tail_qb(t), O.tail_off(case)
        f.loss = None if run.loss is None else run.loss.data_ptr()
    rc = L.load().dpd_adam_tf_fused(P(run.p), P(run.g), P(run.m), P(run.v), case.n, float(lr_t), *_consts(run), ctypes.byref(f), L.cur_stream())
    assert rc == 0, rc


# ------------------------------------------------------------------------------------------------ dpd_adam_tf / dpd_adam_tf_dev
@pytest.mark.parametrize("family", FAMILY_NAMES)
@pytest.mark.parametrize("n", O.PLAIN_N)
def test_adam_tf_and_dev_are_the_restatement_bit_for_bit(dev, n, family):
    """n below, at and above one float4 and one block, and beyond the 2048-block cap with a scalar leftover: both entries equal adam_f32,
    _dev equals the plain entry and leaves its state buffer (lr_t in state[3], NaN elsewhere) unchanged"""
    case = O.FusedCase("plain-%d" % n, n, (), 0, None)
    plain = O.run_fused_case(case, family, plain_step, dev)
    O.check_fused(plain)
    step = DevStep(dev)
    devr = O.run_fused_case(case, family, step, dev, state=plain.state)
    O.check_fused(devr)
    step.check()
    for a, b in ((plain.p, devr.p), (plain.m, devr.m), (plain.v, devr.v)):
        O.same_bits(a, b, "dpd_adam_tf_dev against dpd_adam_tf")


# ------------------------------------------------------------------------------------------------ dpd_adam_tf_fused
@pytest.mark.parametrize("family", FAMILY_NAMES)
@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_fused_case(dev, case, family):
    """one launch on one table entry: p, m, v, g, every derived copy, the loss, the padding and every guard band (optim_cases.check_fused);
    then dpd_adam_tf on a copy of the same state with the tail's gradient already reduced: "same arithmetic, element for element\""""
    run = O.run_fused_case(case, family, fused_step, dev)
    O.check_fused(run)
    plain = O.run_fused_case(O.vector_form(case), family, plain_step, dev, prefill_tail=True, state=run.state)
    O.check_fused(plain, tail_role=False)
    for a, b in ((run.p, plain.p), (run.m, plain.m), (run.v, plain.v)):
        O.same_bits(a, b, "dpd_adam_tf_fused against dpd_adam_tf")


@pytest.mark.parametrize("cid", O.TWO_STEP_CASES)
def test_two_fused_steps_are_two_restatement_steps(dev, cid):
    """the second step starts from the m, v the kernel's own streaming stores wrote"""
    run = O.run_fused_case(O.case_by_id(cid), "real_t1", fused_step, dev, lr_ts=(O.lr_t_of(1), O.lr_t_of(2)))
    O.check_fused(run)


# ------------------------------------------------------------------------------------------------ dpd_l1_loss
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("BN", O.L1_BN)
def test_l1_loss_exact(dev, BN, mode):
    """BN around one block trip, rows with pred == label (sign(0) = 0), NaN in the channels the kernel must not read: the two losses and
    dpred bit for bit; mode 0 writes no gradient (and takes dpred = NULL), mode 1 the first BN rows only, mode 2 all 2 BN"""
    lib = L.load()
    for gscale in O.L1_GSCALE:
        for with_dpred in ((True, False) if mode == 0 else (True,)):
            run = O.L1Run(BN, mode, gscale, dev)
            rc = lib.dpd_l1_loss(P(run.pred), P(run.labels), BN, mode, gscale, P(run.loss), P(run.dpred) if with_dpred else None, L.cur_stream())
            assert rc == 0, rc
            run.check(with_dpred)

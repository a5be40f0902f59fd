"""The average-pool pose encoder (`--pn_pool avg`, models/ipcr_model.py:236-271) without a GPU: the case table of
tests/test_pose_avg_gpu.py keeps its exactness condition, holds the patterns the GPU cases are there for, and the checker rejects wrong
restatements (tests/pose_avg_cases.py); the torch module takes the pool; the library exports the `_pool` entries and refuses what the
header says it refuses."""
import ctypes

import numpy as np
import pytest
import torch

from . import pose_avg_cases as A
from . import pose_cases as P
from .gemm_cases import EXACT

CASES = P.POINT_CASES
IDS = [c.id for c in CASES]


def _case(cid):
    return next(c for c in CASES if c.id == cid)


# ------------------------------------------------------------------------------------------------ the table
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_case_keeps_its_bound_and_its_quotient(case):
    """every reduction of the forward and the backward stays below 2^24 in absolute terms, and the float32 quotient S / N computed in
    float32 equals the float64 quotient rounded to float32 (the double-rounding argument, checked)"""
    fwd, bwd, want = A.avg_reference(case)
    print("%s: forward bound %.3e, backward bound %.3e" % (case.id, fwd["bound"], bwd["bound"]))
    assert fwd["bound"] < EXACT and bwd["bound"] < EXACT
    S32 = fwd["S"].astype(np.float32)
    assert np.array_equal(S32.astype(np.float64), fwd["S"])
    q32 = S32 / np.float32(case.N)
    assert q32.dtype == np.float32 and np.array_equal(q32.astype(np.float64), want["f"])
    # df / N is the integer k, dense
    k = P.point_k(case)
    assert np.array_equal((bwd["df"].astype(np.float32) / np.float32(case.N)).astype(np.float64), k.astype(np.float64))
    assert (k != 0).mean() > 0.8


def test_table_holds_the_patterns():
    pat = {c.id: A.avg_patterns(c) for c in CASES}
    assert sum(p["partial_last_pass"] for p in pat.values()) >= 10 and any(not p["partial_last_pass"] for p in pat.values())
    assert pat["plain-const-N130-C2+1"]["full_words"] > 0
    for cid in ("padwins-far-N33-C2+1", "padwins-far-N65-C2+1"):
        assert pat[cid]["origin_wins"] >= 3 * 64 and pat[cid]["partial_last_pass"]
    for cid in ("dead-plain-N33-C2+1", "dead-plain-N70-C2+1"):
        c = _case(cid)
        fwd, bwd, want = A.avg_reference(c)
        assert pat[cid]["dead"] == 3 * P.OUT and not want["f"].any() and not want["words"].any() and not want["dW5"].any()
    plain = [p for cid, p in pat.items() if cid.startswith("plain-plain")]
    assert all(0.1 < p["open_gates"] < 0.9 for p in plain)              # the gradient is dense: no single row per column
    assert any(p["dead"] > 0 for p in plain)


def test_avg_forward_agrees_with_the_pass_restatement():
    """the per-pass restatement of pose_cases (64-row passes padded with the origin) gives the same hidden activations; summing its real
    rows pass by pass gives S"""
    case = _case("plain-plain-N129-C2+1")
    net = P.point_net(case.net)
    a, b = P.point_clouds(case)
    passes = P.point_forward_passes(net, a, b, case.N)
    fwd, _, _ = A.avg_reference(case)
    for n in ("h1", "h2", "h3", "h4"):
        assert np.array_equal(passes[n], fwd[n])
    S = np.zeros_like(fwd["S"])
    for p0 in range(0, case.N, P.PP):
        S += fwd["a5"][:, p0:p0 + P.PP].sum(1)
    assert np.array_equal(S, fwd["S"])


# ------------------------------------------------------------------------------------------------ the checker has teeth
@pytest.mark.parametrize("fault,cid,first", [
    ("pad_in_sum", "padwins-far-N33-C2+1", "f"), ("pad_in_sum", "padwins-far-N65-C2+1", "f"), ("pad_in_sum", "plain-plain-N129-C2+1", "f"),
    ("div_64nw", "plain-plain-N33-C2+1", "f"), ("div_64nw", "plain-plain-N200-C2+1", "f"),
    ("tie_bits", "plain-plain-N64-C2+1", "words"), ("tie_bits", "plain-const-N130-C2+1", None),
    ("drop_last", "plain-plain-N65-C2+1", "f"), ("drop_last", "plain-plain-N1-C2+1", "f"),
    ("coef_popcount", "plain-plain-N33-C2+1", "dW1"), ("coef_popcount", "plain-plain-N2048-C1+1", "dW1"),
    ("drop_cloud", "plain-plain-N8-C35+30", "dW5"), ("drop_cloud", "plain-plain-N128-C2+1", "dW5")])
def test_checker_rejects_wrong_restatements(fault, cid, first):
    """a wrong restatement is rejected at the named array (None: it must NOT be rejected -- in a `const` cloud every point ties, so tie
    bits and gate bits coincide there, which is why the table needs the other clouds)"""
    case = _case(cid)
    _, _, want = A.avg_reference(case)
    assert P.rejects(want, want, A.AVG_NAMES) is None
    assert P.rejects(A.avg_faulty(case, fault), want, A.AVG_NAMES) == first


def test_drop_last_shows_in_the_word_too():
    case = _case("plain-plain-N65-C2+1")
    _, _, want = A.avg_reference(case)
    assert P.rejects(A.avg_faulty(case, "drop_last"), want, ("words",)) == "words"
    assert want["words"][:, 1].any()                                       # the lone point of the second pass opens gates
    assert int(want["words"][:, 1].max()) <= 1                              # ... and no bit at or beyond N is set


# ------------------------------------------------------------------------------------------------ the torch module
def _pair(B=3, N=40, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(B, N, 3, generator=g) * 2 - 1, torch.rand(B, N, 3, generator=g) * 2 - 1


def test_module_average_pool_is_the_mean_form():
    from dpdist_amd.registration import PoseNet
    torch.manual_seed(3)
    net = PoseNet(pool="avg").eval()
    for m in net.modules():
        if isinstance(m, torch.nn.Linear):
            torch.nn.init.uniform_(m.bias, -0.1, 0.1)
    src, tmpl = _pair()
    want = net.head(torch.cat([net.point(src).mean(1), net.point(tmpl).mean(1)], 1))
    assert net.pool == "avg" and torch.equal(net.raw(src, tmpl), want)
    fs, ft = net.features(src, tmpl)
    assert torch.equal(fs, net.point(src).mean(1)) and torch.equal(ft, net.point(tmpl).mean(1))
    assert not torch.equal(fs, net.point(src).amax(1))


def test_module_max_pool_is_the_old_module():
    from dpdist_amd.registration import PoseNet
    torch.manual_seed(3)
    old = PoseNet().eval()
    torch.manual_seed(3)
    new = PoseNet(1024, 45.0, 0.7, "max").eval()
    assert old.pool == "max" and list(old.state_dict()) == list(new.state_dict())
    assert all(torch.equal(a, b) for a, b in zip(old.state_dict().values(), new.state_dict().values()))
    src, tmpl = _pair()
    want = old.head(torch.cat([old.point(src).amax(1), old.point(tmpl).amax(1)], 1))
    assert torch.equal(old.raw(src, tmpl), want) and torch.equal(new.raw(src, tmpl), want)
    avg = PoseNet(pool="avg")
    assert list(avg.state_dict()) == list(old.state_dict())               # the same variables: load_tf_state_dict serves both


@pytest.mark.parametrize("pool", ["mean", "", None, 1, "MAX"])
def test_module_refuses_a_bad_pool(pool):
    from dpdist_amd.registration import PoseNet
    with pytest.raises(ValueError):
        PoseNet(pool=pool)


def test_support_predicates_take_both_pools():
    from dpdist_amd.registration import PoseNet, native_point_supported, native_refine_supported
    for pool in ("max", "avg"):
        net = PoseNet(pool=pool)
        assert native_point_supported(net) and native_refine_supported(net)


# ------------------------------------------------------------------------------------------------ the library, host side
NEW_ENTRIES = ("dpd_pose_point_fwd_train_pool", "dpd_pose_point_bwd_pool", "dpd_pose_point_bwd_workspace_bytes_pool", "dpd_pose_refine_pool")
E_NULL, E_DIM, E_UNSUPPORTED, E_WORKSPACE = -1, -2, -3, -4
POOL_MAX, POOL_AVG = 0, 1
ADDR = 1 << 30                   # a 256-byte aligned "device address": validation never dereferences it
no_gpu = pytest.mark.skipif(torch.cuda.is_available(), reason="placeholder device pointers: host validation only, not for a machine with a GPU")


@pytest.fixture(scope="module")
def lib():
    from dpdist_amd import build, lib as L
    build.build(verbose=False)
    return L.load()


def test_library_exports_the_pool_entries(lib):
    from dpdist_amd import lib as L
    for name in NEW_ENTRIES:
        assert getattr(lib, name) is not None and name in L.SIGNATURES
    assert L.POOLS == {"max": POOL_MAX, "avg": POOL_AVG}
    header = open(L.HERE + "/../include/dpdist_capi.h").read()
    assert "enum dpd_pool { DPD_POOL_MAX = 0, DPD_POOL_AVG = 1 }" in header


def test_workspace_entry(lib):
    """max: the size of dpd_pose_point_bwd_workspace_bytes_n; avg: that without the max pool's optional coef, plus coef, coef * popcount
    [clouds, 1024] each and min(chunks, 32) partials [1024, 128]; 0 for what the entries refuse"""
    for C in (1, 3, 32, 66):
        for N in (1, 64, 65, 1024, 2048):
            NW = (N + 63) // 64
            old = lib.dpd_pose_point_bwd_workspace_bytes_n(C, N)
            assert lib.dpd_pose_point_bwd_workspace_bytes_pool(C, N, POOL_MAX) == old > 0
            records = old - (4 * C * 1024 if NW > 1 else 0)
            assert lib.dpd_pose_point_bwd_workspace_bytes_pool(C, N, POOL_AVG) == records + 4 * (2 * C * 1024 + min(C * NW, 32) * 1024 * 128)
    for args in ((4, 2049, POOL_AVG), (0, 64, POOL_AVG), (4, 0, POOL_AVG), (4, 64, 2), (4, 64, -1), (4, 2049, POOL_MAX)):
        assert lib.dpd_pose_point_bwd_workspace_bytes_pool(*args) == 0


def _net(out_features=1024, drop=None):
    from dpdist_amd.lib import PoseNetW
    net = PoseNetW()
    for field, n in (("Wp", 5), ("bp", 5), ("Wh", 4), ("bh", 4)):
        for i in range(n):
            getattr(net, field)[i] = None if drop == (field, i) else ADDR
    net.out_features = out_features
    return net


def _arr(n, drop=None):
    return (ctypes.c_void_p * n)(*[None if i == drop else ADDR for i in range(n)])


def _fwd(lib, pool=POOL_AVG, net=None, N=16, nA=2, **kw):
    a = dict(ptsA=ADDR, ptsB=ADDR, f=ADDR, h1=ADDR, h2=ADDR, h3=ADDR, h4=ADDR, words=ADDR)
    a.update(kw)
    return lib.dpd_pose_point_fwd_train_pool(ctypes.byref(net or _net()), a["ptsA"], a["ptsB"], nA, 2, N, pool, a["f"], a["h1"], a["h2"], a["h3"],
                                             a["h4"], a["words"], None)


def _bwd(lib, pool=POOL_AVG, net=None, N=16, nA=2, short=0, dW=None, **kw):
    a = dict(ptsA=ADDR, ptsB=ADDR, df=ADDR, h1=ADDR, h2=ADDR, h3=ADDR, h4=ADDR, words=ADDR, ws=ADDR)
    a.update(kw)
    nb = lib.dpd_pose_point_bwd_workspace_bytes_pool(4, 16, pool if pool in (0, 1) else POOL_AVG) - short
    return lib.dpd_pose_point_bwd_pool(ctypes.byref(net or _net()), a["ptsA"], a["ptsB"], nA, 2, N, pool, a["df"], a["h1"], a["h2"], a["h3"], a["h4"],
                                       a["words"], _arr(5, dW), _arr(5), a["ws"], nb, None)


def _refine(lib, pool=POOL_AVG, net=None, B=2, short=0, **kw):
    a = dict(src=ADDR, tmpl=ADDR, ws=ADDR, moved=ADDR, T_out=ADDR)
    a.update(kw)
    nb = lib.dpd_pose_refine_workspace_bytes(2, 16, 1024) - short
    return lib.dpd_pose_refine_pool(ctypes.byref(net or _net()), a["src"], a["tmpl"], B, 16, 2, 45.0, pool, None, a["ws"], nb, a["moved"], a["T_out"],
                                    None, None)


@no_gpu
@pytest.mark.parametrize("entry", [_fwd, _bwd, _refine], ids=["fwd", "bwd", "refine"])
def test_pool_entries_refuse_an_unknown_pool(lib, entry):
    for pool in (2, -1, 7):
        assert entry(lib, pool=pool) == E_UNSUPPORTED
    # ... after the NULL and dimension checks, as the header orders them
    assert entry(lib, pool=2, net=_net(drop=("Wp", 4))) == E_NULL
    assert entry(lib, pool=2, **({"B": 0} if entry is _refine else {"nA": 0})) == E_DIM


@no_gpu
@pytest.mark.parametrize("pool", [POOL_MAX, POOL_AVG])
def test_pool_entries_keep_the_refusals_of_the_old_entries(lib, pool):
    for name in ("ptsA", "ptsB", "f", "h1", "h2", "h3", "h4", "words"):
        assert _fwd(lib, pool, **{name: None}) == E_NULL, name
    for name in ("ptsA", "ptsB", "df", "h1", "h2", "h3", "h4", "words", "ws"):
        assert _bwd(lib, pool, **{name: None}) == E_NULL, name
    for name in ("src", "tmpl", "ws", "moved", "T_out"):
        assert _refine(lib, pool, **{name: None}) == E_NULL, name
    assert _bwd(lib, pool, dW=4) == E_NULL
    assert _fwd(lib, pool, N=2049) == E_UNSUPPORTED and _bwd(lib, pool, N=2049) == E_UNSUPPORTED
    assert _fwd(lib, pool, N=0) == E_DIM and _bwd(lib, pool, N=0) == E_DIM and _refine(lib, pool, B=0) == E_DIM
    for entry in (_fwd, _bwd, _refine):
        assert entry(lib, pool, net=_net(out_features=512)) == E_UNSUPPORTED
    assert _fwd(lib, pool, h1=ADDR + 4) == E_UNSUPPORTED
    assert _bwd(lib, pool, short=1) == E_WORKSPACE and _refine(lib, pool, short=1) == E_WORKSPACE
    assert _refine(lib, pool, ws=ADDR + 4) == E_UNSUPPORTED
    assert _bwd(lib, POOL_AVG, h4=ADDR + 4) == E_UNSUPPORTED              # the dense dW5 kernel reads h4 in 16-byte pieces

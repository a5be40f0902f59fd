"""Host logic of the pose network's translation units (dpdist_amd/csrc/pose.hip, pose_point.hip, pose_point_bwd.hip, pose_head.hip): the
code every pose entry returns for an argument set it refuses, and the size entries over a grid -- the checks of the network's layers, the
PointNetW packing and the launchers are defined in one unit each and used by the others.  Every literal below was recorded from the
library of the commit before the split.

Every call here is refused by argument validation, which dereferences none of the placeholder pointers.  A library that got a check
wrong could fall through to a launch on those pointers, so the module does not run where a GPU is visible."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="placeholder device pointers: host validation only, not for a machine with a GPU")

E_NULL, E_DIM, E_UNSUPPORTED, E_WORKSPACE = -1, -2, -3, -4
P = 1 << 30                      # any 256-byte aligned "device address": validation never dereferences it
Q = P + 4096                     # a second one (T_in beside T_out)

ENTRIES = ("dpd_pose_apply_fwd", "dpd_pose_apply_bwd", "dpd_pose_refine_workspace_bytes", "dpd_pose_refine", "dpd_pose_point_tie_words",
           "dpd_pose_point_bwd_workspace_bytes", "dpd_pose_point_bwd_workspace_bytes_n", "dpd_pose_point_fwd_train", "dpd_pose_point_bwd",
           "dpd_pose_head_fwd_train", "dpd_pose_head_bwd_workspace_bytes", "dpd_pose_head_bwd")
UNITS = ("pose.hip", "pose_point.hip", "pose_point_bwd.hip", "pose_head.hip")


@pytest.fixture(scope="module")
def lib():
    from dpdist_amd import build, lib as L
    build.build(verbose=False)
    return L.load()


def make_net(drop=None, out_features=1024):
    """dpd_pose_net with every slot set, except `drop` = (field, layer)"""
    from dpdist_amd.lib import PoseNetW
    net = PoseNetW()
    for field, n in (("Wp", 5), ("bp", 5), ("Wh", 4), ("bh", 4)):
        for i in range(n):
            getattr(net, field)[i] = None if drop == (field, i) else P
    net.out_features = out_features
    return net


def grads(n, drop=None):
    """float* const [n] with every entry set, except entry `drop`; drop = -1: no array"""
    if drop == -1:
        return None
    return (ctypes.c_void_p * n)(*[None if i == drop else P for i in range(n)])


def net_arg(a):
    if a.get("net", P) is None:
        return None
    return ctypes.byref(make_net(a.get("slot"), a.get("out_features", 1024)))


def apply_fwd(lib, **kw):
    a = dict(pred=P, src=P, T_in=Q, B=2, N=16, mode=0, pose=P, moved=P, T_out=P)
    a.update(kw)
    return lib.dpd_pose_apply_fwd(a["pred"], a["src"], a["T_in"], a["B"], a["N"], 45.0, a["mode"], a["pose"], a["moved"], a["T_out"], None)


def apply_bwd(lib, **kw):
    a = dict(pred=P, src=P, dmoved=P, B=2, N=16, dpred=P)
    a.update(kw)
    return lib.dpd_pose_apply_bwd(a["pred"], a["src"], a["dmoved"], a["B"], a["N"], 45.0, a["dpred"], None)


def refine(lib, **kw):
    a = dict(src=P, tmpl=P, B=2, N=16, loops=2, ws=P, ws_short=0, moved=P, T_out=P)
    a.update(kw)
    nb = lib.dpd_pose_refine_workspace_bytes(2, 16, 1024) - a["ws_short"]
    return lib.dpd_pose_refine(net_arg(a), a["src"], a["tmpl"], a["B"], a["N"], a["loops"], 45.0, None, a["ws"], nb, a["moved"], a["T_out"], None,
                               None)


def point_fwd(lib, **kw):
    a = dict(ptsA=P, ptsB=P, nA=2, nB=2, N=16, f=P, h1=P, h2=P, h3=P, h4=P, ties=P)
    a.update(kw)
    return lib.dpd_pose_point_fwd_train(net_arg(a), a["ptsA"], a["ptsB"], a["nA"], a["nB"], a["N"], a["f"], a["h1"], a["h2"], a["h3"], a["h4"],
                                        a["ties"], None)


def point_bwd(lib, **kw):
    a = dict(ptsA=P, ptsB=P, nA=2, nB=2, N=16, df=P, h1=P, h2=P, h3=P, h4=P, ties=P, dW=None, db=None, ws=P, ws_short=0)
    a.update(kw)
    nb = lib.dpd_pose_point_bwd_workspace_bytes_n(4, 16) - a["ws_short"]
    return lib.dpd_pose_point_bwd(net_arg(a), a["ptsA"], a["ptsB"], a["nA"], a["nB"], a["N"], a["df"], a["h1"], a["h2"], a["h3"], a["h4"], a["ties"],
                                  grads(5, a["dW"]), grads(5, a["db"]), a["ws"], nb, None)


def head_fwd(lib, **kw):
    a = dict(f=P, B=2, h1=P, h2=P, h3=P, pred=P)
    a.update(kw)
    return lib.dpd_pose_head_fwd_train(net_arg(a), a["f"], a["B"], None, a["h1"], a["h2"], a["h3"], a["pred"], None)


def head_bwd(lib, **kw):
    a = dict(f=P, B=2, h1=P, h2=P, h3=P, dpred=P, dW=None, db=None, df=P, ws=P, ws_short=0)
    a.update(kw)
    nb = lib.dpd_pose_head_bwd_workspace_bytes(2) - a["ws_short"]
    return lib.dpd_pose_head_bwd(net_arg(a), a["f"], a["B"], None, a["h1"], a["h2"], a["h3"], a["dpred"], grads(4, a["dW"]), grads(4, a["db"]),
                                 a["df"], a["ws"], nb, None)


# the pointers whose absence an entry refuses (an optional pointer's absence is a valid call: not for placeholder addresses)
POINTERS = {apply_fwd: ("pred", "src"), apply_bwd: ("pred", "src", "dmoved", "dpred"),
            refine: ("net", "src", "tmpl", "ws", "moved", "T_out"),
            point_fwd: ("net", "ptsA", "ptsB", "f", "h1", "h2", "h3", "h4", "ties"),
            point_bwd: ("net", "ptsA", "ptsB", "df", "h1", "h2", "h3", "h4", "ties", "ws"),
            head_fwd: ("net", "f", "h1", "h2", "h3", "pred"),
            head_bwd: ("net", "f", "h1", "h2", "h3", "dpred", "df", "ws")}
POINT_SLOTS = [(f, i) for f in ("Wp", "bp") for i in range(5)]
HEAD_W, HEAD_B = [("Wh", i) for i in range(4)], [("bh", i) for i in range(4)]
# the slots of the net an entry checks (dpd_pose_head_bwd reads no bias: bh is not among its checks)
SLOTS = {refine: POINT_SLOTS + HEAD_W + HEAD_B, point_fwd: POINT_SLOTS, point_bwd: POINT_SLOTS, head_fwd: HEAD_W + HEAD_B, head_bwd: HEAD_W}
ZERO = {apply_fwd: ("B", "N"), apply_bwd: ("B", "N"), refine: ("B", "N", "loops"), point_fwd: ("nA", "N"), point_bwd: ("nA", "N"),
        head_fwd: ("B",), head_bwd: ("B",)}


def _cases():
    out = []
    for e, names in POINTERS.items():
        for n in names:
            out.append((e, "no " + n, {n: None}))
        for s in SLOTS.get(e, ()):
            out.append((e, "no %s[%d]" % s, dict(slot=s)))
        for n in ZERO[e]:
            out.append((e, n + " 0", {n: 0}))
        if e in SLOTS:
            out.append((e, "out_features 512", dict(out_features=512)))
    out += [(apply_fwd, "no output", dict(pose=None, moved=None, T_out=None)), (apply_fwd, "mode -1", dict(mode=-1)),
            (apply_fwd, "mode 2", dict(mode=2)), (apply_fwd, "T_out == T_in", dict(T_in=P)),
            (refine, "workspace off 16 bytes", dict(ws=P + 4)), (refine, "workspace one byte short", dict(ws_short=1)),
            (point_fwd, "h1 off 16 bytes", dict(h1=P + 4))]
    for e in (point_fwd, point_bwd):
        out += [(e, "nB -1", dict(nB=-1)), (e, "N 2049", dict(N=2049))]
    for e, n in ((point_bwd, 5), (head_bwd, 4)):
        out += [(e, "no dW", dict(dW=-1)), (e, "no db", dict(db=-1))]
        out += [(e, "no dW[%d]" % i, dict(dW=i)) for i in range(n)] + [(e, "no db[%d]" % i, dict(db=i)) for i in range(n)]
        out.append((e, "workspace one byte short", dict(ws_short=1)))
    # two refusals at once: which check comes first
    out += [(apply_fwd, "T_out == T_in, B 0", dict(T_in=P, B=0)), (refine, "out_features 512, B 0", dict(out_features=512, B=0)),
            (refine, "workspace off 16 bytes and short", dict(ws=P + 4, ws_short=1)), (refine, "no bh[3], loops 0", dict(slot=("bh", 3), loops=0)),
            (point_fwd, "out_features 512, no ptsA", dict(out_features=512, ptsA=None)), (point_fwd, "N 2049, nA 0", dict(N=2049, nA=0)),
            (point_fwd, "no ties, N 0", dict(ties=None, N=0)), (point_bwd, "out_features 512, no df", dict(out_features=512, df=None)),
            (point_bwd, "no dW[0], nA 0", dict(dW=0, nA=0)), (point_bwd, "N 2049, workspace short", dict(N=2049, ws_short=1)),
            (head_fwd, "out_features 512, B 0", dict(out_features=512, B=0)), (head_fwd, "no Wh[0], B 0", dict(slot=("Wh", 0), B=0)),
            (head_bwd, "out_features 512, workspace short", dict(out_features=512, ws_short=1)),
            (head_bwd, "out_features 512, B 0", dict(out_features=512, B=0)), (head_bwd, "no db[3], B 0", dict(db=3, B=0))]
    return out


CASES = _cases()
# one code per case, in the order of CASES (recorded from the parent commit's library)
CODES = (-1, -1, -2, -2, -1, -1, -1, -1, -2, -2, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
         -1, -2, -2, -2, -3, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -2, -2, -3, -1, -1, -1, -1, -1, -1,
         -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -2, -2, -3, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -2, -3,
         -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -2, -3, -1, -2, -2, -3, -3, -4, -3, -2, -3, -2, -3, -1, -1, -1, -1, -1, -1, -1, -1,
         -1, -1, -1, -1, -4, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -4, -3, -2, -3, -1, -3, -2, -1, -3, -1, -3, -2, -1, -3, -2, -1)


def test_every_case_has_its_code():
    assert len(CODES) == len(CASES)


@pytest.mark.parametrize("i", range(len(CASES)), ids=["%s: %s" % (c[0].__name__, c[1]) for c in CASES])
def test_refusal_codes(lib, i):
    entry, what, kw = CASES[i]
    assert entry(lib, **kw) == CODES[i], what


TIE_N = (0, 1, 64, 65, 2048)
TIE_WORDS = [0, 1, 1, 2, 32]
WS_CLOUDS, WS_N, WS_B = (0, 1, 33), (64, 65, 2048, 2049), (0, 5, 33)
REFINE_WS = [0, 0, 0, 0, 105984, 106496, 344064, 344576, 697344, 698368, 2268672, 2269696]          # dpd_pose_refine_workspace_bytes(B, N, 1024), B-major
POINT_WS = [0, 100352, 3311616]           # dpd_pose_point_bwd_workspace_bytes(clouds)
POINT_WS_N = [0, 0, 0, 0, 100352, 204800, 3215360, 0, 3311616, 6758400, 106106880, 0]         # dpd_pose_point_bwd_workspace_bytes_n(clouds, N), clouds-major
HEAD_WS = [0, 35840, 236544]            # dpd_pose_head_bwd_workspace_bytes(B)


def test_tie_words(lib):
    assert [lib.dpd_pose_point_tie_words(N) for N in TIE_N] == TIE_WORDS


def test_workspace_bytes(lib):
    assert [lib.dpd_pose_refine_workspace_bytes(B, N, 1024) for B in WS_B for N in WS_N] == REFINE_WS
    assert [lib.dpd_pose_point_bwd_workspace_bytes(C) for C in WS_CLOUDS] == POINT_WS
    assert [lib.dpd_pose_point_bwd_workspace_bytes_n(C, N) for C in WS_CLOUDS for N in WS_N] == POINT_WS_N
    assert [lib.dpd_pose_head_bwd_workspace_bytes(B) for B in WS_B] == HEAD_WS


def test_units_and_entries(lib):
    from dpdist_amd import build
    assert all(u in build.SOURCES for u in UNITS)
    assert build.SOURCES.index("pose.hip") + 3 == build.SOURCES.index("pose_head.hip")      # the new units at pose.hip's place
    for name in ENTRIES:
        assert getattr(lib, name) is not None

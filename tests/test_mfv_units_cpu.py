"""Host logic of the encoder's two translation units (dpdist_amd/csrc/mfv3d.hip, mfv3d_bwd.hip): the code every encoder entry returns
for an argument set it refuses, and dpd_mfv3d_fits / dpd_mfv3d_tile over a grid -- the LDS formulas and default_tile are defined in one
unit and used by both.  Every literal below was recorded from the library of the commit before the split.

Every call here is refused by argument validation, which dereferences none of the placeholder pointers.  A library that got a check
wrong could fall through to a launch on those pointers, so the module does not run where a GPU is visible."""
import pytest
import torch

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="placeholder device pointers: host validation only, not for a machine with a GPU")

E_NULL, E_DIM, E_UNSUPPORTED, E_WORKSPACE = -1, -2, -3, -4
P = 1 << 30                      # any 256-byte aligned "device address": validation never dereferences it
S = 0.125


@pytest.fixture(scope="module")
def lib():
    from dpdist_amd import build, lib as L
    build.build(verbose=False)
    return L.load()


def ws_bytes(C, m):
    return C * 4 * 33 * m ** 3 * 4


def fwd(lib, **kw):
    a = dict(pts=P, C=2, N=16, m=8, sigma=S, fv=P)
    a.update(kw)
    return lib.dpd_mfv3d_fwd(a["pts"], a["C"], a["N"], a["m"], a["sigma"], a["fv"], None)


def fwd_stacked(lib, **kw):
    a = dict(pcA=P, pcB=P, noise=None, C=2, N=16, m=8, sigma=S, pts=P, q=P, fv=P, ssq=None)
    a.update(kw)
    return lib.dpd_mfv3d_fwd_stacked(a["pcA"], a["pcB"], a["noise"], a["C"], a["N"], a["m"], a["sigma"], a["pts"], a["q"], a["fv"], a["ssq"], None)


def bwd(lib, **kw):
    a = dict(pts=P, dfv=P, C=2, N=16, m=8, sigma=S, dpts=P, ws=P, ws_bytes=None)
    a.update(kw)
    nb = ws_bytes(2, 8) if a["ws_bytes"] is None else a["ws_bytes"]
    return lib.dpd_mfv3d_bwd(a["pts"], a["dfv"], a["C"], a["N"], a["m"], a["sigma"], a["dpts"], a["ws"], nb, None)


def fwd_tiled(lib, **kw):
    a = dict(pts=P, C=2, N=16, m=8, sigma=S, tile=0, fv=P)
    a.update(kw)
    return lib.dpd_mfv3d_fwd_tiled(a["pts"], a["C"], a["N"], a["m"], a["sigma"], a["tile"], a["fv"], None)


def bwd_tiled(lib, **kw):
    a = dict(pts=P, dfv=P, C=2, N=16, m=8, sigma=S, tile=0, dpts=P, ws=P, ws_bytes=None)
    a.update(kw)
    nb = ws_bytes(2, 8) if a["ws_bytes"] is None else a["ws_bytes"]
    return lib.dpd_mfv3d_bwd_tiled(a["pts"], a["dfv"], a["C"], a["N"], a["m"], a["sigma"], a["tile"], a["dpts"], a["ws"], nb, None)


def fwd_counts(lib, **kw):
    a = dict(pts=P, counts=P, C=2, N=16, m=8, sigma=S, tile=0, fv=P)
    a.update(kw)
    return lib.dpd_mfv3d_fwd_counts(a["pts"], a["counts"], a["C"], a["N"], a["m"], a["sigma"], a["tile"], a["fv"], None)


def bwd_counts(lib, **kw):
    a = dict(pts=P, counts=P, dfv=P, C=2, N=16, m=8, sigma=S, tile=0, dpts=P, ws=P, ws_bytes=None)
    a.update(kw)
    nb = ws_bytes(2, 8) if a["ws_bytes"] is None else a["ws_bytes"]
    return lib.dpd_mfv3d_bwd_counts(a["pts"], a["counts"], a["dfv"], a["C"], a["N"], a["m"], a["sigma"], a["tile"], a["dpts"], a["ws"], nb, None)


def asloss_tail(lib, **kw):
    """B = 1 -> 2 clouds; k = 3 -> KP >= 27 * 20 + 3 = 543, padded to 544"""
    a = dict(dX=P, vox=P, pts=P, upstream=None, B=1, N=16, m=8, k=3, KP=544, sigma=S, dfv=P, ws=P, ws_bytes=None, gA=P, gB=P)
    a.update(kw)
    nb = ws_bytes(2, 8) if a["ws_bytes"] is None else a["ws_bytes"]
    return lib.dpd_asloss_tail(a["dX"], a["vox"], a["pts"], a["upstream"], a["B"], a["N"], a["m"], a["k"], a["KP"], a["sigma"], a["dfv"], a["ws"], nb,
                               a["gA"], a["gB"], None)


POINTERS = {fwd: ("pts", "fv"), fwd_stacked: ("pcA", "pcB", "fv"), bwd: ("pts", "dfv", "dpts"), fwd_tiled: ("pts", "fv"),
            bwd_tiled: ("pts", "dfv", "dpts"), fwd_counts: ("pts", "counts", "fv"), bwd_counts: ("pts", "counts", "dfv", "dpts"),
            asloss_tail: ("dX", "vox", "pts", "dfv", "ws", "gA", "gB")}
COUNT = {fwd_stacked: "C", asloss_tail: "B"}          # the argument that counts the clouds
TILED = (fwd_tiled, bwd_tiled, fwd_counts, bwd_counts)
BACKWARD = (bwd, bwd_tiled, bwd_counts, asloss_tail)


def _cases():
    out = []
    for e, names in POINTERS.items():
        for n in names:
            out.append((e, "no " + n, {n: None}))
        out.append((e, "no clouds", {COUNT.get(e, "C"): 0}))
        for what, kw in (("N 0", dict(N=0)), ("m 0", dict(m=0)), ("m 11", dict(m=11)), ("sigma 0", dict(sigma=0.0))):
            out.append((e, what, kw))
    for e in BACKWARD:
        out.append((e, "m 9", dict(m=9, ws_bytes=ws_bytes(2, 9))))
    for e in TILED:
        for t in (-8, 4, 12):
            out.append((e, "tile %d" % t, dict(tile=t)))
        # tables beyond 160 KiB: forward (6 m + 6) t + 21 * 128 + 4 floats, backward (6 m + 52) t + 4 floats
        out.append((e, "tile beyond 160 KiB", dict(tile=760 if e in (fwd_tiled, fwd_counts) else 416, N=4096)))
    for e in (bwd_tiled, bwd_counts):
        out.append((e, "workspace one byte short", dict(ws_bytes=ws_bytes(2, 8) - 1)))
        out.append((e, "no workspace", dict(ws=None)))
    out += [(asloss_tail, "k 2", dict(k=2)), (asloss_tail, "k 9", dict(k=9)), (asloss_tail, "KP too small", dict(KP=540)),
            (asloss_tail, "KP % 4 != 0", dict(KP=546)), (asloss_tail, "N 7", dict(N=7)),
            (asloss_tail, "workspace one byte short", dict(ws_bytes=ws_bytes(2, 8) - 1))]
    return out


CASES = _cases()
# one code per case, in the order of CASES (recorded from the parent commit's library)
CODES = (-1, -1, -2, -3, -3, -3, -2, -1, -1, -1, -2, -3, -3, -3, -2, -1, -1, -1, -2, -3, -3, -3, -2, -1, -1, -2, -3, -3, -3, -2, -1, -1,
         -1, -2, -3, -3, -3, -2, -1, -1, -1, -2, -3, -3, -3, -2, -1, -1, -1, -1, -2, -3, -3, -3, -2, -1, -1, -1, -1, -1, -1, -1, -2, -2,
         -3, -3, -2, -3, -3, -3, -3, -3, -3, -3, -3, -3, -3, -3, -3, -3, -3, -3, -3, -3, -3, -3, -3, -4, -4, -4, -4, -3, -3, -2, -2, -3,
         -3)


def test_every_case_has_its_code():
    assert len(CODES) == len(CASES)


@pytest.mark.parametrize("i", range(len(CASES)), ids=["%s: %s" % (c[0].__name__, c[1]) for c in CASES])
def test_refusal_codes(lib, i):
    entry, what, kw = CASES[i]
    assert entry(lib, **kw) == CODES[i], what


def test_workspace_bytes(lib):
    assert [lib.dpd_mfv3d_bwd_workspace_bytes(C, m) for C, m in ((0, 8), (-3, 8), (1, 1), (2, 8), (3, 5))] == WS_BYTES


FITS_N = (1, 7, 8, 64, 402, 403, 705, 706, 1636, 1637, 4096, 4097)
FITS_M = (1, 5, 8, 9, 10, 11)
WS_BYTES = [0, 0, 528, 540672, 198000]
# dpd_mfv3d_fits(N, m, which): one string per (m, which), one digit per N of FITS_N
FITS = {
    (1, 0): '111111111100',  (1, 1): '111111000000',  (1, 2): '111111111100',  (1, 3): '000000000000',
    (5, 0): '111111110000',  (5, 1): '111111000000',  (5, 2): '111111111100',  (5, 3): '000000000000',
    (8, 0): '111111100000',  (8, 1): '111110000000',  (8, 2): '111111111000',  (8, 3): '000000000000',
    (9, 0): '111111000000',  (9, 1): '000000000000',  (9, 2): '000000000000',  (9, 3): '000000000000',
    (10, 0): '111111000000',  (10, 1): '000000000000',  (10, 2): '000000000000',  (10, 3): '000000000000',
    (11, 0): '000000000000',  (11, 1): '000000000000',  (11, 2): '000000000000',  (11, 3): '000000000000',
}
# dpd_mfv3d_tile(m, which) for m of FITS_M, which = 0 .. 3
TILES = {1: (1360, 280, 280, 280), 5: (432, 192, 192, 192), 8: (248, 160, 160, 160), 9: (208, 0, 0, 0), 10: (168, 0, 0, 0), 11: (0, 0, 0, 0)}


def test_fits_grid(lib):
    got = {(m, w): "".join(str(lib.dpd_mfv3d_fits(N, m, w)) for N in FITS_N) for m in FITS_M for w in range(4)}
    assert got == FITS


def test_tile_grid(lib):
    assert {m: tuple(lib.dpd_mfv3d_tile(m, w) for w in range(4)) for m in FITS_M} == TILES

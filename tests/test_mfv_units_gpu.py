"""Two forms of the 3DmFV encoder that are the same routine over the same order of operations (dpdist_amd/csrc/mfv3d_int.h): with ONE
tile, the tiled forward is the eight-point-group forward and the tiled backward is the sliced backward, bit for bit -- the shared device
routines make that true by construction.  Shapes are the smallest that take the paths: N no multiple of 8 (the plain forward then runs
mfv3d_fwd_kernel, not the packed one), N = 3 with five of the eight point groups empty, and N = 50 whose point slices (13, 13, 13, 11)
each fit one tile of 16."""
import numpy as np
import pytest
import torch

from . import mfv_cases as M
from . import mfv_tiled_cases as T

pytestmark = pytest.mark.gpu

C, MG, TILE = 3, 5, 16


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible")
    from dpdist_amd import lib
    lib.load()     # raises if the HIP extension is missing -- never fall back
    return torch.device("cuda:0")


def _points(N, dev):
    return torch.tensor(M.points(("u", C, N, MG, M.S0)), device=dev)


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("N", [13, 3])
def test_one_tile_forward_is_the_plain_forward(dev, N):
    assert not M.uses_fwd2(N)
    pts = _points(N, dev)
    rc_p, fv_p, band_p = M.gpu_forward(pts, MG, M.S0)
    rc_t, fv_t, band_t = T.gpu_forward_tiled(pts, MG, M.S0, TILE)
    assert rc_p == 0 and rc_t == 0
    band_p(), band_t()
    assert not M.untouched(fv_p)
    assert torch.equal(_bits(fv_t), _bits(fv_p))          # NaN patterns included


def test_one_tile_backward_is_the_sliced_backward(dev):
    N = 50
    assert M.takes_sliced(N) and max(M.point_slices(N)) <= TILE
    case = ("u", C, N, MG, M.S0)
    pts = _points(N, dev)
    dfv = torch.tensor(M.upstream(M.forward_ref(case).fv64, [7, C, N, MG]), device=dev)
    rc_p, g_p, bands_p, _ = M.gpu_backward(pts, dfv, MG, M.S0, True)
    rc_t, g_t, bands_t, _ = T.gpu_backward_tiled(pts, dfv, MG, M.S0, TILE)
    assert rc_p == 0 and rc_t == 0
    bands_p(), bands_t()
    assert float(g_p.abs().max()) > 0
    assert torch.equal(_bits(g_t), _bits(g_p))

"""Farthest-point sampling, the parts that need no GPU: the numpy restatement of the definition against itself (float32 == float64 on
lattice clouds, the properties every order has), the argument errors of dpd_fps_order / dpd_fps_gather_fwd / _bwd (decided on the host
before any launch), the Python mirror of the header, and resample_tree's file logic with the restatement as its order function."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from dpdist_amd import dataset as D

from . import fps_cases as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from dpdist_amd import build, lib as L
    build.build(verbose=False)
    return L.load()


def _header_constants():
    txt = open(os.path.join(ROOT, "include", "dpdist_capi.h")).read()
    return {k: int(eval(v)) for k, v in re.findall(r"#define (DPD_FPS_[A-Z_]+) (\(?[0-9 <]+\)?)", txt)}   # plain integer expressions


# ---------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 65, 300, 1500])
def test_restatement_float32_equals_float64_on_lattice_clouds(n):
    for cloud in (F.lattice_cloud(n, 0), F.lattice_cloud_with_duplicates(n, 1)):
        o32, r32 = F.fps_reference(cloud, n, dtype=np.float32)
        o64, r64 = F.fps_reference(cloud, n, dtype=np.float64)
        assert np.array_equal(o32, o64)
        assert np.array_equal(r32, r64.astype(np.float32))                 # the same exact dmin; sqrt rounds once either way
        F.check_properties(o32, r32, n)
        assert sorted(o32.tolist()) == list(range(n))                      # K = n: a full permutation, duplicates included


@pytest.mark.parametrize("n,K", [(7, 7), (100, 100), (1000, 64), (2051, 300)])
def test_restatement_properties_on_random_clouds(n, K):
    cloud = F.random_cloud(n, 3)
    order, radius = F.fps_reference(cloud, K, start=n // 2)
    assert order[0] == n // 2
    F.check_properties(order, radius, n)
    for k in (1, K // 2):                                                  # the order for K is a prefix of the order for K' > K
        o, r = F.fps_reference(cloud, k, start=n // 2)
        assert np.array_equal(o, order[:k]) and np.array_equal(r, radius[:k])
    over, rad = F.fps_reference(cloud[:5], 9)                              # K beyond the cloud: -1 / 0 behind the permutation
    assert sorted(over[:5].tolist()) == list(range(5)) and (over[5:] == -1).all() and (rad[5:] == 0).all()


def test_restatement_all_identical_cloud():
    cloud = np.full((7, 3), 0.25, np.float32)
    order, radius = F.fps_reference(cloud, 7, start=3)
    assert order.tolist() == [3, 0, 1, 2, 4, 5, 6]                         # excluded, not merely at distance 0; ties to the lowest index
    assert np.isposinf(radius[0]) and (radius[1:] == 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# the C entries' refusals and the Python mirror
# ---------------------------------------------------------------------------------------------------------------------
def test_fps_entries_are_declared():
    from dpdist_amd import lib as L
    for name in ("dpd_fps_workspace_bytes", "dpd_fps_order", "dpd_fps_gather_fwd", "dpd_fps_gather_bwd"):
        assert name in L.SIGNATURES
    assert len(L.SIGNATURES["dpd_fps_order"][1]) == 11 and len(L.SIGNATURES["dpd_fps_gather_fwd"][1]) == 8


def test_sampling_mirrors_the_header_constants():
    from dpdist_amd import sampling as S
    lim = _header_constants()
    assert lim["DPD_FPS_THREADS"] == 1024 and lim["DPD_FPS_MAX_POINTS"] >= 1 << 16 and lim["DPD_FPS_MAX_CLOUDS"] == 65535
    assert lim["DPD_FPS_THREADS"] <= lim["DPD_FPS_RESIDENT_POINTS"] < lim["DPD_FPS_MAX_POINTS"]
    assert (S.FPS_THREADS, S.FPS_RESIDENT_POINTS, S.FPS_MAX_POINTS, S.FPS_MAX_CLOUDS) == (
        lim["DPD_FPS_THREADS"], lim["DPD_FPS_RESIDENT_POINTS"], lim["DPD_FPS_MAX_POINTS"], lim["DPD_FPS_MAX_CLOUDS"])
    import dpdist_amd
    assert dpdist_amd.farthest_point_order is S.farthest_point_order and dpdist_amd.farthest_point_sample is S.farthest_point_sample


def test_fps_order_argument_errors_without_gpu(lib):
    """Validated before any HIP call: nothing is dereferenced and nothing is launched."""
    lim = _header_constants()
    R, MAXP, MAXC = lim["DPD_FPS_RESIDENT_POINTS"], lim["DPD_FPS_MAX_POINTS"], lim["DPD_FPS_MAX_CLOUDS"]
    p = ctypes.c_void_p(1 << 30)
    assert lib.dpd_fps_order(None, p, p, 1, 8, 4, p, p, None, 0, None) == -1          # DPD_E_NULL: pts, order
    assert lib.dpd_fps_order(p, p, p, 1, 8, 4, None, p, None, 0, None) == -1
    for S, W, K in ((0, 8, 4), (1, 0, 1), (1, 8, 0), (-1, 8, 4), (1, -8, 4), (1, 8, -4), (1, 8, 9)):
        assert lib.dpd_fps_order(p, None, None, S, W, K, p, None, None, 0, None) == -2    # DPD_E_DIM, K > W included
    assert lib.dpd_fps_order(p, None, None, 1, MAXP + 1, 4, p, None, p, 1 << 40, None) == -3     # DPD_E_UNSUPPORTED: beyond the caps
    assert lib.dpd_fps_order(p, None, None, MAXC + 1, 8, 4, p, None, None, 0, None) == -3
    # the workspace: none up to the resident width, S * W floats beyond; missing or too small is refused
    assert lib.dpd_fps_workspace_bytes(16, R) == 0 and lib.dpd_fps_workspace_bytes(1, 1) == 0
    need = lib.dpd_fps_workspace_bytes(3, R + 1)
    assert need == 3 * (R + 1) * 4 and lib.dpd_fps_workspace_bytes(2, MAXP) == 2 * MAXP * 4
    assert lib.dpd_fps_workspace_bytes(1, MAXP + 1) == 0 and lib.dpd_fps_workspace_bytes(MAXC + 1, 8) == 0
    assert lib.dpd_fps_workspace_bytes(0, 8) == 0 and lib.dpd_fps_workspace_bytes(1, -1) == 0
    assert lib.dpd_fps_order(p, None, None, 3, R + 1, 4, p, None, None, need, None) == -3
    assert lib.dpd_fps_order(p, None, None, 3, R + 1, 4, p, None, p, need - 1, None) == -3


@pytest.mark.parametrize("entry", ["dpd_fps_gather_fwd", "dpd_fps_gather_bwd"])
def test_fps_gather_argument_errors_without_gpu(lib, entry):
    lim = _header_constants()
    fn = getattr(lib, entry)
    p = ctypes.c_void_p(1 << 30)
    assert fn(None, p, 1, 8, 3, 4, p, None) == -1                          # DPD_E_NULL: src / dout, order, out / dsrc
    assert fn(p, None, 1, 8, 3, 4, p, None) == -1
    assert fn(p, p, 1, 8, 3, 4, None, None) == -1
    for S, W, Dm, K in ((0, 8, 3, 4), (1, 0, 3, 1), (1, 8, 0, 4), (1, 8, 3, 0), (-2, 8, 3, 4), (1, 8, -3, 4), (1, 8, 3, 9)):
        assert fn(p, p, S, W, Dm, K, p, None) == -2                        # DPD_E_DIM, K > W included
    assert fn(p, p, 1, lim["DPD_FPS_MAX_POINTS"] + 1, 3, 4, p, None) == -3  # DPD_E_UNSUPPORTED
    assert fn(p, p, lim["DPD_FPS_MAX_CLOUDS"] + 1, 8, 3, 4, p, None) == -3
    assert fn(p, p, 1, lim["DPD_FPS_MAX_POINTS"], 1 << 12, 4, p, None) == -3


def test_python_argument_errors_without_gpu(lib):
    from dpdist_amd import farthest_point_order, farthest_point_sample
    c = torch.zeros(2, 8, 3)
    for bad in ([0, 8], [1, 9], [1], [1.0, 2.0]):
        with pytest.raises(ValueError):
            farthest_point_order(c, 4, counts=bad)
    for bad in ([-1, 0], [0, 8], [0], [0.5, 1.0]):
        with pytest.raises(ValueError):
            farthest_point_order(c, 4, start=bad)
    with pytest.raises(ValueError):
        farthest_point_order(c, 4, counts=[8, 3], start=np.array([7, 3]))         # start beyond its cloud's count
    for K in (0, 9, 2.5):
        with pytest.raises(ValueError):
            farthest_point_order(c, K)
    with pytest.raises(ValueError):
        farthest_point_order(torch.zeros(2, 8, 2), 4)
    with pytest.raises(ValueError):
        farthest_point_sample(c, 4, features=torch.zeros(2, 7, 6))
    with pytest.raises(RuntimeError, match="GPU"):                                # valid arguments, CPU tensors: refused at the boundary
        farthest_point_order(c, 4, counts=[8, 3], start=[7, 2])
    with pytest.raises(RuntimeError, match="GPU"):
        farthest_point_sample(c, 4)


# ---------------------------------------------------------------------------------------------------------------------
# resample_tree on files, with the restatement as its order function
# ---------------------------------------------------------------------------------------------------------------------
TRAIN, TEST = ["chair_0001", "night_stand_0002"], ["chair_0003"]
ROWS = {"chair_0001": 40, "night_stand_0002": 9, "chair_0003": 25}


def _row(sid, i, cols):
    rng = np.random.default_rng([int(sid[-4:]), i])
    v = rng.uniform(-1, 1, cols)
    return ",".join(["%.6f" % x for x in v[:3]] + ["%.4f" % x for x in v[3:]])    # a second format: lines are carried, not re-printed


@pytest.fixture()
def src_tree(tmp_path):
    root = tmp_path / "src"
    root.mkdir()
    (root / D.NAMES_FILE).write_text("chair\nnight_stand\n")
    (root / D.SPLIT_FILES["train"]).write_text("".join(s + "\n" for s in TRAIN))
    (root / D.SPLIT_FILES["test"]).write_text("".join(s + "\n" for s in TEST))
    lines = {}
    for sid in TRAIN + TEST:
        (root / D.shape_name(sid)).mkdir(exist_ok=True)
        lines[sid] = [_row(sid, i, 6 if sid.startswith("chair") else 3) for i in range(ROWS[sid])]
        (root / D.shape_name(sid) / (sid + ".txt")).write_text("".join(ln + "\n" for ln in lines[sid]))
    return root, lines


def _xyz(lines):
    return np.array([ln.split(",")[:3] for ln in lines], np.float64).astype(np.float32)


def test_resample_tree_carries_lines_in_farthest_point_order(src_tree, tmp_path):
    root, lines = src_tree
    dst = tmp_path / "dst"
    calls = []

    def order_fn(points_list, K):
        calls.append((len(points_list), K))
        return F.fps_orders(points_list, K)

    done = D.resample_tree(str(root), str(dst), num_points=16, batch=2, order_fn=order_fn)
    assert len(done) == 3 and sum(c[0] for c in calls) == 3 and max(c[0] for c in calls) == 2     # `batch` shapes per call
    for sid in TRAIN + TEST:
        out = (dst / D.shape_name(sid) / (sid + ".txt")).read_text().splitlines()
        keep = min(16, ROWS[sid])
        want = F.fps_reference(_xyz(lines[sid]), keep)[0]
        assert want[0] == 0 and out == [lines[sid][j] for j in want]       # verbatim lines (6-column rows included), from row 0
        assert len(out) == keep                                            # the 9-row file keeps all its rows, in order
    for name in (D.NAMES_FILE, D.SPLIT_FILES["train"], D.SPLIT_FILES["test"]):
        assert (dst / name).read_bytes() == (root / name).read_bytes()     # list files are copied
    # the resampled tree is a tree: the generator's lists resolve in it
    assert [os.path.exists(raw) for _, _, raw in D.split_items(str(dst), D.SPLIT_FILES["train"])] == [True, True]
    # a prefix of a resampled file is itself the farthest-point sample of that size
    again = F.fps_reference(_xyz((dst / "chair" / "chair_0001.txt").read_text().splitlines()), 16)[0]
    assert again.tolist() == list(range(16))


def test_resample_tree_skips_existing_files_unless_overwrite(src_tree, tmp_path):
    root, lines = src_tree
    dst = tmp_path / "dst"
    (dst / "chair").mkdir(parents=True)
    (dst / "chair" / "chair_0001.txt").write_text("kept\n")
    done = D.resample_tree(str(root), str(dst), num_points=8, order_fn=F.fps_orders)
    assert sorted(os.path.basename(p) for p in done) == ["chair_0003.txt", "night_stand_0002.txt"]
    assert (dst / "chair" / "chair_0001.txt").read_text() == "kept\n"
    assert D.resample_tree(str(root), str(dst), num_points=8, order_fn=F.fps_orders) == []
    done = D.resample_tree(str(root), str(dst), num_points=8, overwrite=True, order_fn=F.fps_orders)
    assert len(done) == 3 and len((dst / "chair" / "chair_0001.txt").read_text().splitlines()) == 8


def test_resample_tree_honours_class_choice_and_refuses_bad_arguments(src_tree, tmp_path):
    root, _ = src_tree
    dst = tmp_path / "dst"
    done = D.resample_tree(str(root), str(dst), num_points=8, class_choice=["chair"], order_fn=F.fps_orders)
    assert sorted(os.path.basename(p) for p in done) == ["chair_0001.txt", "chair_0003.txt"]
    assert not (dst / "night_stand").exists()
    with pytest.raises(ValueError):
        D.resample_tree(str(root), str(root), order_fn=F.fps_orders)
    with pytest.raises(ValueError):
        D.resample_tree(str(root), str(tmp_path / "other"), class_choice=["sofa"], order_fn=F.fps_orders)
    with pytest.raises(RuntimeError):                                      # an order function that repeats an index is refused
        D.resample_tree(str(root), str(tmp_path / "other2"), num_points=4, order_fn=lambda pl, K: [np.zeros(K, np.int32) for _ in pl])


def test_cli_has_the_resample_flags(src_tree, tmp_path, monkeypatch):
    root, _ = src_tree
    seen = {}
    monkeypatch.setattr(D, "resample_tree", lambda *a, **k: seen.update(a=a, k=k) or [])
    monkeypatch.setattr(D, "generate_distance_dataset", lambda *a, **k: seen.update(gen=(a, k)) or [])
    D.main(["--resample_from", str(root), "--root", str(tmp_path / "dst"), "--fps_points", "12", "--only_chair", "--overwrite"])
    assert seen["a"] == (str(root), str(tmp_path / "dst")) and seen["k"] == {"num_points": 12, "class_choice": ["chair"], "overwrite": True}
    assert seen["gen"][0] == (str(tmp_path / "dst"),)                      # the generator then runs on --root, as before
    seen.clear()
    D.main(["--root", str(tmp_path / "dst")])
    assert "a" not in seen and "gen" in seen

"""File-backed training data (dpdist_amd/dataset.py), the parts that need no GPU: the reader of the reference's on-disk label format
(modelnet_dataset.py:30-187), its equivalence with SyntheticDistanceDataset, argument errors of dpd_nn_dist and the trainer's
--data_dir flag."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from dpdist_amd import dataset as D
from dpdist_amd.train import SyntheticDistanceDataset, compose_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from dpdist_amd import build, lib as L
    build.build(verbose=False)
    return L.load()


def _write_lists(root, train, test, names):
    (root / D.NAMES_FILE).write_text("".join(n + "\n" for n in names))
    (root / D.SPLIT_FILES["train"]).write_text("".join(s + "\n" for s in train))
    (root / D.SPLIT_FILES["test"]).write_text("".join(s + "\n" for s in test))
    for n in names:
        (root / n).mkdir(exist_ok=True)


def _write_labels(root, sid, pos, neg_l, neg_u, num=10 ** 4):
    raw = str(root / D.shape_name(sid) / sid) + ".txt"
    for path, a in zip(D.label_paths(raw, num), (pos, neg_l, neg_u)):
        np.savetxt(path, a, fmt="%.6f", delimiter=",")
    return raw


ROWS, NPTS, SEED = 20, 8, 3
TRAIN, TEST = ["chair_0001", "night_stand_0002", "chair_0003"], ["chair_0004"]


@pytest.fixture()
def tree(tmp_path):
    """Two categories, three train shapes (+ one test shape); 20-row files in which row i of every block carries the value i (column 0 of
    the points, column 3 of the negatives), column 1 the shape's number and column 2 the block (0 pos, 1 neg_l, 2 neg_u).  The reader takes
    neg_u through dataset.neg_u_order, so the neg_u FILE is written through the inverse: file[order[k]] = row k."""
    _write_lists(tmp_path, TRAIN, TEST, ["chair", "night_stand"])
    i = np.arange(ROWS, dtype=np.float64)
    for split, ids in (("train", TRAIN), ("test", TEST)):
        for index, sid in enumerate(ids):
            tag = float(sid[-4:])
            pos = np.stack([i, 0 * i + tag, 0 * i], 1)
            neg_l = np.stack([i, 0 * i + tag, 0 * i + 1, i], 1)
            neg_u = np.zeros((ROWS, 4))
            neg_u[D.neg_u_order(SEED, split, index, ROWS)] = np.stack([i, 0 * i + tag, 0 * i + 2, i], 1)
            _write_labels(tmp_path, sid, pos, neg_l, neg_u)
    return tmp_path


def test_file_names_are_the_ones_the_reference_reader_opens(tree):
    assert D.shape_name("night_stand_0002") == "night_stand"
    items = D.split_items(str(tree), D.SPLIT_FILES["train"])
    assert [(i, n) for i, n, _ in items] == [(0, "chair"), (1, "night_stand"), (2, "chair")]
    raw = items[1][2]
    assert raw == os.path.join(str(tree), "night_stand", "night_stand_0002.txt")
    stem = raw[:-4]
    assert D.label_paths(raw) == (stem + "_dist_c_scaled.txt", stem + "_10000_dist_c_neg_l.txt", stem + "_10000_dist_c_neg_u.txt")
    assert D.label_paths(raw, 256)[2] == stem + "_256_dist_c_neg_u.txt"
    D.require_label_files(str(tree))                                       # all there: no error


def test_reader_category_filter_shuffle_default_and_short_last_batch(tree):
    every = D.ModelNetDistanceDataset(str(tree), 2, NPTS, "train", seed=SEED)
    chairs = D.ModelNetDistanceDataset(str(tree), 2, NPTS, "train", class_choice=["chair"], seed=SEED)
    test = D.ModelNetDistanceDataset(str(tree), 2, NPTS, "test", class_choice=["chair"], seed=SEED)
    assert len(every.datapath) == 3 and [n for n, _ in chairs.datapath] == ["chair", "chair"] and len(test.datapath) == 1
    assert every.shuffle is True and test.shuffle is False                 # modelnet_dataset.py:74-78
    assert D.ModelNetDistanceDataset(str(tree), 2, NPTS, "train", shuffle=False).shuffle is False
    assert every.num_channel() == 3 and every.classes == {"chair": 0, "night_stand": 1}
    sizes, tags = [], []
    while every.has_next_batch():
        d, l = every.next_batch()
        assert d.shape[1:] == (3 * NPTS, 3) and l.shape[1:] == (2 * NPTS,) and d.dtype == l.dtype == np.float32
        sizes.append(len(d))
        tags += list(d[:, 0, 1])
    assert sizes == [2, 1] and sorted(tags) == [1.0, 2.0, 3.0]             # 3 shapes in batches of 2: a short last batch
    with pytest.raises(ValueError):
        D.ModelNetDistanceDataset(str(tree), 2, NPTS, "train", class_choice=["sofa"])


def test_reader_item_layout_and_one_permutation_for_the_five_blocks(tree):
    ds = D.ModelNetDistanceDataset(str(tree), 3, NPTS, "train", shuffle=False, seed=SEED)
    perms = []
    for epoch in range(2):
        d, l = ds.next_batch()
        assert not ds.has_next_batch()
        for b, sid in enumerate(TRAIN):
            pts, lab = d[b].reshape(3, NPTS, 3), l[b].reshape(2, NPTS)
            assert (pts[:, :, 1] == float(sid[-4:])).all()                 # the shape's own three files
            assert (pts[:, :, 2] == np.arange(3)[:, None]).all()           # pos | neg_l | neg_u
            perm = pts[0, :, 0]
            assert sorted(perm) == list(range(NPTS))                       # the FIRST npoints rows of each set, permuted
            for block in (pts[1, :, 0], pts[2, :, 0], lab[0], lab[1]):     # ... by one permutation (modelnet_dataset.py:99-111)
                assert np.array_equal(block, perm)
            perms.append(tuple(perm))
        ds.reset()
        if epoch == 0:                                                     # parsed arrays are cached: the files are not read again
            for sid in TRAIN:
                for p in D.label_paths(str(tree / D.shape_name(sid) / sid) + ".txt"):
                    os.remove(p)
    assert len(set(perms)) > 1                                             # a new permutation on every fetch


def test_reader_equals_the_synthetic_dataset_dumped_to_files(tmp_path):
    """A SyntheticDistanceDataset's items written in the on-disk format and read back give the same pcA / pcB / labels through
    compose_batch as the synthetic dataset itself, rounded to the files' 6 decimals.  Both datasets draw their per-fetch permutations from
    default_rng(seed + 17), so with shuffle=False the streams agree; the neg_u shuffle is pinned: each neg_u file is written through the
    inverse of dataset.neg_u_order, so the reader's pick restores the synthetic order."""
    n, seed, num_point = 16, 5, 8
    syn = SyntheticDistanceDataset(3, n, 2, "test", seed=seed, shuffle=False)
    ids = ["chair_%04d" % (i + 1) for i in range(3)]
    _write_lists(tmp_path, [], ids, ["chair"])
    for index, (sid, (pts, lab)) in enumerate(zip(ids, syn.items)):
        far = np.concatenate([pts[2 * n:], lab[n:, None]], 1)
        neg_u = np.zeros_like(far)
        neg_u[D.neg_u_order(seed, "test", index, n)] = far
        _write_labels(tmp_path, sid, pts[:n], np.concatenate([pts[n:2 * n], lab[:n, None]], 1), neg_u)
    ds = D.ModelNetDistanceDataset(str(tmp_path), 2, n, "test", class_choice=["chair"], shuffle=False, seed=seed)
    r6 = lambda a: np.round(a.astype(np.float64), 6).astype(np.float32)   # noqa: E731
    batches = 0
    while syn.has_next_batch():
        assert ds.has_next_batch()
        d0, l0 = syn.next_batch()
        d1, l1 = ds.next_batch()
        for a, b in zip(compose_batch(r6(d0), r6(l0), num_point), compose_batch(d1, l1, num_point)):
            assert a.shape == b.shape and np.array_equal(a, b)
        batches += 1
    assert batches == 2 and not ds.has_next_batch()


def test_missing_label_file_names_the_generator(tree):
    os.remove(D.label_paths(str(tree / "chair" / "chair_0003") + ".txt")[1])
    with pytest.raises(FileNotFoundError, match=r"python -m dpdist_amd\.dataset --root"):
        D.require_label_files(str(tree), ["chair"])
    ds = D.ModelNetDistanceDataset(str(tree), 3, NPTS, "train", shuffle=False)
    with pytest.raises(FileNotFoundError, match=r"python -m dpdist_amd\.dataset --root"):
        ds.next_batch()
    D.require_label_files(str(tree), ["night_stand"], splits=("train",))    # the other category is complete


def test_train_data_dir_without_label_files_raises_with_the_hint(tmp_path):
    from dpdist_amd import train as T
    _write_lists(tmp_path, ["chair_0001"], ["chair_0002"], ["chair"])
    for sid in ("chair_0001", "chair_0002"):
        np.savetxt(str(tmp_path / "chair" / sid) + ".txt", np.zeros((4, 6)), fmt="%.6f", delimiter=",")
    F = T.build_parser().parse_args([])
    assert F.data_dir == "" and F.num_neg_points == 10 ** 4               # default: the synthetic dataset, as before
    with pytest.raises(FileNotFoundError, match=r"python -m dpdist_amd\.dataset --root " + re.escape(str(tmp_path))):
        T.train(["--data_dir", str(tmp_path), "--log_dir", str(tmp_path / "log"), "--max_epoch", "1"])
    assert not (tmp_path / "log").exists()                                 # refused before anything was started


def test_candidate_samplers_are_keyed_and_hold_file_precision():
    a = D._ball_candidates(np.random.default_rng([0, 1, 2, 0, 0]), 4096)
    b = D._ball_candidates(np.random.default_rng([0, 1, 2, 0, 0]), 4096)
    c = D._ball_candidates(np.random.default_rng([0, 1, 2, 0, 1]), 4096)
    assert a.dtype == np.float32 and a.shape == (4096, 3) and a.flags.c_contiguous and np.array_equal(a, b) and not np.array_equal(a, c)
    r = np.sqrt((a.astype(np.float64) ** 2).sum(1))
    assert r.max() <= 1.0 + 1e-6 and abs((r < 0.5).mean() - 0.125) < 0.02  # uniform in the unit ball: P(r < 1/2) = 1/8
    q = D._cube_candidates(np.random.default_rng(0), 4096)
    assert np.abs(q).max() <= 1.0 and abs((np.sqrt((q.astype(np.float64) ** 2).sum(1)) > 1).mean() - (1 - np.pi / 6)) < 0.03
    for x in (a, q):                                                       # what "%.6f" stores is what the kernel saw
        txt = np.array([float("%.6f" % v) for v in x.ravel()[:512]], np.float64).astype(np.float32)
        assert np.array_equal(txt, x.ravel()[:512])


def test_nn_dist_argument_errors_without_gpu(lib):
    """Validated before any HIP call (as in test_capi_cpu.py): nothing is dereferenced."""
    p = ctypes.c_void_p(1 << 30)
    assert lib.dpd_nn_dist(None, p, 1, 4, 4, p, p, None) == -1             # DPD_E_NULL: ref, qry, dist
    assert lib.dpd_nn_dist(p, None, 1, 4, 4, p, p, None) == -1
    assert lib.dpd_nn_dist(p, p, 1, 4, 4, None, p, None) == -1
    for S, P, M in ((0, 4, 4), (1, 0, 4), (1, 4, 0), (-1, 4, 4), (1, -5, 4), (1, 4, -5)):
        assert lib.dpd_nn_dist(p, p, S, P, M, p, None, None) == -2         # DPD_E_DIM (arg = NULL is allowed)
    txt = open(os.path.join(ROOT, "include", "dpdist_capi.h")).read()
    lim = {k: int(eval(v)) for k, v in re.findall(r"#define (DPD_NN_[A-Z_]+) (\(?[0-9 <]+\)?)", txt)}   # plain integer expressions
    assert lim["DPD_NN_MAX_POINTS"] >= 50000 and lim["DPD_NN_MAX_SHAPES"] >= 16
    assert lib.dpd_nn_dist(p, p, 1, lim["DPD_NN_MAX_POINTS"] + 1, 4, p, p, None) == -3      # DPD_E_UNSUPPORTED
    assert lib.dpd_nn_dist(p, p, 1, 4, lim["DPD_NN_MAX_POINTS"] + 1, p, p, None) == -3
    assert lib.dpd_nn_dist(p, p, lim["DPD_NN_MAX_SHAPES"] + 1, 4, 4, p, p, None) == -3
    assert (D.NN_CHUNK, D.NN_TILE) == (lim["DPD_NN_CHUNK"], lim["DPD_NN_TILE"])             # dataset.py mirrors the header


def test_nn_distance_refuses_cpu_tensors_and_other_dtypes(lib):
    with pytest.raises(RuntimeError, match="GPU"):
        D.nn_distance(torch.zeros(4, 3), torch.zeros(5, 3))
    with pytest.raises(RuntimeError):
        D.nn_distance(torch.zeros(4, 3), torch.zeros(2, 5, 3))
    with pytest.raises(RuntimeError):
        D.nn_distance(torch.zeros(4, 2), torch.zeros(5, 2))

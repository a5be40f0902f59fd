"""From raw ModelNet-style clouds to a training run on the HIP path: generate_distance_dataset (restating
dataset_sample_with_gt.py:60-139 on dpd_nn_dist) -> the reference's label files -> ModelNetDistanceDataset -> train.py --data_dir."""
import math
import os

import numpy as np
import pytest

from dpdist_amd import dataset as D
from dpdist_amd import synth
from dpdist_amd.train import compose_batch

pytestmark = pytest.mark.gpu

NUM, CAND, P = 256, 4096, 2000
TRAIN, TEST = ["chair_0001", "chair_0002"], ["chair_0003"]


def _raw_tree(root):
    """Three chair-like clouds of 2000 points (synth's box-union sampler) in the unit ball, as raw <id>.txt with six columns like
    modelnet40_normal_resampled (the generator reads columns 0..2), plus the three list files."""
    rng = np.random.default_rng(42)
    os.makedirs(os.path.join(root, "chair"))
    with open(os.path.join(root, D.NAMES_FILE), "w") as f:
        f.write("chair\ntable\n")
    for split, ids in (("train", TRAIN), ("test", TEST)):
        with open(os.path.join(root, D.SPLIT_FILES[split]), "w") as f:
            f.write("".join(s + "\n" for s in ids))
        for sid in ids:
            pts = synth.make_chair(rng).sample(rng, P) / 0.8
            np.savetxt(os.path.join(root, "chair", sid + ".txt"), np.concatenate([pts, np.zeros((P, 3))], 1), fmt="%.6f", delimiter=",")
    return root


def _files(root):
    out = {}
    for sid in TRAIN + TEST:
        for p in D.label_paths(os.path.join(root, "chair", sid + ".txt"), NUM):
            with open(p, "rb") as f:
                out[os.path.relpath(p, root)] = f.read()
    return out


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = _raw_tree(str(tmp_path_factory.mktemp("modelnet")))
    done = D.generate_distance_dataset(root, class_choice=["chair"], num_neg_points=NUM, candidates=CAND, seed=0)
    assert len(done) == 3
    return root


def test_generated_files_have_the_reference_format_and_true_labels(tree):
    for sid in TRAIN + TEST:
        raw = os.path.join(tree, "chair", sid + ".txt")
        paths = D.label_paths(raw, NUM)
        assert all(os.path.exists(p) for p in paths)
        pos, near, far = (np.loadtxt(p, delimiter=",") for p in paths)
        assert pos.shape == (P, 3) and near.shape == (NUM, 4) and far.shape == (NUM, 4)
        assert np.abs(pos - 0.8 * np.loadtxt(raw, delimiter=",")[:, :3]).max() <= 1e-6
        assert (near[:, 3] > 0.001).all() and (near[:, 3] < 0.1).all()
        assert (far[:, 3] > 0.1).all()
        n_out = int(0.1 * NUM)
        norm = lambda a: np.sqrt((a[:, :3] ** 2).sum(1))     # noqa: E731
        assert n_out == 25 and (norm(far[-n_out:]) > 1).all() and (norm(far[:-n_out]) <= 1).all() and (norm(near) <= 1).all()
        for rows in (near, far):                              # float64 brute force against the STORED cloud: file rounding + fp32
            d = np.sqrt(((rows[:, None, :3] - pos[None]) ** 2).sum(2)).min(1)
            err = np.abs(rows[:, 3] - d).max()
            print("%s: max |stored label - float64 brute force| = %.3g" % (sid, err))
            assert err <= 1.5e-6


def test_generation_is_reproducible_and_seeded(tree, tmp_path):
    first = _files(tree)
    assert D.generate_distance_dataset(tree, class_choice=["chair"], num_neg_points=NUM, candidates=CAND, seed=0) == []   # all there: skipped
    assert len(D.generate_distance_dataset(tree, class_choice=["chair"], num_neg_points=NUM, candidates=CAND, seed=0, overwrite=True,
                                           shapes_per_launch=1)) == 3
    assert _files(tree) == first                               # identical bytes, also with one shape per launch
    other = _raw_tree(str(tmp_path / "other"))
    D.generate_distance_dataset(other, class_choice=["chair"], num_neg_points=NUM, candidates=CAND, seed=1)
    second = _files(other)
    assert sorted(second) == sorted(first)
    for name in first:
        assert (second[name] == first[name]) == name.endswith("_dist_c_scaled.txt"), name      # the cloud stays, every draw differs


def test_reader_feeds_compose_batch(tree):
    N = 64
    ds = D.ModelNetDistanceDataset(tree, 2, 2 * N, "train", class_choice=["chair"], num_neg_points=NUM)
    d, l = ds.next_batch(augment=True)
    assert d.shape == (2, 6 * N, 3) and l.shape == (2, 4 * N) and not ds.has_next_batch()
    pcA, pcB, lab = compose_batch(d, l, N)
    assert pcA.shape == pcB.shape == (2, N, 3) and lab.shape == (2, N)
    assert not lab[:, :N // 2].any() and (lab[:, N // 2:3 * N // 4] < 0.1).all() and (lab[:, 3 * N // 4:] > 0.1).all()


def test_train_runs_on_the_generated_files(tree, tmp_path):
    from dpdist_amd import train as T
    loss = T.train(["--data_dir", tree, "--num_neg_points", str(NUM), "--max_epoch", "1", "--batch_size", "2", "--num_point", "64",
                    "--category", "chair", "--log_dir", str(tmp_path / "log")])
    assert math.isfinite(loss) and loss > 0
    assert os.path.exists(str(tmp_path / "log" / "model.ckpt.npz"))

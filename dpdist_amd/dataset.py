#!/usr/bin/env python3
"""Real-shape training data for the DPDist trainer: nearest-distance labels on the GPU, the reference's on-disk format, and its reader.

    nn_distance                 thin wrapper over dpd_nn_dist (csrc/nn_dist.hip); no torch fallback
    generate_distance_dataset   restates dataset_sample_with_gt.py:60-139 (the reference's label generator) on that kernel
    ModelNetDistanceDataset     restates modelnet_dataset.py:30-187 (the reference's reader) with SyntheticDistanceDataset's interface
    resample_tree               writes a tree whose shape files are in farthest-point order (csrc/fps.hip through dpdist_amd/sampling.py)

    python -m dpdist_amd.dataset --root data/modelnet40_normal_resampled --only_chair      # writes the label files
    python -m dpdist_amd.train --data_dir data/modelnet40_normal_resampled                 # trains on them
    python -m dpdist_amd.dataset --resample_from data/my_shapes --root data/my_resampled [--fps_points 10000]   # resample, then label

THE ROW-ORDER CONTRACT.  Generator and readers take "the first npoints" rows of a shape file (modelnet_dataset.py:121-122,136;
dataset_sample_with_gt.py:79-82), which is a well-spread 64- or 128-point cloud only because modelnet40_normal_resampled was written in
FARTHEST-POINT ORDER: a prefix of such a file is itself a farthest-point sample.  A tree with any other row order (mesh samples, scans)
gives a clustered or arbitrary subset, silently.  `--resample_from SRC` (resample_tree) writes --root from SRC with every file in that
order, from its row 0, before the labels are generated; the text of each row is carried over unchanged.

Files, next to each raw `<root>/<shape>/<id>.txt` (comma separated, `%.6f`):
    <id>_dist_c_scaled.txt            [P,3]    the cloud scaled by 0.8
    <id>_<num>_dist_c_neg_l.txt       [num,4]  x, y, z, d with min_eps < d < 2 eps   (near the surface)
    <id>_<num>_dist_c_neg_u.txt       [num,4]  x, y, z, d with d > 2 eps; the last 10 % lie outside the unit ball
These are the names the reference's reader opens (modelnet_dataset.py:117-129).  The reference's generator assigns the `_l` name and
then overwrites the variable with the `_u` name (dataset_sample_with_gt.py:72-73), so it saves both sets to the `_u` file (:134-135)
and its own reader cannot find `_l`; this module writes the two names the reader needs.

Deviations from the reference's generator, both deliberate:
  * the sampling loop runs until BOTH sets hold `num_neg_points` rows (the reference loops on the near set only, :87, and would
    hand back a short far set for a shape that fills the ball);
  * coordinates are rounded to the files' 6 decimals BEFORE the labels are taken, and the near / far / outside-the-ball selections are
    made on the values as stored, so a file is self-consistent: a stored label is the distance between the stored coordinates (to the
    label's own rounding and fp32), and every stored row satisfies its set's inequality exactly.
Random draws come from numpy generators keyed on (seed, split, shape index, stage, draw): a run is reproducible and a shape's rows do not
depend on how many shapes share a launch.  They do not reproduce numpy's global stream.
"""
import argparse
import os

import numpy as np

from . import lib as L
from .train import SyntheticDistanceDataset

NN_CHUNK = 2048      # include/dpdist_capi.h: DPD_NN_CHUNK, reference points per LDS buffer
NN_TILE = 256        # include/dpdist_capi.h: DPD_NN_TILE, queries per workgroup
SPLIT_FILES = {"train": "modelnet40_train.txt", "test": "modelnet40_test.txt"}
NAMES_FILE = "modelnet40_shape_names.txt"


def nn_distance(ref, qry, return_index=False):
    """dist[..., i] = min_j |qry_i - ref_j| (Euclidean, fp32, exact-difference form) and, with return_index, the lowest such j (int32).
    ref [P,3] and qry [M,3], or batched [S,P,3] and [S,M,3]: CUDA float32 contiguous tensors."""
    import torch
    if ref.dim() != qry.dim() or ref.dim() not in (2, 3) or ref.shape[-1] != 3 or qry.shape[-1] != 3:
        raise RuntimeError("nn_distance takes ref [P,3] / qry [M,3] or ref [S,P,3] / qry [S,M,3], got %s and %s" % (tuple(ref.shape), tuple(qry.shape)))
    S = ref.shape[0] if ref.dim() == 3 else 1
    if qry.dim() == 3 and qry.shape[0] != S:
        raise RuntimeError("ref and qry must hold the same number of shapes, got %d and %d" % (S, qry.shape[0]))
    L.req(ref, name="ref"), L.req(qry, name="qry")
    P, M = ref.shape[-2], qry.shape[-2]
    dist = torch.empty(qry.shape[:-1], device=qry.device, dtype=torch.float32)
    arg = torch.empty(qry.shape[:-1], device=qry.device, dtype=torch.int32) if return_index else None
    L.check(L.load().dpd_nn_dist(L.ptr(ref), L.ptr(qry), S, P, M, L.ptr(dist), L.ptr(arg), L.cur_stream()), "dpd_nn_dist")
    return (dist, arg) if return_index else dist


# --------------------------------------------------------------------------------------------------------------
# file names and lists (dataset_sample_with_gt.py:190-202, modelnet_dataset.py:40-69)
# --------------------------------------------------------------------------------------------------------------
def _lines(path):
    with open(path) as f:
        return [ln.rstrip() for ln in f if ln.strip()]


def shape_name(shape_id):
    return "_".join(shape_id.split("_")[0:-1])


def split_items(root, split_file, class_choice=None):
    """[(index in the split's list, shape name, path of the raw <id>.txt)] after the reference's category filter."""
    if isinstance(class_choice, str):
        class_choice = [class_choice]
    out = []
    for i, sid in enumerate(_lines(os.path.join(root, split_file))):
        name = shape_name(sid)
        if class_choice and name not in class_choice:
            continue
        out.append((i, name, os.path.join(root, name, sid) + ".txt"))
    return out


def label_paths(raw_path, num_neg_points=10 ** 4):
    stem = raw_path[:-4]
    return (stem + "_dist_c_scaled.txt", stem + "_%d_dist_c_neg_l.txt" % num_neg_points, stem + "_%d_dist_c_neg_u.txt" % num_neg_points)


def generator_hint(root):
    return "python -m dpdist_amd.dataset --root %s" % root


def require_label_files(root, class_choice=None, num_neg_points=10 ** 4, splits=("train", "test")):
    """Raise (before any GPU work) when a shape of `splits` lacks one of its three label files."""
    for split in splits:
        for _, _, raw in split_items(root, SPLIT_FILES[split], class_choice):
            for p in label_paths(raw, num_neg_points):
                if not os.path.exists(p):
                    raise FileNotFoundError("%s is missing: write the distance labels first with `%s`" % (p, generator_hint(root)))


# --------------------------------------------------------------------------------------------------------------
# generator
# --------------------------------------------------------------------------------------------------------------
def _round6(a):
    """The value a `%.6f` file holds, as the float32 a reader gets back from it."""
    return np.round(np.asarray(a, np.float64), 6).astype(np.float32, order="C")


def _ball_candidates(rng, n):
    """uniform_sampeling(type='dropped_coordinates') (:178-185): five normals, keep three, divide by the 5-norm -> uniform in the unit ball"""
    g = rng.standard_normal((5, n))
    return _round6((g[2:5] / np.sqrt((g * g).sum(0))).T)


def _cube_candidates(rng, n):
    """uniform_sampeling(type='cube') (:153-154)"""
    return _round6(rng.uniform(-1.0, 1.0, (n, 3)))


def _label(clouds, cands):
    """[S,P,3] float32 clouds and [S,M,3] float32 candidates -> rows [S,M,4] float64 = x, y, z, d as a `%.6f` file stores them"""
    import torch
    d = nn_distance(torch.from_numpy(clouds).cuda(), torch.from_numpy(cands).cuda()).cpu().numpy()
    return np.concatenate([cands.astype(np.float64), np.round(d.astype(np.float64), 6)[..., None]], -1)


def _generate_group(clouds, keys, num_neg_points, candidates, eps, min_eps, seed):
    """clouds [S,P,3] (scaled, rounded) -> per shape (neg_l [num,4], neg_u [num,4]).  keys[s] = (split id, shape index)."""
    S = len(clouds)
    near = [np.zeros((0, 4)) for _ in range(S)]
    far = [np.zeros((0, 4)) for _ in range(S)]
    draw = 0
    while any(len(near[s]) < num_neg_points or len(far[s]) < num_neg_points for s in range(S)):
        c = np.stack([_ball_candidates(np.random.default_rng([seed, k[0], k[1], 0, draw]), candidates) for k in keys])
        rows = _label(clouds, c)
        for s in range(S):
            if len(near[s]) >= num_neg_points and len(far[s]) >= num_neg_points:
                continue                                            # a finished shape ignores the draws its launch-mates still need
            r = rows[s]
            d, inside = r[:, 3], np.sqrt((r[:, :3] ** 2).sum(1)) <= 1.0
            near[s] = np.concatenate([near[s], r[inside & (d > min_eps) & (d < 2 * eps)]])     # :93
            far[s] = np.concatenate([far[s], r[inside & (d > 2 * eps)]])                        # :101
        draw += 1
    near = [a[:num_neg_points] for a in near]
    far = [a[:num_neg_points].copy() for a in far]
    n_out = int(num_neg_points * 0.1)                               # :112-130: the last 10 % of far come from outside the unit ball
    out = [np.zeros((0, 4)) for _ in range(S)]
    draw = 0
    while n_out and any(len(o) < n_out for o in out):
        c = np.stack([_cube_candidates(np.random.default_rng([seed, k[0], k[1], 1, draw]), candidates) for k in keys])
        rows = _label(clouds, c)                                    # every candidate is labelled so that one launch serves all shapes
        for s in range(S):
            if len(out[s]) < n_out:
                out[s] = np.concatenate([out[s], rows[s][np.sqrt((rows[s][:, :3] ** 2).sum(1)) > 1.0]])
        draw += 1
    for s in range(S):
        if n_out:
            far[s][-n_out:] = out[s][:n_out]
    return list(zip(near, far))


def generate_distance_dataset(root, split_files=("modelnet40_test.txt", "modelnet40_train.txt"), class_choice=None, num_neg_points=10 ** 4,
                              candidates=50000, eps=0.05, min_eps=0.001, seed=0, overwrite=False, shapes_per_launch=8, verbose=False):
    """Write the three label files of every shape in `split_files` (after the category filter).  Returns the raw paths written for.
    Shapes that already have their files are skipped unless `overwrite`.  Up to `shapes_per_launch` clouds of equal size share a launch."""
    todo = []
    for si, sf in enumerate(split_files):
        for idx, _, raw in split_items(root, sf, class_choice):
            if overwrite or not all(os.path.exists(p) for p in label_paths(raw, num_neg_points)):     # :75
                todo.append(((si, idx), raw))
    done = []
    group = []

    def flush():
        if not group:
            return
        clouds = np.stack([g[2] for g in group])
        res = _generate_group(clouds, [g[0] for g in group], num_neg_points, candidates, eps, min_eps, seed)
        for (key, raw, pos), (neg_l, neg_u) in zip(group, res):
            fn_pos, fn_l, fn_u = label_paths(raw, num_neg_points)
            np.savetxt(fn_pos, pos, fmt="%.6f", delimiter=",")      # :133-135
            np.savetxt(fn_l, neg_l, fmt="%.6f", delimiter=",")
            np.savetxt(fn_u, neg_u, fmt="%.6f", delimiter=",")
            done.append(raw)
            if verbose:
                print("wrote labels for", raw, flush=True)
        del group[:]

    for key, raw in todo:
        pos = _round6(np.loadtxt(raw, delimiter=",").astype(np.float32)[:, 0:3] * np.float32(0.8))    # :79-82
        if group and (len(group) >= shapes_per_launch or group[0][2].shape != pos.shape):
            flush()
        group.append((key, raw, pos))
    flush()
    return done


# --------------------------------------------------------------------------------------------------------------
# resampler: any tree -> a tree whose files are in farthest-point order
# --------------------------------------------------------------------------------------------------------------
def _hip_fps_orders(points_list, K):
    """the default order_fn of resample_tree: one ragged launch of dpd_fps_order (dpdist_amd/sampling.py) from row 0 of every cloud"""
    import torch
    from .sampling import farthest_point_order
    counts = [len(p) for p in points_list]
    pts = np.zeros((len(points_list), max(counts), 3), np.float32)
    for c, p in enumerate(points_list):
        pts[c, :len(p)] = p
    order = farthest_point_order(torch.from_numpy(pts).cuda(), K, counts=counts).cpu().numpy()
    return [order[c, :min(K, n)] for c, n in enumerate(counts)]


def _read_rows(path):
    """the non-empty text lines of a shape file and the float32 parse of their first three columns (the values np.loadtxt(...).astype(
    np.float32) gives the generator above)"""
    lines = _lines(path)
    if not lines:
        raise ValueError("%s holds no rows" % path)
    xyz = np.array([ln.split(",")[0:3] for ln in lines], dtype=np.float64).astype(np.float32)
    if xyz.ndim != 2 or xyz.shape[1] != 3:
        raise ValueError("%s: every row must start with x,y,z" % path)
    if not np.isfinite(xyz).all():
        raise ValueError("%s holds a coordinate that is not finite" % path)
    return lines, xyz


def resample_tree(src_root, dst_root, num_points=10 ** 4, class_choice=None, overwrite=False, batch=16, order_fn=None):
    """Write every `<shape>/<id>.txt` that the split files of `src_root` name (after the category filter) to the same relative path under
    `dst_root`, holding the first min(num_points, n) rows of the file's FARTHEST-POINT ORDER from row 0 -- the order the readers' "first
    npoints" presumes.  Rows are `x,y,z[,...]`, any count, any order; the text lines themselves are moved, so every value (normals
    included) stays byte for byte, and the order is computed on the float32 parse of the first three columns.  The list files are copied.
    `batch` shapes share a launch as one ragged batch.  A shape whose destination exists is skipped unless `overwrite`.
    order_fn(points_list, K) -> one index sequence per cloud, at least min(K, n) long; default: the HIP op (no torch fallback).
    Returns the destination paths written."""
    import shutil
    if num_points < 1 or batch < 1:
        raise ValueError("num_points and batch must be at least 1")
    if os.path.abspath(src_root) == os.path.abspath(dst_root):
        raise ValueError("resample_tree writes a new tree: dst_root must differ from src_root")
    order_fn = order_fn or _hip_fps_orders
    os.makedirs(dst_root, exist_ok=True)
    todo, seen = [], set()
    for name in [NAMES_FILE] + sorted(SPLIT_FILES.values()):
        src = os.path.join(src_root, name)
        if not os.path.exists(src):
            continue
        if name != NAMES_FILE:
            for _, shape, raw in split_items(src_root, name, class_choice):
                rel = os.path.join(shape, os.path.basename(raw))
                dst = os.path.join(dst_root, rel)
                if rel not in seen and (overwrite or not os.path.exists(dst)):
                    todo.append((raw, dst))
                seen.add(rel)
        if overwrite or not os.path.exists(os.path.join(dst_root, name)):
            shutil.copyfile(src, os.path.join(dst_root, name))
    if not seen:
        raise ValueError("no shape of %s in the split files of %s" % (class_choice, src_root))
    done = []
    for g in range(0, len(todo), batch):
        rows = [_read_rows(raw) for raw, _ in todo[g:g + batch]]
        K = min(num_points, max(len(xyz) for _, xyz in rows))
        orders = order_fn([xyz for _, xyz in rows], K)
        for (raw, dst), (lines, xyz), order in zip(todo[g:g + batch], rows, orders):
            keep = [int(j) for j in list(order)[:min(num_points, len(lines))]]
            if len(keep) != min(num_points, len(lines)) or len(set(keep)) != len(keep) or min(keep) < 0 or max(keep) >= len(lines):
                raise RuntimeError("order_fn returned no valid order for %s" % raw)
            os.makedirs(os.path.dirname(dst), exist_ok=True)
            with open(dst, "w") as f:
                f.write("".join(lines[j] + "\n" for j in keep))
            done.append(dst)
    return done


# --------------------------------------------------------------------------------------------------------------
# reader
# --------------------------------------------------------------------------------------------------------------
def neg_u_order(seed, split, index, size):
    """The shuffled index through which item `index` of `split` picks its far points (modelnet_dataset.py:130-137: the outside-the-ball
    rows are the file's last 10 %, so the first npoints of a shuffle are taken, once, when the item is first built)."""
    return np.random.default_rng([seed, 0 if split == "train" else 1, index]).permutation(size)


class _LabelFileItems:
    """The `items` of SyntheticDistanceDataset, read from label files on first use and cached in memory."""

    def __init__(self, ds):
        self.ds = ds
        self.cache = {}

    def __len__(self):
        return len(self.ds.datapath)

    def __getitem__(self, index):
        index = int(index)
        if index not in self.cache:
            self.cache[index] = self.ds._load_item(index)
        return self.cache[index]


class ModelNetDistanceDataset(SyntheticDistanceDataset):
    """Items of modelnet_dataset.ModelNetDataset (:98-146): point_set [3*npoints,3] = first npoints of pos | first npoints of neg_l |
    npoints of neg_u through a shuffled index, labels [2*npoints] = column 3 of the two negative sets.  reset / has_next_batch /
    next_batch(augment) / num_channel, the per-fetch permutation shared by the five blocks and the y-rotation + shift augmentation are
    SyntheticDistanceDataset's.  (The reference returns an item unpermuted on the fetch that fills its cache; here every fetch permutes.)"""

    def __init__(self, root, batch_size, npoints, split, class_choice=None, shuffle=None, seed=0, num_neg_points=10 ** 4):
        assert split in ("train", "test")
        self.root, self.npoints, self.batch_size, self.split = root, npoints, batch_size, split
        self.seed, self.num_neg_points = seed, num_neg_points
        self.cat = _lines(os.path.join(root, NAMES_FILE))
        self.classes = dict(zip(self.cat, range(len(self.cat))))
        self.datapath = [(name, raw) for _, name, raw in split_items(root, SPLIT_FILES[split], class_choice)]
        if not self.datapath:
            raise ValueError("no shape of %s in %s" % (class_choice, os.path.join(root, SPLIT_FILES[split])))
        self.shuffle = (split == "train") if shuffle is None else shuffle
        self.items = _LabelFileItems(self)
        self._rng = np.random.default_rng(seed + 17)
        self.reset()

    def _load_item(self, index):
        n = self.npoints
        mats = []
        for p in label_paths(self.datapath[index][1], self.num_neg_points):
            if not os.path.exists(p):
                raise FileNotFoundError("%s is missing: write the distance labels first with `%s`" % (p, generator_hint(self.root)))
            mats.append(np.loadtxt(p, delimiter=",", ndmin=2).astype(np.float32))
        pos, neg_l, neg_u = mats
        if min(len(pos), len(neg_l), len(neg_u)) < n:
            raise ValueError("%s holds fewer than npoints = %d rows" % (self.datapath[index][1], n))
        pick = neg_u_order(self.seed, self.split, index, len(neg_u))[:n]
        pts = np.concatenate([pos[:n, :3], neg_l[:n, :3], neg_u[pick, :3]], 0)
        lab = np.concatenate([neg_l[:n, 3], neg_u[pick, 3]], 0)
        return pts, lab


def main(argv=None):
    p = argparse.ArgumentParser(description="write the DPDist distance-label files next to a ModelNet-style tree")
    p.add_argument("--root", required=True, help="directory with modelnet40_{shape_names,train,test}.txt and <shape>/<id>.txt")
    p.add_argument("--only_chair", action="store_true")
    p.add_argument("--num_neg_points", type=int, default=10 ** 4)
    p.add_argument("--candidates", type=int, default=50000)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--overwrite", action="store_true")
    p.add_argument("--resample_from", default=None, help="first write --root from this tree, every shape file in farthest-point order")
    p.add_argument("--fps_points", type=int, default=10 ** 4, help="rows kept per shape by --resample_from")
    F = p.parse_args(argv)
    if F.resample_from:
        wrote = resample_tree(F.resample_from, F.root, num_points=F.fps_points, class_choice=["chair"] if F.only_chair else None,
                              overwrite=F.overwrite)
        print("resampled %d shapes into %s" % (len(wrote), F.root))
    done = generate_distance_dataset(F.root, class_choice=["chair"] if F.only_chair else None, num_neg_points=F.num_neg_points,
                                     candidates=F.candidates, seed=F.seed, overwrite=F.overwrite, verbose=True)
    print("label files written for %d shapes" % len(done))


if __name__ == "__main__":
    main()

"""The registration test protocol without a GPU: argument errors of the four entries of csrc/regtest.hip, a numpy restatement of the
reference's occlusion (the GPU test compares dpd_occlude against it), the success buckets and the result files."""
import ctypes

import numpy as np
import pytest
import torch


@pytest.fixture(scope="module")
def lib():
    from dpdist_amd import build, lib as L
    build.build(verbose=False)          # hipcc cross-compiles gfx950 without a GPU
    return L.load()


def add_occlusions_np(source, seed_idx, drop, perms=None, return_index=False):
    """helper.add_occlusions (helper.py:963-982) with its random draws passed in: seed_idx [B] is its rand_ind, perms[b] -- a
    permutation of range(N - drop), None = the identity -- is what np.random.shuffle does to the surviving indices.  The argsort is the
    stable one, so equal distances keep their index order.  source [B,N,3] float32."""
    source = np.asarray(source)
    assert source.dtype == np.float32
    B, N, _ = source.shape
    out, kept = [], []
    for b in range(B):
        s = source[b]
        dist = np.linalg.norm(s - s[seed_idx[b]], 2, -1)
        indexes = np.argsort(dist, kind="stable")[drop:]
        if perms is not None and perms[b] is not None:
            indexes = indexes[np.asarray(perms[b])]
        idx = indexes
        while idx.shape[0] < N:                   # concatenate with itself, then truncate: row j is survivor j mod S
            idx = np.concatenate([idx, idx], 0)
        idx = idx[:N]
        out.append(s[idx])
        kept.append(idx)
    out, kept = np.stack(out), np.stack(kept).astype(np.int32)
    return (out, kept) if return_index else out


def key_permutation(source, seed_idx, drop, key):
    """The permutation of the survivors that dpd_occlude's order_key stands for: ascending (key, index) among them."""
    perms = []
    for b in range(source.shape[0]):
        dist = np.linalg.norm(source[b] - source[b, seed_idx[b]], 2, -1)
        indexes = np.argsort(dist, kind="stable")[drop:]
        perms.append(np.lexsort((indexes, key[b, indexes])))
    return perms


@pytest.mark.parametrize("N,drop", [(64, 16), (100, 37), (64, 0), (64, 63)])
def test_occlusion_restatement_properties(N, drop):
    rng = np.random.default_rng(7)
    B, S = 3, N - drop
    src = rng.uniform(-1, 1, (B, N, 3)).astype(np.float32)
    seed = rng.integers(0, N, B)
    perms = [rng.permutation(S) for _ in range(B)]
    for pm in (None, perms):
        out, kept = add_occlusions_np(src, seed, drop, pm, return_index=True)
        assert out.shape == (B, N, 3) and kept.shape == (B, N)
        for b in range(B):
            dist = np.linalg.norm(src[b] - src[b, seed[b]], 2, -1)
            removed = np.setdiff1d(np.arange(N), kept[b])
            assert len(removed) == drop
            if drop:                                          # the removed set is the `drop` nearest points (the seed point among them)
                assert dist[removed].max() <= dist[kept[b]].min() and seed[b] in removed
            assert np.array_equal(out[b], src[b, kept[b]])
            assert np.array_equal(kept[b], kept[b, :S][np.arange(N) % S])      # row j is survivor j mod S
            counts = np.bincount(kept[b], minlength=N)[np.unique(kept[b])]
            assert set(counts) <= {N // S, -(-N // S)} and counts.sum() == N
            if pm is None:                                    # without a shuffle the survivors come in distance order
                assert (np.diff(dist[kept[b, :S]]) >= 0).all()
    key = rng.random((B, N)).astype(np.float32)
    _, kept = add_occlusions_np(src, seed, drop, key_permutation(src, seed, drop, key), return_index=True)
    for b in range(B):
        assert (np.diff(key[b, kept[b, :S]]) >= 0).all()


def test_argument_errors_without_gpu(lib):
    """Argument validation happens before any HIP call: nothing is dereferenced, nothing is launched."""
    p = ctypes.c_void_p(1 << 30)          # any non-NULL "device address"
    # dpd_occlude(src, seed_idx, order_key, B, N, drop, out, kept, stream)
    assert lib.dpd_occlude(None, p, None, 1, 64, 16, p, None, None) == -1
    assert lib.dpd_occlude(p, None, None, 1, 64, 16, p, None, None) == -1
    assert lib.dpd_occlude(p, p, None, 1, 64, 16, None, None, None) == -1
    assert lib.dpd_occlude(p, p, p, 0, 64, 16, p, p, None) == -2
    assert lib.dpd_occlude(p, p, p, 1, 0, 0, p, p, None) == -2
    assert lib.dpd_occlude(p, p, p, 1, 64, -1, p, p, None) == -2
    assert lib.dpd_occlude(p, p, p, 1, 64, 64, p, p, None) == -2          # an empty survivor set
    assert lib.dpd_occlude(p, p, p, 1, 2049, 16, p, p, None) == -3         # beyond the reference's MAX_NUM_POINT
    # dpd_pose_trace(pred, L, B, lim_rot_deg, gt_pose, shift, T_all, te, re, ce, stream)
    assert lib.dpd_pose_trace(None, 8, 5, 45.0, p, None, p, p, p, p, None) == -1
    assert lib.dpd_pose_trace(p, 8, 5, 45.0, p, None, None, None, None, None, None) == -1      # nothing asked for
    assert lib.dpd_pose_trace(p, 8, 5, 45.0, None, None, p, p, None, None, None) == -1         # te needs the ground truth
    assert lib.dpd_pose_trace(p, 8, 5, 45.0, None, None, p, None, p, None, None) == -1         # re too
    assert lib.dpd_pose_trace(p, 0, 5, 45.0, p, None, p, p, p, p, None) == -2
    assert lib.dpd_pose_trace(p, 8, 0, 45.0, p, None, p, p, p, p, None) == -2
    # dpd_chamfer_sqrt_fwd / _bwd: the argument lists of dpd_chamfer_fwd / _bwd
    assert lib.dpd_chamfer_sqrt_fwd(None, p, 1, 64, 64, p, p, p, p, p, None) == -1
    assert lib.dpd_chamfer_sqrt_fwd(p, p, 1, 64, 64, p, p, p, p, None, None) == -1
    assert lib.dpd_chamfer_sqrt_fwd(p, p, 0, 64, 64, p, p, p, p, p, None) == -2
    assert lib.dpd_chamfer_sqrt_fwd(p, p, 1, 64, 0, p, p, p, p, p, None) == -2
    assert lib.dpd_chamfer_sqrt_fwd(p, p, 1, 4097, 64, p, p, p, p, p, None) == -3
    assert lib.dpd_chamfer_sqrt_bwd(p, p, 1, 64, 64, None, p, 1.0, p, p, None) == -1
    assert lib.dpd_chamfer_sqrt_bwd(p, p, 1, 64, 64, p, p, 1.0, None, None, None) == -1       # neither gradient asked for
    assert lib.dpd_chamfer_sqrt_bwd(p, p, 1, 0, 64, p, p, 1.0, p, p, None) == -2
    assert lib.dpd_chamfer_sqrt_bwd(p, p, 1, 64, 4097, p, p, 1.0, p, None, None) == -3


def test_wrappers_refuse_cpu_tensors_and_other_dtypes(lib):
    from dpdist_amd import regtest
    with pytest.raises(RuntimeError, match="GPU"):
        regtest.occlude(torch.zeros(2, 64, 3), 0.25)
    with pytest.raises(RuntimeError, match="GPU"):
        regtest.add_noise(torch.zeros(2, 64, 3))
    with pytest.raises(RuntimeError, match="GPU"):
        regtest.chamfer_sqrt(torch.zeros(2, 64, 3), torch.zeros(2, 64, 3))
    with pytest.raises(RuntimeError, match="GPU"):
        regtest.pose_trace(torch.zeros(8, 2, 7), torch.zeros(2, 6))
    with pytest.raises(RuntimeError, match="GPU"):
        regtest.occlude_with(torch.zeros(2, 64, 3), torch.zeros(2, dtype=torch.int32), None, 16)


def test_buckets_are_nested_like_the_reference():
    from dpdist_amd import regtest
    #                 0     1     2     3     4      5     6     7
    rot = np.array([1.0, 2.4, 2.6, 4.9, 7.0, 15.0, 25.0, 1.0])
    tra = np.array([0.01, 0.06, 0.04, 0.04, 0.09, 0.15, 0.01, 0.3])
    b = regtest.buckets(tra, rot)
    assert b == {"idxs_20_2": [0, 1, 2, 3, 4, 5], "idxs_10_1": [0, 1, 2, 3, 4], "idxs_5_5": [0, 2, 3], "idxs_25_5": [0]}
    # pair 1: 2.4 degrees but 0.06 off -- outside 5 / 0.05, hence outside 2.5 as well (the reference nests the ifs)
    assert set(b["idxs_25_5"]) <= set(b["idxs_5_5"]) <= set(b["idxs_10_1"]) <= set(b["idxs_20_2"])
    assert regtest.buckets(np.array([0.2]), np.array([20.0])) == {k: [] for k in b}          # the bounds are strict


def test_summary_and_result_files_round_trip(tmp_path):
    from dpdist_amd import regtest
    rng = np.random.default_rng(3)
    TE, RE = rng.uniform(0, 0.3, (4, 6)), rng.uniform(0, 30, (4, 6))
    CE = np.concatenate([np.ones((1, 6)), rng.uniform(0, 1e-3, (3, 6))])
    res = regtest.summarize(TE, RE, CE, seconds=0.5)
    assert res["pairs"] == 6 and res["iterations"] == 3 and res["pairs_per_s"] == 12.0
    per = res["per_iteration"]
    assert np.array_equal(per["rot_mean"], RE.mean(1)) and np.array_equal(per["rot_std"], RE.std(1))
    assert np.array_equal(per["trans_mean"], TE.mean(1)) and np.array_equal(per["conv_mean"], CE.mean(1))
    assert res["buckets"] == regtest.buckets(TE[-1], RE[-1])          # the final transform decides the bucket
    npz, txt = regtest.write_results(str(tmp_path / "log"), res)
    te, re, ce = regtest.read_results(str(tmp_path / "log"))
    assert te.dtype == np.float64 and np.array_equal(te, TE) and np.array_equal(re, RE) and np.array_equal(ce, CE)
    lines = open(txt).read().splitlines()
    assert lines[1] == "Mean Translation Err: {}".format(np.mean(TE[-1])) and lines[3] == "Mean Rotation Err: {}".format(np.mean(RE[-1]))
    assert lines[4] == "Var Rotation Err: {}".format(np.var(RE[-1]))
    heads = [ln for ln in lines if ln.startswith("######")]
    assert heads == ["###### 2.5 Degree & 0.05 Units ######", "###### 5 Degree & 0.05 Units ######", "###### 10 Degree & 0.1 Units ######",
                     "###### 20 Degree & 0.2 Units ######"]
    counts = [int(ln.split(": ")[1]) for ln in lines if ln.startswith("Count: ")]
    assert counts == [len(res["buckets"][k]) for k in ("idxs_25_5", "idxs_5_5", "idxs_10_1", "idxs_20_2")]
    n20 = len(res["buckets"]["idxs_20_2"])
    assert "Accuray: {}%".format(100.0 * n20 / 6) in lines

"""ctypes binding of libdpdist_hip.so (the C ABI of include/dpdist_capi.h).

There is NO fallback: if the shared library is missing or a call fails, a RuntimeError is raised.
Thin typed wrappers (`ops_*`) take torch CUDA tensors, check dtype/contiguity and pass raw device
pointers + the current HIP stream.
"""
import ctypes
import os
from ctypes import c_long, POINTER, Structure, c_char_p, c_float, c_int, c_int32, c_size_t, c_void_p

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libdpdist_hip.so")

_ERR = {-1: "DPD_E_NULL (null pointer)", -2: "DPD_E_DIM (bad dimension)",
        -3: "DPD_E_UNSUPPORTED (unsupported size/configuration)", -4: "DPD_E_WORKSPACE (workspace too small)"}


class DecoderParams(Structure):
    _fields_ = [(n, c_void_p) for n in ("W1p", "b1", "W2", "b2", "W3", "b3", "W4", "b4", "W2T", "W3T", "W1pT")]


class SmallGrads(Structure):
    _fields_ = [(n, c_void_p) for n in ("db1", "db2", "db3", "dW4", "db4", "partials", "l1_pred", "l1_labels", "l1_loss")] + [
        ("l1_gscale", c_float), ("db_partials", c_void_p), ("fwd_y", c_void_p), ("fwd_pred", c_void_p)]


class AdamFuse(Structure):   # include/dpdist_capi.h: dpd_adam_fuse
    _fields_ = [("WT", c_void_p * 3), ("w_off", c_long * 3), ("w_rows", c_int * 3), ("w_cols", c_int * 3),
                ("W_rc", c_void_p * 3), ("W_r8", c_void_p * 3), ("np", c_int), ("partials", c_void_p),
                ("nparts", c_int), ("rec", c_int), ("H", c_int), ("Qb", c_int), ("tail_off", c_long), ("loss", c_void_p)]


class Planes(Structure):     # include/dpdist_capi.h: dpd_planes
    _fields_ = [("np", c_int), ("Q", c_int), ("Qb", c_int)] + [(n, c_void_p) for n in (
        "X_rc", "X_r8", "h1_rc", "h1_r8", "h2_rc", "h2_r8", "g3_rc", "g3_r8", "g2_rc", "g2_r8", "g1_rc", "g1_r8",
        "W1_r8", "W2_r8", "W3_r8", "W1_rc", "W2_rc", "W3_rc", "h3_rc")]


class PoseNetW(Structure):   # include/dpdist_capi.h: dpd_pose_net
    _fields_ = [("Wp", c_void_p * 5), ("bp", c_void_p * 5), ("Wh", c_void_p * 4), ("bh", c_void_p * 4), ("out_features", c_int)]


class AsLoss(Structure):     # include/dpdist_capi.h: dpd_asloss (the as-loss engine; driven by dpdist_amd/asloss.py)
    _fields_ = ([(n, c_int) for n in ("B", "N", "m", "k", "KP", "H", "dtype")] + [("sigma", c_float)] +
                [(n, c_void_p) for n in ("pts", "q", "fv", "ssq", "mask", "vox", "X", "h1", "h2", "h3", "y", "pred", "dy", "g3", "g2", "g1",
                                         "dX", "dfv", "dpts", "W2T", "W3T", "W1pT", "scratch")] +
                [("mfv_ws", c_void_p), ("mfv_ws_bytes", c_size_t), ("ws", c_void_p), ("ws_bytes", c_size_t),
                 ("planes", Planes), ("params", DecoderParams)])


class CrossChunk(Structure):   # include/dpdist_capi.h: dpd_cross_chunk (carved by dpd_cross_carve; driven by dpdist_amd/pairwise.py)
    BUFFERS = ("Xu", "Xt", "uid", "maskr", "cnt", "Pu", "act0", "act1", "Dd", "h1", "h2", "h3", "y", "pred",
               "dpred", "dy", "ga", "gb", "dq", "gs", "dXs", "dfv")
    _fields_ = ([(n, c_int) for n in ("Ca_chunk", "Cb", "N", "m", "k", "KP", "H", "slot_cap", "rows_p")] + [("bytes", c_size_t)] +
                [(n, c_void_p) for n in BUFFERS])


class LiveRows(Structure):     # include/dpdist_capi.h: dpd_live_rows (carved by dpd_live_rows_carve; the caller sets X .. rows_per_cloud)
    _fields_ = ([(n, c_int) for n in ("Qb", "KP", "H")] +
                [(n, c_void_p) for n in ("cnt", "idx", "pos", "rowflag", "g3c", "h1c", "h2c", "Xc", "X")] + [("ldx", c_int), ("ssq", c_void_p),
                                                                                                       ("clouds", c_int), ("rows_per_cloud", c_int)])


class GemmPairPart(Structure):     # include/dpdist_capi.h: dpd_gemm_pair_part (one of the two problems of dpd_gemm_f32_pair)
    _fields_ = ([(n, c_int) for n in ("transA", "transB", "M", "N", "K")] +
                [("A", c_void_p), ("lda", c_int), ("B", c_void_p), ("ldb", c_int), ("C", c_void_p), ("ldc", c_int), ("gate", c_void_p)] +
                [(n, c_int) for n in ("epilogue", "split_k", "tile")] +
                [("M_dev", c_void_p), ("K_dev", c_void_p), ("bias_parts", c_void_p), ("bias_out", c_void_p), ("bias_nparts", c_int)])


# name -> (restype, argtypes); mirrors include/dpdist_capi.h one to one
SIGNATURES = {
    "dpd_version": (c_char_p, []),
    "dpd_padded_width": (c_int, [c_int]),
    "dpd_mfv3d_fwd": (c_int, [c_void_p, c_int, c_int, c_int, c_float, c_void_p, c_void_p]),
    "dpd_mfv3d_bwd": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_void_p, c_void_p, c_size_t, c_void_p]),
    "dpd_mfv3d_bwd_workspace_bytes": (c_size_t, [c_int, c_int]),
    "dpd_mfv3d_fits": (c_int, [c_int, c_int, c_int]),
    "dpd_mfv3d_tile": (c_int, [c_int, c_int]),
    "dpd_mfv3d_fwd_tiled": (c_int, [c_void_p, c_int, c_int, c_int, c_float, c_int, c_void_p, c_void_p]),
    "dpd_mfv3d_bwd_tiled": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "dpd_patch_rows_fwd": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p,
                                   c_void_p, POINTER(Planes), c_void_p]),
    "dpd_mfv3d_fwd_stacked": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_void_p, c_void_p, c_void_p,
                                      c_void_p, c_void_p]),
    "dpd_patch_rows_fwd_scaled": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p,
                                          c_void_p, POINTER(Planes), c_void_p]),
    "dpd_patch_rows_unique_scratch_bytes": (c_size_t, [c_int, c_int]),
    "dpd_patch_rows_fwd_unique": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p,
                                          c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "dpd_decoder_fwd_unique": (c_int, [c_void_p] * 6 + [c_int, c_int, c_int, POINTER(DecoderParams)] + [c_void_p] * 6),
    "dpd_cross_slot_capacity": (c_int, [c_int] * 4),
    "dpd_cross_workspace_bytes": (c_size_t, [c_int] * 7),
    "dpd_cross_carve": (c_int, [c_void_p, c_size_t] + [c_int] * 8 + [POINTER(CrossChunk)]),
    "dpd_cross_index": (c_int, [c_void_p, c_int, c_int, c_int] + [c_void_p] * 5),
    "dpd_cross_gather": (c_int, [c_void_p] * 7 + [c_int] * 6 + [c_void_p, c_int] + [c_void_p] * 5),
    "dpd_decoder_fwd_cross": (c_int, [c_void_p, c_int, c_int] + [c_void_p] * 5 + [c_int] * 4 + [POINTER(DecoderParams)] + [c_void_p] * 6),
    "dpd_cross_bwd_workspace_bytes": (c_size_t, [c_int] * 7),
    "dpd_cross_invert": (c_int, [c_void_p] * 3 + [c_int] * 3 + [c_void_p] * 4),
    "dpd_decoder_fwd_cross_keep": (c_int, [c_void_p, c_int, c_int] + [c_void_p] * 5 + [c_int] * 4 + [POINTER(DecoderParams)] + [c_void_p] * 7),
    "dpd_cross_slot_sum": (c_int, [c_void_p] * 5 + [c_int] * 8 + [c_void_p] * 3),
    "dpd_cross_scatter": (c_int, [c_void_p] * 3 + [c_int] * 6 + [c_void_p] * 2),
    "dpd_cross_bwd": (c_int, [c_void_p] * 10 + [c_int] * 8 + [POINTER(DecoderParams)] + [c_void_p] * 10),
    # ragged sets: the per-cloud-count twins (counts / qcounts: int32 device memory)
    "dpd_mfv3d_fwd_counts": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_int, c_void_p, c_void_p]),
    "dpd_mfv3d_bwd_counts": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "dpd_cross_index_counts": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int] + [c_void_p] * 5),
    "dpd_decoder_fwd_cross_counts": (c_int, [c_void_p, c_int, c_int] + [c_void_p] * 6 + [c_int] * 5 + [POINTER(DecoderParams)] + [c_void_p] * 6),
    "dpd_cross_bwd_counts": (c_int, [c_void_p] * 11 + [c_int] * 8 + [POINTER(DecoderParams)] + [c_void_p] * 10),
    # paired distances of clouds of different sizes (dpdist_amd/pairs.py)
    "dpd_patch_rows_fwd_counts": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "dpd_decoder_out_pairs": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int, POINTER(DecoderParams)] + [c_void_p] * 6),
    "dpd_pairs_combine": (c_int, [c_void_p] * 5 + [c_int] * 3 + [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    # per-point field (dpdist_amd/field.py)
    "dpd_field_slot_capacity": (c_int, [c_int] * 3),
    "dpd_field_index": (c_int, [c_void_p, c_long, c_void_p] + [c_int] * 4 + [c_void_p] * 5),
    "dpd_field_gather": (c_int, [c_void_p, c_long] + [c_void_p] * 5 + [c_int] * 5 + [c_void_p, c_int] + [c_void_p] * 5),
    "dpd_decoder_fwd_field": (c_int, [c_void_p, c_int, c_int] + [c_void_p] * 5 + [c_int] * 3 + [POINTER(DecoderParams)] + [c_void_p] * 5),
    # ... its slot-summed backward (csrc/field_bwd.hip)
    "dpd_field_invert": (c_int, [c_void_p] * 3 + [c_int] * 4 + [c_void_p] * 5),
    "dpd_field_slot_sum": (c_int, [c_void_p] * 6 + [c_int] * 7 + [c_void_p, c_void_p, c_long, c_void_p]),
    "dpd_field_scatter": (c_int, [c_void_p] * 3 + [c_int] * 6 + [c_void_p] * 2),
    "dpd_field_bwd": (c_int, [c_void_p] * 12 + [c_int] * 7 + [POINTER(DecoderParams)] + [c_void_p] * 7 + [c_int, c_void_p, c_long, c_void_p]),
    # ... with the decoder's own gradients (csrc/field_train.hip)
    "dpd_field_bwd_train_workspace_bytes": (c_size_t, [c_int] * 6),
    "dpd_field_bwd_train": (c_int, [c_void_p] * 12 + [c_void_p, c_int, c_void_p] + [c_int] * 7 + [POINTER(DecoderParams)] + [c_void_p] * 7 +
                            [c_int, c_void_p, c_long] + [c_void_p] * 8 + [c_int, c_void_p, c_size_t, c_void_p]),
    "dpd_decoder_out_asloss": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, POINTER(DecoderParams), c_float, c_void_p, c_void_p, c_void_p, c_void_p,
                                       c_void_p, c_void_p, c_void_p]),
    "dpd_decoder_out_asloss_planes": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, POINTER(DecoderParams), c_float, c_void_p, c_void_p, c_void_p,
                                              c_void_p, c_void_p, POINTER(Planes), c_void_p, c_void_p]),
    "dpd_asloss_tail": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_float, c_void_p, c_void_p, c_size_t,
                                c_void_p, c_void_p, c_void_p]),
    "dpd_asloss_combine": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "dpd_patch_rows_bwd": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p,
                                   c_void_p]),
    "dpd_decoder_fwd": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, POINTER(DecoderParams), c_int, c_void_p,
                                c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, POINTER(Planes), c_void_p]),
    "dpd_decoder_bwd_data": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                                     POINTER(DecoderParams), c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                     POINTER(SmallGrads), c_void_p, c_size_t, POINTER(Planes), c_int, c_void_p]),
    "dpd_stack_clouds": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "dpd_decoder_bwd_weights": (c_int, [c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_void_p,
                                        c_void_p, c_void_p, c_size_t, POINTER(Planes), c_void_p, c_void_p]),
    "dpd_decoder_bwd_weights_pair": (c_int, [c_void_p] * 6 + [c_int] * 5 + [c_void_p, c_size_t, POINTER(Planes), c_void_p, c_void_p, c_void_p]),
    "dpd_live_rows_bytes": (c_size_t, [c_int, c_int, c_int]),
    "dpd_live_rows_carve": (c_int, [c_void_p, c_size_t, c_int, c_int, c_int, POINTER(LiveRows)]),
    "dpd_decoder_bwd_data_live": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                                          POINTER(DecoderParams), c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                          POINTER(SmallGrads), c_void_p, c_size_t, POINTER(Planes), c_int, POINTER(LiveRows), c_void_p]),
    "dpd_decoder_bwd_weights_live": (c_int, [c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_void_p,
                                             c_void_p, c_void_p, c_size_t, POINTER(Planes), c_void_p, POINTER(LiveRows), c_void_p]),
    "dpd_decoder_bwd_weights_pair_live": (c_int, [c_void_p] * 6 + [c_int] * 5 + [c_void_p, c_size_t, POINTER(Planes), c_void_p, c_void_p,
                                                                                 POINTER(LiveRows), c_void_p]),
    "dpd_decoder_bwd_pair_live": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, POINTER(DecoderParams), POINTER(LiveRows), c_void_p]),
    "dpd_decoder_bwd_chain_live": (c_int, [c_void_p] * 6 + [c_int, c_int, c_int, POINTER(DecoderParams)] + [c_void_p] * 4 +
                                           [POINTER(SmallGrads), c_void_p, c_size_t, c_int] + [c_void_p] * 5 + [POINTER(LiveRows), c_void_p]),
    "dpd_decoder_bwd_weights_trio": (c_int, [c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, POINTER(Planes), c_void_p]),
    "dpd_crc32c": (ctypes.c_uint32, [c_void_p, c_size_t, ctypes.c_uint32]),
    "dpd_chamfer_fwd": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int] + [c_void_p] * 6),
    "dpd_chamfer_bwd": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_void_p]),
    # all-pairs Chamfer / Hausdorff (dpdist_amd/baselines.py): S, countsS, Cs, Ns, Q, countsQ, Cq, Nq, ...
    "dpd_chamfer_matrix_fwd": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_int, c_int] + [c_void_p] * 4),
    "dpd_chamfer_matrix_bwd": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_int] + [c_void_p] * 4),
    "dpd_nn_dist": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    # farthest-point sampling (dpdist_amd/sampling.py): pts, counts, start, S, W, K, order, radius, ws, ws_bytes, stream
    "dpd_fps_workspace_bytes": (c_size_t, [c_int, c_int]),
    "dpd_fps_order": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "dpd_fps_gather_fwd": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "dpd_fps_gather_bwd": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "dpd_emd_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "dpd_emd_fwd": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_float] + [c_void_p] * 6 + [c_size_t, c_void_p]),
    "dpd_emd_match_cost": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_float] + [c_void_p] * 5 + [c_size_t, c_void_p]),
    "dpd_emd_matrix_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "dpd_emd_matrix_fwd": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_int, c_int] + [c_void_p] * 3),
    "dpd_emd_matrix_bwd": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_int, c_int] + [c_void_p] * 3 +
                           [c_int, c_void_p, c_size_t, c_void_p]),
    # the baselines per pair, ragged (baselines.py, emd.py): A, countsA, Wa, B, countsB, Wb, P, ...
    "dpd_chamfer_pairs_fwd": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int] + [c_void_p] * 8),
    "dpd_chamfer_pairs_bwd": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_int] + [c_void_p] * 7),
    "dpd_emd_pairs_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "dpd_emd_pairs_fwd": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_int] + [c_void_p] * 3 + [c_size_t, c_void_p]),
    "dpd_emd_pairs_bwd": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_int] + [c_void_p] * 4 + [c_size_t, c_void_p]),
    "dpd_pose_apply_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_float, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "dpd_pose_apply_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_float, c_void_p, c_void_p]),
    "dpd_pose_refine_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "dpd_pose_refine": (c_int, [POINTER(PoseNetW), c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_void_p, c_void_p, c_size_t, c_void_p,
                                c_void_p, c_void_p, c_void_p]),
    "dpd_pose_refine_pool": (c_int, [POINTER(PoseNetW), c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_int, c_void_p, c_void_p, c_size_t, c_void_p,
                                     c_void_p, c_void_p, c_void_p]),
    "dpd_occlude": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "dpd_pose_trace": (c_int, [c_void_p, c_int, c_int, c_float] + [c_void_p] * 7),
    "dpd_chamfer_sqrt_fwd": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int] + [c_void_p] * 6),
    "dpd_chamfer_sqrt_bwd": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_void_p]),
    "dpd_pose_point_bwd_workspace_bytes": (c_size_t, [c_int]),
    "dpd_pose_point_bwd_workspace_bytes_n": (c_size_t, [c_int, c_int]),
    "dpd_pose_point_tie_words": (c_int, [c_int]),
    "dpd_pose_point_fwd_train": (c_int, [POINTER(PoseNetW), c_void_p, c_void_p, c_int, c_int, c_int] + [c_void_p] * 7),
    "dpd_pose_point_bwd": (c_int, [POINTER(PoseNetW), c_void_p, c_void_p, c_int, c_int, c_int] + [c_void_p] * 6 +
                           [POINTER(c_void_p), POINTER(c_void_p), c_void_p, c_size_t, c_void_p]),
    "dpd_pose_point_bwd_workspace_bytes_pool": (c_size_t, [c_int, c_int, c_int]),
    "dpd_pose_point_fwd_train_pool": (c_int, [POINTER(PoseNetW), c_void_p, c_void_p, c_int, c_int, c_int, c_int] + [c_void_p] * 7),
    "dpd_pose_point_bwd_pool": (c_int, [POINTER(PoseNetW), c_void_p, c_void_p, c_int, c_int, c_int, c_int] + [c_void_p] * 6 +
                                [POINTER(c_void_p), POINTER(c_void_p), c_void_p, c_size_t, c_void_p]),
    "dpd_pose_head_bwd_workspace_bytes": (c_size_t, [c_int]),
    "dpd_pose_head_fwd_train": (c_int, [POINTER(PoseNetW), c_void_p, c_int] + [c_void_p] * 6),
    "dpd_pose_head_bwd": (c_int, [POINTER(PoseNetW), c_void_p, c_int] + [c_void_p] * 5 + [POINTER(c_void_p), POINTER(c_void_p), c_void_p, c_void_p,
                                                                                           c_size_t, c_void_p]),
    "dpd_planes_bytes": (c_size_t, [c_int] * 6),
    "dpd_planes_carve": (c_int, [c_void_p, c_size_t] + [c_int] * 6 + [POINTER(Planes)]),
    "dpd_weights_to_planes": (c_int, [POINTER(DecoderParams), c_int, c_int, POINTER(Planes), c_void_p]),
    "dpd_asloss_bytes": (c_size_t, [c_int] * 6),
    "dpd_asloss_carve": (c_int, [c_void_p, c_size_t] + [c_int] * 6 + [c_float, POINTER(AsLoss)]),
    "dpd_asloss_init": (c_int, [POINTER(AsLoss), c_void_p]),
    "dpd_asloss_set_weights": (c_int, [POINTER(AsLoss), POINTER(DecoderParams), c_void_p]),
    "dpd_asloss_forward": (c_int, [POINTER(AsLoss), c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    "dpd_asloss_backward": (c_int, [POINTER(AsLoss), c_void_p, c_void_p, c_void_p, c_void_p]),
    "dpd_asloss_forward_backward": (c_int, [POINTER(AsLoss), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "dpd_weights_transpose": (c_int, [POINTER(DecoderParams), c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "dpd_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "dpd_split_planes": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_long, c_void_p, c_long, c_void_p]),
    "dpd_gemm_planes": (c_int, [c_int] * 6 + [c_void_p, c_int, c_long, c_void_p, c_int, c_long, c_void_p, c_int, c_void_p,
                                c_void_p, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p]),
    "dpd_l1_loss": (c_int, [c_void_p, c_void_p, c_int, c_int, c_float, c_void_p, c_void_p, c_void_p]),
    "dpd_adam_tf": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_float, c_float, c_float, c_float,
                            c_float, c_void_p]),
    "dpd_adam_tf_fused": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_float, c_float, c_float, c_float, c_float,
                                  POINTER(AdamFuse), c_void_p]),
    "dpd_adam_tf_dev": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_float, c_float, c_float, c_float, c_void_p]),
    "dpd_gemm_f32": (c_int, [c_int, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int,
                             c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_size_t, c_void_p]),
    "dpd_gemm_f32_pair": (c_int, [POINTER(GemmPairPart), POINTER(GemmPairPart), c_void_p]),
    "dpd_set_gemm_plan": (c_int, [c_int, c_int, c_int]),
    "dpd_prof_enable": (c_int, [c_int]),
    "dpd_prof_enabled": (c_int, []),
    "dpd_prof_collect_form": (c_int, [c_int, POINTER(ctypes.c_double), POINTER(ctypes.c_double)]),
    "dpd_prof_collect": (c_int, [POINTER(ctypes.c_double), POINTER(ctypes.c_double)]),
    "dpd_prof_collect_stage": (c_int, [c_int, POINTER(ctypes.c_double), POINTER(ctypes.c_double)]),
}

_lib = None


def load():
    """Load the shared library (once).  Raises RuntimeError when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("libdpdist_hip.so not found at %s -- run `python -m dpdist_amd.build` "
                           "(there is no CPU fallback)" % LIB_PATH)
    # Load order matters: the PyTorch-ROCm wheel bundles its own libamdhip64.so.7 / libhsa-runtime64.so.1.  Import
    # torch FIRST so that our DT_NEEDED entries resolve to the HIP runtime torch already initialised; loading this
    # library first would pull /opt/rocm's runtime next to torch's and every launch would fail with hipErrorNoDevice.
    import torch  # noqa: F401
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)      # AttributeError here == header/library mismatch
        fn.restype, fn.argtypes = res, args
    _lib = lib
    return lib


DTYPES = {"f32": 0, "f32x3": 1, "bf16": 2, 0: 0, 1: 1, 2: 2}   # include/dpdist_capi.h: enum dpd_dtype
POOLS = {"max": 0, "avg": 1}                                   # include/dpdist_capi.h: enum dpd_pool


def check(rc, what):
    if rc == 0:
        return
    if rc < 0:
        raise RuntimeError("%s failed: %s" % (what, _ERR.get(rc, rc)))
    raise RuntimeError("%s failed: hipError_t %d" % (what, rc))


def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def cur_stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def req(t, dtype=None, name="tensor", shape=None, numel=None):
    """Boundary check of a tensor handed to the C ABI (which only sees a raw pointer): device, dtype, contiguity and --
    when given -- the exact shape / element count the entry point will read or write."""
    import torch
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise RuntimeError("%s must have shape %s, got %s" % (name, tuple(shape), tuple(t.shape)))
    if numel is not None and t.numel() != numel:
        raise RuntimeError("%s must have %d elements, got %d" % (name, numel, t.numel()))
    if not t.is_cuda:
        raise RuntimeError("%s must live on the GPU (dpdist_amd has no CPU path)" % name)
    if dtype is None:
        dtype = torch.float32
    if t.dtype != dtype:
        raise RuntimeError("%s must be %s, got %s" % (name, dtype, t.dtype))
    if not t.is_contiguous():
        raise RuntimeError("%s must be contiguous" % name)
    return t


def make_params(W1p, b1, W2, b2, W3, b3, W4, b4, W2T=None, W3T=None, W1pT=None):
    return DecoderParams(*[None if t is None else t.data_ptr() for t in (W1p, b1, W2, b2, W3, b3, W4, b4, W2T, W3T, W1pT)])


def make_small_grads(db1, db2, db3, dW4, db4, partials=None, l1_pred=None, l1_labels=None, l1_loss=None, l1_gscale=1.0,
                     db_partials=None, fwd_y=None, fwd_pred=None):
    return SmallGrads(*[None if t is None else t.data_ptr() for t in (db1, db2, db3, dW4, db4, partials, l1_pred, l1_labels, l1_loss)],
                      float(l1_gscale), *[None if t is None else t.data_ptr() for t in (db_partials, fwd_y, fwd_pred)])

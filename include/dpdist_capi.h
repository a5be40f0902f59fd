/*
 * dpdist_capi.h -- C ABI of the MI355X-native DPDist hot path (libdpdist_hip.so).
 *
 * The reference (dahliau/DPDist) has no FFI: its boundary is the Python model-module contract
 *     models/dpdist_and_aue.py:23-86,203-204   placeholder_inputs / get_model / get_loss
 * whose body is ~60 primitive TensorFlow ops in utils/dpdist_util.py.  Each entry point below
 * replaces one group of those ops (file:line cited per function); dpdist_amd/model.py re-assembles
 * them behind the same get_model/get_loss signatures.  INTEGRATION.md shows the ctypes binding.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to contiguous row-major float32 unless stated otherwise;
 *   - the caller owns every buffer: the library never allocates or frees device memory.  Process-wide state is limited to
 *     (a) the GEMM tuning table of dpd_set_gemm_plan (defaults = measured best; not synchronised: set it before use),
 *     (b) the opt-in profiler of dpd_prof_enable (off by default, mutex-protected, owns hipEvents while on) and
 *     (c) a per-(kernel, device) "large LDS opted in" flag set on a kernel's first launch on that device;
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it and is asynchronous;
 *   - return value: 0 = ok, <0 = argument error (DPD_E_*), >0 = the hipError_t of the failing call;
 *   - thread-safe / re-entrant: safe from several host threads on distinct streams.
 *
 * Shapes: C clouds of N points; grid side m (G = m^3 Gaussians == voxels); window side k;
 *   F = 20 Fisher features per Gaussian; E = k^3*F (2500); rows Q = C*N query points, row r = c*N+n
 *   is query point n of query-cloud c evaluated against the Fisher vector fv[c].
 *   The module contract stacks clouds as  pts = [pcA+noise ; pcB],  q = [pcB ; pcA]  (C = 2B).
 *   Decoder input row layout (internal, 16-byte friendly):  X[r] = [ emb(E) | q-centre (3) | 0-pad ]
 *   with leading dimension KP = dpd_padded_width(k) (2528 for k=5: a whole number of 32-deep K-tiles).  W1 is held in the matching
 *   row order: W1p[0:E] = tf_weights1[3:3+E], W1p[E:E+3] = tf_weights1[0:3], zero pad rows.
 */
#ifndef DPDIST_CAPI_H
#define DPDIST_CAPI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DPD_FV_CHANNELS 20
#define DPD_OUT_CHANNELS 3

enum {
    DPD_OK = 0,
    DPD_E_NULL = -1,      /* a required pointer is NULL */
    DPD_E_DIM = -2,       /* non-positive or inconsistent dimension */
    DPD_E_UNSUPPORTED = -3, /* m > 10, k even, k > 7, N > 4096, widths not a multiple of 64 ... */
    DPD_E_WORKSPACE = -4  /* workspace too small (see dpd_workspace_bytes) */
};

/* library version / build target, e.g. "dpdist_hip 0.1 gfx950" */
const char* dpd_version(void);

/* KP: leading dimension of the decoder input rows for window side k (k^3*20+3 rounded up to 32). */
int dpd_padded_width(int k);

/* Input stacking of the module contract (models/dpdist_and_aue.py:45,56-61,69): pcA, pcB, noise [B,N,3]
 * (noise may be NULL) -> pts [2B,N,3] = [pcA+noise ; pcB] (encoder input), q [2B,N,3] = [pcB ; pcA] (queries).  */
int dpd_stack_clouds(const float* pcA, const float* pcB, const float* noise, int B, int N, float* pts, float* q,
                     void* stream);

/* ---------------------------------------------------------------------------------------------
 * 3DmFV encoder.  Replaces utils/dpdist_util.py:22-141 (get_3dmfv_tf, full_fv, normalize=True).
 *   pts [C,N,3] -> fv [C,m^3,20]; Gaussians on the fixed grid of :42-51, uniform weights 1/m^3.
 *   A point further than ~1.7 from every centre underflows every pdf and yields NaN exactly as the
 *   reference does (0/0 at :74).
 *   Sizes: 1 <= m <= 10 and 1 <= N <= 4096, else DPD_E_UNSUPPORTED; sigma > 0 (not NaN) and C >= 1, else DPD_E_DIM.  The
 *   limit on N that binds is the kernel's dynamic LDS, which must fit 160 KiB:
 *       4 * (6*N*m + 6*N + 21*ceil(m^3 / 4) + 164) bytes <= 163840
 *   i.e. N <= 705 for m = 8 (704 for the N % 8 == 0 kernel), N <= 538 for m = 10 (536), N <= 3397 even for m = 1; beyond it
 *   DPD_E_UNSUPPORTED, before anything is launched and with fv untouched.  N % 8 == 0 (N >= 8) runs the kernel that takes the
 *   points in pairs, every other N the eight-point-group kernel; both are held to the same bar against the float64 oracle.  */
int dpd_mfv3d_fwd(const float* pts, int C, int N, int m, float sigma, float* fv, void* stream);

/* Backward of the encoder (TF autodiff of :69-126): dfv [C,m^3,20] -> dpts [C,N,3] (overwritten).
 * Max/min gradients are split evenly among ties, like tf.reduce_max/min.                        */
int dpd_mfv3d_bwd(const float* pts, const float* dfv, int C, int N, int m, float sigma, float* dpts, void* ws,
                  size_t ws_bytes, void* stream);
/* ws (optional): dpd_mfv3d_bwd_workspace_bytes(C, m) bytes let the backward run as 4 workgroups per cloud (sliced over
 * the points, three launches) instead of one -- 2-3x faster at the as-loss batch sizes; NULL keeps the one-launch form.
 * Sizes: as the forward, and m <= 8 (one Gaussian per lane pair; m = 9, 10: DPD_E_UNSUPPORTED).  Dynamic LDS, 160 KiB at most:
 *   one launch:  4 * (6*N*m + 52*N + 684) bytes                       (m = 8: N <= 402)
 *   sliced:      4 * (6*n*m + 52*n + 4) bytes with n = ceil(N / 4)    (m = 8: n <= 409, N <= 1636)
 * beyond it DPD_E_UNSUPPORTED with dpts and ws untouched.  The sliced form needs N >= 8; for N < 8 the entry runs the one-launch
 * kernel even when ws is given (ws is then not written).  Slice s holds the points [s*n, min(N, (s+1)*n)): the last slices may
 * be EMPTY (N = 9: 3, 3, 3, 0 -- its record carries -inf / +inf extrema and zero tie counts, which the merge ignores) or hold ONE
 * point (N = 10, 13).  The tie count of a max / min is taken over the whole cloud, across the slices.                        */
size_t dpd_mfv3d_bwd_workspace_bytes(int C, int m);

/* ---------------------------------------------------------------------------------------------
 * The encoder over TILES of points: clouds of any size 1 <= N <= 4096 (the reference registers clouds of 256 .. 2048 points,
 * pcrnet-registration/iterative_PCRNet_ours.py:40,103-104).  Every statistic of utils/dpdist_util.py:78-109 is a sum, a max or a
 * min over the points, so the kernels walk the points in tiles of at most `tile`, rebuild the tables of the tile's points only
 * (their dynamic LDS depends on the tile, not on N) and carry the running statistics in registers across the tiles.  Same maths
 * as the plain entries above, sums in another order: last-bit differences, the same bars against the float64 oracle.  The plain
 * entries, their kernels and their LDS caps are unchanged; callers route to the tiled ones for the shapes those refuse.
 *
 * dpd_mfv3d_fits: 1 if the PLAIN entry takes (N, m), else 0.  which = 0: dpd_mfv3d_fwd; 1: dpd_mfv3d_bwd without a workspace (one
 *   launch); 2: dpd_mfv3d_bwd with a workspace (sliced; N < 8 runs the one-launch kernel there as well).  Host only: the library's own
 *   statement of the LDS caps quoted above, so that no caller restates the formulas.  0 for sizes no entry takes and for any other
 *   `which`.
 * dpd_mfv3d_tile: the tile the tiled entries choose for tile = 0 -- the largest multiple of 8 whose dynamic LDS (below) stays at or
 *   under 64 KiB, i.e. no opt-in attribute and two workgroups per CU.  which = 0 forward (m = 8: 248, m = 10: 168), otherwise
 *   backward (m = 8: 160).  0 where the entry takes no such m.  Host only.
 * dpd_mfv3d_fwd_tiled: pts [C,N,3] -> the NORMALISED fv [C,m^3,20] (per-channel L2 norm applied, as dpd_mfv3d_fwd does; two launches).
 *   1 <= N <= 4096 and 1 <= m <= 10, else DPD_E_UNSUPPORTED; sigma > 0 (not NaN) and C >= 1, else DPD_E_DIM.
 *   tile: 0 = the library's choice; otherwise a multiple of 8, >= 8, whose dynamic LDS fits 160 KiB:
 *       4 * (6*tile*m + 6*tile + 21*ceil(m^3 / 4) + 4) bytes <= 163840
 *   else DPD_E_UNSUPPORTED.  A tile larger than the cloud is cut to N rounded up to 8.  Every refusal happens before anything is
 *   launched and leaves fv untouched.  A point that underflows every pdf (0/0 at :74) yields NaN throughout, in whichever tile it sits.
 * dpd_mfv3d_bwd_tiled: dfv [C,m^3,20] -> dpts [C,N,3] (overwritten), three launches: each of the 4 point slices of the sliced form
 *   (n = ceil(N / 4) points; record layout and merge as there, empty slices included) walks its points in tiles.  m <= 8 as
 *   dpd_mfv3d_bwd; any 1 <= N <= 4096.  ws is REQUIRED: dpd_mfv3d_bwd_workspace_bytes(C, m) bytes, else DPD_E_WORKSPACE.  tile as
 *   above with
 *       4 * (6*tile*m + 52*tile + 4) bytes <= 163840
 *   and cut to n rounded up to 8.  The tie count of a max / min is taken over the whole cloud, across tiles and slices.  Refusals
 *   leave dpts and ws untouched.                                                                                                 */
int dpd_mfv3d_fits(int N, int m, int which);
int dpd_mfv3d_tile(int m, int which);
int dpd_mfv3d_fwd_tiled(const float* pts, int C, int N, int m, float sigma, int tile, float* fv, void* stream);
int dpd_mfv3d_bwd_tiled(const float* pts, const float* dfv, int C, int N, int m, float sigma, int tile, float* dpts, void* ws,
                        size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Query -> voxel lookup + local-window gather.  Replaces local_z_3d (utils/dpdist_util.py:911-930),
 * get_pc_grid_binary_mask_from_centers (:459-492) and get_emb_and_concat (:434-457) WITHOUT
 * materialising the [C,m^3,k^3*20] window tensor.
 *   q [C,N,3], fv [C,m^3,20] -> X [Q,KP] rows, mask [Q] (1/0), vox [Q] (voxel id, 0 if outside). */
typedef struct dpd_planes dpd_planes;   /* bf16 operand planes that persist between entry points; defined with the decoder below */
/* `pl` (may be NULL): also write X as operand planes pl->X_rc (all rows) and pl->X_r8 (rows < pl->Qb), so that
 * the decoder GEMMs of a bf16-matrix-core compute type need no separate conversion pass; X may then be NULL.  */
int dpd_patch_rows_fwd(const float* q, const float* fv, int C, int N, int m, int k, int KP, float* X,
                       float* mask, int32_t* vox, const struct dpd_planes* pl, void* stream);

/* The front end of a training step in TWO launches instead of four (stack, encoder, norm, gather):
 * dpd_mfv3d_fwd_stacked = dpd_stack_clouds + dpd_mfv3d_fwd in one kernel: it reads pcA (+noise) / pcB directly and also
 *   writes pts [2B,N,3] and q [2B,N,3] (either may be NULL).  With ssq != NULL ([2B][DPD_MFV_SLICES][20] floats) fv is
 *   left WITHOUT the final per-channel L2 normalisation (:124-126) and ssq receives the per-slice sums of squares;
 * dpd_patch_rows_fwd_scaled = dpd_patch_rows_fwd that applies that normalisation while it gathers (ssq NULL = plain).
 * Same bits as the four-launch form (both use one summation order for the norms).                                   */
#define DPD_MFV_SLICES 4
int dpd_mfv3d_fwd_stacked(const float* pcA, const float* pcB, const float* noise, int B, int N, int m, float sigma,
                          float* pts, float* q, float* fv, float* ssq, void* stream);
int dpd_patch_rows_fwd_scaled(const float* q, const float* fv, const float* ssq, int C, int N, int m, int k, int KP,
                              float* X, float* mask, int32_t* vox, const struct dpd_planes* pl, void* stream);

/* The same gather over DISTINCT windows (DPD_F32 training step).  The window part of row r = c*N + n depends on (cloud, voxel)
 * only, so it is written once per distinct pair and layer 1 runs over those rows (dpd_decoder_fwd_unique):
 *   uid [Q]          slot of the row's window = that of the first row of its cloud with the same voxel; slots are dense and in row
 *                    order: [0, U_AB) for the rows < Qb, a gap up to U_ABp = roundup(U_AB, 32), then the rows >= Qb up to M_u;
 *   Xu [KP - 32, Q + 32]  K-MAJOR: column `slot` holds columns [0, KP - 32) of the row that owns the slot; gap columns zero; every
 *                    other column untouched (layer 1 reads it as a weight gradient reads its activations: 128 contiguous bytes per k);
 *   Xt [Q, 32]       columns [KP - 32, KP) of every row (the last window values, q - centre, the zero pad);
 *   cnt [4]          {U_AB, M_u, U_ABp, 0} as device words (the host never needs them);
 *   X [x_rows, KP]   optional (x_rows = 0: none): the whole rows r < x_rows as dpd_patch_rows_fwd_scaled writes them (what the
 *                    weight gradient of layer 1 contracts over); mask, vox as there; ssq as there (NULL = fv is normalised).
 * Qb = the rows of the first half (whole clouds).  scratch: dpd_patch_rows_unique_scratch_bytes(C, N) bytes.  Two launches (index,
 * gather).  Needs k >= 3, KP == dpd_padded_width(k), N % 8 == 0, N <= 1024, x_rows % N == 0, m <= 10 (else DPD_E_UNSUPPORTED: use the plain gather). */
size_t dpd_patch_rows_unique_scratch_bytes(int C, int N);
int dpd_patch_rows_fwd_unique(const float* q, const float* fv, const float* ssq, int C, int N, int m, int k, int KP, int Qb,
                              float* X, int x_rows, float* Xu, float* Xt, float* mask, int32_t* vox, int32_t* uid, int32_t* cnt,
                              void* scratch, size_t scratch_bytes, void* stream);

/* Backward of the gather: dX [Q,KP] -> dq [C,N,3] (overwritten; = dX[:,E:E+3]) and
 * dfv [C,m^3,20] (overwritten; scatter-add of the window columns).  Either output may be NULL.  */
int dpd_patch_rows_bwd(const float* dX, const int32_t* vox, int C, int N, int m, int k, int KP, float* dq,
                       float* dfv, void* stream);

/* Tail of the as-loss backward (pcrnet-registration/iterative_PCRNet_ours.py:255-257, train_multi_gpu_pc_compare_dist.py:457-463:
 * gradients w.r.t. input1 / input2 only) in one launch: dpts [2B,N,3] from dpd_mfv3d_bwd (encoder route), dX [2BN,KP] from
 * dpd_decoder_bwd_data (its q - centre columns are the query route), `scale` = the upstream gradient as a DEVICE scalar (NULL = 1):
 *   gA [B,N,3] = scale * (dpts[0:B]  + dq[B:2B])      (pcA is the query cloud of the BA half)
 *   gB [B,N,3] = scale * (dpts[B:2B] + dq[0:B])                                                                         */
int dpd_asloss_combine(const float* dpts, const float* dX, const float* scale, int B, int N, int k, int KP, float* gA, float* gB,
                       void* stream);

/* The WHOLE non-GEMM tail of an as-loss backward -- dpd_patch_rows_bwd (dX -> dfv), dpd_mfv3d_bwd (dfv -> dpts) and dpd_asloss_combine -- in
 * THREE launches instead of six: [window-gather backward || the encoder backward's statistics pass] -> combine -> apply + both input
 * gradients.  Bit for bit the separate calls.  pts [2B,N,3] = the encoder input of the forward, vox [2BN] from the window gather, dX
 * [2BN,KP]; scratch: dfv [2B,m^3,20] floats and mfv_ws (dpd_mfv3d_bwd_workspace_bytes(2B, m)).  DPD_E_UNSUPPORTED for shapes the sliced
 * encoder backward does not take (N < 8, m > 8): make the separate calls then.
 * Replaces TF autodiff of local_z_3d / get_3dmfv_tf (utils/dpdist_util.py:22-141,911-930) inside tf.gradients(loss, inputs)
 * (pcrnet-registration/iterative_PCRNet_ours.py:255-257).                                                                        */
int dpd_asloss_tail(const float* dX, const int32_t* vox, const float* pts, const float* upstream, int B, int N, int m, int k, int KP,
                    float sigma, float* dfv, void* mfv_ws, size_t mfv_ws_bytes, float* gA, float* gB, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Implicit decoder (shared MLP).  Replaces tf_util.conv2d x4 (utils/dpdist_util.py:513-544,
 * utils/tf_util.py:161-228), relu6/3 (:691) and the mask multiply (:695-698).
 *   X [Q,KP] -> h1,h2,h3 [Q,H] (post-ReLU, kept for backward), y [Q,3] (pre-activation),
 *   pred [Q,3] = clip(y,0,6)/3 * mask.   W1p [KP,H], W2,W3 [H,H], W4 [H,3], biases [H],[H],[H],[3].
 *   H must be a multiple of 64.  dtype: 0 = fp32 MFMA (v_mfma_f32_32x32x2_f32, exact fp32).     */
typedef struct dpd_decoder_params {
    const float* W1p; const float* b1;
    const float* W2;  const float* b2;
    const float* W3;  const float* b3;
    const float* W4;  const float* b4;
    /* optional (NULL = absent) transposed copies written by dpd_weights_transpose: W2T, W3T [H,H], W1pT [H,KP].  With them
     * the backward data GEMMs g2 = g3 W3^T, g1 = g2 W2^T, dX = g1 W1p^T read their weight operand row-coalesced (the
     * register-streamed fp32 kernel then runs them at the forward's rate); without them the LDS-ring kernel is used.  */
    const float* W2T; const float* W3T; const float* W1pT;
} dpd_decoder_params;

/* Refresh the transposed weight copies (one launch): W2T, W3T [H,H] and, if W1pT != NULL, W1pT [H,KP].  Call after
 * loading weights and after every optimizer step (training), once for frozen weights (as-loss mode).  DPD_F32 only.  */
int dpd_weights_transpose(const dpd_decoder_params* p, int KP, int H, float* W2T, float* W3T, float* W1pT, void* stream);

/* With planes that keep h1_rc / h2_rc (plane compute types), h1 / h2 may be NULL: the fp32 copies are then not written; pass
 * NULL for them to dpd_decoder_bwd_data / dpd_decoder_bwd_weights[_pair] as well (the ReLU gate is read from the bf16 plane).  In the same
 * way g2 / g1 of dpd_decoder_bwd_data may be NULL when the planes keep g2_rc + g2_r8 / g1_r8 (and sg->partials is given).          */
int dpd_decoder_fwd(const float* X, const float* mask, int Q, int KP, int H, const dpd_decoder_params* p,
                    int dtype, float* h1, float* h2, float* h3, float* y, float* pred, void* ws, size_t ws_bytes,
                    const dpd_planes* pl, void* stream);

/* dpd_decoder_fwd (DPD_F32) on the outputs of dpd_patch_rows_fwd_unique: layer 1 contracts its first KP - 32 columns once per
 * distinct window -- Pu [Q + 32, H] = Xu^T W1p[0 : KP - 32] over the cnt[1] live slots, the row count read on the device -- and one more launch
 * continues each row's accumulators Pu[uid[r]] with the last 32 columns (Xt), adds the bias and applies the ReLU.  The order of
 * every element's fp32 chain is that of dpd_decoder_fwd's layer 1 on the register-streamed kernels (its default), so h1 -- and
 * with it h2, h3, y, pred -- has the same BITS.  Pu is scratch.  Needs Q % 32 == 0, KP % 32 == 0, KP >= 64, H % 64 == 0.      */
int dpd_decoder_fwd_unique(const float* Xu, const float* Xt, const int32_t* uid, const int32_t* cnt, float* Pu, const float* mask,
                           int Q, int KP, int H, const dpd_decoder_params* p, float* h1, float* h2, float* h3, float* y,
                           float* pred, void* stream);

/* ---------------------------------------------------------------------------------------------
 * All-pairs distance matrix (DPD_F32; its backward is the block below): every cloud of a set A [Ca,N,3] against every cloud of a set B [Cb,N,3],
 *   D_AB[i,j] = mean_n pred(surface A_i ; query B_j[n])[0]
 * -- what get_emb_and_concat / get_pc_grid_binary_mask_from_centers (utils/dpdist_util.py:434-511), the decoder (:513-544), relu6/3 and
 * the mask (:690-698) and the mean of loss_pred (:976-979) give for the pair (A_i, B_j) -- without building the Ca Cb pairs: the
 * encoder runs once per cloud, and because the voxel of a query does not depend on the surface cloud, layer 1 contracts its first
 * KP - 32 columns once per (surface cloud, occupied voxel) instead of once per row.  The other direction is the same calls with the
 * sets swapped.  The caller owns all memory; the host never reads a device word.
 *
 * dpd_cross_index: q [Cb,N,3] -> vox [Cb N], mask [Cb N] (the cell rule and the bits of dpd_patch_rows_fwd; a masked query uses
 *   voxel 0's window), slot_of_vox [m^3] (dense slot of every occupied voxel in ascending voxel id, else -1) and ucount [1] = U, the
 *   number of occupied voxels (<= min(m^3, Cb N)).  One launch, integer only, deterministic.  m <= 10.
 * dpd_cross_slot_capacity: the slot capacity of a chunk of Ca_chunk surface clouds, Ca_chunk * min(m^3, Cb N) rounded up to 32
 *   (0 = refused shape): the columns of Xu and the rows of Pu are sized by it.
 * dpd_cross_gather: Ca_chunk surface clouds fv [Ca_chunk, m^3, 20] (ssq as in dpd_patch_rows_fwd_scaled, NULL = fv is normalised)
 *   against those queries; rows are ordered (i, j, n), rows = Ca_chunk Cb N, rows_p = rows rounded up to 32:
 *     Xu [KP - 32, ldu]  K-MAJOR: column i U + s = columns [0, KP - 32) of the window of surface i around the voxel of slot s, the bits
 *                        dpd_patch_rows_fwd_scaled writes for such a row; nothing beyond the Ca_chunk U live columns is written;
 *     Xt [rows_p, 32]    columns [KP - 32, KP) of every row (the window's last values, q - centre, the zero pad);
 *     uid [rows_p]       i U + slot_of_vox[vox(j, n)];   maskr [rows_p] the mask of the row's query;
 *     cnt [4]            {U, Ca_chunk U, 0, 0}: cnt[1] is the live slot count the decoder reads on the device;
 *   pad rows (rows <= r < rows_p) get uid 0, Xt 0, mask 0.  One launch.  Needs k >= 3, KP == dpd_padded_width(k), m <= 10,
 *   ldu >= dpd_cross_slot_capacity(...) (else DPD_E_UNSUPPORTED / DPD_E_DIM).
 * dpd_decoder_fwd_cross: the launches of dpd_decoder_fwd_unique on those buffers with an explicit slot capacity (Pu [slot_cap, H],
 *   ldu = row stride of Xu) -- same bits of y and pred [rows_p, 3] as dpd_decoder_fwd on the plain rows -- with layers 1 to 3
 *   written into two ping-pong activation buffers act0, act1 [rows_p, H], then Dd [pairs] (pairs = Ca_chunk Cb) = the mean of
 *   pred[:, 0] over the N rows of each pair, in one fixed summation order that does not depend on the chunk.  Pad rows never enter Dd.
 *   Needs H % 64 == 0, KP % 32 == 0, slot_cap % 4 == 0, ldu % 4 == 0.
 * dpd_cross_workspace_bytes: the bytes of one chunk's buffers -- Xu (ldu = the slot capacity), Xt, uid, maskr, cnt, Pu, act0, act1, y,
 *   pred, Dd, in this order, each rounded up to 256 bytes; 0 for a shape the entries refuse.
 * dpd_cross_carve: the library owns that layout (and the backward's, dpd_cross_bwd_workspace_bytes below): one caller-owned allocation
 *   `mem` of at least the matching report's bytes -> the chunk's shape, slot capacity, rows_p, total bytes and one pointer per buffer, at
 *   offsets that are multiples of 256 (mem itself need not be aligned).  backward = 0: the forward's buffers, h1..h3 and every gradient
 *   buffer NULL; backward != 0: the backward's, act0, act1 and Dd NULL.  Host-side pointer arithmetic only (no device call, nothing but
 *   `out` is dereferenced).  DPD_E_NULL for a null mem / out, DPD_E_UNSUPPORTED exactly where the matching report returns 0,
 *   DPD_E_WORKSPACE for bytes below the report; on any error every member of *out is zero.
 * Size limit: the GEMMs address their matrices with 32-bit byte offsets, so Xu [KP - 32, ldu], Pu [slot_cap, H] and the activation
 *   buffers [rows_p, H] must each stay below 4 GiB (DPD_E_UNSUPPORTED from the gather and the decoder, 0 from the workspace report):
 *   take fewer surface clouds per chunk.                                                                                          */
int dpd_cross_slot_capacity(int Ca_chunk, int Cb, int N, int m);
size_t dpd_cross_workspace_bytes(int Ca_chunk, int Cb, int N, int m, int k, int KP, int H);
typedef struct dpd_cross_chunk {
    int Ca_chunk, Cb, N, m, k, KP, H;
    int slot_cap, rows_p;       /* dpd_cross_slot_capacity; Ca_chunk Cb N rounded up to 32 */
    size_t bytes;               /* the matching workspace report */
    void *Xu, *Xt, *uid, *maskr, *cnt, *Pu;      /* both forms */
    void *act0, *act1, *Dd;                      /* the forward only */
    void *h1, *h2, *h3;                          /* the backward only, as the buffers below */
    void *y, *pred;                              /* both forms */
    void *dpred, *dy, *ga, *gb, *dq, *gs, *dXs, *dfv;
} dpd_cross_chunk;
int dpd_cross_carve(void* mem, size_t bytes, int Ca_chunk, int Cb, int N, int m, int k, int KP, int H, int backward, dpd_cross_chunk* out);
int dpd_cross_index(const float* q, int Cb, int N, int m, float* mask, int32_t* vox, int32_t* slot_of_vox, int32_t* ucount, void* stream);
int dpd_cross_gather(const float* q, const int32_t* vox, const float* mask, const int32_t* slot_of_vox, const int32_t* ucount,
                     const float* fv, const float* ssq, int Ca_chunk, int Cb, int N, int m, int k, int KP, float* Xu, int ldu, float* Xt,
                     int32_t* uid, float* maskr, int32_t* cnt, void* stream);
int dpd_decoder_fwd_cross(const float* Xu, int ldu, int slot_cap, const float* Xt, const int32_t* uid, const int32_t* cnt, float* Pu,
                          const float* maskr, int pairs, int N, int KP, int H, const dpd_decoder_params* p, float* act0, float* act1,
                          float* y, float* pred, float* Dd, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Backward of the all-pairs matrix (DPD_F32, as-loss mode: the decoder is frozen, gradients go to the two cloud sets).  Per direction
 * and chunk of whole surface clouds, rows ordered (i, j, n) as in the forward; the layer-1 data gradient is linear, so the gradient rows
 * of all queries that share a (surface, occupied voxel) slot are summed first and multiplied by W1p^T once per slot.  Deterministic: no
 * float atomics, one summation order per element, independent of the launch shape.  The caller owns all memory; the host never reads U.
 *
 * dpd_cross_invert: the inverted index of dpd_cross_index's vox / slot_of_vox / ucount, once per direction (one launch, integer only):
 *   slot_start [m^3 + 1]  start of slot s in qlist for s < U, Cb N for U <= s <= m^3;
 *   qlist [Cb N]          the query ids sorted by slot, ascending query id inside a slot (a stable counting sort);
 *   slot_vox [m^3]        the voxel id of slot s for s < U, -1 beyond.
 * dpd_decoder_fwd_cross_keep: dpd_decoder_fwd_cross (same launches, same bits) with layers 1 to 3 kept in three distinct buffers h1, h2,
 *   h3 [rows_p, H] for the backward.  Dd may be NULL (no pair means).
 * dpd_cross_slot_sum: g1 [rows_p, H] streamed once; cnt / slot_cap as written by / given to dpd_cross_gather for this chunk.
 *     gs [slot_cap, H]   row i U + s = the sum of the g1 rows of surface i whose query lies in slot s, added in list order; the DEAD rows
 *                        Ca_chunk U <= t < slot_cap are written as ZEROS (the slot product runs over the capacity);
 *     dq [rows, 3]       dq[r, c] = g1[r, :] . W1p[E + c, :], E = 20 k^3: the q - centre columns of dX; rows >= Ca_chunk Cb N untouched.
 *   gs = NULL or dq = NULL (not both): that half is skipped.  H % 64 == 0, H <= 4096.
 * dpd_cross_scatter: dXs [>= Ca_chunk U, KP] (row i U + s = the dX of that slot) -> dfv [Ca_chunk, m^3, 20]: dfv[i, v, ch] = the sum over
 *   the slots of surface i whose window covers voxel v, in ascending slot order, of that window column; zero padding at the grid border.
 * dpd_cross_bwd: one chunk: Gd [Ca_chunk Cb] (the direction's upstream of D_dir, chunk rows) -> dpred [rows_p, 3] = (Gd / N, 0, 0), 0 on
 *   the pad rows; dpd_decoder_bwd_data (phases 7, no dX; p needs W2T / W3T, and W1pT when dfv is wanted) with g3 -> ga, g2 -> gb, g1 -> ga;
 *   dpd_cross_slot_sum; dXs [slot_cap, KP] = gs W1pT (one NN GEMM over the capacity); dpd_cross_scatter -> dfv (feed it to dpd_mfv3d_bwd
 *   with the chunk's surface clouds); gQ [Cb, N, 3] = gQ + sum_i dq[(i, j, n)] in ascending i (the caller zeroes gQ before the first chunk
 *   of a direction: the chain is continued, so chunk boundaries change no bit).  dfv = NULL: the surface set needs no gradient (slot sum
 *   of gs, slot product and scatter skipped; gs, dXs, slot_vox may be NULL); gQ = NULL: the query set needs none (dq may be NULL).
 * dpd_cross_bwd_workspace_bytes: the bytes of one backward chunk -- Xu, Xt, uid, maskr, cnt, Pu, h1, h2, h3, y, pred (the forward's
 *   buffers with three activations), then dpred, dy [rows_p, 3], ga, gb [rows_p, H], dq [rows_p, 3], gs [slot_cap, H], dXs [slot_cap, KP],
 *   dfv [Ca_chunk, m^3, 20], in this order, each rounded up to 256 bytes (dpd_cross_carve with backward = 1 hands the pointers out); 0 for a
 *   refused shape: one the forward refuses, H > 4096, or dXs beyond the 4 GiB the GEMMs address (DPD_E_UNSUPPORTED from the entries). */
size_t dpd_cross_bwd_workspace_bytes(int Ca_chunk, int Cb, int N, int m, int k, int KP, int H);
int dpd_cross_invert(const int32_t* vox, const int32_t* slot_of_vox, const int32_t* ucount, int Cb, int N, int m, int32_t* slot_start,
                     int32_t* qlist, int32_t* slot_vox, void* stream);
int dpd_decoder_fwd_cross_keep(const float* Xu, int ldu, int slot_cap, const float* Xt, const int32_t* uid, const int32_t* cnt, float* Pu,
                               const float* maskr, int pairs, int N, int KP, int H, const dpd_decoder_params* p, float* h1, float* h2,
                               float* h3, float* y, float* pred, float* Dd, void* stream);
int dpd_cross_slot_sum(const float* g1, const int32_t* cnt, const int32_t* slot_start, const int32_t* qlist, const float* W1p, int Ca_chunk,
                       int Cb, int N, int m, int k, int KP, int H, int slot_cap, float* gs, float* dq, void* stream);
int dpd_cross_scatter(const float* dXs, const int32_t* cnt, const int32_t* slot_vox, int Ca_chunk, int Cb, int N, int m, int k, int KP,
                      float* dfv, void* stream);
int dpd_cross_bwd(const float* Gd, const float* maskr, const float* y, const float* h1, const float* h2, const float* h3, const int32_t* cnt,
                  const int32_t* slot_start, const int32_t* qlist, const int32_t* slot_vox, int Ca_chunk, int Cb, int N, int m, int k, int KP,
                  int H, int slot_cap, const dpd_decoder_params* p, float* dpred, float* dy, float* ga, float* gb, float* dq, float* gs,
                  float* dXs, float* dfv, float* gQ, void* stream);

/* ---------------------------------------------------------------------------------------------
 * RAGGED sets: clouds of different sizes inside a set, for the all-pairs matrix.  A ragged set is a padded tensor pts [C,N,3] plus
 * counts [C] (int32, DEVICE memory): cloud c consists of its first counts[c] points, 1 <= counts[c] <= N; the rest of its row is padding.
 * The five entries below are the per-cloud-count twins of existing entries and run the same device code with a per-cloud bound: the
 * un-counted entries, their kernels and their bits are unchanged.  Rules for all five:
 *   - the host never reads a device word, so an out-of-range count cannot be refused: the KERNELS clamp every count into [1, N], and
 *     an out-of-range count causes no out-of-bounds access;
 *   - counts (qcounts) = NULL is DPD_E_NULL; every other refusal is that of the un-counted twin, happens before anything is launched and
 *     leaves the outputs untouched.
 * dpd_mfv3d_fwd_counts: dpd_mfv3d_fwd_tiled with n = counts[c] per cloud: the point loop runs to n, the mean's 1 / n and sqrt(w) n use
 *   the cloud's count, the row stride is N.  Sizes, tile rules (the tile is cut to N rounded up to 8), the dynamic-LDS formula, the
 *   normalisation and the NaN-on-0/0 behaviour are those of dpd_mfv3d_fwd_tiled.  The padding is never read.  Cloud c gets the bits
 *   dpd_mfv3d_fwd_tiled gives for it alone ([1, n, 3]) at the same tile.
 * dpd_mfv3d_bwd_counts: dpd_mfv3d_bwd_tiled with the 4 point slices taken per cloud (ceil(n / 4) points each, empty slices as there) and
 *   the combine's 1 / n per cloud.  dpts [C,N,3]: rows n >= counts[c] are WRITTEN as +0.0 (no memset needed).  m <= 8; ws is REQUIRED
 *   (dpd_mfv3d_bwd_workspace_bytes(C, m)).  The bits of dpd_mfv3d_bwd_tiled on the cloud alone at the same tile.
 * dpd_cross_index_counts: dpd_cross_index where a padded query (n >= counts[j]) is treated exactly like a query outside the cube: mask 0,
 *   voxel 0, voxel 0 marked occupied; it is not read.  Gather, slot logic, dpd_cross_invert, slot sum and scatter need no twin.
 * dpd_decoder_fwd_cross_counts: dpd_decoder_fwd_cross with Dd[i, j] = (sum over n < qcounts[j] of pred[(i, j, n), 0]) / qcounts[j], in the
 *   lane order and tree of the un-counted mean.  pairs = surface clouds x Cb; Cb < 1 or pairs % Cb != 0 is DPD_E_DIM.
 *   (dpd_decoder_fwd_cross_keep needs no twin: the backward passes Dd = NULL.)
 * dpd_cross_bwd_counts: dpd_cross_bwd with dpred[(i, j, n)] = (Gd[i, j] / qcounts[j], 0, 0) for n < qcounts[j] and 0 otherwise.       */
int dpd_mfv3d_fwd_counts(const float* pts, const int32_t* counts, int C, int N, int m, float sigma, int tile, float* fv, void* stream);
int dpd_mfv3d_bwd_counts(const float* pts, const int32_t* counts, const float* dfv, int C, int N, int m, float sigma, int tile, float* dpts,
                         void* ws, size_t ws_bytes, void* stream);
int dpd_cross_index_counts(const float* q, const int32_t* counts, int Cb, int N, int m, float* mask, int32_t* vox, int32_t* slot_of_vox,
                           int32_t* ucount, void* stream);
int dpd_decoder_fwd_cross_counts(const float* Xu, int ldu, int slot_cap, const float* Xt, const int32_t* uid, const int32_t* cnt, float* Pu,
                                 const float* maskr, const int32_t* qcounts, int pairs, int Cb, int N, int KP, int H,
                                 const dpd_decoder_params* p, float* act0, float* act1, float* y, float* pred, float* Dd, void* stream);
int dpd_cross_bwd_counts(const float* Gd, const float* maskr, const int32_t* qcounts, const float* y, const float* h1, const float* h2,
                         const float* h3, const int32_t* cnt, const int32_t* slot_start, const int32_t* qlist, const int32_t* slot_vox,
                         int Ca_chunk, int Cb, int N, int m, int k, int KP, int H, int slot_cap, const dpd_decoder_params* p, float* dpred,
                         float* dy, float* ga, float* gb, float* dq, float* gs, float* dXs, float* dfv, float* gQ, void* stream);

/* ---------------------------------------------------------------------------------------------
 * PAIRED distances of clouds of different sizes (DPD_F32): pair b of two sets A [P,Wa,3] and B [P,Wb,3], each with optional per-cloud
 * counts (int32, DEVICE memory, as in the RAGGED block; NULL here = the set is full), gives the two halves the reference computes for
 * one pair at that pair's own sizes (models/dpdist_and_aue.py:56-69, utils/dpdist_util.py:494-511, 690-698, 976-977):
 *   D_AB[b] = (1 / nB[b]) sum_{n < nB[b]} pred(surface A_b[:nA[b]] ; query B_b[n])[0]
 *   D_BA[b] = (1 / nA[b]) sum_{n < nA[b]} pred(surface B_b[:nB[b]] ; query A_b[n])[0]
 * -- the diagonal of the all-pairs matrix above, at P instead of P^2 decoder evaluations.  A real query outside the cube adds 0 and
 * still counts in the denominator.  Row layout of a chunk of P pairs, Q = P (Wb + Wa) rows:
 *   AB half   row b Wb + n          query B_b[n], surface A_b       (rows [0, P Wb))
 *   BA half   row P Wb + b Wa + n   query A_b[n], surface B_b       (rows [P Wb, Q))
 * so a rectangular call (Wa != Wb, no counts) wastes no row; raggedness inside a set costs masked rows.  The rules of the RAGGED block
 * hold: the host never reads a device word, the kernels clamp every count into [1, width], padding is never read, every refusal
 * happens before anything is launched and leaves the outputs untouched.  The rest of the chain is existing entries, called as they are:
 * dpd_mfv3d_fwd[_tiled | _counts] per set, dpd_decoder_fwd with y = pred = NULL, dpd_decoder_bwd_data with phases = 6 and the g3 below,
 * dpd_patch_rows_bwd per half (a padded row carries dX = 0 and voxel 0: it adds nothing), dpd_mfv3d_bwd[_tiled | _counts] per set.
 *
 * dpd_patch_rows_fwd_counts: dpd_patch_rows_fwd (fp32 rows, no planes) with a per-cloud query count: query n >= qcounts[c] is not read,
 *   its row of X is written as KP times +0.0, its mask as 0 and its voxel as 0; a real query gets the bits of dpd_patch_rows_fwd.
 *   Called once per half with the OTHER set's Fisher vectors.  qcounts = NULL is DPD_E_NULL; every other refusal is dpd_patch_rows_fwd's.
 * dpd_decoder_out_pairs: the output layer over the Q rows of that layout: h3 [Q,H], mask [Q] -> y, pred [Q,3], the bits of
 *   dpd_decoder_fwd's output layer on those rows, and Dd [2,P] = (D_AB ; D_BA): the sum of pred[:,0] over each pair's real queries in
 *   2^-32 fixed point (an integer sum: exact, the same bits on every run, independent of the other pairs of the launch) divided by the
 *   pair's count.  pred must be finite.  With dy [Q,3] and g3 [Q,H] (both or neither) also the output-layer backward of
 *   sum_b (D_AB[b] + D_BA[b]): dy = ((1 / count) mask / 3 [0 < y0 < 6], 0, 0) with the count of the row's own segment, g3 = dy0
 *   W4[:,0] [h3 > 0]; the rows of padded queries are +0.0 in both.  Two launches (rows; segment sums).  P, Wa, Wb >= 1 and Q <= 2^30,
 *   else DPD_E_DIM (a segment's fixed-point sum then stays below 2^64); h3 and g3 16-byte aligned, else DPD_E_UNSUPPORTED.
 * dpd_pairs_combine: the tail of the backward in one launch.  Everything between the output layer and the inputs is linear in the two
 *   per-pair upstream scalars G_ab, G_ba [P] (device vectors: d loss / d D_AB, d loss / d D_BA, the gradient of D = (D_AB + D_BA) / 2
 *   folded in by the caller), so they are applied once, here: with dptsA [P,Wa,3], dptsB [P,Wb,3] the encoder routes (dpd_mfv3d_bwd*
 *   of the AB half's dfv with A, of the BA half's with B) and dq = the q - centre columns of dX [Q,KP],
 *     gA[b,n] = G_ab[b] dptsA[b,n] + G_ba[b] dq[P Wb + b Wa + n]        (A_b is the query of the BA half)
 *     gB[b,n] = G_ba[b] dptsB[b,n] + G_ab[b] dq[b Wb + n]
 *   and rows n >= the cloud's count are written as +0.0.  gA = NULL or gB = NULL (not both): that set needs no gradient and its dpts
 *   may be NULL.  KP >= 20 k^3 + 3, k odd, 1 <= k <= 7.                                                                              */
int dpd_patch_rows_fwd_counts(const float* q, const int32_t* qcounts, const float* fv, int C, int N, int m, int k, int KP, float* X,
                              float* mask, int32_t* vox, void* stream);
int dpd_decoder_out_pairs(const float* h3, const float* mask, int P, int Wa, int Wb, const int32_t* countsA, const int32_t* countsB, int H,
                          const dpd_decoder_params* p, float* y, float* pred, float* Dd, float* dy, float* g3, void* stream);
int dpd_pairs_combine(const float* dptsA, const float* dptsB, const float* dX, const float* G_ab, const float* G_ba, int P, int Wa, int Wb,
                      const int32_t* countsA, const int32_t* countsB, int k, int KP, float* gA, float* gB, void* stream);

/* ---------------------------------------------------------------------------------------------
 * PER-POINT FIELD (DPD_F32): the decoder's answer at queries of the caller's choosing, not averaged.  A chunk is n surface clouds
 * fv [n, m^3, 20] (normalised Fisher vectors) times T consecutive queries of each; cloud c's queries start at q + c * q_cloud_stride floats
 * (3 M for clouds with M queries of their own, 0 for one query set shared by all clouds; q points at query t0 of the chunk's first
 * cloud).  Rows are ordered (c, t), rows = n T, rows_p = rows rounded up to 32.  A window depends on (cloud, voxel) only, so layer 1
 * contracts its first KP - 32 columns once per occupied (cloud, voxel) -- at most min(m^3, T) per cloud -- instead of once per row.  The
 * caller owns all memory; the host never reads a device word; every chunk has its own index, slots and slot product.
 *
 * dpd_field_slot_capacity: n * min(m^3, T) rounded up to 32: the columns of Xu and the rows of Pu are sized by it.  0 = refused
 *   (n, T < 1, m outside 1..10, n T > 2^30).
 * dpd_field_index: one workgroup per cloud -> vox [n T], mask [n T] (the cell rule and the bits of dpd_patch_rows_fwd; a masked query
 *   uses voxel 0's window), slot_of_vox [n, m^3] (the dense slot INSIDE cloud c of every voxel its queries occupy, in ascending voxel id,
 *   else -1) and ucount [n] = U_c.  One launch, integer only, deterministic.  qcounts [n] (int32, DEVICE memory; may be NULL = every query
 *   is real): row (c, t) is padding when t0 + t >= max(qcounts[c], 1); a padded query is not read by the index and is a masked query of
 *   voxel 0, as in dpd_cross_index_counts.
 * dpd_field_gather: the windows and the rows' tails of the chunk, one launch:
 *     Xu [KP - 32, ldu]  K-MAJOR: column base_c + s = columns [0, KP - 32) of the window of surface c around the voxel of its slot s, the
 *                        bits dpd_patch_rows_fwd writes for such a row; base_c = sum of U_c' over c' < c (cloud-major, ascending voxel id
 *                        inside a cloud); nothing beyond the sum U_c live columns is written;
 *     Xt [rows_p, 32]    columns [KP - 32, KP) of every row (the window's last values, q - centre, the zero pad); the q - centre of a
 *                        padded query is formed from the padding, which must be finite;
 *     uid [rows_p]       base_c + slot_of_vox[c][vox(c, t)];   maskr [rows_p] the mask of the row's query;
 *     cnt [4]            {n, sum U_c, 0, 0}: cnt[1] is the live slot count the decoder reads on the device;
 *   pad rows (rows <= r < rows_p) get uid 0, Xt 0, mask 0.  Needs k odd in 3..7, KP == dpd_padded_width(k), m <= 10, n T <= 2^30, and
 *   Xu [KP - 32, ldu] below the 4 GiB the GEMMs address (else DPD_E_UNSUPPORTED); ldu >= dpd_field_slot_capacity(n, T, m) (else DPD_E_DIM).
 * dpd_decoder_fwd_field: the launches of dpd_decoder_fwd_cross on those buffers (Pu [slot_cap, H], two ping-pong activation buffers
 *   act0 != act1 [rows_p, H]) without the pair means: y and pred [rows_p, 3] have the bits of dpd_decoder_fwd on the plain rows.  Needs
 *   H % 64 == 0, KP % 32 == 0, slot_cap % 4 == 0, ldu % 4 == 0, rows <= 2^30 and Xu, Pu and the activations below 4 GiB each.
 * The backward over the rows is existing entries: dpd_decoder_fwd_cross_keep(pairs = n, N = T, Dd = NULL), dpd_decoder_bwd_data with dX,
 * dpd_patch_rows_bwd(dX, vox, n, T) -> dq [n, T, 3] and dfv, dpd_mfv3d_bwd*; the slot-summed backward is the next block.
 * NULL argument: DPD_E_NULL; n, T < 1, t0 < 0, a negative stride: DPD_E_DIM; a refused shape: DPD_E_UNSUPPORTED; all before any launch. */
int dpd_field_slot_capacity(int n, int T, int m);
int dpd_field_index(const float* q, long q_cloud_stride, const int32_t* qcounts, int t0, int n, int T, int m, float* mask, int32_t* vox,
                    int32_t* slot_of_vox, int32_t* ucount, void* stream);
int dpd_field_gather(const float* q, long q_cloud_stride, const int32_t* vox, const float* mask, const int32_t* slot_of_vox,
                     const int32_t* ucount, const float* fv, int n, int T, int m, int k, int KP, float* Xu, int ldu, float* Xt, int32_t* uid,
                     float* maskr, int32_t* cnt, void* stream);
int dpd_decoder_fwd_field(const float* Xu, int ldu, int slot_cap, const float* Xt, const int32_t* uid, const int32_t* cnt, float* Pu,
                          const float* maskr, int rows, int KP, int H, const dpd_decoder_params* p, float* act0, float* act1, float* y,
                          float* pred, void* stream);

/* ---------------------------------------------------------------------------------------------
 * SLOT-SUMMED BACKWARD of the per-point field (DPD_F32, as-loss mode: the decoder is frozen, gradients go to the surfaces and the
 * queries).  Per chunk of the forward's plan -- n clouds times T consecutive queries of each, which may be a TILE of one cloud's
 * queries --, on the chunk's own index (dpd_field_index), slots (dpd_field_gather: ucount, cnt) and kept activations
 * (dpd_decoder_fwd_cross_keep with pairs = n, N = T, Dd = NULL).  The layer-1 data gradient is linear, so the g1 rows of all queries of a
 * cloud that share a slot are summed first and multiplied by W1p^T once per slot: no [rows_p, KP] matrix exists and T has no limit of
 * its own.  Slots are the forward's: cloud-major, global slot g = base_c + s, base_c = the sum of U_c' over c' < c, total = the sum of
 * the U_c = cnt[1]; slot_cap = dpd_field_slot_capacity(n, T, m).  Deterministic: no float atomics, one summation order per element,
 * independent of the launch shape.  The caller owns all memory; the host never reads a device word, and the kernels clamp every word
 * they read (counts into [0, min(m^3, T)], clouds into [0, n), list bounds into the cloud's rows, query ids into [0, T)), so no store
 * passes the capacity the host sized.
 *
 * dpd_field_invert: the inverted index of one chunk, one workgroup per cloud (one launch, integer only):
 *     qlist [n, T]               row c: the chunk-local query ids of cloud c sorted by slot, ascending query id inside a slot (a stable
 *                                counting sort);
 *     slot_start [slot_cap + 1]  slot g holds the flat positions [slot_start[g], slot_start[g + 1]) of qlist, i.e. c T + the cloud's own
 *                                prefix; n T for total <= g <= slot_cap;
 *     slot_vox [slot_cap]        the voxel id of slot g;   slot_cloud [slot_cap]  its cloud;   both -1 for the dead slots g >= total.
 * dpd_field_slot_sum: g1 [rows_p, H] streamed once, one workgroup per slot up to the capacity:
 *     gs [slot_cap, H]           row g = the sum of the g1 rows (c, t) of the slot's list, added in list order; the DEAD rows are ZEROS;
 *     dq                         dq[c dq_cloud_stride + 3 t + j] = g1[(c, t), :] . W1p[E + j, :], E = 20 k^3, j = 0..2, for every row of the
 *                                chunk (a masked or padded query lies in voxel 0's slot: its g1 row is 0 through the mask, its dq is 0);
 *                                dq_cloud_stride >= 3 T floats (else DPD_E_DIM): 3 T for a buffer [n, T, 3], 3 M to write the rows of a
 *                                gradient tensor [C, M, 3] in place;
 *   in the form and fixed reduction tree of dpd_cross_slot_sum (the same device routine).  gs = NULL or dq = NULL (not both): that half
 *   is skipped.  H % 64 == 0, H <= 4096.
 * dpd_field_scatter: dXs [slot_cap, KP] (row g = the dX of slot g) -> dfv [n, m^3, 20]: dfv[c, v, ch] = the sum over the cloud's OWN slots
 *   [base_c, base_c + U_c) whose window covers voxel v, in ascending slot order, of that window column; zero padding at the grid border.
 *   accumulate != 0: the chain continues from the value dfv holds (the tiles of one cloud add up in ascending tile order without a
 *   second buffer); accumulate == 0: a plain store, +0.0 for a voxel no slot covers.
 * dpd_field_bwd: one chunk in one call.  dpred [rows_p, 3] is the upstream gradient of pred, FILLED BY THE CALLER with zero pad rows.
 *   dpd_decoder_bwd_data (phases 7, no dX; p needs W2T / W3T, and W1pT when dfv is wanted) with g3 -> ga, g2 -> gb, g1 -> ga;
 *   dpd_field_slot_sum; dXs = gs W1pT (one NN GEMM over the capacity); dpd_field_scatter -> dfv with `accumulate` (feed it to dpd_mfv3d_bwd*
 *   with the chunk's surface clouds after the cloud's last tile); the query route -> gq, which points at query t0 of the chunk's first
 *   cloud as q does in the forward: gq_cloud_stride = 3 M (>= 3 T, else DPD_E_DIM): cloud c's rows are written in place at
 *   gq + c gq_cloud_stride (dq may be NULL); gq_cloud_stride = 0, one shared set: gq[t] = gq[t] + dq[(0, t)] + dq[(1, t)] + ... in ascending
 *   cloud through dq [n, T, 3], continued from the accumulated value (the caller zeroes gq before the first chunk: chunk and tile
 *   boundaries change no bit).  dfv = NULL: the surfaces need no gradient (gs half, slot product and scatter skipped; ucount, slot_vox,
 *   gs, dXs may be NULL); gq = NULL: the queries need none (dq half skipped).  Both NULL: DPD_E_NULL.
 * One predicate for all four: the forward's (dpd_field_gather's shapes), H % 64 == 0 and H <= 4096, and g1 [rows_p, H], gs [slot_cap, H]
 * and dXs [slot_cap, KP] below the 4 GiB the GEMMs address.  NULL argument: DPD_E_NULL; n, T, k, H < 1, slot_cap !=
 * dpd_field_slot_capacity(n, T, m), a stride below 3 T: DPD_E_DIM; a refused shape: DPD_E_UNSUPPORTED; all before any launch.          */
int dpd_field_invert(const int32_t* vox, const int32_t* slot_of_vox, const int32_t* ucount, int n, int T, int m, int slot_cap,
                     int32_t* slot_start, int32_t* qlist, int32_t* slot_vox, int32_t* slot_cloud, void* stream);
int dpd_field_slot_sum(const float* g1, const int32_t* cnt, const int32_t* slot_start, const int32_t* qlist, const int32_t* slot_cloud,
                       const float* W1p, int n, int T, int m, int k, int KP, int H, int slot_cap, float* gs, float* dq, long dq_cloud_stride,
                       void* stream);
int dpd_field_scatter(const float* dXs, const int32_t* ucount, const int32_t* slot_vox, int n, int T, int m, int k, int KP, int accumulate,
                      float* dfv, void* stream);
int dpd_field_bwd(const float* dpred, const float* maskr, const float* y, const float* h1, const float* h2, const float* h3,
                  const int32_t* cnt, const int32_t* ucount, const int32_t* slot_start, const int32_t* qlist, const int32_t* slot_vox,
                  const int32_t* slot_cloud, int n, int T, int m, int k, int KP, int H, int slot_cap, const dpd_decoder_params* p, float* dy,
                  float* ga, float* gb, float* dq, float* gs, float* dXs, float* dfv, int accumulate, float* gq, long gq_cloud_stride,
                  void* stream);

/* ---------------------------------------------------------------------------------------------
 * DECODER GRADIENTS of the per-point field (DPD_F32): dpd_field_bwd with the gradients of the decoder's eight variables, per chunk of the
 * field's plan.  Arguments as dpd_field_bwd, plus the chunk's Xu [KP - 32, ldu] and Xt [rows_p, 32] of dpd_field_gather and eight outputs
 * in the layout of the flat parameter buffer: dW1p [KP, H], db1 [H], dW2 [H, H], db2 [H], dW3 [H, H], db3 [H], dW4 [H, 3], db4 [3]
 * (all eight, or all NULL = no weight gradient wanted: the call is then dpd_field_bwd).
 *   dW1p[0 : KP - 32]  = Xu gs        ONCE PER SLOT: the window part of a row is column uid[r] of Xu, so the sum over the rows of
 *                                     x_r (x) g1_r is Xu times the slot sums gs [slot_cap, H] that dpd_field_slot_sum forms;
 *   dW1p[KP - 32 : KP] = Xt^T g1      over the rows ([32, H]; the rows E + 3 .. KP - 1, the zero pad of Xt, are exact +0.0);
 *   db1 = colsum(g1);  dW2 = h1^T g2, db2 = colsum(g2);  dW3 = h2^T g3, db3 = colsum(g3);  dW4 = h3^T dy, db4 = colsum(dy).
 * The decoder chain runs by phases (1, dW3 / dW4; 2, dW2; 4, the layer-1 parts), because g1 overwrites g3 in ga; g3, g2, g1 and with them
 * dfv and gq have the bits of dpd_field_bwd (the same launches), with and without the weight outputs.  dfv = gq = NULL with the weight
 * outputs: the slot product, the scatter and the query route are skipped, gs is still formed (gs must then be given).
 * Xu is NOT const: nothing beyond the cnt[1] live columns is written by the gather and 0 * NaN is NaN, so the entry ZEROES the columns
 * cnt[1] .. slot_cap - 1 of Xu before the product; the result does not depend on what they held.
 * accumulate_w != 0: the chunk's gradients are ADDED onto what the eight outputs hold (chunks and tiles add up in ascending plan
 * order); == 0: stored.  The chunk's own contribution is formed completely first, in the workspace, so its bits do not depend on what
 * the outputs held.  Deterministic: no float atomics, one summation order per element (two-step column sums over fixed row chunks).
 * ws: dpd_field_bwd_train_workspace_bytes(n, T, m, k, KP, H) bytes (0 = refused shape), 256-byte aligned.
 * NULL argument: DPD_E_NULL; the dims of dpd_field_bwd, ldu < slot_cap: DPD_E_DIM; the predicate of dpd_field_bwd, ldu % 4, or
 * Xu [KP - 32, ldu] beyond the 4 GiB the GEMMs address: DPD_E_UNSUPPORTED; a small workspace: DPD_E_WORKSPACE; all before any launch. */
size_t dpd_field_bwd_train_workspace_bytes(int n, int T, int m, int k, int KP, int H);
int dpd_field_bwd_train(const float* dpred, const float* maskr, const float* y, const float* h1, const float* h2, const float* h3,
                        const int32_t* cnt, const int32_t* ucount, const int32_t* slot_start, const int32_t* qlist, const int32_t* slot_vox,
                        const int32_t* slot_cloud, float* Xu, int ldu, const float* Xt, int n, int T, int m, int k, int KP, int H,
                        int slot_cap, const dpd_decoder_params* p, float* dy, float* ga, float* gb, float* dq, float* gs, float* dXs,
                        float* dfv, int accumulate, float* gq, long gq_cloud_stride, float* dW1p, float* db1, float* dW2, float* db2,
                        float* dW3, float* db3, float* dW4, float* db4, int accumulate_w, void* ws, size_t ws_bytes, void* stream);

/* `dtype` of the decoder entry points = compute type of the three wide layers (inputs/outputs are always fp32):
 *   DPD_F32     exact fp32 on the fp32 matrix-core instruction (bitwise an fmaf chain), no workspace needed in
 *               dpd_decoder_fwd / dpd_decoder_bwd_data (ws may be NULL);
 *   DPD_F32_X3  fp32-equivalent on the bf16 matrix cores: every operand is split into three bf16 planes
 *               (hi+mid+lo, exact to 2^-27) and each product is the sum of the six bf16 MFMA terms of weight
 *               >= 2^-16, accumulated in fp32 (error vs fp64 <= the DPD_F32 path's, tests/test_gpu_parity.py);
 *   DPD_BF16    operands rounded to bf16, fp32 accumulation (mixed-precision training, tolerance ~1e-2 relative).
 * DPD_F32_X3 / DPD_BF16 need ws = dpd_workspace_bytes(Q, KP, H, dtype) bytes (operand planes).  Shapes the plane
 * kernels do not take (contraction length not a multiple of 32, dims not multiples of 8) run as DPD_F32.       */
enum dpd_dtype { DPD_F32 = 0, DPD_F32_X3 = 1, DPD_BF16 = 2 };

/* Operand planes that persist between entry points (caller-owned memory; see dpd_planes_bytes / dpd_planes_carve).
 * Layouts as in dpd_split_planes: RC = [np][rows][cols] bf16, R8 = [np][rows/8][cols][8].  A NULL member means
 * "not kept": its producer skips it and its consumers convert from the fp32 tensor into `ws` instead.  A non-NULL
 * member handed to a CONSUMER must hold what its producer wrote for the current tensors:
 *   producer                         members
 *   dpd_patch_rows_fwd               X_rc [Q,KP], X_r8 (rows < Qb)
 *   dpd_decoder_fwd                  h1_rc, h2_rc [Q,H]; h1_r8, h2_r8 (rows < Qb)          consumes X_rc, W*_r8
 *   dpd_decoder_bwd_data             g3_rc, g3_r8, g2_rc, g2_r8, g1_rc, g1_r8 [Qb,H]       consumes W*_rc
 *   dpd_weights_to_planes            W1_r8, W2_r8, W3_r8 (forward), W1_rc, W2_rc, W3_rc (backward dH / dX)
 *   dpd_decoder_bwd_weights[_pair]   -                                                     consumes X_r8/h*_r8, g*_r8
 * Planes are only used when Q % 8 == 0, Qb % 32 == 0, KP % 32 == 0 (otherwise `pl` is ignored).              */
struct dpd_planes {
    int np;       /* 3 for DPD_F32_X3, 1 for DPD_BF16 */
    int Q, Qb;    /* rows of X/h1/h2 planes; rows that carry gradient (R8 planes of X/h*, all g planes) */
    void *X_rc, *X_r8, *h1_rc, *h1_r8, *h2_rc, *h2_r8;
    void *g3_rc, *g3_r8, *g2_rc, *g2_r8, *g1_rc, *g1_r8;
    void *W1_r8, *W2_r8, *W3_r8, *W1_rc, *W2_rc, *W3_rc;
    void* h3_rc;  /* DPD_BF16 only (NULL otherwise): layer 3's activation as ONE bf16 plane [Q,H] instead of fp32 -- dpd_decoder_fwd writes it when
                   * h3 == NULL and y == NULL, the fused output-layer kernel of dpd_decoder_bwd_data (which then runs the output layer's forward
                   * as well: dpd_small_grads.fwd_y) reads it; 2 instead of 4 bytes per element written once and read once per step */
};

/* Bytes for ALL members (with_dx: also g1_rc and W1_rc, needed only when dX is requested), and the carve-up of one
 * caller buffer of that size into the members (host-side pointer arithmetic only).                          */
size_t dpd_planes_bytes(int Q, int Qb, int KP, int H, int dtype, int with_dx);
int dpd_planes_carve(void* mem, size_t bytes, int Q, int Qb, int KP, int H, int dtype, int with_dx, dpd_planes* out);
/* Weight planes from the fp32 variables (one launch): call after loading weights and after every optimizer step. */
int dpd_weights_to_planes(const dpd_decoder_params* p, int KP, int H, const dpd_planes* pl, void* stream);

/* Backward, data chain: dpred [Qb,3] for the FIRST Qb rows (training mode: Qb = Q/2, only the AB half
 * carries gradient, train_multi_gpu_pc_compare_dist.py:274-277; as-loss mode: Qb = Q).
 * Produces the pre-activation gradients g3,g2,g1 [Qb,H] and dy [Qb,3]; if dX != NULL also
 * dX [Qb,KP] = g1 * W1p^T (as-loss mode, TF autodiff through :516).
 * `sg` (may be NULL) lists the small gradients that fall out of this chain for free and are then written here
 * (overwritten): db3/db2/db1 [H] = column sums of g3/g2/g1 (fused into the dH GEMM epilogues, fp32 atomics),
 * dW4 [H,3] = h3^T dy, db4 [3].  Any member may be NULL.
 * `phases` selects the parts of the chain to run, so that a data-parallel caller can interleave the weight-gradient
 * GEMMs (and start their all-reduce) between them: 1 = output layer (dy, g3, db3, dW4, db4; clears db1/db2),
 * 2 = g2 (+db2), 4 = g1 (+db1) and dX; 7 = everything.  The same buffers must be passed to every call.
 * 16 (with 1): leave db3 / dW4 / db4 as per-block partial sums in sg->partials; 8: reduce those partials (a call with
 * phases = 8 alone may run on another stream, beside the dH GEMMs, once the phase-1 call has been ordered before it).  */
typedef struct dpd_small_grads {
    float* db1; float* db2; float* db3; float* dW4; float* db4;
    float* partials;   /* optional scratch, ((Qb + 7) / 8) * (4 * H + 8) floats: required by phases 16 / 8 (see below) */
    /* optional fused training loss (utils/dpdist_util.py:962-980 + its autodiff, the mode-1 call of dpd_l1_loss): with
     * l1_labels [Qb] != NULL the output-layer backward derives d loss_samples / d pred_AB * l1_gscale from l1_pred [2*Qb,3]
     * itself (`dpred` may be NULL) and l1_loss [2] = (loss_samples, loss_pred) comes out of the same reduction as db3/dW4/db4.
     * Needs H % 256 == 0, H <= 1024 (else DPD_E_UNSUPPORTED: use dpd_l1_loss).                                              */
    const float* l1_pred; const float* l1_labels; float* l1_loss; float l1_gscale;
    /* optional scratch, 2 * ((Qb + 31) / 32) * H floats (DPD_F32): instead of atomic column sums into db2 / db1 (order-dependent
     * round-off), the dH GEMMs store 32-row partial sums of g2 / g1 here and dpd_decoder_bwd_weights(layer 2 / 1, db, ...,
     * db_partials = this pointer) or dpd_decoder_bwd_weights_pair(..., dbA, db_partials) finishes them: bitwise reproducible.
     * db1 / db2 above are then ignored.                                                                                       */
    float* db_partials;
    /* optional (both or neither; needs the fused loss above): the FORWARD of the output layer inside the same pass -- y and pred
     * [2*Qb,3] of the AB rows and their BA twins are computed from h3 (bit-identical to dpd_decoder_fwd's), written here and
     * used instead of the `y` / l1_pred inputs, which may then be NULL.  Call dpd_decoder_fwd with y = pred = NULL before.    */
    float* fwd_y; float* fwd_pred;
} dpd_small_grads;

int dpd_decoder_bwd_data(const float* dpred, const float* mask, const float* y, const float* h1, const float* h2,
                         const float* h3, int Qb, int KP, int H, const dpd_decoder_params* p, int dtype,
                         float* dy, float* g3, float* g2, float* g1, float* dX, const dpd_small_grads* sg,
                         void* ws, size_t ws_bytes, const dpd_planes* pl, int phases, void* stream);

/* Backward, weight gradients of ONE layer (1..4) from the buffers above:
 *   layer 1: dW [KP,H] = X^T g1, db = colsum(g1);  2: h1^T g2;  3: h2^T g3;  4: dW [H,3] = h3^T dy.
 * `act` is the layer's input activation (X, h1, h2 or h3) with leading dimension lda, `g` its
 * pre-activation output gradient.  dW/db are overwritten; db may be NULL for layers 1-3 when it was already
 * produced by dpd_decoder_bwd_data.  ws: dpd_workspace_bytes() bytes.                              */
int dpd_decoder_bwd_weights(int layer, const float* act, int lda, const float* g, int Qb, int Kin, int Nout,
                            int dtype, float* dW, float* db, void* ws, size_t ws_bytes, const dpd_planes* pl,
                            const float* db_partials, void* stream);

/* dW of two layers of identical shape (layers 2 and 3: dW = act^T g, [Kin,Nout]) in ONE grouped launch; no bias
 * gradients unless dbA / dbB are given (see below).  Qb must be a multiple of 32.                          */
int dpd_decoder_bwd_weights_pair(const float* actA, const float* gA, float* dWA, const float* actB, const float* gB,
                                 float* dWB, int lda, int Qb, int Kin, int Nout, int dtype, void* ws, size_t ws_bytes,
                                 const dpd_planes* pl, float* dbA, const float* db_partials, void* stream);
/* dbA + db_partials (may be NULL; DPD_F32 only): layer 2's bias gradient colsum(gA) [Nout], finished from the partial sums
 * dpd_decoder_bwd_data stored in dpd_small_grads::db_partials (see there).  db_partials == NULL with db != NULL in
 * dpd_decoder_bwd_weights keeps the older two-kernel column sum.                                                         */

/* Live rows (DPD_F32 only): the backward GEMMs over the rows that carry gradient.
 * A row r with dy[r] == (0, 0, 0) -- the relu6 clamp or the mask of the output layer zeroed it -- has zero rows in g3, g2, g1 and
 * adds exact zeros to dW1..dW3, db1, db2.  With a descriptor the `_live` twins of the three entries above leave those rows out:
 *   dpd_decoder_bwd_data_live     behind the output layer (phase 1) ONE launch builds the index of the live rows -- L of them,
 *       Lp = L rounded up to 32, both device words: the host never reads a count -- and compact copies g3c / h1c / h2c / Xc of
 *       their rows (positions L .. Lp: zero rows); the dH products (phases 2 / 4) run over the Lp rows only and write g2 / g1 as
 *       COMPACT rows (g3 and dy stay dense; rows of g2 / g1 from Lp on keep what they held); one more launch rebuilds the 32-row
 *       partial sums of sg->db_partials from them (in the dense association).  Needs p->W2T / p->W3T, fp32 operands, no dX, no
 *       phase 8, and db1 / db2 either through sg->db_partials or not at all.
 *   dpd_decoder_bwd_weights_live  layers 1-3: dW = (compact activation)^T (compact g) with the contraction length Lp read from the
 *       device word; `act` is not read (the descriptor's copy is), `g` = the compact g1 / g2 (layer 3: not read, g3c is);
 *       db only with db_partials (layers 1, 2).  Lp = 0 writes zero gradients.
 *   dpd_decoder_bwd_weights_pair_live  (layer 2, layer 3) likewise; actA / actB / gB are not read.
 * live == NULL: exactly the entry without the suffix.
 * VALUES: every gradient compares == to the dense entries' (the sign of a zero may differ): a dW element is one fused-multiply-add
 * chain over the rows in the kernel's visit order and the compact positions keep the live rows in that order; rows whose layer-1
 * input is not finite (a cloud the encoder turned to NaN) count as live, so that the dense NaN * 0 = NaN stays.  With non-finite
 * WEIGHTS the two forms may differ (0 * inf).
 * The caller owns the memory: dpd_live_rows_carve cuts one buffer of dpd_live_rows_bytes (256-byte aligned) into the members and
 * sets Qb / KP / H; the caller then sets X / ldx (the layer-1 input rows [Qb,KP], row stride ldx) and EITHER ssq / clouds /
 * rows_per_cloud (the sums dpd_mfv3d_fwd_stacked left, [clouds][DPD_MFV_SLICES][20]: row r gathers from cloud r / rows_per_cloud and
 * its query point belongs to cloud r / rows_per_cloud + clouds / 2; Qb = clouds / 2 * rows_per_cloud; a cloud with a non-finite sum
 * makes the rows of both live) OR ssq = NULL: one extra launch then looks for non-finite values in the rows of X themselves.
 * Qb % 32 == 0, Qb <= 65536, H % 4 == 0, KP % 4 == 0.                                                                          */
typedef struct dpd_live_rows {
    int Qb, KP, H;
    int32_t* cnt;          /* {L, Lp, 0, 0}: device words, every reader clamps them to Qb */
    int32_t* idx;          /* [Qb] original row of each compact position (pad positions: a valid row) */
    int32_t* pos;          /* [Qb] compact position of each row, -1 = not live */
    int32_t* rowflag;      /* [Qb] scratch of the ssq == NULL form */
    float* g3c; float* h1c; float* h2c;   /* [Qb,H] */
    float* Xc;             /* [Qb,KP] */
    const float* X; int ldx;
    const float* ssq; int clouds; int rows_per_cloud;
} dpd_live_rows;
size_t dpd_live_rows_bytes(int Qb, int KP, int H);
int dpd_live_rows_carve(void* mem, size_t bytes, int Qb, int KP, int H, dpd_live_rows* out);
int dpd_decoder_bwd_data_live(const float* dpred, const float* mask, const float* y, const float* h1, const float* h2,
                              const float* h3, int Qb, int KP, int H, const dpd_decoder_params* p, int dtype,
                              float* dy, float* g3, float* g2, float* g1, float* dX, const dpd_small_grads* sg,
                              void* ws, size_t ws_bytes, const dpd_planes* pl, int phases, const dpd_live_rows* live, void* stream);
int dpd_decoder_bwd_weights_live(int layer, const float* act, int lda, const float* g, int Qb, int Kin, int Nout,
                                 int dtype, float* dW, float* db, void* ws, size_t ws_bytes, const dpd_planes* pl,
                                 const float* db_partials, const dpd_live_rows* live, void* stream);
int dpd_decoder_bwd_weights_pair_live(const float* actA, const float* gA, float* dWA, const float* actB, const float* gB,
                                      float* dWB, int lda, int Qb, int Kin, int Nout, int dtype, void* ws, size_t ws_bytes,
                                      const dpd_planes* pl, float* dbA, const float* db_partials, const dpd_live_rows* live,
                                      void* stream);
/* A live dH product and the weight gradient that does not need its result, in ONE launch (dpd_gemm_f32_pair), behind the compaction:
 *   layer 3:  g_out (compact g2) = (g3c W3T) * [h2c > 0]   beside   dW (dW3) = h2c^T g3c;   g_in is not read
 *   layer 2:  g_out (compact g1) = (g_in W2T) * [h1c > 0]  beside   dW (dW2) = h1c^T g_in;  g_in = the compact g2
 * Same bits as phase 2 / 4 of dpd_decoder_bwd_data_live and dpd_decoder_bwd_weights_live(layer) without a bias gradient.  Tiles:
 * dpd_set_gemm_plan ops 9 (dH part) and 12 (dW part).                                                                             */
int dpd_decoder_bwd_pair_live(int layer, const float* g_in, float* g_out, float* dW, int Qb, int H, const dpd_decoder_params* p,
                              const dpd_live_rows* live, void* stream);
/* The whole exact-fp32 backward of a single-GPU step on the live rows, in the order that keeps every SIMD busy:
 *   1. output layer (+ loss, + small-gradient reduction) and the compaction: phase 1 of dpd_decoder_bwd_data_live, unchanged
 *   2. { dH -> g2 | dW3 }   3. { dH -> g1 | dW2 }     one launch each (dpd_decoder_bwd_pair_live)
 *   4. the 32-row partial sums of db2 / db1, one launch (sg->db_partials given)
 *   5. dW1; its first-row-block waves finish db1 AND db2 (the partials of db2 exist only behind step 4; same block-order sums)
 * One launch less than data (phases 7) + weights(1) + weights_pair, and every gradient -- g2, g1 (compact rows), dW1..dW3, db1, db2 and
 * what phase 1 writes -- has the bits of that sequence.  Arguments as in dpd_decoder_bwd_data_live (dtype DPD_F32, no dX, no planes);
 * `defer_small` != 0 = its phase 16.  sg->db1 / sg->db2 must be NULL (phase 1 would zero them); db1 / db2 here need sg->db_partials. */
int dpd_decoder_bwd_chain_live(const float* dpred, const float* mask, const float* y, const float* h1, const float* h2,
                               const float* h3, int Qb, int KP, int H, const dpd_decoder_params* p, float* dy, float* g3, float* g2,
                               float* g1, const dpd_small_grads* sg, void* ws, size_t ws_bytes, int defer_small, float* dW1,
                               float* dW2, float* dW3, float* db1, float* db2, const dpd_live_rows* live, void* stream);

/* Scratch needed by the decoder entry points for the given sizes and compute type (split-K slabs, column-sum
 * partials and, for dtype != DPD_F32, the bf16 operand planes of one GEMM at a time).                   */
size_t dpd_workspace_bytes(int Q, int KP, int H, int dtype);

/* ---------------------------------------------------------------------------------------------
 * Losses.  Replaces utils/dpdist_util.py:962-980.  pred [2*BN,3] (AB rows first), labels [BN].
 *   loss[0] = loss_samples = mean |pred_AB[:,0] - labels|        (:972)
 *   loss[1] = loss_pred    = (mean pred_AB[:,0] + mean pred_BA[:,0]) / 2      (:976-977)
 * mode 0: no gradient.  mode 1 (training): dpred [BN,3] = d loss_samples / d pred_AB * gscale.
 * mode 2 (as-loss): dpred [2*BN,3] = d loss_pred / d pred * gscale.                              */
int dpd_l1_loss(const float* pred, const float* labels, int BN, int mode, float gscale, float* loss,
                float* dpred, void* stream);

/* DPDist as a frozen loss (pcrnet-registration/iterative_PCRNet_ours.py:229-257; AUE splice train_multi_gpu_pc_compare_dist.py:417-431):
 * the output layer of the decoder (utils/dpdist_util.py:691,695-698), loss_pred (:976-977) and -- when dy / g3 are given -- the
 * output-layer backward for d loss_pred / d pred in ONE launch: replaces the tail of dpd_decoder_fwd (call it with y = pred = NULL),
 * dpd_l1_loss(mode 2) and phase 1 of dpd_decoder_bwd_data (call it with phases = 6 and this g3).
 *   h3 [Q,H], mask [Q], Q = 2*BN rows (AB half first), BN <= 16384;  y, pred [Q,3];  loss_pred [1] (the exact sum of pred[:,0] in
 *   2^-32 fixed point / (2 BN): within an ulp of the fp32 means of :976-977, the same bits on every run);
 *   dy [Q,3], g3 [Q,H] (both or neither) = the gradient of gscale * loss_pred;
 *   scratch: 8 bytes, 8-byte aligned, ZERO before the first call (the kernel leaves it zero; one per concurrently running stream). */
int dpd_decoder_out_asloss(const float* h3, const float* mask, int Q, int H, int BN, const dpd_decoder_params* p, float gscale,
                           float* y, float* pred, float* loss_pred, float* dy, float* g3, float* scratch, void* stream);
/* The same with g3 ALSO written as the RC operand plane(s) pl->g3_rc of the first data-gradient GEMM (plane compute types, pl->Qb == Q,
 * H % 256 == 0, H <= 1024; the bits dpd_split_planes would produce from the fp32 g3): g3 may then be NULL, and dpd_decoder_bwd_data
 * (phases = 6, g3 = NULL) goes on from the plane.  pl == NULL: exactly dpd_decoder_out_asloss.                                     */
int dpd_decoder_out_asloss_planes(const float* h3, const float* mask, int Q, int H, int BN, const dpd_decoder_params* p, float gscale,
                                  float* y, float* pred, float* loss_pred, float* dy, float* g3, const dpd_planes* pl, float* scratch,
                                  void* stream);

/* ---------------------------------------------------------------------------------------------
 * DPDist-as-a-loss ENGINE (round 5): the whole as-loss evaluation -- the reference's spliced graph
 *   input1, input2 -> pc_compare/output1, output2 -> (mean(output1[...,0]) + mean(output2[...,0])) / 2
 * (pcrnet-registration/iterative_PCRNet_ours.py:229-257, train_multi_gpu_pc_compare_dist.py:427-453) and its gradient w.r.t. the two
 * clouds -- behind ONE entry point per direction, on buffers sized once for a fixed (B, N).  Same kernels, same order and same bits as
 * calling dpd_mfv3d_fwd_stacked, dpd_patch_rows_fwd_scaled, dpd_decoder_fwd, dpd_decoder_out_asloss | dpd_decoder_bwd_data (phases 6),
 * dpd_patch_rows_bwd, dpd_mfv3d_bwd, dpd_asloss_combine one by one; what it removes is the host: ~30 buffer allocations and a dozen
 * foreign-function calls per evaluation bound the registration loop at its batch of 16 (one forward + backward per training step, one forward per evaluation batch).
 * All members point into ONE caller-owned allocation (dpd_asloss_bytes / dpd_asloss_carve: host-side pointer arithmetic only); the
 * DPDist weights are frozen in this mode: dpd_asloss_set_weights derives what the compute type needs from them (transposed fp32
 * copies or bf16 operand planes) ONCE and keeps the caller's parameter pointers -- call it again after the weights change.
 * B*N < 16384, N <= 4096, H % 64 == 0; one engine per concurrently running stream.                                               */
typedef struct dpd_asloss {
    int B, N, m, k, KP, H, dtype;      /* dtype: enum dpd_dtype */
    float sigma;
    float *pts, *q, *fv, *ssq, *mask;  /* front end: [2B,N,3] x2, [2B,m^3,20], [2B,DPD_MFV_SLICES,20], [Q] */
    int32_t* vox;                      /* [Q] */
    float *X, *h1, *h2;                /* DPD_F32 only (NULL otherwise: the plane types keep them as bf16 planes) [Q,KP], [Q,H] x2 */
    float *h3, *y, *pred, *dy, *g3;    /* [Q,H], [Q,3] x3, [Q,H] */
    float *g2, *g1;                    /* DPD_F32 only */
    float *dX, *dfv, *dpts;            /* [Q,KP], [2B,m^3,20], [2B,N,3] */
    float *W2T, *W3T, *W1pT;           /* DPD_F32 only: transposed weight copies (dpd_asloss_set_weights) */
    float* scratch;                    /* 8 bytes for dpd_decoder_out_asloss: zeroed by dpd_asloss_init */
    void* mfv_ws; size_t mfv_ws_bytes; /* dpd_mfv3d_bwd_workspace_bytes(2B, m) */
    void* ws; size_t ws_bytes;         /* dpd_workspace_bytes(Q, KP, H, dtype) */
    dpd_planes planes;                 /* plane compute types: X, h1, h2, g3, g2, g1 as RC planes, the weights' R8 + RC planes */
    dpd_decoder_params params;         /* filled by dpd_asloss_set_weights */
} dpd_asloss;
size_t dpd_asloss_bytes(int B, int N, int m, int k, int H, int dtype);
int dpd_asloss_carve(void* mem, size_t bytes, int B, int N, int m, int k, int H, int dtype, float sigma, dpd_asloss* out);
/* zero what must be zero before the first evaluation (the loss accumulator): once, on `stream` */
int dpd_asloss_init(const dpd_asloss* e, void* stream);
/* `e` is updated (its params member); p's W*T members are ignored (the engine owns its own transposed copies) */
int dpd_asloss_set_weights(dpd_asloss* e, const dpd_decoder_params* p, void* stream);
/* pcA, pcB [B,N,3] -> loss [1] (loss_pred, utils/dpdist_util.py:976-979).  want_grad != 0 also leaves what dpd_asloss_backward needs
 * (the output-layer backward runs inside the same launch as the output layer).                                                    */
int dpd_asloss_forward(const dpd_asloss* e, const float* pcA, const float* pcB, int want_grad, float* loss, void* stream);
/* gradient of upstream * loss w.r.t. pcA / pcB -> gA, gB [B,N,3]; upstream = DEVICE scalar (NULL = 1).  Needs the state of the last
 * dpd_asloss_forward(want_grad = 1) on this engine; may be called more than once for it.                                           */
int dpd_asloss_backward(const dpd_asloss* e, const float* upstream, float* gA, float* gB, void* stream);
/* both directions with upstream = 1 (callers without an autograd engine in between) */
int dpd_asloss_forward_backward(const dpd_asloss* e, const float* pcA, const float* pcB, float* loss, float* gA, float* gB, void* stream);

/* Host utility: CRC32C (Castagnoli, reflected, init/xorout ~0) of n bytes continuing from `crc` (0 to start); used
 * by the TensorFlow-checkpoint interchange of dpdist_amd/tf_checkpoint.py.  No device work.                 */
uint32_t dpd_crc32c(const void* data, size_t n, uint32_t crc);

/* ---------------------------------------------------------------------------------------------
 * Chamfer distance (baseline loss of the AUE task).  Replaces pairwise_diff + chmafer_dist
 * (train_multi_gpu_pc_compare_dist.py:891-916): a [B,N,3] (pc), b [B,M,3] (rec_pc),
 *   loss[0] = ( mean_bi min_j |b_bi - a_bj|^2 + mean_bj min_i |a_bj - b_bi|^2 ) / 2     (squared distances).
 * min_a/arg_a [B,N], min_b/arg_b [B,M] receive the per-point minima and their indices (kept for the backward).
 * dpd_chamfer_bwd: da, db (either may be NULL) = gscale * d loss / d a, d loss / d b (overwritten).        */
int dpd_chamfer_fwd(const float* a, const float* b, int B, int N, int M, float* min_a, int32_t* arg_a, float* min_b,
                    int32_t* arg_b, float* loss, void* stream);
int dpd_chamfer_bwd(const float* a, const float* b, int B, int N, int M, const int32_t* arg_a, const int32_t* arg_b,
                    float gscale, float* da, float* db, void* stream);

/* ---------------------------------------------------------------------------------------------
 * All-pairs Chamfer and Hausdorff: the baseline distance matrices of two SETS of clouds (dpdist_amd/baselines.py), one DIRECTED matrix
 * per call; the caller runs each direction with the sets swapped, as for the all-pairs DPDist.  S [Cs,Ns,3]: the "surface" clouds,
 * Q [Cq,Nq,3]: the "query" clouds; countsS / countsQ: per-cloud counts (int32, DEVICE memory, the rules of the RAGGED block: never read
 * by the host, clamped into [1, width] by the kernels, the padding is never read); NULL = the set is full.  With ns_i, nq_j the counts,
 *   d2(q, s)  = (dx*dx + dy*dy) + dz*dz, d? = q? - s?, fp32 and not fused (chamfer_pair_sq of csrc/chamfer_scan.h)
 *   mn(i,j,n) = min_{p < ns_i} d2(Q[j,n], S[i,p]),  arg(i,j,n) = the lowest p that attains it
 *   mean_sq[i,j] = (1 / nq_j) sum_{n < nq_j} mn          mean_rt[i,j] = (1 / nq_j) sum_{n < nq_j} sqrtf(mn)
 *   max_sq[i,j]  = max_{n < nq_j} mn                      (each [Cs,Cq] and optional; at least one, else DPD_E_NULL)
 * dpd_chamfer_matrix_bwd: W [Cs,Cq] = the upstream of the directed mean of `form` (0: mean_sq, 1: mean_rt; else DPD_E_DIM),
 *   dQ[j,n] =   sum_i W[i,j] / nq_j * t(Q[j,n], S[i, arg(i,j,n)])                                   (i ascending)
 *   dS[i,p] = - sum_j W[i,j] / nq_j * sum_{n : arg(i,j,n) = p} t(Q[j,n], S[i,p])                    (j, then n ascending)
 *   t(q, s) = 2 (q - s) for form 0; (q - s) / |q - s| for form 1, with the hardware reciprocal square root of d2 and exactly 0 where
 *   the minimum is 0 (the deviation of dpd_chamfer_sqrt_bwd).  The argmins are recomputed, nothing of size [Cs,Cq,N] is stored.  dS
 *   [Cs,Ns,3] and dQ [Cq,Nq,3] are overwritten, either may be NULL (both: DPD_E_NULL); rows at or beyond a cloud's count are +0.0.
 * Every sum has one fixed order that depends on the pair's two counts only, and there are no atomics: two calls give the same bits, and
 * a pair's forward values are bit for bit those of the entry on that pair alone (Cs = Cq = 1, widths cut to the counts) -- the padded
 * widths, the padding and the other clouds change no bit.  No workspace, no allocation, stream-ordered.
 * Refusals, before anything is launched and with the outputs untouched: DPD_E_NULL for a missing S, Q, W or output; DPD_E_DIM for
 * Cs < 1, Cq < 1 or Cs * Cq >= 2^31; DPD_E_UNSUPPORTED unless 1 <= Ns, Nq <= 4096 (the surface cloud lives in LDS).  The number of
 * clouds is not bound by a grid dimension.                                                                                            */
int dpd_chamfer_matrix_fwd(const float* S, const int32_t* countsS, int Cs, int Ns, const float* Q, const int32_t* countsQ, int Cq, int Nq,
                           float* mean_sq, float* mean_rt, float* max_sq, void* stream);
int dpd_chamfer_matrix_bwd(const float* S, const int32_t* countsS, int Cs, int Ns, const float* Q, const int32_t* countsQ, int Cq, int Nq,
                           int form, const float* W, float* dS, float* dQ, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Nearest-point distance labels of the training set; replaces scipy's cdist(point_set, candidates).min(0) of the reference's
 * label generator (dataset_sample_with_gt.py:90-91,121-122).  For each of S shapes
 *   dist[s][i] = min_j |q_si - p_sj|   (Euclidean, NOT squared),   arg[s][i] = the lowest such j (arg may be NULL).
 * ref [S,P,3], qry [S,M,3], dist [S,M] fp32, arg [S,M] int32.  One launch covers all shapes.
 * The squared distance of a pair is (dx*dx + dy*dy) + dz*dz in fp32 with d? = q? - p?, in that order and not fused (the form of
 * dpd_chamfer_fwd); a minimum does not depend on the visiting order, so dist = sqrtf(min) is defined bit for bit and ties go to the
 * lowest index.  Inputs are assumed finite (a NaN coordinate never wins the minimum; the result for such a cloud is unspecified).
 * Any P, M >= 1 up to DPD_NN_MAX_POINTS and S up to DPD_NN_MAX_SHAPES; beyond: DPD_E_UNSUPPORTED.  The workload's shape is
 * P = 10 000, M = 50 000, S = 1 ... 16.  DPD_NN_CHUNK reference points pass through LDS at a time, DPD_NN_TILE queries per workgroup.  */
#define DPD_NN_CHUNK 2048
#define DPD_NN_TILE 256
#define DPD_NN_MAX_POINTS (1 << 24)
#define DPD_NN_MAX_SHAPES 65535
int dpd_nn_dist(const float* ref, const float* qry, int S, int P, int M, float* dist, int32_t* arg, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Farthest-point sampling: the row order the reference's readers presume when they take "the first npoints" rows of a shape file
 * (modelnet_dataset.py:121-122,136; modelnet40_normal_resampled was written in this order), and the gather of a sample
 * (csrc/fps.hip; dpdist_amd/sampling.py: farthest_point_order, farthest_point_sample; dpdist_amd/dataset.py: resample_tree).
 * This comment is the definition.  For one cloud of n points p_0 .. p_{n-1} (fp32), start index s and K outputs:
 *   dmin_j = +inf, taken_j = false for all j;  cur = s
 *   for k = 0 .. min(K, n) - 1:
 *     order[k]  = cur
 *     radius[k] = (k == 0) ? +inf : sqrtf(dmin_cur)            the distance of the chosen point to all earlier ones
 *     taken_cur = true
 *     d_j    = (dx*dx + dy*dy) + dz*dz, d? = p_j? - p_cur?     fp32, in this order and not fused: the form of dpd_nn_dist
 *     dmin_j = d_j < dmin_j ? d_j : dmin_j
 *     cur    = the j with taken_j == false of largest dmin_j; among equals the LOWEST j
 *   order[k] = -1, radius[k] = 0   for min(K, n) <= k < K
 * The valid part of `order` is a prefix of a permutation of 0 .. n-1: a chosen point is excluded, not merely at distance 0, so duplicate
 * points never repeat an index.  The order for K is a prefix of the order for any K' > K, and radius[1:] is non-increasing.  A maximum
 * does not depend on the visiting order once ties go to the lowest index, so the result is defined bit for bit whatever the tiling (every
 * merge across lanes, waves and rounds compares (dmin, index)).  Inputs must be finite (the result for a cloud with a NaN or infinite
 * coordinate is unspecified, but every index written stays below n).
 * dpd_fps_order: pts [S,W,3]; counts [S] (int32, DEVICE memory, the rules of the RAGGED block: never read by the host, clamped into
 * [1, W] by the kernel, the padding is never read; NULL = every cloud has W points); start [S] (int32, device memory, clamped into
 * [0, n_c - 1] by the kernel; NULL = 0); order [S,K] int32; radius [S,K] fp32 or NULL.  One workgroup of DPD_FPS_THREADS threads per cloud,
 * S clouds in one launch; clouds of W <= DPD_FPS_RESIDENT_POINTS are held in registers, wider ones (up to DPD_FPS_MAX_POINTS) are
 * re-read from global memory every iteration -- the same bits either way.  Two calls give the same bits; a cloud's result does not depend
 * on W, the padding or the other clouds.  ws: dpd_fps_workspace_bytes(S, W) bytes of device scratch, 4-byte aligned: 0 for
 * W <= DPD_FPS_RESIDENT_POINTS (ws may then be NULL), S * W floats beyond (the wide form's dmin; needs no initialisation); 0 as well for
 * a shape the entry refuses.
 * dpd_fps_gather_fwd: out[c,k,:] = src[c, order[c,k], :] for rows of D floats (3: points; 6: points with normals), +0.0 where order is -1.
 * dpd_fps_gather_bwd: its adjoint; dsrc [S,W,D] is fully written by one launch: row order[c,k] receives dout[c,k,:], every other row
 * +0.0.  No atomics: the valid entries of a row of `order` must be DISTINCT (an FPS order is; with repeats the row's value is one of the
 * candidates' and unspecified which).
 * Refusals, before anything is launched and with the outputs untouched: DPD_E_NULL for a missing pts / src / dout, order, out or dsrc;
 * DPD_E_DIM for S, W, K, D < 1 or K > W; DPD_E_UNSUPPORTED for S > DPD_FPS_MAX_CLOUDS, W > DPD_FPS_MAX_POINTS, W * D >= 2^31 or a
 * workspace smaller than dpd_fps_workspace_bytes.  No allocation, stream-ordered.                                                      */
#define DPD_FPS_THREADS 1024
#define DPD_FPS_RESIDENT_POINTS 16384
#define DPD_FPS_MAX_POINTS (1 << 20)
#define DPD_FPS_MAX_CLOUDS 65535
size_t dpd_fps_workspace_bytes(int S, int W);
int dpd_fps_order(const float* pts, const int32_t* counts, const int32_t* start, int S, int W, int K, int32_t* order, float* radius,
                  void* ws, size_t ws_bytes, void* stream);
int dpd_fps_gather_fwd(const float* src, const int32_t* order, int S, int W, int D, int K, float* out, void* stream);
int dpd_fps_gather_bwd(const float* dout, const int32_t* order, int S, int W, int D, int K, float* dsrc, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Earth Mover's distance by approximate matching (Fan et al.), the EMD loss of the registration baselines
 * (utils/tf_util_loss.py:42-47 earth_mover; csrc/emd.hip).  This comment is the definition.
 * For each pair b, xyz1 [B,n,3] has n points and xyz2 [B,m,3] has m.  All arithmetic is fp32; d2(k,l) = (dx*dx + dy*dy) + dz*dz.
 * Matching: remainL[k] = max(n,m)/n, remainR[l] = max(n,m)/m, match[l][k] = 0 (shape [m][n]).  For j = 7, 6, ..., -2 take
 * level = -4^j, except level = 0 at j = -2; each level runs three steps:
 *   1. for every k: ratioL[k] = remainL[k] / (1e-9 + sum_l exp(level d2(k,l)) remainR[l])
 *   2. for every l: s = remainR[l] * sum_k exp(level d2(k,l)) ratioL[k];  ratioR[l] = min(remainR[l] / (s + 1e-9), 1) * remainR[l];
 *      then remainR[l] = max(0, remainR[l] - s)
 *   3. for every k, with w(k,l) = exp(level d2(k,l)) ratioL[k] ratioR[l]:  match[l][k] += w(k,l) for every l;
 *      remainL[k] = max(0, remainL[k] - sum_l w(k,l))
 * Cost and loss: cost[b] = sum_{k,l} match[l][k] sqrt(d2(k,l));  loss[0] = mean_b(cost[b] / n).
 * Gradient (the match is a constant): d cost / d xyz1[k] = sum_l match[l][k] (xyz1[k] - xyz2[l]) / sqrt(max(d2, 1e-20)), d cost / d xyz2[l]
 * the negative of the corresponding sum over k; grad1 [B,n,3] and grad2 [B,m,3] receive them times gscale / (B n), i.e.
 * gscale * d loss / d xyz.  grad1, grad2 and match [B,m,n] are optional (NULL: not computed / not written): cost and gradients are
 * accumulated level by level from w, so nothing of size [B,m,n] exists unless match is asked for, and they are the same bits with
 * and without it.  exp is the hardware base-2 exponential of (level log2 e) d2, 1/sqrt the hardware reciprocal square root.
 * Every sum has a fixed order and there are no atomics: two calls give identical bits.
 * ws: dpd_emd_workspace_bytes(B, n, m) bytes of device scratch (the four vectors and per-point cost; DPD_E_WORKSPACE if smaller).
 * 1 <= n, m <= DPD_EMD_MAX_POINTS and B >= 1; beyond: DPD_E_UNSUPPORTED (dpd_emd_workspace_bytes: 0).
 * dpd_emd_match_cost: cost, loss and the gradients of the same formulas for a GIVEN match [B,m,n] (the op's match_cost).           */
#define DPD_EMD_MAX_POINTS 2048
size_t dpd_emd_workspace_bytes(int B, int n, int m);
int dpd_emd_fwd(const float* xyz1, const float* xyz2, int B, int n, int m, float gscale, float* cost, float* loss, float* grad1,
                float* grad2, float* match, void* ws, size_t ws_bytes, void* stream);
int dpd_emd_match_cost(const float* xyz1, const float* xyz2, int B, int n, int m, const float* match, float gscale, float* cost,
                       float* loss, float* grad1, float* grad2, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * All-pairs Earth Mover's distance: the EMD of every pair of two SETS of clouds (dpdist_amd/emd.py: emd_matrix, EMDMatrix;
 * csrc/emd_matrix.hip), one launch with one workgroup per pair.  A [Ca,Na,3], B [Cb,Nb,3]; countsA / countsB: per-cloud counts (int32,
 * DEVICE memory, the rules of the RAGGED block: never read by the host, clamped into [1, width] by the kernels, the padding is never
 * read); NULL = the set is full.  For pair (i,j), n = countsA[i] and m = countsB[j]:
 *   cost[i,j] = dpd_emd_fwd's cost[0] for xyz1 = A_i[:n], xyz2 = B_j[:m], B = 1 (the definition above, unchanged), bit for bit
 *   dist[i,j] = cost[i,j] / n, which is earth_mover of that pair               (each [Ca,Cb]; either may be NULL, both: DPD_E_NULL)
 * The match is not symmetric: a set against itself is called with B == A and computes all Ca^2 pairs, there is no transpose shortcut.
 * dpd_emd_matrix_bwd: the match is a constant and is recomputed (the forward keeps nothing).  With g1(i,j) [n,3] and g2(i,j) [m,3] the
 * definition's d cost / d xyz1 and d cost / d xyz2 of the pair and W [Ca,Cb] the upstream of dist,
 *   dA[i,k] = sum_j (W[i,j] / n_i) g1(i,j)[k]        j ascending, from +0.0
 *   dB[j,l] = sum_i (W[i,j] / n_i) g2(i,j)[l]        i ascending, a left fold from +0.0, or from dB's value when accumulate_dB != 0
 * so a caller may split A into consecutive row blocks (A, countsA, W and dA advanced, accumulate_dB set from the second block on) without
 * changing a bit.  dA [Ca,Na,3] and dB [Cb,Nb,3]: either may be NULL (both: DPD_E_NULL), a skipped side is not computed; rows at or
 * beyond a cloud's count are written +0.0.  ws: dpd_emd_matrix_workspace_bytes = Ca * Cb * (Na + Nb) * 3 floats of device scratch for
 * the per-pair gradients (the backward only; 0 for a refused shape); a second kernel folds them in the orders above.
 * Every sum has one fixed order that depends on the pair's two counts only, and there are no atomics: two calls give the same bits, and
 * the padded widths, the padding and the other clouds change no bit.  No allocation, stream-ordered.
 * Refusals, before anything is launched and with the outputs untouched: DPD_E_NULL for a missing A, B, W or all outputs; DPD_E_DIM for
 * Ca < 1, Cb < 1 or Ca * Cb >= 2^31; DPD_E_UNSUPPORTED unless 1 <= Na, Nb <= DPD_EMD_MAX_POINTS (both clouds of a pair live in LDS);
 * DPD_E_WORKSPACE for a missing or too small workspace.  The number of pairs is not bound by a grid dimension.                        */
size_t dpd_emd_matrix_workspace_bytes(int Ca, int Na, int Cb, int Nb);
int dpd_emd_matrix_fwd(const float* A, const int32_t* countsA, int Ca, int Na, const float* B, const int32_t* countsB, int Cb, int Nb,
                       float* cost, float* dist, void* stream);
int dpd_emd_matrix_bwd(const float* A, const int32_t* countsA, int Ca, int Na, const float* B, const int32_t* countsB, int Cb, int Nb,
                       const float* W, float* dA, float* dB, int accumulate_dB, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The baselines PER PAIR, for ragged batches: Chamfer / Hausdorff and the Earth Mover's distance of the pairs (A_b, B_b), b < P, of two
 * sets A [P,Wa,3] and B [P,Wb,3] (dpdist_amd/baselines.py: chamfer_pairs, hausdorff_pairs, ChamferPairs; dpdist_amd/emd.py: emd_pairs,
 * EMDPairs; csrc/chamfer_pairs.hip, csrc/emd_pairs.hip).  The definitions are those of the two matrix blocks above restricted to the
 * pairs (b, b); the launch shape is the one for few, large pairs (a pair is spread over workgroups).  countsA / countsB [P]: per-cloud
 * counts (int32, DEVICE memory, the rules of the RAGGED block: never read by the host, clamped into [1, width] by the kernels, the
 * padding is never read); NULL = the set is full.  With na = countsA[b], nb = countsB[b]:
 *
 * dpd_chamfer_pairs_fwd.  A is the surface of the AB direction:
 *   min_ab[b,n] = min_{p < na} d2(B[b,n], A[b,p]), arg_ab[b,n] = the lowest p that attains it      [P,Wb], n < nb
 *   min_ba[b,k] = min_{p < nb} d2(A[b,k], B[b,p]), arg_ba[b,k] likewise                            [P,Wa], k < na
 *   mean_sq, mean_rt, max_sq: [2,P], row 0 the AB direction (over the nb queries of B_b), row 1 BA -- the matrix block's formulas.
 *   The four min / arg arrays are REQUIRED (the means are reduced from them and the backward reads the argmins); their entries at or
 *   beyond a count are NOT written.  The three [2,P] outputs are each optional; with none of them only min / arg are produced.
 *   Every value is bit for bit dpd_chamfer_matrix_fwd's on that pair alone (Cs = Cq = 1, the same counts): a second launch reduces the
 *   minima in that kernel's order (lane t sums the queries t, t + 256, ... ascending, wave_sum's tree, ((w0 + w1) + (w2 + w3))).
 * dpd_chamfer_pairs_bwd.  G_ab, G_ba [P]: the upstreams of the two directed means of `form` (0: mean_sq, 1: mean_rt; else DPD_E_DIM);
 *   either may be NULL (that direction carries no gradient and its routes are skipped; both: DPD_E_NULL).  arg_ab / arg_ba: the forward's.
 *   dA[b,k] = (surface route of AB at A[b,k]) + (query route of BA at A[b,k]),  dB[b,n] = (query route of AB) + (surface route of BA),
 *   each route dpd_chamfer_matrix_bwd's formula at Cs = Cq = 1: w = G[b] / n_query (one fp32 division), terms w * (s * (x - y)) with
 *   s = 2 or the hardware reciprocal square root of d2 (exactly nothing where d2 is 0), the surface route in ascending query order.  The
 *   bits are those of the sum of that entry's two calls on the pair alone.  dA [P,Wa,3], dB [P,Wb,3] are overwritten by ONE kernel with
 *   one writer per element; either may be NULL (both: DPD_E_NULL); rows at or beyond a count are written +0.0.
 *
 * dpd_emd_pairs_fwd.  cost[b] = dpd_emd_fwd's cost[0] of xyz1 = A_b[:na], xyz2 = B_b[:nb] at B = 1, bit for bit; dist[b] = cost[b] / na
 *   (each [P]; either may be NULL, both: DPD_E_NULL).
 * dpd_emd_pairs_bwd.  W [P]: the upstream of dist.  The match is a constant and is recomputed.  With g1(b), g2(b) the definition's
 *   d cost / d xyz1, d cost / d xyz2 of the pair:  dA[b,k] = +0.0 + (W[b] / na) g1(b)[k],  dB[b,l] = +0.0 + (W[b] / na) g2(b)[l]
 *   -- the bits of dpd_emd_matrix_bwd on the pair alone.  Either of dA, dB may be NULL (both: DPD_E_NULL), a skipped side is not
 *   computed; rows at or beyond a count are written +0.0.
 *   form: 0 = the library chooses by the padded widths, 1 = one launch (one workgroup per pair, the all-pairs kernel over the pair map
 *   p -> (p, p)), 2 = per pass (dpd_emd_fwd's own pass kernels, given the counts: a workgroup per 64-point owner tile of a pair, 22 launches).
 *   Both forms run the same pass bodies and give the same bits.  ws: dpd_emd_pairs_workspace_bytes(P, Wa, Wb) = P (3 Wa + 2 Wb) floats
 *   of device scratch (the vectors of form 2; required by every form, since form 0 does not tell; 0 for a refused shape).
 *
 * Every sum has one fixed order that depends on the pair's two counts only, and there are no atomics: two calls give the same bits, and
 * the padded widths, the padding and the other pairs change no bit.  No allocation, stream-ordered; P is not bound by a grid dimension.
 * Refusals, before anything is launched and with the outputs untouched: DPD_E_NULL for a missing set, min / arg array, upstream or all
 * outputs; DPD_E_DIM for P < 1 or a bad form; DPD_E_UNSUPPORTED unless 1 <= Wa, Wb <= 4096 (Chamfer) or DPD_EMD_MAX_POINTS (EMD);
 * DPD_E_WORKSPACE for a missing or too small workspace.                                                                               */
int dpd_chamfer_pairs_fwd(const float* A, const int32_t* countsA, int Wa, const float* B, const int32_t* countsB, int Wb, int P,
                          float* min_ab, int32_t* arg_ab, float* min_ba, int32_t* arg_ba, float* mean_sq, float* mean_rt, float* max_sq,
                          void* stream);
int dpd_chamfer_pairs_bwd(const float* A, const int32_t* countsA, int Wa, const float* B, const int32_t* countsB, int Wb, int P, int form,
                          const int32_t* arg_ab, const int32_t* arg_ba, const float* G_ab, const float* G_ba, float* dA, float* dB,
                          void* stream);
size_t dpd_emd_pairs_workspace_bytes(int P, int Wa, int Wb);
int dpd_emd_pairs_fwd(const float* A, const int32_t* countsA, int Wa, const float* B, const int32_t* countsB, int Wb, int P, int form,
                      float* cost, float* dist, void* ws, size_t ws_bytes, void* stream);
int dpd_emd_pairs_bwd(const float* A, const int32_t* countsA, int Wa, const float* B, const int32_t* countsB, int Wb, int P, int form,
                      const float* W, float* dA, float* dB, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Pose algebra of the iterative registration that consumes DPDist as its loss (row f2; csrc/pose.hip): ONE launch for the chain of
 * ~115 element-wise ops the reference runs per refinement loop.  pred [B,7] = the pose network's raw output (t, angle, axis).
 *   pose   [B,7]   (optional) quat_normalize(pred): (tanh(t) 0.1, cos(a/2), axis sin(a/2)), |a| <= lim_rot_deg
 *                  (pcrnet-registration/models/ipcr_model.py:285-294); lim_rot_deg == 0: pose = pred
 *   moved  [B,N,3] (optional) src R(u)^T + t (helper.py:539-570), u = q / max(|q|, 1e-12) in mode 0 (the forward-only refinements,
 *                  helper.py:309-329) and q / (|q| + 1e-7) in mode 1 (the training evaluation, iterative_PCRNet_ours.py:211-224)
 *   T_out  [B,4,4] (optional) [R(q / max(|q|, 1e-12)) t; 0 1] @ T_in (helper.py:309-329); T_in NULL = the identity; must not alias T_in
 * dpd_pose_apply_bwd: d moved [B,N,3] of a mode-1 forward -> dpred [B,7] (overwritten); src carries no gradient (the refinements
 * are forward-only, iterative_PCRNet_ours.py:414-441).                                                                            */
int dpd_pose_apply_fwd(const float* pred, const float* src, const float* T_in, int B, int N, float lim_rot_deg, int mode, float* pose,
                       float* moved, float* T_out, void* stream);
int dpd_pose_apply_bwd(const float* pred, const float* src, const float* dmoved, int B, int N, float lim_rot_deg, float* dpred,
                       void* stream);

/* The forward-only pose refinements of a registration step (iterative_PCRNet_ours.py:414-441: 7 per training step, 8 per evaluation batch;
 * only `predicted_transformation` is fetched) with the pose NETWORK on the library as well: per loop, shared MLP 3-64-64-64-128-out_features +
 * max pool over the points for source and template (models/ipcr_model.py:198-233; the template's features are computed once: it never
 * moves), fc 2*out_features-1024-512-256, dropout, fc 7 (:273-284), quat_normalize (:285-294), then the source is moved and T composed
 * (helper.py:309-329) -- four launches per loop + two per call (a loop's pose chain and cloud move are the prologue of the next loop's shared MLP; the
 * template's half of the first dense layer's sum is computed once).  Weights are torch.nn.Linear layout: W [out, in] row-major, fp32.
 *   src, tmpl [B,N,3];  drop_mask [loops,B,256] or NULL: multiplied into the 256-wide layer (0 or 1/keep_prob: the caller draws it);
 *   ws: dpd_pose_refine_workspace_bytes(B, N, out_features) bytes, 16-byte aligned;
 *   moved [B,N,3], T_out [B,4,4]: the source and the accumulated transform after `loops` loops (T starts at the identity);
 *   pred_out [loops,B,7] (optional): the network's raw output of every loop.
 * out_features must be 1024, the reference's width (DPD_E_UNSUPPORTED otherwise).                                                        */
typedef struct dpd_pose_net {
    const float* Wp[5]; const float* bp[5];   /* shared MLP: 64x3, 64x64, 64x64, 128x64, out_features x 128 */
    const float* Wh[4]; const float* bh[4];   /* head: 1024 x 2*out_features, 512x1024, 256x512, 7x256 */
    int out_features;
} dpd_pose_net;
size_t dpd_pose_refine_workspace_bytes(int B, int N, int out_features);
int dpd_pose_refine(const dpd_pose_net* net, const float* src, const float* tmpl, int B, int N, int loops, float lim_rot_deg,
                    const float* drop_mask, void* ws, size_t ws_bytes, float* moved, float* T_out, float* pred_out, void* stream);

/* The pool of the pose network's shared MLP (the reference's --pn_pool max|avg).  DPD_POOL_AVG is models/ipcr_model.py:236-271 (pointnet_avg):
 * the same five layers and head, tf_util.avg_pool2d over the points in place of the max pool -- per (cloud, column) the feature is
 *   f = (sum over the cloud's N points of relu(layer 5)) / (float)N,
 * the sum taken in one fixed order (per 64-point pass: each lane adds the rows the 32x32 MFMA gave it, ascending; the lower lane half's sum
 * + the upper one's; then the passes ascending; the origin rows that pad a partial pass are left out) and the quotient as ONE IEEE fp32
 * division (not a product with a reciprocal).  Any other `pool` value: DPD_E_UNSUPPORTED, before any launch.
 * dpd_pose_refine_pool is dpd_pose_refine with that pool (workspace: dpd_pose_refine_workspace_bytes; the same checks); with DPD_POOL_MAX it
 * IS dpd_pose_refine -- the same launches, the same bits.  Its features have the bits of dpd_pose_point_fwd_train_pool's. */
enum dpd_pool { DPD_POOL_MAX = 0, DPD_POOL_AVG = 1 };
int dpd_pose_refine_pool(const dpd_pose_net* net, const float* src, const float* tmpl, int B, int N, int loops, float lim_rot_deg, int pool,
                         const float* drop_mask, void* ws, size_t ws_bytes, float* moved, float* T_out, float* pred_out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The registration experiment's test protocol (pcrnet-registration/results_itrPCRNet_no_stop.py; csrc/regtest.hip): the occlusion of
 * the source clouds, the per-iteration error tables of the no-stop loop and the square-rooted Chamfer baseline.  None of the four
 * entries allocates; all are stream-ordered and deterministic (fixed summation orders, no atomics).
 *
 * dpd_occlude: helper.add_occlusions (helper.py:963-982) with its host random draws passed in.  src [B,N,3]; per cloud b
 *   d_i = sqrtf((dx*dx + dy*dy) + dz*dz), d? = src[b,i,?] - src[b,seed_idx[b],?], in fp32, in that order and not fused (the form of
 *   dpd_nn_dist; equal to np.linalg.norm(s - p, 2, -1) on float32 input bit for bit).  The `drop` points with the smallest (d_i, i),
 *   compared lexicographically (np.argsort(kind="stable")), are removed.  The S = N - drop survivors are emitted in ascending
 *   (order_key[b,i], i) order -- order_key [B,N] is the caller's draw (uniform random numbers stand in for the reference's
 *   np.random.shuffle; it decides which survivors the wrap-around duplicates) -- or, with order_key == NULL, in ascending (d_i, i) order
 *   (the duplicates then all sit at the rim of the hole).  out [B,N,3]: out[b,j] = survivor[j mod S], the reference's
 *   concatenate-with-itself-then-truncate; kept [B,N] (optional) receives the source index of every output row.  drop == 0 with a NULL
 *   key is a copy.  Inputs are assumed finite (no NaN in src or order_key; the result for such a cloud is unspecified, but stays
 *   inside the arrays).  seed_idx [B] int32 must lie in [0,N): that is the caller's to check (the kernel clamps it so that a bad index
 *   cannot read outside the cloud).  drop < 0 or drop >= N: DPD_E_DIM (the reference would loop forever on an empty survivor set);
 *   N > DPD_OCCLUDE_MAX_POINTS (the reference's MAX_NUM_POINT): DPD_E_UNSUPPORTED.
 *
 * dpd_pose_trace: pred [L,B,7] = the raw outputs of L refinement loops (dpd_pose_refine's pred_out) -> for every pair
 *   T_all [L+1,B,4,4] fp32: T_all[0] = I, T_all[l+1] = [R(q / max(|q|, 1e-12)) t; 0 1] @ T_all[l], (t, q) = quat_normalize(pred[l]) --
 *     the mode-0 arithmetic of dpd_pose_apply_fwd (the same device functions: T_all[L] is dpd_pose_refine's T_out bit for bit);
 *   te, re, ce [L+1,B] double, from the fp32 T_all[l], all arithmetic in double:
 *     te = | gt_t - (trans(inv T) + shift) |                                       (get_error + find_errors, :464-474, :112-116)
 *     re = the angle, in degrees, of R_p R_gt^-1 with R_p = euler2mat(mat2euler(rot(inv T))) as helper.find_final_pose_inv and
 *          find_errors build it (:118-133) -- the Euler round trip is the identity on a rotation, and maps the not-quite-orthogonal
 *          fp32 product to one -- taken as atan2(|vee(E - E^T)| / 2, (tr E - 1) / 2) rather than acos, which loses half its digits
 *          near 0 and 180 degrees;
 *     ce[0] = 1, ce[l] = | T_all[l] inv(T_all[l-1]) - I |_F^2                                          (check_convergenceT, :155-167).
 *   gt_pose [B,6] = (t, rx, ry, rz), radians, R_gt = Rx Ry Rz (registration.euler_to_mat); shift [B,3] or NULL = the centroid that was
 *   subtracted from the source (the T of get_error).  T_all, te, re, ce are each optional (at least one; te and re need gt_pose).
 *   One thread per pair.  L < 1 or B < 1: DPD_E_DIM.
 *
 * dpd_chamfer_sqrt_fwd / _bwd: PCRNet's Chamfer loss (utils/tf_util_loss.py:35-39), argument lists of dpd_chamfer_fwd / _bwd:
 *   loss[0] = ( mean_bi sqrt(min_j |b_bi - a_bj|^2) + mean_bj sqrt(min_i |a_bj - b_bi|^2) ) / 2.
 *   min_* receive the SQUARED minima and arg_* the indices: the bits dpd_chamfer_fwd stores (one scan, csrc/chamfer_scan.h).
 *   Backward: autodiff through the stored argmins; a pair's term is (x - y) / |x - y| times its mean's weight.  DEVIATION: where a
 *   minimum is 0 (coincident points) the reference's gradient is inf * 0 = NaN; here that pair contributes exactly zero.           */
#define DPD_OCCLUDE_MAX_POINTS 2048
int dpd_occlude(const float* src, const int32_t* seed_idx, const float* order_key, int B, int N, int drop, float* out, int32_t* kept,
                void* stream);
int dpd_pose_trace(const float* pred, int L, int B, float lim_rot_deg, const float* gt_pose, const float* shift, float* T_all, double* te,
                   double* re, double* ce, void* stream);
int dpd_chamfer_sqrt_fwd(const float* a, const float* b, int B, int N, int M, float* min_a, int32_t* arg_a, float* min_b, int32_t* arg_b,
                         float* loss, void* stream);
int dpd_chamfer_sqrt_bwd(const float* a, const float* b, int B, int N, int M, const int32_t* arg_a, const int32_t* arg_b, float gscale,
                         float* da, float* db, void* stream);

/* The TRAINING evaluation of the pose network's shared MLP + max pool (models/ipcr_model.py:198-233 inside the step of
 * pcrnet-registration/iterative_PCRNet_ours.py:442-470, which differentiates the network w.r.t. its weights only): forward with what the
 * backward needs, and TF / torch autodiff of the five 1x1 convolutions, their ReLUs and tf.reduce_max.
 *   dpd_pose_point_fwd_train: clouds ptsA [nA,N,3] then ptsB [nB,N,3] (nB may be 0) -> f [nA+nB, out_features]; stored for the backward:
 *     h1, h2, h3 [(nA+nB) N, 64], h4 [(nA+nB) N, 128] (16-byte aligned) and the max pool's tie mask, W = dpd_pose_point_tie_words(N) =
 *     ceil(N / 64) words of 8 bytes per (cloud, column): ties [nA+nB, W, out_features]; bit b of word w set <=> point 64 w + b attains the
 *     column's maximum and that maximum is positive (the gradient of reduce_max is shared evenly among ties).  For N <= 64 that is one word
 *     per (cloud, column), [nA+nB, out_features].  N <= 2048 (the reference's MAX_NUM_POINT); beyond: DPD_E_UNSUPPORTED.
 *   dpd_pose_point_bwd: df [nA+nB, out_features] -> dW[i], db[i] (i = 0..4, shapes of net->Wp / bp; overwritten).  ws:
 *     dpd_pose_point_bwd_workspace_bytes_n(nA + nB, N) bytes (one partial record per cloud and 64-point chunk; 0 for an N the entries
 *     refuse); dpd_pose_point_bwd_workspace_bytes(clouds) is that size for N <= 64.  Same N limit.  Deterministic (every sum in a fixed
 *     order, no atomics).  The head's fields of `net` are not read. */
int dpd_pose_point_tie_words(int N);
size_t dpd_pose_point_bwd_workspace_bytes(int clouds);
size_t dpd_pose_point_bwd_workspace_bytes_n(int clouds, int N);
int dpd_pose_point_fwd_train(const dpd_pose_net* net, const float* ptsA, const float* ptsB, int nA, int nB, int N, float* f, float* h1, float* h2,
                             float* h3, float* h4, unsigned long long* ties, void* stream);
int dpd_pose_point_bwd(const dpd_pose_net* net, const float* ptsA, const float* ptsB, int nA, int nB, int N, const float* df, const float* h1,
                       const float* h2, const float* h3, const float* h4, const unsigned long long* ties, float* const* dW, float* const* db,
                       void* ws, size_t ws_bytes, void* stream);
/* The same two entries with the pool as an argument (enum dpd_pool above); with DPD_POOL_MAX they ARE the entries above (which call them):
 * the same launches, the same bits, and dpd_pose_point_bwd_workspace_bytes_pool(clouds, N, DPD_POOL_MAX) ==
 * dpd_pose_point_bwd_workspace_bytes_n(clouds, N).  With DPD_POOL_AVG:
 *   forward: f = sum / (float)N as stated at enum dpd_pool; `words` (the tie words' buffer and layout, [nA+nB, W, out_features]) receives the
 *     GATE words: bit b of word w set <=> point 64 w + b is a real point (< N) and its layer-5 pre-activation is > 0.
 *   backward: coef[c, col] = df[c, col] / (float)N (one IEEE division), g5[c, p, col] = gate bit ? coef[c, col] : 0;
 *     dW5[col, :] = sum over (cloud, point) of g5 h4[point, :] on the fp32 matrix cores: an fmaf chain over the points of a 64-point chunk
 *       ascending, the chunks of a split ascending (cloud-major), then the splits' partials ascending (the (cloud, chunk) range is cut into
 *       min(clouds W, 32) contiguous splits);
 *     db5[col] = sum over the clouds ascending of coef[c, col] * (float)popcount(the gate words of (c, col));
 *     the gradient of layer 4's output and dW1..dW4, db1..db4 through the kernels of the max pool (they do not look at the pool).
 *     ws: dpd_pose_point_bwd_workspace_bytes_pool(nA + nB, N, DPD_POOL_AVG) bytes -- the max pool's records, then coef, coef * popcount
 *     [clouds, out_features] each and the split partials [splits, out_features, 128]; h4 16-byte aligned.
 * Refusals before any launch: pool not in enum dpd_pool: DPD_E_UNSUPPORTED (the workspace entry returns 0); N > 2048, out_features != 1024:
 * DPD_E_UNSUPPORTED; the NULL / dimension / workspace checks of the entries above.  Deterministic (no atomics). */
size_t dpd_pose_point_bwd_workspace_bytes_pool(int clouds, int N, int pool);
int dpd_pose_point_fwd_train_pool(const dpd_pose_net* net, const float* ptsA, const float* ptsB, int nA, int nB, int N, int pool, float* f, float* h1,
                                  float* h2, float* h3, float* h4, unsigned long long* words, void* stream);
int dpd_pose_point_bwd_pool(const dpd_pose_net* net, const float* ptsA, const float* ptsB, int nA, int nB, int N, int pool, const float* df,
                            const float* h1, const float* h2, const float* h3, const float* h4, const unsigned long long* words, float* const* dW,
                            float* const* db, void* ws, size_t ws_bytes, void* stream);

/* The head of the same training evaluation (models/ipcr_model.py:273-284: fc 2 x out_features -> 1024 -> 512 -> 256, ReLU each, dropout on the
 * last, -> 7) and its autodiff.  f [2B, out_features] = the pooled features (rows < B: first cloud set, rows >= B: second; the head reads
 * their concatenation without materialising it); drop_mask [B,256] (0 or 1/keep) or NULL.
 *   dpd_pose_head_fwd_train: -> h1 [B,1024], h2 [B,512], h3 [B,256] (after the mask), pred [B,7] (the network's raw output).
 *   dpd_pose_head_bwd: dpred [B,7] -> dW[i], db[i] (i = 0..3, shapes of net->Wh / bh; overwritten) and df [2B, out_features];
 *     ws: dpd_pose_head_bwd_workspace_bytes(B).  Deterministic.  The shared MLP's fields of `net` are not read.                               */
size_t dpd_pose_head_bwd_workspace_bytes(int B);
int dpd_pose_head_fwd_train(const dpd_pose_net* net, const float* f, int B, const float* drop_mask, float* h1, float* h2, float* h3, float* pred,
                            void* stream);
int dpd_pose_head_bwd(const dpd_pose_net* net, const float* f, int B, const float* drop_mask, const float* h1, const float* h2, const float* h3,
                      const float* dpred, float* const* dW, float* const* db, float* df, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * tf.train.AdamOptimizer step (epsilon-hat form), train_multi_gpu_pc_compare_dist.py:216,301:
 *   g' = g * gscale;  m = b1 m + (1-b1) g';  v = b2 v + (1-b2) g'^2;  p -= lr_t m / (sqrt(v)+eps)
 * with lr_t = lr sqrt(1-b2^t)/(1-b1^t) computed by the caller.  n elements (any n).              */
int dpd_adam_tf(float* p, const float* g, float* m, float* v, size_t n, float lr_t, float b1, float b2,
                float eps, float gscale, void* stream);

/* One-launch optimizer step (same arithmetic, element for element, as dpd_adam_tf):
 *   WT[i] != NULL (or planes, below): the matrix p[w_off[i] ..] of shape [w_rows[i], w_cols[i]] (row-major; cols % 64 == 0, rows % 4 == 0, offsets
 *     ascending) is updated tile-wise and its transposed copy WT[i] [w_cols[i], w_rows[i]] is rewritten in the same pass
 *     (replaces dpd_weights_transpose after the step);
 *   partials != NULL: the LAST 4H+3 elements p[tail_off .. tail_off+4H+3) = [b3 | W4 | b4] (followed by at most 3 zero padding
 *     elements up to n) take their gradient from the block partials
 *     that dpd_decoder_bwd_data(phases | 16) left in dpd_small_grads.partials (nparts = ceil(Qb / 8) records of `rec`
 *     floats); the reduced gradient is stored to g, and when `loss` is given (rec >= 4H+8: fused L1 loss) loss[0..1] are
 *     finished exactly as the deferred reduction would (single-GPU steps only: a data-parallel step needs the reduced
 *     gradient before its all-reduce).                                                                                  */
typedef struct dpd_adam_fuse {
    float* WT[3];
    long w_off[3];
    int w_rows[3], w_cols[3];
    /* bf16-matrix-core compute types: the operand planes of the updated matrices (dpd_planes.W*_rc / W*_r8; either may be NULL),
     * np = 1 or 3 planes each, written in the same pass (replaces dpd_weights_to_planes after the step; rows % 8 == 0);
     * np = 0: none */
    void* W_rc[3];
    void* W_r8[3];
    int np;
    const float* partials;
    int nparts, rec, H, Qb;
    long tail_off;
    float* loss;
} dpd_adam_fuse;
int dpd_adam_tf_fused(float* p, float* g, float* m, float* v, size_t n, float lr_t, float b1, float b2, float eps, float gscale,
                      const dpd_adam_fuse* fuse, void* stream);

/* The same update with lr_t read from DEVICE memory (state[3] of an 8-float caller-owned buffer), so that a captured (hipGraph) step carries
 * no per-step host parameter: the host writes state[3] before every replay (dpdist_amd/optim.py: TFAdam.prepare_replay).  */
int dpd_adam_tf_dev(float* p, const float* g, float* m, float* v, size_t n, const float* state, float b1, float b2, float eps,
                    float gscale, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Building block, exported for tests and roofline measurement: C = epi(op(A) op(B)), fp32 MFMA.
 *   transA = 0: A is [M,K] (lda);  1: A is stored [K,M].   transB = 0: B is [K,N];  1: B is [N,K].
 *   epilogue: 0 none, 1 +bias[n], 2 relu(+bias[n]), 3 multiply by (gate[m,n] > 0) (ldg = ldc).
 *   K, N, lda, ldb, ldc multiples of 4; split_k >= 1 (slabs in ws, reduced by a second kernel,
 *   epilogue applied after the reduction); tile: 0 = auto (= 3); 3 = register-staged 64x64 (any K % 4 == 0); LDS-DMA ring
 *   kernels (K % 32 == 0, else 3 is used) 8 = 64x64/3-stage, 9 = 128x128/3-stage; register-streamed kernels (no LDS, no
 *   barriers; K % 32 == 0; csrc/gemm_rs.h): workgroup of 4 waves, wave tile 30 = 64x64, 31 = 64x32, 32 = 32x64, 33 = 32x32.
 * Pinned by tests/test_gemm_edges_gpu.py (exact against an int64 product, operands and output inside NaN guard bands):
 *   - strides: lda, ldb, ldc may exceed the logical row; only A / B elements inside [M,K] / [K,N] are read and only C[0:M, 0:N]
 *     is written.  The gate is read as gate[m * ldc + n]: it has the row stride of C, not N.  bias is [N];
 *   - fall-back: tiles 8, 9, 30-33 need whole 32-deep K-tiles and M, N >= 4.  With K % 32 != 0, M < 4, N < 4, or a split_k whose
 *     32-rounded slice length leaves the last slice empty (ceil32(ceil(K / split_k)) * (split_k - 1) >= K), the call runs on tile 3
 *     instead: same result, any K % 4 == 0;
 *   - split_k > 1: ws holds split_k slabs of M*N floats (ws_bytes >= split_k * M * N * 4, else DPD_E_WORKSPACE) and need not be
 *     initialised: every slab is written whole before the reduction reads it, a slab whose K slice is empty as zeros;
 *   - split_k = 0 = tail split, tiles 30-33 only: taken when ws_bytes >= 3 * M * N * 4, epilogue = 0, the launch has more than 256
 *     workgroup tiles, its last round of 256 is less than 3/4 full and K gives pieces of at least 256 (csrc/gemm_rs.h); the
 *     tiles of the last whole tile rows are then cut along K into at most 4 pieces (pieces - 1 slabs in ws, uninitialised is
 *     fine).  In every other case split_k = 0 is silently split_k = 1 and ws is not touched;
 *   - refusals, before anything is launched (C and ws untouched): DPD_E_NULL for a NULL A / B / C, epilogue 1 / 2 without bias,
 *     epilogue 3 without gate; DPD_E_DIM for M, N, K <= 0 or split_k < 0; DPD_E_UNSUPPORTED for K, N, lda, ldb or ldc not a
 *     multiple of 4, transA with M % 4 != 0, transA && transB, an epilogue outside 0..3, an unknown tile.                       */
int dpd_gemm_f32(int transA, int transB, int M, int N, int K, const float* A, int lda, const float* B, int ldb,
                 float* Cout, int ldc, const float* bias, const float* gate, int epilogue, int split_k, int tile,
                 void* ws, size_t ws_bytes, void* stream);

/* Two independent exact-fp32 products in ONE launch of the register-streamed kernels (csrc/gemm_rs.h: gemm_rs_pair_kernel): the
 * workgroups of part a come first, those of part b behind them; no workgroup waits for another.  The fields mean what the arguments
 * of dpd_gemm_f32 mean.  The pair form takes exactly:
 *   a  NN (transA = transB = 0), M_dev set (the live row count, a device word <= M; M is the capacity the grid is launched for; rows
 *      from the count on are not written), epilogue 3 with `gate` (row stride ldc);
 *   b  TN (transA = 1: A stored [K,M]), K_dev set (the live contraction length, a device word clamped to [0, K] and rounded down to
 *      32; 0 stores zeros), epilogue 0, K >= 32 and K % 32 == 0; bias_out (may be NULL): [N] = the sum over bias_nparts blocks of
 *      bias_parts [bias_nparts][N], in block order, by the part's first-row-block waves;
 *   both: tile 32 or 33 (same bits), split_k = 1.
 * Every element has the bits the part's own dpd_gemm_f32-style launch gives.  Refusals, before anything is launched: DPD_E_NULL for a
 * NULL part or operand, DPD_E_UNSUPPORTED for any other form (split-K, the tail split, another tile, K < 32 in part b, ...).          */
typedef struct dpd_gemm_pair_part {
    int transA, transB, M, N, K;
    const float* A; int lda;
    const float* B; int ldb;
    float* C; int ldc;
    const float* gate;
    int epilogue, split_k, tile;
    const int32_t* M_dev;
    const int32_t* K_dev;
    const float* bias_parts; float* bias_out; int bias_nparts;
} dpd_gemm_pair_part;
int dpd_gemm_f32_pair(const dpd_gemm_pair_part* a, const dpd_gemm_pair_part* b, void* stream);

/* ---------------------------------------------------------------------------------------------
 * bf16-plane building blocks (gemm_x3.hip).  A plane tensor holds np (1 or 3) bf16 planes of an fp32 matrix in
 * 16-byte chunks of 8 contraction elements:
 *   RC layout (contraction index = column):  plane[r][c],           leading dimension ld_rc (elements)
 *   R8 layout (contraction index = row):     plane[r/8][c][r%8]
 * dpd_split_planes writes either or both (rc / r8 may be NULL) from src [R,C] (row stride ld; R, C multiples of 8).
 * dpd_gemm_planes: C [M,N] fp32 = epi(A B), A/B given as planes; a_fmt/b_fmt: 0 = RC (A stored [M,K], B stored
 * [N,K]), 1 = R8 (A stored [K,M], B stored [K,N]); lda/ldb = row stride for RC, M resp. N for R8; K % 32 == 0;
 * epilogue/bias/gate as in dpd_gemm_f32; tile 0 = default.  out_rc / out_r8 (may be NULL): the result is ALSO
 * written as np planes, RC [np][M][N] and/or R8 [np][r8_rows/8][N][8] (rows < r8_rows), ready to be an operand of
 * the next GEMM; C may then be NULL.
 * Pinned by tests/test_gemm_edges_gpu.py (exact against an int64 product, every buffer inside NaN guard bands):
 *   - dpd_split_planes: ld % 4 == 0; ld_rc, rc_plane and r8_plane (elements between planes) multiples of 8 (16-byte stores; the caller's
 *     duty, not checked); ld, ld_rc may exceed C and the plane strides a plane: only src[0:R, 0:C] is read and only the np planes' [R, C] (RC) / [R/8][C][8] (R8) elements written;
 *   - dpd_gemm_planes: a_fmt / b_fmt (0,1) = NN, (0,0) = NT, (1,1) = TN, (2,2) = TN with both operands as the RC planes of [K,M] / [K,N]
 *     (tiles 0, 1, 2, 3, 5; M, N multiples of 8); lda / ldb multiples of 8, for an RC operand they may exceed its row and the padding
 *     columns are never read; ldc % 4 == 0 may exceed N, only C[0:M, 0:N] is written; the gate has the row stride ldc;
 *   - tiles: 1-5 with one or three planes, 13 one plane and K % 64 == 0, 21 / 23 one plane, 24 three planes; DPD_E_UNSUPPORTED otherwise;
 *   - out_rc / out_r8 need M, N, r8_rows multiples of 8; out_rc is dense ([np][M][N]); rows >= r8_rows have no R8 output.              */
int dpd_split_planes(const float* src, int R, int C, int ld, int np, void* rc, int ld_rc, long rc_plane, void* r8,
                     long r8_plane, void* stream);
int dpd_gemm_planes(int np, int a_fmt, int b_fmt, int M, int N, int K, const void* A, int lda, long a_plane,
                    const void* B, int ldb, long b_plane, float* C, int ldc, const float* bias, const float* gate,
                    int epilogue, int tile, void* out_rc, void* out_r8, int r8_rows, void* stream);

/* Tuning knob (process-wide, never needed for correctness): GEMM tile / split-K per
 * call site.  op: 0 fwd layer 1, 1 fwd layers 2-3, 2 bwd dH, 3 bwd dX, 4 bwd dW1, 5 bwd dW2/3, 6 / 7 bwd dH / dX with a
 * transposed weight copy, 8 layer 1 of dpd_decoder_fwd_unique (tile 32 or 33 only), 9 / 10 / 11 the live-row dH / dW1 / dW2+dW3
 * of the `_live` entries and 12 the dW part of dpd_decoder_bwd_pair_live (tile 32 or 33 only: same bits, default 33; 13-15 are free); 16 + op: one-plane (bf16) tile of gemm_x3.hip for that call site (0 = automatic; 1-5 ring kernels, 13 =
 * 192x128 at BK 64, 21 / 23 / 24 phase-staggered), 32: its grouped dW2/dW3 launch, 33: the grouped dW1/dW2/dW3 launch of
 * dpd_decoder_bwd_weights_trio.  tile as in dpd_gemm_f32 (0 = auto); split_k applies to ops 4, 5 and, for the plane weight gradients
 * (ops 20, 21, 32, 33): n > 1 = n K slices per tile reduced inside the launch (last-arriving slice, slice order: deterministic),
 * n < -1 = |n| fp32 slabs + a reduce launch, 1 = off, 0 = automatic.
 * Defaults are the measured best.                                                                                        */
int dpd_set_gemm_plan(int op, int tile, int split_k);

/* dW1, dW2 and dW3 of a plane compute type (dtype 1 / 2) in ONE grouped launch; all operands are the R8 planes of `pl`
 * (X / g1, h1 / g2, h2 / g3).  Same gradients as dpd_decoder_bwd_weights(1) + dpd_decoder_bwd_weights_pair up to fp32 summation
 * order; no bias gradients (the plane compute types get them from the dH epilogues of dpd_decoder_bwd_data).  DPD_E_UNSUPPORTED
 * when a plane is missing or a shape is not plane-shaped: the caller then makes the separate calls.
 * Replaces TF autodiff of the three tf.nn.conv2d kernels (utils/tf_util.py:213, train_multi_gpu_pc_compare_dist.py:274-277).   */
int dpd_decoder_bwd_weights_trio(int Qb, int KP, int H, int dtype, float* dW1, float* dW2, float* dW3, void* ws, size_t ws_bytes,
                                 const dpd_planes* pl, void* stream);

/* Opt-in profiler for the roofline measurement (bench.py): when enabled, every GEMM kernel launch is bracketed
 * by a hipEvent pair on its own stream.  dpd_prof_collect waits for them and returns the launch count and the
 * summed durations [ms] / flops (2*M*N*K as launched) since dpd_prof_enable(1).                              */
int dpd_prof_enable(int on);
/* the mode the profiler is in (0 = off).  A live-row launch (dpd_live_rows) has no shape the host knows, so its bracket would carry the
 * DENSE 2*M*N*K against a shorter duration and the quotient would no longer be a rate: a caller that wants achieved rates checks this and
 * runs the dense entries while the profiler is on (DPDistTrainer.backward does).                                           */
int dpd_prof_enabled(void);
int dpd_prof_collect(double* total_ms, double* total_flops);
/* the same for ONE product form: 0 = NN / NT (forward layers and data gradients -- in DPD_F32 one kernel, the step's dominant one),
 * 1 = TN (weight gradients)                                                                                               */
int dpd_prof_collect_form(int form, double* total_ms, double* total_flops);
/* dpd_prof_enable(2) additionally brackets the bandwidth-bound kernels of the step and records their ALGORITHMIC HBM bytes (every
 * input read once, every output written once) by stage: 1 3DmFV encoder, 2 window gather, 3 fused output layer (+ loss + its backward),
 * 4 optimizer, 5 small-gradient reduction, 6 weight copies (transposes / operand planes), 7 the finish launch of layer 1 over distinct
 * windows (dpd_decoder_fwd_cross only, which also records its output layer under 3 and its pair means under 5).  Returns the launches of that stage since
 * dpd_prof_enable(2) and fills their summed duration [ms] and bytes; dpd_prof_collect keeps counting GEMM launches only.          */
int dpd_prof_collect_stage(int stage, double* total_ms, double* total_bytes);

#ifdef __cplusplus
}
#endif
#endif /* DPDIST_CAPI_H */

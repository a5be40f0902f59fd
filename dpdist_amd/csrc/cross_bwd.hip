// Backward of the ALL-PAIRS distance matrix (exact fp32, as-loss mode: the decoder is frozen, gradients go to the two cloud sets;
// include/dpdist_capi.h: dpd_cross_invert, dpd_cross_bwd, dpd_cross_bwd_workspace_bytes).
//
// The forward (patch_rows_cross.h) runs layer 1 once per (surface cloud, occupied voxel) slot because the voxel of a query does not
// depend on the surface cloud.  The layer-1 data gradient is linear, so the same holds backwards: the rows g1 [rows_p, H] of all
// queries that share a slot are SUMMED first (gs [slot_cap, H]) and multiplied by W1p^T once per slot (dXs [slot_cap, KP]); the window
// columns of dXs are then scattered to the surface's Fisher vector by a gather over the slots, and only the three q - centre columns
// are taken per row (dq [rows, 3], a dot product with three rows of W1p).  Rows are ordered (i, j, n) as in the forward.
// Everything below is deterministic: no atomics on floats, one summation order per output element, whatever the launch holds.
#include "common.h"
#include "cross_chunk.h"
#include "gemm_host.h"
#include "slot_bwd.h"

namespace dpd {

constexpr int kCF = DPD_FV_CHANNELS;
constexpr int kCrossMaxH = kSlotMaxH;      // slot_sum_kernel: one wave per 256 columns, at most 16 waves

// One workgroup: the queries sorted by slot (invert_block of slot_bwd.h: a stable counting sort, ascending query id inside a slot), the
// start offset of every slot and the voxel of every slot.  Integer only, one order.
//   slot_start [m^3 + 1]  start of slot s in qlist for s < U, QN for s >= U (so slot s holds [slot_start[s], slot_start[s + 1]))
//   qlist [QN]            query ids sorted by (slot, query id)
//   slot_vox [m^3]        voxel id of slot s for s < U, -1 for s >= U
__global__ __launch_bounds__(1024) void cross_invert_kernel(const int32_t* __restrict__ vox, const int32_t* __restrict__ slot_of_vox,
                                                            const int32_t* __restrict__ ucount, int QN, int G,
                                                            int32_t* __restrict__ slot_start, int32_t* __restrict__ qlist,
                                                            int32_t* __restrict__ slot_vox) {
    __shared__ int s_cnt[1024];      // per voxel: the count, then the running position of the voxel's slot
    __shared__ int s_wsum[16];
    const int tid = threadIdx.x;
    const int U = min(max(ucount[0], 0), G);
    if (tid >= U && tid < G) slot_vox[tid] = -1;
    if (tid >= U && tid <= G) slot_start[tid] = QN;
    invert_block(vox, slot_of_vox, U, QN, G, 0, slot_start, qlist, slot_vox, s_cnt, s_wsum);
}

// Upstream spread, the inverse of pair_mean_kernel: dpred[r] = (Gd[pair of r] / N, 0, 0) for the real rows, 0 for the pad rows.
// CNT (dpd_cross_bwd_counts): row (i, j, n) gets Gd[i, j] / qcounts[j] for n < qcounts[j] (clamped into [1, N]) and 0 otherwise.
template <bool CNT>
__device__ __forceinline__ void cross_spread_block(const float* __restrict__ Gd, int N, int rows, int rows_p, float* __restrict__ dpred,
                                                   const int32_t* __restrict__ qcounts, int Cb) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= rows_p) return;
    float v = 0.f;
    if (r < rows) {
        const int pr = r / N;
        const int n1 = CNT ? min(max(qcounts[pr % Cb], 1), N) : N;
        if (!CNT || r - pr * N < n1) v = Gd[pr] / (float)n1;
    }
    dpred[(size_t)r * 3] = v;
    dpred[(size_t)r * 3 + 1] = 0.f;
    dpred[(size_t)r * 3 + 2] = 0.f;
}
__global__ __launch_bounds__(256) void cross_spread_kernel(const float* __restrict__ Gd, int N, int rows, int rows_p, float* __restrict__ dpred) {
    cross_spread_block<false>(Gd, N, rows, rows_p, dpred, nullptr, 1);
}
__global__ __launch_bounds__(256) void cross_spread_counts_kernel(const float* __restrict__ Gd, const int32_t* __restrict__ qcounts, int N, int Cb,
                                                                  int rows, int rows_p, float* __restrict__ dpred) {
    cross_spread_block<true>(Gd, N, rows, rows_p, dpred, qcounts, Cb);
}

// Slot sum + query route: g1 [rows_p, H] is streamed once.  Workgroup t < Ca U owns slot (i, s) = (t / U, t % U): wave w owns the
// columns [256 w, 256 w + 256), lane l the float4 at 256 w + 4 l.  For every query of the slot's list, in list order:
//   gs[t, :] += g1[(i, qn), :]                                  (one chain per element, list order)
//   dq[(i, qn), c] = sum_w wave_sum( g1[(i, qn), cols of w] . W1p[E + c, cols of w] ),  c = 0..2   (fixed tree per wave, waves ascending)
// Workgroups Ca U <= t < slot_cap write ZERO rows of gs: the slot product runs over the capacity.
// gs = NULL: the surface set needs no gradient (only dq); dq = NULL: the query set needs none (only gs).
__global__ __launch_bounds__(1024) void slot_sum_kernel(const float* __restrict__ g1, const int32_t* __restrict__ cnt,
                                                        const int32_t* __restrict__ slot_start, const int32_t* __restrict__ qlist,
                                                        const float* __restrict__ Wq /* W1p + E H: three rows */, int Ca, int QN, int H, int ucap,
                                                        float* __restrict__ gs, float* __restrict__ dq) {
    __shared__ float s_part[kSlotRows][16][3];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int U = min(max(cnt[0], 0), ucap);
    const int t = blockIdx.x;
    const int col = 256 * wave + 4 * lane;
    if (t >= Ca * U) {
        if (gs && col < H) *reinterpret_cast<float4*>(gs + (size_t)t * H + col) = make_float4(0.f, 0.f, 0.f, 0.f);
        return;
    }
    const int i = t / U, s = t % U;
    const int b = min(max(slot_start[s], 0), QN), e = min(max(slot_start[s + 1], b), QN);
    slot_sum_rows(g1 + (size_t)i * QN * H, qlist, b, e, QN, H, Wq, gs ? gs + (size_t)t * H : nullptr, dq ? dq + (size_t)i * QN * 3 : nullptr,
                  s_part);
}

// Window scatter over the slots, as a gather (scatter_slots of slot_bwd.h): workgroup (i, slice) owns a slice of the voxels of surface i
// and, for every (voxel, float4 channel group), sums that window column of every slot of the surface whose window covers the voxel, in
// ascending slot order.  U comes from device memory.
__global__ __launch_bounds__(256) void cross_scatter_kernel(const float* __restrict__ dXs, const int32_t* __restrict__ cnt,
                                                            const int32_t* __restrict__ slot_vox, float* __restrict__ dfv, int m, int k, int KP,
                                                            int ucap, int slices) {
    __shared__ int s_vox[1024];       // packed voxel coordinates of the slots (m <= 10: at most 1000)
    const int c = blockIdx.x / slices, sl = blockIdx.x % slices;
    const int G = m * m * m;
    const int U = min(min(max(cnt[0], 0), ucap), 1024);
    const int gper = (G + slices - 1) / slices;
    const int gbeg = sl * gper, gend = min(G, gbeg + gper);
    scatter_slots(dXs + (size_t)c * U * KP, slot_vox, U, dfv + (size_t)c * G * kCF, m, k, KP, gbeg, gend, false, s_vox);
}

// Query-route reduction: gQ[j, n, c] = gQ[j, n, c] + dq[(0, j, n), c] + dq[(1, j, n), c] + ... in ascending surface: the chain goes on
// from the accumulated value, so a chunk boundary changes no bit (the caller zeroes gQ before the first chunk).
__global__ __launch_bounds__(256) void cross_qreduce_kernel(const float* __restrict__ dq, int Ca, int QN3, float* __restrict__ gQ) {
    qreduce_chain(dq, Ca, QN3, gQ);
}

}  // namespace dpd

namespace {
// THE shape predicate of the all-pairs backward: a chunk the forward takes (dpd_cross_workspace_bytes is cross_shape_ok, patch_rows.hip)
// whose slot product dXs [slot_cap, KP] is addressable by the GEMM kernels, at a width slot_sum_kernel covers
bool cross_bwd_shape_ok(int Ca_chunk, int Cb, int N, int m, int k, int KP, int H) {
    if (H <= 0 || H > dpd::kCrossMaxH || (H & 63)) return false;
    if (!dpd_cross_workspace_bytes(Ca_chunk, Cb, N, m, k, KP, H)) return false;
    const size_t cap = (size_t)dpd_cross_slot_capacity(Ca_chunk, Cb, N, m);
    return cap && dpd::fits_gemm_offsets(cap, (size_t)KP);
}
}  // namespace

extern "C" size_t dpd_cross_bwd_workspace_bytes(int Ca_chunk, int Cb, int N, int m, int k, int KP, int H) {
    if (!cross_bwd_shape_ok(Ca_chunk, Cb, N, m, k, KP, H)) return 0;
    return dpd::cross_chunk_bytes(Ca_chunk, Cb, N, m, KP, H, true);
}

extern "C" int dpd_cross_invert(const int32_t* vox, const int32_t* slot_of_vox, const int32_t* ucount, int Cb, int N, int m,
                                int32_t* slot_start, int32_t* qlist, int32_t* slot_vox, void* stream) {
    using namespace dpd;
    if (!vox || !slot_of_vox || !ucount || !slot_start || !qlist || !slot_vox) return DPD_E_NULL;
    if (Cb <= 0 || N <= 0 || (long)Cb * N > (1L << 24)) return DPD_E_DIM;
    if (m < 1 || m > 10) return DPD_E_UNSUPPORTED;
    StageProf prof(stream, DPD_STAGE_GATHER, (double)Cb * N * 8.0 + (double)m * m * m * 12.0);
    DPD_LAUNCH(cross_invert_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, vox, slot_of_vox, ucount, Cb * N, m * m * m, slot_start, qlist,
               slot_vox);
    DPD_CHECK_LAUNCH();
    return 0;
}

extern "C" int dpd_cross_slot_sum(const float* g1, const int32_t* cnt, const int32_t* slot_start, const int32_t* qlist, const float* W1p,
                                  int Ca_chunk, int Cb, int N, int m, int k, int KP, int H, int slot_cap, float* gs, float* dq, void* stream) {
    using namespace dpd;
    if (!g1 || !cnt || !slot_start || !qlist || (!gs && !dq) || (dq && !W1p)) return DPD_E_NULL;
    if (Ca_chunk <= 0 || Cb <= 0 || N <= 0 || slot_cap <= 0) return DPD_E_DIM;
    if (!cross_bwd_shape_ok(Ca_chunk, Cb, N, m, k, KP, H)) return DPD_E_UNSUPPORTED;
    if (slot_cap != dpd_cross_slot_capacity(Ca_chunk, Cb, N, m)) return DPD_E_DIM;
    const int QN = Cb * N, ucap = cross_ucap(Cb, N, m);
    const int rows = Ca_chunk * QN;
    StageProf prof(stream, DPD_STAGE_SMALL_REDUCE, (double)rows * H * 4.0 + (gs ? (double)slot_cap * H * 4.0 : 0.0) + (dq ? rows * 12.0 : 0.0) + QN * 4.0);
    // with gs = NULL only the live slots matter, but the live count is a device word: the dead workgroups return at once
    DPD_LAUNCH(slot_sum_kernel, dim3(slot_cap), dim3(64 * ((H + 255) / 256)), 0, (hipStream_t)stream, g1, cnt, slot_start, qlist,
               W1p ? W1p + (size_t)(k * k * k * kCF) * H : nullptr, Ca_chunk, QN, H, ucap, gs, dq);
    DPD_CHECK_LAUNCH();
    return 0;
}

extern "C" int dpd_cross_scatter(const float* dXs, const int32_t* cnt, const int32_t* slot_vox, int Ca_chunk, int Cb, int N, int m, int k,
                                 int KP, float* dfv, void* stream) {
    using namespace dpd;
    if (!dXs || !cnt || !slot_vox || !dfv) return DPD_E_NULL;
    if (Ca_chunk <= 0 || Cb <= 0 || N <= 0) return DPD_E_DIM;
    if (!cross_bwd_shape_ok(Ca_chunk, Cb, N, m, k, KP, 64)) return DPD_E_UNSUPPORTED;
    const int G = m * m * m, ucap = cross_ucap(Cb, N, m);
    const int slices = (G * 5 + 255) / 256;      // one (voxel, channel group) item per thread
    StageProf prof(stream, DPD_STAGE_GATHER, (double)Ca_chunk * ucap * (k * k * k * kCF) * 4.0 + (double)Ca_chunk * G * kCF * 4.0);
    DPD_LAUNCH(cross_scatter_kernel, dim3(Ca_chunk * slices), dim3(256), 0, (hipStream_t)stream, dXs, cnt, slot_vox, dfv, m, k, KP, ucap, slices);
    DPD_CHECK_LAUNCH();
    return 0;
}

// qcounts = NULL: dpd_cross_bwd; otherwise the upstream spread over each query cloud's own count (everything after it is unchanged: a
// padded query is a masked query of voxel 0 since dpd_cross_index_counts)
static int cross_bwd(const float* Gd, const float* maskr, const int32_t* qcounts, const float* y, const float* h1, const float* h2,
                     const float* h3, const int32_t* cnt, const int32_t* slot_start, const int32_t* qlist, const int32_t* slot_vox, int Ca_chunk,
                     int Cb, int N, int m, int k, int KP, int H, int slot_cap, const dpd_decoder_params* p, float* dpred, float* dy, float* ga,
                     float* gb, float* dq, float* gs, float* dXs, float* dfv, float* gQ, void* stream) {
    using namespace dpd;
    const bool surface = dfv != nullptr, query = gQ != nullptr;
    if (!Gd || !maskr || !y || !h1 || !h2 || !h3 || !cnt || !slot_start || !qlist || !p || !dpred || !dy || !ga || !gb) return DPD_E_NULL;
    if (!surface && !query) return DPD_E_NULL;
    if (surface && (!slot_vox || !gs || !dXs || !p->W1pT)) return DPD_E_NULL;
    if (query && (!dq || !p->W1p)) return DPD_E_NULL;
    if (!p->W2 || !p->W3 || !p->W4 || !p->W1p) return DPD_E_NULL;
    if (Ca_chunk <= 0 || Cb <= 0 || N <= 0 || slot_cap <= 0) return DPD_E_DIM;
    if (!cross_bwd_shape_ok(Ca_chunk, Cb, N, m, k, KP, H)) return DPD_E_UNSUPPORTED;
    if (slot_cap != dpd_cross_slot_capacity(Ca_chunk, Cb, N, m)) return DPD_E_DIM;
    hipStream_t s = (hipStream_t)stream;
    const int QN = Cb * N, rows = Ca_chunk * QN, rows_p = (int)cross_rows_p(Ca_chunk, Cb, N);
    // 2. upstream spread
    {
        StageProf prof(stream, DPD_STAGE_SMALL_REDUCE, (double)Ca_chunk * Cb * 4.0 + rows_p * 12.0);
        if (qcounts)
            DPD_LAUNCH(cross_spread_counts_kernel, dim3((rows_p + 255) / 256), dim3(256), 0, s, Gd, qcounts, N, Cb, rows, rows_p, dpred);
        else
            DPD_LAUNCH(cross_spread_kernel, dim3((rows_p + 255) / 256), dim3(256), 0, s, Gd, N, rows, rows_p, dpred);
        DPD_CHECK_LAUNCH();
    }
    // 3. layers 4..2: g3 -> ga, g2 -> gb, g1 -> ga (masked queries and pad rows: exact zeros through the mask)
    if (int rc = dpd_decoder_bwd_data(dpred, maskr, y, h1, h2, h3, rows_p, KP, H, p, DPD_F32, dy, ga, gb, ga, nullptr, nullptr, nullptr, 0, nullptr, 7,
                                      stream))
        return rc;
    // 5. slot sum + query route
    if (int rc = dpd_cross_slot_sum(ga, cnt, slot_start, qlist, p->W1p, Ca_chunk, Cb, N, m, k, KP, H, slot_cap, surface ? gs : nullptr,
                                    query ? dq : nullptr, stream))
        return rc;
    if (surface) {
        // 6. slot product over the capacity (the dead rows of gs are zero): dXs [slot_cap, KP] = gs W1p^T, NN on the transposed copy
        GemmF32Call f;
        f.M = slot_cap; f.N = KP; f.K = H;
        f.A = gs; f.lda = H; f.B = p->W1pT; f.ldb = KP; f.C = dXs; f.ldc = KP;
        f.epilogue = EPI_NONE; f.split_k = 1; f.s = s;
        f.tile = ((long)((slot_cap + 127) / 128) * ((KP + 127) / 128) >= 512) ? 30 : 32;      // the choice of the pair path's dX product
        if (int rc = gemm_f32(f)) return rc;
        // 7. window scatter over the slots
        if (int rc = dpd_cross_scatter(dXs, cnt, slot_vox, Ca_chunk, Cb, N, m, k, KP, dfv, stream)) return rc;
    }
    if (query) {
        // 9. query-route reduction, continued from what earlier chunks left in gQ
        StageProf prof(stream, DPD_STAGE_SMALL_REDUCE, (double)rows * 12.0 + QN * 24.0);
        DPD_LAUNCH(cross_qreduce_kernel, dim3((QN * 3 + 255) / 256), dim3(256), 0, s, (const float*)dq, Ca_chunk, QN * 3, gQ);
        DPD_CHECK_LAUNCH();
    }
    return 0;
}

extern "C" int dpd_cross_bwd(const float* Gd, const float* maskr, const float* y, const float* h1, const float* h2, const float* h3,
                             const int32_t* cnt, const int32_t* slot_start, const int32_t* qlist, const int32_t* slot_vox, int Ca_chunk, int Cb,
                             int N, int m, int k, int KP, int H, int slot_cap, const dpd_decoder_params* p, float* dpred, float* dy, float* ga,
                             float* gb, float* dq, float* gs, float* dXs, float* dfv, float* gQ, void* stream) {
    return cross_bwd(Gd, maskr, nullptr, y, h1, h2, h3, cnt, slot_start, qlist, slot_vox, Ca_chunk, Cb, N, m, k, KP, H, slot_cap, p, dpred, dy, ga,
                     gb, dq, gs, dXs, dfv, gQ, stream);
}

extern "C" int dpd_cross_bwd_counts(const float* Gd, const float* maskr, const int32_t* qcounts, const float* y, const float* h1, const float* h2,
                                    const float* h3, const int32_t* cnt, const int32_t* slot_start, const int32_t* qlist,
                                    const int32_t* slot_vox, int Ca_chunk, int Cb, int N, int m, int k, int KP, int H, int slot_cap,
                                    const dpd_decoder_params* p, float* dpred, float* dy, float* ga, float* gb, float* dq, float* gs, float* dXs,
                                    float* dfv, float* gQ, void* stream) {
    if (!qcounts) return DPD_E_NULL;
    return cross_bwd(Gd, maskr, qcounts, y, h1, h2, h3, cnt, slot_start, qlist, slot_vox, Ca_chunk, Cb, N, m, k, KP, H, slot_cap, p, dpred, dy,
                     ga, gb, dq, gs, dXs, dfv, gQ, stream);
}

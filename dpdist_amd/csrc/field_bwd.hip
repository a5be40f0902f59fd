// Slot-summed backward of the PER-POINT FIELD (exact fp32, as-loss mode: the decoder is frozen, gradients go to the surfaces and the
// queries; include/dpdist_capi.h: dpd_field_invert, dpd_field_slot_sum, dpd_field_scatter, dpd_field_bwd).
//
// The forward (patch_rows_field.h) runs layer 1 once per occupied (cloud, voxel) slot.  The layer-1 data gradient is linear, so the same
// holds backwards, as for the all-pairs matrix (cross_bwd.hip): the rows g1 [rows_p, H] of all queries of a cloud that share a slot are
// SUMMED first (gs [slot_cap, H]) and multiplied by W1p^T once per slot (dXs [slot_cap, KP]); the window columns of dXs are gathered into
// the cloud's Fisher-vector gradient over the cloud's OWN slots, and only the three q - centre columns are taken per row.  The layout is
// the field's: every cloud has its own queries and slots, the slots are cloud-major at base_c + s (base_c = the sum of U_c' over c' < c),
// rows are ordered (c, t), and a chunk may be a tile of one cloud's queries.  The device routines are those of the matrix (slot_bwd.h).
// Everything below is deterministic: no atomics on floats, one summation order per output element, whatever the launch holds.
#include "common.h"
#include "field_shape.h"
#include "gemm_host.h"
#include "slot_bwd.h"

namespace dpd {

constexpr int kFC = DPD_FV_CHANNELS;

// by one wave (tid < 64): the slots of the clouds before `cloud` and of all n clouds, each count clamped into [0, ucap] as everywhere
// (integer sums: any order gives the same words; patch_rows_field_kernel adds them up the same way) -> s_base[0], s_base[1]
__device__ __forceinline__ void field_slot_base(const int32_t* __restrict__ ucount, int n, int ucap, int cloud, int* s_base) {
    const int tid = threadIdx.x;
    if (tid >= 64) return;
    int before = 0, all = 0;
    for (int c = tid; c < n; c += 64) {
        const int u = min(max(ucount[c], 0), ucap);
        before += (c < cloud) ? u : 0;
        all += u;
    }
    for (int off = 32; off; off >>= 1) {
        before += __shfl_xor(before, off, 64);
        all += __shfl_xor(all, off, 64);
    }
    if (tid == 0) { s_base[0] = before; s_base[1] = all; }
}

// One workgroup per cloud: the cloud's T chunk queries sorted by slot (invert_block: a stable counting sort, ascending query id inside a
// slot).  Integer only, one order.  With total = the sum of the U_c:
//   qlist [n, T]               row c: the chunk-local query ids of cloud c sorted by (slot, query id)
//   slot_start [slot_cap + 1]  GLOBAL slot base_c + s holds qlist (flat) [slot_start[g], slot_start[g + 1]); n T for total <= g <= slot_cap
//   slot_vox [slot_cap]        voxel id of global slot g; -1 for g >= total
//   slot_cloud [slot_cap]      cloud of global slot g; -1 for g >= total
// Every count is clamped into [0, ucap], ucap = min(m^3, T), so base_c + s < n ucap <= slot_cap: no store passes the capacity.
__global__ __launch_bounds__(1024) void field_invert_kernel(const int32_t* __restrict__ vox, const int32_t* __restrict__ slot_of_vox,
                                                            const int32_t* __restrict__ ucount, int n, int T, int G, int ucap, int slot_cap,
                                                            int32_t* __restrict__ slot_start, int32_t* __restrict__ qlist,
                                                            int32_t* __restrict__ slot_vox, int32_t* __restrict__ slot_cloud) {
    __shared__ int s_cnt[1024];
    __shared__ int s_wsum[16];
    __shared__ int s_base[2];
    const int tid = threadIdx.x, c = blockIdx.x;
    field_slot_base(ucount, n, ucap, c, s_base);
    __syncthreads();
    const int base = s_base[0], total = min(s_base[1], slot_cap);
    const int U = min(min(max(ucount[c], 0), ucap), slot_cap - base);
    if (tid < U) slot_cloud[base + tid] = c;      // (U <= m^3 <= 1000)
    if (c == n - 1) {                             // the dead slots up to the capacity, and the end of the last list
        for (int g = total + tid; g < slot_cap; g += 1024) {
            slot_start[g] = n * T;
            slot_vox[g] = -1;
            slot_cloud[g] = -1;
        }
        if (tid == 0) slot_start[slot_cap] = n * T;
    }
    invert_block(vox + (size_t)c * T, slot_of_vox + (size_t)c * G, U, T, G, c * T, slot_start + base, qlist + (size_t)c * T, slot_vox + base,
                 s_cnt, s_wsum);
}

// Slot sum + query route (slot_sum_rows): workgroup g < total owns global slot g of cloud c = slot_cloud[g]:
//   gs[g, :] = the sum of g1[(c, t), :] over the slot's list, in list order;  dq[c dq_cloud_stride + 3 t + 0..2] = g1[(c, t), :] . Wq[0..2, :]
// Workgroups total <= g < slot_cap write ZERO rows of gs: the slot product runs over the capacity.  total = cnt[1] comes from the device.
// Every device-read word is clamped: the cloud into [0, n), the list into the cloud's rows [c T, c T + T), the query ids into [0, T).
__global__ __launch_bounds__(1024) void field_slot_sum_kernel(const float* __restrict__ g1, const int32_t* __restrict__ cnt,
                                                              const int32_t* __restrict__ slot_start, const int32_t* __restrict__ qlist,
                                                              const int32_t* __restrict__ slot_cloud, const float* __restrict__ Wq, int n, int T,
                                                              int H, int slot_cap, float* __restrict__ gs, float* __restrict__ dq,
                                                              long dq_cloud_stride) {
    __shared__ float s_part[kSlotRows][16][3];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int total = min(max(cnt[1], 0), slot_cap);
    const int g = blockIdx.x;
    const int col = 256 * wave + 4 * lane;
    if (g >= total) {
        if (gs && col < H) *reinterpret_cast<float4*>(gs + (size_t)g * H + col) = make_float4(0.f, 0.f, 0.f, 0.f);
        return;
    }
    const int c = min(max(slot_cloud[g], 0), n - 1);
    const int lo = c * T;
    const int b = min(max(slot_start[g], lo), lo + T), e = min(max(slot_start[g + 1], b), lo + T);
    slot_sum_rows(g1 + (size_t)lo * H, qlist, b, e, T, H, Wq, gs ? gs + (size_t)g * H : nullptr, dq ? dq + (size_t)c * dq_cloud_stride : nullptr,
                  s_part);
}

// Window scatter as a gather (scatter_slots): workgroup (c, slice) owns a slice of the voxels of cloud c and sums over the cloud's OWN
// slots [base_c, base_c + U_c) in ascending slot order.  accumulate: the chain continues from the value dfv[c] holds, so the tiles of one
// cloud add up in ascending tile order; else a plain store (+0.0 for a voxel no slot covers).
__global__ __launch_bounds__(256) void field_scatter_kernel(const float* __restrict__ dXs, const int32_t* __restrict__ ucount,
                                                            const int32_t* __restrict__ slot_vox, float* __restrict__ dfv, int n, int m, int k,
                                                            int KP, int ucap, int slot_cap, int slices, int accumulate) {
    __shared__ int s_vox[1024];       // packed voxel coordinates of the cloud's slots (m <= 10: at most 1000)
    __shared__ int s_base[2];
    const int c = blockIdx.x / slices, sl = blockIdx.x % slices;
    const int G = m * m * m;
    field_slot_base(ucount, n, ucap, c, s_base);
    __syncthreads();
    const int base = min(s_base[0], slot_cap);
    const int U = min(min(min(max(ucount[c], 0), ucap), 1024), slot_cap - base);
    const int gper = (G + slices - 1) / slices;
    const int gbeg = sl * gper, gend = min(G, gbeg + gper);
    scatter_slots(dXs + (size_t)base * KP, slot_vox + base, U, dfv + (size_t)c * G * kFC, m, k, KP, gbeg, gend, accumulate != 0, s_vox);
}

// Query route of ONE SHARED query set: gq[t, :] = gq[t, :] + dq[(0, t), :] + dq[(1, t), :] + ... in ascending cloud, continued from the
// accumulated value (qreduce_chain).  Clouds with their own queries need no launch: the slot sum writes their rows in place.
__global__ __launch_bounds__(256) void field_qreduce_kernel(const float* __restrict__ dq, int n, int T3, float* __restrict__ gq) {
    qreduce_chain(dq, n, T3, gq);
}


// THE shape predicate of the field's backward entries: a chunk the forward takes (field_shape_ok; k <= 0: the window is not known to the
// caller) at a width slot_sum_rows covers (H <= 0: not known either), whose g1 [rows_p, H], gs [slot_cap, H] and slot product
// dXs [slot_cap, KP] are addressable by the GEMM kernels.  -> the slot capacity, 0 = refused
int field_bwd_cap(int n, int T, int m, int k, int KP, int H) {
    if (H > 0 && (H > dpd::kSlotMaxH || (H & 63))) return 0;
    if (!dpd::field_shape_ok(n, T, m, k, KP)) return 0;
    const int cap = dpd_field_slot_capacity(n, T, m);
    if (cap <= 0) return 0;
    if (k > 0 && !dpd::fits_gemm_offsets((size_t)cap, (size_t)KP)) return 0;
    if (H > 0 && !dpd::fits_gemm_offsets((size_t)cap, (size_t)H)) return 0;
    if (H > 0 && !dpd::fits_gemm_offsets(((size_t)n * T + 31) / 32 * 32, (size_t)H)) return 0;      // g1 [rows_p, H]
    return cap;
}

// What follows the decoder chain in dpd_field_bwd, on the chunk's g1 rows (arguments as there, already checked; cap = the slot capacity):
// the slot sum and the query route, then -- for the surfaces -- the slot product and the window scatter, then the chain of a shared
// query set.  keep_gs: gs is formed even when no surface gradient is wanted (dpd_field_bwd_train contracts it with Xu).
int field_routes(const float* g1, const int32_t* cnt, const int32_t* ucount, const int32_t* slot_start, const int32_t* qlist,
                 const int32_t* slot_vox, const int32_t* slot_cloud, int n, int T, int m, int k, int KP, int H, int cap,
                 const dpd_decoder_params* p, float* dq, float* gs, float* dXs, float* dfv, int accumulate, float* gq, long gq_cloud_stride,
                 bool keep_gs, void* stream) {
    const bool surface = dfv != nullptr, query = gq != nullptr;
    const bool shared = query && gq_cloud_stride == 0;
    hipStream_t s = (hipStream_t)stream;
    // slot sum + query route: a cloud's own queries get their rows of gq in place, a shared set goes through dq [n, T, 3]
    if (int rc = dpd_field_slot_sum(g1, cnt, slot_start, qlist, slot_cloud, p->W1p, n, T, m, k, KP, H, cap, (surface || keep_gs) ? gs : nullptr,
                                    query ? (shared ? dq : gq) : nullptr, shared ? 3L * T : gq_cloud_stride, stream))
        return rc;
    if (surface) {
        // slot product over the capacity (the dead rows of gs are zero): dXs [slot_cap, KP] = gs W1p^T, NN on the transposed copy
        GemmF32Call f;
        f.M = cap; f.N = KP; f.K = H;
        f.A = gs; f.lda = H; f.B = p->W1pT; f.ldb = KP; f.C = dXs; f.ldc = KP;
        f.epilogue = EPI_NONE; f.split_k = 1; f.s = s;
        f.tile = ((long)((cap + 127) / 128) * ((KP + 127) / 128) >= 512) ? 30 : 32;      // the tile rule of the matrix's slot product
        if (int rc = gemm_f32(f)) return rc;
        if (int rc = dpd_field_scatter(dXs, ucount, slot_vox, n, T, m, k, KP, accumulate, dfv, stream)) return rc;
    }
    if (shared) {
        StageProf prof(stream, DPD_STAGE_SMALL_REDUCE, (double)n * T * 12.0 + T * 24.0);
        DPD_LAUNCH(field_qreduce_kernel, dim3((T * 3 + 255) / 256), dim3(256), 0, s, (const float*)dq, n, T * 3, gq);
        DPD_CHECK_LAUNCH();
    }
    return 0;
}
}  // namespace dpd

extern "C" int dpd_field_invert(const int32_t* vox, const int32_t* slot_of_vox, const int32_t* ucount, int n, int T, int m, int slot_cap,
                                int32_t* slot_start, int32_t* qlist, int32_t* slot_vox, int32_t* slot_cloud, void* stream) {
    using namespace dpd;
    if (!vox || !slot_of_vox || !ucount || !slot_start || !qlist || !slot_vox || !slot_cloud) return DPD_E_NULL;
    if (n <= 0 || T <= 0 || slot_cap <= 0) return DPD_E_DIM;
    const int cap = field_bwd_cap(n, T, m, 0, 0, 0);
    if (!cap) return DPD_E_UNSUPPORTED;
    if (slot_cap != cap) return DPD_E_DIM;
    const int G = m * m * m;
    StageProf prof(stream, DPD_STAGE_GATHER, (double)n * T * 8.0 + (double)n * G * 4.0 + (double)cap * 16.0);
    DPD_LAUNCH(field_invert_kernel, dim3(n), dim3(1024), 0, (hipStream_t)stream, vox, slot_of_vox, ucount, n, T, G, std::min(G, T), cap, slot_start,
               qlist, slot_vox, slot_cloud);
    DPD_CHECK_LAUNCH();
    return 0;
}

extern "C" int dpd_field_slot_sum(const float* g1, const int32_t* cnt, const int32_t* slot_start, const int32_t* qlist,
                                  const int32_t* slot_cloud, const float* W1p, int n, int T, int m, int k, int KP, int H, int slot_cap, float* gs,
                                  float* dq, long dq_cloud_stride, void* stream) {
    using namespace dpd;
    if (!g1 || !cnt || !slot_start || !qlist || !slot_cloud || (!gs && !dq) || (dq && !W1p)) return DPD_E_NULL;
    if (n <= 0 || T <= 0 || slot_cap <= 0 || H <= 0 || k <= 0) return DPD_E_DIM;
    if (dq && dq_cloud_stride < 3L * T) return DPD_E_DIM;
    const int cap = field_bwd_cap(n, T, m, k, KP, H);
    if (!cap) return DPD_E_UNSUPPORTED;
    if (slot_cap != cap) return DPD_E_DIM;
    const double rows = (double)n * T;
    StageProf prof(stream, DPD_STAGE_SMALL_REDUCE, rows * H * 4.0 + (gs ? (double)cap * H * 4.0 : 0.0) + (dq ? rows * 12.0 : 0.0) + rows * 4.0);
    // with gs = NULL only the live slots matter, but the live count is a device word: the dead workgroups return at once
    DPD_LAUNCH(field_slot_sum_kernel, dim3(cap), dim3(64 * ((H + 255) / 256)), 0, (hipStream_t)stream, g1, cnt, slot_start, qlist, slot_cloud,
               W1p ? W1p + (size_t)(k * k * k * kFC) * H : nullptr, n, T, H, cap, gs, dq, dq_cloud_stride);
    DPD_CHECK_LAUNCH();
    return 0;
}

extern "C" int dpd_field_scatter(const float* dXs, const int32_t* ucount, const int32_t* slot_vox, int n, int T, int m, int k, int KP,
                                 int accumulate, float* dfv, void* stream) {
    using namespace dpd;
    if (!dXs || !ucount || !slot_vox || !dfv) return DPD_E_NULL;
    if (n <= 0 || T <= 0 || k <= 0) return DPD_E_DIM;
    const int cap = field_bwd_cap(n, T, m, k, KP, 0);
    if (!cap) return DPD_E_UNSUPPORTED;
    const int G = m * m * m;
    const int slices = (G * 5 + 255) / 256;      // one (voxel, channel group) item per thread
    StageProf prof(stream, DPD_STAGE_GATHER, (double)cap * (k * k * k * kFC) * 4.0 + (double)n * G * kFC * (accumulate ? 8.0 : 4.0));
    DPD_LAUNCH(field_scatter_kernel, dim3(n * slices), dim3(256), 0, (hipStream_t)stream, dXs, ucount, slot_vox, dfv, n, m, k, KP, std::min(G, T),
               cap, slices, accumulate);
    DPD_CHECK_LAUNCH();
    return 0;
}

extern "C" int dpd_field_bwd(const float* dpred, const float* maskr, const float* y, const float* h1, const float* h2, const float* h3,
                             const int32_t* cnt, const int32_t* ucount, const int32_t* slot_start, const int32_t* qlist,
                             const int32_t* slot_vox, const int32_t* slot_cloud, int n, int T, int m, int k, int KP, int H, int slot_cap,
                             const dpd_decoder_params* p, float* dy, float* ga, float* gb, float* dq, float* gs, float* dXs, float* dfv,
                             int accumulate, float* gq, long gq_cloud_stride, void* stream) {
    using namespace dpd;
    const bool surface = dfv != nullptr, query = gq != nullptr;
    const bool shared = query && gq_cloud_stride == 0;
    if (!dpred || !maskr || !y || !h1 || !h2 || !h3 || !cnt || !slot_start || !qlist || !slot_cloud || !p || !dy || !ga || !gb) return DPD_E_NULL;
    if (!surface && !query) return DPD_E_NULL;
    if (!p->W2 || !p->W3 || !p->W4 || !p->W1p) return DPD_E_NULL;
    if (surface && (!ucount || !slot_vox || !gs || !dXs || !p->W1pT)) return DPD_E_NULL;
    if (shared && !dq) return DPD_E_NULL;
    if (n <= 0 || T <= 0 || slot_cap <= 0 || H <= 0 || k <= 0) return DPD_E_DIM;
    if (query && !shared && gq_cloud_stride < 3L * T) return DPD_E_DIM;
    const int cap = field_bwd_cap(n, T, m, k, KP, H);
    if (!cap) return DPD_E_UNSUPPORTED;
    if (slot_cap != cap) return DPD_E_DIM;
    const int rows_p = (int)(((long)n * T + 31) / 32 * 32);
    // layers 4..2: g3 -> ga, g2 -> gb, g1 -> ga (masked and padded queries and the pad rows: exact zeros through the mask)
    if (int rc = dpd_decoder_bwd_data(dpred, maskr, y, h1, h2, h3, rows_p, KP, H, p, DPD_F32, dy, ga, gb, ga, nullptr, nullptr, nullptr, 0, nullptr, 7,
                                      stream))
        return rc;
    return field_routes(ga, cnt, ucount, slot_start, qlist, slot_vox, slot_cloud, n, T, m, k, KP, H, cap, p, dq, gs, dXs, dfv, accumulate, gq,
                        gq_cloud_stride, false, stream);
}

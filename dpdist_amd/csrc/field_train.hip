// Decoder gradients of the PER-POINT FIELD (exact fp32; include/dpdist_capi.h: dpd_field_bwd_train).
//
// dpd_field_bwd freezes the decoder.  Here the same chunk also yields the gradients of the eight decoder variables.  Layer 1's weight
// gradient is the sum over the rows of x_r (x) g1_r; the first KP - 32 entries of x_r are column uid[r] of Xu, so that part is
//     dW1p[0 : KP - 32] = Xu [KP - 32, slots] gs [slots, H]
// with the slot sums gs the backward forms anyway: one product per SLOT, not per row.  Only the 32 tail columns (Xt: the window's last
// values, q - centre, the zero pad) contract over the rows, together with db1, in a two-step sum over fixed row chunks.  Layers 2 - 4
// are the dense entries of decoder_bwd.hip, between the phases of the data chain (g1 overwrites g3 in ga).  The chunk's gradients are
// formed in the workspace and then stored into or added onto the caller's buffers.  No atomics on floats: every element has one
// summation order, whatever the launch holds.
#include "common.h"
#include "decoder_int.h"
#include "field_shape.h"

namespace dpd {

constexpr int kTailChunks = 64;      // row chunks of the tail product's two-step sum: a constant, so the order depends on rows_p only
constexpr int kTailW = 33;           // the 32 tail columns of a row and a one (db1)

// Xu [rows, ldu]: the columns total .. cap - 1 (the dead slots: never written by the gather) -> 0.  total = cnt[1] clamped into [0, cap].
__global__ __launch_bounds__(256) void field_zero_dead_kernel(float* __restrict__ Xu, int ldu, int rows, const int32_t* __restrict__ cnt, int cap) {
    const int total = min(max(cnt[1], 0), cap);
    const int r = blockIdx.x;
    if (r >= rows) return;
    for (int g = total + threadIdx.x; g < cap; g += 256) Xu[(size_t)r * ldu + g] = 0.f;
}

// Step 1 of  P[j, h] = sum_r Xt[r, j] g1[r, h]  (j < 32)  and  P[32, h] = sum_r g1[r, h]:  workgroup (column block, chunk) sums the rows
// [chunk rper, (chunk + 1) rper) of its 64 columns, four row phases in fixed order -> part [chunk][33][H]
__global__ __launch_bounds__(256) void field_tail_stage1(const float* __restrict__ Xt, const float* __restrict__ g1, int R, int H,
                                                         float* __restrict__ part) {
    __shared__ float red[4][kTailW][64];
    const int lane = threadIdx.x & 63, rs = threadIdx.x >> 6, chunk = blockIdx.y;
    const int col = blockIdx.x * 64 + lane;
    const int rper = (R + kTailChunks - 1) / kTailChunks;
    const int r0 = chunk * rper, r1 = min(R, r0 + rper);
    float acc[kTailW];
#pragma unroll
    for (int j = 0; j < kTailW; ++j) acc[j] = 0.f;
    if (col < H) {
        for (int r = r0 + rs; r < r1; r += 4) {
            const float g = g1[(size_t)r * H + col];
            const float4* x = reinterpret_cast<const float4*>(Xt + (size_t)r * 32);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float4 v = x[j];
                acc[4 * j + 0] += v.x * g; acc[4 * j + 1] += v.y * g; acc[4 * j + 2] += v.z * g; acc[4 * j + 3] += v.w * g;
            }
            acc[32] += g;
        }
    }
#pragma unroll
    for (int j = 0; j < kTailW; ++j) red[rs][j][lane] = acc[j];
    __syncthreads();
    if (rs == 0 && col < H) {
#pragma unroll
        for (int j = 0; j < kTailW; ++j)
            part[((size_t)chunk * kTailW + j) * H + col] = (red[0][j][lane] + red[1][j][lane]) + (red[2][j][lane] + red[3][j][lane]);
    }
}

// Step 2: the chunks in ascending order -> tail [32, H] (the rows from `live` on -- the zero pad of Xt -- are +0.0) and db1 [H]
__global__ __launch_bounds__(256) void field_tail_stage2(const float* __restrict__ part, int H, int live, float* __restrict__ tail,
                                                         float* __restrict__ db1) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= kTailW * H) return;
    const int j = i / H, col = i - j * H;
    float s = 0.f;
    for (int c = 0; c < kTailChunks; ++c) s += part[(size_t)c * kTailW * H + i];
    if (j == 32) db1[col] = s;
    else tail[i] = (j < live) ? s : 0.f;
}

// out = (accumulate ? out : nothing) + the chunk's gradient, for the eight variables in one launch
struct TrainSegs {
    const float* src[8];
    float* dst[8];
    long end[8];      // running end of the segments in the launch's flat index
};
__global__ __launch_bounds__(256) void field_train_store_kernel(TrainSegs S, int accumulate) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= S.end[7]) return;
    int j = 0;
    while (i >= S.end[j]) ++j;      // (i < end[7]: j <= 7)
    const long e = i - (j ? S.end[j - 1] : 0);
    const float v = S.src[j][e];
    S.dst[j][e] = accumulate ? S.dst[j][e] + v : v;
}

namespace {
constexpr size_t al64(size_t floats) { return (floats + 63) / 64 * 64; }

// the workspace in floats: the chunk's eight gradients, the partial sums of the tail product, the scratch of dpd_decoder_bwd_weights
struct TrainWs {
    size_t dW1p, db1, dW2, db2, dW3, db3, dW4, db4, part, scratch, scratch_bytes, bytes;
    TrainWs(int KP, int H) {
        size_t o = 0;
        auto take = [&](size_t floats) { const size_t at = o; o += al64(floats); return at; };
        dW1p = take((size_t)KP * H); db1 = take(H); dW2 = take((size_t)H * H); db2 = take(H); dW3 = take((size_t)H * H); db3 = take(H);
        dW4 = take((size_t)H * 3); db4 = take(3);
        part = take((size_t)kTailChunks * kTailW * H);
        scratch = o;
        // layers 2 and 3: the split-K slabs of the process-wide plan (none by default) and the two-step column sums; layer 4: its sums
        const int split = g_plan_split[OP_BWD_DW23];
        scratch_bytes = (split > 1 ? (size_t)split * H * H * sizeof(float) : 0) + colsum_ws_floats(H, 3) * sizeof(float);
        bytes = (o * sizeof(float) + scratch_bytes + 255) / 256 * 256;
    }
};
}  // namespace

}  // namespace dpd

extern "C" size_t dpd_field_bwd_train_workspace_bytes(int n, int T, int m, int k, int KP, int H) {
    if (n <= 0 || T <= 0 || k <= 0 || H <= 0 || !dpd::field_bwd_cap(n, T, m, k, KP, H)) return 0;
    return dpd::TrainWs(KP, H).bytes;
}

extern "C" int dpd_field_bwd_train(const float* dpred, const float* maskr, const float* y, const float* h1, const float* h2, const float* h3,
                                   const int32_t* cnt, const int32_t* ucount, const int32_t* slot_start, const int32_t* qlist,
                                   const int32_t* slot_vox, const int32_t* slot_cloud, float* Xu, int ldu, const float* Xt, int n, int T, int m,
                                   int k, int KP, int H, int slot_cap, const dpd_decoder_params* p, float* dy, float* ga, float* gb, float* dq,
                                   float* gs, float* dXs, float* dfv, int accumulate, float* gq, long gq_cloud_stride, float* dW1p, float* db1,
                                   float* dW2, float* db2, float* dW3, float* db3, float* dW4, float* db4, int accumulate_w, void* ws,
                                   size_t ws_bytes, void* stream) {
    using namespace dpd;
    float* const outs[8] = {dW1p, db1, dW2, db2, dW3, db3, dW4, db4};
    int given = 0;
    for (float* o : outs) given += o != nullptr;
    if (given == 0)      // no weight gradient wanted: the frozen backward, with its own checks
        return dpd_field_bwd(dpred, maskr, y, h1, h2, h3, cnt, ucount, slot_start, qlist, slot_vox, slot_cloud, n, T, m, k, KP, H, slot_cap, p, dy,
                             ga, gb, dq, gs, dXs, dfv, accumulate, gq, gq_cloud_stride, stream);
    const bool surface = dfv != nullptr, query = gq != nullptr;
    const bool shared = query && gq_cloud_stride == 0;
    if (given != 8) return DPD_E_NULL;
    if (!dpred || !maskr || !y || !h1 || !h2 || !h3 || !cnt || !slot_start || !qlist || !slot_cloud || !p || !dy || !ga || !gb) return DPD_E_NULL;
    if (!Xu || !Xt || !gs || !ws) return DPD_E_NULL;
    if (!p->W2 || !p->W3 || !p->W4 || !p->W1p) return DPD_E_NULL;
    if (surface && (!ucount || !slot_vox || !dXs || !p->W1pT)) return DPD_E_NULL;
    if (shared && !dq) return DPD_E_NULL;
    if (n <= 0 || T <= 0 || slot_cap <= 0 || H <= 0 || k <= 0) return DPD_E_DIM;
    if (query && !shared && gq_cloud_stride < 3L * T) return DPD_E_DIM;
    const int cap = field_bwd_cap(n, T, m, k, KP, H);
    if (!cap) return DPD_E_UNSUPPORTED;
    if (slot_cap != cap || ldu < cap) return DPD_E_DIM;
    if ((ldu & 3) || !fits_gemm_offsets((size_t)(KP - 32), (size_t)ldu)) return DPD_E_UNSUPPORTED;
    const TrainWs w(KP, H);
    if (ws_bytes < w.bytes) return DPD_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    float* f = (float*)ws;
    void* scratch = f + w.scratch;
    const int rows_p = (int)(((long)n * T + 31) / 32 * 32);
    const int E = k * k * k * DPD_FV_CHANNELS;
    auto chain = [&](int phases) {
        return dpd_decoder_bwd_data(dpred, maskr, y, h1, h2, h3, rows_p, KP, H, p, DPD_F32, dy, ga, gb, ga, nullptr, nullptr, nullptr, 0, nullptr,
                                    phases, stream);
    };
    auto layer = [&](int l, const float* act, const float* g, int Nout, float* dW, float* db) {
        return dpd_decoder_bwd_weights(l, act, H, g, rows_p, H, Nout, DPD_F32, dW, db, scratch, w.scratch_bytes, nullptr, nullptr, stream);
    };
    // the data chain of dpd_field_bwd by phases, g3 -> ga, g2 -> gb, g1 -> ga: each layer's weight gradient while its g is alive
    if (int rc = chain(1)) return rc;
    if (int rc = layer(3, h2, ga, H, f + w.dW3, f + w.db3)) return rc;
    if (int rc = layer(4, h3, dy, 3, f + w.dW4, f + w.db4)) return rc;
    if (int rc = chain(2)) return rc;
    if (int rc = layer(2, h1, gb, H, f + w.dW2, f + w.db2)) return rc;
    if (int rc = chain(4)) return rc;
    // gs, the query route, the surface route: the launches of dpd_field_bwd
    if (int rc = field_routes(ga, cnt, ucount, slot_start, qlist, slot_vox, slot_cloud, n, T, m, k, KP, H, cap, p, dq, gs, dXs, dfv, accumulate, gq,
                              gq_cloud_stride, true, stream))
        return rc;
    {   // layer 1 over the rows: the 32 tail columns and db1
        StageProf prof(stream, DPD_STAGE_SMALL_REDUCE, (double)rows_p * (H + 32) * 4.0 + 2.0 * kTailChunks * kTailW * H * 4.0);
        DPD_LAUNCH(field_tail_stage1, dim3((H + 63) / 64, kTailChunks), dim3(256), 0, s, Xt, (const float*)ga, rows_p, H, f + w.part);
        DPD_CHECK_LAUNCH();
        DPD_LAUNCH(field_tail_stage2, dim3((kTailW * H + 255) / 256), dim3(256), 0, s, (const float*)(f + w.part), H, E + 3 - (KP - 32),
                   f + w.dW1p + (size_t)(KP - 32) * H, f + w.db1);
        DPD_CHECK_LAUNCH();
    }
    {   // layer 1 over the slots: the dead columns of Xu hold whatever the buffer held
        StageProf prof(stream, DPD_STAGE_WEIGHT_COPIES, (double)(KP - 32) * (cap / 2) * 4.0);
        DPD_LAUNCH(field_zero_dead_kernel, dim3(KP - 32), dim3(256), 0, s, Xu, ldu, KP - 32, cnt, cap);
        DPD_CHECK_LAUNCH();
    }
    GemmF32Call g;
    g.M = KP - 32; g.N = H; g.K = cap;
    g.A = Xu; g.lda = ldu; g.B = gs; g.ldb = H; g.C = f + w.dW1p; g.ldc = H;
    g.epilogue = EPI_NONE; g.split_k = 1; g.tile = 32; g.s = s;
    if (int rc = gemm_f32(g)) return rc;
    TrainSegs S;
    const size_t at[8] = {w.dW1p, w.db1, w.dW2, w.db2, w.dW3, w.db3, w.dW4, w.db4};
    const long cnts[8] = {(long)KP * H, H, (long)H * H, H, (long)H * H, H, 3L * H, 3};
    long end = 0;
    for (int i = 0; i < 8; ++i) {
        S.src[i] = f + at[i]; S.dst[i] = outs[i];
        S.end[i] = end += cnts[i];
    }
    StageProf prof(stream, DPD_STAGE_WEIGHT_COPIES, (double)end * (accumulate_w ? 12.0 : 8.0));
    DPD_LAUNCH(field_train_store_kernel, dim3((unsigned)((end + 255) / 256)), dim3(256), 0, s, S, accumulate_w);
    DPD_CHECK_LAUNCH();
    return 0;
}

// Output layer of the implicit-surface decoder (decoder.hip): y = h3 W4 + b4, pred = relu6(y) / 3 * mask.  Its forward plain, as a loss
// and for paired clouds, its backward in three forms, and the small gradients (db3, dW4, db4) that come out of the same pass.
// Every kernel that evaluates the layer is in this unit and takes the row dot product from out_row_dot.  (out_fwd_kernel stays beside
// the kernels that pass `keep`: alone in a unit its out_row_dot is specialised before inlining and the kernel's code changes.)
#include "decoder_int.h"

namespace dpd {

// ---- output layer: y = h3 W4 + b4 ; pred = clip(y,0,6)/3 * mask.  One wave per row. ----------------------
// the three dot products of one row with W4 [H,3] (one wave; every lane returns the full sums): ONE definition, so that every
// kernel that evaluates the output layer produces the same bits
// (H % 256 == 0, H <= 1024, W4 16-byte aligned: 16-byte loads of the row AND of W4 -- the 12 floats W4[k..k+3][0..2] are three float4 --
// and the loaded row / column 0 of W4 stay in registers for a caller that goes on to the backward; same additions in the same order)
constexpr int kOutMaxI = 4;
struct OutRowRegs {
    float4 h[kOutMaxI];
    float w0[kOutMaxI][4];
};
__device__ __forceinline__ bool out_row_fast(const float* W4, int H) { return (H & 255) == 0 && H <= 256 * kOutMaxI && !((uintptr_t)W4 & 15); }

__device__ __forceinline__ void out_row_dot(const float* __restrict__ h, const float* __restrict__ W4, int H, int lane, float (&a)[3],
                                            OutRowRegs* keep = nullptr) {
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    if (out_row_fast(W4, H)) {
#pragma unroll
        for (int i = 0; i < kOutMaxI; ++i) {
            const int k = 4 * lane + 256 * i;
            if (k < H) {
                const float4 x = *reinterpret_cast<const float4*>(h + k);
                const float4* wp = reinterpret_cast<const float4*>(W4 + (size_t)k * 3);
                const float4 wa = wp[0], wb = wp[1], wc = wp[2];
                a0 += x.x * wa.x; a1 += x.x * wa.y; a2 += x.x * wa.z;
                a0 += x.y * wa.w; a1 += x.y * wb.x; a2 += x.y * wb.y;
                a0 += x.z * wb.z; a1 += x.z * wb.w; a2 += x.z * wc.x;
                a0 += x.w * wc.y; a1 += x.w * wc.z; a2 += x.w * wc.w;
                if (keep) { keep->h[i] = x; keep->w0[i][0] = wa.x; keep->w0[i][1] = wa.w; keep->w0[i][2] = wb.z; keep->w0[i][3] = wc.y; }
            }
        }
    } else if ((H & 255) == 0) {          // 16 bytes per lane per load: H / 256 loads in flight instead of H / 64 dependent-address ones
        for (int k = 4 * lane; k < H; k += 256) {
            const float4 x = *reinterpret_cast<const float4*>(h + k);
            const float xs[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                a0 += xs[e] * W4[(k + e) * 3 + 0];
                a1 += xs[e] * W4[(k + e) * 3 + 1];
                a2 += xs[e] * W4[(k + e) * 3 + 2];
            }
        }
    } else {
        for (int k = lane; k < H; k += 64) {
            const float x = h[k];
            a0 += x * W4[k * 3 + 0];
            a1 += x * W4[k * 3 + 1];
            a2 += x * W4[k * 3 + 2];
        }
    }
    a[0] = wave_sum(a0); a[1] = wave_sum(a1); a[2] = wave_sum(a2);
}

__global__ __launch_bounds__(256) void out_fwd_kernel(const float* __restrict__ h3, const float* __restrict__ W4,
                                                       const float* __restrict__ b4, const float* __restrict__ mask,
                                                       float* __restrict__ y, float* __restrict__ pred, int Q, int H) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= Q) return;
    float a[3];
    out_row_dot(h3 + (size_t)row * H, W4, H, lane, a);
    if (lane < 3) {
        const float v = (lane == 0 ? a[0] : (lane == 1 ? a[1] : a[2])) + b4[lane];
        y[(size_t)row * 3 + lane] = v;
        pred[(size_t)row * 3 + lane] = fminf(fmaxf(v, 0.f), 6.f) / 3.0f * mask[row];   // relu6(y)/3 (:691) * mask (:697)
    }
}

// DPDist as a frozen loss (pcrnet-registration/iterative_PCRNet_ours.py:229-257): output layer, loss_pred and -- when g3 != NULL -- the
// output-layer backward of d loss_pred / d pred (= gv = 0.5 / BN on channel 0 of every row, models/dpdist_and_aue.py:976-977) in ONE
// launch instead of three (out_fwd + l1_loss + out_bwd: ~5 us each at the PCRNet batch, all launch-latency bound).  One wave per row.
// Same values as the three-kernel chain (loss_pred within an ulp: exact fixed-point sum instead of fp32 partial sums): y / pred through
// out_row_dot, dy = (gv * mask / 3 * [0 < y0 < 6], 0, 0), g3 = dy0 * W4[:,0] * [h3 > 0] (the chain adds two exact zeros to that).
template <int RW>      // rows per wave
__global__ __launch_bounds__(256) void out_asloss_kernel(const float* __restrict__ h3, const float* __restrict__ W4,
                                                          const float* __restrict__ b4, const float* __restrict__ mask,
                                                          float* __restrict__ y, float* __restrict__ pred, float* __restrict__ dy,
                                                          float* __restrict__ g3, int Q, int H, int BN, float gv,
                                                          float* __restrict__ loss, unsigned long long* __restrict__ acc,
                                                          uint16_t* __restrict__ g3_rc, long g3_plane, int g3_np) {
    // g3_rc (round 5, the as-loss engine of the plane compute types): g3 leaves this kernel as the RC operand plane(s) of the first dH GEMM
    // -- the same split as split_planes_kernel, which this saves (one launch and the fp32 round trip of g3; g3 itself may then be NULL)
    __shared__ float s_p[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float p0 = 0.f;
#pragma unroll 1
    for (int rw = 0; rw < RW; ++rw) {
        const int row = (blockIdx.x * 4 + wave) * RW + rw;
        if (row >= Q) break;
        const float* h = h3 + (size_t)row * H;
        float a[3];
        OutRowRegs rr;
        out_row_dot(h, W4, H, lane, a, &rr);
        const float mk = mask[row];
        float yv[3], pv[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            yv[c] = a[c] + b4[c];
            pv[c] = fminf(fmaxf(yv[c], 0.f), 6.f) / 3.0f * mk;
        }
        if (lane < 3) {
            y[(size_t)row * 3 + lane] = lane == 0 ? yv[0] : (lane == 1 ? yv[1] : yv[2]);
            pred[(size_t)row * 3 + lane] = lane == 0 ? pv[0] : (lane == 1 ? pv[1] : pv[2]);
        }
        p0 += pv[0];
        if (dy) {
            const float d0 = (yv[0] > 0.f && yv[0] < 6.f) ? gv * mk / 3.0f : 0.f;
            if (lane < 3) dy[(size_t)row * 3 + lane] = lane == 0 ? d0 : 0.f;
            float* g = g3 ? g3 + (size_t)row * H : nullptr;
            if (out_row_fast(W4, H)) {
#pragma unroll
                for (int i = 0; i < kOutMaxI; ++i) {
                    const int k = 4 * lane + 256 * i;
                    if (k < H) {
                        const float4 x = rr.h[i];
                        float4 o;
                        o.x = x.x > 0.f ? d0 * rr.w0[i][0] : 0.f;
                        o.y = x.y > 0.f ? d0 * rr.w0[i][1] : 0.f;
                        o.z = x.z > 0.f ? d0 * rr.w0[i][2] : 0.f;
                        o.w = x.w > 0.f ? d0 * rr.w0[i][3] : 0.f;
                        if (g) *reinterpret_cast<float4*>(g + k) = o;
                        if (g3_rc) {
                            const float ov[4] = {o.x, o.y, o.z, o.w};
                            unsigned pl4[4][3];
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                if (g3_np == 1) { pl4[e][0] = bf16_bits(ov[e]); pl4[e][1] = 0; pl4[e][2] = 0; }
                                else split3(ov[e], pl4[e]);
                            }
#pragma unroll
                            for (int q = 0; q < 3; ++q)
                                if (q < g3_np)
                                    *reinterpret_cast<uint2*>(g3_rc + q * g3_plane + (size_t)row * H + k) =
                                        make_uint2(pl4[0][q] | (pl4[1][q] << 16), pl4[2][q] | (pl4[3][q] << 16));
                        }
                    }
                }
            } else if (g) {
                for (int k = lane; k < H; k += 64) g[k] = h[k] > 0.f ? d0 * W4[k * 3] : 0.f;
            }
        }
    }
    // loss_pred = sum over ALL rows of pred[:,0] / (2 BN).  The sum is taken in 2^-32 fixed point: integer addition is associative, so
    // the blocks can add their part in any order with ONE relaxed device-scope atomic each and still produce the same bits on every run;
    // the block count rides in the top 16 bits of the same word, so the block that completes it needs no fence and no second look at
    // memory (a __threadfence() per block costs an L2 write-back on this chip: this kernel took 23 us with a ticket + fence, ~6 without)
    if (lane == 0) s_p[wave] = p0;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long part = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) part += (unsigned long long)__double2ll_rn((double)s_p[w] * 4294967296.0);   // pred >= 0
        const unsigned long long add = part + (1ull << 48);
        const unsigned long long old = atomicAdd(acc, add);
        if ((old >> 48) + 1 == (unsigned long long)gridDim.x) {
            const unsigned long long total = (old + add) & ((1ull << 48) - 1);
            loss[0] = (float)((double)total * (1.0 / 4294967296.0) / (2.0 * (double)BN));      // (:976-977)
            atomicExch(acc, 0ull);                                                               // ready for the next launch
        }
    }
}

// dy = dpred * mask * [0 < y < 6] / 3 ;  g3 = (dy W4^T) * [h3 > 0].  One wave per row.
struct ZeroList {   // small accumulators cleared by the first kernel of the backward chain (saves memset launches)
    float* p[5];
    int n[5];
};

__global__ __launch_bounds__(256) void out_bwd_kernel(const float* __restrict__ dpred, const float* __restrict__ mask,
                                                       const float* __restrict__ y, const float* __restrict__ h3,
                                                       const float* __restrict__ W4, float* __restrict__ dy,
                                                       float* __restrict__ g3, int Qb, int H, ZeroList zl) {
    if (blockIdx.x < 5 && zl.p[blockIdx.x]) {
        for (int i = threadIdx.x; i < zl.n[blockIdx.x]; i += 256) zl.p[blockIdx.x][i] = 0.f;
    }
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= Qb) return;
    float d[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float yv = y[(size_t)row * 3 + c];
        d[c] = (yv > 0.f && yv < 6.f) ? dpred[(size_t)row * 3 + c] * mask[row] / 3.0f : 0.f;   // relu6 gradient is 1 on (0,6)
    }
    if (lane < 3) dy[(size_t)row * 3 + lane] = d[lane];
    const float* h = h3 + (size_t)row * H;
    float* g = g3 + (size_t)row * H;
    for (int k = lane; k < H; k += 64) {
        const float v = d[0] * W4[k * 3] + d[1] * W4[k * 3 + 1] + d[2] * W4[k * 3 + 2];
        g[k] = (h[k] > 0.f) ? v : 0.f;
    }
}

// Fused output-layer backward: ONE pass over h3 produces dy, g3 AND the per-block partial sums of
//   db3 = colsum(g3), dW4 = h3^T dy, db4 = colsum(dy)
// (block = 32 rows, 4 waves x 8 rows; lane owns columns lane+64j).  Partials go to `scratch` [nblk][4H+4] and are
// summed in fixed order by small_grads_reduce -> deterministic, no atomics, no memset.  H <= 1024.
constexpr int kOBRows = 8;
constexpr int kOBMaxJ = 16;

__global__ __launch_bounds__(256) void out_bwd_fused_kernel(const float* __restrict__ dpred, const float* __restrict__ mask,
                                                             const float* __restrict__ y, const float* __restrict__ h3,
                                                             const float* __restrict__ W4, float* __restrict__ dy,
                                                             float* __restrict__ g3, int Qb, int H, ZeroList zl,
                                                             float* __restrict__ scratch) {
    extern __shared__ float s_acc[];   // [4H + 4]
    if (blockIdx.x < 5 && zl.p[blockIdx.x]) {
        for (int i = threadIdx.x; i < zl.n[blockIdx.x]; i += 256) zl.p[blockIdx.x][i] = 0.f;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nj = H / 64;
    float w4[kOBMaxJ][3], s3[kOBMaxJ], a4[kOBMaxJ][3];
#pragma unroll
    for (int j = 0; j < kOBMaxJ; ++j) {
        s3[j] = 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) { a4[j][c] = 0.f; w4[j][c] = (j < nj) ? W4[(lane + 64 * j) * 3 + c] : 0.f; }
    }
    float dsum[3] = {0.f, 0.f, 0.f};
    for (int rr = 0; rr < kOBRows / 4; ++rr) {
        const int row = blockIdx.x * kOBRows + wave * (kOBRows / 4) + rr;
        if (row >= Qb) break;
        float d[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float yv = y[(size_t)row * 3 + c];
            d[c] = (yv > 0.f && yv < 6.f) ? dpred[(size_t)row * 3 + c] * mask[row] / 3.0f : 0.f;   // relu6 gradient is 1 on (0,6)
            dsum[c] += d[c];
        }
        if (lane < 3) dy[(size_t)row * 3 + lane] = d[lane];
        const float* h = h3 + (size_t)row * H;
        float* g = g3 + (size_t)row * H;
#pragma unroll
        for (int j = 0; j < kOBMaxJ; ++j) {
            if (j < nj) {
                const int k = lane + 64 * j;
                const float hv = h[k];
                const float v = d[0] * w4[j][0] + d[1] * w4[j][1] + d[2] * w4[j][2];
                const float gv = (hv > 0.f) ? v : 0.f;
                g[k] = gv;
                s3[j] += gv;
#pragma unroll
                for (int c = 0; c < 3; ++c) a4[j][c] += hv * d[c];
            }
        }
    }
    // fixed-order reduction over the 4 waves
    for (int w = 0; w < 4; ++w) {
        if (wave == w) {
#pragma unroll
            for (int j = 0; j < kOBMaxJ; ++j) {
                if (j < nj) {
                    const int k = lane + 64 * j;
                    if (w == 0) {
                        s_acc[k] = s3[j];
#pragma unroll
                        for (int c = 0; c < 3; ++c) s_acc[H + k * 3 + c] = a4[j][c];
                    } else {
                        s_acc[k] += s3[j];
#pragma unroll
                        for (int c = 0; c < 3; ++c) s_acc[H + k * 3 + c] += a4[j][c];
                    }
                }
            }
            if (lane < 3) {
                const float v = (lane == 0) ? dsum[0] : ((lane == 1) ? dsum[1] : dsum[2]);
                if (w == 0) s_acc[4 * H + lane] = v;
                else s_acc[4 * H + lane] += v;
            }
        }
        __syncthreads();
    }
    float* out = scratch + (size_t)blockIdx.x * (4 * H + 4);
    for (int i = threadIdx.x; i < 4 * H + 3; i += 256) out[i] = s_acc[i];
}

// Same contract as out_bwd_fused_kernel for H % 256 == 0, H <= 1024: a lane owns 4 consecutive columns in each
// 256-column group (float4 loads/stores, both rows of a wave in flight together) and the four waves' partials are
// combined with ONE barrier (each wave has its own LDS slab).  LDS: 4 * (4H + 4) floats.
// L1: optional fused loss (training mode, utils/dpdist_util.py:962-980): with l1.labels the kernel derives
// d loss_samples / d pred_AB = sign(pred_AB[:,0] - labels) * gscale / Qb itself (dpred is not read) and adds the three loss sums
// (sum |pred_AB - labels|, sum pred_AB, sum pred_BA over its rows) to the block record [4H+4 .. 4H+6].
struct L1Fuse {
    const float* pred;     // [2*Qb, 3]
    const float* labels;   // [Qb]
    float gscale;
};
constexpr int kOBRec = 8;   // record = 4H + 8 floats: db3 [H] | dW4 [3H] | db4 [3] | pad | loss sums [3] | pad
// Optional bf16 operand planes of g3 written by the same pass (plane compute types: no fp32 g3, no conversion launch): RC
// [np][Qb][H] straight from the registers, R8 [np][Qb/8][H][8] through an LDS image of the block's 8 rows (behind the four slabs).
struct G3Planes {
    uint16_t* rc;
    uint16_t* r8;
    long plane;     // elements per plane (Qb * H)
    int np;
};
// Optional forward of the output layer inside the same pass (training step: no out_fwd launch, h3 rows of the AB half are read
// once): with y != NULL the kernel computes y = h3 W4 + b4 and pred = relu6(y)/3 * mask for its AB rows AND their BA twins
// (row + Qb), in out_fwd_kernel's summation order (bit-identical), writes both, and uses them instead of the y / l1.pred inputs.
struct OutFwd {
    const float* b4;
    float* y;       // [2*Qb, 3]
    float* pred;    // [2*Qb, 3]
};

__global__ __launch_bounds__(256) void out_bwd_fused4_kernel(const float* __restrict__ dpred, const float* __restrict__ mask,
                                                              const float* __restrict__ y, const float* __restrict__ h3,
                                                              const float* __restrict__ W4, float* __restrict__ dy,
                                                              float* __restrict__ g3, int Qb, int H, ZeroList zl,
                                                              float* __restrict__ scratch, L1Fuse l1, OutFwd of, G3Planes gp,
                                                              const uint16_t* __restrict__ h3b) {
    extern __shared__ float s_acc[];   // [4 waves][4H + 8]; reused at the end (gp.r8) as uint16 [np][8][H]
    if (blockIdx.x < 5 && zl.p[blockIdx.x]) {
        for (int i = threadIdx.x; i < zl.n[blockIdx.x]; i += 256) zl.p[blockIdx.x][i] = 0.f;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ng = H / 256;            // column groups (<= 4)
    const int P = 4 * H + kOBRec;
    constexpr int RW = kOBRows / 4;    // rows per wave
    float lsum[3] = {0.f, 0.f, 0.f};   // loss sums of this wave's rows (identical in every lane)
    float dsum[3] = {0.f, 0.f, 0.f};
    float d[RW][3];
    float4 hv[RW][4], hb[RW][4];
    const int row0 = blockIdx.x * kOBRows + wave * RW;
    // Every global load of the kernel is requested HERE, before anything waits: W4 above, the rows (and their BA twins) and the per-row
    // scalars below.  Left where they were used, they made three dependent round trips (W4 -> row 0 -> row 1: 5.5k + 3.9k + 5.7k cycles
    // of a 25k-cycle kernel at B = 32, s_memtime stamps); with one workgroup per CU there is nothing else to hide them behind.
    static_assert(RW == 2, "the lane-pair exchanges below assume two rows per wave");
    const bool odd = lane & 1;
    // exchange a 64-bit value with lane ^ 1 (DPP quad_perm [1,0,3,2])
    auto swap_pair = [](uint2 v) {
        return make_uint2((unsigned)__builtin_amdgcn_mov_dpp((int)v.x, 0xB1, 0xf, 0xf, true), (unsigned)__builtin_amdgcn_mov_dpp((int)v.y, 0xB1, 0xf, 0xf, true));
    };
    auto widen = [](uint2 u) {
        return make_float4(__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u), __uint_as_float(u.y << 16), __uint_as_float(u.y & 0xffff0000u));
    };
    if (h3b) {
        // layer 3's activation as one bf16 plane (DPD_BF16), widened exactly.  A lane's four columns of one row are 8 bytes, and 8-byte
        // accesses run at ~0.6 of the 16-byte rate (round 5: this load phase was 12k of the kernel's 37k cycles at B = 64): the lanes
        // 2p / 2p + 1 therefore load 16 bytes -- the eight columns of BOTH lanes -- of row 0 / row 1 and hand each other the half that
        // belongs to the partner.  Same values in the same registers as two 8-byte loads per lane.
        const int rsel = min(row0 + (odd ? 1 : 0), Qb - 1);
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            if (jj < ng) {
                const uint4 va = *reinterpret_cast<const uint4*>(h3b + (size_t)rsel * H + 256 * jj + 8 * (lane >> 1));
                const uint2 ra = swap_pair(odd ? make_uint2(va.x, va.y) : make_uint2(va.z, va.w));
                hv[0][jj] = widen(odd ? ra : make_uint2(va.x, va.y));
                hv[1][jj] = widen(odd ? make_uint2(va.z, va.w) : ra);
                if (of.y) {
                    const uint4 vb = *reinterpret_cast<const uint4*>(h3b + ((size_t)Qb + rsel) * H + 256 * jj + 8 * (lane >> 1));
                    const uint2 rb = swap_pair(odd ? make_uint2(vb.x, vb.y) : make_uint2(vb.z, vb.w));
                    hb[0][jj] = widen(odd ? rb : make_uint2(vb.x, vb.y));
                    hb[1][jj] = widen(odd ? make_uint2(vb.z, vb.w) : rb);
                }
            }
        }
    } else {
#pragma unroll
        for (int rr = 0; rr < RW; ++rr) {
            const int row = min(row0 + rr, Qb - 1);
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                if (jj < ng) {
                    hv[rr][jj] = *reinterpret_cast<const float4*>(h3 + (size_t)row * H + 256 * jj + 4 * lane);
                    if (of.y) hb[rr][jj] = *reinterpret_cast<const float4*>(h3 + ((size_t)Qb + row) * H + 256 * jj + 4 * lane);
                }
            }
        }
    }
    float w4[4][4][3], s3[4][4], a4[4][4][3];
    const bool w4_vec = !((uintptr_t)W4 & 15);       // the 12 floats W4[k..k+3][0..2] of a lane's four columns are three float4 (k % 4 == 0)
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
        if (w4_vec && jj < ng) {      // 12 loads per lane instead of 48: the address unit was ~6k of this kernel's 24k cycles at B = 32
            const float4* wp = reinterpret_cast<const float4*>(W4 + (size_t)(256 * jj + 4 * lane) * 3);
            const float4 wa = wp[0], wb = wp[1], wc = wp[2];
            const float w[12] = {wa.x, wa.y, wa.z, wa.w, wb.x, wb.y, wb.z, wb.w, wc.x, wc.y, wc.z, wc.w};
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int c = 0; c < 3; ++c) w4[jj][e][c] = w[3 * e + c];
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            s3[jj][e] = 0.f;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                a4[jj][e][c] = 0.f;
                if (!(w4_vec && jj < ng)) w4[jj][e][c] = (jj < ng) ? W4[(256 * jj + 4 * lane + e) * 3 + c] : 0.f;
            }
        }
    }
    // the per-row scalars are requested before the row loop: behind the dot products and wave sums they were one more dependent round trip
    float mk_a[RW], mk_b[RW], lab[RW];
#pragma unroll
    for (int rr = 0; rr < RW; ++rr) {
        const int row = min(row0 + rr, Qb - 1);
        mk_a[rr] = mask[row];
        mk_b[rr] = of.y ? mask[Qb + row] : 0.f;
        lab[rr] = l1.labels ? l1.labels[row] : 0.f;
    }
#pragma unroll
    for (int rr = 0; rr < RW; ++rr) {
        const int row = min(row0 + rr, Qb - 1);
        const bool live = row0 + rr < Qb;
        float yab[3] = {0.f, 0.f, 0.f}, pab0 = 0.f, pba0 = 0.f;
        if (of.y) {                // forward of the output layer for this AB row and its BA twin (out_fwd_kernel's order)
            float a[3] = {0.f, 0.f, 0.f}, b[3] = {0.f, 0.f, 0.f};
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                if (jj < ng) {
                    const float xa[4] = {hv[rr][jj].x, hv[rr][jj].y, hv[rr][jj].z, hv[rr][jj].w};
                    const float xb[4] = {hb[rr][jj].x, hb[rr][jj].y, hb[rr][jj].z, hb[rr][jj].w};
#pragma unroll
                    for (int e = 0; e < 4; ++e)
#pragma unroll
                        for (int c = 0; c < 3; ++c) { a[c] += xa[e] * w4[jj][e][c]; b[c] += xb[e] * w4[jj][e][c]; }
                }
            }
            // empty asm = a schedule fence: row 0's dot products finish before its wave sums start (the instruction order this kernel
            // was measured with; without it the compiler interleaves the two)
            if (rr == 0) asm volatile("" :: "v"(a[0]), "v"(b[2]));
            float yba[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) { yab[c] = wave_sum(a[c]) + of.b4[c]; yba[c] = wave_sum(b[c]) + of.b4[c]; }
            const float ma = mk_a[rr], mb = mk_b[rr];
            float pa[3], pb[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                pa[c] = fminf(fmaxf(yab[c], 0.f), 6.f) / 3.0f * ma;   // relu6(y)/3 (:691) * mask (:697)
                pb[c] = fminf(fmaxf(yba[c], 0.f), 6.f) / 3.0f * mb;
            }
            pab0 = pa[0]; pba0 = pb[0];
            if (live && lane < 3) {
                const float ya = lane == 0 ? yab[0] : (lane == 1 ? yab[1] : yab[2]), yb = lane == 0 ? yba[0] : (lane == 1 ? yba[1] : yba[2]);
                const float qa = lane == 0 ? pa[0] : (lane == 1 ? pa[1] : pa[2]), qb = lane == 0 ? pb[0] : (lane == 1 ? pb[1] : pb[2]);
                of.y[(size_t)row * 3 + lane] = ya; of.y[((size_t)Qb + row) * 3 + lane] = yb;
                of.pred[(size_t)row * 3 + lane] = qa; of.pred[((size_t)Qb + row) * 3 + lane] = qb;
            }
        }
        float dp[3];
        if (l1.labels) {           // d mean|pred_AB[:,0] - labels| / d pred_AB (tf.abs gradient = sign), channels 1, 2 get none
            const float pab = of.y ? pab0 : l1.pred[(size_t)row * 3], pba = of.y ? pba0 : l1.pred[((size_t)Qb + row) * 3];
            const float df = pab - lab[rr];
            dp[0] = ((df > 0.f) ? 1.f : ((df < 0.f) ? -1.f : 0.f)) * (1.0f / (float)Qb) * l1.gscale;
            dp[1] = 0.f; dp[2] = 0.f;
            if (live) { lsum[0] += fabsf(df); lsum[1] += pab; lsum[2] += pba; }
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) dp[c] = dpred[(size_t)row * 3 + c];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float yv = of.y ? yab[c] : y[(size_t)row * 3 + c];
            d[rr][c] = (live && yv > 0.f && yv < 6.f) ? dp[c] * mk_a[rr] / 3.0f : 0.f;   // relu6' = 1 on (0,6)
            dsum[c] += d[rr][c];
        }
    }
    uint2 wpk[RW][4][3] = {};
#pragma unroll
    for (int rr = 0; rr < RW; ++rr) {
        const int row = row0 + rr;
        if (row >= Qb) break;
        if (lane < 3) dy[(size_t)row * 3 + lane] = d[rr][lane];
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            if (jj < ng) {
                const float hh[4] = {hv[rr][jj].x, hv[rr][jj].y, hv[rr][jj].z, hv[rr][jj].w};
                float gg[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float v = d[rr][0] * w4[jj][e][0] + d[rr][1] * w4[jj][e][1] + d[rr][2] * w4[jj][e][2];
                    gg[e] = (hh[e] > 0.f) ? v : 0.f;
                    s3[jj][e] += gg[e];
#pragma unroll
                    for (int c = 0; c < 3; ++c) a4[jj][e][c] += hh[e] * d[rr][c];
                }
                if (g3) *reinterpret_cast<float4*>(g3 + (size_t)row * H + 256 * jj + 4 * lane) = make_float4(gg[0], gg[1], gg[2], gg[3]);
                if (gp.rc || gp.r8) {
                    unsigned pl4[4][3];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        if (gp.np == 1) { pl4[e][0] = bf16_bits(gg[e]); pl4[e][1] = 0; pl4[e][2] = 0; }     // one plane: one conversion, not the three-plane split
                        else split3(gg[e], pl4[e]);
                    }
                    const int col = 256 * jj + 4 * lane;
#pragma unroll
                    for (int q = 0; q < 3; ++q) {
                        const uint2 w = make_uint2(pl4[0][q] | (pl4[1][q] << 16), pl4[2][q] | (pl4[3][q] << 16));
                        wpk[rr][jj][q] = w;      // kept in registers: the LDS image for the R8 chunks reuses the slabs once they are summed
                    }
                    (void)col;
                }
            }
        }
    }
    if (gp.rc) {
        // RC planes: lane 2p stores the eight columns of lanes 2p / 2p + 1 of row 0, lane 2p + 1 those of row 1 -- one 16-byte store per
        // lane, column group and plane instead of two 8-byte ones (the planes exist only for whole 8-row blocks: both rows are valid)
        uint16_t* rcp = gp.rc + (size_t)(row0 + (odd ? 1 : 0)) * H + 8 * (lane >> 1);
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            if (jj < ng) {
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    if (q < gp.np) {
                        const uint2 got = swap_pair(odd ? wpk[0][jj][q] : wpk[1][jj][q]);
                        const uint2 lo = odd ? got : wpk[0][jj][q], hi = odd ? wpk[1][jj][q] : got;
                        *reinterpret_cast<uint4*>(rcp + q * gp.plane + 256 * jj) = make_uint4(lo.x, lo.y, hi.x, hi.y);
                    }
                }
            }
        }
    }
    float* mine = s_acc + wave * P;
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
        if (jj < ng) {
            const int k = 256 * jj + 4 * lane;          // four columns: 4 + 12 contiguous floats, 16-byte aligned (H % 256 == 0, P % 4 == 0)
            *reinterpret_cast<float4*>(mine + k) = make_float4(s3[jj][0], s3[jj][1], s3[jj][2], s3[jj][3]);
            float4* m4 = reinterpret_cast<float4*>(mine + H + k * 3);
            m4[0] = make_float4(a4[jj][0][0], a4[jj][0][1], a4[jj][0][2], a4[jj][1][0]);
            m4[1] = make_float4(a4[jj][1][1], a4[jj][1][2], a4[jj][2][0], a4[jj][2][1]);
            m4[2] = make_float4(a4[jj][2][2], a4[jj][3][0], a4[jj][3][1], a4[jj][3][2]);
        }
    }
    if (lane < 3) mine[4 * H + lane] = (lane == 0) ? dsum[0] : ((lane == 1) ? dsum[1] : dsum[2]);
    if (lane < 3) mine[4 * H + 4 + lane] = (lane == 0) ? lsum[0] : ((lane == 1) ? lsum[1] : lsum[2]);
    if (lane == 3) { mine[4 * H + 3] = 0.f; mine[4 * H + 7] = 0.f; }
    __syncthreads();
    float* out = scratch + (size_t)blockIdx.x * P;
    for (int i = threadIdx.x; i < 4 * H + 7; i += 256) out[i] = ((s_acc[i] + s_acc[P + i]) + s_acc[2 * P + i]) + s_acc[3 * P + i];
    if (gp.r8) {      // the block's 8 rows = one row group: column c's chunk = its 8 rows (Qb % 8 == 0 when planes are in use)
        uint16_t* s_g = reinterpret_cast<uint16_t*>(s_acc);      // [np][8][H] <= 48 KiB: inside the four slabs, which are summed by now
        __syncthreads();
#pragma unroll
        for (int rr = 0; rr < RW; ++rr)
#pragma unroll
            for (int jj = 0; jj < 4; ++jj)
                if (jj < ng)
                    for (int q = 0; q < gp.np; ++q)
                        *reinterpret_cast<uint2*>(s_g + ((size_t)(q * kOBRows + wave * RW + rr) * H + 256 * jj + 4 * lane)) = wpk[rr][jj][q < 3 ? q : 0];
        __syncthreads();
        for (int c = threadIdx.x; c < H; c += 256)
            for (int q = 0; q < gp.np; ++q) {
                unsigned b[8];
#pragma unroll
                for (int rr = 0; rr < 8; ++rr) b[rr] = s_g[(size_t)(q * kOBRows + rr) * H + c];
                *reinterpret_cast<uint4*>(gp.r8 + q * gp.plane + ((size_t)blockIdx.x * H + c) * 8) =
                    make_uint4(b[0] | (b[1] << 16), b[2] | (b[3] << 16), b[4] | (b[5] << 16), b[6] | (b[7] << 16));
            }
    }
}

// out[i] = sum_b scratch[b][i] in a fixed order: 16 outputs x 16 block-slices per workgroup, LDS tree at the end
// rec = floats per block record (4H + 4, or 4H + 8 when the record carries the three loss sums at [4H+4 .. 4H+6]); loss (may be
// NULL) then receives loss_samples = sum|pred_AB - labels| / Qb and loss_pred = (sum pred_AB / Qb + sum pred_BA / Qb) / 2.
__global__ __launch_bounds__(256) void small_grads_reduce(const float* __restrict__ scratch, int nblk, int H,
                                                           float* __restrict__ db3, float* __restrict__ dW4,
                                                           float* __restrict__ db4, int rec, float* __restrict__ loss, int Qb) {
    __shared__ float red[16][17];
    __shared__ float s_loss[3];
    const int li = threadIdx.x & 15, sl = threadIdx.x >> 4;
    const int i = blockIdx.x * 16 + li;
    const int n = (rec > 4 * H + 4 && loss) ? 4 * H + 7 : 4 * H + 3;
    float s = 0.f;
    if (i < n)
        for (int b = sl; b < nblk; b += 16) s += scratch[(size_t)b * rec + i];
    red[sl][li] = s;
    __syncthreads();
    if (sl == 0 && i < n) {
        float t = 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) t += red[k][li];
        if (i < H) { if (db3) db3[i] = t; }
        else if (i < 4 * H) { if (dW4) dW4[i - H] = t; }
        else if (i < 4 * H + 3) { if (db4) db4[i - 4 * H] = t; }
        else if (i >= 4 * H + 4) s_loss[i - 4 * H - 4] = t;       // the three loss sums land in ONE workgroup (16 outputs each)
    }
    if (n > 4 * H + 3 && blockIdx.x == (4 * H + 4) / 16) {
        __syncthreads();
        if (threadIdx.x == 0) {
            const float inv = 1.0f / (float)Qb;
            loss[0] = s_loss[0] * inv;
            loss[1] = (s_loss[1] * inv + s_loss[2] * inv) / 2.0f;
        }
    }
}

// Column sums in ONE launch (the two-stage form is decoder_bwd.hip's colsum_stage1 / colsum_stage2; NW as there): every (column block,
// row chunk) adds its partial with one atomic per output element (output must be zero on entry).  Used for db3 and dW4/db4 behind the
// unfused output-layer backward.
template <int NW>
__global__ __launch_bounds__(256) void colsum_atomic(const float* __restrict__ a, int lda, const float* __restrict__ w,
                                                      int R, int Ncols, float* __restrict__ out, float* __restrict__ wsum) {
    constexpr int W = NW ? NW : 1;
    __shared__ float red[4][64 * W];
    const int col = blockIdx.x * 64 + (threadIdx.x & 63), rs = threadIdx.x >> 6, chunk = blockIdx.y;
    const int rper = (R + gridDim.y - 1) / gridDim.y;
    const int r0 = chunk * rper, r1 = min(R, r0 + rper);
    float acc[W];
#pragma unroll
    for (int c = 0; c < W; ++c) acc[c] = 0.f;
    if (col < Ncols) {
        for (int r = r0 + rs; r < r1; r += 4) {
            const float x = a[(size_t)r * lda + col];
            if (NW == 0) acc[0] += x;
            else {
#pragma unroll
                for (int c = 0; c < NW; ++c) acc[c] += x * w[(size_t)r * NW + c];
            }
        }
    }
#pragma unroll
    for (int c = 0; c < W; ++c) red[rs][(threadIdx.x & 63) * W + c] = acc[c];
    __syncthreads();
    if (rs == 0 && col < Ncols) {
#pragma unroll
        for (int c = 0; c < W; ++c) {
            const int i = (threadIdx.x & 63) * W + c;
            atomicAdd(out + (size_t)col * W + c, (red[0][i] + red[1][i]) + (red[2][i] + red[3][i]));
        }
    }
    if (NW && wsum && blockIdx.x == 0) {   // column sums of w itself (db4 = colsum(dy)), one block column does it
        float s[W];
#pragma unroll
        for (int c = 0; c < W; ++c) s[c] = 0.f;
        for (int r = r0 + threadIdx.x; r < r1; r += 256)
#pragma unroll
            for (int c = 0; c < W; ++c) s[c] += w[(size_t)r * NW + c];
#pragma unroll
        for (int c = 0; c < W; ++c) {
            s[c] = wave_sum(s[c]);
            if ((threadIdx.x & 63) == 0) atomicAdd(wsum + c, s[c]);
        }
    }
}
// Paired distances of clouds of different sizes (dpd_decoder_out_pairs).  Row layout of P pairs: the AB half first (row b Wb + n: query
// B_b[n], Wb rows per pair, real while n < countsB[b]), then the BA half at P Wb (row P Wb + b Wa + n: query A_b[n], real while
// n < countsA[b]).  A segment = one (direction, pair): its rows are contiguous, its length is the query set's width, and neither its
// start nor its length is aligned with anything (widths like 37, 5, 1; the two halves differ).
struct PairSeg {
    int b, n, cnt;      // pair, query index inside the segment, the segment's real queries (clamped into [1, width])
    long row0;          // first row of the segment
};
__device__ __forceinline__ int pair_count(const int32_t* __restrict__ counts, int b, int W) { return counts ? min(max(counts[b], 1), W) : W; }
__device__ __forceinline__ PairSeg pair_seg_of_row(long row, int P, int Wa, int Wb, const int32_t* __restrict__ cA,
                                                   const int32_t* __restrict__ cB) {
    const long nab = (long)P * Wb;
    const bool ba = row >= nab;
    const long rr = ba ? row - nab : row;
    const int W = ba ? Wa : Wb;
    PairSeg s;
    s.b = (int)(rr / W);
    s.n = (int)(rr - (long)s.b * W);
    s.cnt = pair_count(ba ? cA : cB, s.b, W);
    s.row0 = row - s.n;
    return s;
}

// One wave per row: y / pred through out_row_dot (the bits of out_fwd_kernel), and -- with dy -- the output-layer backward of
// sum_b (D_AB[b] + D_BA[b]): unit upstream per directed distance, 1 / count of the row's own segment on channel 0, as out_asloss_kernel
// forms it.  The row of a padded query (n >= count) is written as +0.0 in dy and g3, whatever the sign of W4.
__global__ __launch_bounds__(256) void out_pairs_kernel(const float* __restrict__ h3, const float* __restrict__ W4,
                                                         const float* __restrict__ b4, const float* __restrict__ mask,
                                                         float* __restrict__ y, float* __restrict__ pred, float* __restrict__ dy,
                                                         float* __restrict__ g3, int P, int Wa, int Wb, const int32_t* __restrict__ cA,
                                                         const int32_t* __restrict__ cB, int H) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (long)P * ((long)Wa + Wb)) return;
    const float* h = h3 + (size_t)row * H;
    float a[3];
    OutRowRegs rr;
    out_row_dot(h, W4, H, lane, a, &rr);
    const float mk = mask[row];
    float yv[3], pv[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        yv[c] = a[c] + b4[c];
        pv[c] = fminf(fmaxf(yv[c], 0.f), 6.f) / 3.0f * mk;
    }
    if (lane < 3) {
        y[(size_t)row * 3 + lane] = lane == 0 ? yv[0] : (lane == 1 ? yv[1] : yv[2]);
        pred[(size_t)row * 3 + lane] = lane == 0 ? pv[0] : (lane == 1 ? pv[1] : pv[2]);
    }
    if (!dy) return;
    const PairSeg sg = pair_seg_of_row(row, P, Wa, Wb, cA, cB);
    const bool real = sg.n < sg.cnt;
    const float d0 = (real && yv[0] > 0.f && yv[0] < 6.f) ? (1.0f / (float)sg.cnt) * mk / 3.0f : 0.f;
    if (lane < 3) dy[(size_t)row * 3 + lane] = lane == 0 ? d0 : 0.f;
    float* g = g3 + (size_t)row * H;
    if (out_row_fast(W4, H)) {
#pragma unroll
        for (int i = 0; i < kOutMaxI; ++i) {
            const int k = 4 * lane + 256 * i;
            if (k < H) {
                const float4 x = rr.h[i];
                float4 o;
                o.x = (real && x.x > 0.f) ? d0 * rr.w0[i][0] : 0.f;
                o.y = (real && x.y > 0.f) ? d0 * rr.w0[i][1] : 0.f;
                o.z = (real && x.z > 0.f) ? d0 * rr.w0[i][2] : 0.f;
                o.w = (real && x.w > 0.f) ? d0 * rr.w0[i][3] : 0.f;
                *reinterpret_cast<float4*>(g + k) = o;
            }
        }
    } else {
        for (int k = lane; k < H; k += 64) g[k] = (real && h[k] > 0.f) ? d0 * W4[k * 3] : 0.f;
    }
}

// Dd [2, P]: one workgroup per segment.  Thread t adds pred[:, 0] of the segment's real rows t, t + 256, ... in 2^-32 fixed point
// (pred lies in [0, 2]: at most 2^33 per row), the 256 partial sums are added in a tree through LDS: integer addition, so the sum is
// exact, the same on every run and independent of what else the launch holds.  One rounding to double, one division, one to float.
__global__ __launch_bounds__(256) void pairs_mean_kernel(const float* __restrict__ pred, int P, int Wa, int Wb,
                                                          const int32_t* __restrict__ cA, const int32_t* __restrict__ cB,
                                                          float* __restrict__ Dd) {
    __shared__ unsigned long long s_part[256];
    const int ba = blockIdx.x >= (unsigned)P, b = ba ? blockIdx.x - P : blockIdx.x;
    const int W = ba ? Wa : Wb;
    const int cnt = pair_count(ba ? cA : cB, b, W);
    const float* src = pred + ((size_t)(ba ? (long)P * Wb : 0L) + (size_t)b * W) * 3;
    unsigned long long acc = 0;
    for (int n = threadIdx.x; n < cnt; n += 256) acc += (unsigned long long)__double2ll_rn((double)src[(size_t)n * 3] * 4294967296.0);
    s_part[threadIdx.x] = acc;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) s_part[threadIdx.x] += s_part[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x == 0) Dd[blockIdx.x] = (float)((double)s_part[0] * (1.0 / 4294967296.0) / (double)cnt);
}

int out_layer_fwd(const float* h3, const dpd_decoder_params* p, const float* mask, float* y, float* pred, int Q, int H, hipStream_t s) {
    DPD_LAUNCH(out_fwd_kernel, dim3((Q + 3) / 4), dim3(256), 0, s, h3, p->W4, p->b4, mask, y, pred, Q, H);
    DPD_CHECK_LAUNCH();
    return 0;
}

// ---- output-layer step of dpd_decoder_bwd_data_live (phases 1, 8, 16) ----
// the fused kernel for H % 256 == 0, H <= 1024; *g3_planes: g3 left it as operand planes
static int launch_out_bwd_fused4(const BwdData& b, int nblk, int rec, const ZeroList& zl, float* part, const L1Fuse& lf, const OutFwd& ofw,
                                 bool* g3_planes) {
    const int Qb = b.Qb, H = b.H;
    const dpd_planes* pl = b.pl;
    // plane compute types: g3 leaves this kernel as the operand planes of the first dH GEMM (RC) and of dW3 (R8)
    G3Planes gpl{nullptr, nullptr, (long)Qb * H, pl ? pl->np : 0};
    if (pl && !(Qb % kOBRows)) { gpl.rc = (uint16_t*)pl->g3_rc; gpl.r8 = (uint16_t*)pl->g3_r8; }
    *g3_planes = gpl.rc || gpl.r8;
    const size_t lds = (size_t)4 * rec * sizeof(float);      // (the R8 image of g3, np * 8 * H * 2 bytes, reuses the slabs)
    static LdsOptIn lds_opt;
    if (int rc = ensure_dyn_lds(lds_opt, (const void*)out_bwd_fused4_kernel, lds)) return rc;
    // algorithmic bytes: layer 3's activation in (the Qb gradient rows, and their Qb twins when the layer's forward runs here
    // too; fp32 or one bf16 plane), g3 out (fp32 or both operand planes), the block partials, mask / labels / y / pred
    const double h3_b = b.h3 ? 4.0 : 2.0;
    StageProf prof(b.s, DPD_STAGE_OUT_LAYER,
                   (double)Qb * H * h3_b * (ofw.y ? 2.0 : 1.0) + (b.g3 ? (double)Qb * H * 4.0 : 0.0) +
                       ((gpl.rc ? 1.0 : 0.0) + (gpl.r8 ? 1.0 : 0.0)) * gpl.np * 2.0 * Qb * H + (double)nblk * rec * 4.0 + Qb * 40.0 + H * 12.0);
    DPD_LAUNCH(out_bwd_fused4_kernel, dim3(nblk), dim3(256), lds, b.s, b.dpred, b.mask, b.y, b.h3, b.p->W4, b.dy, b.g3, Qb, H, zl, part, lf, ofw, gpl,
               b.h3 ? nullptr : (const uint16_t*)pl->h3_rc);
    return 0;
}

int out_layer_bwd(const BwdData& b, bool* g3_planes) {
    const int Qb = b.Qb, H = b.H, phases = b.phases;
    const dpd_small_grads* sg = b.sg;
    const dpd_planes* pl = b.pl;
    hipStream_t s = b.s;
    const bool l1 = sg && sg->l1_labels;        // fused training loss: dpred is derived inside the output-layer kernel
    float* db1 = sg ? sg->db1 : nullptr;
    float* db2 = sg ? sg->db2 : nullptr;
    float* db3 = sg ? sg->db3 : nullptr;
    float* dW4 = sg ? sg->dW4 : nullptr;
    float* db4 = sg ? sg->db4 : nullptr;
    const int nblk = (Qb + kOBRows - 1) / kOBRows;
    const bool fused4 = H % 256 == 0 && H <= 1024;
    const int rec = fused4 ? 4 * H + kOBRec : 4 * H + 4;          // floats per block record
    const bool fused = (db3 || dW4 || db4 || l1) && H <= 64 * kOBMaxJ && (size_t)nblk * rec <= (size_t)Qb * H;
    if (l1 && !(fused && fused4)) return DPD_E_UNSUPPORTED;       // the caller then uses dpd_l1_loss + dpred
    if ((phases & 1) && b.h3_plane && !(fused && fused4 && pl)) return DPD_E_UNSUPPORTED;
    const L1Fuse lf{l1 ? sg->l1_pred : nullptr, l1 ? sg->l1_labels : nullptr, l1 ? sg->l1_gscale : 1.0f};
    const bool ofwd = sg && (sg->fwd_y || sg->fwd_pred) && (phases & 1);   // output layer's forward inside the same pass (training step)
    if (ofwd && !(l1 && fused4 && sg->fwd_y && sg->fwd_pred && b.p->b4)) return DPD_E_UNSUPPORTED;
    const OutFwd ofw{ofwd ? b.p->b4 : nullptr, ofwd ? sg->fwd_y : nullptr, ofwd ? sg->fwd_pred : nullptr};
    float* lossp = l1 ? sg->l1_loss : nullptr;
    const int nred = (4 * H + 7 + 15) / 16;
    // block partials of db3 / dW4 / db4: by default in g2 (free until the first dH GEMM); a caller that defers their reduction
    // (phases 16 / 8: it then runs beside the dH GEMMs on another stream) must provide sg->partials
    float* part = (sg && sg->partials) ? sg->partials : b.g2;
    if ((phases & 24) && !(sg && sg->partials)) return DPD_E_NULL;
    // g3 = NULL: only when the fused output-layer kernel writes g3 as operand planes itself (plane compute types, below)
    // (phases without 1 and no fp32 g3: dpd_decoder_out_asloss_planes has left g3 as the RC plane the first dH GEMM reads)
    if (!b.g3 && !(pl && pl->g3_rc && ((pl->g3_r8 && fused && fused4 && !(Qb % kOBRows)) || !(phases & 1)))) return DPD_E_NULL;
    if ((phases & 8) && fused) {   // deferred second stage of the small gradients (a side stream / graph branch runs it)
        DPD_LAUNCH(small_grads_reduce, dim3(nred), dim3(256), 0, s, (const float*)part, nblk, H, db3, dW4, db4, rec, lossp, Qb);
        DPD_CHECK_LAUNCH();
    }
    if (!(phases & 1)) return 0;      // output layer already done by an earlier call
    if (fused) {
        // one pass over h3: dy, g3 and block partials of db3 / dW4 / db4 (g2 is free until the first dH GEMM: scratch)
        ZeroList zl{{db1, db2, nullptr, nullptr, nullptr}, {H, H, 0, 0, 0}};
        if (fused4) {
            if (int rc = launch_out_bwd_fused4(b, nblk, rec, zl, part, lf, ofw, g3_planes)) return rc;
        } else {
            DPD_LAUNCH(out_bwd_fused_kernel, dim3(nblk), dim3(256), (size_t)(4 * H + 4) * sizeof(float), s, b.dpred, b.mask, b.y, b.h3,
                       b.p->W4, b.dy, b.g3, Qb, H, zl, part);
        }
        DPD_CHECK_LAUNCH();
        if (!(phases & 16)) {   // 16: the block partials stay in the scratch (= g2, which must not be overwritten before phase 8 ran)
            StageProf prof(s, DPD_STAGE_SMALL_REDUCE, (double)nblk * rec * 4.0 + (4.0 * H + 3) * 4.0);
            DPD_LAUNCH(small_grads_reduce, dim3(nred), dim3(256), 0, s, (const float*)part, nblk, H, db3, dW4, db4, rec, lossp, Qb);
            DPD_CHECK_LAUNCH();
        }
        return 0;
    }
    ZeroList zl{{db1, db2, db3, dW4, db4}, {H, H, H, H * 3, 3}};
    DPD_LAUNCH(out_bwd_kernel, dim3((Qb + 3) / 4), dim3(256), 0, s, b.dpred, b.mask, b.y, b.h3, b.p->W4, b.dy, b.g3, Qb, H, zl);
    DPD_CHECK_LAUNCH();
    const int chunks = 16;
    if (db3) {   // db3 = colsum(g3)
        DPD_LAUNCH(colsum_atomic<0>, dim3((H + 63) / 64, chunks), dim3(256), 0, s, (const float*)b.g3, H, (const float*)nullptr, Qb,
                   H, db3, (float*)nullptr);
        DPD_CHECK_LAUNCH();
    }
    if (dW4) {   // dW4 = h3^T dy, db4 = colsum(dy)
        DPD_LAUNCH(colsum_atomic<3>, dim3((H + 63) / 64, chunks), dim3(256), 0, s, b.h3, H, (const float*)b.dy, Qb, H, dW4, db4);
        DPD_CHECK_LAUNCH();
    }
    return 0;
}

}  // namespace dpd

extern "C" int dpd_decoder_out_asloss(const float* h3, const float* mask, int Q, int H, int BN, const dpd_decoder_params* p, float gscale,
                                      float* y, float* pred, float* loss_pred, float* dy, float* g3, float* scratch, void* stream) {
    return dpd_decoder_out_asloss_planes(h3, mask, Q, H, BN, p, gscale, y, pred, loss_pred, dy, g3, nullptr, scratch, stream);
}

extern "C" int dpd_decoder_out_asloss_planes(const float* h3, const float* mask, int Q, int H, int BN, const dpd_decoder_params* p, float gscale,
                                             float* y, float* pred, float* loss_pred, float* dy, float* g3, const dpd_planes* pl, float* scratch,
                                             void* stream) {
    using namespace dpd;
    if (!h3 || !mask || !p || !p->W4 || !p->b4 || !y || !pred || !loss_pred || !scratch) return DPD_E_NULL;
    // pl with g3_rc (and dy given): g3 also (or, with g3 == NULL, only) as RC operand plane(s); needs the 16-byte fast path of the row kernel
    uint16_t* g3_rc = (pl && dy) ? (uint16_t*)pl->g3_rc : nullptr;
    if (g3_rc && (pl->Qb != Q || (pl->np != 1 && pl->np != 3) || (H & 255) || H > 256 * kOutMaxI || ((uintptr_t)p->W4 & 15) || ((uintptr_t)h3 & 15)))
        return DPD_E_UNSUPPORTED;
    if (dy && !g3 && !g3_rc) return DPD_E_NULL;
    if (!dy && g3) return DPD_E_NULL;
    if (Q <= 0 || H <= 0 || BN <= 0 || Q != 2 * BN) return DPD_E_DIM;
    if ((H & 3) || ((uintptr_t)scratch & 7) || Q > 8 * 65535 || BN >= (1 << 14)) return DPD_E_UNSUPPORTED;   // 16-bit block count; 48-bit sum: Q rows x at most 2.0 x 2^32 must stay below 2^48
    const float gv = 0.5f * (1.0f / (float)BN) * gscale;      // = l1_loss_kernel mode 2
    // two rows per wave: 9.9 us against 11.2 (one) and 11.9 (four) at the PCRNet batch -- the kernel is a chain of round trips (rows and
    // W4 -> wave sums -> stores -> the atomic's return), not a throughput problem
    DPD_LAUNCH(out_asloss_kernel<2>, dim3((Q + 7) / 8), dim3(256), 0, (hipStream_t)stream, h3, p->W4, p->b4, mask, y, pred, dy, g3, Q, H, BN, gv,
               loss_pred, (unsigned long long*)scratch, g3_rc, g3_rc ? (long)Q * H : 0L, g3_rc ? pl->np : 0);
    DPD_CHECK_LAUNCH();
    return 0;
}

extern "C" int dpd_decoder_out_pairs(const float* h3, const float* mask, int P, int Wa, int Wb, const int32_t* countsA, const int32_t* countsB,
                                     int H, const dpd_decoder_params* p, float* y, float* pred, float* Dd, float* dy, float* g3, void* stream) {
    using namespace dpd;
    if (!h3 || !mask || !p || !p->W4 || !p->b4 || !y || !pred || !Dd || (!dy != !g3)) return DPD_E_NULL;
    if (P <= 0 || Wa <= 0 || Wb <= 0 || H <= 0 || (long)P * ((long)Wa + Wb) > (1L << 30)) return DPD_E_DIM;
    if (((uintptr_t)h3 & 15) || ((uintptr_t)g3 & 15)) return DPD_E_UNSUPPORTED;      // the rows are read and written 16 bytes per lane
    hipStream_t s = (hipStream_t)stream;
    const long Q = (long)P * ((long)Wa + Wb);
    {
        StageProf prof(stream, DPD_STAGE_OUT_LAYER, (double)Q * H * 4.0 * (g3 ? 2.0 : 1.0) + Q * (dy ? 40.0 : 28.0) + H * 12.0);
        DPD_LAUNCH(out_pairs_kernel, dim3((unsigned)((Q + 3) / 4)), dim3(256), 0, s, h3, p->W4, p->b4, mask, y, pred, dy, g3, P, Wa, Wb, countsA,
                   countsB, H);
        DPD_CHECK_LAUNCH();
    }
    StageProf prof(stream, DPD_STAGE_SMALL_REDUCE, (double)Q * 12.0 + P * 8.0);
    DPD_LAUNCH(pairs_mean_kernel, dim3(2 * P), dim3(256), 0, s, (const float*)pred, P, Wa, Wb, countsA, countsB, Dd);
    DPD_CHECK_LAUNCH();
    return 0;
}

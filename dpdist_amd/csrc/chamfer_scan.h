// The nearest-neighbour scan of the paired Chamfer losses of chamfer.hip (squared form, AUE task; square-rooted form, PCRNet's baseline):
// both forms store the same minima and indices because both launch the one min kernel around this body.  Below it, what the counted
// kernels of chamfer_matrix.hip and chamfer_pairs.hip share.  The count clamp of a ragged set is ragged_count (common.h).
#pragma once
#include "common.h"

namespace dpd {

// |x - y|^2 of one pair: reduce_sum over the 3 coordinates, in order (train_multi_gpu_pc_compare_dist.py:905); not fused
__device__ __forceinline__ float chamfer_pair_sq(float px, float py, float pz, const float* __restrict__ y) {
    const float dx = px - y[0], dy = py - y[1], dz = pz - y[2];
    return (dx * dx + dy * dy) + dz * dz;
}

// Body of a 256-thread workgroup of grid B * (chunks_a + chunks_b): mins[b][i] = min_j |x_bi - y_bj|^2, arg[b][i] = that j (the lowest on
// ties).  dir 0: x = a (N points), y = b (M); dir 1: x = b, y = a.  s_y: max(N, M) * 3 floats of LDS.
__device__ __forceinline__ void chamfer_min_scan(const float* __restrict__ a, const float* __restrict__ b, int N, int M,
                                                 float* __restrict__ min_a, int32_t* __restrict__ arg_a, float* __restrict__ min_b,
                                                 int32_t* __restrict__ arg_b, int chunks_a, int chunks_b, float* __restrict__ s_y) {
    const int per = chunks_a + chunks_b;
    const int c = blockIdx.x / per, r = blockIdx.x % per;
    const bool dir = r >= chunks_a;
    const int chunk = dir ? r - chunks_a : r;
    const int nx = dir ? M : N, ny = dir ? N : M;
    const float* x = (dir ? b : a) + (size_t)c * nx * 3;
    const float* y = (dir ? a : b) + (size_t)c * ny * 3;
    for (int e = threadIdx.x; e < ny * 3; e += 256) s_y[e] = y[e];
    __syncthreads();
    const int i = chunk * 256 + threadIdx.x;
    if (i >= nx) return;
    const float px = x[i * 3], py = x[i * 3 + 1], pz = x[i * 3 + 2];
    float best = INFINITY;
    int bj = 0;
    for (int j = 0; j < ny; ++j) {
        const float d = chamfer_pair_sq(px, py, pz, s_y + j * 3);
        if (d < best) { best = d; bj = j; }
    }
    (dir ? min_b : min_a)[(size_t)c * nx + i] = best;
    (dir ? arg_b : arg_a)[(size_t)c * nx + i] = bj;
}

// What the counted kernels share: chamfer_matrix.hip (one workgroup owns a surface cloud and walks query clouds past it) and
// chamfer_pairs.hip (a workgroup takes 256 queries of one pair) clamp, stage, scan and differentiate with these bodies, so a pair gets the
// same bits from either.
constexpr int kCmMaxPoints = 4096;     // the cap of every Chamfer entry: the surface cloud lives in LDS
constexpr int kCmMaxGrid = 1 << 20;    // workgroups per launch; the kernels stride over their units beyond it

__device__ __forceinline__ void cm_stage(float* __restrict__ s_y, const float* __restrict__ y, int ny) {
    for (int e = threadIdx.x; e < ny * 3; e += blockDim.x) s_y[e] = y[e];
}

// best[r] = min_p |q_r - s_p|^2 over the ny staged points, arg[r] = the lowest such p (ARG).  A minimum does not depend on the visiting
// order; the argmin takes the first strict improvement of an ascending walk.
template <int R, bool ARG>
__device__ __forceinline__ void cm_scan(const float* __restrict__ s_y, int ny, const float (&q)[R][3], float (&best)[R], int (&arg)[R]) {
#pragma unroll
    for (int r = 0; r < R; ++r) { best[r] = INFINITY; arg[r] = 0; }
    int p = 0;
    for (; p + 4 <= ny; p += 4) {
        const float4* v = reinterpret_cast<const float4*>(s_y + p * 3);
        const float4 a = v[0], b = v[1], c = v[2];
        const float y[12] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const float d = chamfer_pair_sq(q[r][0], q[r][1], q[r][2], y + k * 3);
                if (ARG) {
                    if (d < best[r]) { best[r] = d; arg[r] = p + k; }
                } else {
                    best[r] = fminf(best[r], d);
                }
            }
        }
    }
    for (; p < ny; ++p) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const float d = chamfer_pair_sq(q[r][0], q[r][1], q[r][2], s_y + p * 3);
            if (ARG) {
                if (d < best[r]) { best[r] = d; arg[r] = p; }
            } else {
                best[r] = fminf(best[r], d);
            }
        }
    }
}

// max over the 64 lanes of NON-NEGATIVE values (a lane without a DPP source reads 0), returned in every lane
__device__ __forceinline__ float cm_wave_max(float v) {
    v = fmaxf(v, dpp_move<0xB1>(v));
    v = fmaxf(v, dpp_move<0x4E>(v));
    v = fmaxf(v, dpp_move<0x141>(v));
    v = fmaxf(v, dpp_move<0x140>(v));
    v = fmaxf(v, dpp_move<0x142, 0xA>(v));
    v = fmaxf(v, dpp_move<0x143, 0xC>(v));
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}

// one term of a gradient: w * t(x, y) added to g.  Squared form: t = 2 (x - y); square-rooted form: t = (x - y) / |x - y| with the
// hardware reciprocal square root of d2 = |x - y|^2, and exactly nothing where d2 is 0 (the deviation of dpd_chamfer_sqrt_bwd).
template <int FORM>
__device__ __forceinline__ void cm_term(float w, float d2, float xx, float xy, float xz, const float* __restrict__ y, float (&g)[3]) {
    float s;
    if (FORM == 0) {
        s = 2.f;
    } else {
        if (!(d2 > 0.f)) return;
        s = rsqrtf(d2);   // v_rsq_f32, with the input scaled where d2 is subnormal
    }
    g[0] += w * (s * (xx - y[0]));
    g[1] += w * (s * (xy - y[1]));
    g[2] += w * (s * (xz - y[2]));
}

}  // namespace dpd

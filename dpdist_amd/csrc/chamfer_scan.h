// The nearest-neighbour scan of the Chamfer losses, shared by chamfer.hip (squared form, AUE task) and regtest.hip (square-rooted form,
// PCRNet's baseline): both store the same minima and indices, bit for bit, because both run this one body.
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

}  // namespace dpd

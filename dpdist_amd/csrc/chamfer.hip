// Chamfer distance between two point sets, both paired forms:
//   squared (dpd_chamfer_fwd / _bwd)            the baseline loss of the AUE task, SURVEY section 8 row f4
//   square-rooted (dpd_chamfer_sqrt_fwd / _bwd) PCRNet's --loss_type chamf (utils/tf_util_loss.py:35-39), the registration baseline
//
// Replaces pairwise_diff + chmafer_dist (train_multi_gpu_pc_compare_dist.py:891-916):
//     d(x, y)[b, i, j] = |x_bi - y_bj|^2                                      (:896-905, squared, no sqrt)
//     loss = ( mean_bi r(min_j d(rec, pc)) + mean_bj r(min_i d(pc, rec)) ) / 2  (:913-915; r = identity, or sqrt for the rooted form)
// without materialising the [B, N, 3, M] tiles of the reference.  One workgroup per (cloud, direction, 256-point
// chunk): the other cloud is staged in LDS, every thread scans it for its own point.  Tiny and latency bound
// (N = M = 64 ... 2048); algorithmic HBM bytes = 12 (N + M) read + 8 (N + M) written per cloud.
// Ties in the minimum (measure zero for float clouds) go to the lowest index; tf.reduce_min would split the
// gradient evenly among them.
// Both forms run ONE min kernel (the scan of chamfer_scan.h), one loss kernel and one gradient kernel templated on the form, and one
// host forward / backward; a form keeps its own arithmetic (chamfer_term below), which is NOT cm_term of the counted kernels.
#include "common.h"
#include "chamfer_scan.h"

namespace dpd {

// mins[b][i] = min_j |x_bi - y_bj|^2, arg[b][i] = that j.  dir 0: x = a (N points), y = b (M); dir 1: x = b, y = a.
__global__ __launch_bounds__(256) void chamfer_min_kernel(const float* __restrict__ a, const float* __restrict__ b, int N, int M,
                                                          float* __restrict__ min_a, int32_t* __restrict__ arg_a,
                                                          float* __restrict__ min_b, int32_t* __restrict__ arg_b, int chunks_a,
                                                          int chunks_b) {
    extern __shared__ float s_y[];   // [ny][3]
    chamfer_min_scan(a, b, N, M, min_a, arg_a, min_b, arg_b, chunks_a, chunks_b, s_y);
}

// loss = (mean(r(min_a)) + mean(r(min_b))) / 2, r = sqrt for the rooted form; fixed summation order (one workgroup)
template <bool ROOT>
__global__ __launch_bounds__(256) void chamfer_loss_kernel(const float* __restrict__ min_a, long na, const float* __restrict__ min_b,
                                                           long nb, float* __restrict__ loss) {
    __shared__ float red[2][256];
    float sa = 0.f, sb = 0.f;
    for (long i = threadIdx.x; i < na; i += 256) sa += ROOT ? sqrtf(min_a[i]) : min_a[i];
    for (long i = threadIdx.x; i < nb; i += 256) sb += ROOT ? sqrtf(min_b[i]) : min_b[i];
    red[0][threadIdx.x] = sa;
    red[1][threadIdx.x] = sb;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) {
            red[0][threadIdx.x] += red[0][threadIdx.x + o];
            red[1][threadIdx.x] += red[1][threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[0] = (red[0][0] / (float)na + red[1][0] / (float)nb) / 2.0f;
}

// One term w t(x, y) of the gradient of the point (px, py, pz); FIRST: the query route, which opens the sum.
//   squared  t = 2 (x - y).  The query route is ASSIGNED, not added to 0: 0 + t would turn a -0.0 term (a coincident pair under a
//            negative gscale, an underflowing product) into +0.0.
//   rooted   t = (x - y) / |x - y| with the IEEE square root and division, added to a sum that starts at 0; a coincident pair
//            contributes exactly nothing (the reference: inf * 0 = NaN).  d is the stored minimum, recomputed: the same bits.
template <bool ROOT, bool FIRST>
__device__ __forceinline__ void chamfer_term(float w, float px, float py, float pz, const float* __restrict__ y, float& gx, float& gy,
                                             float& gz) {
    if (ROOT) {
        if (FIRST) gx = gy = gz = 0.f;
        const float d = chamfer_pair_sq(px, py, pz, y);
        if (d > 0.f) {
            const float s = w / sqrtf(d);
            gx += s * (px - y[0]);
            gy += s * (py - y[1]);
            gz += s * (pz - y[2]);
        }
    } else {
        const float tx = w * 2.f * (px - y[0]), ty = w * 2.f * (py - y[1]), tz = w * 2.f * (pz - y[2]);
        if (FIRST) {
            gx = tx, gy = ty, gz = tz;
        } else {
            gx += tx, gy += ty, gz += tz;
        }
    }
}

// Gradient w.r.t. x (dir 0: a, dir 1: b) as a gather (deterministic, no atomics):
//   dx_i = g * [ wx t(x_i, y_arg_x[i])  +  wy * sum_{j : arg_y[j] == i} t(x_i, y_j) ],  wx = 1/(2 B nx), wy = 1/(2 B ny),
// the hits in ascending j.
template <bool ROOT>
__global__ __launch_bounds__(256) void chamfer_grad_kernel(const float* __restrict__ a, const float* __restrict__ b, int N, int M,
                                                           const int32_t* __restrict__ arg_a, const int32_t* __restrict__ arg_b,
                                                           float gscale, int B, float* __restrict__ da, float* __restrict__ db,
                                                           int chunks_a, int chunks_b) {
    extern __shared__ float s_buf[];   // [ny][3] then [ny] arg (as int)
    const int per = chunks_a + chunks_b;
    const int c = blockIdx.x / per, r = blockIdx.x % per;
    const bool dir = r >= chunks_a;
    const int chunk = dir ? r - chunks_a : r;
    const int nx = dir ? M : N, ny = dir ? N : M;
    float* dx = dir ? db : da;
    if (!dx) return;
    const float* x = (dir ? b : a) + (size_t)c * nx * 3;
    const float* y = (dir ? a : b) + (size_t)c * ny * 3;
    const int32_t* arg_x = (dir ? arg_b : arg_a) + (size_t)c * nx;
    const int32_t* arg_y = (dir ? arg_a : arg_b) + (size_t)c * ny;
    float* s_y = s_buf;
    int* s_arg = reinterpret_cast<int*>(s_buf + ny * 3);
    for (int e = threadIdx.x; e < ny * 3; e += 256) s_y[e] = y[e];
    for (int e = threadIdx.x; e < ny; e += 256) s_arg[e] = arg_y[e];
    __syncthreads();
    const int i = chunk * 256 + threadIdx.x;
    if (i >= nx) return;
    const float wx = gscale / (2.0f * (float)B * (float)nx), wy = gscale / (2.0f * (float)B * (float)ny);
    const float px = x[i * 3], py = x[i * 3 + 1], pz = x[i * 3 + 2];
    const int j0 = min(max(arg_x[i], 0), ny - 1);        // (an index the forward wrote; the clamp keeps a foreign one inside LDS)
    float gx, gy, gz;
    chamfer_term<ROOT, true>(wx, px, py, pz, s_y + j0 * 3, gx, gy, gz);
    for (int j = 0; j < ny; ++j)
        if (s_arg[j] == i) chamfer_term<ROOT, false>(wy, px, py, pz, s_y + j * 3, gx, gy, gz);
    dx[((size_t)c * nx + i) * 3] = gx;
    dx[((size_t)c * nx + i) * 3 + 1] = gy;
    dx[((size_t)c * nx + i) * 3 + 2] = gz;
}

// the argument checks of the four entries, and the grid: B * (chunks of a + chunks of b) workgroups of 256
static int chamfer_check(int B, int N, int M) {
    if (B <= 0 || N <= 0 || M <= 0) return DPD_E_DIM;
    if (N > kCmMaxPoints || M > kCmMaxPoints) return DPD_E_UNSUPPORTED;   // the other cloud lives in LDS (48 KB, 64 KB with its argmins)
    return 0;
}

template <bool ROOT>
static int chamfer_fwd(const float* a, const float* b, int B, int N, int M, float* min_a, int32_t* arg_a, float* min_b, int32_t* arg_b,
                       float* loss, hipStream_t s) {
    if (!a || !b || !min_a || !arg_a || !min_b || !arg_b || !loss) return DPD_E_NULL;
    if (const int rc = chamfer_check(B, N, M)) return rc;
    const int ca = (N + 255) / 256, cb = (M + 255) / 256;
    const size_t lds = (size_t)(N > M ? N : M) * 3 * sizeof(float);
    DPD_LAUNCH(chamfer_min_kernel, dim3(B * (ca + cb)), dim3(256), lds, s, a, b, N, M, min_a, arg_a, min_b, arg_b, ca, cb);
    DPD_CHECK_LAUNCH();
    DPD_LAUNCH(chamfer_loss_kernel<ROOT>, dim3(1), dim3(256), 0, s, (const float*)min_a, (long)B * N, (const float*)min_b, (long)B * M,
               loss);
    DPD_CHECK_LAUNCH();
    return 0;
}

template <bool ROOT>
static int chamfer_bwd(const float* a, const float* b, int B, int N, int M, const int32_t* arg_a, const int32_t* arg_b, float gscale,
                       float* da, float* db, hipStream_t s) {
    if (!a || !b || !arg_a || !arg_b || (!da && !db)) return DPD_E_NULL;
    if (const int rc = chamfer_check(B, N, M)) return rc;
    const int ca = (N + 255) / 256, cb = (M + 255) / 256;
    const size_t lds = (size_t)(N > M ? N : M) * 4 * sizeof(float);
    DPD_LAUNCH(chamfer_grad_kernel<ROOT>, dim3(B * (ca + cb)), dim3(256), lds, s, a, b, N, M, arg_a, arg_b, gscale, B, da, db, ca, cb);
    DPD_CHECK_LAUNCH();
    return 0;
}

}  // namespace dpd

extern "C" int dpd_chamfer_fwd(const float* a, const float* b, int B, int N, int M, float* min_a, int32_t* arg_a, float* min_b,
                               int32_t* arg_b, float* loss, void* stream) {
    return dpd::chamfer_fwd<false>(a, b, B, N, M, min_a, arg_a, min_b, arg_b, loss, (hipStream_t)stream);
}

extern "C" int dpd_chamfer_bwd(const float* a, const float* b, int B, int N, int M, const int32_t* arg_a, const int32_t* arg_b,
                               float gscale, float* da, float* db, void* stream) {
    return dpd::chamfer_bwd<false>(a, b, B, N, M, arg_a, arg_b, gscale, da, db, (hipStream_t)stream);
}

extern "C" int dpd_chamfer_sqrt_fwd(const float* a, const float* b, int B, int N, int M, float* min_a, int32_t* arg_a, float* min_b,
                                    int32_t* arg_b, float* loss, void* stream) {
    return dpd::chamfer_fwd<true>(a, b, B, N, M, min_a, arg_a, min_b, arg_b, loss, (hipStream_t)stream);
}

extern "C" int dpd_chamfer_sqrt_bwd(const float* a, const float* b, int B, int N, int M, const int32_t* arg_a, const int32_t* arg_b,
                                    float gscale, float* da, float* db, void* stream) {
    return dpd::chamfer_bwd<true>(a, b, B, N, M, arg_a, arg_b, gscale, da, db, (hipStream_t)stream);
}


// The registration experiment's TEST protocol (pcrnet-registration/results_itrPCRNet_no_stop.py) on the device:
//   dpd_occlude            helper.add_occlusions (helper.py:963-982): cut the `drop` points nearest a seed point out of every source cloud and
//                          fill the cloud back to N points by repeating the survivors
//   dpd_pose_trace         the bookkeeping of the no-stop loop (:321-378, :464-474): every iteration's accumulated transform and its
//                          translation / rotation / convergence error, for all pairs and iterations in one launch
// Both are tiny and latency bound; they exist to take the per-pair host round trips out of the evaluation.  Deterministic: every sum
// has a fixed order, there are no atomics.  (The protocol's baseline loss, the square-rooted Chamfer distance dpd_chamfer_sqrt_fwd /
// _bwd, is a form of the paired Chamfer unit and lives with it in chamfer.hip.)
#include <float.h>

#include "common.h"
#include "pose_math.h"

namespace dpd {

// ---------------------------------------------------------------------------------------------------------------------------------
// Occlusion.  One workgroup per cloud; the cloud, its distances and its keys sit in LDS (40 KB at N = 2048).  Ranks come from counting,
// rank_i = #{j : (v_j, j) < (v_i, i)}: N^2 compares, every lane reads the SAME element j at a time (an LDS broadcast, no bank conflicts),
// four of them per ds_read_b128, and a thread holds up to PER of the points i in registers so that one read serves PER compares.
// A NaN in the compared array never counts (every comparison with it is false): that is how the padding up to a multiple of four and
// the points that were cut out are kept out of the second ranking.
constexpr int kOccThreads = 256;
constexpr int kOccMaxN = DPD_OCCLUDE_MAX_POINTS;      // the reference's MAX_NUM_POINT; PER = kOccMaxN / kOccThreads = 8 at most

template <int PER>
__device__ __forceinline__ void occ_rank(const float* __restrict__ s_v, int N4, const float (&vi)[PER], int (&cnt)[PER]) {
#pragma unroll
    for (int c = 0; c < PER; ++c) cnt[c] = 0;
    for (int j = 0; j < N4; j += 4) {        // N4 is a kernel argument's function: a wave-uniform loop
        const float4 v = *reinterpret_cast<const float4*>(s_v + j);
        const float vj[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
            for (int c = 0; c < PER; ++c) {
                const int i = (int)threadIdx.x + c * kOccThreads;
                cnt[c] += (vj[u] < vi[c] || (vj[u] == vi[c] && j + u < i)) ? 1 : 0;
            }
        }
    }
}

template <int PER>
__global__ __launch_bounds__(kOccThreads) void occlude_kernel(const float* __restrict__ src, const int32_t* __restrict__ seed_idx,
                                                              const float* __restrict__ order_key, int N, int drop,
                                                              float* __restrict__ out, int32_t* __restrict__ kept) {
    extern __shared__ __align__(16) float lds[];   // d [N4] | key [N4] | points [N][3]; the survivor list reuses d's room
    const int N4 = (N + 3) & ~3;
    float* s_d = lds;
    float* s_key = lds + N4;
    float* s_pts = lds + 2 * N4;
    int* s_list = reinterpret_cast<int*>(lds);
    const int b = blockIdx.x, t = threadIdx.x;
    const float* cloud = src + (size_t)b * N * 3;
    for (int e = t; e < N * 3; e += kOccThreads) s_pts[e] = cloud[e];
    const int seed = min(max(seed_idx[b], 0), N - 1);     // out of range is the caller's error; it must not become a read outside the cloud
    __syncthreads();
    const float sx = s_pts[seed * 3], sy = s_pts[seed * 3 + 1], sz = s_pts[seed * 3 + 2];
    const float nan = __int_as_float(0x7fc00000);
    float vi[PER];
    int cnt[PER];
#pragma unroll
    for (int c = 0; c < PER; ++c) {
        const int i = t + c * kOccThreads;
        vi[c] = nan;
        if (i < N) {
            const float dx = s_pts[i * 3] - sx, dy = s_pts[i * 3 + 1] - sy, dz = s_pts[i * 3 + 2] - sz;
            vi[c] = sqrtf((dx * dx + dy * dy) + dz * dz);      // np.linalg.norm(s - p, 2, -1) on float32, the form of dpd_nn_dist
        }
        if (i < N4) s_d[i] = vi[c];
    }
    __syncthreads();
    occ_rank<PER>(s_d, N4, vi, cnt);
    __syncthreads();                         // every read of d is done: its room becomes the survivor list
    if (order_key) {                         // survivors in ascending (key, index) order: rank them again among themselves
#pragma unroll
        for (int c = 0; c < PER; ++c) {
            const int i = t + c * kOccThreads;
            vi[c] = (i < N && cnt[c] >= drop) ? order_key[(size_t)b * N + i] : nan;
            if (i < N4) s_key[i] = vi[c];
        }
        __syncthreads();
        bool live[PER];
#pragma unroll
        for (int c = 0; c < PER; ++c) live[c] = t + c * kOccThreads < N && cnt[c] >= drop;
        occ_rank<PER>(s_key, N4, vi, cnt);
#pragma unroll
        for (int c = 0; c < PER; ++c)
            if (live[c]) s_list[cnt[c]] = t + c * kOccThreads;
    } else {                                 // ... or in ascending (distance, index) order: the first ranking, shifted
#pragma unroll
        for (int c = 0; c < PER; ++c) {
            const int i = t + c * kOccThreads;
            if (i < N && cnt[c] >= drop) s_list[cnt[c] - drop] = i;
        }
    }
    __syncthreads();
    const int S = N - drop;
    for (int j = t; j < N; j += kOccThreads) {               // concatenate-with-itself-then-truncate (helper.py:977-979)
        const int i = min(max(s_list[j % S], 0), N - 1);     // (a permutation for finite input; the clamp keeps NaN clouds inside the arrays)
        float* o = out + ((size_t)b * N + j) * 3;
        o[0] = s_pts[i * 3]; o[1] = s_pts[i * 3 + 1]; o[2] = s_pts[i * 3 + 2];
        if (kept) kept[(size_t)b * N + j] = i;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Trace.  One thread per pair walks its L iterations.

// registration.euler_to_mat: R = Rx(rx) Ry(ry) Rz(rz) (transforms3d euler2mat(rz, ry, rx, 'szyx'))
__device__ __forceinline__ void euler_to_mat_f64(double rx, double ry, double rz, double R[3][3]) {
    const double cx = cos(rx), sx = sin(rx), cy = cos(ry), sy = sin(ry), cz = cos(rz), sz = sin(rz);
    R[0][0] = cy * cz;                R[0][1] = -cy * sz;               R[0][2] = sy;
    R[1][0] = sx * sy * cz + cx * sz; R[1][1] = cx * cz - sx * sy * sz; R[1][2] = -sx * cy;
    R[2][0] = sx * sz - cx * sy * cz; R[2][1] = cx * sy * sz + sx * cz; R[2][2] = cx * cy;
}

// inverse of the affine [A t; 0 1]: Ai = A^-1 (adjugate / determinant), ti = -Ai t
__device__ __forceinline__ void affine_inverse_f64(const float T[4][4], double Ai[3][3], double ti[3]) {
    double A[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) A[i][j] = (double)T[i][j];
    const double c00 = A[1][1] * A[2][2] - A[1][2] * A[2][1], c01 = A[1][2] * A[2][0] - A[1][0] * A[2][2],
                 c02 = A[1][0] * A[2][1] - A[1][1] * A[2][0];
    const double det = A[0][0] * c00 + A[0][1] * c01 + A[0][2] * c02;
    Ai[0][0] = c00 / det; Ai[1][0] = c01 / det; Ai[2][0] = c02 / det;
    Ai[0][1] = (A[0][2] * A[2][1] - A[0][1] * A[2][2]) / det;
    Ai[1][1] = (A[0][0] * A[2][2] - A[0][2] * A[2][0]) / det;
    Ai[2][1] = (A[0][1] * A[2][0] - A[0][0] * A[2][1]) / det;
    Ai[0][2] = (A[0][1] * A[1][2] - A[0][2] * A[1][1]) / det;
    Ai[1][2] = (A[0][2] * A[1][0] - A[0][0] * A[1][2]) / det;
    Ai[2][2] = (A[0][0] * A[1][1] - A[0][1] * A[1][0]) / det;
    for (int i = 0; i < 3; ++i) ti[i] = -(Ai[i][0] * (double)T[0][3] + Ai[i][1] * (double)T[1][3] + Ai[i][2] * (double)T[2][3]);
}

__global__ __launch_bounds__(64) void pose_trace_kernel(const float* __restrict__ pred, int L, int B, float lim_rad,
                                                        const float* __restrict__ gt_pose, const float* __restrict__ shift,
                                                        float* __restrict__ T_all, double* __restrict__ te, double* __restrict__ re,
                                                        double* __restrict__ ce) {
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= B) return;
    float T[4][4];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) T[i][j] = i == j ? 1.f : 0.f;
    double gt[3] = {0, 0, 0}, sh[3] = {0, 0, 0}, RgT[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    if (gt_pose) {
        const float* g = gt_pose + (size_t)p * 6;
        double Rg[3][3];
        euler_to_mat_f64((double)g[3], (double)g[4], (double)g[5], Rg);
        for (int i = 0; i < 3; ++i) {
            gt[i] = (double)g[i];
            for (int j = 0; j < 3; ++j) RgT[i][j] = Rg[j][i];       // R_gt^-1
        }
    }
    if (shift)
        for (int i = 0; i < 3; ++i) sh[i] = (double)shift[(size_t)p * 3 + i];
    double Pi[3][3], pi[3];                  // inverse of the previous iteration's transform
    for (int l = 0; l <= L; ++l) {
        const size_t row = (size_t)l * B + p;
        if (T_all)
            for (int e = 0; e < 16; ++e) T_all[row * 16 + e] = T[e >> 2][e & 3];
        if (te || re || ce) {
            double Ai[3][3], ti[3];
            affine_inverse_f64(T, Ai, ti);
            if (te) {                        // find_errors: |gt_t - (trans(inv T) + shift)|  (get_error, :464-474)
                const double ex = gt[0] - (ti[0] + sh[0]), ey = gt[1] - (ti[1] + sh[1]), ez = gt[2] - (ti[2] + sh[2]);
                te[row] = sqrt(ex * ex + ey * ey + ez * ez);
            }
            if (re) {
                // The reference reads the pose of inv T as Euler angles (helper.find_final_pose_inv: mat2euler 'szyx') and find_errors
                // rebuilds the matrix from them.  On an exact rotation that round trip is the identity; rot(inv T) is one only to fp32
                // rounding (~1e-7 per iteration), and the round trip maps it to the exact rotation with those angles -- so it is kept.
                const double cy = hypot(Ai[0][0], Ai[0][1]);
                double rx, ry, rz;
                if (cy > 4.0 * DBL_EPSILON) {
                    rx = atan2(-Ai[1][2], Ai[2][2]); ry = atan2(Ai[0][2], cy); rz = atan2(-Ai[0][1], Ai[0][0]);
                } else {
                    rx = atan2(Ai[2][1], Ai[1][1]); ry = atan2(Ai[0][2], cy); rz = 0.0;
                }
                double Rp[3][3], E[3][3];
                euler_to_mat_f64(rx, ry, rz, Rp);
                for (int i = 0; i < 3; ++i)
                    for (int j = 0; j < 3; ++j) E[i][j] = Rp[i][0] * RgT[0][j] + Rp[i][1] * RgT[1][j] + Rp[i][2] * RgT[2][j];
                // the angle of E from both its sine and its cosine: acos alone loses half the digits near 0 and 180 degrees
                const double vx = E[2][1] - E[1][2], vy = E[0][2] - E[2][0], vz = E[1][0] - E[0][1];
                const double s = 0.5 * sqrt(vx * vx + vy * vy + vz * vz), c = 0.5 * ((E[0][0] + E[1][1] + E[2][2]) - 1.0);
                re[row] = atan2(s, c) * (180.0 / 3.14159265358979323846);
            }
            if (ce) {                        // check_convergenceT (:155-167): |T_l inv(T_{l-1}) - I|_F^2; the last rows cancel exactly
                double acc = 1.0;
                if (l > 0) {
                    acc = 0.0;
                    for (int i = 0; i < 3; ++i) {
                        double tr = (double)T[i][3];
                        for (int j = 0; j < 3; ++j) {
                            const double m = ((double)T[i][0] * Pi[0][j] + (double)T[i][1] * Pi[1][j] + (double)T[i][2] * Pi[2][j]) - (i == j ? 1.0 : 0.0);
                            acc += m * m;
                            tr += (double)T[i][j] * pi[j];
                        }
                        acc += tr * tr;
                    }
                }
                ce[row] = acc;
            }
            for (int i = 0; i < 3; ++i) {
                pi[i] = ti[i];
                for (int j = 0; j < 3; ++j) Pi[i][j] = Ai[i][j];
            }
        }
        if (l == L) break;
        // T <- [R(q / max(|q|, 1e-12)) t; 0 1] T: the mode-0 arithmetic of dpd_pose_apply_fwd, through the same device functions
        float pr[7];
        for (int j = 0; j < 7; ++j) pr[j] = pred[row * 7 + j];
        const Pose7 P = quat_normalize_dev(pr, lim_rad);
        const float dc = fmaxf(quat_norm_dev(P.q), 1e-12f);
        float qc[4], R[3][3], Tn[4][4];
        for (int i = 0; i < 4; ++i) qc[i] = P.q[i] / dc;
        quat_to_mat_dev(qc, R);
        for (int j = 0; j < 4; ++j) {
            const float Tc[4] = {T[0][j], T[1][j], T[2][j], T[3][j]};
            for (int i = 0; i < 4; ++i) Tn[i][j] = pose_compose_entry(R, P.t, Tc, i);
        }
        for (int i = 0; i < 4; ++i)
            for (int j = 0; j < 4; ++j) T[i][j] = Tn[i][j];
    }
}

}  // namespace dpd

extern "C" int dpd_occlude(const float* src, const int32_t* seed_idx, const float* order_key, int B, int N, int drop, float* out,
                           int32_t* kept, void* stream) {
    using namespace dpd;
    if (!src || !seed_idx || !out) return DPD_E_NULL;
    if (B <= 0 || N <= 0 || drop < 0 || drop >= N) return DPD_E_DIM;       // an empty survivor set: the reference would loop forever
    if (N > kOccMaxN) return DPD_E_UNSUPPORTED;
    const int N4 = (N + 3) & ~3;
    const size_t lds = (size_t)(2 * N4 + 3 * N) * sizeof(float);
    const hipStream_t s = (hipStream_t)stream;
    if (N <= kOccThreads) DPD_LAUNCH(occlude_kernel<1>, dim3(B), dim3(kOccThreads), lds, s, src, seed_idx, order_key, N, drop, out, kept);
    else if (N <= 2 * kOccThreads) DPD_LAUNCH(occlude_kernel<2>, dim3(B), dim3(kOccThreads), lds, s, src, seed_idx, order_key, N, drop, out, kept);
    else if (N <= 4 * kOccThreads) DPD_LAUNCH(occlude_kernel<4>, dim3(B), dim3(kOccThreads), lds, s, src, seed_idx, order_key, N, drop, out, kept);
    else DPD_LAUNCH(occlude_kernel<8>, dim3(B), dim3(kOccThreads), lds, s, src, seed_idx, order_key, N, drop, out, kept);
    DPD_CHECK_LAUNCH();
    return 0;
}

extern "C" int dpd_pose_trace(const float* pred, int L, int B, float lim_rot_deg, const float* gt_pose, const float* shift, float* T_all,
                              double* te, double* re, double* ce, void* stream) {
    using namespace dpd;
    if (!pred || (!T_all && !te && !re && !ce)) return DPD_E_NULL;
    if ((te || re) && !gt_pose) return DPD_E_NULL;
    if (L < 1 || B < 1) return DPD_E_DIM;
    DPD_LAUNCH(pose_trace_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, pred, L, B, lim_rad_of(lim_rot_deg),
               gt_pose, shift, T_all, te, re, ce);
    DPD_CHECK_LAUNCH();
    return 0;
}

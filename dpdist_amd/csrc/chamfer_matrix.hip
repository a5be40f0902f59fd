// All-pairs Chamfer and Hausdorff: the baseline distance matrices of two sets of clouds (include/dpdist_capi.h: dpd_chamfer_matrix_fwd /
// _bwd; driven by dpdist_amd/baselines.py).  One DIRECTED matrix per call: surface clouds S [Cs,Ns,3], query clouds Q [Cq,Nq,3],
//     mn(i,j,n) = min over the real points p of S_i of |q_jn - s_ip|^2        (chamfer_pair_sq of chamfer_scan.h: fp32, unfused)
// and per pair the mean of mn, the mean of sqrtf(mn) and the max of mn over the real queries of Q_j.  Nothing of size [Cs,Cq,N] exists:
// a workgroup keeps ONE surface cloud in LDS ([p][3] floats, 48 KB at the cap) and walks query clouds past it; every lane reads the
// same surface point (an LDS broadcast, four points per three 16-byte reads) and reuses it for up to four query points it holds in
// registers.  The backward recomputes the argmins (lowest index on ties) instead of storing them.
//
// Determinism: a pair is reduced inside one workgroup, thread t sums its own queries n = t, t + 256, ... in that order, then the
// fixed DPP tree of wave_sum and ((w0 + w1) + (w2 + w3)) over the four waves; invalid lanes add +0.0.  The order depends on the
// pair's two counts only, so neither the padded widths, the padding, the other clouds nor the grid change a bit.  No atomics.
#include "common.h"
#include "chamfer_scan.h"

namespace dpd {

constexpr int kCmQueries = 4;          // query points a thread keeps in registers per pass (forward, query route)
constexpr int kCmPass = 256 * kCmQueries;
constexpr int kCmSurfThreads = 1024;   // surface route: one workgroup per surface cloud
constexpr int kCmFwdUnits = 2048;      // forward: (surface cloud, query group) units aimed at, 8 per CU
constexpr int kCmDqBlocks = 512;       // query route: workgroups aimed at before a thread takes more queries, 2 per CU

// the queries n = first + r * 256 of this thread (r < RMAX) against the staged cloud; `live` (wave-uniform) is how many of the wave's r
// carry a real query, so a wave of a small cloud scans for one or two points per thread, not four.  Lanes without a real query scan the
// origin and are dropped by the caller; the padding is never read.
template <int RMAX, bool ARG>
__device__ __forceinline__ void cm_scan_queries(const float* __restrict__ s_y, int ny, const float* __restrict__ q, int first, int nq, int live,
                                                float (&best)[RMAX], int (&arg)[RMAX]) {
    float pt[RMAX][3];
#pragma unroll
    for (int r = 0; r < RMAX; ++r) {
        const int n = first + r * 256;
        const bool real = n < nq;
        pt[r][0] = real ? q[n * 3] : 0.f;
        pt[r][1] = real ? q[n * 3 + 1] : 0.f;
        pt[r][2] = real ? q[n * 3 + 2] : 0.f;
        best[r] = 0.f;
        arg[r] = 0;
    }
    if constexpr (RMAX == 1) {
        cm_scan<1, ARG>(s_y, ny, pt, best, arg);
    } else {
        if (live <= 1) {
            float b1[1];
            int a1[1];
            const float q1[1][3] = {{pt[0][0], pt[0][1], pt[0][2]}};
            cm_scan<1, ARG>(s_y, ny, q1, b1, a1);
            best[0] = b1[0];
            arg[0] = a1[0];
        } else if (RMAX == 2 || live == 2) {
            float b2[2];
            int a2[2];
            const float q2[2][3] = {{pt[0][0], pt[0][1], pt[0][2]}, {pt[1][0], pt[1][1], pt[1][2]}};
            cm_scan<2, ARG>(s_y, ny, q2, b2, a2);
            best[0] = b2[0]; best[1] = b2[1];
            arg[0] = a2[0]; arg[1] = a2[1];
        } else {
            cm_scan<RMAX, ARG>(s_y, ny, pt, best, arg);
        }
    }
}

// how many r of this wave's pass hold a real query (0: the wave has nothing to do in this pass)
__device__ __forceinline__ int cm_live(int base, int nq, int rmax) {
    const int wave_first = base + (threadIdx.x & ~63);
    if (wave_first >= nq) return 0;
    const int live = (nq - wave_first + 255) / 256;
    return live > rmax ? rmax : live;
}

// Forward.  Unit u = (surface cloud i, group g of `per` consecutive query clouds); a workgroup stages S_i once per unit.
__global__ __launch_bounds__(256) void chamfer_matrix_fwd_kernel(const float* __restrict__ S, const int32_t* __restrict__ countsS, int Cs, int Ns,
                                                                 const float* __restrict__ Q, const int32_t* __restrict__ countsQ, int Cq, int Nq,
                                                                 int groups, int per, float* __restrict__ mean_sq, float* __restrict__ mean_rt,
                                                                 float* __restrict__ max_sq) {
    extern __shared__ __align__(16) float s_y[];   // [ns][3]
    __shared__ float red[3][4];
    const long long units = (long long)Cs * groups;
    for (long long u = blockIdx.x; u < units; u += gridDim.x) {   // 64-bit: the last stride may pass 2^31
        const int i = (int)(u / groups), g = (int)(u % groups);
        const int ns = ragged_count(countsS, i, Ns);
        __syncthreads();
        cm_stage(s_y, S + (size_t)i * Ns * 3, ns);
        __syncthreads();
        const long long run_end = (long long)(g + 1) * per;
        const int j1 = run_end < Cq ? (int)run_end : Cq;
        for (int j = g * per; j < j1; ++j) {
            const int nq = ragged_count(countsQ, j, Nq);
            const float* q = Q + (size_t)j * Nq * 3;
            float ssq = 0.f, srt = 0.f, mx = 0.f;
            for (int base = 0; base < nq; base += kCmPass) {
                const int live = cm_live(base, nq, kCmQueries);
                if (live == 0) continue;
                float best[kCmQueries];
                int arg[kCmQueries];
                const int first = base + threadIdx.x;
                cm_scan_queries<kCmQueries, false>(s_y, ns, q, first, nq, live, best, arg);
#pragma unroll
                for (int r = 0; r < kCmQueries; ++r) {
                    if (first + r * 256 < nq) {
                        ssq += best[r];
                        srt += sqrtf(best[r]);
                        mx = fmaxf(mx, best[r]);
                    }
                }
            }
            ssq = wave_sum(ssq);
            srt = wave_sum(srt);
            mx = cm_wave_max(mx);
            if ((threadIdx.x & 63) == 0) {
                red[0][threadIdx.x >> 6] = ssq;
                red[1][threadIdx.x >> 6] = srt;
                red[2][threadIdx.x >> 6] = mx;
            }
            __syncthreads();
            if (threadIdx.x == 0) {
                const size_t o = (size_t)i * Cq + j;
                if (mean_sq) mean_sq[o] = ((red[0][0] + red[0][1]) + (red[0][2] + red[0][3])) / (float)nq;
                if (mean_rt) mean_rt[o] = ((red[1][0] + red[1][1]) + (red[1][2] + red[1][3])) / (float)nq;
                if (max_sq) max_sq[o] = fmaxf(fmaxf(red[2][0], red[2][1]), fmaxf(red[2][2], red[2][3]));
            }
            __syncthreads();
        }
    }
}

// Query route: dQ[j,n] = sum_i W[i,j] / nq_j * t(q_n, s_arg(i,j,n)), i ascending.  Workgroup (j, chunk of 256 R queries) walks every
// surface cloud, staging each; rows at or beyond the count are written +0.0.  A thread sums its own queries only, so R (the host
// takes the largest that still fills the device) changes no bit.
template <int FORM, int R>
__global__ __launch_bounds__(256) void chamfer_matrix_dq_kernel(const float* __restrict__ S, const int32_t* __restrict__ countsS, int Cs, int Ns,
                                                                const float* __restrict__ Q, const int32_t* __restrict__ countsQ, int Cq, int Nq,
                                                                const float* __restrict__ W, float* __restrict__ dQ) {
    extern __shared__ __align__(16) float s_y[];   // [ns][3]
    const int base = blockIdx.y * (256 * R);
    const int first = base + threadIdx.x;
    for (long long j = blockIdx.x; j < Cq; j += gridDim.x) {   // 64-bit: the last stride may pass 2^31
        const int nq = ragged_count(countsQ, (int)j, Nq);
        const float* q = Q + (size_t)j * Nq * 3;
        float* dq = dQ + (size_t)j * Nq * 3;
        const int live = base < nq ? cm_live(base, nq, R) : 0;
        float acc[R][3] = {};
        if (base < nq) {                                     // workgroup-uniform: a chunk of padding only writes zeros
            for (int i = 0; i < Cs; ++i) {
                const int ns = ragged_count(countsS, i, Ns);
                __syncthreads();
                cm_stage(s_y, S + (size_t)i * Ns * 3, ns);
                __syncthreads();
                if (live == 0) continue;
                const float w = W[(size_t)i * Cq + j] / (float)nq;
                float best[R];
                int arg[R];
                cm_scan_queries<R, true>(s_y, ns, q, first, nq, live, best, arg);
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const int n = first + r * 256;
                    if (n < nq) cm_term<FORM>(w, best[r], q[n * 3], q[n * 3 + 1], q[n * 3 + 2], s_y + arg[r] * 3, acc[r]);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int n = first + r * 256;
            if (n < Nq) {
                const bool real = n < nq;
                dq[n * 3] = real ? acc[r][0] : 0.f;
                dq[n * 3 + 1] = real ? acc[r][1] : 0.f;
                dq[n * 3 + 2] = real ? acc[r][2] : 0.f;
            }
        }
    }
}

// Surface route: dS[i,p] = - sum_j W[i,j] / nq_j * sum_{n : arg(i,j,n) = p} t(q_n, s_p), j ascending and n ascending inside j; the sign
// is taken into the term (t(s_p, q_n) = - t(q_n, s_p) exactly), so a point that nothing selects keeps +0.0.  One workgroup of 1024
// threads per surface cloud: per query cloud it writes the argmins of all queries to LDS, then thread t walks them for its own
// points p = t, t + 1024, ... (deterministic gather, as chamfer_grad_kernel; the match walk is one compare per query).
template <int FORM>
__global__ __launch_bounds__(kCmSurfThreads) void chamfer_matrix_ds_kernel(const float* __restrict__ S, const int32_t* __restrict__ countsS, int Cs,
                                                                           int Ns, const float* __restrict__ Q, const int32_t* __restrict__ countsQ,
                                                                           int Cq, int Nq, const float* __restrict__ W, float* __restrict__ dS) {
    extern __shared__ __align__(16) float s_y[];   // [Ns][3], then the argmins [Nq]
    int* s_arg = reinterpret_cast<int*>(s_y + ((Ns * 3 + 3) & ~3));
    const int t = threadIdx.x;
    for (long long i = blockIdx.x; i < Cs; i += gridDim.x) {   // 64-bit: the last stride may pass 2^31
        const int ns = ragged_count(countsS, (int)i, Ns);
        __syncthreads();
        cm_stage(s_y, S + (size_t)i * Ns * 3, ns);
        __syncthreads();
        float own[4][3], acc[4][3] = {};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int p = t + k * kCmSurfThreads;
#pragma unroll
            for (int c = 0; c < 3; ++c) own[k][c] = p < ns ? s_y[p * 3 + c] : 0.f;
        }
        for (int j = 0; j < Cq; ++j) {
            const int nq = ragged_count(countsQ, j, Nq);
            const float* q = Q + (size_t)j * Nq * 3;
            const float w = W[(size_t)i * Cq + j] / (float)nq;
            for (int base = 0; base < nq; base += kCmSurfThreads) {
                if (base + (t & ~63) >= nq) continue;
                const int n = base + t;
                const bool real = n < nq;
                const float q1[1][3] = {{real ? q[n * 3] : 0.f, real ? q[n * 3 + 1] : 0.f, real ? q[n * 3 + 2] : 0.f}};
                float b1[1];
                int a1[1];
                cm_scan<1, true>(s_y, ns, q1, b1, a1);
                if (real) s_arg[n] = a1[0];
            }
            __syncthreads();
            auto hit = [&](int a, int n) {
                if ((a & (kCmSurfThreads - 1)) != t) return;
                const float qn[3] = {q[n * 3], q[n * 3 + 1], q[n * 3 + 2]};
                const int k = a / kCmSurfThreads;
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) {
                    if (kk == k) {
                        const float d2 = chamfer_pair_sq(qn[0], qn[1], qn[2], own[kk]);   // the scan's bits for this pair of points
                        cm_term<FORM>(w, d2, own[kk][0], own[kk][1], own[kk][2], qn, acc[kk]);
                    }
                }
            };
            int n = 0;
            for (; n + 4 <= nq; n += 4) {                    // four argmins per LDS read, visited in ascending n
                const int4 a4 = *reinterpret_cast<const int4*>(s_arg + n);
                hit(a4.x, n);
                hit(a4.y, n + 1);
                hit(a4.z, n + 2);
                hit(a4.w, n + 3);
            }
            for (; n < nq; ++n) hit(s_arg[n], n);
            __syncthreads();
        }
        float* ds = dS + (size_t)i * Ns * 3;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int p = t + k * kCmSurfThreads;
            if (p < Ns) {
                const bool real = p < ns;
                ds[p * 3] = real ? acc[k][0] : 0.f;
                ds[p * 3 + 1] = real ? acc[k][1] : 0.f;
                ds[p * 3 + 2] = real ? acc[k][2] : 0.f;
            }
        }
    }
}

static int cm_check_dims(int Cs, int Ns, int Cq, int Nq) {
    if (Cs < 1 || Cq < 1 || (long long)Cs * (long long)Cq >= (1ll << 31)) return DPD_E_DIM;
    if (Ns < 1 || Nq < 1 || Ns > kCmMaxPoints || Nq > kCmMaxPoints) return DPD_E_UNSUPPORTED;
    return 0;
}

}  // namespace dpd

extern "C" int dpd_chamfer_matrix_fwd(const float* S, const int32_t* countsS, int Cs, int Ns, const float* Q, const int32_t* countsQ, int Cq,
                                      int Nq, float* mean_sq, float* mean_rt, float* max_sq, void* stream) {
    using namespace dpd;
    if (!S || !Q || (!mean_sq && !mean_rt && !max_sq)) return DPD_E_NULL;
    if (const int rc = cm_check_dims(Cs, Ns, Cq, Nq)) return rc;
    // groups of `per` consecutive query clouds: about kCmFwdUnits units, never more than one unit per pair
    const int want = kCmFwdUnits / Cs > 0 ? kCmFwdUnits / Cs : 1;
    const int per = (Cq + want - 1) / want;
    const int groups = (Cq + per - 1) / per;
    const long long units = (long long)Cs * groups;
    const int grid = units < kCmMaxGrid ? (int)units : kCmMaxGrid;
    const size_t lds = (size_t)((Ns * 3 + 3) & ~3) * sizeof(float);
    DPD_LAUNCH(chamfer_matrix_fwd_kernel, dim3(grid), dim3(256), lds, (hipStream_t)stream, S, countsS, Cs, Ns, Q, countsQ, Cq, Nq, groups, per,
               mean_sq, mean_rt, max_sq);
    DPD_CHECK_LAUNCH();
    return 0;
}

extern "C" int dpd_chamfer_matrix_bwd(const float* S, const int32_t* countsS, int Cs, int Ns, const float* Q, const int32_t* countsQ, int Cq,
                                      int Nq, int form, const float* W, float* dS, float* dQ, void* stream) {
    using namespace dpd;
    if (!S || !Q || !W || (!dS && !dQ)) return DPD_E_NULL;
    if (form != 0 && form != 1) return DPD_E_DIM;
    if (const int rc = cm_check_dims(Cs, Ns, Cq, Nq)) return rc;
    const size_t lds_s = (size_t)((Ns * 3 + 3) & ~3) * sizeof(float);
    if (dQ) {
        // queries per thread: the most (the fewest LDS reads per evaluation) that still gives every CU two workgroups
        int R = kCmQueries;
        while (R > 1 && (long long)Cq * ((Nq + 256 * R - 1) / (256 * R)) < kCmDqBlocks) R /= 2;
        const dim3 grid(Cq < kCmMaxGrid ? Cq : kCmMaxGrid, (Nq + 256 * R - 1) / (256 * R));
        void (*kern)(const float*, const int32_t*, int, int, const float*, const int32_t*, int, int, const float*, float*) =
            form == 0 ? (R == 4 ? chamfer_matrix_dq_kernel<0, 4> : R == 2 ? chamfer_matrix_dq_kernel<0, 2> : chamfer_matrix_dq_kernel<0, 1>)
                      : (R == 4 ? chamfer_matrix_dq_kernel<1, 4> : R == 2 ? chamfer_matrix_dq_kernel<1, 2> : chamfer_matrix_dq_kernel<1, 1>);
        DPD_LAUNCH(kern, grid, dim3(256), lds_s, (hipStream_t)stream, S, countsS, Cs, Ns, Q, countsQ, Cq, Nq, W, dQ);
        DPD_CHECK_LAUNCH();
    }
    if (dS) {
        const dim3 grid(Cs < kCmMaxGrid ? Cs : kCmMaxGrid);
        const size_t lds = lds_s + (size_t)Nq * sizeof(int);   // 64 KB at the cap: no opt-in needed
        if (form == 0)
            DPD_LAUNCH(chamfer_matrix_ds_kernel<0>, grid, dim3(kCmSurfThreads), lds, (hipStream_t)stream, S, countsS, Cs, Ns, Q, countsQ, Cq, Nq, W,
                       dS);
        else
            DPD_LAUNCH(chamfer_matrix_ds_kernel<1>, grid, dim3(kCmSurfThreads), lds, (hipStream_t)stream, S, countsS, Cs, Ns, Q, countsQ, Cq, Nq, W,
                       dS);
        DPD_CHECK_LAUNCH();
    }
    return 0;
}

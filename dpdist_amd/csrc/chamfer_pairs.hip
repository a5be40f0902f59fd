// Chamfer and Hausdorff of the pairs (A_b, B_b) of two ragged sets (include/dpdist_capi.h: dpd_chamfer_pairs_fwd / _bwd; driven by
// dpdist_amd/baselines.py: chamfer_pairs, hausdorff_pairs, ChamferPairs).  Direction AB: A_b is the surface, the points of B_b are the
// queries; direction BA: the sets swapped.  Every value is dpd_chamfer_matrix_fwd / _bwd's on the 1 x 1 matrix of that pair, bit for bit:
// the scan, the term of a gradient and the count clamp are the bodies of chamfer_scan.h that chamfer_matrix.hip runs.
//
// The workload is few, large pairs, so a pair is spread over workgroups instead of owned by one:
//   scan     unit (pair, direction, chunk of 256 queries): stages the pair's real surface points in LDS ([p][3] floats, 48 KB at the cap),
//            each thread scans them for its query and writes min / arg.  A unit wholly in the padding does nothing.
//   finish   unit (pair, direction): reduces the minima to mean_sq, mean_rt, max_sq in the matrix kernel's order -- thread t sums the
//            queries t, t + 256, ... ascending, then wave_sum's tree, then ((w0 + w1) + (w2 + w3)); lanes without a query add +0.0.
//   grad     unit (pair, set, chunk of 256 points of that set): the owner of a point adds its surface route (a walk over the other set's
//            argmins in ascending query order, staged in LDS: a deterministic gather) and its query route (its own argmin), and writes
//            the sum; a row at or beyond the count is written +0.0.  One writer per element, both routes in one kernel.
// Units are strided over at most 2^20 workgroups.  No atomics: two calls give the same bits, and the padded widths, the padding and the
// other pairs change no bit.
#include "common.h"
#include "chamfer_scan.h"

namespace dpd {

__global__ __launch_bounds__(256) void chamfer_pairs_scan_kernel(const float* __restrict__ A, const int32_t* __restrict__ countsA, int Wa,
                                                                 const float* __restrict__ B, const int32_t* __restrict__ countsB, int Wb,
                                                                 long long P, int chunks_ab, int chunks_ba, float* __restrict__ min_ab,
                                                                 int32_t* __restrict__ arg_ab, float* __restrict__ min_ba,
                                                                 int32_t* __restrict__ arg_ba) {
    extern __shared__ __align__(16) float s_y[];   // [ns][3]
    const int per = chunks_ab + chunks_ba;
    const long long units = P * per;
    for (long long u = blockIdx.x; u < units; u += gridDim.x) {
        const long long b = u / per;
        const int r = (int)(u % per);
        const bool dir = r >= chunks_ab;           // 0: AB (surface A, queries B), 1: BA
        const int chunk = dir ? r - chunks_ab : r;
        const int na = ragged_count(countsA, (int)b, Wa), nb = ragged_count(countsB, (int)b, Wb);
        const int ns = dir ? nb : na, nq = dir ? na : nb, Wq = dir ? Wa : Wb;
        if (chunk * 256 >= nq) continue;           // a chunk of padding (workgroup-uniform, ahead of every barrier)
        const float* a = A + (size_t)b * Wa * 3;
        const float* bb = B + (size_t)b * Wb * 3;
        __syncthreads();                           // the unit before this one is done with the LDS
        cm_stage(s_y, dir ? bb : a, ns);
        __syncthreads();
        const int n = chunk * 256 + threadIdx.x;
        if (chunk * 256 + (int)(threadIdx.x & ~63u) >= nq) continue;   // a wave of padding
        const bool real = n < nq;                  // a lane without a query scans the origin and stores nothing
        const float* q = (dir ? a : bb) + (size_t)n * 3;
        const float q1[1][3] = {{real ? q[0] : 0.f, real ? q[1] : 0.f, real ? q[2] : 0.f}};
        float b1[1];
        int a1[1];
        cm_scan<1, true>(s_y, ns, q1, b1, a1);
        if (real) {
            (dir ? min_ba : min_ab)[(size_t)b * Wq + n] = b1[0];
            (dir ? arg_ba : arg_ab)[(size_t)b * Wq + n] = a1[0];
        }
    }
}

// out [2,P]: row 0 the AB direction, row 1 BA
__global__ __launch_bounds__(256) void chamfer_pairs_finish_kernel(const int32_t* __restrict__ countsA, int Wa, const int32_t* __restrict__ countsB,
                                                                   int Wb, long long P, const float* __restrict__ min_ab,
                                                                   const float* __restrict__ min_ba, float* __restrict__ mean_sq,
                                                                   float* __restrict__ mean_rt, float* __restrict__ max_sq) {
    __shared__ float red[3][4];
    for (long long u = blockIdx.x; u < 2 * P; u += gridDim.x) {
        const bool dir = u >= P;
        const long long b = dir ? u - P : u;
        const int nq = dir ? ragged_count(countsA, (int)b, Wa) : ragged_count(countsB, (int)b, Wb);
        const float* mn = dir ? min_ba + (size_t)b * Wa : min_ab + (size_t)b * Wb;
        float ssq = 0.f, srt = 0.f, mx = 0.f;
        for (int n = threadIdx.x; n < nq; n += 256) {
            const float v = mn[n];
            ssq += v;
            srt += sqrtf(v);
            mx = fmaxf(mx, v);
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
            if (mean_sq) mean_sq[u] = ((red[0][0] + red[0][1]) + (red[0][2] + red[0][3])) / (float)nq;
            if (mean_rt) mean_rt[u] = ((red[1][0] + red[1][1]) + (red[1][2] + red[1][3])) / (float)nq;
            if (max_sq) max_sq[u] = fmaxf(fmaxf(red[2][0], red[2][1]), fmaxf(red[2][2], red[2][3]));
        }
        __syncthreads();
    }
}

// Unit (pair b, set, chunk): set 0 owns points of A (surface of AB, query of BA), set 1 points of B (surface of BA, query of AB).
// G_ab / G_ba: the upstream of each directed mean, NULL = that direction carries none and its routes are skipped.
template <int FORM>
__global__ __launch_bounds__(256) void chamfer_pairs_grad_kernel(const float* __restrict__ A, const int32_t* __restrict__ countsA, int Wa,
                                                                 const float* __restrict__ B, const int32_t* __restrict__ countsB, int Wb,
                                                                 long long P, int chunks_a, int chunks_b, const int32_t* __restrict__ arg_ab,
                                                                 const int32_t* __restrict__ arg_ba, const float* __restrict__ G_ab,
                                                                 const float* __restrict__ G_ba, float* __restrict__ dA,
                                                                 float* __restrict__ dB) {
    extern __shared__ __align__(16) int s_arg[];   // the argmins of the other set's real points into this one
    const int per = chunks_a + chunks_b;
    const long long units = P * per;
    for (long long u = blockIdx.x; u < units; u += gridDim.x) {
        const long long b = u / per;
        const int r = (int)(u % per);
        const bool set = r >= chunks_a;
        const int chunk = set ? r - chunks_a : r;
        const int na = ragged_count(countsA, (int)b, Wa), nb = ragged_count(countsB, (int)b, Wb);
        const int nx = set ? nb : na, ny = set ? na : nb, Wx = set ? Wb : Wa, Wy = set ? Wa : Wb;
        const float* x = (set ? B : A) + (size_t)b * Wx * 3;
        const float* y = (set ? A : B) + (size_t)b * Wy * 3;
        float* dx = (set ? dB : dA) + (size_t)b * Wx * 3;
        // this set is the surface of direction (set ? BA : AB), whose queries are the other set's points, and the query of the other
        const float* Gs = set ? G_ba : G_ab;
        const float* Gq = set ? G_ab : G_ba;
        const int32_t* as = (set ? arg_ba : arg_ab) + (size_t)b * Wy;   // [ny], values < nx
        const int32_t* aq = (set ? arg_ab : arg_ba) + (size_t)b * Wx;   // [nx], values < ny
        const int p = chunk * 256 + threadIdx.x;
        float out[3] = {0.f, 0.f, 0.f};
        if (chunk * 256 < nx) {                                         // workgroup-uniform: a chunk of padding only writes zeros
            __syncthreads();                                            // the unit before this one is done with the LDS
            if (Gs)
                for (int n = threadIdx.x; n < ny; n += 256) s_arg[n] = as[n];
            __syncthreads();
            if (p < nx) {
                const float own[3] = {x[p * 3], x[p * 3 + 1], x[p * 3 + 2]};
                float acc_s[3] = {0.f, 0.f, 0.f}, acc_q[3] = {0.f, 0.f, 0.f};
                if (Gs) {
                    const float w = Gs[b] / (float)ny;
                    auto hit = [&](int a, int n) {
                        if (a != p) return;
                        const float qn[3] = {y[n * 3], y[n * 3 + 1], y[n * 3 + 2]};
                        const float d2 = chamfer_pair_sq(qn[0], qn[1], qn[2], own);   // the scan's bits for this pair of points
                        cm_term<FORM>(w, d2, own[0], own[1], own[2], qn, acc_s);
                    };
                    int n = 0;
                    for (; n + 4 <= ny; n += 4) {                        // four argmins per LDS read, visited in ascending n
                        const int4 a4 = *reinterpret_cast<const int4*>(s_arg + n);
                        hit(a4.x, n);
                        hit(a4.y, n + 1);
                        hit(a4.z, n + 2);
                        hit(a4.w, n + 3);
                    }
                    for (; n < ny; ++n) hit(s_arg[n], n);
                }
                if (Gq) {
                    const float w = Gq[b] / (float)nx;
                    int a = aq[p];
                    a = a < 0 ? 0 : (a >= ny ? ny - 1 : a);             // the forward's index; a foreign one cannot leave the cloud
                    const float* s = y + a * 3;
                    const float d2 = chamfer_pair_sq(own[0], own[1], own[2], s);
                    cm_term<FORM>(w, d2, own[0], own[1], own[2], s, acc_q);
                }
#pragma unroll
                for (int c = 0; c < 3; ++c) out[c] = (Gs && Gq) ? acc_s[c] + acc_q[c] : (Gs ? acc_s[c] : acc_q[c]);
            }
        }
        if (p < Wx) {
            dx[p * 3] = out[0];
            dx[p * 3 + 1] = out[1];
            dx[p * 3 + 2] = out[2];
        }
    }
}

static int cp_check(const void* A, const void* B, int Wa, int Wb, int P) {
    if (!A || !B) return DPD_E_NULL;
    if (P < 1) return DPD_E_DIM;
    if (Wa < 1 || Wb < 1 || Wa > kCmMaxPoints || Wb > kCmMaxPoints) return DPD_E_UNSUPPORTED;
    return 0;
}

}  // namespace dpd

extern "C" int dpd_chamfer_pairs_fwd(const float* A, const int32_t* countsA, int Wa, const float* B, const int32_t* countsB, int Wb, int P,
                                     float* min_ab, int32_t* arg_ab, float* min_ba, int32_t* arg_ba, float* mean_sq, float* mean_rt,
                                     float* max_sq, void* stream) {
    using namespace dpd;
    if (!min_ab || !arg_ab || !min_ba || !arg_ba) return DPD_E_NULL;
    if (const int rc = cp_check(A, B, Wa, Wb, P)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int chunks_ab = (Wb + 255) / 256, chunks_ba = (Wa + 255) / 256;
    const long long units = (long long)P * (chunks_ab + chunks_ba);
    const int W = Wa > Wb ? Wa : Wb;
    const size_t lds = (size_t)((W * 3 + 3) & ~3) * sizeof(float);   // 48 KB at the cap: no opt-in needed
    DPD_LAUNCH(chamfer_pairs_scan_kernel, dim3(units < kCmMaxGrid ? (int)units : kCmMaxGrid), dim3(256), lds, s, A, countsA, Wa, B, countsB, Wb,
               (long long)P, chunks_ab, chunks_ba, min_ab, arg_ab, min_ba, arg_ba);
    DPD_CHECK_LAUNCH();
    if (mean_sq || mean_rt || max_sq) {
        const long long fin = 2ll * P;
        DPD_LAUNCH(chamfer_pairs_finish_kernel, dim3(fin < kCmMaxGrid ? (int)fin : kCmMaxGrid), dim3(256), 0, s, countsA, Wa, countsB, Wb,
                   (long long)P, (const float*)min_ab, (const float*)min_ba, mean_sq, mean_rt, max_sq);
        DPD_CHECK_LAUNCH();
    }
    return 0;
}

extern "C" int dpd_chamfer_pairs_bwd(const float* A, const int32_t* countsA, int Wa, const float* B, const int32_t* countsB, int Wb, int P,
                                     int form, const int32_t* arg_ab, const int32_t* arg_ba, const float* G_ab, const float* G_ba, float* dA,
                                     float* dB, void* stream) {
    using namespace dpd;
    if (!arg_ab || !arg_ba || (!G_ab && !G_ba) || (!dA && !dB)) return DPD_E_NULL;
    if (form != 0 && form != 1) return DPD_E_DIM;
    if (const int rc = cp_check(A, B, Wa, Wb, P)) return rc;
    const int chunks_a = dA ? (Wa + 255) / 256 : 0, chunks_b = dB ? (Wb + 255) / 256 : 0;
    const long long units = (long long)P * (chunks_a + chunks_b);
    const int W = Wa > Wb ? Wa : Wb;
    const size_t lds = (size_t)((W + 3) & ~3) * sizeof(int);
    const dim3 grid(units < kCmMaxGrid ? (int)units : kCmMaxGrid);
    if (form == 0)
        DPD_LAUNCH(chamfer_pairs_grad_kernel<0>, grid, dim3(256), lds, (hipStream_t)stream, A, countsA, Wa, B, countsB, Wb, (long long)P, chunks_a,
                   chunks_b, arg_ab, arg_ba, G_ab, G_ba, dA, dB);
    else
        DPD_LAUNCH(chamfer_pairs_grad_kernel<1>, grid, dim3(256), lds, (hipStream_t)stream, A, countsA, Wa, B, countsB, Wb, (long long)P, chunks_a,
                   chunks_b, arg_ab, arg_ba, G_ab, G_ba, dA, dB);
    DPD_CHECK_LAUNCH();
    return 0;
}

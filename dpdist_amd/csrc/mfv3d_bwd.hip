// 3D modified Fisher Vector encoder, BACKWARD: dfv [C,G,20] -> dpts [C,N,3].  (Forward, and the map of all forms: mfv3d.hip; what the
// two units share: mfv3d_int.h.)  Replaces the TF autodiff of utils/dpdist_util.py:22-141.
//
// Everything the forward produced is recomputed from the same factorised tables instead of being saved.  Chain (TF autodiff of :69-126):
//   fv = s * rsqrt(ss_f),  s = pnorm(v)    -> ds = rs*dfv - s * <s,dfv>_G * rs^3            (tf.nn.l2_normalize)
//   v  = stat(raw) * const                 -> d raw: mean -> 1/N to every point, max/min -> ties share evenly
//   raw statistics depend on Q_ng, z_ng    -> dQ_ng and the direct part of dz_ng
//   Q_ng = wp_ng / sum_g wp_ng             -> through the normalisation: dz_ngd -= z_ngd Q_ng (dQ_ng - T_n),
//                                             T_n = sum_g dQ_ng Q_ng ;   dx_n = sum_g dz_ng / sigma
// Mapping of every kernel but the combine (1024 threads; wave <-> 32 Gaussians, lane>>5 <-> half of the points), so the per-
// Gaussian gradient record (20 + 20 floats) lives in REGISTERS; the per-point sums over Gaussians are 32-lane
// xor-shuffle reductions + a fixed-order sum over the 16 waves.  Needs G <= 512 (m <= 8).
#include "mfv3d_int.h"
#include "patch_rows_bwd.h"

namespace dpd {

// this lane's Gaussian and its half of the points
struct BwdLane {
    int lane, wave, half, g, gi, gj, gt;
    bool live;
    __device__ __forceinline__ BwdLane(int tid, int G, int m) {
        lane = tid & 63; wave = tid >> 6; half = lane >> 5;
        g = wave * 32 + (lane & 31);
        live = g < G;
        const int gg = live ? g : 0;
        gi = gg / (m * m); gj = (gg / m) % m; gt = gg % m;
    }
};

// the tables of np_ points as this lane reads them, and the half-wave's share [nbeg, nend) of those points
struct BwdTables {
    const float2 *x, *y, *z;
    int m, nbeg, nend;
    __device__ __forceinline__ BwdTables(const float2* s_zq, int np_, int m_, const BwdLane& L) {
        x = s_zq; y = s_zq + np_ * m_; z = s_zq + 2 * np_ * m_; m = m_;
        const int hpts = (np_ + 1) / 2;
        nbeg = L.half * hpts; nend = min(np_, (L.half + 1) * hpts);
    }
    __device__ __forceinline__ PQ at(int n, const BwdLane& L, float w, float inv_dpi) const {
        return eval_pq(x[n * m + L.gj], y[n * m + L.gi], z[n * m + L.gt], w, inv_dpi);
    }
};

// dz_ngd = Q (ga + 2 gb z) - z Q u, u = dQ - T_n, summed over the 32 Gaussians of the half-wave: its last lane leaves the sums in row[3]
__device__ __forceinline__ void store_dz(const PQ& q, const float* ga, const float* gb, float u, const BwdLane& L, float* row) {
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const float dz = L.live ? q.Q * (ga[d] + 2.0f * gb[d] * q.z[d]) - q.z[d] * q.Q * u : 0.f;
        const float s = half_sum32_hi(dz);
        if ((L.lane & 31) == 31) row[d] = s;
    }
}

// ------------------------------------------------------------------------------------------------------
// One launch, one workgroup per cloud.
// dynamic LDS (floats): zq[6*N*m] | S[3*N] | chred[16*40] | ch[40] | T[N] | part[16*N*3]
// (Its lane variables, point loops, T_n sum and dz store are spelled out: with BwdLane / BwdTables / store_dz / sum16 in their place
//  the kernel came out at 73 or 77 VGPRs instead of 76, EXPERIMENTS G13.)
// ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kFwdThreads) void mfv3d_bwd_kernel(const float* __restrict__ pts, const float* __restrict__ dfv,
                                                                 float* __restrict__ dpts, MfvConst k) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int N = k.N, G = k.G, m = k.m;
    float2* s_zq = reinterpret_cast<float2*>(sm);   // [3][N][m]
    float* s_S = sm + 6 * N * m;                    // [3][N]
    float* s_chred = s_S + 3 * N;                   // [16][40]
    float* s_ch = s_chred + 16 * 2 * kF;            // [40]: ss_f, dot_f
    float* s_T = s_ch + 2 * kF;                     // [N]
    float* s_part = s_T + N;                        // [16][N][3]

    const int tid = threadIdx.x, c = blockIdx.x;
    const int lane = tid & 63, wave = tid >> 6, half = lane >> 5;
    const float* p = pts + (size_t)c * N * 3;
    build_tables(p, 0, N, k, s_zq, s_S, tid);
    const float2* zqx = s_zq;
    const float2* zqy = s_zq + N * m;
    const float2* zqz = s_zq + 2 * N * m;

    const int g = wave * 32 + (lane & 31);
    const bool live = g < G;
    const int gg = live ? g : 0;
    const int gi = gg / (m * m), gj = (gg / m) % m, gt = gg % m;
    const float invN = 1.0f / (float)N, inv_dpi = 1.0f / k.dpi_den;
    const int hpts = (N + 1) / 2;
    const int nbeg = half * hpts, nend = min(N, (half + 1) * hpts);

    // ---- P1: statistics (both half-waves end up with the merged values) ----------------------------------
    float raw[kF];
    {
        MfvStats st;
        st.init();
        for (int n = nbeg; n < nend; ++n) st.add(eval_pq(zqx[n * m + gj], zqy[n * m + gi], zqz[n * m + gt], k.w, inv_dpi));
        st.fold_halves(raw);
#pragma unroll
        for (int f = 0; f < kF; ++f)
            if (mfv_is_sum(f)) raw[f] = raw[f] * invN;
    }
    // ---- channel sums ss_f = sum_g s^2, dot_f = sum_g s*dfv -------------------------------------------------
    const float* df = dfv + ((size_t)c * G + gg) * kF;
    float dr[kF];   // becomes the gradient w.r.t. the raw statistics
    {
        const bool mine = live && half == 0;
#pragma unroll
        for (int f = 0; f < kF; ++f) {
            const float sv = pnorm(raw[f] * mfv_cst(k, f));
            const float dy = mine ? df[f] : 0.f;
            const float a = wave_sum(mine ? sv * sv : 0.f), b = wave_sum(sv * dy);
            if (lane == 0) { s_chred[wave * 2 * kF + f] = a; s_chred[wave * 2 * kF + kF + f] = b; }
        }
    }
    __syncthreads();
    if (tid < 2 * kF) {
        s_ch[tid] = sum16(s_chred, 2 * kF, tid);
    }
    __syncthreads();
    // ---- P2: dfv -> gradient w.r.t. the raw statistics -------------------------------------------------------
#pragma unroll
    for (int f = 0; f < kF; ++f) {
        const float d = d_raw(f, raw[f], s_ch[f], s_ch[kF + f], live ? df[f] : 0.f, k, invN);
        dr[f] = live ? d : 0.f;
    }
    // ---- P1b: tie counts of the max/min statistics (tf.reduce_max/min split the gradient evenly) --------------
    {
        float cnt[13];
#pragma unroll
        for (int i = 0; i < 13; ++i) cnt[i] = 0.f;
        for (int n = nbeg; n < nend; ++n) {
            const PQ q = eval_pq(zqx[n * m + gj], zqy[n * m + gi], zqz[n * m + gt], k.w, inv_dpi);
            count_ties(cnt, q, raw);
        }
        const int mm[13] = {1, 5, 6, 7, 8, 9, 10, 14, 15, 16, 17, 18, 19};
#pragma unroll
        for (int i = 0; i < 13; ++i) {
            const float ctot = sum_x32(cnt[i]);
            dr[mm[i]] = dr[mm[i]] / fmaxf(ctot, 1.f);
        }
    }
    // ---- P3: T_n = sum_g dQ_ng Q_ng ---------------------------------------------------------------------------
    for (int n = nbeg; n < nend; ++n) {
        const PQ q = eval_pq(zqx[n * m + gj], zqy[n * m + gi], zqz[n * m + gt], k.w, inv_dpi);
        float ga[3], gb[3];
        const float dQ = tie_grad(dr, raw, q, inv_dpi, ga, gb);
        const float t = half_sum32_hi(live ? dQ * q.Q : 0.f);
        if ((lane & 31) == 31) s_part[wave * N + n] = t;
    }
    __syncthreads();
    for (int n = tid; n < N; n += kFwdThreads) {
        float t = 0.f;
#pragma unroll
        for (int w = 0; w < 16; ++w) t += s_part[w * N + n];
        s_T[n] = t;
    }
    __syncthreads();
    // ---- P4: dz_ngd = Q (ga + 2 gb z) - z Q (dQ - T_n), summed over the Gaussians ------------------------------
    for (int n = nbeg; n < nend; ++n) {
        const PQ q = eval_pq(zqx[n * m + gj], zqy[n * m + gi], zqz[n * m + gt], k.w, inv_dpi);
        float ga[3], gb[3];
        const float dQ = tie_grad(dr, raw, q, inv_dpi, ga, gb);
        const float u = dQ - s_T[n];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const float dz = live ? q.Q * (ga[d] + 2.0f * gb[d] * q.z[d]) - q.z[d] * q.Q * u : 0.f;
            const float t = half_sum32_hi(dz);
            if ((lane & 31) == 31) s_part[(wave * N + n) * 3 + d] = t;
        }
    }
    __syncthreads();
    float* out = dpts + (size_t)c * N * 3;
    for (int i = tid; i < N * 3; i += kFwdThreads) {
        out[i] = sum16(s_part, N * 3, i) / k.sigma;   // z = (x - mu)/sigma
    }
}

// ------------------------------------------------------------------------------------------------------
// Backward, sliced over the POINTS: kSlices workgroups per cloud (a single workgroup per cloud leaves 3/4 of the chip idle
// at the as-loss batch sizes: 32 clouds at B = 16).  Everything that is a sum over Gaussians for a fixed point (T_n, dx_n)
// is local to the point's slice; the only cross-slice quantity is the per-Gaussian statistic record (7 sums, 7 maxima,
// 6 minima over the points + how many points attain each extreme), exchanged through `part`:
//   mfv3d_bwd_stats_kernel   slice -> part[c][s][33][G]    (sum / max / min over the slice's points, local tie counts)
//   mfv3d_bwd_combine_kernel one workgroup per cloud: merges the records, channel sums, d raw statistics (in place over slice 0)
//   mfv3d_bwd_apply_kernel   (was: every slice combined the kSlices records itself; ties: counts of the slices whose extreme equals the global
//                            one), then runs P2-P4 of mfv3d_bwd_kernel for its own points and writes their dpts.
// Same per-(point, Gaussian) expressions as the monolithic kernel -> identical tie tests; sums differ by association.
// ------------------------------------------------------------------------------------------------------

__device__ __forceinline__ void mfv3d_bwd_stats_block(const float* __restrict__ pts, float* __restrict__ part, const MfvConst& k, int nslice,
                                                      int c, int sl, float* sm) {
    const int N = k.N, G = k.G, m = k.m;
    const int n0 = min(N, sl * nslice), np_ = min(N, n0 + nslice) - n0;
    float2* s_zq = reinterpret_cast<float2*>(sm);   // [3][np_][m]
    float* s_S = sm + 6 * nslice * m;
    const int tid = threadIdx.x;
    const BwdLane L(tid, G, m);
    build_tables(pts + (size_t)c * N * 3, n0, np_, k, s_zq, s_S, tid);
    const BwdTables t(s_zq, np_, m, L);
    const float inv_dpi = 1.0f / k.dpi_den;
    float rec[kRec];
    {
        MfvStats st;
        st.init();
        for (int n = t.nbeg; n < t.nend; ++n) st.add(t.at(n, L, k.w, inv_dpi));
        st.fold_halves(rec);            // SUMS here (the mean's 1/N is applied after the combine)
    }
    {
        float cnt[13];
#pragma unroll
        for (int i = 0; i < 13; ++i) cnt[i] = 0.f;
        for (int n = t.nbeg; n < t.nend; ++n) count_ties(cnt, t.at(n, L, k.w, inv_dpi), rec);
#pragma unroll
        for (int i = 0; i < 13; ++i) rec[20 + i] = sum_x32(cnt[i]);
    }
    if (L.live && L.half == 0) {        // the slice's record of this lane's Gaussian -> part[c][sl][row][g]
        float* out = part + ((size_t)(c * kSlices + sl) * kRec) * G + L.g;
#pragma unroll
        for (int i = 0; i < kRec; ++i) out[(size_t)i * G] = rec[i];
    }
}

__global__ __launch_bounds__(kFwdThreads) void mfv3d_bwd_stats_kernel(const float* __restrict__ pts, float* __restrict__ part,
                                                                       MfvConst k, int nslice) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    mfv3d_bwd_stats_block(pts, part, k, nslice, blockIdx.x / kSlices, blockIdx.x % kSlices, sm);
}

// As-loss backward (asloss.hip): the window-gather backward (dX -> dfv; patch_rows_bwd.h) and the statistics pass above read nothing of each
// other, so they share ONE launch -- workgroups [0, ngather) gather, the rest take the statistics of their point slice (the two used to be
// 17 + 12 us of latency-bound launches back to back at the PCRNet batch).  Same routines, same bits.
__global__ __launch_bounds__(kFwdThreads) void asloss_tail_a_kernel(const float* __restrict__ dX, const int32_t* __restrict__ vox,
                                                                     float* __restrict__ dfv, const float* __restrict__ pts,
                                                                     float* __restrict__ part, MfvConst k, int nslice, int kwin, int KP,
                                                                     int gslices, int ngather) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    if ((int)blockIdx.x < ngather) {
        patch_rows_bwd_block<kFwdThreads>(dX, vox, dfv, k.N, k.m, kwin, KP, blockIdx.x / gslices, blockIdx.x % gslices, gslices,
                                          reinterpret_cast<int*>(sm));
    } else {
        const int b = blockIdx.x - ngather;
        mfv3d_bwd_stats_block(pts, part, k, nslice, b / kSlices, b % kSlices, sm);
    }
}

// Per-cloud combine (thread = Gaussian): merges the kSlices statistic records, takes the channel sums over
// ALL Gaussians, and turns dfv into the gradient w.r.t. the 20 raw statistics of every Gaussian.  This is the sqrt / divide heavy
// part of the backward; it used to be repeated by both half-waves of every one of the kSlices apply workgroups (8x).  Output, in
// place over slice 0's record of the cloud (every thread only touches its own column g): rows 0..19 = d raw statistic (tie
// counts already divided in), rows 20..32 = the 13 global extrema the apply kernel needs for its tie tests.
// (round 3) FOUR workgroups per cloud, five of the 20 statistics each: the channel sums are per statistic, so the quarters never talk to
// each other, every thread requests 24-40 record values instead of 132 (the loads of one workgroup per cloud went through ONE CU's
// address unit: ~17k cycles of this kernel's 18.9 us at the PCRNet batch), and 128 workgroups instead of 32 share the square roots.
// Same expressions per statistic, same summation orders: the same bits.
template <int F0>
__device__ __forceinline__ void mfv3d_bwd_combine_quarter(const float* __restrict__ dfv, float* __restrict__ part, const MfvConst& k, int c,
                                                          float* s_chred, float* s_ch) {
    constexpr int NF = 5;
    const int N = k.N, G = k.G;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = tid;
    const bool live = g < G;
    const int gg = live ? g : 0;
    const float invN = 1.0f / (float)N;
    const float* pc = part + (size_t)c * kSlices * kRec * G + gg;
    float r[kSlices][NF], rt[kSlices][NF];
#pragma unroll
    for (int s2 = 0; s2 < kSlices; ++s2)
#pragma unroll
        for (int j = 0; j < NF; ++j) {
            r[s2][j] = pc[((size_t)s2 * kRec + (F0 + j)) * G];
            rt[s2][j] = 0.f;
        }
#pragma unroll
    for (int s2 = 0; s2 < kSlices; ++s2)
#pragma unroll
        for (int j = 0; j < NF; ++j)
            if (mfv_tie_index(F0 + j) >= 0) rt[s2][j] = pc[((size_t)s2 * kRec + 20 + mfv_tie_index(F0 + j)) * G];
    float raw[NF], cnt[NF];
#pragma unroll
    for (int j = 0; j < NF; ++j) {
        const int f = F0 + j;
        float v = r[0][j];
#pragma unroll
        for (int s2 = 1; s2 < kSlices; ++s2) v = mfv_is_sum(f) ? v + r[s2][j] : (mfv_is_max(f) ? fmaxf(v, r[s2][j]) : fminf(v, r[s2][j]));
        raw[j] = mfv_is_sum(f) ? v * invN : v;
        float t = 0.f;      // tie count of an extremum: the slices that attain it contribute theirs
#pragma unroll
        for (int s2 = 0; s2 < kSlices; ++s2) t += (r[s2][j] == raw[j]) ? rt[s2][j] : 0.f;
        cnt[j] = t;
    }
    // ---- channel sums ss_f = sum_g s^2, dot_f = sum_g s*dfv ----
    const float* df = dfv + ((size_t)c * G + gg) * kF;
#pragma unroll
    for (int j = 0; j < NF; ++j) {
        const int f = F0 + j;
        const float sv = pnorm(raw[j] * mfv_cst(k, f));
        const float dy = live ? df[f] : 0.f;
        const float a = wave_sum(live ? sv * sv : 0.f), b = wave_sum(sv * dy);
        if (lane == 0) { s_chred[wave * 2 * NF + j] = a; s_chred[wave * 2 * NF + NF + j] = b; }
    }
    __syncthreads();
    if (tid < 2 * NF) {
        float t = 0.f;
#pragma unroll
        for (int w = 0; w < 8; ++w) t += s_chred[w * 2 * NF + tid];
        s_ch[tid] = t;
    }
    __syncthreads();
    float* out = part + (size_t)c * kSlices * kRec * G + g;      // slice 0's record of this cloud (rows F0 .. F0+4 and their extremum rows)
#pragma unroll
    for (int j = 0; j < NF; ++j) {
        const int f = F0 + j;
        float d = d_raw(f, raw[j], s_ch[j], s_ch[NF + j], live ? df[f] : 0.f, k, invN);
        d = live ? d : 0.f;
        if (mfv_tie_index(f) >= 0) d = d / fmaxf(cnt[j], 1.f);
        if (live) {
            out[(size_t)f * G] = d;
            if (mfv_tie_index(f) >= 0) out[(size_t)(20 + mfv_tie_index(f)) * G] = raw[j];
        }
    }
}

// NOTE on in-place output: quarter q overwrites rows F0..F0+4 and the extremum rows of ITS statistics in slice 0's record, which no
// other quarter reads (each reads only its own statistic and tie rows), so the four workgroups of a cloud need no ordering.
__device__ __forceinline__ void mfv3d_bwd_combine_block(const float* __restrict__ dfv, float* __restrict__ part, const MfvConst& k) {
    __shared__ float s_chred[8 * 2 * 5];
    __shared__ float s_ch[2 * 5];
    const int c = blockIdx.x >> 2;
    switch (blockIdx.x & 3) {
        case 0: mfv3d_bwd_combine_quarter<0>(dfv, part, k, c, s_chred, s_ch); break;
        case 1: mfv3d_bwd_combine_quarter<5>(dfv, part, k, c, s_chred, s_ch); break;
        case 2: mfv3d_bwd_combine_quarter<10>(dfv, part, k, c, s_chred, s_ch); break;
        default: mfv3d_bwd_combine_quarter<15>(dfv, part, k, c, s_chred, s_ch); break;
    }
}
__global__ __launch_bounds__(512) void mfv3d_bwd_combine_kernel(const float* __restrict__ dfv, float* __restrict__ part, MfvConst k) {
    mfv3d_bwd_combine_block(dfv, part, k);
}
// dpd_mfv3d_bwd_counts: the same quarters with the cloud's own (clamped) count behind the mean statistics' 1 / N
__global__ __launch_bounds__(512) void mfv3d_bwd_combine_counts_kernel(const float* __restrict__ dfv, const int32_t* __restrict__ counts,
                                                                       float* __restrict__ part, MfvConst k) {
    k.N = min(max(counts[blockIdx.x >> 2], 1), k.N);
    mfv3d_bwd_combine_block(dfv, part, k);
}

// the slice's (or tile's) dx of element i = point * 3 + axis from the 16 waves' partial sums store_dz left
__device__ __forceinline__ float dx_from_parts(const float* s_part, int stride, int i, float sigma) {
    return sum16(s_part, stride * 3, i) / sigma;   // z = (x - mu)/sigma
}

template <bool FINAL>
__global__ __launch_bounds__(kFwdThreads) void mfv3d_bwd_apply_kernel(const float* __restrict__ pts, const float* __restrict__ comb,
                                                                       float* __restrict__ dpts, MfvConst k, int nslice, AslossFinal fin) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int N = k.N, G = k.G, m = k.m;
    const int c = blockIdx.x / kSlices, sl = blockIdx.x % kSlices;
    const int n0 = min(N, sl * nslice), np_ = min(N, n0 + nslice) - n0;
    float2* s_zq = reinterpret_cast<float2*>(sm);   // [3][np_][m]
    float* s_S = sm + 6 * nslice * m;               // [3][nslice]
    float* s_T = s_S + 3 * nslice;                  // [nslice]
    float* s_part = s_T + nslice;                   // [16][nslice][3]
    const int tid = threadIdx.x;
    const BwdLane L(tid, G, m);
    build_tables(pts + (size_t)c * N * 3, n0, np_, k, s_zq, s_S, tid);
    const BwdTables t(s_zq, np_, m, L);
    // d raw statistic and the global extrema of this lane's Gaussian, from mfv3d_bwd_combine_kernel (spelled out: as a routine it changed the
    // kernel's register count, EXPERIMENTS G13)
    float dr[kF], raw[kF];
    {
        const float* pc = comb + (size_t)c * kSlices * kRec * G + (L.live ? L.g : 0);
        const int mm[13] = {1, 5, 6, 7, 8, 9, 10, 14, 15, 16, 17, 18, 19};
#pragma unroll
        for (int f = 0; f < kF; ++f) { dr[f] = L.live ? pc[(size_t)f * G] : 0.f; raw[f] = 0.f; }
#pragma unroll
        for (int i = 0; i < 13; ++i) raw[mm[i]] = pc[(size_t)(20 + i) * G];
    }
    // ---- T_n and dz for the slice's own points (as P3 / P4 of mfv3d_bwd_kernel) ----------------------------------
    const float inv_dpi = 1.0f / k.dpi_den;
    for (int n = t.nbeg; n < t.nend; ++n) {
        const PQ q = t.at(n, L, k.w, inv_dpi);
        float ga[3], gb[3];
        const float dQ = tie_grad(dr, raw, q, inv_dpi, ga, gb);
        const float sT = half_sum32_hi(L.live ? dQ * q.Q : 0.f);
        if ((L.lane & 31) == 31) s_part[L.wave * nslice + n] = sT;
    }
    __syncthreads();
    for (int n = tid; n < np_; n += kFwdThreads) s_T[n] = sum16(s_part, nslice, n);
    __syncthreads();
    for (int n = t.nbeg; n < t.nend; ++n) {
        const PQ q = t.at(n, L, k.w, inv_dpi);
        float ga[3], gb[3];
        const float u = tie_grad(dr, raw, q, inv_dpi, ga, gb) - s_T[n];
        store_dz(q, ga, gb, u, L, s_part + (L.wave * nslice + n) * 3);
    }
    __syncthreads();
    float* out = FINAL ? nullptr : dpts + ((size_t)c * N + n0) * 3;
    for (int i = tid; i < np_ * 3; i += kFwdThreads) {
        const float v = dx_from_parts(s_part, nslice, i, k.sigma);
        if (FINAL) {
            const int which = c >= fin.B ? 1 : 0, BN = fin.B * N;
            const int r = (c - which * fin.B) * N + n0 + i / 3, d = i % 3;
            const int qrow = which ? r : BN + r;
            const float sc = fin.scale ? *fin.scale : 1.0f;
            (which ? fin.gB : fin.gA)[(size_t)r * 3 + d] = (v + fin.dX[(size_t)qrow * fin.KP + fin.E + d]) * sc;
        } else {
            out[i] = v;
        }
    }
}

// ------------------------------------------------------------------------------------------------------
// Backward over tiles (why: "The encoder over TILES of points" in mfv3d.hip): the three-launch structure and the workspace layout of the
// sliced form (kSlices records of kRec rows per cloud; mfv3d_bwd_combine_kernel runs unchanged in between).  Each of the kSlices point
// slices walks its ceil(N / kSlices) points in tiles.
//   statistics: tiles once for the sums / maxima / minima, tiles AGAIN for the 13 tie counts against the slice's extrema (tables rebuilt by
//               the same code, the same eval_pq expressions: equality is exact), one record per slice;
//   apply:      per tile tables -> T_n -> dx_n of the tile's points -> store; a tile needs nothing of the other tiles beyond the combined record.
// The routines of the sliced form: with one tile per slice, its bits (tests/test_mfv_units_gpu.py).
// All sums in a fixed order, no float atomics.  An empty slice (or tile count 0) writes the -inf / +inf / 0 record, as the sliced form does.
// dynamic LDS (floats): statistics zq[6*tile*m] | S[3*tile]; apply zq[6*tile*m] | S[3*tile] | T[tile] | part[16*tile*3]
// CNT (dpd_mfv3d_bwd_counts): as in the forward, N is the cloud's clamped count; its point slices are ceil(N / kSlices) points each (the
// slices a cloud of that size has alone), the row stride stays k.N, and the apply kernel writes +0.0 over the padded rows of dpts.
// ------------------------------------------------------------------------------------------------------
// (This body keeps its own lane variables, accumulator, fold and tie counts: over BwdLane / BwdTables / MfvStats / count_ties, as
//  mfv3d_bwd_stats_block is, it had the same registers and code size but other instructions, and 112.8 us per launch against 111.8
//  in the encoder benchmark -- the whole of what the tiled backward lost against the form before the split, EXPERIMENTS G13.)
template <bool CNT>
__device__ __forceinline__ void mfv3d_bwd_stats_tiled_body(const float* __restrict__ pts, float* __restrict__ part, const MfvConst& k,
                                                           int nslice_full, int tile, const int32_t* __restrict__ counts, float sqw) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int G = k.G, m = k.m;
    const int c = blockIdx.x / kSlices, sl = blockIdx.x % kSlices;
    const int N = CNT ? min(max(counts[c], 1), k.N) : k.N;
    const int nslice = CNT ? (N + kSlices - 1) / kSlices : nslice_full;
    const int n0 = min(N, sl * nslice), np_ = min(N, n0 + nslice) - n0;
    float2* s_zq = reinterpret_cast<float2*>(sm);   // [3][tp][m], tp <= tile
    float* s_S = sm + 6 * tile * m;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5;
    const float* p = pts + (size_t)c * k.N * 3;
    const int g = wave * 32 + (lane & 31);
    const bool live = g < G;
    const int gg = live ? g : 0;
    const int gi = gg / (m * m), gj = (gg / m) % m, gt = gg % m;
    const float inv_dpi = 1.0f / (CNT ? sqw * (float)N : k.dpi_den);
    float rec[kRec];
    {
        float pi_s = 0.f, pi_mx = -INFINITY;
        float mu_s[3] = {0.f, 0.f, 0.f}, mu_mx[3] = {-INFINITY, -INFINITY, -INFINITY}, mu_mn[3] = {INFINITY, INFINITY, INFINITY};
        float sg_s[3] = {0.f, 0.f, 0.f}, sg_mx[3] = {-INFINITY, -INFINITY, -INFINITY}, sg_mn[3] = {INFINITY, INFINITY, INFINITY};
        for (int t0 = 0; t0 < np_; t0 += tile) {
            const int tp = min(tile, np_ - t0);
            build_tables(p, n0 + t0, tp, k, s_zq, s_S, tid);
            const float2* zqx = s_zq;
            const float2* zqy = s_zq + tp * m;
            const float2* zqz = s_zq + 2 * tp * m;
            const int hpts = (tp + 1) / 2;
            const int nbeg = half * hpts, nend = min(tp, (half + 1) * hpts);
            for (int n = nbeg; n < nend; ++n) {
                const PQ q = eval_pq(zqx[n * m + gj], zqy[n * m + gi], zqz[n * m + gt], k.w, inv_dpi);
                pi_s += q.dpi; pi_mx = fmaxf(pi_mx, q.dpi);
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    mu_s[d] += q.a[d]; mu_mx[d] = fmaxf(mu_mx[d], q.a[d]); mu_mn[d] = fminf(mu_mn[d], q.a[d]);
                    sg_s[d] += q.b[d]; sg_mx[d] = fmaxf(sg_mx[d], q.b[d]); sg_mn[d] = fminf(sg_mn[d], q.b[d]);
                }
            }
            __syncthreads();    // the next tile overwrites the tables
        }
        rec[0] = sum_x32(pi_s);            // SUMS here (the mean's 1/N is applied after the combine)
        rec[1] = max_x32(pi_mx);
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            rec[2 + d] = sum_x32(mu_s[d]);
            rec[5 + d] = max_x32(mu_mx[d]);
            rec[8 + d] = min_x32(mu_mn[d]);
            rec[11 + d] = sum_x32(sg_s[d]);
            rec[14 + d] = max_x32(sg_mx[d]);
            rec[17 + d] = min_x32(sg_mn[d]);
        }
    }
    {
        float cnt[13];
#pragma unroll
        for (int i = 0; i < 13; ++i) cnt[i] = 0.f;
        for (int t0 = 0; t0 < np_; t0 += tile) {
            const int tp = min(tile, np_ - t0);
            build_tables(p, n0 + t0, tp, k, s_zq, s_S, tid);
            const float2* zqx = s_zq;
            const float2* zqy = s_zq + tp * m;
            const float2* zqz = s_zq + 2 * tp * m;
            const int hpts = (tp + 1) / 2;
            const int nbeg = half * hpts, nend = min(tp, (half + 1) * hpts);
            for (int n = nbeg; n < nend; ++n) {
                const PQ q = eval_pq(zqx[n * m + gj], zqy[n * m + gi], zqz[n * m + gt], k.w, inv_dpi);
                cnt[0] += (q.dpi == rec[1]) ? 1.f : 0.f;
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    cnt[1 + d] += (q.a[d] == rec[5 + d]) ? 1.f : 0.f;
                    cnt[4 + d] += (q.a[d] == rec[8 + d]) ? 1.f : 0.f;
                    cnt[7 + d] += (q.b[d] == rec[14 + d]) ? 1.f : 0.f;
                    cnt[10 + d] += (q.b[d] == rec[17 + d]) ? 1.f : 0.f;
                }
            }
            __syncthreads();
        }
#pragma unroll
        for (int i = 0; i < 13; ++i) rec[20 + i] = sum_x32(cnt[i]);
    }
    if (live && half == 0) {
        float* out = part + ((size_t)(c * kSlices + sl) * kRec) * G + g;
#pragma unroll
        for (int i = 0; i < kRec; ++i) out[(size_t)i * G] = rec[i];
    }
}

__global__ __launch_bounds__(kFwdThreads) void mfv3d_bwd_stats_tiled_kernel(const float* __restrict__ pts, float* __restrict__ part,
                                                                             MfvConst k, int nslice, int tile) {
    mfv3d_bwd_stats_tiled_body<false>(pts, part, k, nslice, tile, nullptr, 0.f);
}
__global__ __launch_bounds__(kFwdThreads) void mfv3d_bwd_stats_counts_kernel(const float* __restrict__ pts, const int32_t* __restrict__ counts,
                                                                              float* __restrict__ part, MfvConst k, int nslice, int tile,
                                                                              float sqw) {
    mfv3d_bwd_stats_tiled_body<true>(pts, part, k, nslice, tile, counts, sqw);
}

template <bool CNT>
__device__ __forceinline__ void mfv3d_bwd_apply_tiled_body(const float* __restrict__ pts, const float* __restrict__ comb,
                                                           float* __restrict__ dpts, const MfvConst& k, int nslice_full, int tile,
                                                           const int32_t* __restrict__ counts, float sqw) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int G = k.G, m = k.m;
    // the point slice [n0, n0 + np_) of this workgroup, the cloud's own N and its 1 / (sqrt(w) N)
    const int c = blockIdx.x / kSlices, sl = blockIdx.x % kSlices;
    const int N = CNT ? min(max(counts[c], 1), k.N) : k.N;
    const int nslice = CNT ? (N + kSlices - 1) / kSlices : nslice_full;
    const int n0 = min(N, sl * nslice), np_ = min(N, n0 + nslice) - n0;
    const float inv_dpi = 1.0f / (CNT ? sqw * (float)N : k.dpi_den);
    float2* s_zq = reinterpret_cast<float2*>(sm);   // [3][tp][m]
    float* s_S = sm + 6 * tile * m;                 // [3][tile]
    float* s_T = s_S + 3 * tile;                    // [tile]
    float* s_part = s_T + tile;                     // [16][tile][3]
    const int tid = threadIdx.x;
    const float* p = pts + (size_t)c * k.N * 3;
    const BwdLane L(tid, G, m);
    if (CNT) {      // the padded rows of this cloud, shared among its kSlices workgroups: +0.0
        float* pad = dpts + (size_t)c * k.N * 3;
        for (int i = N * 3 + sl * kFwdThreads + tid; i < k.N * 3; i += kSlices * kFwdThreads) pad[i] = 0.f;
    }
    // d raw statistic and the global extrema of this lane's Gaussian, from mfv3d_bwd_combine_kernel (spelled out: as a routine it changed the
    // kernel's register count, EXPERIMENTS G13)
    float dr[kF], raw[kF];
    {
        const float* pc = comb + (size_t)c * kSlices * kRec * G + (L.live ? L.g : 0);
        const int mm[13] = {1, 5, 6, 7, 8, 9, 10, 14, 15, 16, 17, 18, 19};
#pragma unroll
        for (int f = 0; f < kF; ++f) { dr[f] = L.live ? pc[(size_t)f * G] : 0.f; raw[f] = 0.f; }
#pragma unroll
        for (int i = 0; i < 13; ++i) raw[mm[i]] = pc[(size_t)(20 + i) * G];
    }
    for (int t0 = 0; t0 < np_; t0 += tile) {
        const int tp = min(tile, np_ - t0);
        build_tables(p, n0 + t0, tp, k, s_zq, s_S, tid);
        const BwdTables t(s_zq, tp, m, L);
        // ---- T_n and dz for the tile's points (as P3 / P4 of mfv3d_bwd_kernel) ----------------------------------
        for (int n = t.nbeg; n < t.nend; ++n) {      // (P3 spelled out too: with tie_grad here the tiled backward measured slower, G13)
            const PQ q = t.at(n, L, k.w, inv_dpi);
            float dQ = (dr[0] + ((q.dpi == raw[1]) ? dr[1] : 0.f)) * inv_dpi;
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                const float ga = dr[2 + d] + ((q.a[d] == raw[5 + d]) ? dr[5 + d] : 0.f) + ((q.a[d] == raw[8 + d]) ? dr[8 + d] : 0.f);
                const float gb = dr[11 + d] + ((q.b[d] == raw[14 + d]) ? dr[14 + d] : 0.f) + ((q.b[d] == raw[17 + d]) ? dr[17 + d] : 0.f);
                dQ += ga * q.z[d] + gb * (q.z[d] * q.z[d] - 1.0f);
            }
            const float sT = half_sum32_hi(L.live ? dQ * q.Q : 0.f);
            if ((L.lane & 31) == 31) s_part[L.wave * tile + n] = sT;
        }
        __syncthreads();
        for (int n = tid; n < tp; n += kFwdThreads) s_T[n] = sum16(s_part, tile, n);
        __syncthreads();
        for (int n = t.nbeg; n < t.nend; ++n) {
            const PQ q = t.at(n, L, k.w, inv_dpi);
            // (spelled out: tie_grad here changed the kernel's register count and occupancy, EXPERIMENTS G13)
            float dQ = (dr[0] + ((q.dpi == raw[1]) ? dr[1] : 0.f)) * inv_dpi;
            float ga[3], gb[3];
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                ga[d] = dr[2 + d] + ((q.a[d] == raw[5 + d]) ? dr[5 + d] : 0.f) + ((q.a[d] == raw[8 + d]) ? dr[8 + d] : 0.f);
                gb[d] = dr[11 + d] + ((q.b[d] == raw[14 + d]) ? dr[14 + d] : 0.f) + ((q.b[d] == raw[17 + d]) ? dr[17 + d] : 0.f);
                dQ += ga[d] * q.z[d] + gb[d] * (q.z[d] * q.z[d] - 1.0f);
            }
            store_dz(q, ga, gb, dQ - s_T[n], L, s_part + (L.wave * tile + n) * 3);
        }
        __syncthreads();
        float* out = dpts + ((size_t)c * k.N + n0 + t0) * 3;
        for (int i = tid; i < tp * 3; i += kFwdThreads) out[i] = dx_from_parts(s_part, tile, i, k.sigma);
        __syncthreads();        // the next tile overwrites the tables and the partial sums
    }
}

__global__ __launch_bounds__(kFwdThreads) void mfv3d_bwd_apply_tiled_kernel(const float* __restrict__ pts, const float* __restrict__ comb,
                                                                             float* __restrict__ dpts, MfvConst k, int nslice, int tile) {
    mfv3d_bwd_apply_tiled_body<false>(pts, comb, dpts, k, nslice, tile, nullptr, 0.f);
}
__global__ __launch_bounds__(kFwdThreads) void mfv3d_bwd_apply_counts_kernel(const float* __restrict__ pts, const int32_t* __restrict__ counts,
                                                                              const float* __restrict__ comb, float* __restrict__ dpts,
                                                                              MfvConst k, int nslice, int tile, float sqw) {
    mfv3d_bwd_apply_tiled_body<true>(pts, comb, dpts, k, nslice, tile, counts, sqw);
}

// ---- host ------------------------------------------------------------------------------------------------------------------
// statistics -> combine -> apply, C * kSlices / C * 4 / C * kSlices workgroups; stats / apply: the launches of the form, which differ in
// their kernels and arguments
template <auto Stats, auto Apply, typename LS, typename LC, typename LA>
static int launch_three(size_t l1, size_t l2, LS stats, LC combine, LA apply) {
    if (int rc = set_lds<Stats>(l1)) return rc;
    if (int rc = set_lds<Apply>(l2)) return rc;
    stats();
    DPD_CHECK_LAUNCH();
    combine();
    DPD_CHECK_LAUNCH();
    apply();
    DPD_CHECK_LAUNCH();
    return 0;
}

}  // namespace dpd

using namespace dpd;

extern "C" size_t dpd_mfv3d_bwd_workspace_bytes(int C, int m) {
    return (size_t)(C > 0 ? C : 0) * kSlices * kRec * (size_t)(m * m * m) * sizeof(float);
}

extern "C" int dpd_mfv3d_bwd(const float* pts, const float* dfv, int C, int N, int m, float sigma, float* dpts, void* ws,
                             size_t ws_bytes, void* stream) {
    if (!pts || !dfv || !dpts) return DPD_E_NULL;
    if (C <= 0) return DPD_E_DIM;
    MfvConst k{};
    if (int rc = make_const(N, m, sigma, k)) return rc;
    if (k.G > 512) return DPD_E_UNSUPPORTED;   // per-Gaussian gradient record lives in registers: one Gaussian per lane pair
    hipStream_t s = (hipStream_t)stream;
    if (ws && ws_bytes >= dpd_mfv3d_bwd_workspace_bytes(C, m) && N >= 2 * kSlices) {
        // sliced over the points: kSlices workgroups per cloud, per-Gaussian statistic records exchanged through `ws`
        const int nslice = (N + kSlices - 1) / kSlices;
        const size_t l1 = bwd_stats_lds_bytes(nslice, m), l2 = bwd_sliced_lds_bytes(nslice, m);
        const dim3 slices(C * kSlices), block(kFwdThreads);
        return launch_three<mfv3d_bwd_stats_kernel, mfv3d_bwd_apply_kernel<false>>(
            l1, l2, [&] { DPD_LAUNCH(mfv3d_bwd_stats_kernel, slices, block, l1, s, pts, (float*)ws, k, nslice); },
            [&] { DPD_LAUNCH(mfv3d_bwd_combine_kernel, dim3(C * 4), dim3(512), 0, s, dfv, (float*)ws, k); },
            [&] { DPD_LAUNCH(mfv3d_bwd_apply_kernel<false>, slices, block, l2, s, pts, (const float*)ws, dpts, k, nslice, AslossFinal{}); });
    }
    const size_t lds = bwd_lds_bytes(N, m);
    if (int rc = set_lds<mfv3d_bwd_kernel>(lds)) return rc;
    DPD_LAUNCH(mfv3d_bwd_kernel, dim3(C), dim3(kFwdThreads), lds, s, pts, dfv, dpts, k);
    DPD_CHECK_LAUNCH();
    return 0;
}

// the tiled entry and its per-cloud-count twin (counts = NULL: the tiled entry, its kernels and its bits)
static int bwd_tiled(const float* pts, const int32_t* counts, const float* dfv, int C, int N, int m, float sigma, int tile, float* dpts,
                     void* ws, size_t ws_bytes, void* stream) {
    if (C <= 0) return DPD_E_DIM;
    MfvConst k{};
    if (int rc = make_const(N, m, sigma, k)) return rc;
    if (k.G > 512) return DPD_E_UNSUPPORTED;   // per-Gaussian gradient record lives in registers: one Gaussian per lane pair
    if (tile > 0 && bwd_sliced_lds_bytes(tile, m) > 160 * 1024) return DPD_E_UNSUPPORTED;          // the tile as given must fit
    const int nslice = (N + kSlices - 1) / kSlices;      // (with counts: the largest slice there can be; the kernels take each cloud's own)
    int T = 0;
    if (int rc = resolve_tile(tile, m, true, nslice, T)) return rc;
    if (!ws || ws_bytes < dpd_mfv3d_bwd_workspace_bytes(C, m)) return DPD_E_WORKSPACE;
    const size_t l1 = bwd_stats_lds_bytes(T, m), l2 = bwd_sliced_lds_bytes(T, m);
    const float sqw = sqrtf(k.w);
    const dim3 slices(C * kSlices), quarters(C * 4), block(kFwdThreads);
    hipStream_t s = (hipStream_t)stream;
    if (counts)
        return launch_three<mfv3d_bwd_stats_counts_kernel, mfv3d_bwd_apply_counts_kernel>(
            l1, l2, [&] { DPD_LAUNCH(mfv3d_bwd_stats_counts_kernel, slices, block, l1, s, pts, counts, (float*)ws, k, nslice, T, sqw); },
            [&] { DPD_LAUNCH(mfv3d_bwd_combine_counts_kernel, quarters, dim3(512), 0, s, dfv, counts, (float*)ws, k); },
            [&] { DPD_LAUNCH(mfv3d_bwd_apply_counts_kernel, slices, block, l2, s, pts, counts, (const float*)ws, dpts, k, nslice, T, sqw); });
    return launch_three<mfv3d_bwd_stats_tiled_kernel, mfv3d_bwd_apply_tiled_kernel>(
        l1, l2, [&] { DPD_LAUNCH(mfv3d_bwd_stats_tiled_kernel, slices, block, l1, s, pts, (float*)ws, k, nslice, T); },
        [&] { DPD_LAUNCH(mfv3d_bwd_combine_kernel, quarters, dim3(512), 0, s, dfv, (float*)ws, k); },
        [&] { DPD_LAUNCH(mfv3d_bwd_apply_tiled_kernel, slices, block, l2, s, pts, (const float*)ws, dpts, k, nslice, T); });
}

extern "C" int dpd_mfv3d_bwd_tiled(const float* pts, const float* dfv, int C, int N, int m, float sigma, int tile, float* dpts, void* ws,
                                   size_t ws_bytes, void* stream) {
    if (!pts || !dfv || !dpts) return DPD_E_NULL;
    return bwd_tiled(pts, nullptr, dfv, C, N, m, sigma, tile, dpts, ws, ws_bytes, stream);
}

// ---- ragged sets: cloud c is the first counts[c] points of its row of N (include/dpdist_capi.h) ----
extern "C" int dpd_mfv3d_bwd_counts(const float* pts, const int32_t* counts, const float* dfv, int C, int N, int m, float sigma, int tile,
                                    float* dpts, void* ws, size_t ws_bytes, void* stream) {
    if (!pts || !counts || !dfv || !dpts) return DPD_E_NULL;
    return bwd_tiled(pts, counts, dfv, C, N, m, sigma, tile, dpts, ws, ws_bytes, stream);
}

// The non-GEMM tail of an as-loss backward in THREE launches instead of six (dpd_patch_rows_bwd + dpd_mfv3d_bwd's three + dpd_asloss_combine):
//   [window-gather backward || encoder statistics]  ->  combine  ->  apply + the two input gradients.
// Bitwise the separate calls (same device routines; tests/test_gpu_parity.py).  DPD_E_UNSUPPORTED for shapes the sliced encoder backward
// does not take (the caller then makes the separate calls).
extern "C" int dpd_asloss_tail(const float* dX, const int32_t* vox, const float* pts, const float* upstream, int B, int N, int m, int k, int KP,
                               float sigma, float* dfv, void* mfv_ws, size_t mfv_ws_bytes, float* gA, float* gB, void* stream) {
    if (!dX || !vox || !pts || !dfv || !mfv_ws || !gA || !gB) return DPD_E_NULL;
    if (B <= 0 || N <= 0) return DPD_E_DIM;
    if (k < 1 || k > 7 || !(k & 1) || N > 8192) return DPD_E_UNSUPPORTED;
    if (KP < k * k * k * kF + 3 || (KP & 3)) return DPD_E_DIM;
    const int C = 2 * B;
    MfvConst kc{};
    if (int rc = make_const(N, m, sigma, kc)) return rc;
    if (kc.G > 512 || N < 2 * kSlices || mfv_ws_bytes < dpd_mfv3d_bwd_workspace_bytes(C, m)) return DPD_E_UNSUPPORTED;
    const int nslice = (N + kSlices - 1) / kSlices;
    const int gslices = (kc.G * 5 + kFwdThreads - 1) / kFwdThreads;      // one (voxel, channel group) item per thread
    const size_t lg = (size_t)N * sizeof(int), l1 = std::max(bwd_stats_lds_bytes(nslice, m), lg), l2 = bwd_sliced_lds_bytes(nslice, m);
    hipStream_t s = (hipStream_t)stream;
    return launch_three<asloss_tail_a_kernel, mfv3d_bwd_apply_kernel<true>>(
        l1, l2,
        [&] { DPD_LAUNCH(asloss_tail_a_kernel, dim3(C * gslices + C * kSlices), dim3(kFwdThreads), l1, s, dX, vox, dfv, pts, (float*)mfv_ws, kc,
                         nslice, k, KP, gslices, C * gslices); },
        [&] { DPD_LAUNCH(mfv3d_bwd_combine_kernel, dim3(C * 4), dim3(512), 0, s, (const float*)dfv, (float*)mfv_ws, kc); },
        [&] { DPD_LAUNCH(mfv3d_bwd_apply_kernel<true>, dim3(C * kSlices), dim3(kFwdThreads), l2, s, pts, (const float*)mfv_ws, (float*)nullptr, kc,
                         nslice, AslossFinal{dX, upstream, gA, gB, B, KP, k * k * k * kF}); });
}

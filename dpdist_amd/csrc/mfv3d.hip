// 3D modified Fisher Vector encoder, FORWARD, one workgroup per cloud and slice of the Gaussians.  (Backward: mfv3d_bwd.hip; what the
// two units share -- constants, the per-(point, Gaussian) expressions, the statistics accumulator, the tables, LDS sizes: mfv3d_int.h.)
//
// Replaces utils/dpdist_util.py:22-141 (get_3dmfv_tf with full_fv=True, normalize=True); mfv3d_bwd.hip replaces its TF autodiff.
//
// Data layout in HBM: pts [C,N,3] fp32 (768 B per 64-point cloud), fv [C,G,20] fp32 (40 KB per cloud for m=8).
// Algorithmic HBM bytes per cloud: N*12 read + G*80 written.  The kernel is latency/VALU bound (N*G pdf
// evaluations ~ 1.3 MFLOP per cloud), not a roofline kernel; it exists to keep the [B,N,G,3] TF tiles
// (5 x 12.6 MB at B=32) out of HBM altogether.
//
// The forms, and where they live:
//   mfv3d.hip      mfv3d_fwd_kernel            any N whose tables fit the LDS (N <= 705 at m = 8): 4 workgroups of 1024 threads per cloud, each
//                                              owning a slice of the Gaussians; tables zq[axis][point][cell] = {z, e/S} of the FACTORISED
//                                              responsibilities in LDS; lane&7 <-> Gaussian, lane>>3 <-> one eighth of the points, 20 running
//                                              statistics (sum/max/min) in registers, the eight point groups merged with three lane exchanges;
//                                              power-1/2 values staged through LDS and written with coalesced float4 stores
//                  mfv3d_fwd2_kernel           the same for N % 8 == 0: points in pairs on the packed VALU, four point groups
//                  mfv3d_norm_kernel           the per-channel L2 norm over the Gaussian axis
//                  mfv3d_fwd_tiled_kernel<NB>  clouds whose tables do not fit: the same grid walking the points in TILES
//                  mfv3d_fwd_counts_kernel<NB> the tiled form over ragged sets (per-cloud point counts)
//   mfv3d_bwd.hip  mfv3d_bwd_kernel            one launch, one workgroup per cloud
//                  mfv3d_bwd_stats / combine / apply kernels   sliced over the POINTS (three launches), their *_tiled and *_counts forms,
//                                              asloss_tail_a_kernel (statistics beside the window-gather backward)
#include "mfv3d_int.h"

namespace dpd {

// ---------------------------------------------------------------------------------------------------------
// Forward: kSlices workgroups of 1024 threads per cloud (each owns a contiguous slice of the Gaussians), then a
// small normalisation kernel.  64 clouds alone would occupy 64 of the 256 CUs; sliced, the chip is full at B = 32.
//
// The Gaussians have diagonal covariance on a product grid, so the responsibility factorises exactly:
//     Q_ng = w p_ng / sum_g' w p_ng' = (ex[n][j]/Sx[n]) * (ey[n][i]/Sy[n]) * (ez[n][t]/Sz[n]),
//     e_a[n][i] = exp(-z_a^2/2),  S_a[n] = sum_i e_a[n][i]          (constants and the weight w cancel)
// which replaces N*G = 32 768 expf + divisions per cloud (:69-74) by 3*N*m = 1 536 of each.  The result differs from
// the reference's fp32 evaluation by a few ulp of Q; the reference's failure mode is reproduced explicitly:
// if w*p_ng underflows to 0 for EVERY Gaussian of some point (0/0 at :74) the whole descriptor is NaN.
//
//   tables  zq[a][n][i] = { z = (p[n][a]-l_i)/sigma , q = e/S }  (float2, one ds_read_b64 per axis per pair)
//   pass 2  lane&7 <-> Gaussian (8 per wave), lane>>3 <-> one eighth of the points; 20 running statistics in registers;
//           the eight point groups are merged with three __shfl_xor per statistic
//   store   power-1/2 values staged through LDS [slice][21] (conflict free), coalesced float4 stores (NaN if 0/0)
//   norm    mfv3d_norm_kernel: per-channel L2 over the Gaussian axis (:124-126), fixed summation order
// dynamic LDS (floats): zq[3*N*m*2] | S[3*N] | minz2[3*N] | stage[slice*21] | flag
// ---------------------------------------------------------------------------------------------------------

// Per-channel sum of squares of one slice of Gaussians, in THE summation order both consumers use (so that the separate norm
// kernel and the fused form give the same bits): 8 parts of ceil(gcount / 8) consecutive Gaussians, summed sequentially,
// then the 8 partials in order.  val(g, ch) reads the slice-local value.  Threads 0..159 take part; result valid for tid < 20.
template <typename F>
__device__ __forceinline__ float slice_ssq(int tid, int gcount, float* s_red /* [8][20] */, F val) {
    const int per = (gcount + 7) / 8;
    if (tid < 8 * kF) {
        const int part = tid / kF, ch = tid % kF;
        float ss = 0.f;
        const int g1 = min(gcount, (part + 1) * per);
        // eight loads in flight, then the SAME additions in the same order (a padded 0 * 0 adds an exact zero): the sequential form was a
        // chain of 16 dependent LDS round trips (1.6k of the forward kernel's 16k cycles, s_memtime stamps)
        for (int g = part * per; g < g1; g += 8) {
            float x[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) x[u] = (g + u < g1) ? val(g + u, ch) : 0.f;
#pragma unroll
            for (int u = 0; u < 8; ++u) ss += x[u] * x[u];
        }
        s_red[part * kF + ch] = ss;
    }
    __syncthreads();
    float t = 0.f;
    if (tid < kF) {
        float x[8];
#pragma unroll
        for (int part = 0; part < 8; ++part) x[part] = s_red[part * kF + tid];
#pragma unroll
        for (int part = 0; part < 8; ++part) t += x[part];
    }
    return t;
}

// the fused form's per-slice sums of squares of the normalised values store_slice wrote back to the stage
__device__ __forceinline__ void store_slice_ssq(float* __restrict__ ssq, int* s_bad, const float* s_stage, int c, int sl, int gcount, bool bad,
                                                int tid) {
    float* s_red = reinterpret_cast<float*>(s_bad) + 4;  // [8][20] partials
    __syncthreads();
    const float t = slice_ssq(tid, gcount, s_red, [&](int g, int ch) { return s_stage[g * kFP + ch]; });
    if (tid < kF) ssq[((size_t)c * kSlices + sl) * kF + tid] = bad ? __int_as_float(0x7fc00000) : t;
}

__global__ __launch_bounds__(kFwdThreads) void mfv3d_fwd_kernel(const float* __restrict__ pts, float* __restrict__ fv,
                                                                 MfvConst k, int gslice, MfvFuse fu) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int N = k.N, G = k.G, m = k.m;
    float2* s_zq = reinterpret_cast<float2*>(sm);   // [3][N][m]
    float* s_S = sm + 6 * N * m;                    // [3][N]
    float* s_mz = s_S + 3 * N;                      // [3][N] min_i z^2
    float* s_stage = s_mz + 3 * N;                  // [gslice][21]
    int* s_bad = reinterpret_cast<int*>(s_stage + gslice * kFP);

    const int tid = threadIdx.x, c = blockIdx.x / kSlices, sl = blockIdx.x % kSlices;
    const int g0 = sl * gslice, gcount = max(0, min(G, g0 + gslice) - g0);
    const int lane = tid & 63, wave = tid >> 6;
    // (prologue and tables stay this kernel's own text: behind routines shared with mfv3d_fwd2_kernel and the tiled body it measured
    //  0.45 us slower at N = 705, EXPERIMENTS G13; with no second caller left, those routines do not exist)
    const float* p = pts ? pts + (size_t)c * N * 3 : (c < fu.B ? fu.pcA + (size_t)c * N * 3 : fu.pcB + (size_t)(c - fu.B) * N * 3);
    const float* nz = (!pts && fu.noise && c < fu.B) ? fu.noise + (size_t)c * N * 3 : nullptr;
    if (tid == 0) *s_bad = 0;
    const int lg_m = lg_or_neg(m), lg_n = lg_or_neg(N);
    for (int e = tid; e < 3 * N * m; e += kFwdThreads) {
        const int em = qdiv(e, m, lg_m), i = e - em * m, a = qdiv(em, N, lg_n), n = em - a * N;
        const float x = nz ? p[n * 3 + a] + nz[n * 3 + a] : p[n * 3 + a];
        const float z = (x - k.ax.c[i]) / k.sigma;               // (batch_points - batch_mu) / batch_sig  (:87)
        s_zq[e] = make_float2(z, expf(-0.5f * (z * z)));
    }
    if (!pts && sl == 0) {      // the stacked tensors the rest of the step reads
        const int twin = c < fu.B ? c + fu.B : c - fu.B;          // q = [pcB ; pcA]: cloud c's raw points are the twin's queries
        for (int e = tid; e < 3 * N; e += kFwdThreads) {
            const float raw = p[e];
            if (fu.pts_out) fu.pts_out[(size_t)c * N * 3 + e] = nz ? raw + nz[e] : raw;
            if (fu.q_out) fu.q_out[(size_t)twin * N * 3 + e] = raw;
        }
    }
    __syncthreads();
    for (int e = tid; e < 3 * N; e += kFwdThreads) {              // e = a*N + n
        float S = 0.f, mz = INFINITY;
        for (int i = 0; i < m; ++i) {
            const float2 v = s_zq[e * m + i];
            S += v.y;
            mz = fminf(mz, v.x * v.x);
            if (v.x != v.x) mz = v.x;
        }
        s_S[e] = S;
        s_mz[e] = mz;
    }
    __syncthreads();
    for (int e = tid; e < 3 * N * m; e += kFwdThreads) s_zq[e].y = s_zq[e].y / s_S[qdiv(e, m, lg_m)];
    for (int n = tid; n < N; n += kFwdThreads) {
        // the reference's 0/0: every w*p_ng == 0  <=>  the largest one is (p is monotone in -|z|^2)
        const float pmax = pdf(k, sqrtf(s_mz[n]), sqrtf(s_mz[N + n]), sqrtf(s_mz[2 * N + n]));
        if (!(pmax * k.w > 0.f)) atomicOr(s_bad, 1);             // also catches NaN inputs
    }
    __syncthreads();
    const float2* zqx = s_zq;
    const float2* zqy = s_zq + N * m;
    const float2* zqz = s_zq + 2 * N * m;

    // ---- per-Gaussian statistics over the points ---------------------------------------------------------------
    const float invN = 1.0f / (float)N;
    const float inv_dpi = 1.0f / k.dpi_den;
    const int npg = (N + 7) / 8;
    const int grp = lane >> 3;
    for (int gbase = wave * 8; gbase < gcount; gbase += 16 * 8) {
        const int gl = gbase + (lane & 7);
        const bool live = gl < gcount;
        const int gg = live ? g0 + gl : 0;
        const int gm = qdiv(gg, m, lg_m), t = gg - gm * m, i = qdiv(gm, m, lg_m), j = gm - i * m;   // centre (x,y,z) = (l[j], l[i], l[t])  (:47-48)
        // (own variables and the expressions of eval_pq spelled out: with MfvStats / eval_pq beside the shared routines below the kernel came
        //  out at 54 or 56 VGPRs instead of 55, EXPERIMENTS G13)
        float pi_s = 0.f, pi_mx = -INFINITY;
        float mu_s[3] = {0.f, 0.f, 0.f}, mu_mx[3] = {-INFINITY, -INFINITY, -INFINITY}, mu_mn[3] = {INFINITY, INFINITY, INFINITY};
        float sg_s[3] = {0.f, 0.f, 0.f}, sg_mx[3] = {-INFINITY, -INFINITY, -INFINITY}, sg_mn[3] = {INFINITY, INFINITY, INFINITY};
        const int n1 = min(N, (grp + 1) * npg);
        for (int n = grp * npg; n < n1; ++n) {
            const float2 vx = zqx[n * m + j], vy = zqy[n * m + i], vz = zqz[n * m + t];
            const float z[3] = {vx.x, vy.x, vz.x};
            const float Q = (vx.y * vy.y) * vz.y;                              // :73-74, factorised
            const float dpi = (Q - k.w) * inv_dpi;                             // :78
            pi_s += dpi;
            pi_mx = fmaxf(pi_mx, dpi);
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                const float a = Q * z[d];                                       // :87
                const float b = Q * (z[d] * z[d] - 1.0f);                       // :100
                mu_s[d] += a; mu_mx[d] = fmaxf(mu_mx[d], a); mu_mn[d] = fminf(mu_mn[d], a);
                sg_s[d] += b; sg_mx[d] = fmaxf(sg_mx[d], b); sg_mn[d] = fminf(sg_mn[d], b);
            }
        }
        // merge the eight point groups (mfv3d_int.h)
        pi_s = sum_groups8(pi_s);
        pi_mx = max_groups8(pi_mx);
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            mu_s[d] = sum_groups8(mu_s[d]); sg_s[d] = sum_groups8(sg_s[d]);
            mu_mx[d] = max_groups8(mu_mx[d]); mu_mn[d] = min_groups8(mu_mn[d]);
            sg_mx[d] = max_groups8(sg_mx[d]); sg_mn[d] = min_groups8(sg_mn[d]);
        }
        if (live && grp == 0) {
            const float r[kF] = {pi_s, pi_mx, mu_s[0], mu_s[1], mu_s[2], mu_mx[0], mu_mx[1], mu_mx[2], mu_mn[0], mu_mn[1], mu_mn[2],
                                 sg_s[0], sg_s[1], sg_s[2], sg_mx[0], sg_mx[1], sg_mx[2], sg_mn[0], sg_mn[1], sg_mn[2]};
            stage_row(r, k, invN, s_stage + gl * kFP);
        }
    }
    __syncthreads();

    // ---- power-1/2 normalisation and coalesced store of the slice; the normalised values go back to the stage for the slice's sums of squares
    const bool bad = *s_bad != 0;
    store_slice<kFwdThreads, true>(fv + ((size_t)c * G + g0) * kF, s_stage, gcount, bad, tid);
    if (fu.ssq) store_slice_ssq(fu.ssq, s_bad, s_stage, c, sl, gcount, bad, tid);
}


// ---------------------------------------------------------------------------------------------------------
// Round 4: the same forward with less VALU work per (Gaussian, point) pair -- the statistics section of the kernel above is
// VALU-issue bound (round-4 s_memtime stamps, profiles/README.md: 11k of 20.6k cycles at B = 32, 12-16k at B = 64 where two
// workgroups share a CU's VALUs), and of its ~90 instructions per Gaussian and point group half were the merge of the eight point groups.
//   * lanes: lane & 15 <-> Gaussian (16 per wave), lane >> 4 <-> a QUARTER of the points: two merge stages (xor 16, xor 32) for 16
//     Gaussians instead of three for 8 -- a third of the merge work per Gaussian; 512-thread workgroups (8 waves x 16 Gaussians = the
//     slice of 128), so a CU holds the same number of waves as before;
//   * points in PAIRS on the packed fp32 VALU (v_pk_mul_f32 / v_pk_add_f32: two lanes' worth of products and running sums per
//     instruction): the tables hold {z(n), z(n+1), q(n), q(n+1)} as one float4 per axis entry (one ds_read_b128 per axis and pair);
//     max / min have no packed form and stay scalar.
// Same expressions per element as the kernel above (Q = (qx qy) qz, (Q - w) / den, Q z, Q (z z - 1)); the running SUMS are taken over
// even and odd points separately and over four groups instead of eight, i.e. in another order: the statistics differ from the kernel
// above in the last bits (both are within the oracle bars).  Needs N % 8 == 0.
// dynamic LDS (floats): zq4[3*(N/2)*m*4] | S[3*N] | minz2[3*N] | stage[slice*21] | flag | red[8*20]    (same size as above)
// ---------------------------------------------------------------------------------------------------------
typedef float mfv_f2 __attribute__((ext_vector_type(2)));

__global__ __launch_bounds__(kFwd2Threads) void mfv3d_fwd2_kernel(const float* __restrict__ pts, float* __restrict__ fv, MfvConst k, int gslice,
                                                                  MfvFuse fu) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int N = k.N, G = k.G, m = k.m, NP = N >> 1;
    float* s_t = sm;                                // [3][N/2][m][4] = {z(2p), z(2p+1), q(2p), q(2p+1)}
    float* s_S = sm + 6 * N * m;                    // [3][N]
    float* s_mz = s_S + 3 * N;                      // [3][N] min_i z^2
    float* s_stage = s_mz + 3 * N;                  // [gslice][21]
    int* s_bad = reinterpret_cast<int*>(s_stage + gslice * kFP);
    auto slot = [&](int a, int n, int i) { return ((a * NP + (n >> 1)) * m + i) * 4 + (n & 1); };    // z; q at + 2

    const int tid = threadIdx.x, c = blockIdx.x / kSlices, sl = blockIdx.x % kSlices;
    const int g0 = sl * gslice, gcount = max(0, min(G, g0 + gslice) - g0);
    const int lane = tid & 63, wave = tid >> 6;
    const float* p = pts ? pts + (size_t)c * N * 3 : (c < fu.B ? fu.pcA + (size_t)c * N * 3 : fu.pcB + (size_t)(c - fu.B) * N * 3);
    const float* nz = (!pts && fu.noise && c < fu.B) ? fu.noise + (size_t)c * N * 3 : nullptr;
    if (tid == 0) *s_bad = 0;
    const int lg_m = lg_or_neg(m), lg_n = lg_or_neg(N);
    // m == 8 (the reference's grid) and whole passes: the 8 entries (a, n, 0..7) of a point and axis sit in 8 consecutive lanes, so the row sum S,
    // the normalised q = e / S and min_i z^2 come out of three DPP steps in registers -- no second pass over the table, no barrier in between
    const bool dpp8 = m == 8 && (3 * N * m) % kFwd2Threads == 0;
    if (dpp8) {
        // (no unroll pragma: the trip count is a run-time value and the body holds convergent DPP operations, so hipcc cannot peel a
        //  remainder -- a requested `unroll 3` was silently refused with a -Wpass-failed warning.  Three iterations at N = 64, 3.0k of the
        //  workgroup's 20.6k cycles (the same round-4 stamps): not where this kernel's time goes)
        for (int e = tid; e < 3 * N * m; e += kFwd2Threads) {
            const int em = e >> 3, i = e & 7, a = qdiv(em, N, lg_n), n = em - a * N;
            const float x = nz ? p[n * 3 + a] + nz[n * 3 + a] : p[n * 3 + a];
            const float z = (x - k.ax.c[i]) / k.sigma;               // (batch_points - batch_mu) / batch_sig  (:87)
            const float ex = expf(-0.5f * (z * z));
            float S = ex, mz = z * z, bad = (z != z) ? 1.f : 0.f;
            S += dpp_move<0xB1>(S); mz = fminf(mz, dpp_move<0xB1>(mz)); bad += dpp_move<0xB1>(bad);        // quad_perm [1,0,3,2]
            S += dpp_move<0x4E>(S); mz = fminf(mz, dpp_move<0x4E>(mz)); bad += dpp_move<0x4E>(bad);        // quad_perm [2,3,0,1]
            S += dpp_move<0x141>(S); mz = fminf(mz, dpp_move<0x141>(mz)); bad += dpp_move<0x141>(bad);     // row_half_mirror: the other quad of the 8
            const int o = slot(a, n, i);
            s_t[o] = z;
            s_t[o + 2] = ex / S;
            if (i == 0) s_mz[em] = bad > 0.f ? __int_as_float(0x7fc00000) : mz;
        }
    } else {
        for (int e = tid; e < 3 * N * m; e += kFwd2Threads) {
            const int em = qdiv(e, m, lg_m), i = e - em * m, a = qdiv(em, N, lg_n), n = em - a * N;
            const float x = nz ? p[n * 3 + a] + nz[n * 3 + a] : p[n * 3 + a];
            const float z = (x - k.ax.c[i]) / k.sigma;               // (batch_points - batch_mu) / batch_sig  (:87)
            const int o = slot(a, n, i);
            s_t[o] = z;
            s_t[o + 2] = expf(-0.5f * (z * z));
        }
    }
    if (!pts && sl == 0) {      // the stacked tensors the rest of the step reads, as in mfv3d_fwd_kernel
        const int twin = c < fu.B ? c + fu.B : c - fu.B;
        for (int e = tid; e < 3 * N; e += kFwd2Threads) {
            const float raw = p[e];
            if (fu.pts_out) fu.pts_out[(size_t)c * N * 3 + e] = nz ? raw + nz[e] : raw;
            if (fu.q_out) fu.q_out[(size_t)twin * N * 3 + e] = raw;
        }
    }
    __syncthreads();
    if (!dpp8) {
        for (int e = tid; e < 3 * N; e += kFwd2Threads) {             // e = a*N + n
            const int a = qdiv(e, N, lg_n), n = e - a * N;
            float S = 0.f, mz = INFINITY;
            for (int i = 0; i < m; ++i) {
                const int o = slot(a, n, i);
                const float zz = s_t[o];
                S += s_t[o + 2];
                mz = fminf(mz, zz * zz);
                if (zz != zz) mz = zz;
            }
            s_S[e] = S;
            s_mz[e] = mz;
        }
        __syncthreads();
        for (int e = tid; e < 3 * N * m; e += kFwd2Threads) {
            const int em = qdiv(e, m, lg_m), i = e - em * m, a = qdiv(em, N, lg_n), n = em - a * N;
            const int o = slot(a, n, i) + 2;
            s_t[o] = s_t[o] / s_S[em];
        }
    }
    for (int n = tid; n < N; n += kFwd2Threads) {
        const float pmax = pdf(k, sqrtf(s_mz[n]), sqrtf(s_mz[N + n]), sqrtf(s_mz[2 * N + n]));
        if (!(pmax * k.w > 0.f)) atomicOr(s_bad, 1);             // the reference's 0/0 (also catches NaN inputs)
    }
    __syncthreads();
    const float4* tx = reinterpret_cast<const float4*>(s_t);
    const float4* ty = tx + NP * m;
    const float4* tz = tx + 2 * NP * m;

    const float invN = 1.0f / (float)N;
    const float inv_dpi = 1.0f / k.dpi_den;
    const int grp = lane >> 4;                      // quarter of the points
    const int ppg = NP >> 2;                        // point pairs per group (N % 8 == 0)
    const mfv_f2 w2 = {k.w, k.w}, inv2 = {inv_dpi, inv_dpi}, one2 = {1.0f, 1.0f};
    for (int gbase = wave * 16; gbase < gcount; gbase += (kFwd2Threads / 64) * 16) {
        const int gl = gbase + (lane & 15);
        const bool live = gl < gcount;
        const int gg = live ? g0 + gl : 0;
        const int gm = qdiv(gg, m, lg_m), t = gg - gm * m, i = qdiv(gm, m, lg_m), j = gm - i * m;   // centre (x,y,z) = (l[j], l[i], l[t])  (:47-48)
        mfv_f2 pi_s2 = {0.f, 0.f}, mu_s2[3] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}}, sg_s2[3] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};
        float pi_mx = -INFINITY;
        float mu_mx[3] = {-INFINITY, -INFINITY, -INFINITY}, mu_mn[3] = {INFINITY, INFINITY, INFINITY};
        float sg_mx[3] = {-INFINITY, -INFINITY, -INFINITY}, sg_mn[3] = {INFINITY, INFINITY, INFINITY};
        // four pairs per trip with their twelve table reads requested up front: with two waves per SIMD nothing else hides the LDS latency
        // (3.3k cycles for eight pairs before, by s_memtime stamps); a partial last trip re-reads its last valid pair and skips the update
        const int pp_end = (grp + 1) * ppg;
        for (int pp0 = grp * ppg; pp0 < pp_end; pp0 += 4) {
          float4 lx[4], ly[4], lz[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
              const int pq = min(pp0 + u, pp_end - 1);
              lx[u] = tx[pq * m + j]; ly[u] = ty[pq * m + i]; lz[u] = tz[pq * m + t];
          }
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            if (pp0 + u >= pp_end) break;
            const float4 vx = lx[u], vy = ly[u], vz = lz[u];
            const mfv_f2 z[3] = {{vx.x, vx.y}, {vy.x, vy.y}, {vz.x, vz.y}};
            const mfv_f2 qx = {vx.z, vx.w}, qy = {vy.z, vy.w}, qz = {vz.z, vz.w};
            const mfv_f2 Q = (qx * qy) * qz;                                   // :73-74, factorised
            const mfv_f2 dpi = (Q - w2) * inv2;                                // :78
            pi_s2 += dpi;
            pi_mx = fmaxf(fmaxf(pi_mx, dpi.x), dpi.y);
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                const mfv_f2 a = Q * z[d];                                      // :87
                const mfv_f2 b = Q * (z[d] * z[d] - one2);                      // :100
                mu_s2[d] += a; sg_s2[d] += b;
                mu_mx[d] = fmaxf(fmaxf(mu_mx[d], a.x), a.y); mu_mn[d] = fminf(fminf(mu_mn[d], a.x), a.y);
                sg_mx[d] = fmaxf(fmaxf(sg_mx[d], b.x), b.y); sg_mn[d] = fminf(fminf(sg_mn[d], b.x), b.y);
            }
          }
        }
        // even + odd points, then the four point groups (lanes l, l ^ 16, l ^ 32, l ^ 48 hold the same Gaussian): xor 16 through
        // ds_swizzle, xor 32 as a v_permlane32_swap (both halves receive lower + upper)
        MfvStats st;
        st.pi_s = pi_s2.x + pi_s2.y; st.pi_mx = pi_mx;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            st.mu_s[d] = mu_s2[d].x + mu_s2[d].y; st.sg_s[d] = sg_s2[d].x + sg_s2[d].y;
            st.mu_mx[d] = mu_mx[d]; st.mu_mn[d] = mu_mn[d]; st.sg_mx[d] = sg_mx[d]; st.sg_mn[d] = sg_mn[d];
        }
        float r[kF];
        st.fold(r, [](float v) { v += xor16(v); return sum_x32(v); }, [](float v) { v = fmaxf(v, xor16(v)); return max_x32(v); },
                [](float v) { v = fminf(v, xor16(v)); return min_x32(v); });
        if (live && grp == 0) stage_row(r, k, invN, s_stage + gl * kFP);
    }
    __syncthreads();
    // power-1/2 normalisation (:119-121) + coalesced store + the slice's sums of squares: as in mfv3d_fwd_kernel
    const bool bad = *s_bad != 0;
    store_slice<kFwd2Threads, true>(fv + ((size_t)c * G + g0) * kF, s_stage, gcount, bad, tid);
    if (fu.ssq) store_slice_ssq(fu.ssq, s_bad, s_stage, c, sl, gcount, bad, tid);
}

// L2 normalisation over the Gaussian axis, per channel (:124-126), in place.  One 256-thread block per cloud.  The per-channel
// sums are taken slice by slice in slice_ssq order and the slices added in order: the same bits as the fused form (ssq from the
// forward kernel + scale applied by the window gather).
__device__ __forceinline__ float l2_scale(float ss) { return 1.0f / sqrtf(fmaxf(ss, 1e-12f)); }   // x * rsqrt(max(sum x^2, eps))

__global__ __launch_bounds__(1024) void mfv3d_norm_kernel(float* __restrict__ fv, int G, int gslice) {
    // thread (slice, part, ch): the same partial sums, in the same order, as slice_ssq computes inside the forward kernel
    __shared__ float s_red[kSlices][8 * kF];
    __shared__ float s_scale[kF];
    const int tid = threadIdx.x, c = blockIdx.x;
    float* base = fv + (size_t)c * G * kF;
    if (tid < kSlices * 8 * kF) {
        const int sl = tid / (8 * kF), part = (tid / kF) % 8, ch = tid % kF;
        const int g0 = sl * gslice, gcount = max(0, min(G, g0 + gslice) - g0);
        const int per = (gcount + 7) / 8, g1 = min(gcount, (part + 1) * per);
        float ss = 0.f;
        for (int g = part * per; g < g1; ++g) { const float x = base[(size_t)(g0 + g) * kF + ch]; ss += x * x; }
        s_red[sl][part * kF + ch] = ss;
    }
    __syncthreads();
    if (tid < kF) {
        float total = 0.f;
        for (int sl = 0; sl < kSlices; ++sl) {
            float t = 0.f;
            for (int part = 0; part < 8; ++part) t += s_red[sl][part * kF + tid];
            total += t;
        }
        s_scale[tid] = l2_scale(total);
    }
    __syncthreads();
    float4* b4 = reinterpret_cast<float4*>(base);
    for (int i = tid; i < G * 5; i += 1024) {
        const int part = i % 5;
        float4 v = b4[i];
        v.x *= s_scale[part * 4]; v.y *= s_scale[part * 4 + 1]; v.z *= s_scale[part * 4 + 2]; v.w *= s_scale[part * 4 + 3];
        b4[i] = v;
    }
}

// ------------------------------------------------------------------------------------------------------
// The encoder over TILES of points (dpd_mfv3d_fwd_tiled / dpd_mfv3d_bwd_tiled): the kernels above stage the tables of ALL N points of a
// cloud (or of a point slice) in LDS, which caps N at 705 (forward, m = 8), 402 / 1636 (backward).  Every Fisher-vector statistic is a
// sum, a max or a min over the points, so the tiled kernels walk the points in tiles of at most `tile`, rebuild the tables {z, e/S} for
// the tile's points only and carry the statistics in REGISTERS across the tiles; everything after the point loop (merge of the point
// groups, power-1/2, coalesced store, mfv3d_norm_kernel; combine kernel of the backward) runs once, as in the kernels above.
// Same expressions per (point, Gaussian); the sums are taken in another order (tile by tile), so the results differ from the plain
// entries in the last bits and are held to the same bars against the float64 oracle.
//
// Forward: the eight-point-group formulation of mfv3d_fwd_kernel (any N, any tile; the same device routines: with ONE tile, the same
// bits -- tests/test_mfv_units_gpu.py).  Grid and Gaussian slices as there.
//   * the 0/0 flag accumulates over ALL tiles (s_bad is cleared once, before the first tile);
//   * the mean's 1 / N and dpi_den = sqrt(w) N use the cloud's N (MfvConst), never the tile's;
//   * a ragged last tile (down to one point) leaves some of the eight point groups empty: they add nothing to the running statistics,
//     which start at 0 / -inf / +inf;
//   * m = 9, 10: a slice holds 183 / 250 Gaussians, more than the 16 waves x 8 of one batch.  NB = 2 keeps ONE STATISTICS SET PER BATCH
//     in registers (2 x 20 running values per lane) instead of making the batch the outer loop, which would rebuild every table twice:
//     the kernel has 128 VGPRs per lane at 1024 threads and needs 93 for both sets, 66 for one (resource table in DESIGN section 3), no scratch.
// dynamic LDS (floats): zq[3*tile*m*2] | S[3*tile] | minz2[3*tile] | stage[slice*21] | flag
// ------------------------------------------------------------------------------------------------------
// Tables of one tile, the np_ points at p: zq[a][n][i] = {z, e/S}, S[a][n], mz[a][n] = min_i z^2 (NaN if a z is), and the reference's 0/0
// flag OR-ed into *s_bad (cleared by the caller: it accumulates over the tiles).  Ends on a barrier.  The text of mfv3d_fwd_kernel's
// tables without the noise; the tiled body is its one caller (why the plain kernel keeps its own: there).
__device__ __forceinline__ void build_tile_tables(const float* p, int np_, const MfvConst& k, float2* s_zq, float* s_S, float* s_mz, int* s_bad,
                                                  int tid) {
    const int m = k.m;
    const int lg_m = lg_or_neg(m), lg_np = lg_or_neg(np_);
    for (int e = tid; e < 3 * np_ * m; e += kFwdThreads) {
        const int em = qdiv(e, m, lg_m), i = e - em * m, a = qdiv(em, np_, lg_np), n = em - a * np_;
        const float z = (p[n * 3 + a] - k.ax.c[i]) / k.sigma;    // (batch_points - batch_mu) / batch_sig  (:87)
        s_zq[e] = make_float2(z, expf(-0.5f * (z * z)));
    }
    __syncthreads();
    for (int e = tid; e < 3 * np_; e += kFwdThreads) {            // e = a*np_ + n
        float S = 0.f, mz = INFINITY;
        for (int i = 0; i < m; ++i) {
            const float2 v = s_zq[e * m + i];
            S += v.y;
            mz = fminf(mz, v.x * v.x);
            if (v.x != v.x) mz = v.x;
        }
        s_S[e] = S;
        s_mz[e] = mz;
    }
    __syncthreads();
    for (int e = tid; e < 3 * np_ * m; e += kFwdThreads) s_zq[e].y = s_zq[e].y / s_S[qdiv(e, m, lg_m)];
    for (int n = tid; n < np_; n += kFwdThreads) {
        // the reference's 0/0: every w*p_ng == 0  <=>  the largest one is (p is monotone in -|z|^2)
        const float pmax = pdf(k, sqrtf(s_mz[n]), sqrtf(s_mz[np_ + n]), sqrtf(s_mz[2 * np_ + n]));
        if (!(pmax * k.w > 0.f)) atomicOr(s_bad, 1);             // also catches NaN inputs
    }
    __syncthreads();
}

// CNT (the *_counts entries): cloud c holds its first counts[c] points of a row of k.N (clamped into [1, k.N] here: the host never reads
// the device words); N below is then the cloud's own count -- loop bound, the mean's 1 / N and sqrt(w) N (sqw = the host's sqrt(w), the
// product formed as make_const forms it) -- and the row stride stays k.N.  The padding is never read.  CNT = false: the code as it was.
template <int NB, bool CNT>
__device__ __forceinline__ void mfv3d_fwd_tiled_body(const float* __restrict__ pts, float* __restrict__ fv, const MfvConst& k, int gslice,
                                                     int tile, const int32_t* __restrict__ counts, float sqw) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int G = k.G, m = k.m;
    const int N = CNT ? min(max(counts[blockIdx.x / kSlices], 1), k.N) : k.N;
    float2* s_zq = reinterpret_cast<float2*>(sm);   // [3][np_][m], np_ <= tile
    float* s_S = sm + 6 * tile * m;                 // [3][np_]
    float* s_mz = s_S + 3 * tile;                   // [3][np_] min_i z^2
    float* s_stage = s_mz + 3 * tile;               // [gslice][21]
    int* s_bad = reinterpret_cast<int*>(s_stage + gslice * kFP);

    const int tid = threadIdx.x, c = blockIdx.x / kSlices, sl = blockIdx.x % kSlices;
    const int g0 = sl * gslice, gcount = max(0, min(G, g0 + gslice) - g0);
    const int lane = tid & 63, wave = tid >> 6, grp = lane >> 3;
    const int lg_m = lg_or_neg(m);
    if (tid == 0) *s_bad = 0;

    // this lane's Gaussian of every batch: centre (x,y,z) = (l[j], l[i], l[t])  (:47-48)
    int gl[NB], gi[NB], gj[NB], gt[NB];
    bool live[NB], act[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int gbase = wave * 8 + b * 16 * 8;
        act[b] = gbase < gcount;                    // wave-uniform
        gl[b] = gbase + (lane & 7);
        live[b] = gl[b] < gcount;
        const int gg = live[b] ? g0 + gl[b] : 0;
        const int gm = qdiv(gg, m, lg_m);
        gt[b] = gg - gm * m; gi[b] = qdiv(gm, m, lg_m); gj[b] = gm - gi[b] * m;
    }
    // (arrays, not MfvStats st[NB]: over the struct's members the four instantiations came out at 64 / 90 / 64 / 91 VGPRs instead of
    //  66 / 93 / 66 / 95 and NB = 1 at occupancy 8 instead of 7; with st[b].add(eval_pq(..)) at 70 / 90 / 71 / 91, EXPERIMENTS G13)
    float pi_s[NB], pi_mx[NB], mu_s[NB][3], mu_mx[NB][3], mu_mn[NB][3], sg_s[NB][3], sg_mx[NB][3], sg_mn[NB][3];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        pi_s[b] = 0.f; pi_mx[b] = -INFINITY;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            mu_s[b][d] = 0.f; mu_mx[b][d] = -INFINITY; mu_mn[b][d] = INFINITY;
            sg_s[b][d] = 0.f; sg_mx[b][d] = -INFINITY; sg_mn[b][d] = INFINITY;
        }
    }
    const float inv_dpi = 1.0f / (CNT ? sqw * (float)N : k.dpi_den);

    for (int t0 = 0; t0 < N; t0 += tile) {
        const int np_ = min(tile, N - t0);
        build_tile_tables(pts + ((size_t)c * k.N + t0) * 3, np_, k, s_zq, s_S, s_mz, s_bad, tid);
        const float2* zqx = s_zq;
        const float2* zqy = s_zq + np_ * m;
        const float2* zqz = s_zq + 2 * np_ * m;
        // ---- the tile's share of the running statistics: lane & 7 <-> Gaussian, lane >> 3 <-> an eighth of the TILE's points ----
        const int npg = (np_ + 7) / 8;
        const int n1 = min(np_, (grp + 1) * npg);
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            if (!act[b]) continue;
            for (int n = grp * npg; n < n1; ++n) {      // (the expressions of eval_pq spelled out: eval_pq here cost NB = 1 two VGPRs, G13)
                const float2 vx = zqx[n * m + gj[b]], vy = zqy[n * m + gi[b]], vz = zqz[n * m + gt[b]];
                const float z[3] = {vx.x, vy.x, vz.x};
                const float Q = (vx.y * vy.y) * vz.y;                              // :73-74, factorised
                const float dpi = (Q - k.w) * inv_dpi;                             // :78
                pi_s[b] += dpi;
                pi_mx[b] = fmaxf(pi_mx[b], dpi);
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    const float a = Q * z[d];                                       // :87
                    const float bb = Q * (z[d] * z[d] - 1.0f);                      // :100
                    mu_s[b][d] += a; mu_mx[b][d] = fmaxf(mu_mx[b][d], a); mu_mn[b][d] = fminf(mu_mn[b][d], a);
                    sg_s[b][d] += bb; sg_mx[b][d] = fmaxf(sg_mx[b][d], bb); sg_mn[b][d] = fminf(sg_mn[b][d], bb);
                }
            }
        }
        __syncthreads();        // the next tile overwrites the tables
    }

    // ---- once, after the last tile: merge the eight point groups, the mean over the CLOUD's N, stage (spelled out: through stage_row the
    // four instantiations came out 1 to 3 VGPRs lower, EXPERIMENTS G13) ----
    const float invN = 1.0f / (float)N;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        if (!act[b]) continue;
        float v[kF];
        v[0] = sum_groups8(pi_s[b]) * invN;                                            // :81 reduce_mean over the CLOUD's N
        v[1] = max_groups8(pi_mx[b]);                                                  // :80
#pragma unroll
        for (int d = 0; d < 3; ++d) {                                           // :89-98, :102-109
            v[2 + d] = (sum_groups8(mu_s[b][d]) * invN) * k.mu_scale;
            v[5 + d] = max_groups8(mu_mx[b][d]) * k.mu_scale;
            v[8 + d] = min_groups8(mu_mn[b][d]) * k.mu_scale;
            v[11 + d] = (sum_groups8(sg_s[b][d]) * invN) * k.sig_scale;
            v[14 + d] = max_groups8(sg_mx[b][d]) * k.sig_scale;
            v[17 + d] = min_groups8(sg_mn[b][d]) * k.sig_scale;
        }
        if (live[b] && grp == 0) {
#pragma unroll
            for (int f = 0; f < kF; ++f) s_stage[gl[b] * kFP + f] = v[f];
        }
    }
    __syncthreads();
    // power-1/2 normalisation (:119-121) and coalesced store of the slice, as in mfv3d_fwd_kernel
    store_slice<kFwdThreads, false>(fv + ((size_t)c * G + g0) * kF, s_stage, gcount, *s_bad != 0, tid);
}

template <int NB>
__global__ __launch_bounds__(kFwdThreads) void mfv3d_fwd_tiled_kernel(const float* __restrict__ pts, float* __restrict__ fv, MfvConst k,
                                                                       int gslice, int tile) {
    mfv3d_fwd_tiled_body<NB, false>(pts, fv, k, gslice, tile, nullptr, 0.f);
}
template <int NB>
__global__ __launch_bounds__(kFwdThreads) void mfv3d_fwd_counts_kernel(const float* __restrict__ pts, const int32_t* __restrict__ counts,
                                                                        float* __restrict__ fv, MfvConst k, int gslice, int tile, float sqw) {
    mfv3d_fwd_tiled_body<NB, true>(pts, fv, k, gslice, tile, counts, sqw);
}

// ---- host ------------------------------------------------------------------------------------------------------------------
int make_const(int N, int m, float sigma, MfvConst& k) {
    if (m < 1 || m > 10) return DPD_E_UNSUPPORTED;
    if (N < 1 || N > 4096) return DPD_E_UNSUPPORTED;
    if (!(sigma > 0.f)) return DPD_E_DIM;
    k.ax = make_axis(m);
    k.N = N; k.m = m; k.G = m * m * m;
    k.sigma = sigma;
    const double D = 3.0;
    k.lognorm = (float)(0.5 * D * log(2.0 * M_PI) + D * log((double)sigma));
    k.w = 1.0f / (float)k.G;
    k.dpi_den = sqrtf(k.w) * (float)N;
    k.mu_scale = 1.0f / sqrtf(k.w);
    k.sig_scale = 1.0f / sqrtf(2.0f * k.w);
    return 0;
}

// no opt-in attribute at or under 64 KiB, two workgroups per CU (m = 8: 248 forward, 160 backward; m = 10: 168 forward); no tile for m
// outside 1..10 and, backward, m > 8
int default_tile(int m, bool backward) {
    if (m < 1 || m > 10 || (backward && m > 8)) return 0;
    const int gslice = (m * m * m + kSlices - 1) / kSlices;
    int t = 0;
    while ((backward ? bwd_sliced_lds_bytes(t + 8, m) : fwd_tiled_lds_bytes(t + 8, m, gslice)) <= 64 * 1024) t += 8;
    return t;
}

int resolve_tile(int tile, int m, bool backward, int npoints, int& T) {
    if (tile < 0 || (tile != 0 && (tile < 8 || tile % 8))) return DPD_E_UNSUPPORTED;
    T = tile ? tile : default_tile(m, backward);
    if (T < 8) return DPD_E_UNSUPPORTED;
    const int cap = (npoints + 7) / 8 * 8;
    if (T > cap) T = cap;
    return 0;
}

// round-4 forward kernel (pairs of points on the packed VALU, four point groups) where N % 8 == 0; the round-3 kernel otherwise
static bool use_fwd2(int N) { return N >= 8 && N % 8 == 0; }

template <auto Kern, int THREADS>
static int launch_fwd_kernel(const float* pts, float* fv, const MfvConst& k, int C, int gslice, const MfvFuse& fuse, hipStream_t s) {
    const size_t lds = fwd_lds_bytes(k.N, k.m, gslice);
    if (int rc = set_lds<Kern>(lds)) return rc;
    DPD_LAUNCH(Kern, dim3(C * kSlices), dim3(THREADS), lds, s, pts, fv, k, gslice, fuse);
    DPD_CHECK_LAUNCH();
    return 0;
}

// the plain forward over C clouds (pts, or the fused front end's inputs in `fuse`) and, unless the caller takes the per-slice sums of
// squares instead, the L2 norm
static int launch_fwd(const float* pts, float* fv, const MfvConst& k, int C, const MfvFuse& fuse, void* stream) {
    const int gslice = (k.G + kSlices - 1) / kSlices;
    hipStream_t s = (hipStream_t)stream;
    if (int rc = use_fwd2(k.N) ? launch_fwd_kernel<mfv3d_fwd2_kernel, kFwd2Threads>(pts, fv, k, C, gslice, fuse, s)
                               : launch_fwd_kernel<mfv3d_fwd_kernel, kFwdThreads>(pts, fv, k, C, gslice, fuse, s))
        return rc;
    if (!fuse.ssq) {
        DPD_LAUNCH(mfv3d_norm_kernel, dim3(C), dim3(1024), 0, s, fv, k.G, gslice);
        DPD_CHECK_LAUNCH();
    }
    return 0;
}

// the tiled forward and its per-cloud-count twin (counts = NULL: the tiled entry, its kernel and its bits); NB = 2 for m = 9, 10: two
// batches of Gaussians per wave
template <int NB>
static int launch_fwd_tiled(const float* pts, const int32_t* counts, float* fv, const MfvConst& k, int C, int gslice, int T, hipStream_t s) {
    const size_t lds = fwd_tiled_lds_bytes(T, k.m, gslice);
    const dim3 grid(C * kSlices), block(kFwdThreads);
    if (counts) {
        if (int rc = set_lds<mfv3d_fwd_counts_kernel<NB>>(lds)) return rc;
        DPD_LAUNCH(mfv3d_fwd_counts_kernel<NB>, grid, block, lds, s, pts, counts, fv, k, gslice, T, sqrtf(k.w));
    } else {
        if (int rc = set_lds<mfv3d_fwd_tiled_kernel<NB>>(lds)) return rc;
        DPD_LAUNCH(mfv3d_fwd_tiled_kernel<NB>, grid, block, lds, s, pts, fv, k, gslice, T);
    }
    DPD_CHECK_LAUNCH();
    DPD_LAUNCH(mfv3d_norm_kernel, dim3(C), dim3(1024), 0, s, fv, k.G, gslice);
    DPD_CHECK_LAUNCH();
    return 0;
}

static int fwd_tiled(const float* pts, const int32_t* counts, int C, int N, int m, float sigma, int tile, float* fv, void* stream) {
    if (C <= 0) return DPD_E_DIM;
    MfvConst k{};
    if (int rc = make_const(N, m, sigma, k)) return rc;
    const int gslice = (k.G + kSlices - 1) / kSlices;
    if (tile > 0 && fwd_tiled_lds_bytes(tile, m, gslice) > 160 * 1024) return DPD_E_UNSUPPORTED;    // the tile as given must fit
    int T = 0;
    if (int rc = resolve_tile(tile, m, false, N, T)) return rc;
    StageProf prof(stream, DPD_STAGE_ENCODER, (double)C * (N * 12.0 * kSlices + k.G * 80.0));      // every Gaussian slice reads the points
    return gslice > 16 * 8 ? launch_fwd_tiled<2>(pts, counts, fv, k, C, gslice, T, (hipStream_t)stream)
                           : launch_fwd_tiled<1>(pts, counts, fv, k, C, gslice, T, (hipStream_t)stream);
}

}  // namespace dpd

using namespace dpd;

extern "C" int dpd_mfv3d_fwd(const float* pts, int C, int N, int m, float sigma, float* fv, void* stream) {
    if (!pts || !fv) return DPD_E_NULL;
    if (C <= 0) return DPD_E_DIM;
    MfvConst k{};
    if (int rc = make_const(N, m, sigma, k)) return rc;
    StageProf prof(stream, DPD_STAGE_ENCODER, (double)C * (N * 12.0 + k.G * 80.0));      // points in, [G,20] Fisher vector out
    return launch_fwd(pts, fv, k, C, MfvFuse{}, stream);
}

extern "C" int dpd_mfv3d_fwd_stacked(const float* pcA, const float* pcB, const float* noise, int B, int N, int m, float sigma,
                                     float* pts, float* q, float* fv, float* ssq, void* stream) {
    if (!pcA || !pcB || !fv) return DPD_E_NULL;
    if (B <= 0) return DPD_E_DIM;
    MfvConst k{};
    if (int rc = make_const(N, m, sigma, k)) return rc;
    const int C = 2 * B;
    // points (+ noise) in; stacked pts / q and the [G,20] Fisher vector (+ per-slice sums of squares) out
    StageProf prof(stream, DPD_STAGE_ENCODER, (double)C * (N * 12.0 * (noise ? 1.5 : 1.0) + N * 24.0 + k.G * 80.0 + (ssq ? kSlices * 80.0 : 0.0)));
    return launch_fwd(nullptr, fv, k, C, MfvFuse{pcA, pcB, noise, pts, q, ssq, B}, stream);
}

// ---- the tiled entries: any 1 <= N <= 4096 (the plain entries above are unchanged and keep their LDS caps) ----
extern "C" int dpd_mfv3d_fits(int N, int m, int which) {
    if (N < 1 || N > 4096 || m < 1 || m > 10) return 0;
    const int G = m * m * m;
    const size_t cap = 160 * 1024;
    if (which == 0) return fwd_lds_bytes(N, m, (G + kSlices - 1) / kSlices) <= cap;
    if (G > 512) return 0;
    if (which == 1 || (which == 2 && N < 2 * kSlices)) return bwd_lds_bytes(N, m) <= cap;
    if (which == 2) return bwd_sliced_lds_bytes((N + kSlices - 1) / kSlices, m) <= cap;
    return 0;
}

extern "C" int dpd_mfv3d_tile(int m, int which) { return default_tile(m, which != 0); }

extern "C" int dpd_mfv3d_fwd_tiled(const float* pts, int C, int N, int m, float sigma, int tile, float* fv, void* stream) {
    if (!pts || !fv) return DPD_E_NULL;
    return fwd_tiled(pts, nullptr, C, N, m, sigma, tile, fv, stream);
}

// ---- ragged sets: cloud c is the first counts[c] points of its row of N (include/dpdist_capi.h) ----
extern "C" int dpd_mfv3d_fwd_counts(const float* pts, const int32_t* counts, int C, int N, int m, float sigma, int tile, float* fv,
                                    void* stream) {
    if (!pts || !counts || !fv) return DPD_E_NULL;
    return fwd_tiled(pts, counts, C, N, m, sigma, tile, fv, stream);
}

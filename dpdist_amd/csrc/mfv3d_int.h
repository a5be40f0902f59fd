// What the two translation units of the 3DmFV encoder share: mfv3d.hip (forward) and mfv3d_bwd.hip (backward).  Every kernel lives in
// exactly one unit; the device routines here are the pieces that several kernels run over the same operands in the same order (the
// per-(point, Gaussian) expressions, the 20 running statistics, the tie-gated gradient, the backward's tables, the forward's merge and tail), written once.
// Included by those two units only.
#pragma once
#include <cstdlib>

#include "common.h"

namespace dpd {

constexpr int kF = DPD_FV_CHANNELS;  // 20
constexpr int kFP = kF + 1;          // padded LDS row
constexpr int kRec = 33;             // record of the sliced backward: 20 statistics + 13 tie counts
constexpr int kFwdThreads = 1024;
constexpr int kFwd2Threads = 512;
constexpr int kSlices = kMfvSlices;   // common.h (the window gather sums the per-slice norms)

struct MfvConst {
    GridAxis ax;
    int N, m, G;
    float sigma;
    float lognorm;   // 0.5*D*log(2*pi) + D*log(sigma)
    float w;         // 1/G
    float dpi_den;   // sqrt(w) * N            (:78)
    float mu_scale;  // 1/sqrt(w)              (:98)
    float sig_scale; // 1/sqrt(2w)             (:109)
};

// Optional fusions of the training step's front end (all NULL = plain encoder over pts):
//   pcA/pcB/noise: cloud c < B is pcA[c] + noise[c], cloud c >= B is pcB[c - B] (dpdist_and_aue.py:45,56-61); slice 0 of every
//                  cloud also writes the stacked encoder input pts_out [2B,N,3] and the query clouds q_out = [pcB ; pcA] (:69),
//                  so that dpd_stack_clouds is not launched;
//   ssq:           [C][kSlices][20] receives this slice's per-channel sums of squares (in the order of slice_ssq, mfv3d.hip); the caller then
//                  skips mfv3d_norm_kernel and the window gather applies the L2 scale instead (patch_rows.hip).
struct MfvFuse {
    const float* pcA; const float* pcB; const float* noise;
    float* pts_out; float* q_out;
    float* ssq;
    int B;
};

// FINAL (as-loss backward): instead of dpts, the evaluation's two input gradients leave the apply kernel (= dpd_asloss_combine on its output):
//   clouds c < B are pcA, queried by the BA half of the rows; c >= B are pcB, queried by the AB half (models/dpdist_and_aue.py:56-69):
//   g[r, d] = (dpts[c, n, d] + dX[qrow, E + d]) * upstream
struct AslossFinal {
    const float* dX;
    const float* scale;
    float* gA;
    float* gB;
    int B, KP, E;
};

// Index arithmetic without the integer divider gfx950 does not have (~35 VALU instructions per run-time division; the table loops of
// these kernels run three of them per entry with four waves per SIMD: 3.3k of the forward kernel's 21.7k cycles at B = 32): the usual
// sizes (m = 8, N = 64, slices of 16 points) are powers of two, so quotients are shifts; anything else keeps the division.
__device__ __forceinline__ int lg_or_neg(int d) { return (d > 0 && !(d & (d - 1))) ? __ffs(d) - 1 : -1; }
__device__ __forceinline__ int qdiv(int x, int d, int lg) { return lg >= 0 ? x >> lg : x / d; }

__device__ __forceinline__ void gauss_centre(const MfvConst& k, int g, float& cx, float& cy, float& cz) {
    // g = i*m*m + j*m + t  ->  (x,y,z) = (l[j], l[i], l[t])   (np.meshgrid 'xy' indexing, :47-48)
    const int m = k.m;
    const int i = g / (m * m), j = (g / m) % m, t = g % m;
    cx = k.ax.c[j];
    cy = k.ax.c[i];
    cz = k.ax.c[t];
}

__device__ __forceinline__ float pdf(const MfvConst& k, float zx, float zy, float zz) {
    // MultivariateNormalDiag.prob (:69-71): exp(-0.5*sum z^2 - (0.5*D*log 2pi + sum log sigma)), fp32 like TF
    return expf(-0.5f * (zx * zx + zy * zy + zz * zz) - k.lognorm);
}

__device__ __forceinline__ float pnorm(float x) {
    // sign(x) * max(|x|,1e-12)^0.5  (:119-121).  NaN in -> NaN out, as in the oracle (sign(NaN) = NaN there); the
    // only source of NaN is the reference's own 0/0 for a point that underflows every pdf.
    if (x != x) return x;
    const float s = (x > 0.f) ? 1.f : ((x < 0.f) ? -1.f : 0.f);
    return s * sqrtf(fmaxf(fabsf(x), 1e-12f));
}

// the 20 statistics of a Gaussian: sums {0, 2..4, 11..13}, maxima {1, 5..7, 14..16}, minima {8..10, 17..19}
__device__ __forceinline__ constexpr bool mfv_is_sum(int f) { return f == 0 || (f >= 2 && f < 5) || (f >= 11 && f < 14); }
__device__ __forceinline__ constexpr bool mfv_is_max(int f) { return f == 1 || (f >= 5 && f < 8) || (f >= 14 && f < 17); }
// index of statistic f among the 13 extrema {1, 5..10, 14..19} (tie-count / extremum rows 20 + index), -1 for a sum
__device__ __forceinline__ constexpr int mfv_tie_index(int f) { return f == 1 ? 0 : (f >= 5 && f < 11 ? f - 4 : (f >= 14 ? f - 7 : -1)); }
// the constant between raw statistic f and the value the power-1/2 normalisation sees (:81, :98, :109)
__device__ __forceinline__ float mfv_cst(const MfvConst& k, int f) { return (f < 2) ? 1.0f : ((f < 11) ? k.mu_scale : k.sig_scale); }

struct PQ {   // per-(point, Gaussian) quantities from the tables (identical expressions in every pass -> exact tie tests)
    float z[3], a[3], b[3], Q, dpi;
};

__device__ __forceinline__ PQ eval_pq(const float2 vx, const float2 vy, const float2 vz, float w, float inv_dpi) {
    PQ r;
    r.z[0] = vx.x; r.z[1] = vy.x; r.z[2] = vz.x;
    r.Q = (vx.y * vy.y) * vz.y;                                                // :73-74, factorised
    r.dpi = (r.Q - w) * inv_dpi;                                               // :78
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        r.a[d] = r.Q * r.z[d];                                                 // :87
        r.b[d] = r.Q * (r.z[d] * r.z[d] - 1.0f);                               // :100
    }
    return r;
}

// The 20 running statistics of one Gaussian over the points one lane walks, in registers.  fold() merges the lanes that hold the same
// Gaussian with the caller's three reducers (backward: sum_x32 / max_x32 / min_x32 over the two half-waves; packed forward: its four-group
// chain) into r[20] in statistic order -- SUMS, not yet means: the 1 / N is the caller's.
struct MfvStats {
    float pi_s, pi_mx, mu_s[3], mu_mx[3], mu_mn[3], sg_s[3], sg_mx[3], sg_mn[3];
    __device__ __forceinline__ void init() {
        pi_s = 0.f; pi_mx = -INFINITY;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            mu_s[d] = 0.f; mu_mx[d] = -INFINITY; mu_mn[d] = INFINITY;
            sg_s[d] = 0.f; sg_mx[d] = -INFINITY; sg_mn[d] = INFINITY;
        }
    }
    __device__ __forceinline__ void add(const PQ& q) {
        pi_s += q.dpi; pi_mx = fmaxf(pi_mx, q.dpi);
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            mu_s[d] += q.a[d]; mu_mx[d] = fmaxf(mu_mx[d], q.a[d]); mu_mn[d] = fminf(mu_mn[d], q.a[d]);
            sg_s[d] += q.b[d]; sg_mx[d] = fmaxf(sg_mx[d], q.b[d]); sg_mn[d] = fminf(sg_mn[d], q.b[d]);
        }
    }
    template <typename S, typename MX, typename MN>
    __device__ __forceinline__ void fold(float* r, S sum, MX mx, MN mn) const {
        r[0] = sum(pi_s);
        r[1] = mx(pi_mx);
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            r[2 + d] = sum(mu_s[d]);
            r[5 + d] = mx(mu_mx[d]);
            r[8 + d] = mn(mu_mn[d]);
            r[11 + d] = sum(sg_s[d]);
            r[14 + d] = mx(sg_mx[d]);
            r[17 + d] = mn(sg_mn[d]);
        }
    }
    __device__ __forceinline__ void fold_halves(float* r) const {      // lanes l, l ^ 32 hold the same Gaussian
        fold(r, [](float v) { return sum_x32(v); }, [](float v) { return max_x32(v); }, [](float v) { return min_x32(v); });
    }
};

// tie counts of the 13 max / min statistics against the extrema in rec[] (tf.reduce_max / min split the gradient evenly)
__device__ __forceinline__ void count_ties(float* cnt, const PQ& q, const float* rec) {
    cnt[0] += (q.dpi == rec[1]) ? 1.f : 0.f;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        cnt[1 + d] += (q.a[d] == rec[5 + d]) ? 1.f : 0.f;
        cnt[4 + d] += (q.a[d] == rec[8 + d]) ? 1.f : 0.f;
        cnt[7 + d] += (q.b[d] == rec[14 + d]) ? 1.f : 0.f;
        cnt[10 + d] += (q.b[d] == rec[17 + d]) ? 1.f : 0.f;
    }
}

// dQ_ng and the direct gradients ga / gb of a = Q z, b = Q (z z - 1) from the gradient dr[] w.r.t. the raw statistics: a mean reaches
// every point, a max / min the points that attain the extremum raw[] (dr already holds the share of a tie)
__device__ __forceinline__ float tie_grad(const float* dr, const float* raw, const PQ& q, float inv_dpi, float* ga, float* gb) {
    float dQ = (dr[0] + ((q.dpi == raw[1]) ? dr[1] : 0.f)) * inv_dpi;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        ga[d] = dr[2 + d] + ((q.a[d] == raw[5 + d]) ? dr[5 + d] : 0.f) + ((q.a[d] == raw[8 + d]) ? dr[8 + d] : 0.f);
        gb[d] = dr[11 + d] + ((q.b[d] == raw[14 + d]) ? dr[14 + d] : 0.f) + ((q.b[d] == raw[17 + d]) ? dr[17 + d] : 0.f);
        dQ += ga[d] * q.z[d] + gb[d] * (q.z[d] * q.z[d] - 1.0f);
    }
    return dQ;
}

// sum over the 16 waves' partials of element i, in wave order
__device__ __forceinline__ float sum16(const float* s, int stride, int i) {
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < 16; ++w) t += s[w * stride + i];
    return t;
}

// dfv -> gradient w.r.t. raw statistic f of one Gaussian:  fv = s * rsqrt(ss_f), s = pnorm(v), v = raw * cst (a mean: raw = sum / N);
// ss = sum_g s^2, dot = sum_g s * dfv over the Gaussians of the cloud, dy = this Gaussian's dfv
__device__ __forceinline__ float d_raw(int f, float raw_f, float ss, float dot, float dy, const MfvConst& k, float invN) {
    const float cst = mfv_cst(k, f);
    const float v = raw_f * cst;
    const float sv = pnorm(v);
    float ds;
    if (ss >= 1e-12f) {
        const float rs = 1.0f / sqrtf(ss);
        ds = rs * dy - sv * dot * rs * rs * rs;
    } else {
        ds = dy * 1e6f;                       // clamp active: y = s * rsqrt(1e-12)
    }
    // s = sign(v) max(|v|,1e-12)^0.5: gradient reaches v only where |v| >= 1e-12 (tf.maximum), tf.sign has none
    float dv = 0.f;
    if (fabsf(v) >= 1e-12f) dv = ds * 0.5f / sqrtf(fabsf(v));
    float d = dv * cst;
    if (mfv_is_sum(f)) d *= invN;             // reduce_mean: 1/N to every point
    return d;
}

// Tables of the backward for np_ points from point n0 of cloud p: zq[a][n][i] = {z, e/S}.  Ends on a barrier.
__device__ __forceinline__ void build_tables(const float* p, int n0, int np_, const MfvConst& k, float2* s_zq, float* s_S, int tid) {
    const int m = k.m;
    const int lg_m = lg_or_neg(m), lg_np = lg_or_neg(np_);
    for (int e = tid; e < 3 * np_ * m; e += kFwdThreads) {
        const int em = qdiv(e, m, lg_m), i = e - em * m, a = qdiv(em, np_, lg_np), ln = em - a * np_;
        const float z = (p[(n0 + ln) * 3 + a] - k.ax.c[i]) / k.sigma;
        s_zq[e] = make_float2(z, expf(-0.5f * (z * z)));
    }
    __syncthreads();
    for (int e = tid; e < 3 * np_; e += kFwdThreads) {
        float S = 0.f;
        for (int i = 0; i < m; ++i) S += s_zq[e * m + i].y;
        s_S[e] = S;
    }
    __syncthreads();
    for (int e = tid; e < 3 * np_ * m; e += kFwdThreads) s_zq[e].y = s_zq[e].y / s_S[qdiv(e, m, lg_m)];
    __syncthreads();
}

// ---- forward ------------------------------------------------------------------------------------------------------------------
// Merge of the eight point groups (lanes l, l^8, l^16, l^32 ... hold the same Gaussian).  __shfl_xor is a ds_bpermute (LDS crossbar +
// an address register) per value and stage: 60 of them made this merge as expensive as the point loop, and the section is VALU /
// issue bound (four waves per SIMD).  xor 8 is a DPP row rotate, xor 32 a v_permlane32_swap (both halves receive lower + upper),
// only xor 16 still goes through the crossbar (ds_swizzle, no address).  Same operands, same order: the same bits.
__device__ __forceinline__ float xor8(float v) { return dpp_move<0x128>(v); }                                                  // row_ror:8 = lane ^ 8
__device__ __forceinline__ float xor16(float v) { return __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(v), 0x401F)); }   // bit mode: xor 16
__device__ __forceinline__ float sum_groups8(float v) { v += xor8(v); v += xor16(v); return sum_x32(v); }
__device__ __forceinline__ float max_groups8(float v) { v = fmaxf(v, xor8(v)); v = fmaxf(v, xor16(v)); return max_x32(v); }
__device__ __forceinline__ float min_groups8(float v) { v = fminf(v, xor8(v)); v = fminf(v, xor16(v)); return min_x32(v); }
// merged sums / maxima / minima r[20] of one Gaussian ->the 20 statistics before the power-1/2, into its row of the stage
__device__ __forceinline__ void stage_row(const float* r, const MfvConst& k, float invN, float* row) {
    float v[kF];
    v[0] = r[0] * invN;                                                 // :81 reduce_mean
    v[1] = r[1];                                                        // :80
#pragma unroll
    for (int d = 0; d < 3; ++d) {                                       // :89-98, :102-109
        v[2 + d] = (r[2 + d] * invN) * k.mu_scale;
        v[5 + d] = r[5 + d] * k.mu_scale;
        v[8 + d] = r[8 + d] * k.mu_scale;
        v[11 + d] = (r[11 + d] * invN) * k.sig_scale;
        v[14 + d] = r[14 + d] * k.sig_scale;
        v[17 + d] = r[17 + d] * k.sig_scale;
    }
#pragma unroll
    for (int f = 0; f < kF; ++f) row[f] = v[f];
}

// Power-1/2 normalisation (:119-121) and coalesced store of the slice, one pass of ALL threads: out[g][f], 4 consecutive f of one g per
// thread.  (Inside the merge branch only 8 lanes of 64 were alive for 20 square roots each, four waves per SIMD queueing for the same
// VALU: 15k of the forward kernel's 30k cycles by s_memtime stamps.)  WRITE_BACK: the normalised values go back to the stage for the
// slice's sums of squares.
template <int THREADS, bool WRITE_BACK>
__device__ __forceinline__ void store_slice(float* __restrict__ out, float* s_stage, int gcount, bool bad, int tid) {
    const float qnan = __int_as_float(0x7fc00000);
    for (int i4 = tid; i4 < gcount * kF / 4; i4 += THREADS) {
        const int e = i4 * 4, g = e / kF, f = e % kF;
        float* sp = s_stage + g * kFP + f;
        float4 o = make_float4(pnorm(sp[0]), pnorm(sp[1]), pnorm(sp[2]), pnorm(sp[3]));
        if (WRITE_BACK) { sp[0] = o.x; sp[1] = o.y; sp[2] = o.z; sp[3] = o.w; }
        if (bad) o = make_float4(qnan, qnan, qnan, qnan);   // 0/0 at :74 poisons every statistic of the cloud
        *reinterpret_cast<float4*>(out + e) = o;
    }
}

// One record per KERNEL: the template parameter is the kernel itself, not its type -- the two forward kernels have the same
// signature (as have the two instantiations of the apply kernel), and a record keyed on the type let the first of them to pass
// 64 KiB answer for the other, which then launched without ever having been opted in.
template <auto Kern>
static int set_lds(size_t lds) {
    static LdsOptIn lds_opt;
    return ensure_dyn_lds(lds_opt, (const void*)Kern, lds);
}

// ---- dynamic LDS, in bytes (the layouts stand at the kernels) ----
inline size_t fwd_lds_bytes(int N, int m, int gslice) { return (size_t)(6 * N * m + 6 * N + gslice * kFP + 4 + 8 * kF) * sizeof(float); }
inline size_t fwd_tiled_lds_bytes(int tile, int m, int gslice) { return (size_t)(6 * tile * m + 6 * tile + gslice * kFP + 4) * sizeof(float); }
inline size_t bwd_lds_bytes(int N, int m) { return (size_t)(6 * N * m + 3 * N + 16 * 2 * kF + 2 * kF + N + 16 * N * 3 + 4) * sizeof(float); }
// statistics / apply kernel of the sliced and tiled backward, np = points of a slice or of a tile
inline size_t bwd_stats_lds_bytes(int np, int m) { return (size_t)(6 * np * m + 3 * np + 4) * sizeof(float); }
inline size_t bwd_sliced_lds_bytes(int np, int m) { return (size_t)(6 * np * m + 3 * np + np + 16 * np * 3 + 4) * sizeof(float); }

// ---- mfv3d.hip ----
int make_const(int N, int m, float sigma, MfvConst& k);
// The library's choice of tile: the largest multiple of 8 whose dynamic LDS stays at or under 64 KiB; 0 where there is none.
int default_tile(int m, bool backward);
// explicit tile: a multiple of 8, >= 8; 0: the library's.  Clamped to the points there are (rounded up to 8): the tables are sized by it.
int resolve_tile(int tile, int m, bool backward, int npoints, int& T);

}  // namespace dpd

// The pass bodies of the approximate matching (include/dpdist_capi.h: dpd_emd_fwd), written once: the paired kernels of emd.hip (a pass
// is a launch, the vectors live in the workspace) and the one-workgroup-per-pair kernel of emd_matrix.hip (a pass is a loop between
// two barriers, the vectors live in LDS) call the same scans and the same finishes, so with -ffp-contract=off a pair gets the same
// bits from either.  A scan is what ONE wave does for the point its lane owns over its quarter of the other cloud; a finish is what
// the owner does with the four partial sums, already combined as (p0 + p1) + (p2 + p3).
#pragma once
#include "common.h"

namespace dpd {

constexpr int kEmdThreads = 256;
constexpr int kEmdWaves = kEmdThreads / kWave;   // 4: the quarters of the other cloud
constexpr int kEmdMax = DPD_EMD_MAX_POINTS;      // 2048: a staged cloud is 32 KiB of LDS
constexpr int kEmdLevels = 10;

__device__ __forceinline__ float emd_exp2(float x) { return __builtin_amdgcn_exp2f(x); }
__device__ __forceinline__ float emd_rsqrt(float x) { return __builtin_amdgcn_rsqf(x); }

// level * log2(e) of the ten levels: exp(level d^2) = exp2(lv d^2)
struct EmdLevels {
    float v[kEmdLevels];
};
inline EmdLevels emd_levels() {
    EmdLevels lv;
    for (int i = 0; i < kEmdLevels; ++i) {
        const int j = 7 - i;
        const double level = j == -2 ? 0.0 : -(j >= 0 ? (double)(1 << (2 * j)) : 0.25);
        lv.v[i] = (float)(level * 1.4426950408889634074);
    }
    return lv;
}

// Row scan of the owner (x, y, z) of point k over s2[l0 .. l1) = {x2, y2, z2, remainR[l]}.  W: step 3 of the level with base-2 scale lw
// (rl = ratioL[k], sR = ratioR): acc[0] = sum w, acc[1] = sum w sqrt(d^2), acc[2..4] = sum w (x1 - x2) / sqrt(max(d^2, 1e-20)); mrow
// (or NULL) = match + k, written or added to (first) with row stride n.  R: step 1 of the level with scale lr: acc[5].
template <bool W, bool R>
__device__ __forceinline__ void emd_row_scan(const float4* __restrict__ s2, const float* __restrict__ sR, int l0, int l1, float x, float y,
                                             float z, float rl, float lw, float lr, float* __restrict__ mrow, int n, int first,
                                             float (&acc)[6]) {
    float sw = 0.f, sc = 0.f, gx = 0.f, gy = 0.f, gz = 0.f, sr = 0.f;
#pragma unroll 4
    for (int l = l0; l < l1; ++l) {
        const float4 q = s2[l];
        const float dx = x - q.x, dy = y - q.y, dz = z - q.z;
        const float d2 = (dx * dx + dy * dy) + dz * dz;
        if (W) {
            const float w = emd_exp2(lw * d2) * rl * sR[l];
            const float inv = emd_rsqrt(fmaxf(d2, 1e-20f));
            sw += w;
            sc += w * (d2 * inv);                        // w sqrt(d^2); 0 at d^2 = 0
            const float t = w * inv;
            gx += t * dx, gy += t * dy, gz += t * dz;
            if (mrow) {                                  // lanes = consecutive k: coalesced
                float* e = mrow + (size_t)l * n;
                *e = first ? w : *e + w;
            }
        }
        if (R) sr += emd_exp2(lr * d2) * q.w;
    }
    acc[0] = sw, acc[1] = sc, acc[2] = gx, acc[3] = gy, acc[4] = gz, acc[5] = sr;
}

// What the owner of point k does with the combined sums t of a row pass.  first: no level has run yet (remainL is its initial constant
// initL, the accumulators are written, not added to); g (or NULL) = grad1 + 3 k, which leaves scaled by gs.
template <bool W, bool R>
__device__ __forceinline__ void emd_row_finish(const float (&t)[6], int first, float initL, float& remainL, float& costk, float& ratioL,
                                               float* __restrict__ g, float gs) {
    float rem = (first && !W) ? initL : remainL;
    if (W) {
        rem = fmaxf(0.f, rem - t[0]);
        remainL = rem;
        costk = first ? t[1] : costk + t[1];
        if (g) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float v = first ? t[2 + c] : g[c] + t[2 + c];
                g[c] = v * gs;
            }
        }
    } else {
        remainL = rem;
    }
    if (R) ratioL = rem / (1e-9f + t[5]);
}

// Column scan of the owner (x, y, z) of point l over s1[k0 .. k1) = {x1, y1, z1, ratioL[k]}: step 2 of the level with base-2 scale lv.
// acc[0] = sum exp(level d^2) ratioL[k]; G: acc[1..3] = the same sum weighted by (x1 - x2) / sqrt(max(d^2, 1e-20)).
template <bool G>
__device__ __forceinline__ void emd_col_scan(const float4* __restrict__ s1, int k0, int k1, float x, float y, float z, float lv,
                                             float (&acc)[4]) {
    float s = 0.f, gx = 0.f, gy = 0.f, gz = 0.f;
#pragma unroll 4
    for (int k = k0; k < k1; ++k) {
        const float4 q = s1[k];
        const float dx = q.x - x, dy = q.y - y, dz = q.z - z;          // x1 - x2, the sign grad1 uses
        const float d2 = (dx * dx + dy * dy) + dz * dz;
        const float a = emd_exp2(lv * d2) * q.w;
        s += a;
        if (G) {
            const float t = a * emd_rsqrt(fmaxf(d2, 1e-20f));
            gx += t * dx, gy += t * dy, gz += t * dz;
        }
    }
    acc[0] = s, acc[1] = gx, acc[2] = gy, acc[3] = gz;
}

// What the owner of point l does with the combined sums t of a column pass; g = grad2 + 3 l (read only when G).
template <bool G>
__device__ __forceinline__ void emd_col_finish(const float (&t)[4], int first, float initR, float& remainR, float& ratioR,
                                               float* __restrict__ g, float gs) {
    const float rem = first ? initR : remainR;
    const float sum = rem * t[0];
    const float rr = fminf(rem / (sum + 1e-9f), 1.0f) * rem;
    ratioR = rr;
    remainR = fmaxf(0.f, rem - sum);
    if (G) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float v = first ? -(rr * t[1 + c]) : g[c] - rr * t[1 + c];
            g[c] = v * gs;
        }
    }
}

// ---- a pass as a launch: what one 256-thread workgroup does for one owner tile (64 points) of ONE pair.  The pass kernels of emd.hip
// call these with the pair's own n, m and rows of the padded widths (a dense batch: n = Wa, m = Wb for every pair).

struct EmdWs {            // the vectors of P pairs of padded widths Wa, Wb, carved from the caller's workspace, floats
    float* remainL;       // [P,Wa]
    float* ratioL;        // [P,Wa]
    float* costk;         // [P,Wa]  sum_l match[l][k] sqrt(d^2)
    float* remainR;       // [P,Wb]
    float* ratioR;        // [P,Wb]
};
using EmdVec = EmdWs;     // the same five pointers advanced to one pair

// the carve of dpd_emd_workspace_bytes(P, Wa, Wb) = dpd_emd_pairs_workspace_bytes(P, Wa, Wb)
inline EmdWs emd_carve(void* ws, int P, int Wa, int Wb) {
    float* f = (float*)ws;
    const size_t pa = (size_t)P * Wa, pb = (size_t)P * Wb;
    return EmdWs{f, f + pa, f + 2 * pa, f + 3 * pa, f + 3 * pa + pb};
}

// stage `cnt` points of cloud p [cnt,3] with their vector entry v (or the constant c when v is NULL) as float4 {x,y,z,v}
__device__ __forceinline__ void emd_stage(float4* s, const float* __restrict__ p, const float* __restrict__ v, float c, int cnt) {
    for (int i = threadIdx.x; i < cnt; i += kEmdThreads) s[i] = make_float4(p[i * 3], p[i * 3 + 1], p[i * 3 + 2], v ? v[i] : c);
}

// Row pass of owner tile `tile` of the pair p1 [n,3], p2 [m,3].  s2 [m] float4, sR [m] floats (W only), red: LDS of the workgroup.
// Lane i of EVERY wave owns point 64 tile + i; wave v scans quarter v of the other cloud.  grad1 / match: the pair's, or NULL.
template <bool W, bool R>
__device__ __forceinline__ void emd_row_tile(float4* __restrict__ s2, float* __restrict__ sR, float (*__restrict__ red)[6][kWave],
                                             const float* __restrict__ p1, const float* __restrict__ p2, int n, int m, int tile, float lw,
                                             float lr, int first, const EmdVec& v, float* __restrict__ grad1, float* __restrict__ match,
                                             float gs) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const float initL = (float)max(n, m) / (float)n, initR = (float)max(n, m) / (float)m;
    // step 1 of the first level reads the initial remainR; later ones read what the column pass left
    emd_stage(s2, p2, (first && !W) ? nullptr : v.remainR, initR, m);
    if (W)
        for (int i = threadIdx.x; i < m; i += kEmdThreads) sR[i] = v.ratioR[i];
    __syncthreads();

    const int k0 = tile * kWave + lane;
    const int k = min(k0, n - 1);                        // a tail lane recomputes the last point and stores nothing
    const float x = p1[k * 3], y = p1[k * 3 + 1], z = p1[k * 3 + 2];
    const float rl = W ? v.ratioL[k] : 0.f;
    float* mrow = match ? match + k : nullptr;

    const int per = (m + kEmdWaves - 1) / kEmdWaves;
    const int l0 = wave * per, l1 = min(m, l0 + per);
    float acc[6];
    emd_row_scan<W, R>(s2, sR, l0, l1, x, y, z, rl, lw, lr, k0 < n ? mrow : nullptr, n, first, acc);
#pragma unroll
    for (int c = 0; c < 6; ++c) red[wave][c][lane] = acc[c];
    __syncthreads();
    if (wave != 0 || k0 >= n) return;
    float t[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) t[c] = (red[0][c][lane] + red[1][c][lane]) + (red[2][c][lane] + red[3][c][lane]);
    emd_row_finish<W, R>(t, first, initL, v.remainL[k], v.costk[k], v.ratioL[k], grad1 ? grad1 + k * 3 : nullptr, gs);
}

// Column pass of owner tile `tile` of the pair: step 2 of the level with scale lv, and grad2's share of that level (G; grad2: the pair's).
template <bool G>
__device__ __forceinline__ void emd_col_tile(float4* __restrict__ s1, float (*__restrict__ red)[4][kWave], const float* __restrict__ p1,
                                             const float* __restrict__ p2, int n, int m, int tile, float lv, int first, const EmdVec& v,
                                             float* __restrict__ grad2, float gs) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    emd_stage(s1, p1, v.ratioL, 0.f, n);
    __syncthreads();

    const int l0 = tile * kWave + lane;
    const int l = min(l0, m - 1);
    const float x = p2[l * 3], y = p2[l * 3 + 1], z = p2[l * 3 + 2];

    const int per = (n + kEmdWaves - 1) / kEmdWaves;
    const int k0 = wave * per, k1 = min(n, k0 + per);
    float acc[4];
    emd_col_scan<G>(s1, k0, k1, x, y, z, lv, acc);
    red[wave][0][lane] = acc[0];
    if (G) red[wave][1][lane] = acc[1], red[wave][2][lane] = acc[2], red[wave][3][lane] = acc[3];
    __syncthreads();
    if (wave != 0 || l0 >= m) return;
    float t[4] = {};
#pragma unroll
    for (int c = 0; c < (G ? 4 : 1); ++c) t[c] = (red[0][c][lane] + red[1][c][lane]) + (red[2][c][lane] + red[3][c][lane]);
    emd_col_finish<G>(t, first, (float)max(n, m) / (float)m, v.remainR[l], v.ratioR[l], G ? grad2 + l * 3 : nullptr, gs);
}

// ---- the 21 pass launches of the matching over the pairs (b, b) of two sets (host side; defined in emd.hip, next to the pass kernels;
// dpd_emd_fwd and the per-pass form of emd_pairs.hip call it).  counts NULL: full sets.  g1 [P,Wa,3] / g2 [P,Wb,3] (either may be NULL)
// receive the gradients of each pair's real rows, scaled by gs in the last launch; match [P,Wb,Wa] (or NULL) is taken with NULL counts
// only (DPD_E_UNSUPPORTED otherwise); w.costk holds the per-point costs afterwards.
constexpr int kEmdMaxGrid = 1 << 20;   // workgroups along the pairs per launch; the kernels stride over their pairs beyond it
int emd_passes(const float* A, const int32_t* countsA, int Wa, const float* B, const int32_t* countsB, int Wb, int P, const EmdWs& w, float* g1,
               float* g2, float* match, float gs, hipStream_t s);

// ---- the pairs (b, b) of two sets through the one-workgroup-per-pair kernel of emd_matrix.hip (host side; emd_pairs.hip calls them).
// cost / dist [P] (either may be NULL); g1 [P,Wa,3] / g2 [P,Wb,3]: the unscaled d cost / d xyz of each pair's real rows (either may be NULL).
int em_diag_fwd(const float* A, const int32_t* countsA, int Wa, const float* B, const int32_t* countsB, int Wb, int P, float* cost,
                float* dist, hipStream_t s);
int em_diag_grads(const float* A, const int32_t* countsA, int Wa, const float* B, const int32_t* countsB, int Wb, int P, float* g1, float* g2,
                  hipStream_t s);

}  // namespace dpd

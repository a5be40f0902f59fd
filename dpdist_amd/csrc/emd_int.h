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

}  // namespace dpd

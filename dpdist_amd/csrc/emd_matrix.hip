// All-pairs Earth Mover's distance: cost[i,j] and dist[i,j] = cost / n_i of every pair (A_i, B_j) of two sets of clouds, and the gradients
// of the matrix under an upstream W (include/dpdist_capi.h: dpd_emd_matrix_fwd / _bwd; driven by dpdist_amd/emd.py).  A pair's value is
// dpd_emd_fwd's on that pair alone, bit for bit: the pass bodies are those of emd.hip (emd_int.h).
//
// One workgroup per pair, one launch.  The paired entry makes a pass a launch (22 dependent launches, launch-bound at 64 points); a matrix
// has Ca * Cb independent pairs, so here a pass is a loop between two barriers and everything a pass hands to the next stays in LDS:
//     s1 [Na] float4 {x1, y1, z1, ratioL[k]}     s2 [Nb] float4 {x2, y2, z2, remainR[l]}     remainL [Na]   costk [Na]   ratioR [Nb]
//     red [groups][4 quarters][6][64]            the partial sums of the owner tiles in flight
// sized from the padded widths (a 64-point pair takes 9 KiB, so a CU holds eight of them; 2048 / 2048 takes 94 KiB, or 112 KiB wide).
// The passes are those of dpd_emd_fwd: row<ratio> | col row<w,ratio> x 9 | col row<w> | cost.  An owner tile is 64 consecutive points;
// waves 4g .. 4g + 3 ("group" g) work the same tile, wave 4g + v scans quarter v of the other cloud, and the owner lanes of wave 4g
// combine the partials as (p0 + p1) + (p2 + p3) -- dpd_emd_fwd's order.  The narrow form has one group (256 threads), the wide form four
// (1024 threads, four tiles in flight); which group works a tile changes no bit.  costk is summed as emd_finish_kernel does it: thread
// t < 256 takes k = t, t + 256, ..., then the tree of block_sum_256.
//
// Backward: the match is a constant and nothing is kept by the forward, so the pair kernel runs again and accumulates the contract's
// d cost / d xyz1 and d cost / d xyz2 of its pair level by level, in the caller's workspace ([Ca,Cb,Na,3] then [Ca,Cb,Nb,3]; a row is
// read and written by its owner lane alone).  A second kernel folds them: dA[i,k] = sum_j (W[i,j] / n_i) g1(i,j)[k], j ascending, and
// dB[j,l] = sum_i (W[i,j] / n_i) g2(i,j)[l], i ascending, a left fold from +0.0 (or from dB's value: accumulate_dB).  No atomics, one
// writer per element, padding never read, rows at or beyond a count written +0.0.
//
// The same kernel serves the pairs (b, b) of two sets of equal length (em_diag_fwd / em_diag_grads below: the one-launch form of
// dpd_emd_pairs_fwd / _bwd, emd_pairs.hip) through its pair map: diag != 0 takes p -> (p, p) instead of p -> (p / Cb, p % Cb).
#include "emd_int.h"

#ifndef DPD_EMD_WIDE_FROM
#define DPD_EMD_WIDE_FROM 256   // the wide form from this padded width on (the larger of Na, Nb); measured, DESIGN.md 3.12
#endif

namespace dpd {

constexpr int kEmMaxGrid = 1 << 20;   // workgroups per launch; the kernels stride over their pairs beyond it
constexpr int kEmRed = kEmdWaves * 6 * kWave;   // floats of partial sums per group

// Row pass of one pair over its owner tiles; the barrier that ends the last tile ends the pass.
template <int GROUPS, bool W, bool R, bool COST, bool G1>
__device__ __forceinline__ void em_row_pass(float4* __restrict__ s1, const float4* __restrict__ s2, const float* __restrict__ ratioR,
                                            float* __restrict__ remainL, float* __restrict__ costk, float* __restrict__ red, int n, int m,
                                            float lw, float lr, int first, float initL, float* __restrict__ g1) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave, grp = wave / kEmdWaves, q = wave % kEmdWaves;
    const int per = (m + kEmdWaves - 1) / kEmdWaves;
    const int l0 = q * per, l1 = min(m, l0 + per);
    const int tiles = (n + kWave - 1) / kWave;
    float* mine = red + (grp * kEmdWaves + q) * 6 * kWave + lane;
    const float* part = red + grp * kEmRed + lane;
    for (int t0 = 0; t0 < tiles; t0 += GROUPS) {
        const int tile = t0 + grp;
        const bool live = tile < tiles;                    // wave-uniform
        const int k0 = tile * kWave + lane;
        const int k = min(k0, n - 1);                      // a tail lane recomputes the last point and stores nothing
        if (live) {
            const float4 o = s1[k];
            float acc[6];
            emd_row_scan<W, R>(s2, ratioR, l0, l1, o.x, o.y, o.z, W ? o.w : 0.f, lw, lr, nullptr, n, first, acc);
            if (W) {
                mine[0] = acc[0];
                if (COST) mine[kWave] = acc[1];
                if (G1) mine[2 * kWave] = acc[2], mine[3 * kWave] = acc[3], mine[4 * kWave] = acc[4];
            }
            if (R) mine[5 * kWave] = acc[5];
        }
        __syncthreads();
        if (live && q == 0 && k0 < n) {
            float t[6] = {};
#pragma unroll
            for (int c = 0; c < 6; ++c) {
                const bool used = c == 0 ? W : c == 1 ? (W && COST) : c == 5 ? R : (W && G1);
                if (used)
                    t[c] = (part[c * kWave] + part[(6 + c) * kWave]) + (part[(12 + c) * kWave] + part[(18 + c) * kWave]);
            }
            emd_row_finish<W, R>(t, first, initL, remainL[k], costk[k], s1[k].w, G1 ? g1 + k * 3 : nullptr, 1.f);
        }
        __syncthreads();
    }
}

// Column pass of one pair over its owner tiles.
template <int GROUPS, bool G2>
__device__ __forceinline__ void em_col_pass(const float4* __restrict__ s1, float4* __restrict__ s2, float* __restrict__ ratioR,
                                            float* __restrict__ red, int n, int m, float lv, int first, float initR, float* __restrict__ g2) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave, grp = wave / kEmdWaves, q = wave % kEmdWaves;
    const int per = (n + kEmdWaves - 1) / kEmdWaves;
    const int k0 = q * per, k1 = min(n, k0 + per);
    const int tiles = (m + kWave - 1) / kWave;
    float* mine = red + (grp * kEmdWaves + q) * 6 * kWave + lane;
    const float* part = red + grp * kEmRed + lane;
    for (int t0 = 0; t0 < tiles; t0 += GROUPS) {
        const int tile = t0 + grp;
        const bool live = tile < tiles;
        const int l0 = tile * kWave + lane;
        const int l = min(l0, m - 1);
        if (live) {
            const float4 o = s2[l];
            float acc[4];
            emd_col_scan<G2>(s1, k0, k1, o.x, o.y, o.z, lv, acc);
            mine[0] = acc[0];
            if (G2) mine[kWave] = acc[1], mine[2 * kWave] = acc[2], mine[3 * kWave] = acc[3];
        }
        __syncthreads();
        if (live && q == 0 && l0 < m) {
            float t[4] = {};
#pragma unroll
            for (int c = 0; c < (G2 ? 4 : 1); ++c)
                t[c] = (part[c * kWave] + part[(6 + c) * kWave]) + (part[(12 + c) * kWave] + part[(18 + c) * kWave]);
            emd_col_finish<G2>(t, first, initR, s2[l].w, ratioR[l], G2 ? g2 + l * 3 : nullptr, 1.f);
        }
        __syncthreads();
    }
}

// COST: the forward (cost / dist); G1 / G2: the backward's per-pair gradients into gw1 [pairs,Na,3] / gw2 [pairs,Nb,3].
// diag: the pair map p -> (p, p) over Ca = Cb clouds (the one-launch form of dpd_emd_pairs_fwd / _bwd) instead of p -> (p / Cb, p % Cb).
template <int GROUPS, bool COST, bool G1, bool G2>
__global__ __launch_bounds__(GROUPS* kEmdThreads) void emd_matrix_kernel(const float* __restrict__ A, const int32_t* __restrict__ countsA, int Ca,
                                                                        int Na, const float* __restrict__ B,
                                                                        const int32_t* __restrict__ countsB, int Cb, int Nb, EmdLevels lv,
                                                                        float* __restrict__ cost, float* __restrict__ dist,
                                                                        float* __restrict__ gw1, float* __restrict__ gw2, int diag) {
    extern __shared__ __align__(16) float4 em_lds[];
    float4* s1 = em_lds;                                   // [Na] {x1, y1, z1, ratioL}
    float4* s2 = s1 + Na;                                  // [Nb] {x2, y2, z2, remainR}
    float* remainL = reinterpret_cast<float*>(s2 + Nb);    // [Na]
    float* costk = remainL + Na;                           // [Na]
    float* ratioR = costk + Na;                            // [Nb]
    float* red = ratioR + Nb;                              // [GROUPS][4][6][64]
    float* red4 = red + GROUPS * kEmRed;                   // [4]
    const int nthr = GROUPS * kEmdThreads;
    const long long pairs = diag ? (long long)Ca : (long long)Ca * Cb;
    for (long long p = blockIdx.x; p < pairs; p += gridDim.x) {   // 64-bit: the last stride may pass 2^31
        const int i = diag ? (int)p : (int)(p / Cb), j = diag ? (int)p : (int)(p % Cb);
        const int n = ragged_count(countsA, i, Na), m = ragged_count(countsB, j, Nb);
        const float* a = A + (size_t)i * Na * 3;
        const float* b = B + (size_t)j * Nb * 3;
        float* g1 = G1 ? gw1 + (size_t)p * Na * 3 : nullptr;
        float* g2 = G2 ? gw2 + (size_t)p * Nb * 3 : nullptr;
        const float initL = (float)max(n, m) / (float)n, initR = (float)max(n, m) / (float)m;
        __syncthreads();                                   // the pair before this one is done with the LDS
        for (int k = threadIdx.x; k < n; k += nthr) {
            s1[k] = make_float4(a[k * 3], a[k * 3 + 1], a[k * 3 + 2], 0.f);
            remainL[k] = initL;
        }
        for (int l = threadIdx.x; l < m; l += nthr) s2[l] = make_float4(b[l * 3], b[l * 3 + 1], b[l * 3 + 2], initR);
        __syncthreads();
        em_row_pass<GROUPS, false, true, COST, G1>(s1, s2, ratioR, remainL, costk, red, n, m, 0.f, lv.v[0], 1, initL, g1);
#pragma unroll 1
        for (int level = 0; level < kEmdLevels - 1; ++level) {
            em_col_pass<GROUPS, G2>(s1, s2, ratioR, red, n, m, lv.v[level], level == 0, initR, g2);
            em_row_pass<GROUPS, true, true, COST, G1>(s1, s2, ratioR, remainL, costk, red, n, m, lv.v[level], lv.v[level + 1], level == 0, initL,
                                                      g1);
        }
        em_col_pass<GROUPS, G2>(s1, s2, ratioR, red, n, m, lv.v[kEmdLevels - 1], 0, initR, g2);
        em_row_pass<GROUPS, true, false, COST, G1>(s1, s2, ratioR, remainL, costk, red, n, m, lv.v[kEmdLevels - 1], 0.f, 0, initL, g1);
        if (COST) {                                        // emd_finish_kernel's order: stride-256 partials, then block_sum_256's tree
            float s = 0.f;
            if (threadIdx.x < 256)
                for (int k = threadIdx.x; k < n; k += 256) s += costk[k];
            s = wave_sum(s);
            if (threadIdx.x < 256 && (threadIdx.x & 63) == 0) red4[threadIdx.x >> 6] = s;
            __syncthreads();
            if (threadIdx.x == 0) {
                const float c = (red4[0] + red4[1]) + (red4[2] + red4[3]);
                if (cost) cost[p] = c;
                if (dist) dist[p] = c / (float)n;
            }
        }
    }
}

// dA[i,k,c] = sum_j (W[i,j] / n_i) g1(i,j)[k,c], j ascending from +0.0; one thread per element
__global__ __launch_bounds__(256) void emd_matrix_fold_a_kernel(const float* __restrict__ gw1, const int32_t* __restrict__ countsA, int Ca, int Na,
                                                                int Cb, const float* __restrict__ W, float* __restrict__ dA) {
    const long long total = (long long)Ca * Na * 3, row = (long long)Na * 3;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const int i = (int)(e / row), r = (int)(e % row);
        const int n = ragged_count(countsA, i, Na);
        float acc = 0.f;
        if (r / 3 < n) {
            const float* g = gw1 + (size_t)i * Cb * row + r;
            const float* w = W + (size_t)i * Cb;
            for (int j = 0; j < Cb; ++j) acc += (w[j] / (float)n) * g[(size_t)j * row];
        }
        dA[e] = acc;
    }
}

// dB[j,l,c] = sum_i (W[i,j] / n_i) g2(i,j)[l,c], i ascending from +0.0 or from dB's value; one thread per element
__global__ __launch_bounds__(256) void emd_matrix_fold_b_kernel(const float* __restrict__ gw2, const int32_t* __restrict__ countsA, int Ca, int Na,
                                                                const int32_t* __restrict__ countsB, int Cb, int Nb,
                                                                const float* __restrict__ W, float* __restrict__ dB, int accumulate) {
    const long long total = (long long)Cb * Nb * 3, row = (long long)Nb * 3;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const int j = (int)(e / row), r = (int)(e % row);
        const int m = ragged_count(countsB, j, Nb);
        float acc = 0.f;
        if (r / 3 < m) {
            if (accumulate) acc = dB[e];
            const float* g = gw2 + (size_t)j * row + r;
            for (int i = 0; i < Ca; ++i) {
                const float n = (float)ragged_count(countsA, i, Na);
                acc += (W[(size_t)i * Cb + j] / n) * g[(size_t)i * Cb * row];
            }
        }
        dB[e] = acc;
    }
}

static int em_check_dims(int Ca, int Na, int Cb, int Nb) {
    if (Ca < 1 || Cb < 1 || (long long)Ca * (long long)Cb >= (1ll << 31)) return DPD_E_DIM;
    if (Na < 1 || Nb < 1 || Na > kEmdMax || Nb > kEmdMax) return DPD_E_UNSUPPORTED;
    return 0;
}

template <int GROUPS, bool COST, bool G1, bool G2>
static int em_launch(const float* A, const int32_t* countsA, int Ca, int Na, const float* B, const int32_t* countsB, int Cb, int Nb, float* cost,
                     float* dist, float* gw1, float* gw2, int diag, hipStream_t s) {
    auto kern = emd_matrix_kernel<GROUPS, COST, G1, G2>;
    const size_t lds = (size_t)(Na + Nb) * sizeof(float4) + ((size_t)2 * Na + Nb + GROUPS * kEmRed + 4) * sizeof(float);
    static LdsOptIn lds_opt;   // one per template instantiation
    if (int rc = ensure_dyn_lds(lds_opt, (const void*)kern, lds)) return rc;
    const long long pairs = diag ? (long long)Ca : (long long)Ca * Cb;
    DPD_LAUNCH(kern, dim3(pairs < kEmMaxGrid ? (int)pairs : kEmMaxGrid), dim3(GROUPS * kEmdThreads), lds, s, A, countsA, Ca, Na, B, countsB, Cb,
               Nb, emd_levels(), cost, dist, gw1, gw2, diag);
    DPD_CHECK_LAUNCH();
    return 0;
}

template <bool COST, bool G1, bool G2>
static int em_pairs(const float* A, const int32_t* countsA, int Ca, int Na, const float* B, const int32_t* countsB, int Cb, int Nb, float* cost,
                    float* dist, float* gw1, float* gw2, hipStream_t s, int diag = 0) {
    if ((Na > Nb ? Na : Nb) >= DPD_EMD_WIDE_FROM)
        return em_launch<4, COST, G1, G2>(A, countsA, Ca, Na, B, countsB, Cb, Nb, cost, dist, gw1, gw2, diag, s);
    return em_launch<1, COST, G1, G2>(A, countsA, Ca, Na, B, countsB, Cb, Nb, cost, dist, gw1, gw2, diag, s);
}

int em_diag_fwd(const float* A, const int32_t* countsA, int Wa, const float* B, const int32_t* countsB, int Wb, int P, float* cost,
                float* dist, hipStream_t s) {
    return em_pairs<true, false, false>(A, countsA, P, Wa, B, countsB, P, Wb, cost, dist, nullptr, nullptr, s, 1);
}

int em_diag_grads(const float* A, const int32_t* countsA, int Wa, const float* B, const int32_t* countsB, int Wb, int P, float* g1, float* g2,
                  hipStream_t s) {
    if (g1 && g2) return em_pairs<false, true, true>(A, countsA, P, Wa, B, countsB, P, Wb, nullptr, nullptr, g1, g2, s, 1);
    if (g1) return em_pairs<false, true, false>(A, countsA, P, Wa, B, countsB, P, Wb, nullptr, nullptr, g1, g2, s, 1);
    return em_pairs<false, false, true>(A, countsA, P, Wa, B, countsB, P, Wb, nullptr, nullptr, g1, g2, s, 1);
}

}  // namespace dpd

extern "C" size_t dpd_emd_matrix_workspace_bytes(int Ca, int Na, int Cb, int Nb) {
    if (dpd::em_check_dims(Ca, Na, Cb, Nb)) return 0;
    return (size_t)Ca * (size_t)Cb * (size_t)(Na + Nb) * 3 * sizeof(float);
}

extern "C" int dpd_emd_matrix_fwd(const float* A, const int32_t* countsA, int Ca, int Na, const float* B, const int32_t* countsB, int Cb, int Nb,
                                  float* cost, float* dist, void* stream) {
    using namespace dpd;
    if (!A || !B || (!cost && !dist)) return DPD_E_NULL;
    if (const int rc = em_check_dims(Ca, Na, Cb, Nb)) return rc;
    return em_pairs<true, false, false>(A, countsA, Ca, Na, B, countsB, Cb, Nb, cost, dist, nullptr, nullptr, (hipStream_t)stream);
}

extern "C" int dpd_emd_matrix_bwd(const float* A, const int32_t* countsA, int Ca, int Na, const float* B, const int32_t* countsB, int Cb, int Nb,
                                  const float* W, float* dA, float* dB, int accumulate_dB, void* ws, size_t ws_bytes, void* stream) {
    using namespace dpd;
    if (!A || !B || !W || (!dA && !dB)) return DPD_E_NULL;
    if (const int rc = em_check_dims(Ca, Na, Cb, Nb)) return rc;
    if (!ws || ws_bytes < dpd_emd_matrix_workspace_bytes(Ca, Na, Cb, Nb)) return DPD_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    float* gw1 = (float*)ws;
    float* gw2 = gw1 + (size_t)Ca * Cb * Na * 3;
    int rc;
    if (dA && dB)
        rc = em_pairs<false, true, true>(A, countsA, Ca, Na, B, countsB, Cb, Nb, nullptr, nullptr, gw1, gw2, s);
    else if (dA)
        rc = em_pairs<false, true, false>(A, countsA, Ca, Na, B, countsB, Cb, Nb, nullptr, nullptr, gw1, gw2, s);
    else
        rc = em_pairs<false, false, true>(A, countsA, Ca, Na, B, countsB, Cb, Nb, nullptr, nullptr, gw1, gw2, s);
    if (rc) return rc;
    if (dA) {
        const long long blocks = ((long long)Ca * Na * 3 + 255) / 256;
        DPD_LAUNCH(emd_matrix_fold_a_kernel, dim3(blocks < kEmMaxGrid ? (int)blocks : kEmMaxGrid), dim3(256), 0, s, (const float*)gw1, countsA, Ca,
                   Na, Cb, W, dA);
        DPD_CHECK_LAUNCH();
    }
    if (dB) {
        const long long blocks = ((long long)Cb * Nb * 3 + 255) / 256;
        DPD_LAUNCH(emd_matrix_fold_b_kernel, dim3(blocks < kEmMaxGrid ? (int)blocks : kEmMaxGrid), dim3(256), 0, s, (const float*)gw2, countsA, Ca,
                   Na, countsB, Cb, Nb, W, dB, accumulate_dB);
        DPD_CHECK_LAUNCH();
    }
    return 0;
}

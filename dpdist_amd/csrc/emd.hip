// Earth Mover's distance between two point sets by approximate matching (the published scheme of Fan et al.), the third loss of the
// registration comparison (pcrnet-registration/run_train_and_eval_PCRNet.bash:64-72; utils/tf_util_loss.py:42-47 earth_mover).
// The contract is stated in include/dpdist_capi.h (dpd_emd_fwd); it is the definition, there is no reference binary.
//
// Ten levels, each three dependent passes over the n x m pair grid.  A pass is either a row pass (a thread owns a point k of xyz1 and
// sums over every l of xyz2) or a column pass (a thread owns l and sums over every k), and one pass needs the finished vectors of the one
// before it, so a pass is a launch and the stream is the barrier:
//     row<ratio>(L7) | col(L7) row<w,ratio>(L7,L6) | col(L6) row<w,ratio>(L6,L5) | ... | col(L-2) row<w>(L-2) | finish
// Step 3 of a level and step 1 of the next are both row passes over the same pairs, so they share one launch (and one d^2): 21 pass
// launches and one finish.  A pair's rows are split over ceil(n / 64) workgroups, so a 2048-point batch of 16 fills the device
// (512 workgroups) where one workgroup per pair would use 16 of the 256 CUs.
//
// Fused form: w(k,l) = exp(level d^2) ratioL[k] ratioR[l] is what a level adds to match[l][k], and cost and both gradients are linear in the
// match, so they are accumulated while w is in registers and match [B,m,n] is written only when the caller asks for it:
//     row pass (owner k):     cost_k += sum_l w sqrt(d^2),   grad1[k] += sum_l w (x1_k - x2_l) / sqrt(max(d^2, 1e-20))
//     column pass (owner l):  grad2[l] -= ratioR[l] * sum_k exp(level d^2) ratioL[k] (x1_k - x2_l) / sqrt(max(d^2, 1e-20))
// (ratioR[l] is a factor of every w of column l, so the column pass that computes it can apply it to a sum it already runs over).
//
// Geometry: 256 threads = 4 waves.  Lane i of EVERY wave owns point 64 * blockIdx.y + i; the other cloud sits in LDS as float4
// {x, y, z, its vector entry} and wave v scans quarter v of it (all lanes read one address: a broadcast ds_read_b128 per pair of points).
// The four partial sums of a point are combined through LDS as (p0 + p1) + (p2 + p3).  Every sum has one order, there are no atomics, and
// every output element has one writer per launch: two runs give identical bits.
// exp goes through v_exp_f32 (base 2) with log2(e) folded into the level on the host; 1 / sqrt through v_rsq_f32.
// The scan of a wave and the finish of an owner are written once, in emd_int.h: the all-pairs kernel of emd_matrix.hip calls them too;
// so is what a workgroup does for one owner tile of one pair (emd_row_tile, emd_col_tile).  The pass kernels and their launch schedule
// (emd_passes) below are the only ones: the per-pass form of the ragged pairs (emd_pairs.hip) runs them with counts.
#include "emd_int.h"

namespace dpd {

// The pass kernels serve "pair b of two sets with optional counts and padded strides": A [P,Wa,3], B [P,Wb,3]; the vectors, grad1 / grad2
// and match are rows of the padded widths.  dpd_emd_fwd: counts = NULL, Wa = n, Wb = m; the per-pass form of emd_pairs.hip: match = NULL,
// gs = 1.  Grid (min(P, kEmdMaxGrid), owner tiles of the padded width); a tile wholly beyond its pair's count leaves before a barrier.

// the five vectors of pair b: rows of the padded widths
__device__ __forceinline__ EmdVec emd_vec(const EmdWs& ws, long long b, int Wa, int Wb) {
    const size_t ba = (size_t)b * Wa, bb = (size_t)b * Wb;
    return EmdVec{ws.remainL + ba, ws.ratioL + ba, ws.costk + ba, ws.remainR + bb, ws.ratioR + bb};
}

// Row pass.  W: step 3 of the level whose base-2 exponent scale is lw (match += w, remainL -= sum w, cost and grad1);
// R: step 1 of the level with scale lr (ratioL).  first: no level has run yet (remainL / remainR are their initial constants, the
// accumulators are written, not added to); gs is 1 except in the last launch of the dense entry, where grad1 leaves scaled.
// match [P,Wb,Wa] is an argument of the M instances only (the branch on it sits in the scan's inner loop, so the training paths run the
// instances without it); its row stride is the pair's n, so it goes with counts = NULL only (emd_passes refuses the combination).
template <bool W, bool R, bool M>
__global__ __launch_bounds__(kEmdThreads) void emd_row_kernel(const float* __restrict__ A, const int32_t* __restrict__ countsA, int Wa,
                                                              const float* __restrict__ B, const int32_t* __restrict__ countsB, int Wb,
                                                              long long P, float lw, float lr, int first, EmdWs ws, float* __restrict__ grad1,
                                                              float* __restrict__ match, float gs) {
    __shared__ float4 s2[kEmdMax];                       // {x2, y2, z2, remainR[l]}
    __shared__ float sR[W ? kEmdMax : 1];                // ratioR[l]
    __shared__ float red[kEmdWaves][6][kWave];
    const int tile = blockIdx.y;
    for (long long b = blockIdx.x; b < P; b += gridDim.x) {
        const int n = ragged_count(countsA, (int)b, Wa), m = ragged_count(countsB, (int)b, Wb);
        if (tile * kWave >= n) continue;                 // a tile of padding: nothing to own
        __syncthreads();                                 // the pair before this one is done with the LDS
        emd_row_tile<W, R>(s2, sR, red, A + (size_t)b * Wa * 3, B + (size_t)b * Wb * 3, n, m, tile, lw, lr, first, emd_vec(ws, b, Wa, Wb),
                           grad1 ? grad1 + (size_t)b * Wa * 3 : nullptr, M ? match + (size_t)b * Wb * Wa : nullptr, gs);
    }
}

// Column pass: step 2 of the level with base-2 exponent scale lv, and grad2's share of that level (G; grad2 is read only then).
template <bool G>
__global__ __launch_bounds__(kEmdThreads) void emd_col_kernel(const float* __restrict__ A, const int32_t* __restrict__ countsA, int Wa,
                                                              const float* __restrict__ B, const int32_t* __restrict__ countsB, int Wb,
                                                              long long P, float lv, int first, EmdWs ws, float* __restrict__ grad2, float gs) {
    __shared__ float4 s1[kEmdMax];                       // {x1, y1, z1, ratioL[k]}
    __shared__ float red[kEmdWaves][4][kWave];
    const int tile = blockIdx.y;
    for (long long b = blockIdx.x; b < P; b += gridDim.x) {
        const int n = ragged_count(countsA, (int)b, Wa), m = ragged_count(countsB, (int)b, Wb);
        if (tile * kWave >= m) continue;
        __syncthreads();
        emd_col_tile<G>(s1, red, A + (size_t)b * Wa * 3, B + (size_t)b * Wb * 3, n, m, tile, lv, first, emd_vec(ws, b, Wa, Wb),
                        G ? grad2 + (size_t)b * Wb * 3 : nullptr, gs);
    }
}

// cost[b] = sum_k costk[b][k] and loss = mean_b cost[b] / n, one workgroup, fixed order
__global__ __launch_bounds__(256) void emd_finish_kernel(const float* __restrict__ costk, int B, int n, float* __restrict__ cost,
                                                         float* __restrict__ loss) {
    __shared__ float red[4];
    float tot = 0.f;
    for (int b = 0; b < B; ++b) {
        float s = 0.f;
        for (int k = threadIdx.x; k < n; k += 256) s += costk[(size_t)b * n + k];
        s = block_sum_256(s, red);
        if (threadIdx.x == 0) cost[b] = s;
        tot += s / (float)n;
    }
    if (threadIdx.x == 0) loss[0] = tot / (float)B;
}

// cost and gradients of a GIVEN match (the op's match_cost): dir 0 owns k (cost, grad1), dir 1 owns l (grad2)
__global__ __launch_bounds__(kEmdThreads) void emd_match_cost_kernel(const float* __restrict__ xyz1, const float* __restrict__ xyz2, int n,
                                                                     int m, const float* __restrict__ match, int chunks1,
                                                                     float* __restrict__ costk, float* __restrict__ grad1,
                                                                     float* __restrict__ grad2, float gs) {
    __shared__ float4 so[kEmdMax];
    __shared__ float red[kEmdWaves][4][kWave];
    const int b = blockIdx.x, lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const bool dir = (int)blockIdx.y >= chunks1;
    const int chunk = dir ? blockIdx.y - chunks1 : blockIdx.y;
    const int nown = dir ? m : n, noth = dir ? n : m;
    const float* own = (dir ? xyz2 : xyz1) + (size_t)b * nown * 3;
    emd_stage(so, (dir ? xyz1 : xyz2) + (size_t)b * noth * 3, nullptr, 0.f, noth);
    __syncthreads();
    const int i0 = chunk * kWave + lane, i = min(i0, nown - 1);
    const float x = own[i * 3], y = own[i * 3 + 1], z = own[i * 3 + 2];
    const float* mt = match + (size_t)b * m * n;
    const int per = (noth + kEmdWaves - 1) / kEmdWaves;
    const int j0 = wave * per, j1 = min(noth, j0 + per);
    float sc = 0.f, gx = 0.f, gy = 0.f, gz = 0.f;
    for (int j = j0; j < j1; ++j) {
        const float4 q = so[j];
        const float dx = x - q.x, dy = y - q.y, dz = z - q.z;          // own - other: d cost / d own
        const float d2 = (dx * dx + dy * dy) + dz * dz;
        const float w = dir ? mt[(size_t)i * n + j] : mt[(size_t)j * n + i];
        const float inv = emd_rsqrt(fmaxf(d2, 1e-20f));
        sc += w * (d2 * inv);
        const float t = w * inv;
        gx += t * dx, gy += t * dy, gz += t * dz;
    }
    red[wave][0][lane] = sc, red[wave][1][lane] = gx, red[wave][2][lane] = gy, red[wave][3][lane] = gz;
    __syncthreads();
    if (wave != 0 || i0 >= nown) return;
    float t[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) t[c] = (red[0][c][lane] + red[1][c][lane]) + (red[2][c][lane] + red[3][c][lane]);
    if (!dir) costk[(size_t)b * n + i] = t[0];
    float* g = dir ? grad2 : grad1;
    if (g)
        for (int c = 0; c < 3; ++c) g[((size_t)b * nown + i) * 3 + c] = t[1 + c] * gs;
}

static int emd_check(const void* xyz1, const void* xyz2, int B, int n, int m, const void* cost, const void* loss, const void* ws,
                     size_t ws_bytes) {
    if (!xyz1 || !xyz2 || !cost || !loss || !ws) return DPD_E_NULL;
    if (B <= 0 || n <= 0 || m <= 0) return DPD_E_DIM;
    if (n > kEmdMax || m > kEmdMax) return DPD_E_UNSUPPORTED;
    if (ws_bytes < dpd_emd_workspace_bytes(B, n, m)) return DPD_E_WORKSPACE;
    return 0;
}

// The launch schedule of the matching (contract in emd_int.h; emd_pairs.hip calls it too): row<ratio> | (col, row) x 10, 21 launches on s
int emd_passes(const float* A, const int32_t* countsA, int Wa, const float* B, const int32_t* countsB, int Wb, int P, const EmdWs& w, float* g1,
               float* g2, float* match, float gs, hipStream_t s) {
    if (match && (countsA || countsB)) return DPD_E_UNSUPPORTED;       // match's row stride is the pair's n: full sets only
    const int px = P < kEmdMaxGrid ? P : kEmdMaxGrid;
    const dim3 grow(px, (Wa + kWave - 1) / kWave), gcol(px, (Wb + kWave - 1) / kWave), blk(kEmdThreads);
    const long long PP = P;
    const EmdLevels levels = emd_levels();
    const float* lv = levels.v;
#define EMD_ROW(W, R, M, lw, lr, first, g) \
    DPD_LAUNCH((emd_row_kernel<W, R, M>), grow, blk, 0, s, A, countsA, Wa, B, countsB, Wb, PP, lw, lr, first, w, g1, match, g)
#define EMD_COL(G, lv, first, g) DPD_LAUNCH((emd_col_kernel<G>), gcol, blk, 0, s, A, countsA, Wa, B, countsB, Wb, PP, lv, first, w, g2, g)
    EMD_ROW(false, true, false, 0.f, lv[0], 1, 1.f);
    DPD_CHECK_LAUNCH();
    for (int i = 0; i < kEmdLevels; ++i) {
        const int first = i == 0;
        const bool last = i == kEmdLevels - 1;
        if (g2) EMD_COL(true, lv[i], first, last ? gs : 1.f);
        else EMD_COL(false, lv[i], first, 1.f);
        DPD_CHECK_LAUNCH();
        if (!last && match) EMD_ROW(true, true, true, lv[i], lv[i + 1], first, 1.f);
        else if (!last) EMD_ROW(true, true, false, lv[i], lv[i + 1], first, 1.f);
        else if (match) EMD_ROW(true, false, true, lv[i], 0.f, first, gs);
        else EMD_ROW(true, false, false, lv[i], 0.f, first, gs);
        DPD_CHECK_LAUNCH();
    }
#undef EMD_ROW
#undef EMD_COL
    return 0;
}

}  // namespace dpd

extern "C" size_t dpd_emd_workspace_bytes(int B, int n, int m) {
    if (B <= 0 || n <= 0 || m <= 0 || n > dpd::kEmdMax || m > dpd::kEmdMax) return 0;
    return ((size_t)B * n * 3 + (size_t)B * m * 2) * sizeof(float);
}

extern "C" int dpd_emd_fwd(const float* xyz1, const float* xyz2, int B, int n, int m, float gscale, float* cost, float* loss, float* grad1,
                           float* grad2, float* match, void* ws, size_t ws_bytes, void* stream) {
    using namespace dpd;
    if (const int rc = emd_check(xyz1, xyz2, B, n, m, cost, loss, ws, ws_bytes)) return rc;
    const EmdWs w = emd_carve(ws, B, n, m);
    hipStream_t s = (hipStream_t)stream;
    if (const int rc = emd_passes(xyz1, nullptr, n, xyz2, nullptr, m, B, w, grad1, grad2, match, gscale / ((float)B * (float)n), s)) return rc;
    DPD_LAUNCH(emd_finish_kernel, dim3(1), dim3(256), 0, s, (const float*)w.costk, B, n, cost, loss);
    DPD_CHECK_LAUNCH();
    return 0;
}

extern "C" int dpd_emd_match_cost(const float* xyz1, const float* xyz2, int B, int n, int m, const float* match, float gscale,
                                  float* cost, float* loss, float* grad1, float* grad2, void* ws, size_t ws_bytes, void* stream) {
    using namespace dpd;
    if (!match) return DPD_E_NULL;
    if (const int rc = emd_check(xyz1, xyz2, B, n, m, cost, loss, ws, ws_bytes)) return rc;
    const EmdWs w = emd_carve(ws, B, n, m);
    const int c1 = (n + kWave - 1) / kWave, c2 = grad2 ? (m + kWave - 1) / kWave : 0;
    DPD_LAUNCH(emd_match_cost_kernel, dim3(B, c1 + c2), dim3(kEmdThreads), 0, (hipStream_t)stream, xyz1, xyz2, n, m, match, c1, w.costk,
               grad1, grad2, gscale / ((float)B * (float)n));
    DPD_CHECK_LAUNCH();
    DPD_LAUNCH(emd_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)w.costk, B, n, cost, loss);
    DPD_CHECK_LAUNCH();
    return 0;
}

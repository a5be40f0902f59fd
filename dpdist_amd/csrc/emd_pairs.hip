// Earth Mover's distance of the pairs (A_b, B_b) of two ragged sets: cost[b], dist[b] = cost[b] / n_b and the gradients under an upstream
// W [P] of dist (include/dpdist_capi.h: dpd_emd_pairs_fwd / _bwd; driven by dpdist_amd/emd.py: emd_pairs, EMDPairs).  A pair's values are
// dpd_emd_fwd's on that pair alone and dpd_emd_matrix_fwd / _bwd's on the 1 x 1 matrix of that pair, bit for bit: every form runs the
// pass bodies of emd_int.h.
//
// Two forms, the same bits:
//   1  one launch     emd_matrix_kernel (emd_matrix.hip) over the pair map p -> (p, p): one workgroup owns a pair, a pass is a loop between
//                     two barriers, the vectors live in LDS.  P workgroups; for the widths where 22 dependent launches bind.
//   2  per pass       the pass kernels and the launch schedule of dpd_emd_fwd themselves (emd.hip: emd_passes), given the counts: a pass
//                     is a launch, a workgroup takes one owner tile (64 points) of one pair, the vectors live in the workspace (the
//                     carve of emd_int.h, shared with the dense entry) with the padded width as their row stride.  P * ceil(W / 64)
//                     workgroups per launch: 16 pairs of 2048 points are 512 workgroups where form 1 has 16.  A tile wholly beyond its
//                     pair's count leaves before the first barrier.
// form 0 takes form 2 from the padded width DPD_EMD_PAIRS_PER_PASS_FROM on (the larger of Wa, Wb; the host never reads a count).
//
// Backward: the match is a constant and is recomputed.  Either form accumulates the contract's d cost / d xyz1 and d cost / d xyz2 of each
// pair level by level straight into the real rows of dA / dB (a row is read and written by its owner lane alone), unscaled; one fold
// launch per set then writes every row in place: dA[b,k] = +0.0 + (W[b] / n_b) g1(b)[k] for a real row -- the 1 x 1 fold of
// emd_matrix_fold_a_kernel / _b_kernel -- and +0.0 for a row at or beyond the count.  The fold is a launch of its own, not the scale of
// the last pass, because the contract's "+0.0 +" turns a -0.0 product into +0.0 and because the padded rows need a writer anyway.
// No atomics, one writer per element per launch, the padding is never read.
#include "emd_int.h"

#ifndef DPD_EMD_PAIRS_PER_PASS_FROM
#define DPD_EMD_PAIRS_PER_PASS_FROM 256   // form 2 from this padded width on (the larger of Wa, Wb); measured, DESIGN.md 3.13
#endif

namespace dpd {

// cost[b] = sum_k costk[b][k] in emd_finish_kernel's order (thread t sums k = t, t + 256, ..., then block_sum_256), dist[b] = cost[b] / n_b
__global__ __launch_bounds__(256) void emd_pairs_finish_kernel(const float* __restrict__ costk, const int32_t* __restrict__ countsA, int Wa,
                                                               long long P, float* __restrict__ cost, float* __restrict__ dist) {
    __shared__ float red[4];
    for (long long b = blockIdx.x; b < P; b += gridDim.x) {
        const int n = ragged_count(countsA, (int)b, Wa);
        float s = 0.f;
        for (int k = threadIdx.x; k < n; k += 256) s += costk[(size_t)b * Wa + k];
        s = block_sum_256(s, red);
        if (threadIdx.x == 0) {
            if (cost) cost[b] = s;
            if (dist) dist[b] = s / (float)n;
        }
    }
}

// g [P,Wx,3] in place: a real row becomes +0.0 + (W[b] / n_b) g, n_b the count of A_b; a row at or beyond the count of X_b becomes +0.0.
// One thread per element.
__global__ __launch_bounds__(256) void emd_pairs_fold_kernel(float* __restrict__ g, const int32_t* __restrict__ countsX, int Wx,
                                                             const int32_t* __restrict__ countsA, int Wa, long long P,
                                                             const float* __restrict__ W) {
    const long long row = (long long)Wx * 3, total = P * row;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const long long b = e / row;
        const int r = (int)(e % row);
        float acc = 0.f;
        if (r / 3 < ragged_count(countsX, (int)b, Wx)) acc += (W[b] / (float)ragged_count(countsA, (int)b, Wa)) * g[e];
        g[e] = acc;
    }
}

static int ep_check(const void* A, const void* B, int Wa, int Wb, int P, int form) {
    if (!A || !B) return DPD_E_NULL;
    if (P < 1 || form < 0 || form > 2) return DPD_E_DIM;
    if (Wa < 1 || Wb < 1 || Wa > kEmdMax || Wb > kEmdMax) return DPD_E_UNSUPPORTED;
    return 0;
}

static int ep_form(int form, int Wa, int Wb) { return form ? form : ((Wa > Wb ? Wa : Wb) >= DPD_EMD_PAIRS_PER_PASS_FROM ? 2 : 1); }

}  // namespace dpd

extern "C" size_t dpd_emd_pairs_workspace_bytes(int P, int Wa, int Wb) { return dpd_emd_workspace_bytes(P, Wa, Wb); }

extern "C" int dpd_emd_pairs_fwd(const float* A, const int32_t* countsA, int Wa, const float* B, const int32_t* countsB, int Wb, int P, int form,
                                 float* cost, float* dist, void* ws, size_t ws_bytes, void* stream) {
    using namespace dpd;
    if (!cost && !dist) return DPD_E_NULL;
    if (const int rc = ep_check(A, B, Wa, Wb, P, form)) return rc;
    if (!ws || ws_bytes < dpd_emd_pairs_workspace_bytes(P, Wa, Wb)) return DPD_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    if (ep_form(form, Wa, Wb) == 1) return em_diag_fwd(A, countsA, Wa, B, countsB, Wb, P, cost, dist, s);
    const EmdWs w = emd_carve(ws, P, Wa, Wb);
    if (const int rc = emd_passes(A, countsA, Wa, B, countsB, Wb, P, w, nullptr, nullptr, nullptr, 1.f, s)) return rc;
    DPD_LAUNCH(emd_pairs_finish_kernel, dim3(P < kEmdMaxGrid ? P : kEmdMaxGrid), dim3(256), 0, s, (const float*)w.costk, countsA, Wa, (long long)P,
               cost, dist);
    DPD_CHECK_LAUNCH();
    return 0;
}

extern "C" int dpd_emd_pairs_bwd(const float* A, const int32_t* countsA, int Wa, const float* B, const int32_t* countsB, int Wb, int P, int form,
                                 const float* W, float* dA, float* dB, void* ws, size_t ws_bytes, void* stream) {
    using namespace dpd;
    if (!W || (!dA && !dB)) return DPD_E_NULL;
    if (const int rc = ep_check(A, B, Wa, Wb, P, form)) return rc;
    if (!ws || ws_bytes < dpd_emd_pairs_workspace_bytes(P, Wa, Wb)) return DPD_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    if (ep_form(form, Wa, Wb) == 1) {
        if (const int rc = em_diag_grads(A, countsA, Wa, B, countsB, Wb, P, dA, dB, s)) return rc;
    } else {
        if (const int rc = emd_passes(A, countsA, Wa, B, countsB, Wb, P, emd_carve(ws, P, Wa, Wb), dA, dB, nullptr, 1.f, s)) return rc;
    }
    for (int side = 0; side < 2; ++side) {
        float* g = side ? dB : dA;
        if (!g) continue;
        const int Wx = side ? Wb : Wa;
        const long long blocks = ((long long)P * Wx * 3 + 255) / 256;
        DPD_LAUNCH(emd_pairs_fold_kernel, dim3(blocks < kEmdMaxGrid ? (int)blocks : kEmdMaxGrid), dim3(256), 0, s, g, side ? countsB : countsA, Wx,
                   countsA, Wa, (long long)P, W);
        DPD_CHECK_LAUNCH();
    }
    return 0;
}

// Register-streamed fp32 MFMA GEMM (gfx950 / CDNA4): no LDS, no barriers.
//
// Why: v_mfma_f32_32x32x2_f32 runs at 1/16 of the bf16 rate (64 cycles per instruction per SIMD), so one wave needs only
// ONE VGPR per operand per 64 cycles -- 16x less operand bandwidth per flop than a bf16 GEMM.  At that rate the L1/L2 path
// can feed the MFMA operands straight into registers; what limited the LDS-ring kernel of gemm_f32.hip (73 % of the MFMA peak)
// was not data but synchronisation: a workgroup barrier per K-tile plus the LDS-DMA refill cost it 22 % (ablations in
// DESIGN.md section 3.1).  Here every wave is independent:
//   * a wave owns a (32*TM) x (32*TN) output tile (TM*TN accumulators of 16 VGPRs) and streams its own operands with
//     buffer loads, one K-tile (32 contraction steps) ahead of the MFMAs (double-buffered in VGPRs, counted vmcnt by hipcc);
//   * lane (l31, half) of a 32x32x2 MFMA supplies A[l31][k] / B[k][l31] for k = the lane's half of the k pair.  Inside a
//     32-deep K-tile the contraction index is assigned as  k = 32 t + 16 half + 4 b + s  (block b = 0..3, step s = 0..3):
//       K-contiguous operand  -> the lane reads 64 contiguous bytes of its row as four dwordx4 (b = 0..3): the four loads
//                                of a half-wave hit the same 32 x 128-B lines back to back (L1 hits after the first);
//       MN-contiguous operand -> one dword per (b, s): 32 lanes read 128 contiguous bytes of row k (perfectly coalesced);
//     A and B use the same assignment, which is all the contraction needs;
//   * addresses: one buffer descriptor per operand, a loop-invariant per-lane voffset, the K progress in the SCALAR offset
//     -> no vector address arithmetic in the loop; out-of-range rows/columns are clamped (never stored);
//   * the workgroup (WR x WC waves, one per SIMD for 2x2) only exists to place waves that share operand rows/columns on
//     one CU (L1 reuse) and to make the block -> tile map XCD-aware; waves never wait for each other, so ragged tiles
//     simply retire early.
// (A fused-window-gather form of this kernel -- X never materialised, the A operand gathered from the Fisher vectors per lane -- was
// built in round 2, was bitwise, and measured slower (layer 1: 180 us against 147 + 13.5 us: the per-lane address arithmetic sits in the
// in-order issue stream of an MFMA-bound wave; profiles/r02_variants.txt); removed in round 6.)
// Results are bitwise identical to the LDS kernels (a k-ordered fmaf chain per output element; the permutation inside a
// K-tile changes the ORDER of the chain, so "identical" holds between rs configurations, not against the ring kernels).
#pragma once
#include "gemm_shared.h"

namespace dpd {

typedef unsigned rs_u4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ __amdgpu_buffer_rsrc_t rs_rsrc(const void* p, size_t bytes) {
    // raw (untyped, stride 0) buffer; word3 = 0x00020000 is the gfx9/CDNA data format for dword MUBUF accesses
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, (int)(bytes > 0xffffffffull ? 0xffffffffull : bytes), 0x00020000);
}

// One operand tile (32 rows/cols of the wave tile) of one K-tile: v[b][s] = operand value for block b, step s
struct RsFrag {
    float v[4][4];
};

// the loads of one operand tile that belong to step (b, s) of a K-tile (issued one pipeline depth ahead of their use)
template <bool KC>
__device__ __forceinline__ void rs_load_step(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned k0, unsigned ld, int b, int s, RsFrag& f) {
    if (KC) {   // voff = (row*ld + 16*half)*4 ; soffset = k0*4 ; block b -> +16 B ; one dwordx4 carries the four steps
        if (s == 0) {
            const rs_u4 x = __builtin_amdgcn_raw_buffer_load_b128(r, voff + 16u * b, k0 * 4u, 0);
            f.v[b][0] = __uint_as_float(x.x); f.v[b][1] = __uint_as_float(x.y);
            f.v[b][2] = __uint_as_float(x.z); f.v[b][3] = __uint_as_float(x.w);
        }
    } else {    // voff = (16*half*ld + col)*4 ; soffset = (k0 + 4b + s)*ld*4
        f.v[b][s] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, voff, (k0 + 4u * b + s) * ld * 4u, 0));
    }
}

// out[col] = the sum over `nparts` blocks of in[block][col], in block order, for this lane's column of each of the wave's TN tiles
// (the second step of a bias gradient, GemmArgs::colsum_part, as the CS2 form of the kernel runs it; out / in may be NULL: nothing)
template <int TN>
__device__ __forceinline__ void rs_colsum_finish(float* out, const float* in, int nparts, int N, int n0, int l31) {
    if (!out || !in) return;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int col = n0 + 32 * j + l31;
        if (col < N) {
            float t = 0.f;
            for (int pb0 = 0; pb0 < nparts; pb0 += 16) {     // 16 loads in flight, added in block order
                float v[16];
#pragma unroll
                for (int u = 0; u < 16; ++u) v[u] = (pb0 + u < nparts) ? in[(size_t)(pb0 + u) * N + col] : 0.f;
#pragma unroll
                for (int u = 0; u < 16; ++u) t += v[u];
            }
            out[col] = t;
        }
    }
}

// D = pipeline depth in K-tiles (operand register sets): the loads of K-tile t+D-1 are issued, step by step, between the
// MFMAs of K-tile t, so every operand has D-1 whole tile times ((TM*TN*16) MFMAs x 64 cycles each) to arrive.
// DM: the live row count comes from the device word g.M_dev (GemmArgs::M_dev); g.M is the capacity the grid was launched for.
// DK: the live contraction length comes from the device word g.K_dev (GemmArgs::K_dev); g.K is the capacity the operands hold.  A
//     length of 0 runs no K-tile at all: the accumulators leave as the zeros they were set to, and the epilogues run as always.
// CS2: a launch that is not grouped finishes TWO bias gradients (GemmArgs::colsum_b and colsum_b2) in its first-row-block waves.
template <bool AK, bool BKC, int TM, int TN, int WR, int WC, int D, bool DM = false, bool DK = false, bool CS2 = false>
__global__ __launch_bounds__(64 * WR * WC) void gemm_rs_kernel(GemmArgs g) {
    const int bid = (int)blockIdx.x;
#include "gemm_rs_body.h"
}

// Two independent problems in ONE launch (the live-row backward: a dH product beside a dW product that does not need its result).
//   workgroups [0, nblk_a)  problem a: NN form, live row count from a.M_dev (the dH product; nblk_a = its tiles at the capacity a.M)
//   workgroups [nblk_a, ..) problem b: TN form, live contraction length from b.K_dev (a dW product: a fixed tile count)
// The branch is uniform over the workgroup; each part runs the wave body (gemm_rs_body.h) exactly as its own launch would, with its own id range, so the
// XCD map of a part runs over that part's live tiles and a workgroup beyond them leaves at once.  Problem a comes first: its
// K-deep chains are the long ones (the dispatcher hands out workgroups in id order).  No workgroup waits for another: there is no
// flag, counter or atomic between them, only two kernels' worth of independent waves sharing the SIMDs.
template <int TNA, int TNB>
__global__ __launch_bounds__(256) void gemm_rs_pair_kernel(GemmArgs ga, GemmArgs gb, int nblk_a) {
    constexpr int TM = 1, WR = 2, WC = 2, D = 2;
    constexpr bool BKC = false, CS2 = false;
    if ((int)blockIdx.x < nblk_a) {
        constexpr bool AK = true, DM = true, DK = false;
        constexpr int TN = TNA;
        GemmArgs g = ga;
        const int bid = (int)blockIdx.x;
#include "gemm_rs_body.h"
    } else {
        constexpr bool AK = false, DM = false, DK = true;
        constexpr int TN = TNB;
        GemmArgs g = gb;
        const int bid = (int)blockIdx.x - nblk_a;
#include "gemm_rs_body.h"
    }
}

// tileA / tileB: 32 or 33 (checked by the caller); a.M_dev and b.K_dev set, no split of any kind, b not grouped
static int launch_rs_pair(int tileA, int tileB, const GemmArgs& a, const GemmArgs& b, hipStream_t s) {
    const int bna = tileA == 32 ? 128 : 64, bnb = tileB == 32 ? 128 : 64;
    const int nblk_a = ((a.M + 63) / 64) * ((a.N + bna - 1) / bna);
    const int nblk_b = ((b.M + 63) / 64) * ((b.N + bnb - 1) / bnb);
    const dim3 grid(nblk_a + nblk_b), blk(256);
    if (tileA == 33 && tileB == 33) DPD_LAUNCH((gemm_rs_pair_kernel<1, 1>), grid, blk, 0, s, a, b, nblk_a);
    else if (tileA == 33) DPD_LAUNCH((gemm_rs_pair_kernel<1, 2>), grid, blk, 0, s, a, b, nblk_a);
    else if (tileB == 33) DPD_LAUNCH((gemm_rs_pair_kernel<2, 1>), grid, blk, 0, s, a, b, nblk_a);
    else DPD_LAUNCH((gemm_rs_pair_kernel<2, 2>), grid, blk, 0, s, a, b, nblk_a);
    return (int)hipGetLastError();
}

// C[r][:] += sum_z slab_z[r][:] for the rows of the tail tiles (fixed order; float4, N % 4 == 0)
__global__ __launch_bounds__(256) void tail_reduce_kernel(float* __restrict__ C, int ldc, const float* __restrict__ slab, int nslab,
                                                           long slab_stride, int row0, int M, int N) {
    const long total4 = (long)(M - row0) * N / 4;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total4; i += (long)gridDim.x * blockDim.x) {
        const long e = i * 4;
        const int row = row0 + (int)(e / N), col = (int)(e % N);
        float4 a = *reinterpret_cast<const float4*>(C + (size_t)row * ldc + col);
        for (int z = 0; z < nslab; ++z) {
            const float4 x = *reinterpret_cast<const float4*>(slab + (size_t)z * slab_stride + (size_t)row * N + col);
            a.x += x.x; a.y += x.y; a.z += x.z; a.w += x.w;
        }
        *reinterpret_cast<float4*>(C + (size_t)row * ldc + col) = a;
    }
}

template <bool AK, bool BKC, int TM, int TN, int WR, int WC, int D, bool DM = false, bool DK = false, bool CS2 = false>
static int launch_rs(const GemmArgs& g_in, hipStream_t s) {
    constexpr int BM = 32 * TM * WR, BN = 32 * TN * WC;
    GemmArgs g = g_in;
    const int tilesM = (g.M + BM - 1) / BM, tilesN = (g.N + BN - 1) / BN, T = tilesM * tilesN;
    int nblk = T * g.split_k * (g.A2 ? 2 : 1);
    int row0 = 0;
    if (g.tail_split == -1) {
        // Tail split requested (tail_slab given): T workgroup tiles on 256 CUs run in ceil(T / 256) rounds; when the last round
        // is less than 3/4 full its tiles are cut into K pieces so that it takes 1/pieces of a round (dW1: 640 tiles = 2.5 rounds
        // -> 512 whole tiles + 128 tiles x 2 halves: 3 rounds become 2.5).  Whole tile ROWS only, >= 8 K-tiles per piece.
        g.tail_split = 0;
        const int r = T % 256, nfull = T - r;
        if (T > 256 && r > 0 && r < 192 && g.split_k == 1 && !g.A2 && g.epi == EPI_NONE && !g.colsum && !g.colsum_part && g.tail_slab) {
            int pieces = (256 + r / 2) / r;
            pieces = pieces > 4 ? 4 : pieces;
            const int first = (nfull / tilesN) * tilesN;
            const int chunk = ((g.K / 32 + pieces - 1) / pieces) * 32;
            if (pieces >= 2 && first > 0 && chunk >= 256 && chunk * (pieces - 1) < g.K) {
                g.tail_first = first; g.tail_split = pieces; g.tail_chunk = chunk;
                nblk = first + (T - first) * pieces;
                row0 = (first / tilesN) * BM;
            }
        }
    }
    DPD_LAUNCH((gemm_rs_kernel<AK, BKC, TM, TN, WR, WC, D, DM, DK, CS2>), dim3(nblk), dim3(64 * WR * WC), 0, s, g);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return (int)e;
    if (g.tail_split > 1) {
        const long total4 = (long)(g.M - row0) * g.N / 4;
        const int blocks = (int)((total4 + 255) / 256 < 1024 ? (total4 + 255) / 256 : 1024);
        DPD_LAUNCH(tail_reduce_kernel, dim3(blocks), dim3(256), 0, s, g.C, g.ldc, (const float*)g.tail_slab, g.tail_split - 1,
                   (long)g.M * g.N, row0, g.M, g.N);
        return (int)hipGetLastError();
    }
    return 0;
}

// tile codes 30..33: register-streamed kernels (wave tile, waves per workgroup, pipeline depth)
template <bool AK, bool BKC>
static int launch_rs_tile(int tile, const GemmArgs& g, hipStream_t s) {
    if (g.M_dev) {      // live row count on the device: the TN and NN forms of the two 32-row wave tiles (a k-ordered chain per element: same bits)
        if constexpr (!BKC) {
            if (g.split_k != 1 || g.tail_split || g.A2 || g.K_dev) return DPD_E_UNSUPPORTED;
            if (tile == 32) return launch_rs<AK, BKC, 1, 2, 2, 2, 2, true>(g, s);
            if (tile == 33) return launch_rs<AK, BKC, 1, 1, 2, 2, 2, true>(g, s);
        }
        return DPD_E_UNSUPPORTED;
    }
    if (g.K_dev) {      // live contraction length on the device: the TN form (single or grouped) of the same two tiles
        if constexpr (!AK && !BKC) {
            if (g.split_k != 1 || g.tail_split || g.K < 32) return DPD_E_UNSUPPORTED;
            if (g.colsum_b2 && !g.A2) {      // two bias gradients finished by one problem's waves
                if (tile == 32) return launch_rs<AK, BKC, 1, 2, 2, 2, 2, false, true, true>(g, s);
                if (tile == 33) return launch_rs<AK, BKC, 1, 1, 2, 2, 2, false, true, true>(g, s);
            }
            if (tile == 32) return launch_rs<AK, BKC, 1, 2, 2, 2, 2, false, true>(g, s);
            if (tile == 33) return launch_rs<AK, BKC, 1, 1, 2, 2, 2, false, true>(g, s);
        }
        return DPD_E_UNSUPPORTED;
    }
    switch (tile) {
        case 30: return launch_rs<AK, BKC, 2, 2, 2, 2, 2>(g, s);   // 128x128 workgroup, 4 waves of 64x64, 2 operand sets
        case 31: return launch_rs<AK, BKC, 2, 1, 2, 2, 2>(g, s);   // 128x64,  4 waves of 64x32
        case 32: return launch_rs<AK, BKC, 1, 2, 2, 2, 2>(g, s);   //  64x128, 4 waves of 32x64
        case 33: return launch_rs<AK, BKC, 1, 1, 2, 2, 2>(g, s);   //  64x64,  4 waves of 32x32
        default: return DPD_E_UNSUPPORTED;
    }
}

}  // namespace dpd

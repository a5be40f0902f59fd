// Host interface of the GEMMs (gemm_f32.hip, gemm_x3.hip): what the decoder and the C-ABI wrappers call across translation units.
// A call is ONE plain struct: set the fields the call uses; every default is the "not used" value.
#pragma once
#include "gemm_shared.h"

namespace dpd {

// fp32 tile codes (gemm_f32): the kernel families by name
constexpr int kF32TileStaged = 3;                                        // register-staged 64x64: takes every shape (any K % 4 == 0)
constexpr bool f32_tile_dma(int tile) { return tile == 8 || tile == 9; }     // LDS-DMA ring kernels: whole 32-deep K-tiles
constexpr bool f32_tile_rs(int tile) { return tile >= 30 && tile <= 33; }    // register-streamed kernels (gemm_rs.h): whole 32-deep K-tiles

// C[M,N] = epi( op(A) op(B) ), exact fp32 (gemm_f32.hip)
struct GemmF32Call {
    int transA = 0, transB = 0;
    int M = 0, N = 0, K = 0;
    const float* A = nullptr;
    int lda = 0;
    const float* B = nullptr;
    int ldb = 0;
    float* C = nullptr;
    int ldc = 0;
    const float* bias = nullptr;
    const float* gate = nullptr;
    int epilogue = EPI_NONE;
    int split_k = 1;                      // 0 = tail split (gemm_rs.h)
    int tile = 0;                         // 0 = the register-staged kernel
    void* ws = nullptr;                   // split-K slabs
    size_t ws_bytes = 0;
    hipStream_t s = nullptr;
    float* colsum = nullptr;              // GemmArgs::colsum
    const float* A2 = nullptr;            // second problem of identical shape (grouped launch)
    const float* B2 = nullptr;
    float* C2 = nullptr;
    const ColsumTwoStep* cs2 = nullptr;   // two-step bias gradient (register-streamed kernels)
    const int* M_dev = nullptr;           // GemmArgs::M_dev (TN or NN, tiles 32 / 33, no split): M is then the capacity
    const int* K_dev = nullptr;           // GemmArgs::K_dev (TN, tiles 32 / 33, no split, single or grouped): K is then the capacity
    // A second, independent problem in the SAME launch (gemm_rs_pair_kernel): this call is then the NN product with M_dev and the gate
    // epilogue (a live-row dH), *pair a TN product with K_dev, no epilogue, at most the second step of a bias gradient (a live-row dW):
    // tiles 32 / 33 each, split_k == 1, not grouped, K >= 32 for the TN part, the same stream; anything else: DPD_E_UNSUPPORTED
    const GemmF32Call* pair = nullptr;
};
int gemm_f32(const GemmF32Call& c);

// out[m,n] = epi( sum_z slabs[z][m,n] ), fixed order (gemm_f32.hip); slabs are dense [M,N], N % 4 == 0
int splitk_reduce(const float* slabs, int split_k, long slab_stride, int M, int N, float* C, int ldc, const float* bias,
                  const float* gate, int epi, hipStream_t s);

// optional bf16-plane outputs of a gemm_x3 result (gemm_x3.hip): RC planes [np][M][ld_rc], R8 planes
// [np][r8_rows/8][N][8] for the rows < r8_rows.  rc = r8 = NULL: none
struct X3Out {
    uint16_t* rc = nullptr;
    uint16_t* r8 = nullptr;
    long rc_plane = 0, r8_plane = 0;
    int ld_rc = 0, r8_rows = 0, np = 0;
};

// further problems of a grouped plain plane-GEMM launch (gemm_x3.hip): same N, K, B layout and tile; own operands, output and rows.
// A2 = NULL: none.  M2 / M3 = 0: the rows of problem 0.  Problems with other rows than problem 0, and a third problem, run on the
// ring kernels only.
struct X3Extra {
    const uint16_t* A2 = nullptr;
    const uint16_t* B2 = nullptr;
    float* C2 = nullptr;
    int M2 = 0;
    const uint16_t* A3 = nullptr;
    const uint16_t* B3 = nullptr;
    float* C3 = nullptr;
    int M3 = 0;
};

// C[M,N] (fp32) = epi( op(A) op(B) ) from bf16 planes (gemm_x3.hip).  a_fmt / b_fmt: 0 = RC (k contiguous), 1 = R8 (k = row index),
// 2 = RC plane of an operand whose k is its ROW index (both operands: A stored [K][M], B stored [K][N]; lda / ldb = row strides).
struct X3Call {
    int np = 0, a_fmt = 0, b_fmt = 0;
    int M = 0, N = 0, K = 0;
    const uint16_t* A = nullptr;
    int lda = 0;
    long a_plane = 0;
    const uint16_t* B = nullptr;
    int ldb = 0;
    long b_plane = 0;
    float* C = nullptr;
    int ldc = 0;
    const float* bias = nullptr;
    const float* gate = nullptr;
    int epilogue = EPI_NONE;
    int tile = 0;
    hipStream_t s = nullptr;
    float* colsum = nullptr;
    X3Out out;
    X3Extra ex;
    int split_k = 1;
    void* ws = nullptr;                   // split-K slabs: dense (slabs + reduce launch) or, with red_cnt, tile-padded (in-launch reduction)
    size_t ws_bytes = 0;
    const uint16_t* gate16 = nullptr;     // GemmArgs::gate16
    int gate16_r8 = 0;
    void* red_cnt = nullptr;              // arrival words of the in-launch reduction, 8 bytes each
    int red_cnt_words = 0;
};
int gemm_x3(const X3Call& c);

int split_planes(const float* src, int R, int C, int ld, int np, uint16_t* rc, int ld_rc, long rc_plane, uint16_t* r8,
                 long r8_plane, hipStream_t s);
int split_planes_multi(SplitJobs jobs, hipStream_t s);

// in-stream GEMM profiler (gemm_f32.hip): event pair around one GEMM (kernel + split-K reduce)
bool prof_begin(hipStream_t s);
// form: 0 = the contraction runs along A's rows (NN / NT: the forward and data-gradient products), 1 = TN (weight gradients)
void prof_end(bool on, hipStream_t s, double flops, int form = 0);
struct ProfScope {
    bool on; hipStream_t s; double fl; int form;
    ~ProfScope() { prof_end(on, s, fl, form); }
};

}  // namespace dpd

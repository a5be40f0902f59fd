// What the decoder's translation units share: decoder.hip (GEMM plan and dispatch, workspace, weight copies, forward), decoder_out.hip
// (output layer), decoder_bwd.hip (dense backward), decoder_live.hip (live-row backward).  Host declarations only: every kernel lives in
// exactly one unit, every function declared here has its one definition in the unit named beside it.
#pragma once
#include "gemm_host.h"

namespace dpd {

// process-wide GEMM plan (tile, split_k) per call site; 0 = automatic.  The only global state of the library:
// a tuning knob (dpd_set_gemm_plan), never needed for correctness.  Defined in decoder.hip.
enum { OP_FWD_L1 = 0, OP_FWD_L23 = 1, OP_BWD_DH = 2, OP_BWD_DX = 3, OP_BWD_DW1 = 4, OP_BWD_DW23 = 5, OP_BWD_DH_T = 6, OP_BWD_DX_T = 7,
       OP_COUNT = 8 };   // _T: the same product with a transposed weight copy (NN form)
enum { LIVE_DH = 0, LIVE_DW1 = 1, LIVE_DW23 = 2, LIVE_PAIR_DW = 3 };
extern int g_plan_tile[OP_COUNT], g_plan_split[OP_COUNT], g_x3_tile[OP_COUNT], g_x3_split[OP_COUNT];
extern int g_x3_pair_tile, g_x3_pair_split, g_x3_trio_tile, g_x3_trio_split, g_l1u_tile, g_live_tile[4];

constexpr size_t kRedCntBytes = 8192;                 // arrival words of the in-launch reduction: the last 8 KiB of the base workspace
constexpr int kColChunks = 16;                        // row chunks of the two-stage column sums (colsum_stage1 / colsum_stage2)

// Compute type of the three wide layers (the `dtype` argument of the decoder entry points):
//   0  exact fp32 on the fp32 MFMA (gemm_f32.hip)
//   1  fp32-equivalent on the bf16 MFMA: operands split into 3 bf16 planes, 6 MFMA terms (gemm_x3.hip)
//   2  bf16 operands, fp32 accumulation and fp32 outputs (mixed-precision training, BASELINE config 3)
// For 1 and 2 each GEMM first writes the planes of its two operands into `scr` (unfused producers).
struct Scratch {
    char* p;
    size_t bytes;
};

// ---- decoder.hip ----
// Split-K plan of the plane weight gradients (TN, plain products; 1-3 grouped problems of rows[0 .. nprob) x N, contraction K = query
// rows): the ONE place that turns a requested split (g_x3_split: 0 automatic, n > 1 in-launch, n < -1 slabs + reduce launch, 1 off)
// into what gemm_x3 gets.  `base` / `base_bytes` = the base workspace (base_ws_bytes), NULL / 0 when the caller's workspace does not
// hold it: its last kRedCntBytes are the arrival words of the in-launch reduction, everything before them the slabs.
struct X3SplitPlan {
    int split = 1;
    void* slab = nullptr;
    size_t slab_bytes = 0;
    void* cnt = nullptr;     // arrival words: the in-launch form
};
X3SplitPlan x3_plan_split(int np, int tile, int request, const int* rows, int nprob, int N, int K, void* base, size_t base_bytes);
void set_split(X3Call& c, const X3SplitPlan& p);

// One dense product of the decoder in the compute type `dtype`, with the tile / split of call site `op`
struct GemmDtCall {
    int dtype = 0, op = 0;
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
    void* ws = nullptr;           // fp32: split-K slabs; plane types: the base workspace (x3_plan_split)
    size_t ws_bytes = 0;
    Scratch scr{nullptr, 0};
    hipStream_t s = nullptr;
    float* colsum = nullptr;
    const void* Apl = nullptr;    // operand planes that already exist (else the fp32 operand is split into `scr`)
    const void* Bpl = nullptr;
    X3Out out;                    // plane outputs
    const ColsumTwoStep* cs2 = nullptr;
    const void* gate16 = nullptr;
    int gate16_r8 = 0;
};
int gemm_dt(const GemmDtCall& c);

// `pl` is honoured only for these shapes (everything the fused producers and the plane GEMMs assume)
const dpd_planes* usable_planes(const dpd_planes* pl, int dtype, int Q, int Qb, int KP, int H);
int check_planes(const dpd_planes* pl, int dtype);
X3Out make_out(const dpd_planes* pl, void* rc, int rc_rows, void* r8, int r8_rows, int cols);

size_t colsum_ws_floats(int ncols, int nw);
size_t base_ws_bytes(int KP, int H);
size_t base_ws_or_0(const void* ws, size_t ws_bytes, int KP, int H);      // the base workspace when `ws` holds it, else 0
Scratch scratch_of(void* ws, size_t ws_bytes, int KP, int H);             // plane scratch = the tail of the workspace

// ---- the parts of dpd_decoder_bwd_data_live (decoder_bwd.hip): its arguments after validation ----
struct BwdData {
    const float* dpred; const float* mask; const float* y; const float* h1; const float* h2; const float* h3;
    int Qb, KP, H, dtype, phases;
    const dpd_decoder_params* p;
    float* dy; float* g3; float* g2; float* g1; float* dX;
    const dpd_small_grads* sg;
    const dpd_planes* pl;      // the usable planes, or NULL
    bool h3_plane;             // layer 3's activation is the bf16 plane h3_rc of the planes the caller passed
    Scratch scr;
    const dpd_live_rows* live;
    hipStream_t s;
};
// decoder_out.hip: phases 1, 8 and 16 (output-layer backward and the small gradients); *g3_planes: g3 was written as operand planes
int out_layer_bwd(const BwdData& b, bool* g3_planes);
// decoder_out.hip: the out_fwd_kernel launch of the forward entries, y = h3 W4 + b4 and pred [Q,3]
int out_layer_fwd(const float* h3, const dpd_decoder_params* p, const float* mask, float* y, float* pred, int Q, int H, hipStream_t s);

// ---- decoder_live.hip: what the _live entries of decoder_bwd.hip do with a descriptor ----
int check_live(const dpd_live_rows* lv, int Qb, int KP, int H);      // what every entry checks of a descriptor before a kernel sees it
int live_data_chain(const BwdData& b);
int live_bwd_weights(int layer, const float* g, int Qb, int Kin, int Nout, int dtype, float* dW, float* db, const float* db_partials,
                     const dpd_live_rows* live, hipStream_t s);
int live_bwd_weights_pair(const float* gA, float* dWA, float* dWB, int Qb, int Kin, int Nout, int dtype, float* dbA, const float* db_partials,
                          const dpd_live_rows* live, hipStream_t s);

}  // namespace dpd

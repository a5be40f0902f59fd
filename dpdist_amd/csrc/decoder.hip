// Implicit-surface decoder: shared MLP  KP(=2503 padded) -> H -> H -> H -> 3, relu6/3, mask.  Forward and backward.
//
// Replaces utils/dpdist_util.py:513-544 (four tf_util.conv2d "1xW VALID conv" == dense layers,
// utils/tf_util.py:161-228), :691 (relu6/3), :695-698 (split + mask) and TF's autodiff of them.
//
// The three wide layers run on the fp32 MFMA GEMM of gemm_f32.hip (bias+ReLU / ReLU-gate fused in the epilogue);
// the 3-wide output layer and the bias gradients are small HBM-bound kernels in this file.
// Algorithmic work per query row (H = 1024): 4 663 296 MAC forward.  Activations h1,h2,h3 [Q,H] stay in HBM
// (16.8 MB each at Q = 4096, resident in the 256 MiB Infinity Cache) for the backward pass.
#include <initializer_list>

#include "gemm_x3.h"

namespace dpd {

// process-wide GEMM plan (tile, split_k) per call site; 0 = automatic.  The only global state of the library:
// a tuning knob (dpd_set_gemm_plan), never needed for correctness.
enum { OP_FWD_L1 = 0, OP_FWD_L23 = 1, OP_BWD_DH = 2, OP_BWD_DX = 3, OP_BWD_DW1 = 4, OP_BWD_DW23 = 5, OP_BWD_DH_T = 6, OP_BWD_DX_T = 7,
       OP_COUNT = 8 };   // _T: the same product with a transposed weight copy (NN form)
// Defaults measured on MI355X at B=32 (tools/gemm_bench.py, profiles/): LDS-DMA ring kernels everywhere;
//   fwd L1 (4096x1024x2528)  128x128 16-wave 3-stage ring  ~127 TFLOP/s    fwd L2/3 (K=1024) 128x128 3-stage  ~120
//   bwd dH (2048x1024x1024)   64x64  3-stage               ~ 93..106       bwd dX            64x64 3-stage    ~103
//   bwd dW1 (2528x1024x2048)  64x64  3-stage, split-K 2    ~102            bwd dW2/3         64x64 3-stage    ~ 97
// (run-to-run spread between boxes is ~10 %; the ranking inside one run is stable.  DMA kernels need K % 32 == 0;
//  gemm_f32 falls back to the register-staged 64x64 kernel otherwise.)
static int g_plan_tile[OP_COUNT] = {32, 32, 8, 8, 33, 33, 32, 32};
static int g_plan_split[OP_COUNT] = {1, 1, 1, 1, 1, 1, 1, 1};   // (0 = tail split, gemm_rs.h: measured no gain on dW1, 0.525 vs 0.5215 ms of GEMM per step)
static int g_x3_tile[OP_COUNT] = {0, 0, 0, 0, 0, 0, 0, 0};   // one-plane (bf16) tile override per call site, 0 = automatic
// split-K of the plane weight-gradient GEMMs (K = query rows is long, M x N gives 64-160 tiles of 128x128 for 256 CUs):
//   n > 1: n slices per output tile, reduced INSIDE the launch by the last-arriving slice in slice order (gemm_x3.hip: inlaunch_reduce;
//          deterministic); n < -1: the round-2 form, |n| fp32 slabs + a reduce launch (A/B reference); 1: off; 0: automatic
static int g_x3_split[OP_COUNT] = {1, 1, 1, 1, 0, 0, 1, 1};
static int g_x3_pair_tile = 0, g_x3_pair_split = 0;   // plane dW2+dW3 pair: tile (0 = automatic), split-K (as above)
static int g_x3_trio_tile = 0, g_x3_trio_split = 1;   // plane dW1+dW2+dW3 in one launch (dpd_decoder_bwd_weights_trio): tile, split-K
static int g_l1u_tile = 33;   // layer 1 over distinct windows (dpd_decoder_fwd_unique): 32 or 33 (dpd_set_gemm_plan op 8)
// live-row backward (dpd_live_rows): dH over the live rows, dW1, dW2 + dW3 over the live contraction length: 32 or 33 (dpd_set_gemm_plan
// ops 9, 10, 11).  The short dH wants the 32x32 wave tile: a wave's K loop is as long as the dense one's, only the tiles get fewer
// (op 12: the dW part of a pair launch, dpd_decoder_bwd_pair_live; its dH part takes op 9's)
enum { LIVE_DH = 0, LIVE_DW1 = 1, LIVE_DW23 = 2, LIVE_PAIR_DW = 3 };
static int g_live_tile[4] = {33, 33, 33, 33};
constexpr size_t kRedCntBytes = 8192;                 // arrival words of the in-launch reduction: the last 8 KiB of the base workspace

// Compute type of the three wide layers (the `dtype` argument of the decoder entry points):
//   0  exact fp32 on the fp32 MFMA (gemm_f32.hip)
//   1  fp32-equivalent on the bf16 MFMA: operands split into 3 bf16 planes, 6 MFMA terms (gemm_x3.hip)
//   2  bf16 operands, fp32 accumulation and fp32 outputs (mixed-precision training, BASELINE config 3)
// For 1 and 2 each GEMM first writes the planes of its two operands into `scr` (unfused producers).
struct Scratch {
    char* p;
    size_t bytes;
};
static size_t plane_bytes(int dtype, int Q, int KP, int H) {
    if (dtype == 0) return 0;
    const size_t np = dtype == 1 ? 3 : 1;
    const size_t big = (size_t)(KP > H ? KP : H);
    return np * 2 * ((size_t)Q * big + big * H) + 256;
}

// Automatic split-K of a plane weight-gradient GEMM: enough slices that the launch has about two 128x128 workgroups per CU (their
// 64 KiB LDS rings let two co-reside: one wave of tiles alone cannot keep the LDS-DMA ring of a CU full), each with >= 1024 deep K.
static int x3_auto_split(int np, X3Tile t, int M, int N, int K) {
    if (np != 1 || !t.ring) return 1;
    const long tiles = (long)((M + t.bm - 1) / t.bm) * ((N + t.bn - 1) / t.bn);
    int split = (int)(480 / (tiles > 0 ? tiles : 1));
    while (split > 1 && K / split < 1024) --split;
    return split < 1 ? 1 : (split > 4 ? 4 : split);
}

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
static X3SplitPlan x3_plan_split(int np, int tile, int request, const int* rows, int nprob, int N, int K, void* base, size_t base_bytes) {
    X3SplitPlan p;
    if (!base || base_bytes <= kRedCntBytes) return p;
    const size_t slab_bytes = base_bytes - kRedCntBytes;
    const X3Tile t = x3_tile(tile);
    int split = request;
    if (split == 0) {   // automatic: the grouped problems counted as one of the summed rows
        int sum = 0;
        for (int i = 0; i < nprob; ++i) sum += rows[i];
        split = x3_auto_split(np, t, sum, N, K);
    }
    // In-launch split-K parks the raw accumulators of every slice in TILE-PADDED slabs (gemm_x3.hip: tiles * split * bm * bn floats):
    // the largest split <= `split` whose slabs fit (with small H the base workspace holds fewer slabs than the automatic
    // split asked for, and the call failed with DPD_E_WORKSPACE instead of running unsplit)
    if (split > 1 && t.ring) {
        const size_t tiles = x3_tile_count(t, rows, nprob, N);
        while (split > 1 && (tiles * split * t.bm * t.bn * sizeof(float) > slab_bytes || tiles > kRedCntBytes / 8)) --split;
    }
    const bool inlaunch = split > 1 && t.ring;
    if (!inlaunch) split = split < -1 ? -split : 1;   // the other tiles: only the round-2 form
    if (split == 1 || x3_last_slice_empty(K, split)) return p;
    p.split = split; p.slab = base; p.slab_bytes = slab_bytes;
    if (inlaunch) p.cnt = (char*)base + slab_bytes;
    return p;
}
static void set_split(X3Call& c, const X3SplitPlan& p) {
    c.split_k = p.split; c.ws = p.slab; c.ws_bytes = p.slab_bytes; c.red_cnt = p.cnt; c.red_cnt_words = (int)(kRedCntBytes / 8);
}

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
static int gemm_dt(const GemmDtCall& c) {
    const int M = c.M, N = c.N, K = c.K;
    const int ra = c.transA ? K : M, ca = c.transA ? M : K;   // stored shape of A, B
    const int rb = c.transB ? N : K, cb = c.transB ? K : N;
    const bool planes_out = c.out.rc || c.out.r8;
    const bool planes_ok = c.dtype != 0 && !(K % 32) && !(ra & 7) && !(ca & 7) && !(rb & 7) && !(cb & 7) && !(c.transA && c.transB);
    if (!planes_ok) {   // exact fp32 (also for shapes the plane kernels do not take)
        if (c.Apl || c.Bpl || planes_out || (c.gate16 && !c.gate)) return DPD_E_UNSUPPORTED;   // callers only pass planes for shapes planes_shape_ok() accepts
        GemmF32Call f;
        f.transA = c.transA; f.transB = c.transB; f.M = M; f.N = N; f.K = K;
        f.A = c.A; f.lda = c.lda; f.B = c.B; f.ldb = c.ldb; f.C = c.C; f.ldc = c.ldc;
        f.bias = c.bias; f.gate = c.gate; f.epilogue = c.epilogue;
        f.split_k = (c.dtype == 0 && !c.colsum) ? g_plan_split[c.op] : 1;
        f.tile = g_plan_tile[c.op];
        // the 128x128 one-workgroup-per-CU kernels need >= ~200 tiles to fill the chip (B = 32 forward); smaller batches
        // (as-loss mode at the PCRNet batch of 16: M = 2048 -> 128 tiles) run the 64x64 kernel, 3 workgroups per CU
        const long tiles128 = (long)((M + 127) / 128) * ((N + 127) / 128);
        if (f.tile == 9 && tiles128 < 200) f.tile = 8;
        // register-streamed NN products: once there are two 128x128 tiles per CU, 64x64 wave tiles (half the operand loads per
        // flop) keep two waves per SIMD as well -- measured at B = 64: family 0.75 -> 0.85 of peak, step 1.206 -> 1.081 ms
        if (f.tile == 32 && tiles128 >= 512 && !c.transA && !c.transB) f.tile = 30;
        f.ws = c.ws; f.ws_bytes = c.ws_bytes; f.s = c.s; f.colsum = c.colsum; f.cs2 = c.cs2;
        return gemm_f32(f);
    }
    if (c.cs2) return DPD_E_UNSUPPORTED;
    const int np = c.dtype == 1 ? 3 : 1;
    const size_t ae = (size_t)M * K, be = (size_t)K * N;
    const size_t need = (size_t)np * 2 * ((c.Apl ? 0 : ae) + (c.Bpl ? 0 : be));
    if (need && (!c.scr.p || c.scr.bytes < need)) return DPD_E_WORKSPACE;
    const uint16_t* Ap = (const uint16_t*)c.Apl;
    const uint16_t* Bp = (const uint16_t*)c.Bpl;
    uint16_t* cursor = (uint16_t*)c.scr.p;
    if (!Ap) {
        if (!c.A) return DPD_E_NULL;
        if (int rc = split_planes(c.A, ra, ca, c.lda, np, c.transA ? nullptr : cursor, ca, (long)ae, c.transA ? cursor : nullptr, (long)ae, c.s))
            return rc;
        Ap = cursor;
        cursor += (size_t)np * ae;
    }
    if (!Bp) {
        if (!c.B) return DPD_E_NULL;
        if (int rc = split_planes(c.B, rb, cb, c.ldb, np, c.transB ? cursor : nullptr, cb, (long)be, c.transB ? nullptr : cursor, (long)be, c.s))
            return rc;
        Bp = cursor;
    }
    // largest tile that still gives the 256 CUs at least ~200 workgroups
    auto blocks = [&](int bm, int bn) { return (long)((M + bm - 1) / bm) * ((N + bn - 1) / bn); };
    // (measured, tools/x3_bench.py: 160 blocks of 128x128 beat 320 of 64x128 on the 2528x1024 dW1; 64x64 only when even
    //  64x128 leaves most CUs idle)
    int tile = blocks(128, 128) >= 150 ? 2 : (blocks(64, 128) >= 100 ? 3 : 5);
    // one plane (bf16) and enough rows for one 256x128 workgroup per CU (B = 64: 8192 x 1024 -> 256 tiles): the phase-staggered
    // BK = 64 kernel (gemm_p8_kernel, tile 21).  Measured on the forward shapes, profiles/r03_x3_bench_p8.txt: layer 1 53.2 -> 48.8 us,
    // layers 2/3 28.1 -> 27.0 us; the backward shapes (M = 4096: 128 such tiles) stay on the 128x128 ring kernel
    if (np == 1 && !c.transA && blocks(256, 128) >= 224) tile = 21;
    // three planes: the same schedule at BK = 32 on 128x128 tiles (tile 24) wherever the ring kernel ran 128x128 tiles: layer 1 at
    // B = 32 132 -> 118 us, layers 2/3 52.6 -> 50.0 us, dW1 88 -> 79 us (tools/p8_probe.py, NP=3)
    if (np == 3 && tile == 2) tile = 24;
    const int xt = g_x3_tile[c.op];   // tuning override (dpd_set_gemm_plan, ops 16..24)
    if (np == 1 && xt && (xt >= 20 || !(K % 64))) tile = xt;
    if (np == 3 && xt >= 24 && xt <= 26) tile = xt;
    X3Call x;
    x.np = np; x.a_fmt = c.transA; x.b_fmt = !c.transB; x.M = M; x.N = N; x.K = K;
    x.A = Ap; x.lda = ca; x.a_plane = (long)ae; x.B = Bp; x.ldb = cb; x.b_plane = (long)be;
    x.C = c.C; x.ldc = c.ldc; x.bias = c.bias; x.gate = c.gate; x.epilogue = c.epilogue; x.tile = tile; x.s = c.s;
    x.colsum = c.colsum; x.out = c.out; x.gate16 = (const uint16_t*)c.gate16; x.gate16_r8 = c.gate16_r8;
    // plane weight gradients (TN, plain product): split-K when the tiles alone leave CUs idle
    if (c.transA && !c.transB && c.epilogue == EPI_NONE && !c.colsum && !planes_out && c.C)
        set_split(x, x3_plan_split(np, tile, g_x3_split[c.op], &M, 1, N, K, c.ws, c.ws_bytes));
    return gemm_x3(x);
}

// `pl` is honoured only for these shapes (everything the fused producers and the plane GEMMs assume)
static const dpd_planes* usable_planes(const dpd_planes* pl, int dtype, int Q, int Qb, int KP, int H) {
    if (!pl || dtype == 0) return nullptr;
    if ((Q & 7) || (Qb & 31) || (KP & 31) || (H & 63)) return nullptr;
    return pl;
}
static int check_planes(const dpd_planes* pl, int dtype) {
    if (!pl) return 0;
    if (pl->np != (dtype == 1 ? 3 : 1)) return DPD_E_DIM;
    return 0;
}
static X3Out make_out(const dpd_planes* pl, void* rc, int rc_rows, void* r8, int r8_rows, int cols) {
    X3Out o;
    o.rc = (uint16_t*)rc; o.r8 = (uint16_t*)r8; o.np = pl->np; o.ld_rc = cols; o.r8_rows = r8_rows;
    o.rc_plane = (long)rc_rows * cols; o.r8_plane = (long)r8_rows * cols;
    return o;
}

// ---- output layer: y = h3 W4 + b4 ; pred = clip(y,0,6)/3 * mask.  One wave per row. ----------------------
// the three dot products of one row with W4 [H,3] (one wave; every lane returns the full sums): ONE definition, so that every
// kernel that evaluates the output layer produces the same bits
// (H % 256 == 0, H <= 1024, W4 16-byte aligned: 16-byte loads of the row AND of W4 -- the 12 floats W4[k..k+3][0..2] are three float4 --
// and the loaded row / column 0 of W4 stay in registers for a caller that goes on to the backward; same additions in the same order)
constexpr int kOutMaxI = 4;
struct OutRowRegs {
    float4 h[kOutMaxI];
    float w0[kOutMaxI][4];
};
__device__ __forceinline__ bool out_row_fast(const float* W4, int H) { return (H & 255) == 0 && H <= 256 * kOutMaxI && !((uintptr_t)W4 & 15); }

__device__ __forceinline__ void out_row_dot(const float* __restrict__ h, const float* __restrict__ W4, int H, int lane, float (&a)[3],
                                            OutRowRegs* keep = nullptr) {
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    if (out_row_fast(W4, H)) {
#pragma unroll
        for (int i = 0; i < kOutMaxI; ++i) {
            const int k = 4 * lane + 256 * i;
            if (k < H) {
                const float4 x = *reinterpret_cast<const float4*>(h + k);
                const float4* wp = reinterpret_cast<const float4*>(W4 + (size_t)k * 3);
                const float4 wa = wp[0], wb = wp[1], wc = wp[2];
                a0 += x.x * wa.x; a1 += x.x * wa.y; a2 += x.x * wa.z;
                a0 += x.y * wa.w; a1 += x.y * wb.x; a2 += x.y * wb.y;
                a0 += x.z * wb.z; a1 += x.z * wb.w; a2 += x.z * wc.x;
                a0 += x.w * wc.y; a1 += x.w * wc.z; a2 += x.w * wc.w;
                if (keep) { keep->h[i] = x; keep->w0[i][0] = wa.x; keep->w0[i][1] = wa.w; keep->w0[i][2] = wb.z; keep->w0[i][3] = wc.y; }
            }
        }
    } else if ((H & 255) == 0) {          // 16 bytes per lane per load: H / 256 loads in flight instead of H / 64 dependent-address ones
        for (int k = 4 * lane; k < H; k += 256) {
            const float4 x = *reinterpret_cast<const float4*>(h + k);
            const float xs[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                a0 += xs[e] * W4[(k + e) * 3 + 0];
                a1 += xs[e] * W4[(k + e) * 3 + 1];
                a2 += xs[e] * W4[(k + e) * 3 + 2];
            }
        }
    } else {
        for (int k = lane; k < H; k += 64) {
            const float x = h[k];
            a0 += x * W4[k * 3 + 0];
            a1 += x * W4[k * 3 + 1];
            a2 += x * W4[k * 3 + 2];
        }
    }
    a[0] = wave_sum(a0); a[1] = wave_sum(a1); a[2] = wave_sum(a2);
}

__global__ __launch_bounds__(256) void out_fwd_kernel(const float* __restrict__ h3, const float* __restrict__ W4,
                                                       const float* __restrict__ b4, const float* __restrict__ mask,
                                                       float* __restrict__ y, float* __restrict__ pred, int Q, int H) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= Q) return;
    float a[3];
    out_row_dot(h3 + (size_t)row * H, W4, H, lane, a);
    if (lane < 3) {
        const float v = (lane == 0 ? a[0] : (lane == 1 ? a[1] : a[2])) + b4[lane];
        y[(size_t)row * 3 + lane] = v;
        pred[(size_t)row * 3 + lane] = fminf(fmaxf(v, 0.f), 6.f) / 3.0f * mask[row];   // relu6(y)/3 (:691) * mask (:697)
    }
}

// DPDist as a frozen loss (pcrnet-registration/iterative_PCRNet_ours.py:229-257): output layer, loss_pred and -- when g3 != NULL -- the
// output-layer backward of d loss_pred / d pred (= gv = 0.5 / BN on channel 0 of every row, models/dpdist_and_aue.py:976-977) in ONE
// launch instead of three (out_fwd + l1_loss + out_bwd: ~5 us each at the PCRNet batch, all launch-latency bound).  One wave per row.
// Same values as the three-kernel chain (loss_pred within an ulp: exact fixed-point sum instead of fp32 partial sums): y / pred through
// out_row_dot, dy = (gv * mask / 3 * [0 < y0 < 6], 0, 0), g3 = dy0 * W4[:,0] * [h3 > 0] (the chain adds two exact zeros to that).
template <int RW>      // rows per wave
__global__ __launch_bounds__(256) void out_asloss_kernel(const float* __restrict__ h3, const float* __restrict__ W4,
                                                          const float* __restrict__ b4, const float* __restrict__ mask,
                                                          float* __restrict__ y, float* __restrict__ pred, float* __restrict__ dy,
                                                          float* __restrict__ g3, int Q, int H, int BN, float gv,
                                                          float* __restrict__ loss, unsigned long long* __restrict__ acc,
                                                          uint16_t* __restrict__ g3_rc, long g3_plane, int g3_np) {
    // g3_rc (round 5, the as-loss engine of the plane compute types): g3 leaves this kernel as the RC operand plane(s) of the first dH GEMM
    // -- the same split as split_planes_kernel, which this saves (one launch and the fp32 round trip of g3; g3 itself may then be NULL)
    __shared__ float s_p[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float p0 = 0.f;
#pragma unroll 1
    for (int rw = 0; rw < RW; ++rw) {
        const int row = (blockIdx.x * 4 + wave) * RW + rw;
        if (row >= Q) break;
        const float* h = h3 + (size_t)row * H;
        float a[3];
        OutRowRegs rr;
        out_row_dot(h, W4, H, lane, a, &rr);
        const float mk = mask[row];
        float yv[3], pv[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            yv[c] = a[c] + b4[c];
            pv[c] = fminf(fmaxf(yv[c], 0.f), 6.f) / 3.0f * mk;
        }
        if (lane < 3) {
            y[(size_t)row * 3 + lane] = lane == 0 ? yv[0] : (lane == 1 ? yv[1] : yv[2]);
            pred[(size_t)row * 3 + lane] = lane == 0 ? pv[0] : (lane == 1 ? pv[1] : pv[2]);
        }
        p0 += pv[0];
        if (dy) {
            const float d0 = (yv[0] > 0.f && yv[0] < 6.f) ? gv * mk / 3.0f : 0.f;
            if (lane < 3) dy[(size_t)row * 3 + lane] = lane == 0 ? d0 : 0.f;
            float* g = g3 ? g3 + (size_t)row * H : nullptr;
            if (out_row_fast(W4, H)) {
#pragma unroll
                for (int i = 0; i < kOutMaxI; ++i) {
                    const int k = 4 * lane + 256 * i;
                    if (k < H) {
                        const float4 x = rr.h[i];
                        float4 o;
                        o.x = x.x > 0.f ? d0 * rr.w0[i][0] : 0.f;
                        o.y = x.y > 0.f ? d0 * rr.w0[i][1] : 0.f;
                        o.z = x.z > 0.f ? d0 * rr.w0[i][2] : 0.f;
                        o.w = x.w > 0.f ? d0 * rr.w0[i][3] : 0.f;
                        if (g) *reinterpret_cast<float4*>(g + k) = o;
                        if (g3_rc) {
                            const float ov[4] = {o.x, o.y, o.z, o.w};
                            unsigned pl4[4][3];
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                if (g3_np == 1) { pl4[e][0] = bf16_bits(ov[e]); pl4[e][1] = 0; pl4[e][2] = 0; }
                                else split3(ov[e], pl4[e]);
                            }
#pragma unroll
                            for (int q = 0; q < 3; ++q)
                                if (q < g3_np)
                                    *reinterpret_cast<uint2*>(g3_rc + q * g3_plane + (size_t)row * H + k) =
                                        make_uint2(pl4[0][q] | (pl4[1][q] << 16), pl4[2][q] | (pl4[3][q] << 16));
                        }
                    }
                }
            } else if (g) {
                for (int k = lane; k < H; k += 64) g[k] = h[k] > 0.f ? d0 * W4[k * 3] : 0.f;
            }
        }
    }
    // loss_pred = sum over ALL rows of pred[:,0] / (2 BN).  The sum is taken in 2^-32 fixed point: integer addition is associative, so
    // the blocks can add their part in any order with ONE relaxed device-scope atomic each and still produce the same bits on every run;
    // the block count rides in the top 16 bits of the same word, so the block that completes it needs no fence and no second look at
    // memory (a __threadfence() per block costs an L2 write-back on this chip: this kernel took 23 us with a ticket + fence, ~6 without)
    if (lane == 0) s_p[wave] = p0;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long part = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) part += (unsigned long long)__double2ll_rn((double)s_p[w] * 4294967296.0);   // pred >= 0
        const unsigned long long add = part + (1ull << 48);
        const unsigned long long old = atomicAdd(acc, add);
        if ((old >> 48) + 1 == (unsigned long long)gridDim.x) {
            const unsigned long long total = (old + add) & ((1ull << 48) - 1);
            loss[0] = (float)((double)total * (1.0 / 4294967296.0) / (2.0 * (double)BN));      // (:976-977)
            atomicExch(acc, 0ull);                                                               // ready for the next launch
        }
    }
}

// dy = dpred * mask * [0 < y < 6] / 3 ;  g3 = (dy W4^T) * [h3 > 0].  One wave per row.
struct ZeroList {   // small accumulators cleared by the first kernel of the backward chain (saves memset launches)
    float* p[5];
    int n[5];
};

__global__ __launch_bounds__(256) void out_bwd_kernel(const float* __restrict__ dpred, const float* __restrict__ mask,
                                                       const float* __restrict__ y, const float* __restrict__ h3,
                                                       const float* __restrict__ W4, float* __restrict__ dy,
                                                       float* __restrict__ g3, int Qb, int H, ZeroList zl) {
    if (blockIdx.x < 5 && zl.p[blockIdx.x]) {
        for (int i = threadIdx.x; i < zl.n[blockIdx.x]; i += 256) zl.p[blockIdx.x][i] = 0.f;
    }
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= Qb) return;
    float d[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float yv = y[(size_t)row * 3 + c];
        d[c] = (yv > 0.f && yv < 6.f) ? dpred[(size_t)row * 3 + c] * mask[row] / 3.0f : 0.f;   // relu6 gradient is 1 on (0,6)
    }
    if (lane < 3) dy[(size_t)row * 3 + lane] = d[lane];
    const float* h = h3 + (size_t)row * H;
    float* g = g3 + (size_t)row * H;
    for (int k = lane; k < H; k += 64) {
        const float v = d[0] * W4[k * 3] + d[1] * W4[k * 3 + 1] + d[2] * W4[k * 3 + 2];
        g[k] = (h[k] > 0.f) ? v : 0.f;
    }
}

// Fused output-layer backward: ONE pass over h3 produces dy, g3 AND the per-block partial sums of
//   db3 = colsum(g3), dW4 = h3^T dy, db4 = colsum(dy)
// (block = 32 rows, 4 waves x 8 rows; lane owns columns lane+64j).  Partials go to `scratch` [nblk][4H+4] and are
// summed in fixed order by small_grads_reduce -> deterministic, no atomics, no memset.  H <= 1024.
constexpr int kOBRows = 8;
constexpr int kOBMaxJ = 16;

__global__ __launch_bounds__(256) void out_bwd_fused_kernel(const float* __restrict__ dpred, const float* __restrict__ mask,
                                                             const float* __restrict__ y, const float* __restrict__ h3,
                                                             const float* __restrict__ W4, float* __restrict__ dy,
                                                             float* __restrict__ g3, int Qb, int H, ZeroList zl,
                                                             float* __restrict__ scratch) {
    extern __shared__ float s_acc[];   // [4H + 4]
    if (blockIdx.x < 5 && zl.p[blockIdx.x]) {
        for (int i = threadIdx.x; i < zl.n[blockIdx.x]; i += 256) zl.p[blockIdx.x][i] = 0.f;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nj = H / 64;
    float w4[kOBMaxJ][3], s3[kOBMaxJ], a4[kOBMaxJ][3];
#pragma unroll
    for (int j = 0; j < kOBMaxJ; ++j) {
        s3[j] = 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) { a4[j][c] = 0.f; w4[j][c] = (j < nj) ? W4[(lane + 64 * j) * 3 + c] : 0.f; }
    }
    float dsum[3] = {0.f, 0.f, 0.f};
    for (int rr = 0; rr < kOBRows / 4; ++rr) {
        const int row = blockIdx.x * kOBRows + wave * (kOBRows / 4) + rr;
        if (row >= Qb) break;
        float d[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float yv = y[(size_t)row * 3 + c];
            d[c] = (yv > 0.f && yv < 6.f) ? dpred[(size_t)row * 3 + c] * mask[row] / 3.0f : 0.f;   // relu6 gradient is 1 on (0,6)
            dsum[c] += d[c];
        }
        if (lane < 3) dy[(size_t)row * 3 + lane] = d[lane];
        const float* h = h3 + (size_t)row * H;
        float* g = g3 + (size_t)row * H;
#pragma unroll
        for (int j = 0; j < kOBMaxJ; ++j) {
            if (j < nj) {
                const int k = lane + 64 * j;
                const float hv = h[k];
                const float v = d[0] * w4[j][0] + d[1] * w4[j][1] + d[2] * w4[j][2];
                const float gv = (hv > 0.f) ? v : 0.f;
                g[k] = gv;
                s3[j] += gv;
#pragma unroll
                for (int c = 0; c < 3; ++c) a4[j][c] += hv * d[c];
            }
        }
    }
    // fixed-order reduction over the 4 waves
    for (int w = 0; w < 4; ++w) {
        if (wave == w) {
#pragma unroll
            for (int j = 0; j < kOBMaxJ; ++j) {
                if (j < nj) {
                    const int k = lane + 64 * j;
                    if (w == 0) {
                        s_acc[k] = s3[j];
#pragma unroll
                        for (int c = 0; c < 3; ++c) s_acc[H + k * 3 + c] = a4[j][c];
                    } else {
                        s_acc[k] += s3[j];
#pragma unroll
                        for (int c = 0; c < 3; ++c) s_acc[H + k * 3 + c] += a4[j][c];
                    }
                }
            }
            if (lane < 3) {
                const float v = (lane == 0) ? dsum[0] : ((lane == 1) ? dsum[1] : dsum[2]);
                if (w == 0) s_acc[4 * H + lane] = v;
                else s_acc[4 * H + lane] += v;
            }
        }
        __syncthreads();
    }
    float* out = scratch + (size_t)blockIdx.x * (4 * H + 4);
    for (int i = threadIdx.x; i < 4 * H + 3; i += 256) out[i] = s_acc[i];
}

// Same contract as out_bwd_fused_kernel for H % 256 == 0, H <= 1024: a lane owns 4 consecutive columns in each
// 256-column group (float4 loads/stores, both rows of a wave in flight together) and the four waves' partials are
// combined with ONE barrier (each wave has its own LDS slab).  LDS: 4 * (4H + 4) floats.
// L1: optional fused loss (training mode, utils/dpdist_util.py:962-980): with l1.labels the kernel derives
// d loss_samples / d pred_AB = sign(pred_AB[:,0] - labels) * gscale / Qb itself (dpred is not read) and adds the three loss sums
// (sum |pred_AB - labels|, sum pred_AB, sum pred_BA over its rows) to the block record [4H+4 .. 4H+6].
struct L1Fuse {
    const float* pred;     // [2*Qb, 3]
    const float* labels;   // [Qb]
    float gscale;
};
constexpr int kOBRec = 8;   // record = 4H + 8 floats: db3 [H] | dW4 [3H] | db4 [3] | pad | loss sums [3] | pad
// Optional bf16 operand planes of g3 written by the same pass (plane compute types: no fp32 g3, no conversion launch): RC
// [np][Qb][H] straight from the registers, R8 [np][Qb/8][H][8] through an LDS image of the block's 8 rows (behind the four slabs).
struct G3Planes {
    uint16_t* rc;
    uint16_t* r8;
    long plane;     // elements per plane (Qb * H)
    int np;
};
// Optional forward of the output layer inside the same pass (training step: no out_fwd launch, h3 rows of the AB half are read
// once): with y != NULL the kernel computes y = h3 W4 + b4 and pred = relu6(y)/3 * mask for its AB rows AND their BA twins
// (row + Qb), in out_fwd_kernel's summation order (bit-identical), writes both, and uses them instead of the y / l1.pred inputs.
struct OutFwd {
    const float* b4;
    float* y;       // [2*Qb, 3]
    float* pred;    // [2*Qb, 3]
};

__global__ __launch_bounds__(256) void out_bwd_fused4_kernel(const float* __restrict__ dpred, const float* __restrict__ mask,
                                                              const float* __restrict__ y, const float* __restrict__ h3,
                                                              const float* __restrict__ W4, float* __restrict__ dy,
                                                              float* __restrict__ g3, int Qb, int H, ZeroList zl,
                                                              float* __restrict__ scratch, L1Fuse l1, OutFwd of, G3Planes gp,
                                                              const uint16_t* __restrict__ h3b) {
    extern __shared__ float s_acc[];   // [4 waves][4H + 8]; reused at the end (gp.r8) as uint16 [np][8][H]
    if (blockIdx.x < 5 && zl.p[blockIdx.x]) {
        for (int i = threadIdx.x; i < zl.n[blockIdx.x]; i += 256) zl.p[blockIdx.x][i] = 0.f;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ng = H / 256;            // column groups (<= 4)
    const int P = 4 * H + kOBRec;
    constexpr int RW = kOBRows / 4;    // rows per wave
    float lsum[3] = {0.f, 0.f, 0.f};   // loss sums of this wave's rows (identical in every lane)
    float dsum[3] = {0.f, 0.f, 0.f};
    float d[RW][3];
    float4 hv[RW][4], hb[RW][4];
    const int row0 = blockIdx.x * kOBRows + wave * RW;
    // Every global load of the kernel is requested HERE, before anything waits: W4 above, the rows (and their BA twins) and the per-row
    // scalars below.  Left where they were used, they made three dependent round trips (W4 -> row 0 -> row 1: 5.5k + 3.9k + 5.7k cycles
    // of a 25k-cycle kernel at B = 32, s_memtime stamps); with one workgroup per CU there is nothing else to hide them behind.
    static_assert(RW == 2, "the lane-pair exchanges below assume two rows per wave");
    const bool odd = lane & 1;
    // exchange a 64-bit value with lane ^ 1 (DPP quad_perm [1,0,3,2])
    auto swap_pair = [](uint2 v) {
        return make_uint2((unsigned)__builtin_amdgcn_mov_dpp((int)v.x, 0xB1, 0xf, 0xf, true), (unsigned)__builtin_amdgcn_mov_dpp((int)v.y, 0xB1, 0xf, 0xf, true));
    };
    auto widen = [](uint2 u) {
        return make_float4(__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u), __uint_as_float(u.y << 16), __uint_as_float(u.y & 0xffff0000u));
    };
    if (h3b) {
        // layer 3's activation as one bf16 plane (DPD_BF16), widened exactly.  A lane's four columns of one row are 8 bytes, and 8-byte
        // accesses run at ~0.6 of the 16-byte rate (round 5: this load phase was 12k of the kernel's 37k cycles at B = 64): the lanes
        // 2p / 2p + 1 therefore load 16 bytes -- the eight columns of BOTH lanes -- of row 0 / row 1 and hand each other the half that
        // belongs to the partner.  Same values in the same registers as two 8-byte loads per lane.
        const int rsel = min(row0 + (odd ? 1 : 0), Qb - 1);
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            if (jj < ng) {
                const uint4 va = *reinterpret_cast<const uint4*>(h3b + (size_t)rsel * H + 256 * jj + 8 * (lane >> 1));
                const uint2 ra = swap_pair(odd ? make_uint2(va.x, va.y) : make_uint2(va.z, va.w));
                hv[0][jj] = widen(odd ? ra : make_uint2(va.x, va.y));
                hv[1][jj] = widen(odd ? make_uint2(va.z, va.w) : ra);
                if (of.y) {
                    const uint4 vb = *reinterpret_cast<const uint4*>(h3b + ((size_t)Qb + rsel) * H + 256 * jj + 8 * (lane >> 1));
                    const uint2 rb = swap_pair(odd ? make_uint2(vb.x, vb.y) : make_uint2(vb.z, vb.w));
                    hb[0][jj] = widen(odd ? rb : make_uint2(vb.x, vb.y));
                    hb[1][jj] = widen(odd ? make_uint2(vb.z, vb.w) : rb);
                }
            }
        }
    } else {
#pragma unroll
        for (int rr = 0; rr < RW; ++rr) {
            const int row = min(row0 + rr, Qb - 1);
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                if (jj < ng) {
                    hv[rr][jj] = *reinterpret_cast<const float4*>(h3 + (size_t)row * H + 256 * jj + 4 * lane);
                    if (of.y) hb[rr][jj] = *reinterpret_cast<const float4*>(h3 + ((size_t)Qb + row) * H + 256 * jj + 4 * lane);
                }
            }
        }
    }
    float w4[4][4][3], s3[4][4], a4[4][4][3];
    const bool w4_vec = !((uintptr_t)W4 & 15);       // the 12 floats W4[k..k+3][0..2] of a lane's four columns are three float4 (k % 4 == 0)
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
        if (w4_vec && jj < ng) {      // 12 loads per lane instead of 48: the address unit was ~6k of this kernel's 24k cycles at B = 32
            const float4* wp = reinterpret_cast<const float4*>(W4 + (size_t)(256 * jj + 4 * lane) * 3);
            const float4 wa = wp[0], wb = wp[1], wc = wp[2];
            const float w[12] = {wa.x, wa.y, wa.z, wa.w, wb.x, wb.y, wb.z, wb.w, wc.x, wc.y, wc.z, wc.w};
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int c = 0; c < 3; ++c) w4[jj][e][c] = w[3 * e + c];
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            s3[jj][e] = 0.f;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                a4[jj][e][c] = 0.f;
                if (!(w4_vec && jj < ng)) w4[jj][e][c] = (jj < ng) ? W4[(256 * jj + 4 * lane + e) * 3 + c] : 0.f;
            }
        }
    }
    // the per-row scalars are requested before the row loop: behind the dot products and wave sums they were one more dependent round trip
    float mk_a[RW], mk_b[RW], lab[RW];
#pragma unroll
    for (int rr = 0; rr < RW; ++rr) {
        const int row = min(row0 + rr, Qb - 1);
        mk_a[rr] = mask[row];
        mk_b[rr] = of.y ? mask[Qb + row] : 0.f;
        lab[rr] = l1.labels ? l1.labels[row] : 0.f;
    }
#pragma unroll
    for (int rr = 0; rr < RW; ++rr) {
        const int row = min(row0 + rr, Qb - 1);
        const bool live = row0 + rr < Qb;
        float yab[3] = {0.f, 0.f, 0.f}, pab0 = 0.f, pba0 = 0.f;
        if (of.y) {                // forward of the output layer for this AB row and its BA twin (out_fwd_kernel's order)
            float a[3] = {0.f, 0.f, 0.f}, b[3] = {0.f, 0.f, 0.f};
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                if (jj < ng) {
                    const float xa[4] = {hv[rr][jj].x, hv[rr][jj].y, hv[rr][jj].z, hv[rr][jj].w};
                    const float xb[4] = {hb[rr][jj].x, hb[rr][jj].y, hb[rr][jj].z, hb[rr][jj].w};
#pragma unroll
                    for (int e = 0; e < 4; ++e)
#pragma unroll
                        for (int c = 0; c < 3; ++c) { a[c] += xa[e] * w4[jj][e][c]; b[c] += xb[e] * w4[jj][e][c]; }
                }
            }
            // empty asm = a schedule fence: row 0's dot products finish before its wave sums start (the instruction order this kernel
            // was measured with; without it the compiler interleaves the two)
            if (rr == 0) asm volatile("" :: "v"(a[0]), "v"(b[2]));
            float yba[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) { yab[c] = wave_sum(a[c]) + of.b4[c]; yba[c] = wave_sum(b[c]) + of.b4[c]; }
            const float ma = mk_a[rr], mb = mk_b[rr];
            float pa[3], pb[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                pa[c] = fminf(fmaxf(yab[c], 0.f), 6.f) / 3.0f * ma;   // relu6(y)/3 (:691) * mask (:697)
                pb[c] = fminf(fmaxf(yba[c], 0.f), 6.f) / 3.0f * mb;
            }
            pab0 = pa[0]; pba0 = pb[0];
            if (live && lane < 3) {
                const float ya = lane == 0 ? yab[0] : (lane == 1 ? yab[1] : yab[2]), yb = lane == 0 ? yba[0] : (lane == 1 ? yba[1] : yba[2]);
                const float qa = lane == 0 ? pa[0] : (lane == 1 ? pa[1] : pa[2]), qb = lane == 0 ? pb[0] : (lane == 1 ? pb[1] : pb[2]);
                of.y[(size_t)row * 3 + lane] = ya; of.y[((size_t)Qb + row) * 3 + lane] = yb;
                of.pred[(size_t)row * 3 + lane] = qa; of.pred[((size_t)Qb + row) * 3 + lane] = qb;
            }
        }
        float dp[3];
        if (l1.labels) {           // d mean|pred_AB[:,0] - labels| / d pred_AB (tf.abs gradient = sign), channels 1, 2 get none
            const float pab = of.y ? pab0 : l1.pred[(size_t)row * 3], pba = of.y ? pba0 : l1.pred[((size_t)Qb + row) * 3];
            const float df = pab - lab[rr];
            dp[0] = ((df > 0.f) ? 1.f : ((df < 0.f) ? -1.f : 0.f)) * (1.0f / (float)Qb) * l1.gscale;
            dp[1] = 0.f; dp[2] = 0.f;
            if (live) { lsum[0] += fabsf(df); lsum[1] += pab; lsum[2] += pba; }
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) dp[c] = dpred[(size_t)row * 3 + c];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float yv = of.y ? yab[c] : y[(size_t)row * 3 + c];
            d[rr][c] = (live && yv > 0.f && yv < 6.f) ? dp[c] * mk_a[rr] / 3.0f : 0.f;   // relu6' = 1 on (0,6)
            dsum[c] += d[rr][c];
        }
    }
    uint2 wpk[RW][4][3] = {};
#pragma unroll
    for (int rr = 0; rr < RW; ++rr) {
        const int row = row0 + rr;
        if (row >= Qb) break;
        if (lane < 3) dy[(size_t)row * 3 + lane] = d[rr][lane];
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            if (jj < ng) {
                const float hh[4] = {hv[rr][jj].x, hv[rr][jj].y, hv[rr][jj].z, hv[rr][jj].w};
                float gg[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float v = d[rr][0] * w4[jj][e][0] + d[rr][1] * w4[jj][e][1] + d[rr][2] * w4[jj][e][2];
                    gg[e] = (hh[e] > 0.f) ? v : 0.f;
                    s3[jj][e] += gg[e];
#pragma unroll
                    for (int c = 0; c < 3; ++c) a4[jj][e][c] += hh[e] * d[rr][c];
                }
                if (g3) *reinterpret_cast<float4*>(g3 + (size_t)row * H + 256 * jj + 4 * lane) = make_float4(gg[0], gg[1], gg[2], gg[3]);
                if (gp.rc || gp.r8) {
                    unsigned pl4[4][3];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        if (gp.np == 1) { pl4[e][0] = bf16_bits(gg[e]); pl4[e][1] = 0; pl4[e][2] = 0; }     // one plane: one conversion, not the three-plane split
                        else split3(gg[e], pl4[e]);
                    }
                    const int col = 256 * jj + 4 * lane;
#pragma unroll
                    for (int q = 0; q < 3; ++q) {
                        const uint2 w = make_uint2(pl4[0][q] | (pl4[1][q] << 16), pl4[2][q] | (pl4[3][q] << 16));
                        wpk[rr][jj][q] = w;      // kept in registers: the LDS image for the R8 chunks reuses the slabs once they are summed
                    }
                    (void)col;
                }
            }
        }
    }
    if (gp.rc) {
        // RC planes: lane 2p stores the eight columns of lanes 2p / 2p + 1 of row 0, lane 2p + 1 those of row 1 -- one 16-byte store per
        // lane, column group and plane instead of two 8-byte ones (the planes exist only for whole 8-row blocks: both rows are valid)
        uint16_t* rcp = gp.rc + (size_t)(row0 + (odd ? 1 : 0)) * H + 8 * (lane >> 1);
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            if (jj < ng) {
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    if (q < gp.np) {
                        const uint2 got = swap_pair(odd ? wpk[0][jj][q] : wpk[1][jj][q]);
                        const uint2 lo = odd ? got : wpk[0][jj][q], hi = odd ? wpk[1][jj][q] : got;
                        *reinterpret_cast<uint4*>(rcp + q * gp.plane + 256 * jj) = make_uint4(lo.x, lo.y, hi.x, hi.y);
                    }
                }
            }
        }
    }
    float* mine = s_acc + wave * P;
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
        if (jj < ng) {
            const int k = 256 * jj + 4 * lane;          // four columns: 4 + 12 contiguous floats, 16-byte aligned (H % 256 == 0, P % 4 == 0)
            *reinterpret_cast<float4*>(mine + k) = make_float4(s3[jj][0], s3[jj][1], s3[jj][2], s3[jj][3]);
            float4* m4 = reinterpret_cast<float4*>(mine + H + k * 3);
            m4[0] = make_float4(a4[jj][0][0], a4[jj][0][1], a4[jj][0][2], a4[jj][1][0]);
            m4[1] = make_float4(a4[jj][1][1], a4[jj][1][2], a4[jj][2][0], a4[jj][2][1]);
            m4[2] = make_float4(a4[jj][2][2], a4[jj][3][0], a4[jj][3][1], a4[jj][3][2]);
        }
    }
    if (lane < 3) mine[4 * H + lane] = (lane == 0) ? dsum[0] : ((lane == 1) ? dsum[1] : dsum[2]);
    if (lane < 3) mine[4 * H + 4 + lane] = (lane == 0) ? lsum[0] : ((lane == 1) ? lsum[1] : lsum[2]);
    if (lane == 3) { mine[4 * H + 3] = 0.f; mine[4 * H + 7] = 0.f; }
    __syncthreads();
    float* out = scratch + (size_t)blockIdx.x * P;
    for (int i = threadIdx.x; i < 4 * H + 7; i += 256) out[i] = ((s_acc[i] + s_acc[P + i]) + s_acc[2 * P + i]) + s_acc[3 * P + i];
    if (gp.r8) {      // the block's 8 rows = one row group: column c's chunk = its 8 rows (Qb % 8 == 0 when planes are in use)
        uint16_t* s_g = reinterpret_cast<uint16_t*>(s_acc);      // [np][8][H] <= 48 KiB: inside the four slabs, which are summed by now
        __syncthreads();
#pragma unroll
        for (int rr = 0; rr < RW; ++rr)
#pragma unroll
            for (int jj = 0; jj < 4; ++jj)
                if (jj < ng)
                    for (int q = 0; q < gp.np; ++q)
                        *reinterpret_cast<uint2*>(s_g + ((size_t)(q * kOBRows + wave * RW + rr) * H + 256 * jj + 4 * lane)) = wpk[rr][jj][q < 3 ? q : 0];
        __syncthreads();
        for (int c = threadIdx.x; c < H; c += 256)
            for (int q = 0; q < gp.np; ++q) {
                unsigned b[8];
#pragma unroll
                for (int rr = 0; rr < 8; ++rr) b[rr] = s_g[(size_t)(q * kOBRows + rr) * H + c];
                *reinterpret_cast<uint4*>(gp.r8 + q * gp.plane + ((size_t)blockIdx.x * H + c) * 8) =
                    make_uint4(b[0] | (b[1] << 16), b[2] | (b[3] << 16), b[4] | (b[5] << 16), b[6] | (b[7] << 16));
            }
    }
}

// out[i] = sum_b scratch[b][i] in a fixed order: 16 outputs x 16 block-slices per workgroup, LDS tree at the end
// rec = floats per block record (4H + 4, or 4H + 8 when the record carries the three loss sums at [4H+4 .. 4H+6]); loss (may be
// NULL) then receives loss_samples = sum|pred_AB - labels| / Qb and loss_pred = (sum pred_AB / Qb + sum pred_BA / Qb) / 2.
__global__ __launch_bounds__(256) void small_grads_reduce(const float* __restrict__ scratch, int nblk, int H,
                                                           float* __restrict__ db3, float* __restrict__ dW4,
                                                           float* __restrict__ db4, int rec, float* __restrict__ loss, int Qb) {
    __shared__ float red[16][17];
    __shared__ float s_loss[3];
    const int li = threadIdx.x & 15, sl = threadIdx.x >> 4;
    const int i = blockIdx.x * 16 + li;
    const int n = (rec > 4 * H + 4 && loss) ? 4 * H + 7 : 4 * H + 3;
    float s = 0.f;
    if (i < n)
        for (int b = sl; b < nblk; b += 16) s += scratch[(size_t)b * rec + i];
    red[sl][li] = s;
    __syncthreads();
    if (sl == 0 && i < n) {
        float t = 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) t += red[k][li];
        if (i < H) { if (db3) db3[i] = t; }
        else if (i < 4 * H) { if (dW4) dW4[i - H] = t; }
        else if (i < 4 * H + 3) { if (db4) db4[i - 4 * H] = t; }
        else if (i >= 4 * H + 4) s_loss[i - 4 * H - 4] = t;       // the three loss sums land in ONE workgroup (16 outputs each)
    }
    if (n > 4 * H + 3 && blockIdx.x == (4 * H + 4) / 16) {
        __syncthreads();
        if (threadIdx.x == 0) {
            const float inv = 1.0f / (float)Qb;
            loss[0] = s_loss[0] * inv;
            loss[1] = (s_loss[1] * inv + s_loss[2] * inv) / 2.0f;
        }
    }
}

// Column sums in two deterministic stages.  Stage 1: block (colblock, chunk) -> partial[chunk][...].
//   NW = 0: partial[chunk][n]     = sum_r g[r][n]                       (bias gradient)
//   NW = 3: partial[chunk][n*3+c] = sum_r a[r][n] * w[r*3+c]            (dW4 = h3^T dy)
constexpr int kColChunks = 16;

template <int NW>
__global__ __launch_bounds__(256) void colsum_stage1(const float* __restrict__ a, int lda, const float* __restrict__ w,
                                                      int R, int Ncols, float* __restrict__ partial) {
    __shared__ float red[4][64 * (NW ? NW : 1)];
    const int col = blockIdx.x * 64 + (threadIdx.x & 63), rs = threadIdx.x >> 6, chunk = blockIdx.y;
    const int rper = (R + kColChunks - 1) / kColChunks;
    const int r0 = chunk * rper, r1 = min(R, r0 + rper);
    float acc[NW ? NW : 1];
#pragma unroll
    for (int c = 0; c < (NW ? NW : 1); ++c) acc[c] = 0.f;
    if (col < Ncols) {
        for (int r = r0 + rs; r < r1; r += 4) {
            const float x = a[(size_t)r * lda + col];
            if (NW == 0) acc[0] += x;
            else {
#pragma unroll
                for (int c = 0; c < NW; ++c) acc[c] += x * w[(size_t)r * NW + c];
            }
        }
    }
    constexpr int W = NW ? NW : 1;
#pragma unroll
    for (int c = 0; c < W; ++c) red[rs][(threadIdx.x & 63) * W + c] = acc[c];
    __syncthreads();
    if (rs == 0 && col < Ncols) {
#pragma unroll
        for (int c = 0; c < W; ++c) {
            const int i = (threadIdx.x & 63) * W + c;
            partial[((size_t)chunk * Ncols + col) * W + c] = (red[0][i] + red[1][i]) + (red[2][i] + red[3][i]);
        }
    }
}

// Single-launch variant: every (column block, row chunk) adds its partial with one atomic per output element
// (output must be zero on entry).  Used for db3 and dW4/db4 inside the backward data chain.
template <int NW>
__global__ __launch_bounds__(256) void colsum_atomic(const float* __restrict__ a, int lda, const float* __restrict__ w,
                                                      int R, int Ncols, float* __restrict__ out, float* __restrict__ wsum) {
    constexpr int W = NW ? NW : 1;
    __shared__ float red[4][64 * W];
    const int col = blockIdx.x * 64 + (threadIdx.x & 63), rs = threadIdx.x >> 6, chunk = blockIdx.y;
    const int rper = (R + gridDim.y - 1) / gridDim.y;
    const int r0 = chunk * rper, r1 = min(R, r0 + rper);
    float acc[W];
#pragma unroll
    for (int c = 0; c < W; ++c) acc[c] = 0.f;
    if (col < Ncols) {
        for (int r = r0 + rs; r < r1; r += 4) {
            const float x = a[(size_t)r * lda + col];
            if (NW == 0) acc[0] += x;
            else {
#pragma unroll
                for (int c = 0; c < NW; ++c) acc[c] += x * w[(size_t)r * NW + c];
            }
        }
    }
#pragma unroll
    for (int c = 0; c < W; ++c) red[rs][(threadIdx.x & 63) * W + c] = acc[c];
    __syncthreads();
    if (rs == 0 && col < Ncols) {
#pragma unroll
        for (int c = 0; c < W; ++c) {
            const int i = (threadIdx.x & 63) * W + c;
            atomicAdd(out + (size_t)col * W + c, (red[0][i] + red[1][i]) + (red[2][i] + red[3][i]));
        }
    }
    if (NW && wsum && blockIdx.x == 0) {   // column sums of w itself (db4 = colsum(dy)), one block column does it
        float s[W];
#pragma unroll
        for (int c = 0; c < W; ++c) s[c] = 0.f;
        for (int r = r0 + threadIdx.x; r < r1; r += 256)
#pragma unroll
            for (int c = 0; c < W; ++c) s[c] += w[(size_t)r * NW + c];
#pragma unroll
        for (int c = 0; c < W; ++c) {
            s[c] = wave_sum(s[c]);
            if ((threadIdx.x & 63) == 0) atomicAdd(wsum + c, s[c]);
        }
    }
}

__global__ __launch_bounds__(256) void colsum_stage2(const float* __restrict__ partial, int n, float* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < kColChunks; ++c) s += partial[(size_t)c * n + i];
    out[i] = s;
}

// dy [R,3] column sums (db4): single block
__global__ __launch_bounds__(256) void dy_colsum_kernel(const float* __restrict__ dy, int R, float* __restrict__ db) {
    __shared__ float red[4][3];
    float a[3] = {0.f, 0.f, 0.f};
    for (int r = threadIdx.x; r < R; r += 256) {
        a[0] += dy[(size_t)r * 3]; a[1] += dy[(size_t)r * 3 + 1]; a[2] += dy[(size_t)r * 3 + 2];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        a[c] = wave_sum(a[c]);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][c] = a[c];
    }
    __syncthreads();
    if (threadIdx.x < 3) db[threadIdx.x] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

static size_t colsum_ws_floats(int ncols, int nw) { return (size_t)kColChunks * ncols * (nw ? nw : 1); }

// out[c][r] = in[r][c] for up to three matrices in one launch (64x64 tiles through LDS, both sides coalesced)
struct TransposeJobs {
    const float* in[3];
    float* out[3];
    int R[3], C[3], blk0[4];
    int n;
};
__global__ __launch_bounds__(256) void transpose_kernel(TransposeJobs J) {
    __shared__ float t[64][65];
    int j = 0;
    while (j + 1 < J.n && (int)blockIdx.x >= J.blk0[j + 1]) ++j;
    const int R = J.R[j], C = J.C[j], tc = (C + 63) / 64;
    const int b = blockIdx.x - J.blk0[j];
    const int r0 = (b / tc) * 64, c0 = (b % tc) * 64;
    const float* __restrict__ in = J.in[j];
    float* __restrict__ out = J.out[j];
    const int x4 = (threadIdx.x & 15) * 4, y0 = threadIdx.x >> 4;          // 16 float4 per 64-wide row, 16 rows per pass
    const bool vec = !(C & 3) && !(R & 3);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int y = y0 + 16 * i;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r0 + y < R) {
            const float* src = in + (size_t)(r0 + y) * C + c0 + x4;
            if (vec && c0 + x4 + 3 < C) v = *reinterpret_cast<const float4*>(src);
            else {
                if (c0 + x4 < C) v.x = src[0];
                if (c0 + x4 + 1 < C) v.y = src[1];
                if (c0 + x4 + 2 < C) v.z = src[2];
                if (c0 + x4 + 3 < C) v.w = src[3];
            }
        }
        t[y][x4] = v.x; t[y][x4 + 1] = v.y; t[y][x4 + 2] = v.z; t[y][x4 + 3] = v.w;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int y = y0 + 16 * i;                                           // output row c0 + y, output columns r0 + x4 .. +3
        if (c0 + y < C) {
            const float4 v = make_float4(t[x4][y], t[x4 + 1][y], t[x4 + 2][y], t[x4 + 3][y]);
            float* dst = out + (size_t)(c0 + y) * R + r0 + x4;
            if (vec && r0 + x4 + 3 < R) *reinterpret_cast<float4*>(dst) = v;
            else {
                if (r0 + x4 < R) dst[0] = v.x;
                if (r0 + x4 + 1 < R) dst[1] = v.y;
                if (r0 + x4 + 2 < R) dst[2] = v.z;
                if (r0 + x4 + 3 < R) dst[3] = v.w;
            }
        }
    }
}

// Layer 1 over distinct windows, second step (dpd_decoder_fwd_unique): wave = one 32 x 32 tile of h1.  The accumulators of row r are
// those of its window, Pu[uid[r]] (the chain over the K-tiles before the last), loaded in the MFMA accumulator layout; the chain goes on
// with the 16 MFMAs of the last K-tile on Xt [Q, 32] and the last 32 rows of W1p -- the same (b, s) order and lane <-> k assignment as
// gemm_rs_kernel (k = 16 half + 4 b + s) -- then bias, ReLU and put_tile.  An fp32 accumulator that passes through memory keeps its
// bits, so h1 is bit for bit what gemm_rs_kernel leaves for the whole rows.
__global__ __launch_bounds__(256) void l1_finish_kernel(const float* __restrict__ Pu, const int32_t* __restrict__ uid,
                                                        const float* __restrict__ Xt, const float* __restrict__ Wt,
                                                        const float* __restrict__ bias, float* __restrict__ h1, int Q, int H) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int l31 = lane & 31, half = lane >> 5;
    const int tilesN = H / 32, t = blockIdx.x * 4 + wave;
    if (t >= (Q / 32) * tilesN) return;
    const int m0 = (t / tilesN) * 32, col = (t % tilesN) * 32 + l31;
    int u[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) u[r] = uid[m0 + (r & 3) + 8 * (r >> 2) + 4 * half];
    float a[4][4], w[4][4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const float4 x = *reinterpret_cast<const float4*>(Xt + (size_t)(m0 + l31) * 32 + 16 * half + 4 * b);
        a[b][0] = x.x; a[b][1] = x.y; a[b][2] = x.z; a[b][3] = x.w;
#pragma unroll
        for (int s = 0; s < 4; ++s) w[b][s] = Wt[(size_t)(16 * half + 4 * b + s) * H + col];
    }
    const float bv = bias[col];
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = Pu[(size_t)u[r] * H + col];
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[b][s], w[b][s], acc, 0, 0, 0);
    float v[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) v[r] = fmaxf(acc[r] + bv, 0.f);
    GemmArgs g{};
    g.C = h1; g.M = Q; g.N = H; g.ldc = H;
    put_tile(g, v, 0, m0, col, half);
}

// All-pairs distance matrix (dpd_decoder_fwd_cross): Dd[p] = mean over the N rows of pair p of pred[:, 0].  One wave per pair: lane l
// adds rows l, l + 64, ... in order, then the fixed tree of wave_sum -- the same order for every pair, whatever the launch holds.
// CNT (dpd_decoder_fwd_cross_counts): pair p = (i, j) sums the first qcounts[j] of its N rows (clamped into [1, N]) and divides by that
// count; the same lane order and tree.
template <bool CNT>
__device__ __forceinline__ void pair_mean_block(const float* __restrict__ pred, int N, int pairs, float* __restrict__ Dd,
                                                const int32_t* __restrict__ qcounts, int Cb) {
    const int lane = threadIdx.x & 63, pr = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pr >= pairs) return;
    const float* src = pred + (size_t)pr * N * 3;
    const int n1 = CNT ? min(max(qcounts[pr % Cb], 1), N) : N;
    float a = 0.f;
    for (int n = lane; n < n1; n += 64) a += src[(size_t)n * 3];
    a = wave_sum(a);
    if (lane == 0) Dd[pr] = a / (float)n1;
}
__global__ __launch_bounds__(256) void pair_mean_kernel(const float* __restrict__ pred, int N, int pairs, float* __restrict__ Dd) {
    pair_mean_block<false>(pred, N, pairs, Dd, nullptr, 1);
}
__global__ __launch_bounds__(256) void pair_mean_counts_kernel(const float* __restrict__ pred, const int32_t* __restrict__ qcounts, int N,
                                                               int pairs, int Cb, float* __restrict__ Dd) {
    pair_mean_block<true>(pred, N, pairs, Dd, qcounts, Cb);
}

// Paired distances of clouds of different sizes (dpd_decoder_out_pairs).  Row layout of P pairs: the AB half first (row b Wb + n: query
// B_b[n], Wb rows per pair, real while n < countsB[b]), then the BA half at P Wb (row P Wb + b Wa + n: query A_b[n], real while
// n < countsA[b]).  A segment = one (direction, pair): its rows are contiguous, its length is the query set's width, and neither its
// start nor its length is aligned with anything (widths like 37, 5, 1; the two halves differ).
struct PairSeg {
    int b, n, cnt;      // pair, query index inside the segment, the segment's real queries (clamped into [1, width])
    long row0;          // first row of the segment
};
__device__ __forceinline__ int pair_count(const int32_t* __restrict__ counts, int b, int W) { return counts ? min(max(counts[b], 1), W) : W; }
__device__ __forceinline__ PairSeg pair_seg_of_row(long row, int P, int Wa, int Wb, const int32_t* __restrict__ cA,
                                                   const int32_t* __restrict__ cB) {
    const long nab = (long)P * Wb;
    const bool ba = row >= nab;
    const long rr = ba ? row - nab : row;
    const int W = ba ? Wa : Wb;
    PairSeg s;
    s.b = (int)(rr / W);
    s.n = (int)(rr - (long)s.b * W);
    s.cnt = pair_count(ba ? cA : cB, s.b, W);
    s.row0 = row - s.n;
    return s;
}

// One wave per row: y / pred through out_row_dot (the bits of out_fwd_kernel), and -- with dy -- the output-layer backward of
// sum_b (D_AB[b] + D_BA[b]): unit upstream per directed distance, 1 / count of the row's own segment on channel 0, as out_asloss_kernel
// forms it.  The row of a padded query (n >= count) is written as +0.0 in dy and g3, whatever the sign of W4.
__global__ __launch_bounds__(256) void out_pairs_kernel(const float* __restrict__ h3, const float* __restrict__ W4,
                                                         const float* __restrict__ b4, const float* __restrict__ mask,
                                                         float* __restrict__ y, float* __restrict__ pred, float* __restrict__ dy,
                                                         float* __restrict__ g3, int P, int Wa, int Wb, const int32_t* __restrict__ cA,
                                                         const int32_t* __restrict__ cB, int H) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (long)P * ((long)Wa + Wb)) return;
    const float* h = h3 + (size_t)row * H;
    float a[3];
    OutRowRegs rr;
    out_row_dot(h, W4, H, lane, a, &rr);
    const float mk = mask[row];
    float yv[3], pv[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        yv[c] = a[c] + b4[c];
        pv[c] = fminf(fmaxf(yv[c], 0.f), 6.f) / 3.0f * mk;
    }
    if (lane < 3) {
        y[(size_t)row * 3 + lane] = lane == 0 ? yv[0] : (lane == 1 ? yv[1] : yv[2]);
        pred[(size_t)row * 3 + lane] = lane == 0 ? pv[0] : (lane == 1 ? pv[1] : pv[2]);
    }
    if (!dy) return;
    const PairSeg sg = pair_seg_of_row(row, P, Wa, Wb, cA, cB);
    const bool real = sg.n < sg.cnt;
    const float d0 = (real && yv[0] > 0.f && yv[0] < 6.f) ? (1.0f / (float)sg.cnt) * mk / 3.0f : 0.f;
    if (lane < 3) dy[(size_t)row * 3 + lane] = lane == 0 ? d0 : 0.f;
    float* g = g3 + (size_t)row * H;
    if (out_row_fast(W4, H)) {
#pragma unroll
        for (int i = 0; i < kOutMaxI; ++i) {
            const int k = 4 * lane + 256 * i;
            if (k < H) {
                const float4 x = rr.h[i];
                float4 o;
                o.x = (real && x.x > 0.f) ? d0 * rr.w0[i][0] : 0.f;
                o.y = (real && x.y > 0.f) ? d0 * rr.w0[i][1] : 0.f;
                o.z = (real && x.z > 0.f) ? d0 * rr.w0[i][2] : 0.f;
                o.w = (real && x.w > 0.f) ? d0 * rr.w0[i][3] : 0.f;
                *reinterpret_cast<float4*>(g + k) = o;
            }
        }
    } else {
        for (int k = lane; k < H; k += 64) g[k] = (real && h[k] > 0.f) ? d0 * W4[k * 3] : 0.f;
    }
}

// Dd [2, P]: one workgroup per segment.  Thread t adds pred[:, 0] of the segment's real rows t, t + 256, ... in 2^-32 fixed point
// (pred lies in [0, 2]: at most 2^33 per row), the 256 partial sums are added in a tree through LDS: integer addition, so the sum is
// exact, the same on every run and independent of what else the launch holds.  One rounding to double, one division, one to float.
__global__ __launch_bounds__(256) void pairs_mean_kernel(const float* __restrict__ pred, int P, int Wa, int Wb,
                                                          const int32_t* __restrict__ cA, const int32_t* __restrict__ cB,
                                                          float* __restrict__ Dd) {
    __shared__ unsigned long long s_part[256];
    const int ba = blockIdx.x >= (unsigned)P, b = ba ? blockIdx.x - P : blockIdx.x;
    const int W = ba ? Wa : Wb;
    const int cnt = pair_count(ba ? cA : cB, b, W);
    const float* src = pred + ((size_t)(ba ? (long)P * Wb : 0L) + (size_t)b * W) * 3;
    unsigned long long acc = 0;
    for (int n = threadIdx.x; n < cnt; n += 256) acc += (unsigned long long)__double2ll_rn((double)src[(size_t)n * 3] * 4294967296.0);
    s_part[threadIdx.x] = acc;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) s_part[threadIdx.x] += s_part[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x == 0) Dd[blockIdx.x] = (float)((double)s_part[0] * (1.0 / 4294967296.0) / (double)cnt);
}

// ---------------------------------------------------------------------------------------------------------
// Live rows of the exact-fp32 backward (dpd_live_rows).  A row whose dy is zero has zero rows in g3, g2 and g1 and adds exact zeros
// to every weight and bias gradient, so the dH and dW GEMMs run over the rows that carry gradient only, compacted to the front of
// copies of their operands.  What keeps the VALUES (up to the sign of a zero):
//   * a dH row depends on its own operand row only (a chain over H in a fixed order): the compact row has the dense row's bits;
//   * a dW element is ONE fmaf chain over the rows in the order gemm_rs_kernel visits them: (K-tile t, b, s, half) with row
//     k = 32 t + 16 half + 4 b + s, i.e. visit rank 2 (4 b + s) + half inside a 32-row tile.  Dropping a dead row's exact zero from
//     the chain changes nothing as long as the ORDER of what remains does: the live row the dense chain reaches as its j-th live row
//     goes to the compact position the compact chain visits j-th (live_position);
//   * rows whose layer-1 input is not finite (a cloud the encoder's 0/0 turned to NaN) give NaN * 0 = NaN in the dense
//     dW1: they count as live (from the encoder's ssq sums of the row's two clouds or, without them, a pass over the rows of X);
//   * positions L .. Lp (L rounded up to whole K-tiles) are zero rows in every copy.
// Rank of local row i (0..31) among the rows of its 32-row tile in visit order: the rows visited before it, as a mask over local rows
__device__ __forceinline__ unsigned live_before_mask(int i) {
    const int w = i & 15, h = i >> 4;
    return ((1u << w) - 1u) * 0x10001u | (h ? (1u << w) : 0u);
}
// compact position that the chain visits j-th, and the inverse: the visit rank of position p
__device__ __forceinline__ int live_position(int j) { return (j & ~31) + 16 * (j & 1) + ((j & 31) >> 1); }
__device__ __forceinline__ int live_rank(int p) { return (p & ~31) + 2 * (p & 15) + ((p >> 4) & 1); }

constexpr int kLiveMaxBlocks = 2048;     // 32-row tiles whose masks one workgroup keeps in LDS: Qb <= 65536
constexpr int kLiveMaxClouds = 1024;

struct LiveArgs {
    const float* dy;            // [Qb,3]
    const float* ssq;           // [clouds][kMfvSlices][20] or NULL
    const int32_t* rowflag;     // [Qb] (non-zero: the row's X is not finite) or NULL
    const float* g3; const float* h1; const float* h2; const float* X;
    int32_t* cnt; int32_t* idx; int32_t* pos;
    float* g3c; float* h1c; float* h2c; float* Xc;
    int Qb, H, KP, ldx, clouds, rows_per_cloud;
};

__device__ __forceinline__ bool not_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }

// rowflag[r] = the row X[r][0 .. KP) holds a value that is not finite; one wave per row
__global__ __launch_bounds__(256) void live_rowflag_kernel(const float* __restrict__ X, int ldx, int KP, int Qb, int32_t* __restrict__ flag) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= Qb) return;
    const float4* x = reinterpret_cast<const float4*>(X + (size_t)r * ldx);
    bool bad = false;
    for (int i = lane; i < KP / 4; i += 64) {
        const float4 v = x[i];
        bad = bad || not_finite(v.x) || not_finite(v.y) || not_finite(v.z) || not_finite(v.w);
    }
    const bool any = __ballot(bad) != 0ull;
    if (lane == 0) flag[r] = any ? 1 : 0;
}

// Every workgroup derives the whole index itself (liveness of all Qb rows, live rows per 32-row tile, their prefix sum: no ticket, no
// wait between workgroups).  It then writes pos[] of its contiguous share of the rows and fills the compact positions p = blockIdx.x,
// + gridDim.x, ... < Lp -- an even share of the LIVE rows whatever their spread: the row of a position comes from a search in the prefix
// sums -- with the row's copies, or with zeros for the pad positions.  Qb % 32 == 0, H % 4 == 0, KP % 4 == 0, ldx % 4 == 0.
__global__ __launch_bounds__(256) void live_compact_kernel(LiveArgs a) {
    __shared__ unsigned s_mask[kLiveMaxBlocks];
    __shared__ int s_pref[kLiveMaxBlocks + 1];
    __shared__ int s_cloud[kLiveMaxClouds];
    const int tid = threadIdx.x, lane = tid & 63;
    const int Qb = a.Qb, nblk = Qb >> 5;
    if (a.ssq) {
        for (int c = tid; c < a.clouds; c += 256) s_cloud[c] = 0;
        __syncthreads();
        const int per = kMfvSlices * 20;
        for (int e = tid; e < a.clouds * per; e += 256)
            if (not_finite(a.ssq[e])) s_cloud[e / per] = 1;      // (every writer stores the same value)
        __syncthreads();
    }
    for (int r0 = 0; r0 < Qb; r0 += 4 * 256) {      // four rows per thread and trip: their twelve loads in flight together
        float d[4][3];
        int fl[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int r = min(r0 + 256 * u + tid, Qb - 1);
#pragma unroll
            for (int c = 0; c < 3; ++c) d[u][c] = a.dy[3 * (size_t)r + c];
            fl[u] = a.rowflag ? a.rowflag[r] : 0;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int r = r0 + 256 * u + tid;
            bool live = false;
            if (r < Qb) {
                live = !(d[u][0] == 0.f && d[u][1] == 0.f && d[u][2] == 0.f) || fl[u] != 0;      // (a NaN compares unequal: live)
                if (a.ssq) {      // the cloud whose Fisher vectors the row gathers and the cloud its query point belongs to
                    const int c = min(r / a.rows_per_cloud, a.clouds - 1), c2 = (c + a.clouds / 2) % a.clouds;
                    live = live || (s_cloud[c] | s_cloud[c2]) != 0;
                }
            }
            const unsigned long long b = __ballot(live);
            if ((lane & 31) == 0 && r < Qb) s_mask[r >> 5] = (unsigned)(b >> (lane & 32));
        }
    }
    __syncthreads();
    if (tid < 64) {      // exclusive prefix sum of the live rows per tile: one wave, 64 tiles per trip
        int carry = 0;
        for (int b0 = 0; b0 < nblk; b0 += 64) {
            const int b = b0 + tid;
            const int v = b < nblk ? __popc(s_mask[b]) : 0;
            int inc = v;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int t = __shfl_up(inc, o, 64);
                if (tid >= o) inc += t;
            }
            if (b < nblk) s_pref[b] = carry + inc - v;
            carry += __shfl(inc, 63, 64);
        }
        if (tid == 0) s_pref[nblk] = carry;
    }
    __syncthreads();
    const int L = s_pref[nblk], Lp = (L + 31) & ~31;      // (L <= Qb and Qb % 32 == 0: Lp <= Qb)
    if (blockIdx.x == 0 && tid == 0) { a.cnt[0] = L; a.cnt[1] = Lp; a.cnt[2] = 0; a.cnt[3] = 0; }
    const int per = (Qb + gridDim.x - 1) / gridDim.x;
    for (int r = blockIdx.x * per + tid; r < min(Qb, (int)(blockIdx.x + 1) * per); r += 256) {
        const unsigned m = s_mask[r >> 5];
        const int i = r & 31;
        a.pos[r] = ((m >> i) & 1u) ? live_position(s_pref[r >> 5] + __popc(m & live_before_mask(i))) : -1;
    }
    const int H4 = a.H / 4, KP4 = a.KP / 4;
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int p = blockIdx.x; p < Lp; p += gridDim.x) {      // (everything up to the copies is uniform over the workgroup)
        const int j = live_rank(p);
        float4* dg = reinterpret_cast<float4*>(a.g3c + (size_t)p * a.H);
        float4* d1 = reinterpret_cast<float4*>(a.h1c + (size_t)p * a.H);
        float4* d2 = reinterpret_cast<float4*>(a.h2c + (size_t)p * a.H);
        float4* dx = reinterpret_cast<float4*>(a.Xc + (size_t)p * a.KP);
        if (j >= L) {      // pad position: zero rows, idx on a valid row
            if (tid == 0) a.idx[p] = 0;
            for (int e = tid; e < H4; e += 256) { dg[e] = z4; d1[e] = z4; d2[e] = z4; }
            for (int e = tid; e < KP4; e += 256) dx[e] = z4;
            continue;
        }
        int lo = 0, hi = nblk - 1;      // the tile of the j-th live row: the last one with s_pref <= j (it holds more than j - s_pref rows)
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (s_pref[mid] <= j) lo = mid; else hi = mid - 1;
        }
        const unsigned m = s_mask[lo];
        const int n = j - s_pref[lo];
        int i = 0;
        for (int c = 0; c < 32; ++c)
            if (((m >> c) & 1u) && __popc(m & live_before_mask(c)) == n) i = c;
        const int r = 32 * lo + i;
        if (tid == 0) a.idx[p] = r;
        const float4* sg = reinterpret_cast<const float4*>(a.g3 + (size_t)r * a.H);
        const float4* s1 = reinterpret_cast<const float4*>(a.h1 + (size_t)r * a.H);
        const float4* s2 = reinterpret_cast<const float4*>(a.h2 + (size_t)r * a.H);
        const float4* sx = reinterpret_cast<const float4*>(a.X + (size_t)r * a.ldx);
        for (int e = tid; e < H4; e += 256) { dg[e] = sg[e]; d1[e] = s1[e]; d2[e] = s2[e]; }
        for (int e = tid; e < KP4; e += 256) dx[e] = sx[e];
    }
}

// The 32-row partial column sums the dense dH epilogue stores for db2 / db1 (put_tile: per half of the wave the tile's 16 rows in
// register order, then half 0 + half 1), rebuilt from the compact rows: block = ORIGINAL 32-row tile, dead rows (exact zeros in the
// dense sum) left out.  grid (Qb / 32, ceil(H / 256), layers); gc[z] / out[z] = NULL: layer not wanted.
struct LivePartArgs {
    const float* gc[2];
    float* out[2];
    const int32_t* pos; const int32_t* cnt;
    int Qb, H;
};
__global__ __launch_bounds__(256) void live_db_partials_kernel(LivePartArgs a) {
    __shared__ int s_pos[32];
    const float* gc = a.gc[blockIdx.z];
    float* out = a.out[blockIdx.z];
    if (!gc || !out) return;
    const int tid = threadIdx.x, blk = blockIdx.x;
    if (tid < 32) {
        const int lp = min(a.cnt[1], a.Qb), p = a.pos[blk * 32 + tid];
        s_pos[tid] = (p >= 0 && p < lp) ? p : -1;      // (a wrong word must not move an address out of the buffer)
    }
    __syncthreads();
    const int col = blockIdx.y * 256 + tid;
    if (col >= a.H) return;
    float cs[2], x[2][16];
    bool live[2][16];
#pragma unroll
    for (int half = 0; half < 2; ++half) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int p = s_pos[(r & 3) + 8 * (r >> 2) + 4 * half];
            x[half][r] = gc[(size_t)max(p, 0) * a.H + col];      // (all 32 loads in flight; a dead row reads row 0 and is not added)
            live[half][r] = p >= 0;
        }
    }
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        float c = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) c = live[half][r] ? c + x[half][r] : c;
        cs[half] = c;
    }
    out[(size_t)blk * a.H + col] = cs[0] + cs[1];
}

}  // namespace dpd

extern "C" int dpd_set_gemm_plan(int op, int tile, int split_k) {
    if (op == 8) {      // layer 1 over distinct windows: the two 32-row wave tiles (same bits)
        if (tile != 32 && tile != 33) return DPD_E_DIM;
        dpd::g_l1u_tile = tile;
        return 0;
    }
    if (op >= 9 && op <= 12) {      // live-row backward: dH, dW1, dW2 + dW3, the dW part of a pair launch (same bits on either tile)
        if (tile != 32 && tile != 33) return DPD_E_DIM;
        dpd::g_live_tile[op - 9] = tile;
        return 0;
    }
    // plane GEMMs: ops 16.. = call sites, 32 = the grouped dW2 + dW3 launch; split_k: n > 1 in-launch reduction, n < -1 slabs + reduce
    // launch, 1 off, 0 automatic (decoder.hip: g_x3_split)
    if (op >= 16 && op < 16 + dpd::OP_COUNT && tile >= 0 && tile <= 26 && split_k >= -8 && split_k <= 8) {
        dpd::g_x3_tile[op - 16] = tile;
        if (op - 16 == dpd::OP_BWD_DW1 || op - 16 == dpd::OP_BWD_DW23) dpd::g_x3_split[op - 16] = split_k;
        return 0;
    }
    if (op == 32 && tile >= 0 && tile <= 16 && split_k >= -4 && split_k <= 4) { dpd::g_x3_pair_tile = tile; dpd::g_x3_pair_split = split_k; return 0; }
    if (op == 33 && tile >= 0 && tile <= 16 && split_k >= 1 && split_k <= 4) { dpd::g_x3_trio_tile = tile; dpd::g_x3_trio_split = split_k; return 0; }
    if (op < 0 || op >= dpd::OP_COUNT || tile < 0 || tile > 33 || split_k < 0 || split_k > 8) return DPD_E_DIM;
    dpd::g_plan_tile[op] = tile;
    dpd::g_plan_split[op] = split_k;
    return 0;
}

static size_t base_ws_bytes(int KP, int H) {
    const size_t slabs = (size_t)8 * (size_t)(KP > H ? KP : H) * H * sizeof(float);   // split-K <= 8 of the largest dW
    const size_t cols = dpd::colsum_ws_floats(H, 3) * sizeof(float);
    return (slabs + cols + 255) / 256 * 256 + dpd::kRedCntBytes;
}
// the base workspace when `ws` holds it, else 0
static size_t base_ws_or_0(const void* ws, size_t ws_bytes, int KP, int H) {
    const size_t base = base_ws_bytes(KP, H);
    return (ws && ws_bytes >= base) ? base : 0;
}
// plane scratch = the tail of the workspace
static dpd::Scratch scratch_of(void* ws, size_t ws_bytes, int KP, int H) {
    const size_t base = base_ws_bytes(KP, H);
    if (!ws || ws_bytes <= base) return dpd::Scratch{nullptr, 0};
    return dpd::Scratch{(char*)ws + base, ws_bytes - base};
}

extern "C" size_t dpd_workspace_bytes(int Q, int KP, int H, int dtype) {
    return base_ws_bytes(KP, H) + dpd::plane_bytes(dtype, Q, KP, H);
}

namespace {
struct PlaneSizes {
    size_t X_rc, X_r8, h_rc, h_r8, g, W1, W23;
};
PlaneSizes plane_sizes(int Q, int Qb, int KP, int H, int np) {
    auto al = [](size_t b) { return (b + 255) / 256 * 256; };
    PlaneSizes z;
    z.X_rc = al((size_t)np * 2 * Q * KP); z.X_r8 = al((size_t)np * 2 * Qb * KP);
    z.h_rc = al((size_t)np * 2 * Q * H);  z.h_r8 = al((size_t)np * 2 * Qb * H);
    z.g = al((size_t)np * 2 * Qb * H);
    z.W1 = al((size_t)np * 2 * KP * H);   z.W23 = al((size_t)np * 2 * H * H);
    return z;
}
}  // namespace

extern "C" size_t dpd_planes_bytes(int Q, int Qb, int KP, int H, int dtype, int with_dx) {
    if (dtype != 1 && dtype != 2) return 0;
    const PlaneSizes z = plane_sizes(Q, Qb, KP, H, dtype == 1 ? 3 : 1);
    return z.X_rc + z.X_r8 + 2 * (z.h_rc + z.h_r8) + (with_dx ? 6 : 5) * z.g + (with_dx ? 2 : 1) * z.W1 + 4 * z.W23 + (dtype == 2 ? z.h_rc : 0);
}

extern "C" int dpd_planes_carve(void* mem, size_t bytes, int Q, int Qb, int KP, int H, int dtype, int with_dx, dpd_planes* out) {
    if (!mem || !out) return DPD_E_NULL;
    if (dtype != 1 && dtype != 2) return DPD_E_UNSUPPORTED;
    if (Q <= 0 || Qb <= 0 || Qb > Q || KP <= 0 || H <= 0) return DPD_E_DIM;
    if (bytes < dpd_planes_bytes(Q, Qb, KP, H, dtype, with_dx)) return DPD_E_WORKSPACE;
    const int np = dtype == 1 ? 3 : 1;
    const PlaneSizes z = plane_sizes(Q, Qb, KP, H, np);
    char* c = (char*)mem;
    auto take = [&](size_t n) { void* r = c; c += n; return r; };
    *out = dpd_planes{};
    out->np = np; out->Q = Q; out->Qb = Qb;
    out->X_rc = take(z.X_rc); out->X_r8 = take(z.X_r8);
    out->h1_rc = take(z.h_rc); out->h1_r8 = take(z.h_r8); out->h2_rc = take(z.h_rc); out->h2_r8 = take(z.h_r8);
    out->g3_rc = take(z.g); out->g3_r8 = take(z.g); out->g2_rc = take(z.g); out->g2_r8 = take(z.g); out->g1_r8 = take(z.g);
    out->g1_rc = with_dx ? take(z.g) : nullptr;
    out->W1_r8 = take(z.W1); out->W2_r8 = take(z.W23); out->W3_r8 = take(z.W23);
    out->W2_rc = take(z.W23); out->W3_rc = take(z.W23);
    out->W1_rc = with_dx ? take(z.W1) : nullptr;
    out->h3_rc = (dtype == 2) ? take(z.h_rc) : nullptr;
    return 0;
}

extern "C" int dpd_weights_to_planes(const dpd_decoder_params* p, int KP, int H, const dpd_planes* pl, void* stream) {
    using namespace dpd;
    if (!p || !pl || !p->W1p || !p->W2 || !p->W3) return DPD_E_NULL;
    if (KP <= 0 || H <= 0 || (KP & 7) || (H & 7) || (pl->np != 1 && pl->np != 3)) return DPD_E_UNSUPPORTED;
    SplitJobs jobs{};
    auto add = [&](const float* src, int R, void* rc, void* r8) {
        if (!rc && !r8) return;
        jobs.j[jobs.n++] = SplitJob{src, (uint16_t*)rc, (uint16_t*)r8, (long)R * H, (long)R * H, R, H, H, H, pl->np, 0};
    };
    add(p->W1p, KP, pl->W1_rc, pl->W1_r8);
    add(p->W2, H, pl->W2_rc, pl->W2_r8);
    add(p->W3, H, pl->W3_rc, pl->W3_r8);
    if (!jobs.n) return 0;
    double by = 0.0;
    for (int t = 0; t < jobs.n; ++t) by += (double)jobs.j[t].R * H * (4.0 + pl->np * 2.0 * ((jobs.j[t].rc ? 1 : 0) + (jobs.j[t].r8 ? 1 : 0)));
    StageProf prof(stream, DPD_STAGE_WEIGHT_COPIES, by);
    return split_planes_multi(jobs, (hipStream_t)stream);
}

extern "C" int dpd_weights_transpose(const dpd_decoder_params* p, int KP, int H, float* W2T, float* W3T, float* W1pT, void* stream) {
    using namespace dpd;
    if (!p || !p->W2 || !p->W3 || !W2T || !W3T) return DPD_E_NULL;
    if (W1pT && !p->W1p) return DPD_E_NULL;
    if (KP <= 0 || H <= 0) return DPD_E_DIM;
    TransposeJobs J{};
    auto add = [&](const float* in, float* out, int R, int C) {
        J.in[J.n] = in; J.out[J.n] = out; J.R[J.n] = R; J.C[J.n] = C;
        J.blk0[J.n + 1] = J.blk0[J.n] + ((R + 63) / 64) * ((C + 63) / 64);
        ++J.n;
    };
    add(p->W2, W2T, H, H);
    add(p->W3, W3T, H, H);
    if (W1pT) add(p->W1p, W1pT, KP, H);
    StageProf prof(stream, DPD_STAGE_WEIGHT_COPIES, 8.0 * ((double)2 * H * H + (W1pT ? (double)KP * H : 0.0)));
    DPD_LAUNCH(transpose_kernel, dim3(J.blk0[J.n]), dim3(256), 0, (hipStream_t)stream, J);
    DPD_CHECK_LAUNCH();
    return 0;
}

extern "C" int dpd_decoder_fwd(const float* X, const float* mask, int Q, int KP, int H, const dpd_decoder_params* p,
                               int dtype, float* h1, float* h2, float* h3, float* y, float* pred, void* ws, size_t ws_bytes,
                               const dpd_planes* pl, void* stream) {
    using namespace dpd;
    pl = dpd::usable_planes(pl, dtype, Q, pl ? pl->Qb : 0, KP, H);
    if (!X && !(pl && pl->X_rc)) return DPD_E_NULL;
    // y = pred = NULL: the output layer is left to dpd_decoder_bwd_data (dpd_small_grads.fwd_y).  h1 / h2 = NULL: plane compute
    // types whose planes keep h1_rc / h2_rc need no fp32 copy (the next layer, the weight gradients and the ReLU gate of the backward
    // all read the planes): 2 x Q x H x 4 bytes less to write per forward
    // h3 = NULL (DPD_BF16, y = pred = NULL): layer 3 leaves its activation as the bf16 plane pl->h3_rc only
    const bool h3_plane = !h3 && pl && pl->np == 1 && pl->h3_rc && !y;
    if (!mask || !p || (!h3 && !h3_plane) || (!y != !pred)) return DPD_E_NULL;
    if ((!h1 && !(pl && pl->h1_rc)) || (!h2 && !(pl && pl->h2_rc))) return DPD_E_NULL;
    if (pl && (pl->Q != Q || pl->Qb > Q)) return DPD_E_DIM;
    if (int rc = dpd::check_planes(pl, dtype)) return rc;
    if (!p->W1p || !p->b1 || !p->W2 || !p->b2 || !p->W3 || !p->b3 || !p->W4 || !p->b4) return DPD_E_NULL;
    if (Q <= 0 || KP <= 0 || H <= 0) return DPD_E_DIM;
    if ((H & 63) || (KP & 3) || dtype < 0 || dtype > 2) return DPD_E_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    const Scratch scr = scratch_of(ws, ws_bytes, KP, H);
    // layer 1..3: h = relu(in W + b)   (tf_util.conv2d: conv2d + bias_add + relu, utils/tf_util.py:213-227)
    GemmDtCall l1, l2, l3;
    for (GemmDtCall* c : {&l1, &l2, &l3}) {
        c->dtype = dtype; c->op = OP_FWD_L23; c->M = Q; c->N = H; c->K = H; c->lda = H; c->ldb = H; c->ldc = H;
        c->epilogue = EPI_BIAS_RELU; c->scr = scr; c->s = s;
    }
    l1.op = OP_FWD_L1; l1.K = KP; l1.lda = KP;
    l1.A = X; l1.B = p->W1p; l1.bias = p->b1; l1.C = h1;
    l2.A = h1; l2.B = p->W2; l2.bias = p->b2; l2.C = h2;
    l3.A = h2; l3.B = p->W3; l3.bias = p->b3; l3.C = h3;
    if (pl) {   // operands from / results to the persistent planes (no conversion passes)
        l1.Apl = pl->X_rc; l1.Bpl = pl->W1_r8; l1.out = make_out(pl, pl->h1_rc, Q, pl->h1_r8, pl->Qb, H);
        l2.Apl = pl->h1_rc; l2.Bpl = pl->W2_r8; l2.out = make_out(pl, pl->h2_rc, Q, pl->h2_r8, pl->Qb, H);
        l3.Apl = pl->h2_rc; l3.Bpl = pl->W3_r8;
        if (h3_plane) l3.out = make_out(pl, pl->h3_rc, Q, nullptr, 0, H);
    } else if (dtype != 0 && !scr.p) {
        return DPD_E_WORKSPACE;
    }
    for (const GemmDtCall* c : {&l1, &l2, &l3})
        if (int rc = gemm_dt(*c)) return rc;
    if (!y) return 0;
    DPD_LAUNCH(out_fwd_kernel, dim3((Q + 3) / 4), dim3(256), 0, s, h3, p->W4, p->b4, mask, y, pred, Q, H);
    DPD_CHECK_LAUNCH();
    return 0;
}

// Layer 1 over `cap` slots of Xu (k-major, row stride lda; the live count is the device word *m_dev) and its finish launch, layers 2 and 3,
// the output layer: the launches of dpd_decoder_fwd_unique and dpd_decoder_fwd_cross
static int fwd_over_slots(const float* Xu, int lda, int cap, const float* Xt, const int32_t* uid, const int32_t* m_dev, float* Pu, const float* mask,
                          int Q, int KP, int H, const dpd_decoder_params* p, float* h1, float* h2, float* h3, float* y, float* pred,
                          hipStream_t s, bool prof_stages) {
    using namespace dpd;
    // layer 1, first step: Pu [cap, H] = XuT^T W1p[0 : KP - 32] over the live slots (raw accumulators); XuT is k-major
    GemmF32Call f;
    f.transA = 1; f.M = cap; f.N = H; f.K = KP - 32;
    f.A = Xu; f.lda = lda; f.B = p->W1p; f.ldb = H; f.C = Pu; f.ldc = H;
    f.epilogue = EPI_NONE; f.split_k = 1; f.tile = g_l1u_tile; f.s = s; f.M_dev = m_dev;
    if (int rc = gemm_f32(f)) return rc;
    // second step: the last K-tile, bias and ReLU per row
    {
        // (prof_stages: the all-pairs engine brackets the two launches that are no GEMM; bytes: Pu rows, Xt, uid in, h1 out)
        StageProf prof(s, DPD_STAGE_L1_FINISH, (double)Q * (2.0 * H + 33.0) * 4.0, prof_stages);
        DPD_LAUNCH(l1_finish_kernel, dim3(((Q / 32) * (H / 32) + 3) / 4), dim3(256), 0, s, (const float*)Pu, uid, Xt,
                   p->W1p + (size_t)(KP - 32) * H, p->b1, h1, Q, H);
        DPD_CHECK_LAUNCH();
    }
    GemmDtCall l2, l3;
    for (GemmDtCall* c : {&l2, &l3}) {
        c->dtype = 0; c->op = OP_FWD_L23; c->M = Q; c->N = H; c->K = H; c->lda = H; c->ldb = H; c->ldc = H;
        c->epilogue = EPI_BIAS_RELU; c->s = s;
    }
    l2.A = h1; l2.B = p->W2; l2.bias = p->b2; l2.C = h2;
    l3.A = h2; l3.B = p->W3; l3.bias = p->b3; l3.C = h3;
    for (const GemmDtCall* c : {&l2, &l3})
        if (int rc = gemm_dt(*c)) return rc;
    if (!y) return 0;
    StageProf prof(s, DPD_STAGE_OUT_LAYER, (double)Q * (H + 7.0) * 4.0, prof_stages);
    DPD_LAUNCH(out_fwd_kernel, dim3((Q + 3) / 4), dim3(256), 0, s, h3, p->W4, p->b4, mask, y, pred, Q, H);
    DPD_CHECK_LAUNCH();
    return 0;
}

extern "C" int dpd_decoder_fwd_unique(const float* Xu /* k-major */, const float* Xt, const int32_t* uid, const int32_t* cnt, float* Pu, const float* mask,
                                      int Q, int KP, int H, const dpd_decoder_params* p, float* h1, float* h2, float* h3, float* y,
                                      float* pred, void* stream) {
    if (!Xu || !Xt || !uid || !cnt || !Pu || !mask || !p || !h1 || !h2 || !h3 || (!y != !pred)) return DPD_E_NULL;
    if (!p->W1p || !p->b1 || !p->W2 || !p->b2 || !p->W3 || !p->b3 || !p->W4 || !p->b4) return DPD_E_NULL;
    if (Q <= 0 || KP <= 0 || H <= 0) return DPD_E_DIM;
    if ((H & 63) || (KP & 31) || KP < 64 || (Q & 31)) return DPD_E_UNSUPPORTED;
    return fwd_over_slots(Xu, Q + 32, Q + 32, Xt, uid, cnt + 1, Pu, mask, Q, KP, H, p, h1, h2, h3, y, pred, (hipStream_t)stream, false);
}

// qcounts = NULL: dpd_decoder_fwd_cross; otherwise the pair means over each query cloud's own count (pairs = surface clouds x Cb)
static int fwd_cross(const float* Xu /* k-major */, int ldu, int slot_cap, const float* Xt, const int32_t* uid, const int32_t* cnt, float* Pu,
                     const float* maskr, const int32_t* qcounts, int pairs, int Cb, int N, int KP, int H, const dpd_decoder_params* p,
                     float* act0, float* act1, float* y, float* pred, float* Dd, void* stream) {
    using namespace dpd;
    if (!p->W1p || !p->b1 || !p->W2 || !p->b2 || !p->W3 || !p->b3 || !p->W4 || !p->b4) return DPD_E_NULL;
    if (pairs <= 0 || N <= 0 || KP <= 0 || H <= 0 || slot_cap <= 0 || ldu < slot_cap || (long)pairs * N > (1L << 30)) return DPD_E_DIM;
    if (qcounts && (Cb <= 0 || pairs % Cb)) return DPD_E_DIM;
    if ((H & 63) || (KP & 31) || KP < 64 || (slot_cap & 3) || (ldu & 3)) return DPD_E_UNSUPPORTED;
    const int Q = (pairs * N + 31) / 32 * 32;       // the rows and their pad rows
    // (the GEMMs address Xu, Pu and the activations with 32-bit byte offsets)
    if (!fits_gemm_offsets((size_t)(KP - 32), (size_t)ldu) || !fits_gemm_offsets((size_t)slot_cap, (size_t)H) || !fits_gemm_offsets((size_t)Q, (size_t)H))
        return DPD_E_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    // h1 -> act0, h2 -> act1, h3 -> act0: nothing is kept for a backward pass
    if (int rc = fwd_over_slots(Xu, ldu, slot_cap, Xt, uid, cnt + 1, Pu, maskr, Q, KP, H, p, act0, act1, act0, y, pred, s, true)) return rc;
    StageProf prof(stream, DPD_STAGE_SMALL_REDUCE, (double)pairs * N * 12.0 + pairs * 4.0);
    if (qcounts)
        DPD_LAUNCH(pair_mean_counts_kernel, dim3((pairs + 3) / 4), dim3(256), 0, s, (const float*)pred, qcounts, N, pairs, Cb, Dd);
    else
        DPD_LAUNCH(pair_mean_kernel, dim3((pairs + 3) / 4), dim3(256), 0, s, (const float*)pred, N, pairs, Dd);
    DPD_CHECK_LAUNCH();
    return 0;
}

extern "C" int dpd_decoder_fwd_cross(const float* Xu /* k-major */, int ldu, int slot_cap, const float* Xt, const int32_t* uid, const int32_t* cnt,
                                     float* Pu, const float* maskr, int pairs, int N, int KP, int H, const dpd_decoder_params* p, float* act0,
                                     float* act1, float* y, float* pred, float* Dd, void* stream) {
    if (!Xu || !Xt || !uid || !cnt || !Pu || !maskr || !p || !act0 || !act1 || !y || !pred || !Dd) return DPD_E_NULL;
    return fwd_cross(Xu, ldu, slot_cap, Xt, uid, cnt, Pu, maskr, nullptr, pairs, 0, N, KP, H, p, act0, act1, y, pred, Dd, stream);
}

extern "C" int dpd_decoder_fwd_cross_counts(const float* Xu /* k-major */, int ldu, int slot_cap, const float* Xt, const int32_t* uid,
                                            const int32_t* cnt, float* Pu, const float* maskr, const int32_t* qcounts, int pairs, int Cb, int N,
                                            int KP, int H, const dpd_decoder_params* p, float* act0, float* act1, float* y, float* pred,
                                            float* Dd, void* stream) {
    if (!Xu || !Xt || !uid || !cnt || !Pu || !maskr || !qcounts || !p || !act0 || !act1 || !y || !pred || !Dd) return DPD_E_NULL;
    return fwd_cross(Xu, ldu, slot_cap, Xt, uid, cnt, Pu, maskr, qcounts, pairs, Cb, N, KP, H, p, act0, act1, y, pred, Dd, stream);
}

// dpd_decoder_fwd_cross with the three activations kept for dpd_cross_bwd: the same launches on the same operands, so the same bits
extern "C" int dpd_decoder_fwd_cross_keep(const float* Xu /* k-major */, int ldu, int slot_cap, const float* Xt, const int32_t* uid,
                                          const int32_t* cnt, float* Pu, const float* maskr, int pairs, int N, int KP, int H,
                                          const dpd_decoder_params* p, float* h1, float* h2, float* h3, float* y, float* pred, float* Dd,
                                          void* stream) {
    using namespace dpd;
    if (!Xu || !Xt || !uid || !cnt || !Pu || !maskr || !p || !h1 || !h2 || !h3 || !y || !pred) return DPD_E_NULL;      // (Dd = NULL: no pair means)
    if (h1 == h2 || h2 == h3 || h1 == h3) return DPD_E_DIM;
    if (!p->W1p || !p->b1 || !p->W2 || !p->b2 || !p->W3 || !p->b3 || !p->W4 || !p->b4) return DPD_E_NULL;
    if (pairs <= 0 || N <= 0 || KP <= 0 || H <= 0 || slot_cap <= 0 || ldu < slot_cap || (long)pairs * N > (1L << 30)) return DPD_E_DIM;
    if ((H & 63) || (KP & 31) || KP < 64 || (slot_cap & 3) || (ldu & 3)) return DPD_E_UNSUPPORTED;
    const int Q = (pairs * N + 31) / 32 * 32;
    if (!fits_gemm_offsets((size_t)(KP - 32), (size_t)ldu) || !fits_gemm_offsets((size_t)slot_cap, (size_t)H) || !fits_gemm_offsets((size_t)Q, (size_t)H))
        return DPD_E_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    if (int rc = fwd_over_slots(Xu, ldu, slot_cap, Xt, uid, cnt + 1, Pu, maskr, Q, KP, H, p, h1, h2, h3, y, pred, s, true)) return rc;
    if (!Dd) return 0;
    StageProf prof(stream, DPD_STAGE_SMALL_REDUCE, (double)pairs * N * 12.0 + pairs * 4.0);
    DPD_LAUNCH(pair_mean_kernel, dim3((pairs + 3) / 4), dim3(256), 0, s, (const float*)pred, N, pairs, Dd);
    DPD_CHECK_LAUNCH();
    return 0;
}

extern "C" int dpd_decoder_out_asloss(const float* h3, const float* mask, int Q, int H, int BN, const dpd_decoder_params* p, float gscale,
                                      float* y, float* pred, float* loss_pred, float* dy, float* g3, float* scratch, void* stream) {
    return dpd_decoder_out_asloss_planes(h3, mask, Q, H, BN, p, gscale, y, pred, loss_pred, dy, g3, nullptr, scratch, stream);
}

extern "C" int dpd_decoder_out_asloss_planes(const float* h3, const float* mask, int Q, int H, int BN, const dpd_decoder_params* p, float gscale,
                                             float* y, float* pred, float* loss_pred, float* dy, float* g3, const dpd_planes* pl, float* scratch,
                                             void* stream) {
    using namespace dpd;
    if (!h3 || !mask || !p || !p->W4 || !p->b4 || !y || !pred || !loss_pred || !scratch) return DPD_E_NULL;
    // pl with g3_rc (and dy given): g3 also (or, with g3 == NULL, only) as RC operand plane(s); needs the 16-byte fast path of the row kernel
    uint16_t* g3_rc = (pl && dy) ? (uint16_t*)pl->g3_rc : nullptr;
    if (g3_rc && (pl->Qb != Q || (pl->np != 1 && pl->np != 3) || (H & 255) || H > 256 * kOutMaxI || ((uintptr_t)p->W4 & 15) || ((uintptr_t)h3 & 15)))
        return DPD_E_UNSUPPORTED;
    if (dy && !g3 && !g3_rc) return DPD_E_NULL;
    if (!dy && g3) return DPD_E_NULL;
    if (Q <= 0 || H <= 0 || BN <= 0 || Q != 2 * BN) return DPD_E_DIM;
    if ((H & 3) || ((uintptr_t)scratch & 7) || Q > 8 * 65535 || BN >= (1 << 14)) return DPD_E_UNSUPPORTED;   // 16-bit block count; 48-bit sum: Q rows x at most 2.0 x 2^32 must stay below 2^48
    const float gv = 0.5f * (1.0f / (float)BN) * gscale;      // = l1_loss_kernel mode 2
    // two rows per wave: 9.9 us against 11.2 (one) and 11.9 (four) at the PCRNet batch -- the kernel is a chain of round trips (rows and
    // W4 -> wave sums -> stores -> the atomic's return), not a throughput problem
    DPD_LAUNCH(out_asloss_kernel<2>, dim3((Q + 7) / 8), dim3(256), 0, (hipStream_t)stream, h3, p->W4, p->b4, mask, y, pred, dy, g3, Q, H, BN, gv,
               loss_pred, (unsigned long long*)scratch, g3_rc, g3_rc ? (long)Q * H : 0L, g3_rc ? pl->np : 0);
    DPD_CHECK_LAUNCH();
    return 0;
}

extern "C" int dpd_decoder_out_pairs(const float* h3, const float* mask, int P, int Wa, int Wb, const int32_t* countsA, const int32_t* countsB,
                                     int H, const dpd_decoder_params* p, float* y, float* pred, float* Dd, float* dy, float* g3, void* stream) {
    using namespace dpd;
    if (!h3 || !mask || !p || !p->W4 || !p->b4 || !y || !pred || !Dd || (!dy != !g3)) return DPD_E_NULL;
    if (P <= 0 || Wa <= 0 || Wb <= 0 || H <= 0 || (long)P * ((long)Wa + Wb) > (1L << 30)) return DPD_E_DIM;
    if (((uintptr_t)h3 & 15) || ((uintptr_t)g3 & 15)) return DPD_E_UNSUPPORTED;      // the rows are read and written 16 bytes per lane
    hipStream_t s = (hipStream_t)stream;
    const long Q = (long)P * ((long)Wa + Wb);
    {
        StageProf prof(stream, DPD_STAGE_OUT_LAYER, (double)Q * H * 4.0 * (g3 ? 2.0 : 1.0) + Q * (dy ? 40.0 : 28.0) + H * 12.0);
        DPD_LAUNCH(out_pairs_kernel, dim3((unsigned)((Q + 3) / 4)), dim3(256), 0, s, h3, p->W4, p->b4, mask, y, pred, dy, g3, P, Wa, Wb, countsA,
                   countsB, H);
        DPD_CHECK_LAUNCH();
    }
    StageProf prof(stream, DPD_STAGE_SMALL_REDUCE, (double)Q * 12.0 + P * 8.0);
    DPD_LAUNCH(pairs_mean_kernel, dim3(2 * P), dim3(256), 0, s, (const float*)pred, P, Wa, Wb, countsA, countsB, Dd);
    DPD_CHECK_LAUNCH();
    return 0;
}

// ---- live rows: host side ----
extern "C" size_t dpd_live_rows_bytes(int Qb, int KP, int H) {
    if (Qb <= 0 || KP <= 0 || H <= 0) return 0;
    const size_t al = 256;
    auto up = [&](size_t b) { return (b + al - 1) / al * al; };
    return up(4 * sizeof(int32_t)) + 3 * up((size_t)Qb * sizeof(int32_t)) + 3 * up((size_t)Qb * H * sizeof(float)) + up((size_t)Qb * KP * sizeof(float));
}
extern "C" int dpd_live_rows_carve(void* mem, size_t bytes, int Qb, int KP, int H, dpd_live_rows* out) {
    if (!mem || !out) return DPD_E_NULL;
    if (Qb <= 0 || KP <= 0 || H <= 0) return DPD_E_DIM;
    if (((uintptr_t)mem & 255) || (Qb & 31) || (H & 3) || (KP & 3)) return DPD_E_UNSUPPORTED;
    if (bytes < dpd_live_rows_bytes(Qb, KP, H)) return DPD_E_WORKSPACE;
    char* c = (char*)mem;
    auto take = [&](size_t b) { char* r = c; c += (b + 255) / 256 * 256; return r; };
    *out = dpd_live_rows{};
    out->Qb = Qb; out->KP = KP; out->H = H;
    out->cnt = (int32_t*)take(4 * sizeof(int32_t));
    out->idx = (int32_t*)take((size_t)Qb * sizeof(int32_t));
    out->pos = (int32_t*)take((size_t)Qb * sizeof(int32_t));
    out->rowflag = (int32_t*)take((size_t)Qb * sizeof(int32_t));
    out->g3c = (float*)take((size_t)Qb * H * sizeof(float));
    out->h1c = (float*)take((size_t)Qb * H * sizeof(float));
    out->h2c = (float*)take((size_t)Qb * H * sizeof(float));
    out->Xc = (float*)take((size_t)Qb * KP * sizeof(float));
    return 0;
}

namespace dpd {
// what every entry checks of a descriptor before a kernel sees it
static int check_live(const dpd_live_rows* lv, int Qb, int KP, int H) {
    if (!lv->cnt || !lv->idx || !lv->pos || !lv->g3c || !lv->h1c || !lv->h2c || !lv->Xc) return DPD_E_NULL;
    if (lv->Qb != Qb || lv->H != H || (KP > 0 && lv->KP != KP)) return DPD_E_DIM;
    if ((Qb & 31) || (H & 3) || (lv->KP & 3) || Qb / 32 > kLiveMaxBlocks) return DPD_E_UNSUPPORTED;
    return 0;
}

// compaction launch (behind the output-layer backward that wrote dy and g3)
static int live_compact(const dpd_live_rows* lv, const float* dy, const float* g3, const float* h1, const float* h2, hipStream_t s) {
    if (!lv->X) return DPD_E_NULL;
    if (lv->ldx < lv->KP || (lv->ldx & 3) || (((uintptr_t)lv->X | (uintptr_t)g3 | (uintptr_t)h1 | (uintptr_t)h2) & 15)) return DPD_E_UNSUPPORTED;
    if (lv->ssq && (lv->clouds <= 0 || (lv->clouds & 1) || lv->clouds > kLiveMaxClouds || lv->rows_per_cloud <= 0 ||
                    (long)lv->clouds / 2 * lv->rows_per_cloud != lv->Qb))
        return DPD_E_DIM;      // the rows are the AB half: one query cloud of rows_per_cloud rows per PAIR of clouds
    const int32_t* rowflag = nullptr;
    if (!lv->ssq) {            // no encoder sums: look at the rows themselves
        if (!lv->rowflag) return DPD_E_NULL;
        DPD_LAUNCH(live_rowflag_kernel, dim3((lv->Qb + 3) / 4), dim3(256), 0, s, lv->X, lv->ldx, lv->KP, lv->Qb, lv->rowflag);
        DPD_CHECK_LAUNCH();
        rowflag = lv->rowflag;
    }
    LiveArgs a{dy, lv->ssq, rowflag, g3, h1, h2, lv->X, lv->cnt, lv->idx, lv->pos, lv->g3c, lv->h1c, lv->h2c, lv->Xc,
               lv->Qb, lv->H, lv->KP, lv->ldx, lv->clouds, lv->rows_per_cloud};
    DPD_LAUNCH(live_compact_kernel, dim3(lv->Qb < 512 ? lv->Qb : 512), dim3(256), 0, s, a);
    DPD_CHECK_LAUNCH();
    return 0;
}

// g (compact rows) = (A W^T) * [gate > 0] over the Lp live rows; WT = the transposed weight copy (NN form)
static int live_dh(const dpd_live_rows* lv, const float* A, const float* WT, float* C, const float* gate, hipStream_t s) {
    GemmF32Call f;
    f.M = lv->Qb; f.N = lv->H; f.K = lv->H;
    f.A = A; f.lda = lv->H; f.B = WT; f.ldb = lv->H; f.C = C; f.ldc = lv->H;
    f.gate = gate; f.epilogue = EPI_GATE; f.tile = g_live_tile[LIVE_DH]; f.s = s; f.M_dev = lv->cnt + 1;
    return gemm_f32(f);
}
}  // namespace dpd

extern "C" int dpd_decoder_bwd_data(const float* dpred, const float* mask, const float* y, const float* h1,
                                    const float* h2, const float* h3, int Qb, int KP, int H, const dpd_decoder_params* p,
                                    int dtype, float* dy, float* g3, float* g2, float* g1, float* dX,
                                    const dpd_small_grads* sg, void* ws, size_t ws_bytes, const dpd_planes* pl, int phases,
                                    void* stream) {
    return dpd_decoder_bwd_data_live(dpred, mask, y, h1, h2, h3, Qb, KP, H, p, dtype, dy, g3, g2, g1, dX, sg, ws, ws_bytes, pl, phases, nullptr, stream);
}

extern "C" int dpd_decoder_bwd_data_live(const float* dpred, const float* mask, const float* y, const float* h1,
                                         const float* h2, const float* h3, int Qb, int KP, int H, const dpd_decoder_params* p,
                                         int dtype, float* dy, float* g3, float* g2, float* g1, float* dX,
                                         const dpd_small_grads* sg, void* ws, size_t ws_bytes, const dpd_planes* pl, int phases,
                                         const dpd_live_rows* live, void* stream) {
    using namespace dpd;
    const bool l1 = sg && sg->l1_labels;        // fused training loss: dpred is derived inside the output-layer kernel
    if (phases <= 0 || phases > 31) return DPD_E_DIM;
    // (phases without 1: the output layer was done before -- an earlier call or dpd_decoder_out_asloss -- and only g3 is read)
    // h3 = NULL: the bf16 plane pl->h3_rc of dpd_decoder_fwd (DPD_BF16; only the fused output-layer kernel reads it: checked below)
    const bool h3_plane = !h3 && pl && pl->np == 1 && pl->h3_rc;
    if (!p || ((phases & 1) && ((!dpred && !l1) || !mask || (!y && !(sg && sg->fwd_y)) || (!h3 && !h3_plane) || !dy))) return DPD_E_NULL;
    if ((!h1 && !(pl && pl->h1_rc)) || (!h2 && !(pl && pl->h2_rc))) return DPD_E_NULL;   // gate from the fp32 activation or its bf16 plane
    // g2 / g1 = NULL: plane compute types whose planes keep g2_rc + g2_r8 (g1_r8, and g1_rc when dX is wanted) need no fp32 copy of
    // the pre-activation gradients either (the next dH GEMM and the weight gradients read the planes; db2 / db1 come out of the
    // epilogue); the block partials then need their own scratch (sg->partials)
    // (phases without 1 -- the as-loss chain behind dpd_decoder_out_asloss -- has no block partials and, without weight gradients to
    //  follow, needs only the RC planes: g2_rc for the next dH GEMM, g1_rc for dX)
    if (!g2 && !(pl && pl->g2_rc && ((pl->g2_r8 && sg && sg->partials) || !(phases & 1)))) return DPD_E_NULL;
    if (!g1 && !(pl && (pl->g1_r8 || pl->g1_rc) && (!dX || pl->g1_rc))) return DPD_E_NULL;
    if (l1 && (!sg->l1_pred || !sg->l1_loss)) return DPD_E_NULL;
    if (!p->W1p || !p->W2 || !p->W3 || !p->W4) return DPD_E_NULL;
    if (Qb <= 0 || KP <= 0 || H <= 0) return DPD_E_DIM;
    if ((H & 63) || (KP & 3) || dtype < 0 || dtype > 2) return DPD_E_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    const Scratch scr = scratch_of(ws, ws_bytes, KP, H);
    pl = usable_planes(pl, dtype, pl ? pl->Q : 0, Qb, KP, H);
    if (pl && pl->Qb != Qb) return DPD_E_DIM;
    if (int rc = check_planes(pl, dtype)) return rc;
    if (dtype != 0 && !pl && !scr.p) return DPD_E_WORKSPACE;
    if (live) {     // exact fp32, fp32 operands, the NN products on the transposed weight copies, bias gradients in the two-step form or none
        if (dtype != 0 || dX || !dy || !g3 || !g2 || !g1 || !h1 || !h2 || !p->W3T || !p->W2T || (phases & 8)) return DPD_E_UNSUPPORTED;
        if (sg && (sg->db1 || sg->db2) && !sg->db_partials) return DPD_E_UNSUPPORTED;
        if (int rc = check_live(live, Qb, KP, H)) return rc;
    }
    float* db1 = sg ? sg->db1 : nullptr;
    float* db2 = sg ? sg->db2 : nullptr;
    float* db3 = sg ? sg->db3 : nullptr;
    float* dW4 = sg ? sg->dW4 : nullptr;
    float* db4 = sg ? sg->db4 : nullptr;
    const int nblk = (Qb + kOBRows - 1) / kOBRows;
    const bool fused4 = H % 256 == 0 && H <= 1024;
    const int rec = fused4 ? 4 * H + kOBRec : 4 * H + 4;          // floats per block record
    const bool fused = (db3 || dW4 || db4 || l1) && H <= 64 * kOBMaxJ && (size_t)nblk * rec <= (size_t)Qb * H;
    if (l1 && !(fused && fused4)) return DPD_E_UNSUPPORTED;       // the caller then uses dpd_l1_loss + dpred
    if ((phases & 1) && h3_plane && !(fused && fused4 && pl)) return DPD_E_UNSUPPORTED;
    const L1Fuse lf{l1 ? sg->l1_pred : nullptr, l1 ? sg->l1_labels : nullptr, l1 ? sg->l1_gscale : 1.0f};
    const bool ofwd = sg && (sg->fwd_y || sg->fwd_pred) && (phases & 1);   // output layer's forward inside the same pass (training step)
    if (ofwd && !(l1 && fused4 && sg->fwd_y && sg->fwd_pred && p->b4)) return DPD_E_UNSUPPORTED;
    const OutFwd ofw{ofwd ? p->b4 : nullptr, ofwd ? sg->fwd_y : nullptr, ofwd ? sg->fwd_pred : nullptr};
    float* lossp = l1 ? sg->l1_loss : nullptr;
    const int nred = (4 * H + 7 + 15) / 16;
    // block partials of db3 / dW4 / db4: by default in g2 (free until the first dH GEMM); a caller that defers their reduction
    // (phases 16 / 8: it then runs beside the dH GEMMs on another stream) must provide sg->partials
    float* part = (sg && sg->partials) ? sg->partials : g2;
    if ((phases & 24) && !(sg && sg->partials)) return DPD_E_NULL;
    // g3 = NULL: only when the fused output-layer kernel writes g3 as operand planes itself (plane compute types, below)
    bool g3_planes_done = false;
    // (phases without 1 and no fp32 g3: dpd_decoder_out_asloss_planes has left g3 as the RC plane the first dH GEMM reads)
    if (!g3 && !(pl && pl->g3_rc && ((pl->g3_r8 && fused && fused4 && !(Qb % kOBRows)) || !(phases & 1)))) return DPD_E_NULL;
    if ((phases & 8) && fused) {   // deferred second stage of the small gradients (a side stream / graph branch runs it)
        DPD_LAUNCH(small_grads_reduce, dim3(nred), dim3(256), 0, s, (const float*)part, nblk, H, db3, dW4, db4, rec, lossp, Qb);
        DPD_CHECK_LAUNCH();
    }
    if (!(phases & 1)) {
        // output layer already done by an earlier call
    } else if (fused) {
        // one pass over h3: dy, g3 and block partials of db3 / dW4 / db4 (g2 is free until the first dH GEMM: scratch)
        ZeroList zl{{db1, db2, nullptr, nullptr, nullptr}, {H, H, 0, 0, 0}};
        if (fused4) {
            // plane compute types: g3 leaves this kernel as the operand planes of the first dH GEMM (RC) and of dW3 (R8)
            G3Planes gpl{nullptr, nullptr, (long)Qb * H, pl ? pl->np : 0};
            if (pl && !(Qb % kOBRows)) { gpl.rc = (uint16_t*)pl->g3_rc; gpl.r8 = (uint16_t*)pl->g3_r8; }
            g3_planes_done = gpl.rc || gpl.r8;
            const size_t lds = (size_t)4 * rec * sizeof(float);      // (the R8 image of g3, np * 8 * H * 2 bytes, reuses the slabs)
            static LdsOptIn lds_opt;
            if (int rc = ensure_dyn_lds(lds_opt, (const void*)out_bwd_fused4_kernel, lds)) return rc;
            // algorithmic bytes: layer 3's activation in (the Qb gradient rows, and their Qb twins when the layer's forward runs here
            // too; fp32 or one bf16 plane), g3 out (fp32 or both operand planes), the block partials, mask / labels / y / pred
            const double h3_b = h3 ? 4.0 : 2.0;
            StageProf prof(stream, DPD_STAGE_OUT_LAYER,
                           (double)Qb * H * h3_b * (ofwd ? 2.0 : 1.0) + (g3 ? (double)Qb * H * 4.0 : 0.0) +
                               ((gpl.rc ? 1.0 : 0.0) + (gpl.r8 ? 1.0 : 0.0)) * gpl.np * 2.0 * Qb * H + (double)nblk * rec * 4.0 + Qb * 40.0 + H * 12.0);
            DPD_LAUNCH(out_bwd_fused4_kernel, dim3(nblk), dim3(256), lds, s, dpred, mask, y, h3, p->W4, dy, g3, Qb, H, zl, part, lf, ofw, gpl,
                       h3 ? nullptr : (const uint16_t*)pl->h3_rc);
        } else {
            DPD_LAUNCH(out_bwd_fused_kernel, dim3(nblk), dim3(256), (size_t)(4 * H + 4) * sizeof(float), s, dpred, mask, y, h3,
                       p->W4, dy, g3, Qb, H, zl, part);
        }
        DPD_CHECK_LAUNCH();
        if (!(phases & 16)) {   // 16: the block partials stay in the scratch (= g2, which must not be overwritten before phase 8 ran)
            StageProf prof(stream, DPD_STAGE_SMALL_REDUCE, (double)nblk * rec * 4.0 + (4.0 * H + 3) * 4.0);
            DPD_LAUNCH(small_grads_reduce, dim3(nred), dim3(256), 0, s, (const float*)part, nblk, H, db3, dW4, db4, rec, lossp, Qb);
            DPD_CHECK_LAUNCH();
        }
    } else {
        ZeroList zl{{db1, db2, db3, dW4, db4}, {H, H, H, H * 3, 3}};
        DPD_LAUNCH(out_bwd_kernel, dim3((Qb + 3) / 4), dim3(256), 0, s, dpred, mask, y, h3, p->W4, dy, g3, Qb, H, zl);
        DPD_CHECK_LAUNCH();
        const int chunks = 16;
        if (db3) {   // db3 = colsum(g3)
            DPD_LAUNCH(colsum_atomic<0>, dim3((H + 63) / 64, chunks), dim3(256), 0, s, (const float*)g3, H, (const float*)nullptr, Qb,
                       H, db3, (float*)nullptr);
            DPD_CHECK_LAUNCH();
        }
        if (dW4) {   // dW4 = h3^T dy, db4 = colsum(dy)
            DPD_LAUNCH(colsum_atomic<3>, dim3((H + 63) / 64, chunks), dim3(256), 0, s, h3, H, (const float*)dy, Qb, H, dW4, db4);
            DPD_CHECK_LAUNCH();
        }
    }
    if (live) {
        // The rows that carry gradient only (see live_compact_kernel): compaction behind the output layer, the two dH products over
        // the Lp live rows of the compact copies -- g2 / g1 then hold COMPACT rows -- and ONE launch for the 32-row partial sums of
        // db2 / db1 in the dense association (a compact tile mixes the original tiles: its epilogue cannot produce them)
        if (phases & 1)
            if (int rc = live_compact(live, dy, g3, h1, h2, s)) return rc;
        if (phases & 2)
            if (int rc = live_dh(live, live->g3c, p->W3T, g2, live->h2c, s)) return rc;
        if (phases & 4)
            if (int rc = live_dh(live, g2, p->W2T, g1, live->h1c, s)) return rc;
        float* dbp = sg ? sg->db_partials : nullptr;
        if (dbp && (phases & 6)) {
            const int nb = Qb / 32;
            LivePartArgs a{{(phases & 2) ? g2 : nullptr, (phases & 4) ? g1 : nullptr}, {dbp, dbp + (size_t)nb * H}, live->pos, live->cnt, Qb, H};
            DPD_LAUNCH(live_db_partials_kernel, dim3(nb, (H + 255) / 256, 2), dim3(256), 0, s, a);
            DPD_CHECK_LAUNCH();
        }
        return 0;
    }
    // g2 = (g3 W3^T) * [h2 > 0] ;  g1 = (g2 W2^T) * [h1 > 0];  db2 / db1 = column sums, fused into the epilogue;
    // as-loss mode: gradient w.r.t. the gathered rows, dX = g1 W1p^T  [Qb,KP]
    GemmDtCall d3, d2, dx;
    for (GemmDtCall* c : {&d3, &d2, &dx}) {
        c->dtype = dtype; c->op = OP_BWD_DH; c->transB = 1; c->M = Qb; c->N = H; c->K = H; c->lda = H; c->ldb = H; c->ldc = H;
        c->epilogue = EPI_GATE; c->scr = scr; c->s = s;
    }
    d3.A = g3; d3.B = p->W3; d3.C = g2; d3.gate = h2; d3.colsum = db2;
    d2.A = g2; d2.B = p->W2; d2.C = g1; d2.gate = h1; d2.colsum = db1;
    dx.op = OP_BWD_DX; dx.N = KP; dx.ldc = KP; dx.epilogue = EPI_NONE;
    dx.A = g1; dx.B = p->W1p; dx.C = dX;
    ColsumTwoStep c2{}, c1{};
    if (pl) {
        // g3 from a kernel that wrote no planes (this call's unfused output layer, or -- phases without 1 and an fp32 g3 given --
        // dpd_decoder_out_asloss): one conversion launch for the layouts the planes keep
        if ((((phases & 1) && !g3_planes_done) || (!(phases & 1) && g3 && (phases & 2))) && (pl->g3_rc || pl->g3_r8)) {
            if (!g3) return DPD_E_NULL;
            if (int rc = split_planes(g3, Qb, H, H, pl->np, (uint16_t*)pl->g3_rc, H, (long)Qb * H, (uint16_t*)pl->g3_r8, (long)Qb * H, s))
                return rc;
        }
        // the ReLU gate from the fp32 activation or, without one, from its bf16 plane
        d3.Apl = pl->g3_rc; d3.Bpl = pl->W3_rc; d3.out = make_out(pl, pl->g2_rc, Qb, pl->g2_r8, Qb, H);
        d3.gate16 = h2 ? nullptr : (pl->h2_r8 ? pl->h2_r8 : pl->h2_rc); d3.gate16_r8 = pl->h2_r8 != nullptr;
        d2.Apl = pl->g2_rc; d2.Bpl = pl->W2_rc; d2.out = make_out(pl, dX ? pl->g1_rc : nullptr, Qb, pl->g1_r8, Qb, H);
        d2.gate16 = h1 ? nullptr : (pl->h1_r8 ? pl->h1_r8 : pl->h1_rc); d2.gate16_r8 = pl->h1_r8 != nullptr;
        dx.Apl = pl->g1_rc; dx.Bpl = pl->W1_rc;
    } else {
        // exact-fp32 path with transposed weight copies: the NT products become NN (weights read row-coalesced)
        if (dtype == 0 && p->W3T) { d3.op = OP_BWD_DH_T; d3.transB = 0; d3.B = p->W3T; }
        if (dtype == 0 && p->W2T) { d2.op = OP_BWD_DH_T; d2.transB = 0; d2.B = p->W2T; }
        if (dtype == 0 && p->W1pT) { dx.op = OP_BWD_DX_T; dx.transB = 0; dx.B = p->W1pT; dx.ldb = KP; }
        // deterministic db2 / db1: the dH GEMMs store 32-row partial column sums of g2 / g1 into sg->db_partials ([2][ceil(Qb/32)][H]);
        // dpd_decoder_bwd_weights[_pair] called with the same pointer adds them up.  Needs the register-streamed kernels.
        if (float* dbp = (sg && dtype == 0) ? sg->db_partials : nullptr) {
            if (!(f32_tile_rs(g_plan_tile[d3.op]) && f32_tile_rs(g_plan_tile[d2.op]))) return DPD_E_UNSUPPORTED;
            c2.part_out = dbp; c1.part_out = dbp + (size_t)((Qb + 31) / 32) * H;
            d3.colsum = nullptr; d3.cs2 = &c2;
            d2.colsum = nullptr; d2.cs2 = &c1;
        }
    }
    if (phases & 2)
        if (int rc = gemm_dt(d3)) return rc;
    if (phases & 4)
        if (int rc = gemm_dt(d2)) return rc;
    if (dX && (phases & 4))
        if (int rc = gemm_dt(dx)) return rc;
    return 0;
}

extern "C" int dpd_decoder_bwd_weights(int layer, const float* act, int lda, const float* g, int Qb, int Kin, int Nout,
                                       int dtype, float* dW, float* db, void* ws, size_t ws_bytes, const dpd_planes* pl,
                                       const float* db_partials, void* stream) {
    return dpd_decoder_bwd_weights_live(layer, act, lda, g, Qb, Kin, Nout, dtype, dW, db, ws, ws_bytes, pl, db_partials, nullptr, stream);
}

extern "C" int dpd_decoder_bwd_weights_live(int layer, const float* act, int lda, const float* g, int Qb, int Kin, int Nout,
                                            int dtype, float* dW, float* db, void* ws, size_t ws_bytes, const dpd_planes* pl,
                                            const float* db_partials, const dpd_live_rows* live, void* stream) {
    using namespace dpd;
    if (live) {
        // dW = (compact activation)^T (compact g) over the live contraction length Lp (a device word): the activation is the
        // descriptor's copy (`act` is not read), g of layers 1 / 2 the compact rows dpd_decoder_bwd_data_live wrote, g of layer 3 g3c
        if (!dW || ((layer == 1 || layer == 2) && !g)) return DPD_E_NULL;
        if (layer < 1 || layer > 3 || Qb <= 0 || Kin <= 0 || Nout <= 0) return DPD_E_DIM;
        if (dtype != 0 || (db && !(db_partials && layer != 3))) return DPD_E_UNSUPPORTED;
        if (int rc = check_live(live, Qb, layer == 1 ? Kin : 0, Nout)) return rc;
        if (layer != 1 && Kin != live->H) return DPD_E_DIM;
        ColsumTwoStep cs{};
        cs.part_in = db_partials ? db_partials + (layer == 1 ? (size_t)(Qb / 32) * Nout : 0) : nullptr;
        cs.out = db; cs.nparts = Qb / 32;
        GemmF32Call f;
        f.transA = 1; f.M = Kin; f.N = Nout; f.K = Qb;
        f.A = layer == 1 ? live->Xc : (layer == 2 ? live->h1c : live->h2c); f.lda = Kin;
        f.B = layer == 3 ? live->g3c : g; f.ldb = Nout; f.C = dW; f.ldc = Nout;
        f.tile = g_live_tile[layer == 1 ? LIVE_DW1 : LIVE_DW23]; f.s = (hipStream_t)stream;
        f.cs2 = db ? &cs : nullptr; f.K_dev = live->cnt + 1;
        return gemm_f32(f);
    }
    if (!dW || ((!act || !g) && !(pl && dtype != 0))) return DPD_E_NULL;   // (act / g may be NULL when their R8 planes exist: checked below)
    if (layer == 4 && (!db || !act || !g)) return DPD_E_NULL;
    if (layer < 1 || layer > 4 || Qb <= 0 || Kin <= 0 || Nout <= 0 || lda < Kin) return DPD_E_DIM;
    if (dtype < 0 || dtype > 2) return DPD_E_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    if (layer == 4) {
        if (Nout != 3) return DPD_E_DIM;
        if (!ws || ws_bytes < colsum_ws_floats(Kin, 3) * sizeof(float)) return DPD_E_WORKSPACE;
        float* part = (float*)ws;
        DPD_LAUNCH(colsum_stage1<3>, dim3((Kin + 63) / 64, kColChunks), dim3(256), 0, s, act, lda, g, Qb, Kin, part);
        DPD_CHECK_LAUNCH();
        DPD_LAUNCH(colsum_stage2, dim3((Kin * 3 + 255) / 256), dim3(256), 0, s, (const float*)part, Kin * 3, dW);
        DPD_CHECK_LAUNCH();
        DPD_LAUNCH(dy_colsum_kernel, dim3(1), dim3(256), 0, s, g, Qb, db);
        DPD_CHECK_LAUNCH();
        return 0;
    }
    if ((Nout & 3) || (Kin & 3) || (lda & 3)) return DPD_E_UNSUPPORTED;
    const int op = (layer == 1) ? OP_BWD_DW1 : OP_BWD_DW23;
    const int split = dtype == 0 ? g_plan_split[op] : 1;      // 0 = tail split: up to 3 slabs for the last round's K pieces
    size_t slab_bytes = (split > 1) ? (size_t)split * Kin * Nout * sizeof(float) : 0;
    if (split == 0) slab_bytes = (ws && ws_bytes >= (size_t)3 * Kin * Nout * sizeof(float)) ? (size_t)3 * Kin * Nout * sizeof(float) : 0;
    const size_t col_bytes = db ? colsum_ws_floats(Nout, 0) * sizeof(float) : 0;
    if ((slab_bytes + col_bytes) && (!ws || ws_bytes < slab_bytes + col_bytes)) return DPD_E_WORKSPACE;
    const Scratch scr = scratch_of(ws, ws_bytes, Kin > Nout ? Kin : Nout, Nout);
    pl = usable_planes(pl, dtype, pl ? pl->Q : 0, Qb, layer == 1 ? Kin : 32, Nout);
    if (pl && pl->Qb != Qb) return DPD_E_DIM;
    if (int rc = check_planes(pl, dtype)) return rc;
    const void* apl = !pl ? nullptr : (layer == 1 ? pl->X_r8 : (layer == 2 ? pl->h1_r8 : pl->h2_r8));
    const void* gpl = !pl ? nullptr : (layer == 1 ? pl->g1_r8 : (layer == 2 ? pl->g2_r8 : pl->g3_r8));
    if (dtype != 0 && !(apl && gpl) && !scr.p) return DPD_E_WORKSPACE;
    if ((!act && !apl) || (!g && !gpl) || (!g && db)) return DPD_E_NULL;
    // dW [Kin,Nout] = act^T [Kin,Qb] * g [Qb,Nout].  On the register-streamed fp32 kernels the bias gradient db = colsum(g) falls out
    // of the B operand the GEMM streams anyway (deterministic, no atomics, no extra launch).
    // With db_partials (the 32-row partial column sums dpd_decoder_bwd_data stored for this layer's g: layers 1 and 2) the bias
    // gradient is finished by this GEMM's first-row-block waves: deterministic, no atomics, no extra launch.
    const bool free_db = db && db_partials && (layer == 1 || layer == 2) && dtype == 0 && f32_tile_rs(g_plan_tile[op]) && !(Qb % 32);
    if (db && db_partials && !free_db) return DPD_E_UNSUPPORTED;
    ColsumTwoStep cs{};
    cs.part_in = db_partials ? db_partials + (layer == 1 ? (size_t)((Qb + 31) / 32) * Nout : 0) : nullptr;
    cs.out = db; cs.nparts = (Qb + 31) / 32;
    GemmDtCall c;
    c.dtype = dtype; c.op = op; c.transA = 1; c.M = Kin; c.N = Nout; c.K = Qb;
    c.A = act; c.lda = lda; c.B = g; c.ldb = Nout; c.C = dW; c.ldc = Nout;
    // fp32: the split-K slabs; plane compute types: the base workspace serves the split-K of gemm_dt
    c.ws = ws; c.ws_bytes = dtype == 0 ? slab_bytes : base_ws_or_0(ws, ws_bytes, Kin > Nout ? Kin : Nout, Nout);
    c.scr = scr; c.s = s; c.Apl = apl; c.Bpl = gpl; c.cs2 = free_db ? &cs : nullptr;
    if (int rc = gemm_dt(c)) return rc;
    if (!db || free_db) return 0;   // bias gradient not wanted / already produced
    float* part = (float*)((char*)ws + slab_bytes);
    DPD_LAUNCH(colsum_stage1<0>, dim3((Nout + 63) / 64, kColChunks), dim3(256), 0, s, g, Nout, (const float*)nullptr,
                       Qb, Nout, part);
    DPD_CHECK_LAUNCH();
    DPD_LAUNCH(colsum_stage2, dim3((Nout + 255) / 256), dim3(256), 0, s, (const float*)part, Nout, db);
    DPD_CHECK_LAUNCH();
    return 0;
}

// dW of layers 2 and 3 in ONE grouped launch (identical shapes [H,H] = act^T g): 2 x 256 tiles fill the chip twice
// as well as two 256-tile launches and pay one prologue/epilogue instead of two.
extern "C" int dpd_decoder_bwd_weights_pair(const float* actA, const float* gA, float* dWA, const float* actB, const float* gB,
                                            float* dWB, int lda, int Qb, int Kin, int Nout, int dtype, void* ws,
                                            size_t ws_bytes, const dpd_planes* pl, float* dbA, const float* db_partials, void* stream) {
    return dpd_decoder_bwd_weights_pair_live(actA, gA, dWA, actB, gB, dWB, lda, Qb, Kin, Nout, dtype, ws, ws_bytes, pl, dbA, db_partials, nullptr, stream);
}

extern "C" int dpd_decoder_bwd_weights_pair_live(const float* actA, const float* gA, float* dWA, const float* actB, const float* gB,
                                                 float* dWB, int lda, int Qb, int Kin, int Nout, int dtype, void* ws,
                                                 size_t ws_bytes, const dpd_planes* pl, float* dbA, const float* db_partials,
                                                 const dpd_live_rows* live, void* stream) {
    using namespace dpd;
    if (live) {     // (layer 2, layer 3) over the live contraction length: h1c^T gA and h2c^T g3c (actA / actB / gB are not read)
        if (!dWA || !dWB || !gA) return DPD_E_NULL;
        if (Qb <= 0 || Kin <= 0 || Nout <= 0) return DPD_E_DIM;
        if (dtype != 0 || (dbA && !db_partials)) return DPD_E_UNSUPPORTED;
        if (int rc = check_live(live, Qb, 0, Nout)) return rc;
        if (Kin != live->H) return DPD_E_DIM;
        ColsumTwoStep cs{};
        cs.part_in = db_partials; cs.out = dbA; cs.nparts = Qb / 32;
        GemmF32Call f;
        f.transA = 1; f.M = Kin; f.N = Nout; f.K = Qb;
        f.A = live->h1c; f.lda = Kin; f.B = gA; f.ldb = Nout; f.C = dWA; f.ldc = Nout;
        f.A2 = live->h2c; f.B2 = live->g3c; f.C2 = dWB;
        f.tile = g_live_tile[LIVE_DW23]; f.s = (hipStream_t)stream; f.cs2 = dbA ? &cs : nullptr; f.K_dev = live->cnt + 1;
        return gemm_f32(f);
    }
    if (!dWA || !dWB) return DPD_E_NULL;
    if ((!actA || !actB || !gA || !gB) && !(dtype != 0 && pl && pl->h1_r8 && pl->h2_r8 && pl->g2_r8 && pl->g3_r8)) return DPD_E_NULL;
    if (Qb <= 0 || Kin <= 0 || Nout <= 0 || lda < Kin) return DPD_E_DIM;
    if (dtype < 0 || dtype > 2 || (Nout & 3) || (Kin & 3) || (lda & 3) || (Qb & 31)) return DPD_E_UNSUPPORTED;
    if (dtype != 0 && dbA) return DPD_E_UNSUPPORTED;
    if (dtype != 0) {   // plane path: two launches (the planes of one GEMM at a time live in the scratch)
        const Scratch scr = scratch_of(ws, ws_bytes, Kin > Nout ? Kin : Nout, Nout);
        pl = usable_planes(pl, dtype, pl ? pl->Q : 0, Qb, 32, Nout);
        if (pl && pl->Qb != Qb) return DPD_E_DIM;
        if (int rc = check_planes(pl, dtype)) return rc;
        const bool have = pl && pl->h1_r8 && pl->g2_r8 && pl->h2_r8 && pl->g3_r8;   // pair = (layer 2, layer 3)
        if (!have && !scr.p) return DPD_E_WORKSPACE;
        if (have) {
            // both GEMMs in ONE grouped launch of 64x128 tiles over the whole K (2 x 128 workgroups).  A split-K-2 form on 128x128
            // tiles (2 x 64 x 2 workgroups, two fp32 slabs added in a fixed order) is available through dpd_set_gemm_plan(32,
            // tile, 2) and tested, but measured slower in every compute type (bf16 B=64: 0.3903 vs 0.3861 ms per step; the slab
            // traffic and the reduce launch cost more than the shorter K loop saves).
            // Round 4: split-K with the reduction INSIDE the launch (gemm_x3.hip: inlaunch_reduce; g_x3_pair_split > 1 or automatic):
            // 2 x 64 tiles of 128x128 x 3-4 slices = two workgroups per CU instead of one on half of them.
            // Without a tile from dpd_set_gemm_plan: 128x128 (tile 2) when split, the whole-K 64x128 launch (tile 3) when not.
            int request = g_x3_pair_split;
            if (request < -1 && Qb % (128 * -request)) request = 1;   // the round-2 form of this launch: even slices of whole 128-deep pieces
            int tile = g_x3_pair_tile ? g_x3_pair_tile : 2;
            const int rows2[2] = {Kin, Kin};
            const X3SplitPlan plan = x3_plan_split(pl->np, tile, request, rows2, 2, Nout, Qb, ws, base_ws_or_0(ws, ws_bytes, Kin > Nout ? Kin : Nout, Nout));
            if (!g_x3_pair_tile && plan.split == 1) tile = 3;
            if (tile >= 8 && (pl->np != 1 || Qb % (64 * plan.split))) tile = plan.split > 1 ? 2 : 3;
            X3Call x;
            x.np = pl->np; x.a_fmt = 1; x.b_fmt = 1; x.M = Kin; x.N = Nout; x.K = Qb;
            x.A = (const uint16_t*)pl->h1_r8; x.lda = Kin; x.a_plane = (long)Kin * Qb;
            x.B = (const uint16_t*)pl->g2_r8; x.ldb = Nout; x.b_plane = (long)Qb * Nout;
            x.C = dWA; x.ldc = Nout; x.tile = tile; x.s = (hipStream_t)stream;
            x.ex.A2 = (const uint16_t*)pl->h2_r8; x.ex.B2 = (const uint16_t*)pl->g3_r8; x.ex.C2 = dWB;
            set_split(x, plan);
            return gemm_x3(x);
        }
        // one GEMM after the other, operands split into the scratch
        GemmDtCall c;
        c.dtype = dtype; c.op = OP_BWD_DW23; c.transA = 1; c.M = Kin; c.N = Nout; c.K = Qb;
        c.A = actA; c.lda = lda; c.B = gA; c.ldb = Nout; c.C = dWA; c.ldc = Nout; c.scr = scr; c.s = (hipStream_t)stream;
        if (int rc = gemm_dt(c)) return rc;
        c.A = actB; c.B = gB; c.C = dWB;
        return gemm_dt(c);
    }
    int tile = g_plan_tile[OP_BWD_DW23];
    if (!(f32_tile_dma(tile) || f32_tile_rs(tile))) tile = 8;
    if (dbA && !(db_partials && f32_tile_rs(tile))) return DPD_E_UNSUPPORTED;   // layer 2's bias gradient from the stored partials
    ColsumTwoStep cs{};
    cs.part_in = db_partials; cs.out = dbA; cs.nparts = (Qb + 31) / 32;     // (layer 2 = problem A: the first half of the scratch)
    GemmF32Call f;
    f.transA = 1; f.M = Kin; f.N = Nout; f.K = Qb;
    f.A = actA; f.lda = lda; f.B = gA; f.ldb = Nout; f.C = dWA; f.ldc = Nout;
    f.tile = tile; f.s = (hipStream_t)stream; f.A2 = actB; f.B2 = gB; f.C2 = dWB; f.cs2 = dbA ? &cs : nullptr;
    return gemm_f32(f);
}

// One live dH product beside the weight gradient that does not wait for it (gemm_rs_pair_kernel).  The live dH launch alone is 160
// workgroups for 256 CUs at the training shapes, each wave one dependent chain of H / 2 MFMAs: 40 % of the SIMDs idle and the rest
// hold one wave whose load latency nothing hides.  The dW product of the layer ABOVE reads only what exists already (dW3 = h2c^T g3c
// beside g3c -> g2; dW2 = h1c^T g2 beside g2 -> g1) and fills those SIMDs.  Every element comes from the same wave body over the same
// operands in the same k order as in the separate launches: same bits.
extern "C" int dpd_decoder_bwd_pair_live(int layer, const float* g_in, float* g_out, float* dW, int Qb, int H, const dpd_decoder_params* p,
                                         const dpd_live_rows* live, void* stream) {
    using namespace dpd;
    if (!p || !live || !g_out || !dW || (layer == 2 && !g_in)) return DPD_E_NULL;
    if ((layer != 2 && layer != 3) || Qb <= 0 || H <= 0) return DPD_E_DIM;
    if (!p->W2T || !p->W3T) return DPD_E_UNSUPPORTED;
    if (int rc = check_live(live, Qb, 0, H)) return rc;
    const float* gin = layer == 3 ? live->g3c : g_in;
    const float* act = layer == 3 ? live->h2c : live->h1c;      // the dH part's gate and the dW part's A operand
    GemmF32Call a, b;
    a.M = Qb; a.N = H; a.K = H;
    a.A = gin; a.lda = H; a.B = layer == 3 ? p->W3T : p->W2T; a.ldb = H; a.C = g_out; a.ldc = H;
    a.gate = act; a.epilogue = EPI_GATE; a.tile = g_live_tile[LIVE_DH]; a.s = (hipStream_t)stream; a.M_dev = live->cnt + 1;
    b.transA = 1; b.M = H; b.N = H; b.K = Qb;
    b.A = act; b.lda = H; b.B = gin; b.ldb = H; b.C = dW; b.ldc = H;
    b.tile = g_live_tile[LIVE_PAIR_DW]; b.s = a.s; b.K_dev = live->cnt + 1;
    a.pair = &b;
    return gemm_f32(a);
}

extern "C" int dpd_decoder_bwd_chain_live(const float* dpred, const float* mask, const float* y, const float* h1, const float* h2,
                                          const float* h3, int Qb, int KP, int H, const dpd_decoder_params* p, float* dy, float* g3,
                                          float* g2, float* g1, const dpd_small_grads* sg, void* ws, size_t ws_bytes, int defer_small,
                                          float* dW1, float* dW2, float* dW3, float* db1, float* db2, const dpd_live_rows* live,
                                          void* stream) {
    using namespace dpd;
    if (!live || !dW1 || !dW2 || !dW3 || !g2 || !g1) return DPD_E_NULL;
    if (sg && (sg->db1 || sg->db2)) return DPD_E_UNSUPPORTED;      // (the output-layer launch would zero them behind nobody's back)
    float* dbp = sg ? sg->db_partials : nullptr;
    if ((db1 || db2) && !dbp) return DPD_E_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    // 1. output layer, small gradients, compaction (every check of the shapes and of the descriptor happens in there)
    if (int rc = dpd_decoder_bwd_data_live(dpred, mask, y, h1, h2, h3, Qb, KP, H, p, 0, dy, g3, g2, g1, nullptr, sg, ws, ws_bytes, nullptr,
                                           1 | (defer_small ? 16 : 0), live, stream))
        return rc;
    // 2. / 3. the two pair launches
    if (int rc = dpd_decoder_bwd_pair_live(3, nullptr, g2, dW3, Qb, H, p, live, stream)) return rc;
    if (int rc = dpd_decoder_bwd_pair_live(2, g2, g1, dW2, Qb, H, p, live, stream)) return rc;
    // 4. the partial sums of db2 (first half of the scratch) and db1 in the dense association
    const int nb = Qb / 32;
    if (dbp) {
        LivePartArgs a{{db2 ? g2 : nullptr, db1 ? g1 : nullptr}, {dbp, dbp + (size_t)nb * H}, live->pos, live->cnt, Qb, H};
        DPD_LAUNCH(live_db_partials_kernel, dim3(nb, (H + 255) / 256, 2), dim3(256), 0, s, a);
        DPD_CHECK_LAUNCH();
    }
    // 5. dW1 = Xc^T g1 over the live contraction length; its first-row-block waves add up db1 and, behind it, db2 (in the five-launch form
    // dW2's waves do that: the same sum over the same partials in the same block order)
    ColsumTwoStep cs{};
    cs.part_in = db1 ? dbp + (size_t)nb * H : nullptr; cs.out = db1;
    cs.part_in2 = db2 ? dbp : nullptr; cs.out2 = db2;
    cs.nparts = nb;
    GemmF32Call f;
    f.transA = 1; f.M = KP; f.N = H; f.K = Qb;
    f.A = live->Xc; f.lda = KP; f.B = g1; f.ldb = H; f.C = dW1; f.ldc = H;
    f.tile = g_live_tile[LIVE_DW1]; f.s = s; f.cs2 = (db1 || db2) ? &cs : nullptr; f.K_dev = live->cnt + 1;
    return gemm_f32(f);
}

// dW1, dW2 and dW3 of a plane compute type in ONE grouped launch (round 4).  Every weight-gradient GEMM of the step contracts over the
// query rows (K = Qb = 4096 at B = 64): a workgroup's K loop takes ~27 us whatever the grid, and dW1 alone has 160 tiles of 128x128,
// dW2 / dW3 64 each, for 256 CUs -- launched one after the other they leave 96-192 CUs idle for 27 us each time (tools/
// overlap_probe_bf16.py: dW1 37 us, one dW 27-35 us, both on two streams 42 us).  Here the three problems share one grid (288 tiles of
// 128x128): all operands come from the R8 planes (X / g1, h1 / g2, h2 / g3).  DPD_E_UNSUPPORTED when the planes are not all there
// (the caller then uses dpd_decoder_bwd_weights + _pair); bias gradients are not produced here (plane types: dH epilogues).
extern "C" int dpd_decoder_bwd_weights_trio(int Qb, int KP, int H, int dtype, float* dW1, float* dW2, float* dW3, void* ws, size_t ws_bytes,
                                            const dpd_planes* pl, void* stream) {
    using namespace dpd;
    if (!dW1 || !dW2 || !dW3 || !pl) return DPD_E_NULL;
    if (Qb <= 0 || KP <= 0 || H <= 0) return DPD_E_DIM;
    if (dtype != 1 && dtype != 2) return DPD_E_UNSUPPORTED;
    pl = usable_planes(pl, dtype, pl->Q, Qb, KP, H);
    if (!pl) return DPD_E_UNSUPPORTED;
    if (pl->Qb != Qb) return DPD_E_DIM;
    if (int rc = check_planes(pl, dtype)) return rc;
    if (!(pl->X_r8 && pl->g1_r8 && pl->h1_r8 && pl->g2_r8 && pl->h2_r8 && pl->g3_r8) || (KP & 7) || (Qb % 64)) return DPD_E_UNSUPPORTED;
    // Default tile (one plane): 192x128 (gemm_x3.hip tile 13).  A workgroup's K loop is bound by the LDS-DMA fill of its CU
    // (~30 B/clk/CU for linear 1-KiB pieces), i.e. its time is ~ (BM + BN) * K * 2 B / 72 GB/s whatever else runs, and a CU that gets
    // two tiles takes twice as long: the best tile is the one with the smallest BM + BN that still gives every CU at most ONE
    // workgroup -- 128x128 makes 288 tiles (32 CUs get two: 58 us), 192x128 makes 112 + 48 + 48 = 208 (36 us), 256x128 144 (44 us).
    // Measured in the bf16 step at B = 64 (profiles/r04_bf16_trio_sweep.txt): the three launches apart 71 us, grouped on 128x128
    // tiles 67 us, on 192x128 tiles 51 us (step 0.3107 -> 0.2909 ms on that box).
    int tile = g_x3_trio_tile ? g_x3_trio_tile : ((pl->np == 1 && !(Qb % 64)) ? 13 : 2);
    if (tile > 5 && (pl->np != 1 || g_x3_trio_split > 1 || (Qb % 64))) tile = 2;       // the BK = 64 tiles: one plane, whole K
    const int rows3[3] = {KP, H, H};
    X3Call x;
    x.np = pl->np; x.a_fmt = 1; x.b_fmt = 1; x.M = KP; x.N = H; x.K = Qb;
    x.A = (const uint16_t*)pl->X_r8; x.lda = KP; x.a_plane = (long)KP * Qb;
    x.B = (const uint16_t*)pl->g1_r8; x.ldb = H; x.b_plane = (long)Qb * H;
    x.C = dW1; x.ldc = H; x.tile = tile; x.s = (hipStream_t)stream;
    x.ex.A2 = (const uint16_t*)pl->h1_r8; x.ex.B2 = (const uint16_t*)pl->g2_r8; x.ex.C2 = dW2; x.ex.M2 = H;
    x.ex.A3 = (const uint16_t*)pl->h2_r8; x.ex.B3 = (const uint16_t*)pl->g3_r8; x.ex.C3 = dW3; x.ex.M3 = H;
    set_split(x, x3_plan_split(pl->np, tile, g_x3_trio_split, rows3, 3, H, Qb, ws, base_ws_or_0(ws, ws_bytes, KP > H ? KP : H, H)));
    return gemm_x3(x);
}

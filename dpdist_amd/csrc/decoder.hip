// Implicit-surface decoder: shared MLP  KP(=2503 padded) -> H -> H -> H -> 3, relu6/3, mask.  Forward and backward.
//
// Replaces utils/dpdist_util.py:513-544 (four tf_util.conv2d "1xW VALID conv" == dense layers,
// utils/tf_util.py:161-228), :691 (relu6/3), :695-698 (split + mask) and TF's autodiff of them.
//
// The three wide layers run on the fp32 MFMA GEMM of gemm_f32.hip (bias+ReLU / ReLU-gate fused in the epilogue);
// the 3-wide output layer and the bias gradients are small HBM-bound kernels (decoder_out.hip, decoder_bwd.hip).
// Algorithmic work per query row (H = 1024): 4 663 296 MAC forward.  Activations h1,h2,h3 [Q,H] stay in HBM
// (16.8 MB each at Q = 4096, resident in the 256 MiB Infinity Cache) for the backward pass.
//
// This unit: the GEMM plan and dispatch (gemm_dt), workspace and plane carving, the weight copies and the forward entries.  The
// output layer is decoder_out.hip, the dense backward decoder_bwd.hip, the live-row backward decoder_live.hip (decoder_int.h).
#include <initializer_list>

#include "decoder_int.h"
#include "gemm_x3.h"

namespace dpd {

// The process-wide GEMM plan (decoder_int.h): the one definition.
// Defaults measured on MI355X at B=32 (tools/gemm_bench.py, profiles/): LDS-DMA ring kernels everywhere;
//   fwd L1 (4096x1024x2528)  128x128 16-wave 3-stage ring  ~127 TFLOP/s    fwd L2/3 (K=1024) 128x128 3-stage  ~120
//   bwd dH (2048x1024x1024)   64x64  3-stage               ~ 93..106       bwd dX            64x64 3-stage    ~103
//   bwd dW1 (2528x1024x2048)  64x64  3-stage, split-K 2    ~102            bwd dW2/3         64x64 3-stage    ~ 97
// (run-to-run spread between boxes is ~10 %; the ranking inside one run is stable.  DMA kernels need K % 32 == 0;
//  gemm_f32 falls back to the register-staged 64x64 kernel otherwise.)
int g_plan_tile[OP_COUNT] = {32, 32, 8, 8, 33, 33, 32, 32};
int g_plan_split[OP_COUNT] = {1, 1, 1, 1, 1, 1, 1, 1};   // (0 = tail split, gemm_rs.h: measured no gain on dW1, 0.525 vs 0.5215 ms of GEMM per step)
int g_x3_tile[OP_COUNT] = {0, 0, 0, 0, 0, 0, 0, 0};   // one-plane (bf16) tile override per call site, 0 = automatic
// split-K of the plane weight-gradient GEMMs (K = query rows is long, M x N gives 64-160 tiles of 128x128 for 256 CUs):
//   n > 1: n slices per output tile, reduced INSIDE the launch by the last-arriving slice in slice order (gemm_x3.hip: inlaunch_reduce;
//          deterministic); n < -1: the round-2 form, |n| fp32 slabs + a reduce launch (A/B reference); 1: off; 0: automatic
int g_x3_split[OP_COUNT] = {1, 1, 1, 1, 0, 0, 1, 1};
int g_x3_pair_tile = 0, g_x3_pair_split = 0;   // plane dW2+dW3 pair: tile (0 = automatic), split-K (as above)
int g_x3_trio_tile = 0, g_x3_trio_split = 1;   // plane dW1+dW2+dW3 in one launch (dpd_decoder_bwd_weights_trio): tile, split-K
int g_l1u_tile = 33;   // layer 1 over distinct windows (dpd_decoder_fwd_unique): 32 or 33 (dpd_set_gemm_plan op 8)
// live-row backward (dpd_live_rows): dH over the live rows, dW1, dW2 + dW3 over the live contraction length: 32 or 33 (dpd_set_gemm_plan
// ops 9, 10, 11).  The short dH wants the 32x32 wave tile: a wave's K loop is as long as the dense one's, only the tiles get fewer
// (op 12: the dW part of a pair launch, dpd_decoder_bwd_pair_live; its dH part takes op 9's)
int g_live_tile[4] = {33, 33, 33, 33};

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

// Split-K plan of the plane weight gradients (X3SplitPlan, decoder_int.h)
X3SplitPlan x3_plan_split(int np, int tile, int request, const int* rows, int nprob, int N, int K, void* base, size_t base_bytes) {
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
void set_split(X3Call& c, const X3SplitPlan& p) {
    c.split_k = p.split; c.ws = p.slab; c.ws_bytes = p.slab_bytes; c.red_cnt = p.cnt; c.red_cnt_words = (int)(kRedCntBytes / 8);
}

// One dense product of the decoder in the compute type `dtype`, with the tile / split of call site `op` (GemmDtCall, decoder_int.h)
int gemm_dt(const GemmDtCall& c) {
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
const dpd_planes* usable_planes(const dpd_planes* pl, int dtype, int Q, int Qb, int KP, int H) {
    if (!pl || dtype == 0) return nullptr;
    if ((Q & 7) || (Qb & 31) || (KP & 31) || (H & 63)) return nullptr;
    return pl;
}
int check_planes(const dpd_planes* pl, int dtype) {
    if (!pl) return 0;
    if (pl->np != (dtype == 1 ? 3 : 1)) return DPD_E_DIM;
    return 0;
}
X3Out make_out(const dpd_planes* pl, void* rc, int rc_rows, void* r8, int r8_rows, int cols) {
    X3Out o;
    o.rc = (uint16_t*)rc; o.r8 = (uint16_t*)r8; o.np = pl->np; o.ld_rc = cols; o.r8_rows = r8_rows;
    o.rc_plane = (long)rc_rows * cols; o.r8_plane = (long)r8_rows * cols;
    return o;
}

size_t colsum_ws_floats(int ncols, int nw) { return (size_t)kColChunks * ncols * (nw ? nw : 1); }

size_t base_ws_bytes(int KP, int H) {
    const size_t slabs = (size_t)8 * (size_t)(KP > H ? KP : H) * H * sizeof(float);   // split-K <= 8 of the largest dW
    const size_t cols = colsum_ws_floats(H, 3) * sizeof(float);
    return (slabs + cols + 255) / 256 * 256 + kRedCntBytes;
}
size_t base_ws_or_0(const void* ws, size_t ws_bytes, int KP, int H) {
    const size_t base = base_ws_bytes(KP, H);
    return (ws && ws_bytes >= base) ? base : 0;
}
Scratch scratch_of(void* ws, size_t ws_bytes, int KP, int H) {
    const size_t base = base_ws_bytes(KP, H);
    if (!ws || ws_bytes <= base) return Scratch{nullptr, 0};
    return Scratch{(char*)ws + base, ws_bytes - base};
}

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

extern "C" size_t dpd_workspace_bytes(int Q, int KP, int H, int dtype) {
    return dpd::base_ws_bytes(KP, H) + dpd::plane_bytes(dtype, Q, KP, H);
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
    return out_layer_fwd(h3, p, mask, y, pred, Q, H, s);
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
    return out_layer_fwd(h3, p, mask, y, pred, Q, H, s);
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

// The weights and shapes every all-pairs forward takes (qcounts = NULL: no per-cloud counts); *Q = the rows and their pad rows
static int check_cross(const dpd_decoder_params* p, int ldu, int slot_cap, const int32_t* qcounts, int pairs, int Cb, int N, int KP, int H, int* Q) {
    using namespace dpd;
    if (!p->W1p || !p->b1 || !p->W2 || !p->b2 || !p->W3 || !p->b3 || !p->W4 || !p->b4) return DPD_E_NULL;
    if (pairs <= 0 || N <= 0 || KP <= 0 || H <= 0 || slot_cap <= 0 || ldu < slot_cap || (long)pairs * N > (1L << 30)) return DPD_E_DIM;
    if (qcounts && (Cb <= 0 || pairs % Cb)) return DPD_E_DIM;
    if ((H & 63) || (KP & 31) || KP < 64 || (slot_cap & 3) || (ldu & 3)) return DPD_E_UNSUPPORTED;
    *Q = (pairs * N + 31) / 32 * 32;
    // (the GEMMs address Xu, Pu and the activations with 32-bit byte offsets)
    if (!fits_gemm_offsets((size_t)(KP - 32), (size_t)ldu) || !fits_gemm_offsets((size_t)slot_cap, (size_t)H) || !fits_gemm_offsets((size_t)*Q, (size_t)H))
        return DPD_E_UNSUPPORTED;
    return 0;
}

// qcounts = NULL: dpd_decoder_fwd_cross; otherwise the pair means over each query cloud's own count (pairs = surface clouds x Cb)
static int fwd_cross(const float* Xu /* k-major */, int ldu, int slot_cap, const float* Xt, const int32_t* uid, const int32_t* cnt, float* Pu,
                     const float* maskr, const int32_t* qcounts, int pairs, int Cb, int N, int KP, int H, const dpd_decoder_params* p,
                     float* act0, float* act1, float* y, float* pred, float* Dd, void* stream) {
    using namespace dpd;
    int Q = 0;
    if (int rc = check_cross(p, ldu, slot_cap, qcounts, pairs, Cb, N, KP, H, &Q)) return rc;
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

// Per-point field (patch_rows.hip: dpd_field_gather): the launches of dpd_decoder_fwd_cross over the chunk's rows, without pair means
extern "C" int dpd_decoder_fwd_field(const float* Xu /* k-major */, int ldu, int slot_cap, const float* Xt, const int32_t* uid, const int32_t* cnt,
                                     float* Pu, const float* maskr, int rows, int KP, int H, const dpd_decoder_params* p, float* act0, float* act1,
                                     float* y, float* pred, void* stream) {
    if (!Xu || !Xt || !uid || !cnt || !Pu || !maskr || !p || !act0 || !act1 || !y || !pred) return DPD_E_NULL;
    if (act0 == act1) return DPD_E_DIM;
    int Q = 0;
    if (int rc = check_cross(p, ldu, slot_cap, nullptr, rows, 0, 1, KP, H, &Q)) return rc;
    // h1 -> act0, h2 -> act1, h3 -> act0: nothing is kept for a backward pass
    return fwd_over_slots(Xu, ldu, slot_cap, Xt, uid, cnt + 1, Pu, maskr, Q, KP, H, p, act0, act1, act0, y, pred, (hipStream_t)stream, true);
}

// dpd_decoder_fwd_cross with the three activations kept for dpd_cross_bwd: the same launches on the same operands, so the same bits
extern "C" int dpd_decoder_fwd_cross_keep(const float* Xu /* k-major */, int ldu, int slot_cap, const float* Xt, const int32_t* uid,
                                          const int32_t* cnt, float* Pu, const float* maskr, int pairs, int N, int KP, int H,
                                          const dpd_decoder_params* p, float* h1, float* h2, float* h3, float* y, float* pred, float* Dd,
                                          void* stream) {
    using namespace dpd;
    if (!Xu || !Xt || !uid || !cnt || !Pu || !maskr || !p || !h1 || !h2 || !h3 || !y || !pred) return DPD_E_NULL;      // (Dd = NULL: no pair means)
    if (h1 == h2 || h2 == h3 || h1 == h3) return DPD_E_DIM;
    int Q = 0;
    if (int rc = check_cross(p, ldu, slot_cap, nullptr, pairs, 0, N, KP, H, &Q)) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (int rc = fwd_over_slots(Xu, ldu, slot_cap, Xt, uid, cnt + 1, Pu, maskr, Q, KP, H, p, h1, h2, h3, y, pred, s, true)) return rc;
    if (!Dd) return 0;
    StageProf prof(stream, DPD_STAGE_SMALL_REDUCE, (double)pairs * N * 12.0 + pairs * 4.0);
    DPD_LAUNCH(pair_mean_kernel, dim3((pairs + 3) / 4), dim3(256), 0, s, (const float*)pred, N, pairs, Dd);
    DPD_CHECK_LAUNCH();
    return 0;
}

// Dense backward of the implicit-surface decoder (decoder.hip): the data chain g3 -> g2 -> g1 (-> dX) and the weight gradients, one by
// one, as a pair and as a trio, in the three compute types.  The output-layer step of the data chain is decoder_out.hip's; what an
// entry does with a live-row descriptor (`live` != NULL) is decoder_live.hip's, behind one call each.
#include <initializer_list>

#include "decoder_int.h"

namespace dpd {

// Column sums in two deterministic stages.  Stage 1: block (colblock, chunk) -> partial[chunk][...].
//   NW = 0: partial[chunk][n]     = sum_r g[r][n]                       (bias gradient)
//   NW = 3: partial[chunk][n*3+c] = sum_r a[r][n] * w[r*3+c]            (dW4 = h3^T dy)
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

// Dense data chain (phases 2 and 4) behind the output-layer step:
// g2 = (g3 W3^T) * [h2 > 0] ;  g1 = (g2 W2^T) * [h1 > 0];  db2 / db1 = column sums, fused into the epilogue;
// as-loss mode: gradient w.r.t. the gathered rows, dX = g1 W1p^T  [Qb,KP]
static int dense_data_chain(const BwdData& b, bool g3_planes_done) {
    const int Qb = b.Qb, KP = b.KP, H = b.H, dtype = b.dtype, phases = b.phases;
    const dpd_decoder_params* p = b.p;
    const dpd_planes* pl = b.pl;
    const dpd_small_grads* sg = b.sg;
    GemmDtCall d3, d2, dx;
    for (GemmDtCall* c : {&d3, &d2, &dx}) {
        c->dtype = dtype; c->op = OP_BWD_DH; c->transB = 1; c->M = Qb; c->N = H; c->K = H; c->lda = H; c->ldb = H; c->ldc = H;
        c->epilogue = EPI_GATE; c->scr = b.scr; c->s = b.s;
    }
    d3.A = b.g3; d3.B = p->W3; d3.C = b.g2; d3.gate = b.h2; d3.colsum = sg ? sg->db2 : nullptr;
    d2.A = b.g2; d2.B = p->W2; d2.C = b.g1; d2.gate = b.h1; d2.colsum = sg ? sg->db1 : nullptr;
    dx.op = OP_BWD_DX; dx.N = KP; dx.ldc = KP; dx.epilogue = EPI_NONE;
    dx.A = b.g1; dx.B = p->W1p; dx.C = b.dX;
    ColsumTwoStep c2{}, c1{};
    if (pl) {
        // g3 from a kernel that wrote no planes (this call's unfused output layer, or -- phases without 1 and an fp32 g3 given --
        // dpd_decoder_out_asloss): one conversion launch for the layouts the planes keep
        if ((((phases & 1) && !g3_planes_done) || (!(phases & 1) && b.g3 && (phases & 2))) && (pl->g3_rc || pl->g3_r8)) {
            if (!b.g3) return DPD_E_NULL;
            if (int rc = split_planes(b.g3, Qb, H, H, pl->np, (uint16_t*)pl->g3_rc, H, (long)Qb * H, (uint16_t*)pl->g3_r8, (long)Qb * H, b.s))
                return rc;
        }
        // the ReLU gate from the fp32 activation or, without one, from its bf16 plane
        d3.Apl = pl->g3_rc; d3.Bpl = pl->W3_rc; d3.out = make_out(pl, pl->g2_rc, Qb, pl->g2_r8, Qb, H);
        d3.gate16 = b.h2 ? nullptr : (pl->h2_r8 ? pl->h2_r8 : pl->h2_rc); d3.gate16_r8 = pl->h2_r8 != nullptr;
        d2.Apl = pl->g2_rc; d2.Bpl = pl->W2_rc; d2.out = make_out(pl, b.dX ? pl->g1_rc : nullptr, Qb, pl->g1_r8, Qb, H);
        d2.gate16 = b.h1 ? nullptr : (pl->h1_r8 ? pl->h1_r8 : pl->h1_rc); d2.gate16_r8 = pl->h1_r8 != nullptr;
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
    if (b.dX && (phases & 4))
        if (int rc = gemm_dt(dx)) return rc;
    return 0;
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
    const BwdData b{dpred, mask, y, h1, h2, h3, Qb, KP, H, dtype, phases, p, dy, g3, g2, g1, dX, sg, pl, h3_plane, scr, live, s};
    bool g3_planes_done = false;
    if (int rc = out_layer_bwd(b, &g3_planes_done)) return rc;
    return live ? live_data_chain(b) : dense_data_chain(b, g3_planes_done);
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
    if (live) return live_bwd_weights(layer, g, Qb, Kin, Nout, dtype, dW, db, db_partials, live, (hipStream_t)stream);      // (`act` is not read)
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
    // (actA / actB / gB are not read)
    if (live) return live_bwd_weights_pair(gA, dWA, dWB, Qb, Kin, Nout, dtype, dbA, db_partials, live, (hipStream_t)stream);
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

// Live-row backward of the implicit-surface decoder (decoder.hip): everything that reads a dpd_live_rows descriptor.
#include "decoder_int.h"

namespace dpd {

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
int check_live(const dpd_live_rows* lv, int Qb, int KP, int H) {
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

// The three launches of the live form, each built in ONE place (the entries have checked the descriptor against their Qb, KP and H).
// dH: C (compact rows) = (A WT) * [gate > 0] over the Lp live rows; WT = the transposed weight copy (NN form)
static GemmF32Call live_dh_call(const dpd_live_rows* lv, const float* A, const float* WT, float* C, const float* gate, hipStream_t s) {
    GemmF32Call f;
    f.M = lv->Qb; f.N = lv->H; f.K = lv->H;
    f.A = A; f.lda = lv->H; f.B = WT; f.ldb = lv->H; f.C = C; f.ldc = lv->H;
    f.gate = gate; f.epilogue = EPI_GATE; f.tile = g_live_tile[LIVE_DH]; f.s = s; f.M_dev = lv->cnt + 1;
    return f;
}
// dW [M, H] = (compact activation [., M])^T (compact g) over the live contraction length Lp (a device word); `tile`: LIVE_DW1 / LIVE_DW23 /
// LIVE_PAIR_DW; cs (may be NULL): the bias gradient's second step in the GEMM's first-row-block waves; act2 / g2 / dW2 (may be NULL): a
// second problem of the same shape in the launch
static GemmF32Call live_dw_call(const dpd_live_rows* lv, const float* act, const float* g, float* dW, int M, int tile, const ColsumTwoStep* cs,
                                hipStream_t s, const float* act2 = nullptr, const float* g2 = nullptr, float* dW2 = nullptr) {
    GemmF32Call f;
    f.transA = 1; f.M = M; f.N = lv->H; f.K = lv->Qb;
    f.A = act; f.lda = M; f.B = g; f.ldb = lv->H; f.C = dW; f.ldc = lv->H;
    f.A2 = act2; f.B2 = g2; f.C2 = dW2;
    f.tile = g_live_tile[tile]; f.s = s; f.cs2 = cs; f.K_dev = lv->cnt + 1;
    return f;
}
// ONE launch for the 32-row partial sums of db2 (from the compact g2: first half of dbp) and db1 (g1) in the dense association (a compact
// tile mixes the original tiles: its epilogue cannot produce them); g2 / g1 = NULL: not wanted
static int live_db_partials(const dpd_live_rows* lv, const float* g2, const float* g1, float* dbp, hipStream_t s) {
    const int nb = lv->Qb / 32;
    LivePartArgs a{{g2, g1}, {dbp, dbp + (size_t)nb * lv->H}, lv->pos, lv->cnt, lv->Qb, lv->H};
    DPD_LAUNCH(live_db_partials_kernel, dim3(nb, (lv->H + 255) / 256, 2), dim3(256), 0, s, a);
    DPD_CHECK_LAUNCH();
    return 0;
}

// The data chain over the rows that carry gradient only (see live_compact_kernel): compaction behind the output layer, the two dH
// products over the Lp live rows of the compact copies -- g2 / g1 then hold COMPACT rows -- and the partial sums of db2 / db1
int live_data_chain(const BwdData& b) {
    const dpd_live_rows* live = b.live;
    const int phases = b.phases;
    if (phases & 1)
        if (int rc = live_compact(live, b.dy, b.g3, b.h1, b.h2, b.s)) return rc;
    if (phases & 2)
        if (int rc = gemm_f32(live_dh_call(live, live->g3c, b.p->W3T, b.g2, live->h2c, b.s))) return rc;
    if (phases & 4)
        if (int rc = gemm_f32(live_dh_call(live, b.g2, b.p->W2T, b.g1, live->h1c, b.s))) return rc;
    float* dbp = b.sg ? b.sg->db_partials : nullptr;
    if (dbp && (phases & 6)) return live_db_partials(live, (phases & 2) ? b.g2 : nullptr, (phases & 4) ? b.g1 : nullptr, dbp, b.s);
    return 0;
}

// dpd_decoder_bwd_weights_live with a descriptor: the activation is the descriptor's copy, g of layers 1 / 2 the compact rows
// dpd_decoder_bwd_data_live wrote, g of layer 3 g3c
int live_bwd_weights(int layer, const float* g, int Qb, int Kin, int Nout, int dtype, float* dW, float* db, const float* db_partials,
                     const dpd_live_rows* live, hipStream_t s) {
    if (!dW || ((layer == 1 || layer == 2) && !g)) return DPD_E_NULL;
    if (layer < 1 || layer > 3 || Qb <= 0 || Kin <= 0 || Nout <= 0) return DPD_E_DIM;
    if (dtype != 0 || (db && !(db_partials && layer != 3))) return DPD_E_UNSUPPORTED;
    if (int rc = check_live(live, Qb, layer == 1 ? Kin : 0, Nout)) return rc;
    if (layer != 1 && Kin != live->H) return DPD_E_DIM;
    ColsumTwoStep cs{};
    cs.part_in = db_partials ? db_partials + (layer == 1 ? (size_t)(Qb / 32) * Nout : 0) : nullptr;
    cs.out = db; cs.nparts = Qb / 32;
    return gemm_f32(live_dw_call(live, layer == 1 ? live->Xc : (layer == 2 ? live->h1c : live->h2c), layer == 3 ? live->g3c : g, dW, Kin,
                                 layer == 1 ? LIVE_DW1 : LIVE_DW23, db ? &cs : nullptr, s));
}

// dpd_decoder_bwd_weights_pair_live with a descriptor: (layer 2, layer 3) in one launch, h1c^T gA and h2c^T g3c
int live_bwd_weights_pair(const float* gA, float* dWA, float* dWB, int Qb, int Kin, int Nout, int dtype, float* dbA, const float* db_partials,
                          const dpd_live_rows* live, hipStream_t s) {
    if (!dWA || !dWB || !gA) return DPD_E_NULL;
    if (Qb <= 0 || Kin <= 0 || Nout <= 0) return DPD_E_DIM;
    if (dtype != 0 || (dbA && !db_partials)) return DPD_E_UNSUPPORTED;
    if (int rc = check_live(live, Qb, 0, Nout)) return rc;
    if (Kin != live->H) return DPD_E_DIM;
    ColsumTwoStep cs{};
    cs.part_in = db_partials; cs.out = dbA; cs.nparts = Qb / 32;
    return gemm_f32(live_dw_call(live, live->h1c, gA, dWA, Kin, LIVE_DW23, dbA ? &cs : nullptr, s, live->h2c, live->g3c, dWB));
}
}  // namespace dpd

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
    GemmF32Call a = live_dh_call(live, gin, layer == 3 ? p->W3T : p->W2T, g_out, act, (hipStream_t)stream);
    const GemmF32Call b = live_dw_call(live, act, gin, dW, H, LIVE_PAIR_DW, nullptr, a.s);
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
    if (dbp)
        if (int rc = live_db_partials(live, db2 ? g2 : nullptr, db1 ? g1 : nullptr, dbp, s)) return rc;
    // 5. dW1 = Xc^T g1 over the live contraction length; its first-row-block waves add up db1 and, behind it, db2 (in the five-launch form
    // dW2's waves do that: the same sum over the same partials in the same block order)
    const int nb = Qb / 32;
    ColsumTwoStep cs{};
    cs.part_in = db1 ? dbp + (size_t)nb * H : nullptr; cs.out = db1;
    cs.part_in2 = db2 ? dbp : nullptr; cs.out2 = db2;
    cs.nparts = nb;
    return gemm_f32(live_dw_call(live, live->Xc, g1, dW1, KP, LIVE_DW1, (db1 || db2) ? &cs : nullptr, s));
}

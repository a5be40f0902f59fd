// Shared MLP of the pose network, forward (models/ipcr_model.py:198-233: 3-64-64-64-128-1024 + max pool): pose_point_kernel, one workgroup per
// (cloud, 128-column slice of the last layer), all five layers for the cloud's points in LDS, max pool in the epilogue.
//   <false>  the forward-only refinement (dpd_pose_refine in pose.hip, through launch_pose_point): loops 2..n move the cloud first (PoseMove)
//   <true>   the training evaluation (dpd_pose_point_fwd_train, here): hidden activations and the max pool's tie masks stored for
//            pose_point_bwd.hip
// Second flag AVG: the average-pool encoder (models/ipcr_model.py:236-271, --pn_pool avg): the epilogue sums relu(layer 5) over the cloud's
// points instead of taking their maximum, and the training form stores GATE words instead of tie words (see pose_point_kernel).
// What the units of the pose network share: pose_int.h.  fp32 throughout (MFMA fp32 / FMA).
#include "pose_int.h"
#include "pose_math.h"

namespace dpd {

// LDS (floats).  Weights arrive by LDS-DMA (global_load_lds_dwordx4: no registers, no wait until they are needed), unpadded, with the
// 16-byte chunks of row r stored at position chunk ^ (r & 15) (the DMA writes 1 KiB contiguously per wave, so the swizzle is applied to
// the SOURCE address: dma_piece of lds_dma.h, retired by wait_vmcnt<0> before the barrier in front of the first read; a b128 read of 16 consecutive rows at one k then touches every bank once).  Activations are written by ds_write
// and keep 16-byte-aligned padded rows (KIN + 4 floats).  W5's slice comes in two halves of 64 columns: half 0 has its own 32 KiB,
// half 1 replaces W2 | W3 once layer 3 is done with them and is in flight under layer 4.
constexpr int kS64 = 68, kS128 = 132;
constexpr int kW2 = 0, kW3 = 64 * 64, kW4 = 2 * 64 * 64, kW5a = kW4 + 128 * 64, kW5b = 0;
constexpr int kHA = kW5a + 64 * 128, kHB = kHA + 64 * kS64, kW1 = kHB + 64 * kS128, kBias = kW1 + 192, kPts = kBias + 448, kPointLds = kPts + 192;
static_assert(kPointLds * 4 <= 160 * 1024, "LDS budget");

// ROWS x KIN weights (row-major, contiguous in global memory) -> LDS at float offset `off`, swizzled as above; 4 waves share the pieces
template <int KIN, int ROWS>
__device__ __forceinline__ void dma_weights(const float* __restrict__ W, unsigned lds_base, int off, int wave, int lane) {
    constexpr int CPR = KIN / 4;                              // 16-byte chunks per row
    constexpr int PIECES = ROWS * KIN * 4 / 1024;
#pragma unroll
    for (int p = 0; p < PIECES / 4; ++p) {
        const int piece = wave + 4 * p;
        const int g = piece * 64 + lane, r = g / CPR, pos = g % CPR;
        dma_piece(W + (size_t)r * KIN + 4 * (pos ^ (r & 15)), lds_base + (unsigned)(off * 4 + piece * 1024));
    }
}

// One layer on the fp32 matrix cores: C[pt][out] = bias[out] + sum_k h[pt][k] W[out][k] for NPT 32-point tiles (ptile0 ..) x one 32-output
// tile (weight rows wrow0 .. + 31) per wave.  v_mfma_f32_32x32x2_f32: lane l supplies A[i = l & 31][k = l >> 5] and B[k = l >> 5][j = l & 31];
// here every lane reads ONE float4 of its h row and one of its W row at columns k0 + 4 (l >> 5) .. + 3 and issues four MFMAs (element s of
// both: the same k on both sides, so the order of k inside the step does not matter) -- 8 k per step, an exact fp32 fmaf chain per output.
template <int KIN, int NPT>
__device__ __forceinline__ void mfma_layer(const float* __restrict__ hin, const float* __restrict__ Ws, float bj, int ptile0, int wrow0,
                                           f32x16& c0, f32x16& c1) {
    const int l = threadIdx.x & 63, i = l & 31, h = l >> 5;
#pragma unroll
    for (int r = 0; r < 16; ++r) { c0[r] = bj; c1[r] = bj; }
    const float* ap = hin + (ptile0 * 32 + i) * (KIN + 4) + 4 * h;
    const float* bp = Ws + (wrow0 + i) * KIN;
    const int sw = (wrow0 + i) & 15;
#pragma unroll 2
    for (int k = 0; k < KIN; k += 8) {
        const float4 b = *reinterpret_cast<const float4*>(bp + 4 * (((k >> 2) + h) ^ sw));
        const float4 a0 = *reinterpret_cast<const float4*>(ap + k);
        float4 a1 = a0;
        if (NPT == 2) a1 = *reinterpret_cast<const float4*>(ap + 32 * (KIN + 4) + k);
        c0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.x, b.x, c0, 0, 0, 0);
        if (NPT == 2) c1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.x, b.x, c1, 0, 0, 0);
        c0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.y, b.y, c0, 0, 0, 0);
        if (NPT == 2) c1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.y, b.y, c1, 0, 0, 0);
        c0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.z, b.z, c0, 0, 0, 0);
        if (NPT == 2) c1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.z, b.z, c1, 0, 0, 0);
        c0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.w, b.w, c0, 0, 0, 0);
        if (NPT == 2) c1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.w, b.w, c1, 0, 0, 0);
    }
}

template <int KOUT>
__device__ __forceinline__ void store_relu_tile(float* __restrict__ hout, int ptile, int otile, const f32x16& c) {
    const int l = threadIdx.x & 63;
#pragma unroll
    for (int r = 0; r < 16; ++r) hout[(ptile * 32 + mfma_row(r, l)) * (KOUT + 4) + otile * 32 + (l & 31)] = fmaxf(c[r], 0.f);
}

// models/ipcr_model.py:198-233: cloud c (< nA: ptsA[c], else ptsB[c - nA]) -> f[(row0 + c), slice*128 .. +128) = max over the points of
// relu(W5 relu(W4 relu(W3 relu(W2 relu(W1 p + b1) + b2) + b3) + b4) + b5)
// TRAIN (the training evaluation, dpd_pose_point_fwd_train): the slice-0 workgroup of a cloud also stores the four hidden activations, and every
// workgroup the TIE MASK of its 128 columns -- W = ceil(N / 64) words per (cloud, column), ties[cloud][w][column]; bit b of word w is set iff
// point 64 w + b attains the column's maximum and that maximum is positive (relu' = 0 at 0): what the gradient of reduce_max needs
// (tf.reduce_max / torch.amax share it evenly among ties).  N <= kTrainMaxN.
// Every 64-point pass stores its word against the PASS maximum (the accumulators of its points are in registers only then); the thread
// that stores a column's words keeps the column's running maximum and two pass sets: the passes that attain it (`alive`) and the passes
// whose stored word a later, larger maximum made stale -- it stores zero over those after the last pass (same thread, same address:
// program order).  The comparisons are on the fp32 values the MFMAs produced, so equality is exact.
template <bool TRAIN>
__device__ __forceinline__ void save_rows(float* __restrict__ dst, const float* __restrict__ src_lds, int np, int W, int stride, int t) {
    for (int e = t; e < np * (W / 4); e += 256) {
        const int r = e / (W / 4), c4 = e % (W / 4);
        *reinterpret_cast<float4*>(dst + (size_t)r * W + 4 * c4) = *reinterpret_cast<const float4*>(src_lds + r * stride + 4 * c4);
    }
}
// AVG (models/ipcr_model.py:236-271, tf_util.avg_pool2d over the points): f = (sum over the cloud's real points of relu(layer 5)) / (float)N.
// The sum has ONE order: inside a pass every lane adds the rows it holds, ascending (rows r & 3 + 8 (r >> 2) + 4 half of the first 32-row tile,
// then of the second), the lower lane half's partial sum and the upper one's are added (lower + upper), and the pass sums are added to the
// running sum passes ascending; the quotient is one IEEE division, not a product with a reciprocal.  The origin rows that pad a partial pass
// are left out of the sum.  TRAIN stores, in the tie words' buffer and layout, the GATE words: bit b of word w is set iff point 64 w + b is a
// real point and its layer-5 pre-activation is > 0 (the ReLU gate: every such point carries gradient df / N).  No running maximum, no stale
// word.  TRAIN and !TRAIN run the same epilogue: the same feature bits.
template <bool TRAIN, bool AVG>
__global__ __launch_bounds__(256) void pose_point_kernel(const float* __restrict__ ptsA, const float* __restrict__ ptsB, int nA, int N,
                                                         PointNetW net, int OUT, int row0, float* __restrict__ f, PointSave sv, PoseMove mv) {
    extern __shared__ __attribute__((aligned(16))) float lds[];      // (float4 reads; the alignment the one-unit build took from pose_bwd_cloud_kernel's declaration)
    const int c = blockIdx.x, slice = blockIdx.y, t = threadIdx.x, og = t & 15, pg = t >> 4, l = t & 63;
    const int wv = __builtin_amdgcn_readfirstlane(t >> 6);
    const unsigned lds_base = (unsigned)(uintptr_t)(lds_ptr_t)lds;
    const float* pts = c < nA ? ptsA + (size_t)c * N * 3 : ptsB + (size_t)(c - nA) * N * 3;
    const float* W5s = net.W[4] + (size_t)slice * kSlice * 128;
    float vmax = 0.f;                                          // column wv * 32 + (l & 31) of the slice, over this lane's rows; relu outputs are >= 0 (AVG: the column's running sum)
    float runmax = 0.f;                                        // TRAIN: the column's maximum over the passes so far (all of its points)
    unsigned alive = 0, stale = 0;                             // TRAIN: passes whose word stands / has to be zeroed (see above)
    const int NW = (N + kPP - 1) / kPP;
    dma_weights<64, 64>(net.W[1], lds_base, kW2, wv, l);
    dma_weights<64, 64>(net.W[2], lds_base, kW3, wv, l);
    dma_weights<64, 128>(net.W[3], lds_base, kW4, wv, l);
    dma_weights<128, 64>(W5s, lds_base, kW5a, wv, l);
    // the biases and W1 once
    if (t < 192) lds[kW1 + t] = net.W[0][t];
    if (t < 64) { lds[kBias + t] = net.b[0][t]; lds[kBias + 64 + t] = net.b[1][t]; lds[kBias + 128 + t] = net.b[2][t]; }
    if (t < 128) { lds[kBias + 192 + t] = net.b[3][t]; lds[kBias + 320 + t] = net.b[4][slice * kSlice + t]; }
    const bool move = !TRAIN && mv.h3 != nullptr && c < nA;
    float R[3][3] = {{1.f, 0.f, 0.f}, {0.f, 1.f, 0.f}, {0.f, 0.f, 1.f}}, tr[3] = {0.f, 0.f, 0.f};
    if (move) {
        float* prs = lds + kHA;                                // scratch until layer 1 writes hA (after the loop's first barrier)
        if (wv == 0) {                                         // fc4 as pose_apply_fwd_kernel runs it (pose_math.h)
            float p4[7];
            pose_fc4_wave(mv.h3, c, mv.W4, mv.b4, mv.K4, l, p4);
            if (l == 0) {
#pragma unroll
                for (int j = 0; j < 7; ++j) prs[j] = p4[j];
            }
        }
        __syncthreads();
        float pr[7];
#pragma unroll
        for (int j = 0; j < 7; ++j) pr[j] = prs[j];
        const Pose7 P = quat_normalize_dev(pr, mv.lim_rad);
        const float nrm = quat_norm_dev(P.q);
        const float dc = fmaxf(nrm, 1e-12f);
        float qc[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) qc[i] = P.q[i] / dc;
        quat_to_mat_dev(qc, R);
        tr[0] = P.t[0]; tr[1] = P.t[1]; tr[2] = P.t[2];
        if (slice == 0) {
            if (mv.pred_out && t < 7) mv.pred_out[(size_t)c * 7 + t] = pr[t];
            if (t < 16) {                                      // helper.py:309-329: T <- [R(qc) t; 0 1] @ T
                float Tc[4];
                pose_load_T_col(mv.T_in, c, t & 3, Tc);
                const float v = pose_compose_entry(R, P.t, Tc, t >> 2);
                mv.T_out[(size_t)c * 16 + t] = v;
            }
        }
    }
    for (int p0 = 0; p0 < N; p0 += kPP) {
        const int np = min(kPP, N - p0);
        if (p0 > 0) {
            __syncthreads();                                   // the previous pass is done with W5's second half: W2 | W3 come back
            dma_weights<64, 64>(net.W[1], lds_base, kW2, wv, l);
            dma_weights<64, 64>(net.W[2], lds_base, kW3, wv, l);
        }
        if (!move) {
            if (t < 192) lds[kPts + t] = t < np * 3 ? pts[(size_t)p0 * 3 + t] : 0.f;
        } else if (t < kPP) {                                  // one point per thread, moved by pose_math.h's pose_move_point (mode 0 of the apply kernel)
            float o[3] = {0.f, 0.f, 0.f};
            if (t < np) {
                const float* sp = pts + (size_t)(p0 + t) * 3;
                pose_move_point(R, tr, sp[0], sp[1], sp[2], o);
                if (slice == 0) {
                    float* om = mv.moved + ((size_t)c * N + p0 + t) * 3;
                    om[0] = o[0]; om[1] = o[1]; om[2] = o[2];
                }
            }
            lds[kPts + t * 3] = o[0]; lds[kPts + t * 3 + 1] = o[1]; lds[kPts + t * 3 + 2] = o[2];
        }
        wait_vmcnt<0>();
        __syncthreads();
        // layer 1: 3 -> 64 into hA (K = 3: vector ALU; 4 points x 4 outputs per thread)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float x = lds[kPts + (pg * 4 + i) * 3], y = lds[kPts + (pg * 4 + i) * 3 + 1], z = lds[kPts + (pg * 4 + i) * 3 + 2];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int o = og + 16 * j;
                const float v = fmaf(z, lds[kW1 + o * 3 + 2], fmaf(y, lds[kW1 + o * 3 + 1], fmaf(x, lds[kW1 + o * 3], lds[kBias + o])));
                lds[kHA + (pg * 4 + i) * kS64 + o] = fmaxf(v, 0.f);
            }
        }
        __syncthreads();
        if (TRAIN && slice == 0) save_rows<TRAIN>(sv.h[0] + ((size_t)(row0 + c) * N + p0) * 64, lds + kHA, np, 64, kS64, t);
        f32x16 c0, c1;
        // layer 2: hA -> hB (64 wide): wave = (point tile wv & 1, output tile wv >> 1)
        mfma_layer<64, 1>(lds + kHA, lds + kW2, lds[kBias + 64 + (wv >> 1) * 32 + (l & 31)], wv & 1, (wv >> 1) * 32, c0, c1);
        store_relu_tile<64>(lds + kHB, wv & 1, wv >> 1, c0);
        __syncthreads();
        if (TRAIN && slice == 0) save_rows<TRAIN>(sv.h[1] + ((size_t)(row0 + c) * N + p0) * 64, lds + kHB, np, 64, kS64, t);
        // layer 3: hB -> hA
        mfma_layer<64, 1>(lds + kHB, lds + kW3, lds[kBias + 128 + (wv >> 1) * 32 + (l & 31)], wv & 1, (wv >> 1) * 32, c0, c1);
        store_relu_tile<64>(lds + kHA, wv & 1, wv >> 1, c0);
        __syncthreads();                                       // W2 | W3 are done with: the second half of W5's slice takes their place,
        if (TRAIN && slice == 0) save_rows<TRAIN>(sv.h[2] + ((size_t)(row0 + c) * N + p0) * 64, lds + kHA, np, 64, kS64, t);
        dma_weights<128, 64>(W5s + 64 * 128, lds_base, kW5b, wv, l);      // in flight under layer 4
        // layer 4: hA -> hB (128 wide): wave = output tile wv, both point tiles
        mfma_layer<64, 2>(lds + kHA, lds + kW4, lds[kBias + 192 + wv * 32 + (l & 31)], 0, wv * 32, c0, c1);
        store_relu_tile<128>(lds + kHB, 0, wv, c0);
        store_relu_tile<128>(lds + kHB, 1, wv, c1);
        wait_vmcnt<0>();
        __syncthreads();
        if (TRAIN && slice == 0) save_rows<TRAIN>(sv.h[3] + ((size_t)(row0 + c) * N + p0) * 128, lds + kHB, np, 128, kS128, t);
        // layer 5 (slice): waves 0, 1 on the first half of the slice, 2, 3 on the second; max over this lane's valid points
        mfma_layer<128, 2>(lds + kHB, lds + (wv < 2 ? kW5a : kW5b), lds[kBias + 320 + wv * 32 + (l & 31)], 0, (wv & 1) * 32, c0, c1);
        if (AVG) {
            float ps = 0.f;                                    // this lane's rows of the pass, ascending
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (mfma_row(r, l) < np) ps += fmaxf(c0[r], 0.f);
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (32 + mfma_row(r, l) < np) ps += fmaxf(c1[r], 0.f);
            vmax += sum_x32(ps);                               // lower lane half + upper (the other rows of the same column), in both; passes ascending
            if (TRAIN) {
                unsigned lo = 0, hi = 0;                       // rows 0..31 come from c0, rows 32..63 from c1
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = mfma_row(r, l);
                    if (row < np && c0[r] > 0.f) lo |= 1u << row;
                    if (32 + row < np && c1[r] > 0.f) hi |= 1u << row;
                }
                lo |= (unsigned)__shfl_xor((int)lo, 32, 64);
                hi |= (unsigned)__shfl_xor((int)hi, 32, 64);
                if ((l >> 5) == 0)
                    sv.ties[((size_t)(row0 + c) * NW + p0 / kPP) * OUT + slice * kSlice + wv * 32 + (l & 31)] = ((unsigned long long)hi << 32) | lo;
            }
            continue;
        }
        float pmax = 0.f;                                      // this pass alone
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            if (mfma_row(r, l) < np) pmax = fmaxf(pmax, c0[r]);          // = max(relu(.)): starts at 0
            if (32 + mfma_row(r, l) < np) pmax = fmaxf(pmax, c1[r]);
        }
        vmax = fmaxf(vmax, pmax);
        if (TRAIN) {        // (the accumulators of this pass's points are still in registers)
            __syncthreads();
            float* red = lds + kHA;                            // (layer 1 of the next pass writes hA after that pass's first two barriers)
            red[(l >> 5) * kSlice + wv * 32 + (l & 31)] = pmax;
            __syncthreads();
            const int col = wv * 32 + (l & 31);
            float m = fmaxf(red[col], red[kSlice + col]);      // the pass maximum of the column
            const int w = p0 / kPP;
            if (m > runmax) { stale |= alive; alive = 1u << w; runmax = m; }
            else if (m == runmax && m > 0.f) alive |= 1u << w;
            else m = 0.f;                                      // a smaller pass maximum (or none positive): an empty word
            unsigned lo = 0, hi = 0;                           // rows 0..31 come from c0, rows 32..63 from c1
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = mfma_row(r, l);
                if (row < np && m > 0.f && c0[r] == m) lo |= 1u << row;
                if (32 + row < np && m > 0.f && c1[r] == m) hi |= 1u << row;
            }
            lo |= (unsigned)__shfl_xor((int)lo, 32, 64);       // the two lane halves hold the other rows of the same column
            hi |= (unsigned)__shfl_xor((int)hi, 32, 64);
            if ((l >> 5) == 0) sv.ties[((size_t)(row0 + c) * NW + w) * OUT + slice * kSlice + col] = ((unsigned long long)hi << 32) | lo;
        }
    }
    if (AVG) {                                                 // (both lane halves hold the column's sum)
        if ((l >> 5) == 0) f[(size_t)(row0 + c) * OUT + slice * kSlice + wv * 32 + (l & 31)] = vmax / (float)N;
        return;
    }
    if (TRAIN && (l >> 5) == 0) {
        while (stale) {
            const int w = __ffs((int)stale) - 1;
            stale &= stale - 1;
            sv.ties[((size_t)(row0 + c) * NW + w) * OUT + slice * kSlice + wv * 32 + (l & 31)] = 0ull;
        }
    }
    __syncthreads();
    float* red = lds + kHA;                                    // [2 lane halves][128 columns]
    red[(l >> 5) * kSlice + wv * 32 + (l & 31)] = vmax;
    __syncthreads();
    if (t < kSlice) f[(size_t)(row0 + c) * OUT + slice * kSlice + t] = fmaxf(red[t], red[kSlice + t]);
}

}  // namespace dpd

int dpd::check_point_layers(const dpd_pose_net* net) {
    if (!net) return DPD_E_NULL;
    for (int i = 0; i < 5; ++i)
        if (!net->Wp[i] || !net->bp[i]) return DPD_E_NULL;
    return 0;
}

dpd::PointNetW dpd::point_net_of(const dpd_pose_net* net) {
    PointNetW pw{};
    for (int i = 0; i < 5; ++i) { pw.W[i] = net->Wp[i]; pw.b[i] = net->bp[i]; }
    return pw;
}

namespace dpd {
template <bool TRAIN, bool AVG>
static int launch_pose_point_form(const float* ptsA, const float* ptsB, int nA, int clouds, int N, const PointNetW& pw, int OUT, float* f,
                                  const PointSave& sv, const PoseMove& mv, hipStream_t s) {
    static LdsOptIn opt_in;                                  // of this instantiation's kernel
    const size_t lds = (size_t)kPointLds * sizeof(float);
    if (int rc = ensure_dyn_lds(opt_in, (const void*)pose_point_kernel<TRAIN, AVG>, lds)) return rc;
    DPD_LAUNCH((pose_point_kernel<TRAIN, AVG>), dim3((unsigned)clouds, (unsigned)(OUT / kSlice)), dim3(256), lds, s, ptsA, ptsB, nA, N, pw, OUT, 0, f, sv, mv);
    DPD_CHECK_LAUNCH();
    return 0;
}
}  // namespace dpd

template <bool TRAIN>
int dpd::launch_pose_point(const float* ptsA, const float* ptsB, int nA, int clouds, int N, const PointNetW& pw, int OUT, float* f, const PointSave& sv,
                           const PoseMove& mv, bool avg, hipStream_t s) {
    return avg ? launch_pose_point_form<TRAIN, true>(ptsA, ptsB, nA, clouds, N, pw, OUT, f, sv, mv, s)
               : launch_pose_point_form<TRAIN, false>(ptsA, ptsB, nA, clouds, N, pw, OUT, f, sv, mv, s);
}
template int dpd::launch_pose_point<false>(const float*, const float*, int, int, int, const PointNetW&, int, float*, const PointSave&, const PoseMove&,
                                           bool, hipStream_t);
template int dpd::launch_pose_point<true>(const float*, const float*, int, int, int, const PointNetW&, int, float*, const PointSave&, const PoseMove&,
                                          bool, hipStream_t);

extern "C" int dpd_pose_point_tie_words(int N) { return N > 0 ? (N + dpd::kPP - 1) / dpd::kPP : 0; }

extern "C" int dpd_pose_point_fwd_train_pool(const dpd_pose_net* net, const float* ptsA, const float* ptsB, int nA, int nB, int N, int pool, float* f,
                                             float* h1, float* h2, float* h3, float* h4, unsigned long long* words, void* stream) {
    using namespace dpd;
    if (int rc = check_point_layers(net)) return rc;
    if (net->out_features != 1024) return DPD_E_UNSUPPORTED;
    if (!ptsA || (nB > 0 && !ptsB) || !f || !h1 || !h2 || !h3 || !h4 || !words) return DPD_E_NULL;
    if (nA <= 0 || nB < 0 || N <= 0) return DPD_E_DIM;
    if (!pool_known(pool)) return DPD_E_UNSUPPORTED;
    if (N > kTrainMaxN) return DPD_E_UNSUPPORTED;          // the kernel keeps its pass sets in 32-bit words
    if ((((uintptr_t)h1 | (uintptr_t)h2 | (uintptr_t)h3 | (uintptr_t)h4) & 15) != 0) return DPD_E_UNSUPPORTED;
    return launch_pose_point<true>(ptsA, ptsB, nA, nA + nB, N, point_net_of(net), net->out_features, f, PointSave{{h1, h2, h3, h4}, words}, PoseMove{},
                                   pool == DPD_POOL_AVG, (hipStream_t)stream);
}

extern "C" int dpd_pose_point_fwd_train(const dpd_pose_net* net, const float* ptsA, const float* ptsB, int nA, int nB, int N, float* f,
                                        float* h1, float* h2, float* h3, float* h4, unsigned long long* ties, void* stream) {
    return dpd_pose_point_fwd_train_pool(net, ptsA, ptsB, nA, nB, N, DPD_POOL_MAX, f, h1, h2, h3, h4, ties, stream);
}

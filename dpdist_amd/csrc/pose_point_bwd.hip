// Shared MLP of the pose network, backward (what the units of the pose network share: pose_int.h).
// The training evaluation of a registration step (pcrnet-registration/iterative_PCRNet_ours.py:442-470) differentiates the pose network
// w.r.t. its WEIGHTS only (the refined source cloud is a constant of the step).  Shared MLP + max pool (models/ipcr_model.py:198-233) here:
//   dpd_pose_point_fwd_train   (pose_point.hip) the forward kernel with its hidden activations and the max pool's tie masks stored
//   dpd_pose_point_bwd         d features [clouds, OUT] -> dW1..dW5, db1..db5 (TF / torch autodiff of five 1x1 convolutions, ReLU, reduce_max)
// The max pool makes the last layer's gradient SPARSE: per (cloud, column) only the points that attain a positive maximum carry gradient
// (evenly shared among ties, like tf.reduce_max), i.e. one 128-vector per (cloud, column) instead of a [points, 1024] matrix:
//   pose_bwd_w5_dh4_kernel  ONE launch, two block roles:
//     (w5)  wave = output column c: dW5[c, :] = sum over clouds of coef * h4[tied point, :], db5[c] = sum of the column's gradient
//     (dh4) the gradient of layer 4's output, g4 = S W5 with the selection matrix S built from the tie masks, on the fp32
//                           matrix cores (workgroup = cloud x 32x32 tile, wave = 128 columns): independent of how the maxima spread over points
//   pose_bwd_cloud_kernel   workgroup = (cloud, 64-point chunk): layers 4..1 on v_mfma_f32_32x32x2_f32 out of LDS; one partial record of weight
//                           gradients per chunk
//   pose_bwd_reduce_kernel  sums the clouds x chunks partials in (cloud, chunk) order
// fp32 throughout (MFMA fp32 = an fmaf chain per element); every sum has a fixed order (bitwise reproducible).
// The average pool (dpd_pose_point_bwd_pool with DPD_POOL_AVG) makes that gradient DENSE -- every point with an open ReLU gate carries df / N:
// dW5 is then a real product (pose_avg_dw5_kernel, further down, with its coefficient and reduce kernels); the g4 role, the per-cloud kernel and
// the reduce kernel above serve both pools.
#include "pose_int.h"

namespace dpd {

constexpr int kPart = 128 * 64 + 128 + 64 * 64 + 64 + 64 * 64 + 64 + 64 * 3 + 64;      // dW4 | db4 | dW3 | db3 | dW2 | db2 | dW1 | db1 per (cloud, chunk)

// (wave = output column c; the blocks after the g4 tiles of pose_bwd_w5_dh4_kernel, eight columns each)
__device__ __forceinline__ void bwd_w5_wave(const float* __restrict__ df, const unsigned long long* __restrict__ ties, const float* __restrict__ h4,
                                            int C, int N, int OUT, float* __restrict__ dW5, float* __restrict__ db5, int c) {
    const int l = threadIdx.x & 63;
    if (c >= OUT) return;
    float a0 = 0.f, a1 = 0.f, bsum = 0.f;
    const int NW = (N + 63) / 64;
    for (int cl0 = 0; cl0 < C; cl0 += 64) {
        // lane = cloud: the column's tie words and gradient of 64 clouds requested together, so that the row loads below do not wait on them
        const int mine = cl0 + l;
        int mycnt = 0, myfirst = 0;                          // tied points over the NW words; the lowest of them
        if (mine < C) {
            for (int w = 0; w < NW; ++w) {
                const unsigned long long b = ties[((size_t)mine * NW + w) * OUT + c];
                if (b && !mycnt) myfirst = 64 * w + __ffsll((long long)b) - 1;
                mycnt += __popcll(b);
            }
        }
        const float myg = mycnt ? df[(size_t)mine * OUT + c] : 0.f;
        const float mycoef = mycnt ? myg / (float)mycnt : 0.f;
        const bool multi = mycnt > 1;
        const int n = min(64, C - cl0);
        for (int k0 = 0; k0 < n; k0 += 8) {          // eight clouds at a time: their (single) tied rows are requested together
            float2 h[8];
            float cf[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int k = min(k0 + u, n - 1);
                cf[u] = (k0 + u < n) ? __shfl(mycoef, k, 64) : 0.f;
                const int p = __shfl(myfirst, k, 64);
                h[u] = *reinterpret_cast<const float2*>(h4 + ((size_t)(cl0 + k) * N + p) * 128 + 2 * l);
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) { a0 += cf[u] * h[u].x; a1 += cf[u] * h[u].y; }      // (a cloud without a positive maximum: coef 0)
        }
        // further tied points of a column (duplicated points): rare, one at a time, after the first ones, in cloud / point order
        unsigned long long any = __ballot(multi);
        while (any) {
            const int k = __ffsll((long long)any) - 1;
            any &= any - 1;
            const float coef = __shfl(mycoef, k, 64);
            const int first = __shfl(myfirst, k, 64);
            for (int w = first >> 6; w < NW; ++w) {  // word by word, points ascending (wave-uniform loads)
                unsigned long long bits = ties[((size_t)(cl0 + k) * NW + w) * OUT + c];
                if (w == (first >> 6)) bits &= bits - 1;      // the first point was taken above
                while (bits) {
                    const int p = 64 * w + __ffsll((long long)bits) - 1;
                    bits &= bits - 1;
                    const float2 hh = *reinterpret_cast<const float2*>(h4 + ((size_t)(cl0 + k) * N + p) * 128 + 2 * l);
                    a0 += coef * hh.x;
                    a1 += coef * hh.y;
                }
            }
        }
        // db5[c] = sum of the column's gradient over the clouds in which the maximum is positive: lane sums in a fixed tree
        float g = myg;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) g += __shfl_xor(g, o, 64);
        bsum += g;
    }
    *reinterpret_cast<float2*>(dW5 + (size_t)c * 128 + 2 * l) = make_float2(a0, a1);
    if (l == 0) db5[c] = bsum;
}

// g4[cloud, p, :] = [h4 > 0] * sum over the columns whose maximum point p attains of coef * W5[column, :], coef = df / (number of tied points).
// As a product on the fp32 matrix cores: g4 = S W5 with S [64 points][1024 columns] holding coef[col] at the point(s) that attain column col's
// maximum -- one nonzero per column -- so the zeros cost 16.8 MFLOP per cloud and NOTHING depends on how the maxima are spread over the points.
// (The sparse forms walked each point's hit list: a few "critical" points attain hundreds of columns while most attain none, and every batch of
// weight rows was a dependent L2 round trip -- 30 us with a wave per point, 39-47 us with a workgroup per point.)
// Workgroup = (cloud, 32 points x 32 inputs tile), eight waves, wave w = columns 128 w .. + 127: the A operand is built in registers from the tie
// word and the coefficient of its column (LDS broadcasts), the B operand W5[col][n0 + lane % 32] is read straight from global memory (coalesced:
// v_mfma_f32_32x32x2_f32 wants one k per lane half), all 64 of them requested before the first product.  The eight partial tiles are added in
// wave order: columns ascending, deterministic; adding an exact zero changes nothing, so this IS the ascending-column sum of the sparse forms.
// ONE launch for both consumers of d features: blocks [0, clouds x tiles) the g4 tiles, the rest dW5 / db5 (eight columns per block) -- two
// launches of 10.6 + 5.6 us that read the same df / ties and write disjoint outputs.
// N > 64: a cloud has 4 ceil(N / 32) tiles; a 32-point tile lies inside ONE tie word (m0 >> 6), but the coefficient divides by the tied points of
// ALL words -- pose_tie_coef_kernel makes coef [clouds, OUT] once (`coefg`) instead of every tile counting NW words per column.
__global__ __launch_bounds__(256) void pose_tie_coef_kernel(const float* __restrict__ df, const unsigned long long* __restrict__ ties, int C, int NW,
                                                             int OUT, float* __restrict__ coef) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= C * OUT) return;
    const int c = i / OUT, col = i % OUT;
    int cnt = 0;
    for (int w = 0; w < NW; ++w) cnt += __popcll(ties[((size_t)c * NW + w) * OUT + col]);
    coef[i] = cnt ? df[i] / (float)cnt : 0.f;
}

__global__ __launch_bounds__(512) void pose_bwd_w5_dh4_kernel(const float* __restrict__ df, const unsigned long long* __restrict__ ties,
                                                               const float* __restrict__ W5, const float* __restrict__ h4, int C, int N, int OUT,
                                                               float* __restrict__ g4g, float* __restrict__ dW5, float* __restrict__ db5,
                                                               int tiles, const float* __restrict__ coefg) {
    __shared__ unsigned long long sT[1024];
    __shared__ float sC[1024];
    __shared__ float part[8][1024];
    if ((int)blockIdx.x >= C * tiles) {
        bwd_w5_wave(df, ties, h4, C, N, OUT, dW5, db5, ((int)blockIdx.x - C * tiles) * 8 + (int)(threadIdx.x >> 6));
        return;
    }
    const int c = (int)blockIdx.x / tiles, tile = (int)blockIdx.x % tiles, m0 = (tile >> 2) * 32, n0 = (tile & 3) * 32;
    const int NW = (N + 63) / 64;
    const int t = threadIdx.x, wv = t >> 6, l = t & 63, i = l & 31, h = l >> 5;
    const int kb = wv * 128;
    // every global load of the kernel is requested here, together
    float w[64];
    const float* wp = W5 + (size_t)(kb + h) * 128 + n0 + i;
#pragma unroll
    for (int j = 0; j < 64; ++j) w[j] = wp[(size_t)j * 256];
    unsigned long long tb[2];
    float dv[2], hv[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int col = q * 512 + t;
        tb[q] = ties[((size_t)c * NW + (m0 >> 6)) * OUT + col];
        dv[q] = coefg ? coefg[(size_t)c * OUT + col] : df[(size_t)c * OUT + col];
        const int pr = m0 + (col >> 5);                       // (the epilogue's element: row col / 32 of the tile, input n0 + col % 32)
        hv[q] = pr < N ? h4[((size_t)c * N + pr) * 128 + n0 + (col & 31)] : 0.f;
    }
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        sT[q * 512 + t] = tb[q];
        sC[q * 512 + t] = coefg ? dv[q] : (tb[q] ? dv[q] / (float)__popcll(tb[q]) : 0.f);      // (coefg == nullptr: one word, NW == 1)
    }
    __syncthreads();
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const int sh = (m0 + i) & 63;
#pragma unroll
    for (int j = 0; j < 64; ++j) {
        const int col = kb + 2 * j + h;
        const float a = ((sT[col] >> sh) & 1ull) ? sC[col] : 0.f;
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, w[j], acc, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) part[wv][mfma_row(r, l) * 32 + i] = acc[r];
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int o = q * 512 + t, pr = m0 + (o >> 5);
        float sum = part[0][o];
#pragma unroll
        for (int u = 1; u < 8; ++u) sum += part[u][o];
        if (pr < N) g4g[((size_t)c * N + pr) * 128 + n0 + (o & 31)] = hv[q] > 0.f ? sum : 0.f;
    }
}

// ---- layers 4..1 of one cloud on the fp32 matrix cores.  Every product is C[m][n] = sum_k A[m][k] B[n][k] with BOTH operands k-contiguous in
// LDS (rows padded by 4 floats: conflict-free 16-byte reads), so each tensor is kept in the orientation(s) its products contract over:
//   dW_l [o][i] = sum_p g_l[p][o] h_{l-1}[p][i]      A = g_l^T [o][p], B = h_{l-1}^T [i][p]
//   dh   [p][i] = sum_o g_l[p][o] W_l[o][i]          A = g_l [p][o],   B = W_l^T [i][o];   g_{l-1} = dh * [h_{l-1} > 0]
// 32x32 output tiles of v_mfma_f32_32x32x2_f32 (an exact fp32 fmaf chain per element, k ascending), four waves.  The FMA form of this kernel
// (one output row per thread, operands re-read from LDS for every multiply) was LDS-bandwidth bound at 45 us.
template <int K>
__device__ __forceinline__ f32x16 bwd_mm_tile(const float* __restrict__ A, int sa, const float* __restrict__ Bm, int sb, int m0, int n0) {
    const int l = threadIdx.x & 63, i = l & 31, h = l >> 5;
    f32x16 c;
#pragma unroll
    for (int r = 0; r < 16; ++r) c[r] = 0.f;
    const float* ap = A + (m0 + i) * sa + 4 * h;
    const float* bp = Bm + (n0 + i) * sb + 4 * h;
#pragma unroll 4
    for (int k = 0; k < K; k += 8) {
        const float4 a = *reinterpret_cast<const float4*>(ap + k);
        const float4 b = *reinterpret_cast<const float4*>(bp + k);
        c = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, c, 0, 0, 0);
    }
    return c;
}
// (the k order inside a step of 8 is 4 h + e for lane half h: the two halves of the wave supply the two k of each 32x32x2 product)

constexpr int kBT = 256;       // threads of the per-cloud backward workgroup (four waves)
constexpr int kP64 = 68, kP128 = 132;
// LDS (floats): G [64 p][132] | GT [128 o][68] | HT [64 i][68] | WT [64 i][132] | GA [64][68] | GAT [64][68] | points [64][4]
//   layer 4: G = g4, GT = g4^T, HT = h3^T, WT = W4^T -> dW4, g3 (GA, GAT)
//   layer 3: HT = h2^T, WT = W3^T (stride 68)         -> dW3, g2 (G as [64][68], GT as [64][68])
//   layer 2: HT = h1^T, WT = W2^T                     -> dW2, g1 (GA)
constexpr int kMG = 0, kMGT = kMG + 64 * kP128, kMHT = kMGT + 128 * kP64, kMWT = kMHT + 64 * kP64, kMGA = kMWT + 64 * kP128, kMGAT = kMGA + 64 * kP64,
              kMPts = kMGAT + 64 * kP64, kBwdLds = kMPts + 256;
static_assert(kBwdLds * 4 <= 160 * 1024, "LDS budget");

// src [rows][cols] row-major in global memory (rows < nrow valid, else zero) -> dst[c][r] (transposed, stride ds), and optionally dst2[r][c]
__device__ __forceinline__ void lds_load_t(const float* __restrict__ src, int nrow, int rows, int cols, float* __restrict__ dstT, int dsT,
                                           float* __restrict__ dst, int ds, int t) {
    const int c4n = cols / 4;
    for (int e = t; e < rows * c4n; e += kBT) {
        const int r = e / c4n, c4 = (e % c4n) * 4;
        const float4 v = r < nrow ? *reinterpret_cast<const float4*>(src + (size_t)r * cols + c4) : make_float4(0.f, 0.f, 0.f, 0.f);
        dstT[(c4 + 0) * dsT + r] = v.x; dstT[(c4 + 1) * dsT + r] = v.y; dstT[(c4 + 2) * dsT + r] = v.z; dstT[(c4 + 3) * dsT + r] = v.w;
        if (dst) *reinterpret_cast<float4*>(dst + r * ds + c4) = v;
    }
}

// the same for a [64][64] matrix in two steps, so that the NEXT layer's operands are requested before this layer's products and written to LDS
// after them (a dependent global round trip per layer otherwise): thread t holds rows r = t / 16 + 16 q (q = 0..3), columns 4 (t % 16) .. + 3
struct Pre64 {
    float4 v[4];
};
__device__ __forceinline__ Pre64 pre64_load(const float* __restrict__ src, int nrow, int t) {
    Pre64 x;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int r = (t >> 4) + 16 * q, c4 = (t & 15) * 4;
        x.v[q] = r < nrow ? *reinterpret_cast<const float4*>(src + (size_t)r * 64 + c4) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    return x;
}
__device__ __forceinline__ void pre64_store_t(const Pre64& x, float* __restrict__ dstT, int t) {      // dstT[c][r], stride 68
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int r = (t >> 4) + 16 * q, c4 = (t & 15) * 4;
        dstT[(c4 + 0) * kP64 + r] = x.v[q].x; dstT[(c4 + 1) * kP64 + r] = x.v[q].y; dstT[(c4 + 2) * kP64 + r] = x.v[q].z; dstT[(c4 + 3) * kP64 + r] = x.v[q].w;
    }
}

// dW tile(s) of this wave -> the cloud's partial record; db[o] = sum_p g[p][o] by the first KO threads (G^T rows are contiguous in p)
template <int KO>
__device__ __forceinline__ void bwd_layer_dw(const float* __restrict__ GT, const float* __restrict__ HT, float* __restrict__ dW, float* __restrict__ db,
                                             int np, int t) {
    const int wv = t >> 6, l = t & 63;
    constexpr int TILES = (KO / 32) * 2;                  // 32x32 tiles of dW [KO][64]
    for (int tile = wv; tile < TILES; tile += 4) {
        const int m0 = (tile >> 1) * 32, n0 = (tile & 1) * 32;
        const f32x16 c = bwd_mm_tile<64>(GT, kP64, HT, kP64, m0, n0);
#pragma unroll
        for (int r = 0; r < 16; ++r) dW[(m0 + mfma_row(r, l)) * 64 + n0 + (l & 31)] = c[r];
    }
    if (t < KO) {
        float s = 0.f;
        for (int p = 0; p < np; ++p) s += GT[t * kP64 + p];
        db[t] = s;
    }
}

// g_prev = (g W) * [h_prev > 0]: tile (wave) of [64 p][64 i]; written as [p][i] (stride so) and transposed [i][p] (stride 68)
template <int KO>
__device__ __forceinline__ void bwd_layer_dx(const float* __restrict__ G, int sg, const float* __restrict__ WT, int sw, const float* __restrict__ HT,
                                             float* __restrict__ out, int so, float* __restrict__ outT, int t) {
    const int wv = t >> 6, l = t & 63;
    const int m0 = (wv >> 1) * 32, n0 = (wv & 1) * 32;
    const f32x16 c = bwd_mm_tile<KO>(G, sg, WT, sw, m0, n0);
    const int col = n0 + (l & 31);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = m0 + mfma_row(r, l);
        const float v = HT[col * kP64 + row] > 0.f ? c[r] : 0.f;       // (rows >= np: h = 0 there, so g = 0)
        out[row * so + col] = v;
        if (outT) outT[col * kP64 + row] = v;
    }
}

__global__ __launch_bounds__(kBT) void pose_bwd_cloud_kernel(const float* __restrict__ ptsA, const float* __restrict__ ptsB, int nA, int N,
                                                              PointNetW net, const float* __restrict__ g4g, PointSave sv,
                                                              float* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* G = lds + kMG;
    float* GT = lds + kMGT;
    float* HT = lds + kMHT;
    float* WT = lds + kMWT;
    float* GA = lds + kMGA;
    float* GAT = lds + kMGAT;
    float* sp = lds + kMPts;
    // workgroup = (cloud, 64-point chunk): chunk-major records, NW per cloud; rows at or beyond np stay zero
    const int NW = (N + 63) / 64;
    const int c = (int)blockIdx.x / NW, p0 = ((int)blockIdx.x % NW) * 64, t = threadIdx.x;
    const int np = min(64, N - p0);
    const float* pts = (c < nA ? ptsA + (size_t)c * N * 3 : ptsB + (size_t)(c - nA) * N * 3) + (size_t)p0 * 3;
    const size_t prow = (size_t)c * N + p0;                  // first row of the chunk in g4g / h1..h3
    float* out = part + (size_t)blockIdx.x * kPart;
    // layer 4 (W4 [128 o][64 i]): g4 -> G [p][o], GT [o][p]; h3 -> HT [i][p]; W4 -> WT [i][o]
    lds_load_t(g4g + prow * 128, np, 64, 128, GT, kP64, G, kP128, t);
    lds_load_t(sv.h[2] + prow * 64, np, 64, 64, HT, kP64, nullptr, 0, t);
    lds_load_t(net.W[3], 128, 128, 64, WT, kP128, nullptr, 0, t);
    if (t < 192) sp[(t / 3) * 4 + t % 3] = (t / 3) < np ? pts[t] : 0.f;
    Pre64 ph = pre64_load(sv.h[1] + prow * 64, np, t), pw = pre64_load(net.W[2], 64, t);      // layer 3's operands, in flight
    __syncthreads();
    bwd_layer_dw<128>(GT, HT, out, out + 128 * 64, np, t);
    bwd_layer_dx<128>(G, kP128, WT, kP128, HT, GA, kP64, GAT, t);                      // g3 -> GA [p][o3], GAT [o3][p]
    __syncthreads();
    // layer 3 (W3 [64][64]): h2 -> HT, W3 -> WT (stride 68)
    pre64_store_t(ph, HT, t);
    pre64_store_t(pw, WT, t);
    ph = pre64_load(sv.h[0] + prow * 64, np, t);                                              // layer 2's
    pw = pre64_load(net.W[1], 64, t);
    __syncthreads();
    float* o3 = out + 128 * 64 + 128;
    bwd_layer_dw<64>(GAT, HT, o3, o3 + 64 * 64, np, t);
    bwd_layer_dx<64>(GA, kP64, WT, kP64, HT, G, kP64, GT, t);                          // g2 -> G [p][o2] (stride 68), GT [o2][p]
    __syncthreads();
    // layer 2 (W2 [64][64]): h1 -> HT, W2 -> WT
    pre64_store_t(ph, HT, t);
    pre64_store_t(pw, WT, t);
    __syncthreads();
    float* o2 = o3 + 64 * 64 + 64;
    bwd_layer_dw<64>(GT, HT, o2, o2 + 64 * 64, np, t);
    bwd_layer_dx<64>(G, kP64, WT, kP64, HT, GA, kP64, nullptr, t);                     // g1 -> GA [p][o1]
    __syncthreads();
    // layer 1 (64 x 3): dW1[o][i] = sum_p g1[p][o] pts[p][i], db1
    float* o1 = o2 + 64 * 64 + 64;
    if (t < 64) {
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, bs = 0.f;
        for (int p = 0; p < np; ++p) {
            const float a = GA[p * kP64 + t];
            bs += a; a0 += a * sp[p * 4]; a1 += a * sp[p * 4 + 1]; a2 += a * sp[p * 4 + 2];
        }
        o1[t * 3] = a0; o1[t * 3 + 1] = a1; o1[t * 3 + 2] = a2;
        o1[192 + t] = bs;
    }
}

__global__ __launch_bounds__(256) void pose_bwd_reduce_kernel(const float* __restrict__ part, int C, float* __restrict__ dW4, float* __restrict__ db4,
                                                               float* __restrict__ dW3, float* __restrict__ db3, float* __restrict__ dW2,
                                                               float* __restrict__ db2, float* __restrict__ dW1, float* __restrict__ db1) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= kPart) return;
    float s = 0.f;
    int c = 0;
    for (; c + 8 <= C; c += 8) {                       // eight clouds' records requested together; added in cloud order
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = part[(size_t)(c + u) * kPart + i];
#pragma unroll
        for (int u = 0; u < 8; ++u) s += v[u];
    }
    for (; c < C; ++c) s += part[(size_t)c * kPart + i];
    int k = i;
    if (k < 128 * 64) { dW4[k] = s; return; }
    k -= 128 * 64;
    if (k < 128) { db4[k] = s; return; }
    k -= 128;
    if (k < 64 * 64) { dW3[k] = s; return; }
    k -= 64 * 64;
    if (k < 64) { db3[k] = s; return; }
    k -= 64;
    if (k < 64 * 64) { dW2[k] = s; return; }
    k -= 64 * 64;
    if (k < 64) { db2[k] = s; return; }
    k -= 64;
    if (k < 192) { dW1[k] = s; return; }
    k -= 192;
    db1[k] = s;
}

// ---- the average pool (models/ipcr_model.py:236-271): f = sum over the points of relu(layer 5) / N, so EVERY point whose ReLU gate is open
// carries the gradient coef[c, col] = df[c, col] / (float)N -- about half of all (point, column) entries, and dW5 is a real
// [1024, C N] x [C N, 128] product:  g5[c, p, col] = gate ? coef[c, col] : 0,  dW5[col, :] = sum over (cloud, point) of g5 h4[point, :].
//   pose_avg_coef_kernel    coef [C, OUT] (one IEEE division per entry) and bterm [C, OUT] = coef * popcount(the (cloud, column)'s gate words)
//   pose_bwd_w5_dh4_kernel  its g4 role only, with coefg = coef (also at NW == 1): g4 = S W5 costs the same whatever S holds
//   pose_avg_dw5_kernel     the product on v_mfma_f32_32x32x2_f32, partials per split of the (cloud, chunk) range
//   pose_avg_reduce_kernel  dW5 = the partials added in ascending split order; db5[col] = bterm[:, col] added clouds ascending
// Every sum has one order (below): bitwise reproducible, no atomics.
constexpr int kAvgCols = 128;          // columns of dW5 per workgroup: four waves x 32
constexpr int kAvgMaxSplit = 32;       // (OUT / kAvgCols = 8 column blocks) x 32 splits = 256 workgroups, one per CU

inline int avg_splits(int chunks) { return chunks < kAvgMaxSplit ? chunks : kAvgMaxSplit; }      // every split owns at least one chunk

__global__ __launch_bounds__(256) void pose_avg_coef_kernel(const float* __restrict__ df, const unsigned long long* __restrict__ gates, int C, int NW,
                                                             int N, int OUT, float* __restrict__ coef, float* __restrict__ bterm) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= C * OUT) return;
    const int c = i / OUT, col = i % OUT;
    int cnt = 0;
    for (int w = 0; w < NW; ++w) cnt += __popcll(gates[((size_t)c * NW + w) * OUT + col]);
    const float cf = df[i] / (float)N;
    coef[i] = cf;
    bterm[i] = cf * (float)cnt;
}

// One 64-point chunk of h4 in flight: thread t holds float4 q of rows (t >> 5) + 8 q, columns 4 (t & 31) .. + 3, and its column's gate word and
// coefficient.  Rows at or beyond the cloud's last point are ZERO (their gate bits are 0, but 0 x the next cloud's value must stay 0 and the
// last cloud's chunk ends where h4 ends).
struct AvgChunk {
    float4 v[8];
    unsigned long long gate;
    float coef;
};
__device__ __forceinline__ void avg_chunk_load(AvgChunk& x, const float* __restrict__ h4, const unsigned long long* __restrict__ gates,
                                               const float* __restrict__ coef, int ch, int NW, int N, int OUT, int col, int t) {
    const int c = ch / NW, w = ch % NW, np = min(64, N - 64 * w);
    const float* src = h4 + ((size_t)c * N + 64 * w) * 128;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int r = (t >> 5) + 8 * q;
        x.v[q] = r < np ? *reinterpret_cast<const float4*>(src + (size_t)r * 128 + 4 * (t & 31)) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    x.gate = gates[((size_t)c * NW + w) * OUT + col];
    x.coef = coef[(size_t)c * OUT + col];
}

// Workgroup = (column block cb of 128 columns, split sp of the C NW (cloud, chunk)s: chunks [sp CH / S, (sp + 1) CH / S), ascending); wave = 32
// columns x all 128 inputs = four 32x32 accumulators.  Per chunk the h4 rows [64, 128] are staged in LDS ONCE (float4 writes, 32 KiB) and shared
// by the four waves; the A operand is not a matrix in memory: lane (i = l & 31, half = l >> 5) builds A[column i][k = half] of step j -- point
// 2 j + half of the chunk -- from its column's gate word and coefficient (bit ? coef : 0), and reads B[k][input] = h4[point][32 n + i] as one
// ds_read_b32 per product (the two lane halves read two rows: no bank conflict; 256 B of LDS per 64-cycle MFMA).  The next chunk's rows, gate
// word and coefficient are requested before the 128 products of the current one and written to LDS after them.
// Order of every dW5 element's sum: an fp32 fmaf chain over the points of a chunk ascending, chunks ascending inside the split (cloud-major),
// then the splits ascending in pose_avg_reduce_kernel.
__global__ __launch_bounds__(256) void pose_avg_dw5_kernel(const float* __restrict__ coef, const unsigned long long* __restrict__ gates,
                                                            const float* __restrict__ h4, int C, int N, int OUT, int S, float* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) float sH[64 * 128];
    const int ncb = OUT / kAvgCols;
    const int cb = (int)blockIdx.x % ncb, sp = (int)blockIdx.x / ncb;
    const int NW = (N + 63) / 64, CH = C * NW;
    const int ch0 = (int)((long long)sp * CH / S), ch1 = (int)((long long)(sp + 1) * CH / S);
    const int t = threadIdx.x, wv = t >> 6, l = t & 63, i = l & 31, h = l >> 5;
    const int col = cb * kAvgCols + wv * 32 + i;
    f32x16 acc[4];
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[n][r] = 0.f;
    AvgChunk nx;
    avg_chunk_load(nx, h4, gates, coef, ch0, NW, N, OUT, col, t);
    for (int ch = ch0; ch < ch1; ++ch) {
        __syncthreads();                                   // the previous chunk's products are done with sH
#pragma unroll
        for (int q = 0; q < 8; ++q) *reinterpret_cast<float4*>(sH + ((t >> 5) + 8 * q) * 128 + 4 * (t & 31)) = nx.v[q];
        const unsigned long long g = nx.gate >> h;         // bit 2 j: point 2 j + half
        const unsigned glo = (unsigned)g, ghi = (unsigned)(g >> 32);
        const float cf = nx.coef;
        __syncthreads();
        if (ch + 1 < ch1) avg_chunk_load(nx, h4, gates, coef, ch + 1, NW, N, OUT, col, t);
        const float* bp = sH + h * 128 + i;
#pragma unroll
        for (int j = 0; j < 32; ++j) {
            const unsigned bit = j < 16 ? (glo >> (2 * j)) & 1u : (ghi >> (2 * j - 32)) & 1u;
            const float a = bit ? cf : 0.f;
#pragma unroll
            for (int n = 0; n < 4; ++n) acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bp[j * 256 + 32 * n], acc[n], 0, 0, 0);
        }
    }
    float* out = part + ((size_t)sp * OUT + cb * kAvgCols + wv * 32) * 128;
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) out[(size_t)mfma_row(r, l) * 128 + 32 * n + i] = acc[n][r];
}

// threads [0, OUT * 128): dW5 element = partials of the S splits, ascending; threads [OUT * 128, OUT * 128 + OUT): db5 = bterm over the clouds, ascending
__global__ __launch_bounds__(256) void pose_avg_reduce_kernel(const float* __restrict__ part, int S, const float* __restrict__ bterm, int C, int OUT,
                                                               float* __restrict__ dW5, float* __restrict__ db5) {
    const int i = blockIdx.x * 256 + threadIdx.x, n = OUT * 128;
    if (i < n) {
        float s = part[i];
        for (int sp = 1; sp < S; ++sp) s += part[(size_t)sp * n + i];
        dW5[i] = s;
        return;
    }
    const int col = i - n;
    if (col >= OUT) return;
    float s = bterm[col];
    for (int c = 1; c < C; ++c) s += bterm[(size_t)c * OUT + col];
    db5[col] = s;
}

}  // namespace dpd

// partial weight gradients per (cloud, 64-point chunk) + g4 [clouds * chunks * 64, 128] (+ coef [clouds, OUT] when a cloud has several chunks)
extern "C" size_t dpd_pose_point_bwd_workspace_bytes_n(int clouds, int N) {
    if (clouds <= 0 || N <= 0 || N > dpd::kTrainMaxN) return 0;
    const size_t W = (size_t)dpd_pose_point_tie_words(N);
    return ((size_t)clouds * W * (dpd::kPart + 64 * 128) + (W > 1 ? (size_t)clouds * 1024 : 0)) * sizeof(float);
}

extern "C" size_t dpd_pose_point_bwd_workspace_bytes(int clouds) { return dpd_pose_point_bwd_workspace_bytes_n(clouds, dpd::kPP); }      // N <= 64

// average pool: the records and g4 as above, then coef [clouds, OUT], bterm [clouds, OUT] and the dW5 partials [splits, OUT, 128]
extern "C" size_t dpd_pose_point_bwd_workspace_bytes_pool(int clouds, int N, int pool) {
    if (pool == DPD_POOL_MAX) return dpd_pose_point_bwd_workspace_bytes_n(clouds, N);
    if (pool != DPD_POOL_AVG || clouds <= 0 || N <= 0 || N > dpd::kTrainMaxN) return 0;
    const size_t W = (size_t)dpd_pose_point_tie_words(N);
    return ((size_t)clouds * W * (dpd::kPart + 64 * 128) + (size_t)clouds * 1024 * 2 + (size_t)dpd::avg_splits((int)(clouds * W)) * 1024 * 128) * sizeof(float);
}

extern "C" int dpd_pose_point_bwd(const dpd_pose_net* net, const float* ptsA, const float* ptsB, int nA, int nB, int N, const float* df,
                                  const float* h1, const float* h2, const float* h3, const float* h4, const unsigned long long* ties,
                                  float* const* dW, float* const* db, void* ws, size_t ws_bytes, void* stream) {
    return dpd_pose_point_bwd_pool(net, ptsA, ptsB, nA, nB, N, DPD_POOL_MAX, df, h1, h2, h3, h4, ties, dW, db, ws, ws_bytes, stream);
}

extern "C" int dpd_pose_point_bwd_pool(const dpd_pose_net* net, const float* ptsA, const float* ptsB, int nA, int nB, int N, int pool, const float* df,
                                       const float* h1, const float* h2, const float* h3, const float* h4, const unsigned long long* words,
                                       float* const* dW, float* const* db, void* ws, size_t ws_bytes, void* stream) {
    using namespace dpd;
    if (int rc = check_point_layers(net)) return rc;
    if (net->out_features != 1024) return DPD_E_UNSUPPORTED;
    if (!ptsA || (nB > 0 && !ptsB) || !df || !h1 || !h2 || !h3 || !h4 || !words || !dW || !db || !ws) return DPD_E_NULL;
    for (int i = 0; i < 5; ++i)
        if (!dW[i] || !db[i]) return DPD_E_NULL;
    if (nA <= 0 || nB < 0 || N <= 0) return DPD_E_DIM;
    if (!pool_known(pool)) return DPD_E_UNSUPPORTED;
    if (N > kTrainMaxN) return DPD_E_UNSUPPORTED;
    const bool avg = pool == DPD_POOL_AVG;
    if (avg && ((uintptr_t)h4 & 15) != 0) return DPD_E_UNSUPPORTED;      // pose_avg_dw5_kernel reads h4 in 16-byte pieces
    const int C = nA + nB, OUT = net->out_features, NW = dpd_pose_point_tie_words(N);
    if (ws_bytes < dpd_pose_point_bwd_workspace_bytes_pool(C, N, pool)) return DPD_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const PointNetW pw = point_net_of(net);
    PointSave sv{{const_cast<float*>(h1), const_cast<float*>(h2), const_cast<float*>(h3), const_cast<float*>(h4)},
                 const_cast<unsigned long long*>(words)};
    const size_t lds = (size_t)kBwdLds * sizeof(float);
    static LdsOptIn cloud_opt_in;                          // of pose_bwd_cloud_kernel, launched here only
    if (int rc = ensure_dyn_lds(cloud_opt_in, (const void*)pose_bwd_cloud_kernel, lds)) return rc;
    float* g4g = (float*)ws + (size_t)C * NW * kPart;              // [C * N, 128]
    float* coef = (NW > 1 || avg) ? g4g + (size_t)C * NW * 64 * 128 : nullptr;      // [C, OUT]
    const int tiles = NW > 1 ? 4 * ((N + 31) / 32) : 8;            // 32 points x 32 inputs each
    if (avg) {
        float* bterm = coef + (size_t)C * OUT;                     // [C, OUT]
        float* part = bterm + (size_t)C * OUT;                     // [S, OUT, 128]
        const int S = avg_splits(C * NW);
        DPD_LAUNCH(pose_avg_coef_kernel, dim3((unsigned)((C * OUT + 255) / 256)), dim3(256), 0, s, df, words, C, NW, N, OUT, coef, bterm);
        DPD_CHECK_LAUNCH();
        // the g4 role alone (no dW5 / db5 blocks): S = the gate bits, coefg = coef also where a cloud has one chunk
        DPD_LAUNCH(pose_bwd_w5_dh4_kernel, dim3((unsigned)(C * tiles)), dim3(512), 0, s, df, words, net->Wp[4], h4, C, N, OUT, g4g, dW[4], db[4], tiles,
                   (const float*)coef);
        DPD_CHECK_LAUNCH();
        DPD_LAUNCH(pose_avg_dw5_kernel, dim3((unsigned)(OUT / kAvgCols * S)), dim3(256), 0, s, (const float*)coef, words, h4, C, N, OUT, S, part);
        DPD_CHECK_LAUNCH();
        DPD_LAUNCH(pose_avg_reduce_kernel, dim3((unsigned)((OUT * 128 + OUT + 255) / 256)), dim3(256), 0, s, (const float*)part, S, (const float*)bterm, C, OUT,
                   dW[4], db[4]);
        DPD_CHECK_LAUNCH();
    } else {
        if (coef) {
            DPD_LAUNCH(pose_tie_coef_kernel, dim3((unsigned)((C * OUT + 255) / 256)), dim3(256), 0, s, df, words, C, NW, OUT, coef);
            DPD_CHECK_LAUNCH();
        }
        DPD_LAUNCH(pose_bwd_w5_dh4_kernel, dim3((unsigned)(C * tiles + (OUT + 7) / 8)), dim3(512), 0, s, df, words, net->Wp[4], h4, C, N, OUT, g4g, dW[4],
                   db[4], tiles, (const float*)coef);
        DPD_CHECK_LAUNCH();
    }
    DPD_LAUNCH(pose_bwd_cloud_kernel, dim3((unsigned)(C * NW)), dim3(kBT), lds, s, ptsA, ptsB, nA, N, pw, (const float*)g4g, sv, (float*)ws);
    DPD_CHECK_LAUNCH();
    DPD_LAUNCH(pose_bwd_reduce_kernel, dim3((unsigned)((kPart + 255) / 256)), dim3(256), 0, s, (const float*)ws, C * NW, dW[3], db[3], dW[2], db[2], dW[1],
               db[1], dW[0], db[0]);
    DPD_CHECK_LAUNCH();
    return 0;
}

// Head of the pose network (what the units of the pose network share: pose_int.h).
// models/ipcr_model.py:273-284: fc 2048 -> 1024 -> 512 -> 256 (ReLU each, dropout on the last) -> 7, and TF / torch autodiff of it:
//   forward   pose_fc_kernel x 3 (launch_pose_fc: the training evaluation here keeps the hidden activations; the forward-only refinement of
//             pose.hip calls the same launcher), pose_fc4_fwd_kernel
//   backward  pose_fc4_bwd_kernel: gradient of the 256-wide activation (dropout mask and ReLU gate applied) + dW4 / db4
//             pose_fc_dw3_kernel (dW = g^T x, db of the three wide layers in one launch: 16 terms per entry, bound by the 8 MB fc1 writes), per layer
//             pose_fc_dx_kernel (gx = (g W) * [x > 0] on v_mfma_f32_16x16x4_f32; the weight is streamed once: 16 input columns per workgroup,
//             sixteen waves each contracting a sixteenth of the outputs, partial tiles added in wave order -- 128 / 64 / 32 workgroups)
#include "pose_int.h"

namespace dpd {

// out[r, j] = act(sum_k in[r, k] W[j, k] + bias[j]) (* mask[r, j]) for <= 16 rows per blockIdx.y; in = [inA (KA columns) | inB (K - KA)]
// (the head's first layer reads cat(source feature, template feature) without materialising it).
// One workgroup of 16 waves per 16 output columns: wave w takes K / 16 of the reduction, NIT = K / 256 steps of 16 k each; per step every
// lane loads ONE float4 of W (row j0 + lane % 16, columns k + 4 (lane / 16) .. + 3) and one of `in` (row lane % 16, same columns) and
// issues four v_mfma_f32_16x16x4_f32 (element s of both float4s: A[i][kk] = W[j0 + i][.], B[kk][n] = in[n][.], same k on both sides).
// All 2 NIT loads of a lane are in flight at once; the 16 partial tiles are added in wave order through LDS (deterministic).
typedef float f32x4 __attribute__((ext_vector_type(4)));
template <int NIT>
__global__ __launch_bounds__(1024) void pose_fc_kernel(const float* __restrict__ inA, const float* __restrict__ inB, int KA,
                                                       const float* __restrict__ W, const float* __restrict__ bias, int J, int R, int relu,
                                                       const float* __restrict__ mask, float* __restrict__ out, int ldw,
                                                       const float* __restrict__ rowbias) {
    constexpr int K = NIT * 256;
    __shared__ float part[16][256];
    const int j0 = blockIdx.x * 16, r0 = blockIdx.y * 16, wv = threadIdx.x >> 6, l = threadIdx.x & 63;
    const int n = l & 15, kk = l >> 4;
    const int row = min(r0 + n, R - 1);
    const int kw = wv * (K / 16);                              // this wave's K range: [kw, kw + 16 NIT)
    const float* x = kw < KA ? inA + (size_t)row * KA + kw : inB + (size_t)row * (K - KA) + (kw - KA);
    const float* w = W + (size_t)(j0 + n) * ldw + kw;       // ldw >= K: a column block of a wider weight matrix
    // the epilogue's element (threads 0..255) and what it needs from global memory, requested with the operands
    const int e = threadIdx.x, el = e >> 2, er = e & 3, en = el & 15, ej = j0 + 4 * (el >> 4) + er, orow = r0 + en;
    const bool live = e < 256 && orow < R && ej < J;
    const float bj = live ? (rowbias ? rowbias[(size_t)orow * J + ej] : bias[ej]) : 0.f;      // rowbias [R][J]: a precomputed part of the sum
    const float mk = (live && mask) ? mask[(size_t)orow * J + ej] : 1.f;
    float4 wr[NIT], xr[NIT];
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
        wr[i] = *reinterpret_cast<const float4*>(w + 16 * i + 4 * kk);
        xr[i] = *reinterpret_cast<const float4*>(x + 16 * i + 4 * kk);
    }
    f32x4 c = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
        c = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[i].x, xr[i].x, c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[i].y, xr[i].y, c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[i].z, xr[i].z, c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[i].w, xr[i].w, c, 0, 0, 0);
    }
    // lane l holds C[j = 4 (l / 16) + r][n = l % 16], r = 0..3
#pragma unroll
    for (int r = 0; r < 4; ++r) part[wv][l * 4 + r] = c[r];
    __syncthreads();
    if (live) {
        float v = part[0][e];
#pragma unroll
        for (int q = 1; q < 16; ++q) v += part[q][e];
        v += bj;
        if (relu) v = fmaxf(v, 0.f);
        if (mask) v *= mk;
        out[(size_t)orow * J + ej] = v;
    }
}

// pred[b][o] = sum_k h3[b][k] W4[o][k] + b4[o], o < 7, K4 = 256: one wave per row
__global__ __launch_bounds__(64) void pose_fc4_fwd_kernel(const float* __restrict__ h3, const float* __restrict__ W4, const float* __restrict__ b4,
                                                           int K4, float* __restrict__ pred) {
    const int b = blockIdx.x, l = threadIdx.x;
    float acc[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int k = l; k < K4; k += 64) {
        const float x = h3[(size_t)b * K4 + k];
#pragma unroll
        for (int o = 0; o < 7; ++o) acc[o] += x * W4[(size_t)o * K4 + k];
    }
#pragma unroll
    for (int o = 0; o < 7; ++o) {
        float v = acc[o];
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s, 64);
        if (l == 0) pred[(size_t)b * 7 + o] = v + b4[o];
    }
}

// blocks [0, B): g3[b][k] = (sum_o dpred[b][o] W4[o][k]) * mask[b][k] * [h3[b][k] > 0]; block B: dW4[o][k] = sum_b dpred[b][o] h3[b][k], db4
__global__ __launch_bounds__(256) void pose_fc4_bwd_kernel(const float* __restrict__ dpred, const float* __restrict__ W4, const float* __restrict__ h3,
                                                            const float* __restrict__ mask, int B, int K4, float* __restrict__ g3,
                                                            float* __restrict__ dW4, float* __restrict__ db4) {
    const int t = threadIdx.x;
    if ((int)blockIdx.x < B) {
        const int b = blockIdx.x;
        float d[7];
#pragma unroll
        for (int o = 0; o < 7; ++o) d[o] = dpred[(size_t)b * 7 + o];
        for (int k = t; k < K4; k += 256) {
            float v = 0.f;
#pragma unroll
            for (int o = 0; o < 7; ++o) v += d[o] * W4[(size_t)o * K4 + k];
            if (mask) v *= mask[(size_t)b * K4 + k];
            g3[(size_t)b * K4 + k] = h3[(size_t)b * K4 + k] > 0.f ? v : 0.f;
        }
        return;
    }
    // workgroup B + o: row o of dW4 (and db4[o]); the batch's terms are requested eight at a time and added in batch order
    const int o = blockIdx.x - B;
    for (int k = t; k < K4; k += 256) {
        float v = 0.f;
        int b = 0;
        for (; b + 8 <= B; b += 8) {
            float d[8], hh[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) { d[u] = dpred[(size_t)(b + u) * 7 + o]; hh[u] = h3[(size_t)(b + u) * K4 + k]; }
#pragma unroll
            for (int u = 0; u < 8; ++u) v += d[u] * hh[u];
        }
        for (; b < B; ++b) v += dpred[(size_t)b * 7 + o] * h3[(size_t)b * K4 + k];
        dW4[(size_t)o * K4 + k] = v;
    }
    if (t == 0) {
        float v = 0.f;
        for (int b = 0; b < B; ++b) v += dpred[(size_t)b * 7 + o];
        db4[o] = v;
    }
}

// dW[j][k] = sum_r g[r][j] x[r][k] (r ascending), db[j] = sum_r g[r][j].  x = [xA (KA columns) | xB (K - KA)] like pose_fc_kernel's input.
// block = 16 output rows x 256 columns: thread = (four rows j, one float4 of columns)
struct FcDwJob {               // dW [J,K] = g^T [J,R] x [R,K] (x = [xA | xB], xA KA columns wide), db [J]; K / 256 x J / 64 blocks
    const float* g;
    const float* xA;
    const float* xB;
    float* dW;
    float* db;
    int KA, J, K;
    int blocks;                 // (K / 256) * (J / 64)
};
__device__ __forceinline__ void fc_dw_block(const float* __restrict__ g, const float* __restrict__ xA, const float* __restrict__ xB, int KA, int J,
                                            int K, int R, float* __restrict__ dW, float* __restrict__ db, int bx, int by) {
    // block = 64 outputs j x 256 inputs k: wave w = outputs 16 w .. + 15 (its g values are wave-uniform: scalar loads), lane = four inputs.
    // The first sixteen rows of x stay in registers for all sixteen outputs (one round of loads; a thread of the 4 j x 4 k form re-read them
    // four times as often: 43 MB of L2 traffic for fc1); further rows (batch > 16) are read again per group of outputs.
    const int t = threadIdx.x, kq = t & 63, jg = __builtin_amdgcn_readfirstlane(t >> 6);
    const int k = bx * 256 + 4 * kq, jw = by * 64 + 16 * jg;
    if (k >= K) return;
    const float* x = k < KA ? xA + k : xB + (k - KA);
    const int ldx = k < KA ? KA : K - KA;
    float4 xr[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) xr[r] = r < R ? *reinterpret_cast<const float4*>(x + (size_t)r * ldx) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 1
    for (int jc = 0; jc < 4; ++jc) {
        const int j0 = jw + 4 * jc;
        float4 acc[4];
        float bs[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[u] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float4 gv = r < R ? *reinterpret_cast<const float4*>(g + (size_t)r * J + j0) : make_float4(0.f, 0.f, 0.f, 0.f);
            const float gg[4] = {gv.x, gv.y, gv.z, gv.w};
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                acc[u].x += gg[u] * xr[r].x; acc[u].y += gg[u] * xr[r].y; acc[u].z += gg[u] * xr[r].z; acc[u].w += gg[u] * xr[r].w;
                bs[u] += gg[u];
            }
        }
        for (int r = 16; r < R; ++r) {
            const float4 xv = *reinterpret_cast<const float4*>(x + (size_t)r * ldx);
            const float4 gv = *reinterpret_cast<const float4*>(g + (size_t)r * J + j0);
            const float gg[4] = {gv.x, gv.y, gv.z, gv.w};
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                acc[u].x += gg[u] * xv.x; acc[u].y += gg[u] * xv.y; acc[u].z += gg[u] * xv.z; acc[u].w += gg[u] * xv.w;
                bs[u] += gg[u];
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) *reinterpret_cast<float4*>(dW + (size_t)(j0 + u) * K + k) = acc[u];
        if (bx == 0 && kq == 0) {
#pragma unroll
            for (int u = 0; u < 4; ++u) db[j0 + u] = bs[u];
        }
    }
}
// the three wide layers' weight gradients in ONE launch (they depend on g3, g2, g1 only: after the second dx launch, beside nothing else --
// three launches of 7-8 us each were mostly launch ramp): block ranges [0, n0) fc3, [n0, n0 + n1) fc2, the rest fc1 (8 + 32 + 128 blocks)
__global__ __launch_bounds__(256) void pose_fc_dw3_kernel(FcDwJob a, FcDwJob b, FcDwJob c, int R) {
    int id = blockIdx.x;
    const FcDwJob* j = &a;
    if (id >= a.blocks) { id -= a.blocks; j = &b; }
    if (j == &b && id >= b.blocks) { id -= b.blocks; j = &c; }
    const int nbx = j->K / 256;
    fc_dw_block(j->g, j->xA, j->xB, j->KA, j->J, j->K, R, j->dW, j->db, id % nbx, id / nbx);
}

// gx[r][k] = (sum_j g[r][j] W[j][k]) * [xprev[r][k] > 0] for <= 16 rows per blockIdx.y and the 64 columns k0 .. k0 + 63 of blockIdx.x.
// Eight waves share the reduction (wave w: j in [w J / 8, (w + 1) J / 8), NIT = J / 32 steps of four j); per step a lane loads ONE float4 of W
// (row j0 + lane / 16, columns k0 + 4 (lane % 16) .. + 3) and one g value (row r0 + lane % 16, column j0 + lane / 16) and issues four
// v_mfma_f32_16x16x4_f32: A_e[i][kk] = W[j0 + kk][k0 + 4 i + e], B[kk][n] = g[r0 + n][j0 + kk] -> C_e[i][n] = partial gx[r0 + n][k0 + 4 i + e].
// A lane then holds the 16 consecutive columns k0 + 16 (lane / 16) .. + 15 of row r0 + lane % 16; the eight partial tiles are added in wave
// order through LDS (deterministic).  xprev == NULL: no gate (the pooled features).  out rows: row r -> out + r * ldo (+ column k); for the
// first layer the columns >= split go to the rows of the second cloud set: out[(R + r) * ldo + k - split].
template <int NIT>
__global__ __launch_bounds__(1024) void pose_fc_dx_kernel(const float* __restrict__ g, const float* __restrict__ W, const float* __restrict__ xprev,
                                                           int K, int R, float* __restrict__ out, int ldo, int split) {
    constexpr int J = NIT * 64;
    __shared__ float part[16][256];
    const int k0 = blockIdx.x * 16, r0 = blockIdx.y * 16, wv = threadIdx.x >> 6, l = threadIdx.x & 63;
    const int n = l & 15, kk = l >> 4;
    const int row = min(r0 + n, R - 1);
    const int jw = wv * (J / 16);
    // the epilogue's element (threads 0..255): row r0 + (t / 4) % 16, column k0 + 4 (t / 64) + t % 4; its ReLU gate is requested with the operands
    const int et = threadIdx.x, err = r0 + ((et >> 2) & 15), ek = k0 + 4 * (et >> 6) + (et & 3);
    const float gate = (et < 256 && err < R && xprev) ? xprev[(size_t)err * K + ek] : 1.f;
    float wr[NIT], gr[NIT];
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
        wr[i] = W[(size_t)(jw + 4 * i + kk) * K + k0 + n];
        gr[i] = g[(size_t)row * J + jw + 4 * i + kk];
    }
    f32x4 c = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < NIT; ++i) c = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[i], gr[i], c, 0, 0, 0);
    // lane l holds C[i = 4 (l / 16) + r][n = l % 16]: column k0 + i of row n
#pragma unroll
    for (int r = 0; r < 4; ++r) part[wv][l * 4 + r] = c[r];
    __syncthreads();
    if (et < 256) {
        float v = part[0][et];
#pragma unroll
        for (int q = 1; q < 16; ++q) v += part[q][et];
        if (err < R) {
            if (!(gate > 0.f)) v = 0.f;
            if (ek < split) out[(size_t)err * ldo + ek] = v;
            else out[(size_t)(R + err) * ldo + ek - split] = v;
        }
    }
}

}  // namespace dpd

int dpd::check_head_layers(const dpd_pose_net* net, bool biases) {
    if (!net) return DPD_E_NULL;
    for (int i = 0; i < 4; ++i)
        if (!net->Wh[i] || (biases && !net->bh[i])) return DPD_E_NULL;
    return 0;
}

int dpd::launch_pose_fc(const dpd_pose_net* net, int layer, FcIn in, int wcol0, const float* rowbias, bool relu, const float* mask, float* out, int R,
                        hipStream_t s) {
    static const int kWidth[4] = {2048, 1024, 512, 256};           // layer l: Wh[l] is [kWidth[l + 1], kWidth[l]]
    const int J = kWidth[layer + 1], ldw = kWidth[layer];
    const dim3 grid((unsigned)(J / 16), (unsigned)((R + 15) / 16));
    const float* W = net->Wh[layer] + wcol0;
    const float* bias = net->bh[layer];
    switch (in.K) {
        case 512: DPD_LAUNCH(pose_fc_kernel<2>, grid, dim3(1024), 0, s, in.A, in.B, in.KA, W, bias, J, R, (int)relu, mask, out, ldw, rowbias); break;
        case 1024: DPD_LAUNCH(pose_fc_kernel<4>, grid, dim3(1024), 0, s, in.A, in.B, in.KA, W, bias, J, R, (int)relu, mask, out, ldw, rowbias); break;
        case 2048: DPD_LAUNCH(pose_fc_kernel<8>, grid, dim3(1024), 0, s, in.A, in.B, in.KA, W, bias, J, R, (int)relu, mask, out, ldw, rowbias); break;
        default: return DPD_E_UNSUPPORTED;
    }
    DPD_CHECK_LAUNCH();
    return 0;
}

extern "C" int dpd_pose_head_fwd_train(const dpd_pose_net* net, const float* f, int B, const float* drop_mask, float* h1, float* h2, float* h3,
                                       float* pred, void* stream) {
    using namespace dpd;
    if (!net || !f || !h1 || !h2 || !h3 || !pred) return DPD_E_NULL;
    if (int rc = check_head_layers(net, true)) return rc;
    if (B <= 0) return DPD_E_DIM;
    if (net->out_features != 1024) return DPD_E_UNSUPPORTED;
    const int OUT = 1024;
    hipStream_t s = (hipStream_t)stream;
    if (int rc = launch_pose_fc(net, 0, FcIn{f, f + (size_t)B * OUT, OUT, 2 * OUT}, /*wcol0*/ 0, /*rowbias*/ nullptr, /*relu*/ true, /*mask*/ nullptr, h1, B, s)) return rc;
    if (int rc = launch_pose_fc(net, 1, FcIn{h1, nullptr, 1024, 1024}, /*wcol0*/ 0, /*rowbias*/ nullptr, /*relu*/ true, /*mask*/ nullptr, h2, B, s)) return rc;
    if (int rc = launch_pose_fc(net, 2, FcIn{h2, nullptr, 512, 512}, /*wcol0*/ 0, /*rowbias*/ nullptr, /*relu*/ true, /*mask*/ drop_mask, h3, B, s)) return rc;
    DPD_LAUNCH(pose_fc4_fwd_kernel, dim3((unsigned)B), dim3(64), 0, s, (const float*)h3, net->Wh[3], net->bh[3], 256, pred);
    DPD_CHECK_LAUNCH();
    return 0;
}

extern "C" size_t dpd_pose_head_bwd_workspace_bytes(int B) { return B > 0 ? (size_t)B * (256 + 512 + 1024) * sizeof(float) : 0; }

extern "C" int dpd_pose_head_bwd(const dpd_pose_net* net, const float* f, int B, const float* drop_mask, const float* h1, const float* h2,
                                 const float* h3, const float* dpred, float* const* dW, float* const* db, float* df, void* ws, size_t ws_bytes,
                                 void* stream) {
    using namespace dpd;
    if (!net || !f || !h1 || !h2 || !h3 || !dpred || !dW || !db || !df || !ws) return DPD_E_NULL;
    if (int rc = check_head_layers(net, false)) return rc;      // the backward reads no bias
    for (int i = 0; i < 4; ++i)
        if (!dW[i] || !db[i]) return DPD_E_NULL;
    if (B <= 0) return DPD_E_DIM;
    if (net->out_features != 1024) return DPD_E_UNSUPPORTED;
    if (ws_bytes < dpd_pose_head_bwd_workspace_bytes(B)) return DPD_E_WORKSPACE;
    const int OUT = 1024;
    hipStream_t s = (hipStream_t)stream;
    float* g3 = (float*)ws;                  // [B, 256]
    float* g2 = g3 + (size_t)B * 256;        // [B, 512]
    float* g1 = g2 + (size_t)B * 512;        // [B, 1024]
    const unsigned ry = (unsigned)((B + 15) / 16);
    DPD_LAUNCH(pose_fc4_bwd_kernel, dim3((unsigned)B + 7), dim3(256), 0, s, dpred, net->Wh[3], h3, drop_mask, B, 256, g3, dW[3], db[3]);
    DPD_CHECK_LAUNCH();
    // fc3: W [256, 512]
    DPD_LAUNCH(pose_fc_dx_kernel<4>, dim3(512 / 16, ry), dim3(1024), 0, s, (const float*)g3, net->Wh[2], h2, 512, B, g2, 512, 512);
    DPD_CHECK_LAUNCH();
    // fc2: W [512, 1024]
    DPD_LAUNCH(pose_fc_dx_kernel<8>, dim3(1024 / 16, ry), dim3(1024), 0, s, (const float*)g2, net->Wh[1], h1, 1024, B, g1, 1024, 1024);
    DPD_CHECK_LAUNCH();
    // fc1: W [1024, 2048], input = [features of the first B clouds | of the second B clouds]; its dX is d features [2B, 1024] (no gate)
    {
        const FcDwJob j3{g3, h2, nullptr, dW[2], db[2], 512, 256, 512, (512 / 256) * (256 / 64)};
        const FcDwJob j2{g2, h1, nullptr, dW[1], db[1], 1024, 512, 1024, (1024 / 256) * (512 / 64)};
        const FcDwJob j1{g1, f, f + (size_t)B * OUT, dW[0], db[0], OUT, 1024, 2048, (2048 / 256) * (1024 / 64)};
        DPD_LAUNCH(pose_fc_dw3_kernel, dim3((unsigned)(j3.blocks + j2.blocks + j1.blocks)), dim3(256), 0, s, j3, j2, j1, B);
        DPD_CHECK_LAUNCH();
    }
    DPD_LAUNCH(pose_fc_dx_kernel<16>, dim3(2048 / 16, ry), dim3(1024), 0, s, (const float*)g1, net->Wh[0], (const float*)nullptr, 2048, B, df, OUT, OUT);
    DPD_CHECK_LAUNCH();
    return 0;
}

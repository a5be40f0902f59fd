// Pose algebra of the iterative registration (BASELINE config 5) as ONE launch per direction.
//
// Around the DPDist loss the reference's registration step (pcrnet-registration/iterative_PCRNet_ours.py:410-470) runs, eight times per
// step, a chain of ~115 tiny element-wise TensorFlow ops on [B,7] / [B,4,4] tensors:
//   models/ipcr_model.py:285-294   quat_normalize: (t, angle, axis) -> (tanh(t) 0.1, cos(a/2), axis sin(a/2)), |a| <= lim_rot degrees
//   helper.py:309-329              transformation_quat2mat: normalise the quaternion (transforms3d.quat2mat), T <- [R t; 0 1] T, move the cloud
//   helper.py:539-570              transformation_quat_tensor: Besl-McKay quaternion -> R, data R^T + t
//   iterative_PCRNet_ours.py:211-224   the training evaluation: quaternion / (|q| + 1e-7), then transformation_quat_tensor
// With eager PyTorch that is ~115 launches per refinement loop (1000 of the ~1300 launches of a registration step, which is host-bound at
// 9.2 ms for 0.4 ms of DPDist: profiles/r05_registration_engine_ab.txt).  Here: one workgroup per cloud pair does the whole chain.
//   dpd_pose_apply_fwd   raw pose-network output [B,7] + source cloud [B,N,3] (+ T [B,4,4]) -> pose [B,7], moved cloud, T_out
//   dpd_pose_apply_bwd   d moved [B,N,3] -> d raw output [B,7]  (training evaluation only: the refinements carry no gradient, :414-441)
// dpdist_amd/registration.py keeps the same algebra as plain torch functions (pinned to the reference's goldens); tests compare the two.
//
// The forward-only refinements (7 of the 8 pose-network evaluations of a step, :414-441, and all 8 of an evaluation batch) also run the
// pose NETWORK here -- models/ipcr_model.py:198-233 (shared MLP 3-64-64-64-128-1024 + max pool) and :273-284 (fc 2048-1024-512-256-7,
// dropout before the last layer) -- in four launches per loop (+ two per call) instead of ~25 (dpd_pose_refine):
//   pose_point_kernel   one workgroup per (cloud, 128-column slice of the last layer): all five layers for the cloud's points in LDS,
//                       max pool in the epilogue; the template's features are computed once per call (the template does not move)
//   pose_fc_kernel      the three wide head layers for <= 16 rows on v_mfma_f32_16x16x4_f32: workgroup = 16 outputs, sixteen waves split K;
//                       the template's half of fc1's sum once per call (`rowbias`), every loop contracts the source's half only
//   pose_apply_fwd_kernel   fc4 (256 x 7) as its prologue, then the pose chain above: the LAST loop's pose only -- the pose of every other loop
//                       (fc4, chain, move, T composition) is the prologue of the NEXT loop's pose_point_kernel (PoseMove), not a launch
// fp32 throughout (MFMA fp32 / FMA).
//
// The pose network's units (pose_int.h holds what they share; each kernel is defined in one unit and launched through that unit's launcher):
//   pose.hip             this file: pose_apply_fwd / _bwd kernels and entries, dpd_pose_refine as host orchestration over the launchers
//   pose_point.hip       pose_point_kernel (both instantiations), dpd_pose_point_fwd_train, dpd_pose_point_tie_words
//   pose_point_bwd.hip   the shared MLP's backward: dpd_pose_point_bwd and its workspace entries
//   pose_head.hip        pose_fc_kernel and the head's training evaluation, forward and backward
// fc4, the move of a point and the T_in column are written once in pose_math.h for the two kernels that run them (the apply kernel here,
// the PoseMove prologue of pose_point_kernel) and for regtest.hip's trace.
#include "common.h"
#include "pose_int.h"
#include "pose_math.h"

namespace dpd {

// one workgroup (one wave) per cloud pair.  mode 0: refinement loop (helper.transformation_quat2mat: quaternion / max(|q|, 1e-12), the
// moved cloud and T_out use the same normalised pose); mode 1: training evaluation (moved cloud from quaternion / (|q| + 1e-7),
// iterative_PCRNet_ours.py:211-224; T_out -- the step's returned transform -- from the max(|q|, 1e-12) form like every other loop).
// fc4 prologue (h3 != nullptr): pred[b] = W4 [7,K4] h3[b] + b4, K4 % 4 == 0 (models/ipcr_model.py:284); pred_out (optional) receives it.
__global__ __launch_bounds__(64) void pose_apply_fwd_kernel(const float* __restrict__ pred, const float* __restrict__ src,
                                                            const float* __restrict__ T_in, int N, float lim_rad, int mode,
                                                            float* __restrict__ pose, float* __restrict__ moved,
                                                            float* __restrict__ T_out, const float* __restrict__ h3,
                                                            const float* __restrict__ W4, const float* __restrict__ b4, int K4,
                                                            float* __restrict__ pred_out) {
    const int b = blockIdx.x;
    // what the tail needs from global memory is requested here, before the head's products (N <= 64: one point per lane, else the loop below)
    const int n0 = threadIdx.x;
    float sx = 0.f, sy = 0.f, sz = 0.f;
    if (moved && n0 < N) { const float* s = src + ((size_t)b * N + n0) * 3; sx = s[0]; sy = s[1]; sz = s[2]; }
    float Tc[4] = {0.f, 0.f, 0.f, 0.f};              // column j of T_in (nullptr: the identity, the first loop of a refinement), lanes 0..15
    if (T_out && threadIdx.x < 16) pose_load_T_col(T_in, b, threadIdx.x & 3, Tc);
    float pr[7];
    if (h3) {
        pose_fc4_wave(h3, b, W4, b4, K4, threadIdx.x, pr);
        if (pred_out && threadIdx.x < 7) {
            float v = pr[0];
#pragma unroll
            for (int j = 1; j < 7; ++j) v = (int)threadIdx.x == j ? pr[j] : v;
            pred_out[(size_t)b * 7 + threadIdx.x] = v;
        }
    } else {
#pragma unroll
        for (int j = 0; j < 7; ++j) pr[j] = pred[(size_t)b * 7 + j];
    }
    const Pose7 P = quat_normalize_dev(pr, lim_rad);
    const float nrm = quat_norm_dev(P.q);
    const float dc = fmaxf(nrm, 1e-12f), dt = nrm + 1e-7f;
    float qc[4], qm[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { qc[i] = P.q[i] / dc; qm[i] = mode == 1 ? P.q[i] / dt : qc[i]; }
    float R[3][3];
    quat_to_mat_dev(qm, R);
    if (moved) {
        for (int n = n0; n < N; n += 64) {
            float x = sx, y = sy, z = sz;
            if (n != n0) { const float* s = src + ((size_t)b * N + n) * 3; x = s[0]; y = s[1]; z = s[2]; }
            pose_move_point(R, P.t, x, y, z, moved + ((size_t)b * N + n) * 3);
        }
    }
    if (threadIdx.x == 0 && pose) {          // the network's pose as registration.PoseNet returns it (quat_normalize applied, not re-normalised)
        float* o = pose + (size_t)b * 7;
        o[0] = P.t[0]; o[1] = P.t[1]; o[2] = P.t[2]; o[3] = P.q[0]; o[4] = P.q[1]; o[5] = P.q[2]; o[6] = P.q[3];
    }
    if (T_out && threadIdx.x < 16) {         // helper.py:309-329: T <- [R(qc) t; 0 1] @ T
        float Rc[3][3];
        quat_to_mat_dev(qc, Rc);
        const int i = threadIdx.x >> 2;
        const float v = pose_compose_entry(Rc, P.t, Tc, i);
        T_out[(size_t)b * 16 + threadIdx.x] = v;
    }
}

// d moved [B,N,3] -> d pred [B,7] through moved = src R(u)^T + t, u = q / (|q| + 1e-7), (t, q) = quat_normalize(pred)
__global__ __launch_bounds__(64) void pose_apply_bwd_kernel(const float* __restrict__ pred, const float* __restrict__ src,
                                                            const float* __restrict__ dmoved, int N, float lim_rad,
                                                            float* __restrict__ dpred) {
    const int b = blockIdx.x;
    float acc[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) acc[i] = 0.f;
    for (int n = threadIdx.x; n < N; n += 64) {
        const float* s = src + ((size_t)b * N + n) * 3;
        const float* g = dmoved + ((size_t)b * N + n) * 3;
        const float x = s[0], y = s[1], z = s[2];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const float gi = g[i];
            acc[i * 3 + 0] += gi * x; acc[i * 3 + 1] += gi * y; acc[i * 3 + 2] += gi * z;      // dR[i][j] = sum_n dm[n][i] src[n][j]
            acc[9 + i] += gi;                                                                   // dt[i]
        }
    }
#pragma unroll
    for (int i = 0; i < 12; ++i) acc[i] = wave_sum(acc[i]);
    if (threadIdx.x != 0) return;
    const float* p = pred + (size_t)b * 7;
    const Pose7 P = quat_normalize_dev(p, lim_rad);
    const float nrm = quat_norm_dev(P.q);
    const float den = nrm + 1e-7f;
    const float u0 = P.q[0] / den, u1 = P.q[1] / den, u2 = P.q[2] / den, u3 = P.q[3] / den;
    const float (*dR)[3] = reinterpret_cast<const float (*)[3]>(acc);
    // d R(u) / d u, from helper.py:552-554
    float du[4];
    du[0] = 2.f * (u0 * dR[0][0] - u3 * dR[0][1] + u2 * dR[0][2] + u3 * dR[1][0] + u0 * dR[1][1] - u1 * dR[1][2] - u2 * dR[2][0] + u1 * dR[2][1] + u0 * dR[2][2]);
    du[1] = 2.f * (u1 * dR[0][0] + u2 * dR[0][1] + u3 * dR[0][2] + u2 * dR[1][0] - u1 * dR[1][1] - u0 * dR[1][2] + u3 * dR[2][0] + u0 * dR[2][1] - u1 * dR[2][2]);
    du[2] = 2.f * (-u2 * dR[0][0] + u1 * dR[0][1] + u0 * dR[0][2] + u1 * dR[1][0] + u2 * dR[1][1] + u3 * dR[1][2] - u0 * dR[2][0] + u3 * dR[2][1] - u2 * dR[2][2]);
    du[3] = 2.f * (-u3 * dR[0][0] - u0 * dR[0][1] + u1 * dR[0][2] + u0 * dR[1][0] - u3 * dR[1][1] + u2 * dR[1][2] + u1 * dR[2][0] + u2 * dR[2][1] + u3 * dR[2][2]);
    // u = q / (|q| + eps):  dq_k = du_k / den - (du . q) / den^2 * q_k / |q|
    const float dot = du[0] * P.q[0] + du[1] * P.q[1] + du[2] * P.q[2] + du[3] * P.q[3];
    float dq[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) dq[k] = du[k] / den - (nrm > 0.f ? dot / (den * den) * (P.q[k] / nrm) : 0.f);
    float* o = dpred + (size_t)b * 7;
    if (lim_rad == 0.f) {
        o[0] = acc[9]; o[1] = acc[10]; o[2] = acc[11]; o[3] = dq[0]; o[4] = dq[1]; o[5] = dq[2]; o[6] = dq[3];
        return;
    }
    // quat_normalize: t = tanh(p0..2) 0.1; a = tanh(p3) lim; ax = p4..6 / (|p4..6| + 1e-6); q = (cos(a/2), ax sin(a/2))
    const float th = tanhf(p[3]);
    const float ang = th * lim_rad;
    const float sn = sinf(ang / 2.f), cs = cosf(ang / 2.f);
    const float r0 = sqrtf(p[4] * p[4] + p[5] * p[5] + p[6] * p[6]);
    const float r = r0 + 1e-6f;
    const float ax[3] = {p[4] / r, p[5] / r, p[6] / r};
    const float da = 0.5f * (cs * (ax[0] * dq[1] + ax[1] * dq[2] + ax[2] * dq[3]) - sn * dq[0]);
    o[3] = da * lim_rad * (1.f - th * th);
    const float dax[3] = {sn * dq[1], sn * dq[2], sn * dq[3]};
    const float dotp = dax[0] * p[4] + dax[1] * p[5] + dax[2] * p[6];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        o[4 + k] = dax[k] / r - (r0 > 0.f ? dotp / (r * r) * (p[4 + k] / r0) : 0.f);
        const float tk = tanhf(p[k]);
        o[k] = acc[9 + k] * 0.1f * (1.f - tk * tk);
    }
}

}  // namespace dpd

int dpd::launch_pose_apply_fwd(const float* pred, const float* src, const float* T_in, int B, int N, float lim_rad, int mode, float* pose,
                               float* moved, float* T_out, const float* h3, const float* W4, const float* b4, int K4, float* pred_out, hipStream_t s) {
    DPD_LAUNCH(pose_apply_fwd_kernel, dim3((unsigned)B), dim3(64), 0, s, pred, src, T_in, N, lim_rad, mode, pose, moved, T_out, h3, W4, b4, K4, pred_out);
    DPD_CHECK_LAUNCH();
    return 0;
}

extern "C" int dpd_pose_apply_fwd(const float* pred, const float* src, const float* T_in, int B, int N, float lim_rot_deg, int mode,
                                  float* pose, float* moved, float* T_out, void* stream) {
    if (!pred || (moved && !src)) return DPD_E_NULL;         // T_in == NULL with T_out: composed onto the identity
    if (!pose && !moved && !T_out) return DPD_E_NULL;
    if (T_out && T_out == T_in) return DPD_E_UNSUPPORTED;
    if (B <= 0 || N <= 0 || mode < 0 || mode > 1) return DPD_E_DIM;
    return dpd::launch_pose_apply_fwd(pred, src, T_in, B, N, dpd::lim_rad_of(lim_rot_deg), mode, pose, moved, T_out, nullptr, nullptr, nullptr, 0, nullptr,
                                      (hipStream_t)stream);
}

extern "C" int dpd_pose_apply_bwd(const float* pred, const float* src, const float* dmoved, int B, int N, float lim_rot_deg, float* dpred,
                                  void* stream) {
    if (!pred || !src || !dmoved || !dpred) return DPD_E_NULL;
    if (B <= 0 || N <= 0) return DPD_E_DIM;
    const float lim_rad = dpd::lim_rad_of(lim_rot_deg);
    DPD_LAUNCH(dpd::pose_apply_bwd_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, pred, src, dmoved, N, lim_rad, dpred);
    DPD_CHECK_LAUNCH();
    return 0;
}

namespace {

struct RefineWs {
    float *f, *h1, *h2, *h3, *cloud[2], *T[2], *tb;
    size_t total;
};

RefineWs refine_ws(float* base, int B, int N, int OUT) {
    RefineWs w{};
    size_t off = 0;
    auto take = [&](size_t n) { float* p = base ? base + off : nullptr; off += (n + 63) / 64 * 64; return p; };
    w.f = take((size_t)2 * B * OUT); w.h1 = take((size_t)B * 1024); w.h2 = take((size_t)B * 512); w.h3 = take((size_t)B * 256);
    w.cloud[0] = take((size_t)B * N * 3); w.cloud[1] = take((size_t)B * N * 3); w.T[0] = take((size_t)B * 16); w.T[1] = take((size_t)B * 16);
    w.tb = take((size_t)B * 1024);
    w.total = off * sizeof(float);
    return w;
}

}  // namespace

extern "C" size_t dpd_pose_refine_workspace_bytes(int B, int N, int out_features) {
    if (B <= 0 || N <= 0 || out_features <= 0) return 0;
    return refine_ws(nullptr, B, N, out_features).total;
}

extern "C" int dpd_pose_refine(const dpd_pose_net* net, const float* src, const float* tmpl, int B, int N, int loops, float lim_rot_deg,
                               const float* drop_mask, void* ws, size_t ws_bytes, float* moved, float* T_out, float* pred_out, void* stream) {
    return dpd_pose_refine_pool(net, src, tmpl, B, N, loops, lim_rot_deg, DPD_POOL_MAX, drop_mask, ws, ws_bytes, moved, T_out, pred_out, stream);
}

extern "C" int dpd_pose_refine_pool(const dpd_pose_net* net, const float* src, const float* tmpl, int B, int N, int loops, float lim_rot_deg, int pool,
                                    const float* drop_mask, void* ws, size_t ws_bytes, float* moved, float* T_out, float* pred_out, void* stream) {
    using namespace dpd;
    if (!net || !src || !tmpl || !ws || !moved || !T_out) return DPD_E_NULL;
    if (int rc = check_point_layers(net)) return rc;
    if (int rc = check_head_layers(net, true)) return rc;
    if (B <= 0 || N <= 0 || loops <= 0) return DPD_E_DIM;
    if (!pool_known(pool)) return DPD_E_UNSUPPORTED;
    const bool avg = pool == DPD_POOL_AVG;                 // the shared MLP's epilogue only: the head and the pose chain do not look at the pool
    const int OUT = net->out_features;
    if (OUT != 1024) return DPD_E_UNSUPPORTED;             // the reference's width (models/ipcr_model.py:226); the head kernel's K is a template parameter
    if (((uintptr_t)ws & 15) != 0) return DPD_E_UNSUPPORTED;
    const RefineWs w = refine_ws((float*)ws, B, N, OUT);
    if (ws_bytes < w.total) return DPD_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const float lim_rad = dpd::lim_rad_of(lim_rot_deg);
    const PointNetW pw = point_net_of(net);
    const float* f_tmpl = w.f + (size_t)B * OUT;
    // loop it: features of source_it (and of the template, once) -> head up to its last hidden layer h3_it.  The pose of loop it - 1 -- fc4,
    // quat_normalize, the move source_{it-1} -> source_it, T <- M T -- is the PROLOGUE of loop it's shared MLP (PoseMove); the last loop's pose is
    // the one pose_apply_fwd_kernel launch of the call: 4 loops + 1 launches.
    const float* cur = src;                 // source_{it-1} while loop it is being enqueued
    const float* Tcur = nullptr;
    for (int it = 0; it < loops; ++it) {
        if (it == 0) {
            if (int rc = launch_pose_point<false>(cur, tmpl, B, 2 * B, N, pw, OUT, w.f, PointSave{}, PoseMove{}, avg, s)) return rc;
            // the template never moves: its half of fc1's sum (W1[:, OUT:] f_tmpl + b1) once per call, every loop then contracts the source's
            // half only (4 MB of weights per loop instead of 8)
            if (int rc = launch_pose_fc(net, 0, FcIn{f_tmpl, nullptr, OUT, OUT}, /*wcol0*/ OUT, /*rowbias*/ nullptr, /*relu*/ false, /*mask*/ nullptr, w.tb, B, s)) return rc;
        } else {
            float* nxt = w.cloud[(it - 1) & 1];
            float* Tn = w.T[(it - 1) & 1];
            const PoseMove mv{w.h3, net->Wh[3], net->bh[3], Tcur, nxt, Tn, pred_out ? pred_out + (size_t)(it - 1) * B * 7 : (float*)nullptr, lim_rad, 256};
            if (int rc = launch_pose_point<false>(cur, nullptr, B, B, N, pw, OUT, w.f, PointSave{}, mv, avg, s)) return rc;
            cur = nxt;
            Tcur = Tn;
        }
        const float* dm = drop_mask ? drop_mask + (size_t)it * B * 256 : (const float*)nullptr;
        if (int rc = launch_pose_fc(net, 0, FcIn{w.f, nullptr, OUT, OUT}, /*wcol0*/ 0, /*rowbias*/ w.tb, /*relu*/ true, /*mask*/ nullptr, w.h1, B, s)) return rc;
        if (int rc = launch_pose_fc(net, 1, FcIn{w.h1, nullptr, 1024, 1024}, /*wcol0*/ 0, /*rowbias*/ nullptr, /*relu*/ true, /*mask*/ nullptr, w.h2, B, s)) return rc;
        if (int rc = launch_pose_fc(net, 2, FcIn{w.h2, nullptr, 512, 512}, /*wcol0*/ 0, /*rowbias*/ nullptr, /*relu*/ true, /*mask*/ dm, w.h3, B, s)) return rc;
    }
    return launch_pose_apply_fwd(nullptr, cur, Tcur, B, N, lim_rad, 0, nullptr, moved, T_out, w.h3, net->Wh[3], net->bh[3], 256,
                                 pred_out ? pred_out + (size_t)(loops - 1) * B * 7 : (float*)nullptr, s);
}

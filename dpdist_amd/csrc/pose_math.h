// Pose algebra shared by the kernels that compose the registration's transforms (pose.hip: the apply kernel, the last loop of a
// refinement; pose_point.hip: the PoseMove prologue of the shared MLP, every other loop; regtest.hip: the per-iteration trace of the
// test protocol).  One definition, so that every kernel produces the same fp32 bits for the same raw network output (the build has
// -ffp-contract=off: an expression is the same roundings wherever it is inlined).
#pragma once
#include "common.h"

namespace dpd {

// lim_rot in degrees (the entry points' argument) -> the kernels' lim_rad; 0 stays 0 (no limit: the network's output is the pose)
inline float lim_rad_of(float lim_rot_deg) { return (float)(3.14159265358979323846 / 180.0 * (double)lim_rot_deg); }

struct Pose7 {
    float t[3];
    float q[4];
};

// models/ipcr_model.py:285-294; lim_rad = pi/180 * lim_rot.  lim_rad == 0: the network's output IS the pose (lim_rot falsy).
__device__ __forceinline__ Pose7 quat_normalize_dev(const float* __restrict__ p, float lim_rad) {
    Pose7 o;
    if (lim_rad == 0.f) {
        o.t[0] = p[0]; o.t[1] = p[1]; o.t[2] = p[2];
        o.q[0] = p[3]; o.q[1] = p[4]; o.q[2] = p[5]; o.q[3] = p[6];
        return o;
    }
    const float ang = tanhf(p[3]) * lim_rad;
    const float r = sqrtf(p[4] * p[4] + p[5] * p[5] + p[6] * p[6]) + 1e-6f;
    const float s = sinf(ang / 2.f);
    o.t[0] = tanhf(p[0]) * 0.1f; o.t[1] = tanhf(p[1]) * 0.1f; o.t[2] = tanhf(p[2]) * 0.1f;
    o.q[0] = cosf(ang / 2.f);
    o.q[1] = p[4] / r * s; o.q[2] = p[5] / r * s; o.q[3] = p[6] / r * s;
    return o;
}

// helper.py:552-554 (no normalisation inside)
__device__ __forceinline__ void quat_to_mat_dev(const float* q, float R[3][3]) {
    const float q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3];
    R[0][0] = q0 * q0 + q1 * q1 - q2 * q2 - q3 * q3; R[0][1] = 2.f * (q1 * q2 - q0 * q3); R[0][2] = 2.f * (q1 * q3 + q0 * q2);
    R[1][0] = 2.f * (q1 * q2 + q0 * q3); R[1][1] = q0 * q0 + q2 * q2 - q1 * q1 - q3 * q3; R[1][2] = 2.f * (q2 * q3 - q0 * q1);
    R[2][0] = 2.f * (q1 * q3 - q0 * q2); R[2][1] = 2.f * (q2 * q3 + q0 * q1); R[2][2] = q0 * q0 + q3 * q3 - q1 * q1 - q2 * q2;
}

// |q|: the refinement loop divides by max(|q|, 1e-12) (transforms3d.quat2mat inside helper.transformation_quat2mat)
__device__ __forceinline__ float quat_norm_dev(const float q[4]) { return sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]); }

// Entry (i, j) of [R t; 0 1] @ T, given column j of T in Tc (helper.py:309-329); the last row is T's own
__device__ __forceinline__ float pose_compose_entry(const float R[3][3], const float t[3], const float Tc[4], int i) {
    if (i < 3) return ((R[i][0] * Tc[0] + R[i][1] * Tc[1]) + R[i][2] * Tc[2]) + t[i] * Tc[3];
    return Tc[3];
}

// Column j of T_in[b] for the composition above; T_in == nullptr: of the identity (the first loop of a refinement)
__device__ __forceinline__ void pose_load_T_col(const float* __restrict__ T_in, int b, int j, float Tc[4]) {
#pragma unroll
    for (int r = 0; r < 4; ++r) Tc[r] = T_in ? T_in[(size_t)b * 16 + r * 4 + j] : (r == j ? 1.f : 0.f);
}

// The head's last layer on ONE wave (models/ipcr_model.py:284): pr[j] = W4[j, :] . h3[b, :] + b4[j], j < 7, in every lane; K4 % 4 == 0.
// Lane l takes the float4s at k = 4 l, 4 l + 256, ...; the lanes' sums meet in wave_sum's fixed tree.  (The row is indexed inside the loop:
// handed over as a row pointer it cost pose_apply_fwd_kernel six VGPRs and a wave of occupancy.)
__device__ __forceinline__ void pose_fc4_wave(const float* __restrict__ h3, int b, const float* __restrict__ W4, const float* __restrict__ b4, int K4,
                                              int lane, float pr[7]) {
    float bb[7], acc[7];
#pragma unroll
    for (int j = 0; j < 7; ++j) { bb[j] = b4[j]; acc[j] = 0.f; }
    for (int k = lane * 4; k < K4; k += 256) {
        const float4 x = *reinterpret_cast<const float4*>(h3 + (size_t)b * K4 + k);
#pragma unroll
        for (int j = 0; j < 7; ++j) {
            const float4 w = *reinterpret_cast<const float4*>(W4 + (size_t)j * K4 + k);
            acc[j] = fmaf(x.x, w.x, fmaf(x.y, w.y, fmaf(x.z, w.z, fmaf(x.w, w.w, acc[j]))));
        }
    }
#pragma unroll
    for (int j = 0; j < 7; ++j) pr[j] = wave_sum(acc[j]) + bb[j];
}

// One point moved: o = R p + t (helper.py:539-570: data R^T + t, row vectors)
__device__ __forceinline__ void pose_move_point(const float R[3][3], const float t[3], float x, float y, float z, float o[3]) {
    o[0] = (x * R[0][0] + y * R[0][1] + z * R[0][2]) + t[0];
    o[1] = (x * R[1][0] + y * R[1][1] + z * R[1][2]) + t[1];
    o[2] = (x * R[2][0] + y * R[2][1] + z * R[2][2]) + t[2];
}

}  // namespace dpd

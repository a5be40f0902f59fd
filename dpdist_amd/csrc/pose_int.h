// What the pose network's translation units share: pose.hip (the quaternion chain and the forward-only refinement), pose_point.hip (shared
// MLP forward), pose_point_bwd.hip (its backward), pose_head.hip (the head, forward and backward).  Every kernel lives in exactly one unit;
// a unit that needs another unit's kernel calls the launcher declared here, which has its one definition in the unit named beside it.
#pragma once
#include "common.h"
#include "lds_dma.h"      // f32x16

namespace dpd {

constexpr int kPP = 64;                 // points per pass of the shared MLP
constexpr int kTrainMaxN = 2048;        // training evaluation: at most 32 passes (the reference's MAX_NUM_POINT, iterative_PCRNet_ours.py:103-104)
constexpr int kSlice = 128;             // columns of the last shared layer per workgroup

struct PointNetW {
    const float* W[5];   // [out, in] row-major (torch nn.Linear): 64x3, 64x64, 64x64, 128x64, OUTx128
    const float* b[5];
};

// C/D map of the 32x32 MFMA: register r of lane l is row (r & 3) + 8 (r >> 2) + 4 (l >> 5), column l & 31
__device__ __forceinline__ int mfma_row(int r, int l) { return (r & 3) + 8 * (r >> 2) + 4 * (l >> 5); }

// What the training evaluation keeps of the shared MLP's forward (pose_point.hip writes it, pose_point_bwd.hip reads it): the four hidden
// activations and the TIE MASK of the max pool -- W = ceil(N / 64) words per (cloud, column), ties[cloud][w][column]; bit b of word w is set
// iff point 64 w + b attains the column's maximum and that maximum is positive.  Under the average pool the same buffer holds the GATE
// words: bit b of word w is set iff point 64 w + b is a real point and its layer-5 pre-activation is > 0.
struct PointSave {
    float* h[4];                    // [clouds * N, 64] x 3, [clouds * N, 128]
    unsigned long long* ties;       // [clouds, ceil(N / 64), OUT]
};
// Refinement loops 2..n (dpd_pose_refine): the cloud a workgroup reads is the PREVIOUS loop's source moved by the pose the head made of it --
// fc4 (pred = W4 h3 + b4), quat_normalize, R, the move and the T composition are a prologue of the next loop's shared MLP instead of a launch
// of their own (pose_apply_fwd_kernel: 5-9 us per loop for a microsecond of work).  Every (cloud, slice) workgroup recomputes its pair's pose
// (wave 0, with the routines of pose_math.h that the apply kernel runs, so the same bits) while the weight images are in flight; slice 0
// stores the moved cloud, T and the raw prediction.  h3 == nullptr: no move (first loop, training evaluation).
struct PoseMove {
    const float* h3;                // [B, K4] activations of the head's last hidden layer (previous loop)
    const float* W4;                // [7, K4]
    const float* b4;                // [7]
    const float* T_in;              // [B, 16] or nullptr (identity)
    float* moved;                   // [B, N, 3]
    float* T_out;                   // [B, 16]
    float* pred_out;                // [B, 7] or nullptr
    float lim_rad;
    int K4;
};

// ---- pose_point.hip ----
int check_point_layers(const dpd_pose_net* net);           // DPD_E_NULL unless net and its five Wp / bp are there
PointNetW point_net_of(const dpd_pose_net* net);
// pose_point_kernel<TRAIN, avg> over `clouds` clouds (cloud c < nA: ptsA[c], else ptsB[c - nA]) -> f [clouds, OUT]; avg: the average pool
// (f = sum / N, PointSave::ties receives the GATE words) instead of the max pool
template <bool TRAIN>
int launch_pose_point(const float* ptsA, const float* ptsB, int nA, int clouds, int N, const PointNetW& pw, int OUT, float* f, const PointSave& sv,
                      const PoseMove& mv, bool avg, hipStream_t s);
inline bool pool_known(int pool) { return pool == DPD_POOL_MAX || pool == DPD_POOL_AVG; }      // enum dpd_pool; anything else: DPD_E_UNSUPPORTED

// ---- pose_head.hip ----
int check_head_layers(const dpd_pose_net* net, bool biases);      // DPD_E_NULL unless net and its four Wh (and, with `biases`, bh) are there
// The input of one wide head layer: [A (KA columns) | B (K - KA)], R rows; B == nullptr: A alone (KA == K)
struct FcIn {
    const float* A;
    const float* B;
    int KA, K;
};
// pose_fc_kernel<K / 256>: out [R, J] = act(in Wh[layer][:, wcol0 .. wcol0 + K)^T + bias) (* mask), J = the layer's width (1024, 512, 256);
// rowbias [R, J] replaces bh[layer] (a part of the sum made earlier); K = 512, 1024 or 2048
int launch_pose_fc(const dpd_pose_net* net, int layer, FcIn in, int wcol0, const float* rowbias, bool relu, const float* mask, float* out, int R,
                   hipStream_t s);

// ---- pose.hip ----
// pose_apply_fwd_kernel, one workgroup per pair; h3 != nullptr: pred = W4 h3 + b4 first (fc4 prologue), stored to pred_out if given
int launch_pose_apply_fwd(const float* pred, const float* src, const float* T_in, int B, int N, float lim_rad, int mode, float* pose, float* moved,
                          float* T_out, const float* h3, const float* W4, const float* b4, int K4, float* pred_out, hipStream_t s);

}  // namespace dpd

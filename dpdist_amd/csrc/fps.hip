// Farthest-point sampling of S clouds in one launch, and the gather of a sample (include/dpdist_capi.h: dpd_fps_order,
// dpd_fps_gather_fwd / _bwd; driven by dpdist_amd/sampling.py and the resampler of dpdist_amd/dataset.py).
//
// The reference's readers take "the first npoints rows" of a shape file (modelnet_dataset.py:121-122,136), which is a well-spread sample only
// because modelnet40_normal_resampled was written in farthest-point order.  This kernel produces that order for any cloud:
//     order[0] = start;  order[k] = the not yet chosen j of largest dmin_j = min_{i < k} d2(p_j, p_order[i]), among equals the LOWEST j
// with d2 = (dx*dx + dy*dy) + dz*dz in fp32, in that order and not fused (-ffp-contract=off): the form of nn_dist.hip.  A maximum does not
// depend on the visiting order once ties go to the lowest index, so the order is defined bit for bit whatever the tiling.
//
// The loop is sequential in k, so a cloud gets ONE workgroup of 1024 threads (16 waves, 4 per SIMD: at most 128 registers per lane) and
// the whole loop runs inside it; S clouds are S workgroups.  Thread t owns the points j = t + 1024 r.  A chosen point, and a slot past the
// cloud's count, holds dmin = -1: it never passes `d < dmin` nor `dmin > best`, so it is excluded, not merely at distance 0.
//   resident form (clouds up to DPD_FPS_RESIDENT_POINTS = 16 points per thread): coordinates and dmin live in registers, 4 PPT of them per
//     lane; the kernel is a template on PPT = 1 / 2 / 4 / 8 / 16 so that a 64-point cloud does not pay for a 16 384-point one;
//   streamed form (wider clouds, up to DPD_FPS_MAX_POINTS): a rolled loop over the thread's points; dmin lives in the caller's workspace
//     ([S,W] floats, each element read and written by its owning thread only) and the coordinates are re-read from global memory every
//     iteration (lane-consecutive points: a wave reads 768 contiguous bytes per round; 16 bytes per point and iteration, out of L2).
//     A rolled loop needs under 50 registers at any size; 64 points per thread unrolled in registers did not fit the 128 of this launch shape.
// Per iteration each lane updates its dmin against the current point and keeps its best (dmin, j) WITH that point's coordinates (ascending
// j and a strict `>`: the lowest j of the lane).  The wave reduces a 64-bit key: dmin >= 0, so its bit pattern orders as an unsigned
// integer, and ~j in the low word makes one `max` implement the tie rule; an excluded slot has key 0, below every live key.  The
// reduction runs on the DPP path (two dependent 32-bit maxima, ~10 cycles per step) rather than __shfl_xor, whose six dependent trips
// through the LDS crossbar cost more than the scan of a 2048-point cloud (measured 1.25 -> 0.70 us per iteration).  The wave's winning
// lane writes key and coordinates into one of two alternating LDS slots, ONE __syncthreads(), and every wave merges the 16 records (one
// LDS read, a 16-lane row reduction): each thread knows the next point and its coordinates without a global load.  The slot written in
// iteration k is written again in k + 2, behind the barrier of k + 1, which no thread passes before it has read the records of k.
// A cloud occupies one CU; a single large cloud is latency-bound on it.  That is accepted.
#include "common.h"

namespace dpd {

constexpr int kFpsThreads = DPD_FPS_THREADS;
constexpr int kFpsWaves = kFpsThreads / kWave;        // 16
constexpr int kFpsResidentPpt = DPD_FPS_RESIDENT_POINTS / kFpsThreads;
static_assert(kFpsResidentPpt == 16 && kFpsResidentPpt * kFpsThreads == DPD_FPS_RESIDENT_POINTS, "resident cap = 16 points per thread");
static_assert(kFpsWaves == 16, "the records of a slot fill one 16-lane row");
static_assert(DPD_FPS_MAX_POINTS >= (1 << 16) && DPD_FPS_MAX_POINTS < (1 << 30), "~j of the key's low word stays above 2^31");

// Unsigned maxima on the DPP path, the tree of common.h's wave_sum with max in place of + (a lane without a valid source reads 0, the
// identity of an unsigned max).  The key (hi, lo) is reduced as two dependent 32-bit maxima -- the largest hi, then the largest lo among
// the lanes that hold it -- which is the 64-bit maximum.
template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ unsigned dpp_u32(unsigned v) {
    return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xf, true);
}
__device__ __forceinline__ unsigned row_max16(unsigned v) {      // every lane of a 16-lane row gets the maximum of its row
    v = max(v, dpp_u32<0xB1>(v));       // quad_perm [1,0,3,2]
    v = max(v, dpp_u32<0x4E>(v));       // quad_perm [2,3,0,1]
    v = max(v, dpp_u32<0x141>(v));      // row_half_mirror
    v = max(v, dpp_u32<0x140>(v));      // row_mirror
    return v;
}
__device__ __forceinline__ unsigned wave_max(unsigned v) {       // the maximum over the 64 lanes, uniform
    v = row_max16(v);
    v = max(v, dpp_u32<0x142, 0xA>(v));  // row_bcast15 into rows 1 and 3
    v = max(v, dpp_u32<0x143, 0xC>(v));  // row_bcast31 into rows 2 and 3: lane 63 holds all four rows
    return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}

// high word of a key: 0 for an excluded slot (d < 0), else the bits of d (d >= 0: they order as an unsigned integer) + 1
__device__ __forceinline__ unsigned fps_key_hi(float d) { return d < 0.0f ? 0u : __float_as_uint(d) + 1u; }

// RESIDENT: PPT points per thread in registers.  Streamed (PPT = 0): a rolled loop over the cloud, dmin in `ws` ([S,W] floats).
template <int PPT, bool RESIDENT>
__global__ __launch_bounds__(kFpsThreads) void fps_order_kernel(const float* __restrict__ pts, const int32_t* __restrict__ counts,
                                                                const int32_t* __restrict__ start, int W, int K,
                                                                int32_t* __restrict__ order, float* __restrict__ radius, float* __restrict__ ws) {
    __shared__ unsigned s_hi[2][kFpsWaves], s_lo[2][kFpsWaves];
    __shared__ float s_xyz[2][kFpsWaves][4];
    const int c = blockIdx.x, t = threadIdx.x;
    const int lane = t & (kWave - 1), wave = t / kWave;
    const int n = ragged_count(counts, c, W);
    const int kn = min(K, n);
    const float* p = pts + (size_t)c * W * 3;
    int32_t* ord = order + (size_t)c * K;
    float* rad = radius ? radius + (size_t)c * K : nullptr;
    float* gd = RESIDENT ? nullptr : ws + (size_t)c * W;

    constexpr int R = RESIDENT ? PPT : 1;
    float dmin[R], px[R], py[R], pz[R];
    if (RESIDENT) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int j = t + kFpsThreads * r;
            const int jj = min(j, n - 1);                // a slot past the count re-reads the last point and never takes part
            dmin[r] = j < n ? INFINITY : -1.0f;
            px[r] = p[jj * 3], py[r] = p[jj * 3 + 1], pz[r] = p[jj * 3 + 2];
        }
    }

    int cur = start ? min(max(start[c], 0), n - 1) : 0;
    float cx = p[cur * 3], cy = p[cur * 3 + 1], cz = p[cur * 3 + 2];
    float dwin = INFINITY;
    for (int k = 0; k < kn; ++k) {
        if (t == 0) {
            ord[k] = cur;
            if (rad) rad[k] = k == 0 ? INFINITY : sqrtf(dwin);
        }
        if (k + 1 == kn) break;                          // uniform: nothing is chosen after the last output
        float bd = -1.0f, bx = 0.0f, by = 0.0f, bz = 0.0f;
        int bj = 0;
        if (RESIDENT) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int j = t + kFpsThreads * r;
                const float dx = px[r] - cx, dy = py[r] - cy, dz = pz[r] - cz;
                const float d = (dx * dx + dy * dy) + dz * dz;
                float m = dmin[r];
                m = d < m ? d : m;
                m = j == cur ? -1.0f : m;
                dmin[r] = m;
                if (m > bd) { bd = m, bj = j, bx = px[r], by = py[r], bz = pz[r]; }      // ascending j + strict > : the lowest index of this lane
            }
        } else {
#pragma unroll 8
            for (int j = t; j < n; j += kFpsThreads) {   // only rows below the count are read
                const float x = p[j * 3], y = p[j * 3 + 1], z = p[j * 3 + 2];   // 3 W < 2^31
                const float dx = x - cx, dy = y - cy, dz = z - cz;
                const float d = (dx * dx + dy * dy) + dz * dz;
                float m = k == 0 ? INFINITY : gd[j];     // the first iteration initialises the workspace: it is never read before written
                m = d < m ? d : m;
                m = j == cur ? -1.0f : m;
                gd[j] = m;                               // re-read by this thread only
                if (m > bd) { bd = m, bj = j, bx = x, by = y, bz = z; }
            }
        }
        const unsigned hi = fps_key_hi(bd);
        const unsigned htop = wave_max(hi);
        const unsigned lo = (hi == htop && hi != 0u) ? (unsigned)~bj : 0u;   // live low words are >= 2^31 and distinct (they hold j)
        const unsigned ltop = wave_max(lo);
        const int slot = k & 1;
        if (htop != 0u ? (hi == htop && lo == ltop) : lane == 0) {           // one writer per wave
            s_hi[slot][wave] = htop, s_lo[slot][wave] = ltop;
            s_xyz[slot][wave][0] = bx, s_xyz[slot][wave][1] = by, s_xyz[slot][wave][2] = bz;
        }
        __syncthreads();
        // every wave merges the 16 records, one per lane of each 16-lane row, all to the same result
        const unsigned qh = s_hi[slot][lane & (kFpsWaves - 1)], ql = s_lo[slot][lane & (kFpsWaves - 1)];
        const unsigned th = row_max16(qh);
        const unsigned tl = row_max16(qh == th ? ql : 0u);
        const int w = (__ffsll((long long)__ballot(qh == th && ql == tl)) - 1) & (kFpsWaves - 1);   // all excluded: wave 0, never used
        cur = min(max((int)~tl, 0), n - 1);              // k + 1 < n: a live key exists for finite input; the clamp keeps any input in bounds
        dwin = __uint_as_float(max(th, 1u) - 1u);
        cx = s_xyz[slot][w][0], cy = s_xyz[slot][w][1], cz = s_xyz[slot][w][2];
    }
    for (int k = kn + t; k < K; k += kFpsThreads) {
        ord[k] = -1;
        if (rad) rad[k] = 0.0f;
    }
}

// out[c,k,:] = src[c, order[c,k], :], +0.0 where the order holds -1 (or anything outside the cloud's rows)
__global__ __launch_bounds__(256) void fps_gather_fwd_kernel(const float* __restrict__ src, const int32_t* __restrict__ order, int W, int D, int K,
                                                             float* __restrict__ out) {
    const int c = blockIdx.y;
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long long)K * D) return;
    const int k = (int)(e / D), d = (int)(e - (long long)k * D);
    const int o = order[(size_t)c * K + k];
    out[(size_t)c * K * D + e] = (o >= 0 && o < W) ? src[((size_t)c * W + o) * D + d] : 0.0f;
}

// dsrc[c, order[c,k], :] = dout[c,k,:], every other row +0.0, in one launch and without atomics: a workgroup owns kFpsBwdRows rows of one
// cloud, clears them, passes a barrier (which completes its stores), then scans the cloud's K order entries and writes the rows that fall
// into its range.  Row ranges are disjoint, and the entries of an order are distinct (the precondition): one writer per element after the
// barrier.
constexpr int kFpsBwdRows = 4096;
__global__ __launch_bounds__(kFpsThreads) void fps_gather_bwd_kernel(const float* __restrict__ dout, const int32_t* __restrict__ order, int W, int D,
                                                                     int K, float* __restrict__ dsrc) {
    const int c = blockIdx.y;
    const int w0 = blockIdx.x * kFpsBwdRows, w1 = min(w0 + kFpsBwdRows, W);
    float* g = dsrc + (size_t)c * W * D;
    for (long long e = (long long)w0 * D + threadIdx.x; e < (long long)w1 * D; e += kFpsThreads) g[e] = 0.0f;
    __syncthreads();
    const long long KD = (long long)K * D;
    for (long long e = threadIdx.x; e < KD; e += kFpsThreads) {
        const int k = (int)(e / D), d = (int)(e - (long long)k * D);
        const int o = order[(size_t)c * K + k];
        if (o >= w0 && o < w1) g[(size_t)o * D + d] = dout[(size_t)c * K * D + e];
    }
}

template <int PPT, bool RESIDENT>
static int fps_launch(const float* pts, const int32_t* counts, const int32_t* start, int S, int W, int K, int32_t* order, float* radius,
                      float* ws, hipStream_t s) {
    DPD_LAUNCH((fps_order_kernel<PPT, RESIDENT>), dim3(S), dim3(kFpsThreads), 0, s, pts, counts, start, W, K, order, radius, ws);
    DPD_CHECK_LAUNCH();
    return 0;
}

}  // namespace dpd

extern "C" size_t dpd_fps_workspace_bytes(int S, int W) {
    if (S < 1 || W < 1 || S > DPD_FPS_MAX_CLOUDS || W > DPD_FPS_MAX_POINTS) return 0;
    return W <= DPD_FPS_RESIDENT_POINTS ? 0 : (size_t)S * W * sizeof(float);       // the streamed form's dmin; the resident form has none
}

extern "C" int dpd_fps_order(const float* pts, const int32_t* counts, const int32_t* start, int S, int W, int K, int32_t* order, float* radius,
                             void* ws, size_t ws_bytes, void* stream) {
    using namespace dpd;
    if (!pts || !order) return DPD_E_NULL;
    if (S < 1 || W < 1 || K < 1 || K > W) return DPD_E_DIM;
    if (S > DPD_FPS_MAX_CLOUDS || W > DPD_FPS_MAX_POINTS) return DPD_E_UNSUPPORTED;
    const size_t need = dpd_fps_workspace_bytes(S, W);
    if (need > 0 && (!ws || ws_bytes < need)) return DPD_E_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    const int ppt = (W + kFpsThreads - 1) / kFpsThreads;
    if (ppt <= 1) return fps_launch<1, true>(pts, counts, start, S, W, K, order, radius, nullptr, s);
    if (ppt <= 2) return fps_launch<2, true>(pts, counts, start, S, W, K, order, radius, nullptr, s);
    if (ppt <= 4) return fps_launch<4, true>(pts, counts, start, S, W, K, order, radius, nullptr, s);
    if (ppt <= 8) return fps_launch<8, true>(pts, counts, start, S, W, K, order, radius, nullptr, s);
    if (ppt <= kFpsResidentPpt) return fps_launch<kFpsResidentPpt, true>(pts, counts, start, S, W, K, order, radius, nullptr, s);
    return fps_launch<0, false>(pts, counts, start, S, W, K, order, radius, (float*)ws, s);
}

static int fps_gather_check(const void* a, const void* order, const void* b, int S, int W, int D, int K) {
    if (!a || !order || !b) return DPD_E_NULL;
    if (S < 1 || W < 1 || D < 1 || K < 1 || K > W) return DPD_E_DIM;
    if (S > DPD_FPS_MAX_CLOUDS || W > DPD_FPS_MAX_POINTS || (long long)W * D >= (1ll << 31)) return DPD_E_UNSUPPORTED;
    return 0;
}

extern "C" int dpd_fps_gather_fwd(const float* src, const int32_t* order, int S, int W, int D, int K, float* out, void* stream) {
    using namespace dpd;
    const int rc = fps_gather_check(src, order, out, S, W, D, K);
    if (rc) return rc;
    const long long KD = (long long)K * D;
    DPD_LAUNCH(fps_gather_fwd_kernel, dim3((unsigned)((KD + 255) / 256), S), dim3(256), 0, (hipStream_t)stream, src, order, W, D, K, out);
    DPD_CHECK_LAUNCH();
    return 0;
}

extern "C" int dpd_fps_gather_bwd(const float* dout, const int32_t* order, int S, int W, int D, int K, float* dsrc, void* stream) {
    using namespace dpd;
    const int rc = fps_gather_check(dout, order, dsrc, S, W, D, K);
    if (rc) return rc;
    DPD_LAUNCH(fps_gather_bwd_kernel, dim3((W + kFpsBwdRows - 1) / kFpsBwdRows, S), dim3(kFpsThreads), 0, (hipStream_t)stream, dout, order, W, D, K,
               dsrc);
    DPD_CHECK_LAUNCH();
    return 0;
}

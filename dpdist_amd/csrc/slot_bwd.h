// Device routines of the SLOT-SUMMED layer-1 backward, written once for the two layouts that use it: the all-pairs matrix (cross_bwd.hip:
// one query set shared by all surfaces, one U per chunk, rows (i, j, n)) and the per-point field (field_bwd.hip: every cloud its own
// queries and slots, slots cloud-major, rows (c, t)).  The kernels of the two files differ in how they find a workgroup's slot, list and
// rows; what they then do is below.  Everything is deterministic: no float atomics, one summation order per output element.
#pragma once
#include "common.h"

namespace dpd {

constexpr int kSlotMaxH = 4096;       // slot_sum_rows: one wave per 256 columns, at most 16 waves
constexpr int kSlotRows = 32;         // rows between two exchanges of the waves' partial dot products

// One workgroup of 1024 threads: the QN queries vox [QN] sorted by slot (a stable counting sort: ascending query id inside a slot), the
// start offset of every slot and the voxel of every slot.  Counts by integer LDS atomics (any order gives the same counts), an exclusive
// prefix over the voxels, then wave 0 places the queries 64 at a time in query order: lanes of one slot take consecutive positions by
// their rank among the lanes of that slot (a ballot), so the order inside a slot is the query id.  Integer only, one order.
//   slot_start [U]   list_base + the start of slot s in qlist (the caller writes the entries beyond U)
//   qlist [QN]       query ids sorted by (slot, query id)
//   slot_vox [U]     voxel id of slot s
// U is the clamped slot count of this workgroup's queries; slot_start and slot_vox point at its slot 0.  s_cnt [1024], s_wsum [16].
__device__ __forceinline__ void invert_block(const int32_t* __restrict__ vox, const int32_t* __restrict__ slot_of_vox, int U, int QN, int G,
                                             int list_base, int32_t* __restrict__ slot_start, int32_t* __restrict__ qlist,
                                             int32_t* __restrict__ slot_vox, int* s_cnt, int* s_wsum) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    s_cnt[tid] = 0;
    __syncthreads();
    for (int r = tid; r < QN; r += 1024) {
        int v = vox[r];
        if ((unsigned)v >= (unsigned)G) v = 0;
        atomicAdd(&s_cnt[v], 1);
    }
    __syncthreads();
    // exclusive prefix of the counts in voxel order (= slot order: the slots are the occupied voxels in ascending voxel id)
    const int c = s_cnt[tid];
    int incl = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(incl, d, 64);
        if (lane >= d) incl += o;
    }
    if (lane == 63) s_wsum[wave] = incl;
    __syncthreads();
    int before = 0;
    for (int w = 0; w < 16; ++w) before += (w < wave) ? s_wsum[w] : 0;
    const int start = before + incl - c;
    __syncthreads();
    s_cnt[tid] = start;
    if (tid < G) {
        const int sl = slot_of_vox[tid];
        if (sl >= 0 && sl < U) { slot_start[sl] = list_base + start; slot_vox[sl] = tid; }
    }
    __syncthreads();
    if (wave != 0) return;
    volatile int* pos_of = s_cnt;      // written by one lane, read by others of the same wave in the next round
    for (int r0 = 0; r0 < QN; r0 += 64) {
        const int r = r0 + lane;
        const bool live = r < QN;
        int v = live ? vox[r] : 0;
        if ((unsigned)v >= (unsigned)G) v = 0;
        // the live lanes with this lane's voxel, from one ballot per bit of the voxel id (G <= 1000: 10 bits) instead of one round per
        // distinct voxel among the 64: a tile of 10 000 queries has about 60 distinct voxels in every round
        unsigned long long same = __ballot(live);
#pragma unroll
        for (int bit = 0; bit < 10; ++bit) {
            const bool set = (v >> bit) & 1;
            const unsigned long long b = __ballot(set);
            same &= set ? b : ~b;
        }
        const int rank = __popcll(same & ((1ull << lane) - 1ull)), total = __popcll(same);
        if (live) {
            const int pos = pos_of[v] + rank;
            if ((unsigned)pos < (unsigned)QN) qlist[pos] = r;      // (the counts bound every position)
        }
        // one lane per voxel advances its position (LDS is in order inside one wave)
        if (live && rank == total - 1) pos_of[v] = pos_of[v] + total;
    }
}

// Slot sum + query route of ONE slot: g1 [QN, H] are the gradient rows of the slot's cloud, list [b, e) the slot's queries.  Wave w owns
// the columns [256 w, 256 w + 256), lane l the float4 at 256 w + 4 l.  For every query of the list, in list order:
//   gs_row[:] += g1[qn, :]                                  (one chain per element, list order)
//   dq[qn, c] = sum_w wave_sum( g1[qn, cols of w] . Wq[c, cols of w] ),  c = 0..2   (fixed tree per wave, waves ascending)
// gs_row = NULL or dq = NULL: that half is skipped.  Every list entry is clamped into [0, QN).
__device__ __forceinline__ void slot_sum_rows(const float* __restrict__ g1, const int32_t* __restrict__ qlist, int b, int e, int QN, int H,
                                              const float* __restrict__ Wq /* W1p + E H: three rows */, float* __restrict__ gs_row,
                                              float* __restrict__ dq, float (*s_part)[16][3]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int col = 256 * wave + 4 * lane;
    const bool has = col < H;
    float4 w0 = make_float4(0.f, 0.f, 0.f, 0.f), w1 = w0, w2 = w0, acc = w0;
    if (dq && has) {
        w0 = *reinterpret_cast<const float4*>(Wq + col);
        w1 = *reinterpret_cast<const float4*>(Wq + (size_t)H + col);
        w2 = *reinterpret_cast<const float4*>(Wq + 2 * (size_t)H + col);
    }
    for (int p0 = b; p0 < e; p0 += kSlotRows) {
        const int np = min(kSlotRows, e - p0);
        for (int p = 0; p < np; ++p) {
            int qn = qlist[p0 + p];
            qn = min(max(qn, 0), QN - 1);
            float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
            if (has) x = *reinterpret_cast<const float4*>(g1 + (size_t)qn * H + col);
            acc.x += x.x; acc.y += x.y; acc.z += x.z; acc.w += x.w;
            if (dq) {
                const float d0 = wave_sum(((x.x * w0.x + x.y * w0.y) + x.z * w0.z) + x.w * w0.w);
                const float d1 = wave_sum(((x.x * w1.x + x.y * w1.y) + x.z * w1.z) + x.w * w1.w);
                const float d2 = wave_sum(((x.x * w2.x + x.y * w2.y) + x.z * w2.z) + x.w * w2.w);
                if (lane == 0) { s_part[p][wave][0] = d0; s_part[p][wave][1] = d1; s_part[p][wave][2] = d2; }
            }
        }
        if (dq) {
            __syncthreads();
            for (int x = threadIdx.x; x < np * 3; x += blockDim.x) {
                const int p = x / 3, c = x % 3;
                float d = s_part[p][0][c];
                for (int w = 1; w < nw; ++w) d += s_part[p][w][c];
                int qn = qlist[p0 + p];
                qn = min(max(qn, 0), QN - 1);
                dq[(size_t)qn * 3 + c] = d;
            }
            __syncthreads();
        }
    }
    if (gs_row && has) *reinterpret_cast<float4*>(gs_row + col) = acc;
}

// Window scatter over the U slots of ONE cloud, as a gather (the form of patch_rows_bwd.h), by a workgroup of 256 threads that owns the
// voxels [gbeg, gend) of the cloud: for every (voxel, float4 channel group) it sums that window column of every slot whose window covers
// the voxel, in ascending slot order.  A voxel outside the grid has no item: zero padding at the border.  Every item is computed by ONE
// thread from the same loads in the same order whatever the launch shape is.  slot_vox [U] and dXs [U, KP] point at the cloud's slot 0,
// dfv [m^3, 20] at the cloud's vector; U <= 1024 (s_vox [1024]).  accumulate: the chain starts from the value dfv holds, else from +0.0.
__device__ __forceinline__ void scatter_slots(const float* __restrict__ dXs, const int32_t* __restrict__ slot_vox, int U,
                                              float* __restrict__ dfv, int m, int k, int KP, int gbeg, int gend, bool accumulate, int* s_vox) {
    constexpr int kCh = DPD_FV_CHANNELS;
    const int tid = threadIdx.x;
    const int G = m * m * m, h = (k - 1) / 2;
    for (int n = tid; n < U; n += 256) {
        int v = slot_vox[n];
        if ((unsigned)v >= (unsigned)G) v = 0;
        s_vox[n] = (v / (m * m)) | (((v / m) % m) << 8) | ((v % m) << 16);
    }
    __syncthreads();
    for (int item = tid; item < (gend - gbeg) * 5; item += 256) {
        const int g = gbeg + item / 5, part = item % 5;
        const int g0 = g / (m * m) + h, g1 = (g / m) % m + h, g2 = g % m + h;
        float* out = dfv + (size_t)g * kCh + part * 4;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        if (accumulate) acc = *reinterpret_cast<const float4*>(out);
        for (int n0 = 0; n0 < U; n0 += 64) {
            unsigned long long hm = 0;
            const int lim = min(64, U - n0);
            for (int j = 0; j < lim; ++j) {
                const int pv = s_vox[n0 + j];
                const int d0 = g0 - (pv & 255), d1 = g1 - ((pv >> 8) & 255), d2 = g2 - (pv >> 16);
                if ((unsigned)d0 < (unsigned)k && (unsigned)d1 < (unsigned)k && (unsigned)d2 < (unsigned)k) hm |= 1ull << j;
            }
            while (__any(hm != 0)) {
                float4 x[16];
                bool hit[16];
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    hit[j] = hm != 0;
                    const int bit = hit[j] ? __ffsll((long long)hm) - 1 : 0;
                    hm = hit[j] ? (hm & (hm - 1)) : 0;
                    const int n = n0 + bit;
                    const int pv = s_vox[n];
                    const int d0 = g0 - (pv & 255), d1 = g1 - ((pv >> 8) & 255), d2 = g2 - (pv >> 16);
                    const size_t off = hit[j] ? (size_t)n * KP + ((d0 * k + d1) * k + d2) * kCh + part * 4 : 0;
                    x[j] = *reinterpret_cast<const float4*>(dXs + off);
                }
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    acc.x = hit[j] ? acc.x + x[j].x : acc.x; acc.y = hit[j] ? acc.y + x[j].y : acc.y;
                    acc.z = hit[j] ? acc.z + x[j].z : acc.z; acc.w = hit[j] ? acc.w + x[j].w : acc.w;
                }
            }
        }
        *reinterpret_cast<float4*>(out) = acc;
    }
}

// Query-route reduction by a grid of 256-thread workgroups: gQ[e] = gQ[e] + dq[0, e] + dq[1, e] + ... over the Ca clouds in ascending
// order, e < QN3.  The chain goes on from the accumulated value, so a chunk boundary changes no bit.
__device__ __forceinline__ void qreduce_chain(const float* __restrict__ dq, int Ca, int QN3, float* __restrict__ gQ) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= QN3) return;
    float acc = gQ[e];
    for (int i = 0; i < Ca; ++i) acc = acc + dq[(size_t)i * QN3 + e];
    gQ[e] = acc;
}

}  // namespace dpd

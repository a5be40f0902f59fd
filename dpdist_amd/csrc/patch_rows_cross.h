// Window gather for the ALL-PAIRS distance matrix (exact fp32, the forward; its backward is cross_bwd.hip; included by patch_rows.hip inside
// namespace dpd).
//
// Every cloud of one set (the SURFACE clouds, fv [Ca, m^3, 20]) against every query of the other set (q [Cb, N, 3]): row (i, j, n) of
// the decoder is [window of surface i around the voxel of query (j, n) | q - centre | pad].  The voxel of a query does not depend on
// the surface cloud, so the queries are indexed ONCE (cross_index_kernel: the occupied voxels in ascending voxel id, U of them, at most
// min(m^3, Cb N)) and every surface cloud has the same U windows.  Layer 1 then runs over Ca U slots instead of Ca Cb N rows
// (decoder.hip: dpd_decoder_fwd_cross, the chain of dpd_decoder_fwd_unique):
//   slot_of_vox [m^3]     dense slot of an occupied voxel, -1 otherwise; ucount [1] = U                       (index)
//   Xu [KP - 32, ldu]     k-major: column i U + s = columns [0, KP - 32) of the window of surface i around the voxel of slot s;
//                         nothing else is written
//   Xt [rows_p, 32]       columns [KP - 32, KP) of row (i, j, n); uid [rows_p] = i U + slot of the row's voxel; maskr [rows_p]
//   cnt [4]               {U, Ca U, 0, 0}: cnt[1] is the live slot count layer 1 reads on the device
// rows_p = the rows rounded up to 32 (the finish kernel works on 32-row tiles): pad rows get uid 0, Xt 0, mask 0.
#pragma once

// ---- the two steps of an index workgroup of 1024 threads, shared with patch_rows_field.h ----
// voxel and mask of one query (the cell rule of patch_rows_fwd_kernel); a query that is not `real` (padding) is not read and is masked
__device__ __forceinline__ int index_query(const float* __restrict__ q, bool real, int m, const GridAxis& ax, bool* valid) {
    int ix = -1, iy = -1, iz = -1;
    if (real) {
        const float qx = q[0], qy = q[1], qz = q[2];
        ix = cell_of(ax, m, qx); iy = cell_of(ax, m, qy); iz = cell_of(ax, m, qz);
    }
    *valid = (ix >= 0) && (iy >= 0) && (iz >= 0);
    if (!*valid) { ix = 0; iy = 0; iz = 0; }      // a masked query shares the window of voxel 0 (patch_rows_fwd_kernel)
    return (iy * m + ix) * m + iz;
}
// ballot prefix over the occupancy flags s_occ [1024] (complete, behind a barrier): slot_of_vox [G], ucount [1]
__device__ __forceinline__ void index_slots(const int* s_occ, int* s_wsum, int G, int32_t* __restrict__ slot_of_vox,
                                            int32_t* __restrict__ ucount) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool occ = tid < G && s_occ[tid];
    const unsigned long long b = __ballot(occ);
    if (lane == 0) s_wsum[wave] = __popcll(b);
    __syncthreads();
    int before = 0, all = 0;
    for (int w = 0; w < 16; ++w) {
        const int c = s_wsum[w];
        before += (w < wave) ? c : 0;
        all += c;
    }
    if (tid < G) slot_of_vox[tid] = occ ? before + __popcll(b & ((1ull << lane) - 1ull)) : -1;
    if (tid == 0) ucount[0] = all;
}

// One workgroup: voxel and mask of every query (the cell rule of patch_rows_fwd_kernel), then the occupied voxels in ascending id.
// An occupancy flag per voxel in LDS (plain stores of 1), a ballot prefix over the flags: integer only, one order.
// CNT (dpd_cross_index_counts): query cloud j holds its first counts[j] queries of a row of N (clamped into [1, N] here); a padded query
// is not read and is treated exactly like a query outside the cube, so nothing downstream knows about padding but the denominators.
template <bool CNT>
__device__ __forceinline__ void cross_index_block(const float* __restrict__ q, int QN, int m, const GridAxis& ax, float* __restrict__ mask,
                                                  int32_t* __restrict__ vox, int32_t* __restrict__ slot_of_vox, int32_t* __restrict__ ucount,
                                                  const int32_t* __restrict__ counts, int N) {
    __shared__ int s_occ[1024];      // m <= 10: m^3 <= 1000
    __shared__ int s_wsum[16];
    const int tid = threadIdx.x;
    s_occ[tid] = 0;
    __syncthreads();
    for (int r = tid; r < QN; r += 1024) {
        bool real = true;
        if (CNT) {
            const int j = r / N;
            real = r - j * N < min(max(counts[j], 1), N);
        }
        bool valid;
        const int v = index_query(q + (size_t)r * 3, real, m, ax, &valid);
        mask[r] = valid ? 1.f : 0.f;
        vox[r] = v;
        s_occ[v] = 1;
    }
    __syncthreads();
    index_slots(s_occ, s_wsum, m * m * m, slot_of_vox, ucount);
}

__global__ __launch_bounds__(1024) void cross_index_kernel(const float* __restrict__ q, int QN, int m, GridAxis ax, float* __restrict__ mask,
                                                           int32_t* __restrict__ vox, int32_t* __restrict__ slot_of_vox,
                                                           int32_t* __restrict__ ucount) {
    cross_index_block<false>(q, QN, m, ax, mask, vox, slot_of_vox, ucount, nullptr, 0);
}
__global__ __launch_bounds__(1024) void cross_index_counts_kernel(const float* __restrict__ q, const int32_t* __restrict__ counts, int QN, int N,
                                                                  int m, GridAxis ax, float* __restrict__ mask, int32_t* __restrict__ vox,
                                                                  int32_t* __restrict__ slot_of_vox, int32_t* __restrict__ ucount) {
    cross_index_block<true>(q, QN, m, ax, mask, vox, slot_of_vox, ucount, counts, N);
}

// patch_rows_fwd_unique_kernel for one surface cloud against all queries: kCrossChunks workgroups per surface cloud, each with the
// cloud's scaled Fisher vector in LDS (the uq_* pieces of patch_rows_unique.h: same products, same bits as the plain gather).  Chunk c writes its share of the units of
// Xu (wave = float4 unit of the window, lane = slot: four dword stores of U x 4 contiguous bytes) and its share of the surface's
// rows of Xt, uid and maskr; workgroup 0 also writes the pad rows and the counts.
constexpr int kCrossChunks = 8;
__global__ __launch_bounds__(512) void patch_rows_cross_kernel(const float* __restrict__ q, const int32_t* __restrict__ vox,
                                                               const float* __restrict__ maskq, const int32_t* __restrict__ slot_of_vox,
                                                               const int32_t* __restrict__ ucount, int ucap, const float* __restrict__ fv,
                                                               float* __restrict__ XuT, int ldu, float* __restrict__ Xt,
                                                               int32_t* __restrict__ uid, float* __restrict__ maskr, int32_t* __restrict__ cnt,
                                                               int Ca, int QN, int rows_p, int m, int k, int KP, GridAxis ax,
                                                               const float* __restrict__ ssq, int nsl, unsigned mg_k, unsigned mg_kk) {
    extern __shared__ __attribute__((aligned(16))) int2 s_tabx[];             // [KP/4] unit table, the scaled vector [G*kF] fp32, then per slot / per voxel
    const int U = KP / 4, UW = U - 8;                                         // float4 units of a row; of its Xu part
    const int G = m * m * m, GF = G * kF;
    float* s_fv = reinterpret_cast<float*>(s_tabx + U);
    UqRow* s_rec = reinterpret_cast<UqRow*>(s_fv + GF);                       // [G] window record of slot s
    int* s_slot = reinterpret_cast<int*>(s_rec + G);                          // [G] slot of voxel v
    __shared__ __attribute__((aligned(16))) float s_sc[kF];
    const int tid = threadIdx.x;
    const int cloud = blockIdx.x % Ca, chunk = blockIdx.x / Ca;               // the chunks of a cloud share an XCD when Ca is a multiple of 8
    const float4* fvc = reinterpret_cast<const float4*>(fv + (size_t)cloud * GF);
    const int nv = GF / 4;
    float4 pre[kUqPre];
    uq_prefetch(fvc, nv, tid, pre);
    if (tid < kF) s_sc[tid] = ssq ? fv_scale(ssq, nsl, cloud, tid) : 1.0f;
    const int nslots = min(max(ucount[0], 0), ucap);                          // (the capacity the host sized Xu for bounds every store)
    for (int v = tid; v < G; v += 512) {
        int sl = slot_of_vox[v];
        if (sl >= nslots) sl = -1;
        s_slot[v] = sl;
        if (sl >= 0) {
            const int iy = v / (m * m), ix = (v / m) % m, iz = v % m;
            s_rec[sl] = uq_record(iy, ix, iz, m, k);
        }
    }
    uq_build_table(s_tabx, U, m, k, mg_k, mg_kk, tid);
    __syncthreads();
    uq_stage(s_fv, s_sc, ssq != nullptr, fvc, nv, tid, pre);
    __syncthreads();
    const float4 no_dq = make_float4(0.f, 0.f, 0.f, 0.f);
    const int wv = tid >> 6, lane = tid & 63;
    const int base = cloud * nslots;
    // ---- the surface's rows (i, j, n) of this chunk: Xt, uid, maskr ----
    {
        const int per = (QN + kCrossChunks - 1) / kCrossChunks;
        const int n0 = chunk * per, n1 = min(QN, n0 + per);
        for (int i = tid; i < 8 * (n1 - n0); i += 512) {
            const int n = n0 + (i >> 3), j = UW + (i & 7);
            int v = vox[n];
            if ((unsigned)v >= (unsigned)G) v = 0;
            const int sl = max(s_slot[v], 0);
            const size_t row = (size_t)cloud * QN + n;
            const int2 e = s_tabx[j];
            float4 dq = no_dq;
            if ((e.y >> 24) == 1) {
                const int iy = v / (m * m), ix = (v / m) % m, iz = v % m;
                dq = make_float4(q[(size_t)n * 3] - ax.c[ix], q[(size_t)n * 3 + 1] - ax.c[iy], q[(size_t)n * 3 + 2] - ax.c[iz], 0.f);   // point_cloud - Centers (:491)
            }
            const float4 x = uq_unit(s_fv, e, s_rec[sl], dq);
            *reinterpret_cast<float4*>(Xt + row * 32 + 4 * (j - UW)) = x;
            if ((i & 7) == 0) {
                uid[row] = base + sl;
                maskr[row] = maskq[n];
            }
        }
    }
    if (blockIdx.x == 0) {
        const int rows = Ca * QN;
        for (int i = tid; i < 8 * (rows_p - rows); i += 512) {
            const size_t row = (size_t)rows + (i >> 3);
            *reinterpret_cast<float4*>(Xt + row * 32 + 4 * (i & 7)) = make_float4(0.f, 0.f, 0.f, 0.f);
            if ((i & 7) == 0) { uid[row] = 0; maskr[row] = 0.f; }
        }
        if (tid == 0) { cnt[0] = nslots; cnt[1] = Ca * nslots; cnt[2] = 0; cnt[3] = 0; }
    }
    // ---- the surface's windows: wave = unit, lane = slot ----
    const int per = (UW + kCrossChunks - 1) / kCrossChunks;
    const int j1 = min(UW, (chunk + 1) * per);
    for (int j = chunk * per + wv; j < j1; j += 8) {
        const int2 e = s_tabx[j];
        for (int s0 = 0; s0 < nslots; s0 += 64) {
            const int sl = s0 + lane;
            if (sl < nslots) {
                const float4 v = uq_unit(s_fv, e, s_rec[sl], no_dq);      // (units < UW are window units: the host checks k^3 * 20 >= KP - 32)
                float* d = XuT + (size_t)(4 * j) * ldu + base + sl;
                d[0] = v.x; d[ldu] = v.y; d[2 * (size_t)ldu] = v.z; d[3 * (size_t)ldu] = v.w;
            }
        }
    }
}

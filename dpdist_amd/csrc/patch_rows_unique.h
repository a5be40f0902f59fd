// Window gather over DISTINCT windows (exact fp32 training step; included by patch_rows.hip inside namespace dpd).
//
// Row r = c*N + n of X is [k^3 x 20 window of cloud c around the voxel of query n | q - centre | pad]: the window depends on
// (cloud, voxel) only, and the 64 queries of a cloud fall into ~40 voxels.  Layer 1 therefore runs its first KP - 32 contraction steps
// once per distinct window and a finish kernel (decoder.hip: l1_finish_kernel) continues every row's accumulator chain with the
// last K-tile, which holds the columns that differ between rows.  What this file produces for it:
//   uid [Q]            slot of row r's window: the first row of its cloud with the same voxel owns the slot; slots are dense and in
//                      row order, [0, U_AB) for the rows < BN (the half that carries gradient), a gap up to U_ABp = roundup(U_AB, 32),
//                      then the other half up to M_u = U_ABp + U_BA
//   XuT [KP - 32, Q + 32]  columns [0, KP - 32) of the slot's window, one COLUMN per slot (k-major), gap columns zero; nothing else is
//                      written.  k-major because layer 1 then reads it like a weight gradient reads its activations (32 lanes = 128
//                      contiguous bytes of one k): with 32 x 32 wave tiles -- the granularity that lets ~2600 rows fill 1024 SIMDs in
//                      three rounds -- the row-major form pays one cache line per lane and load and was measured no faster than
//                      the 4096-row product (docs/EXPERIMENTS.md)
//   Xt [Q, 32]         columns [KP - 32, KP) of every row: the window's last values, q - centre, the zero pad
//   cnt [4]            {U_AB, M_u, U_ABp, 0} -- device words, never read by the host
// Two launches: the index (one wave per cloud: voxel of every query, first occurrence, dense slot inside the cloud, slots per
// cloud) and the gather (the LDS form of patch_rows_fwd_lds_kernel: row workgroups for X[:x_rows] and their Xt, cloud workgroups
// for XuT, uid and the other rows' Xt; every cloud workgroup adds up the slot counts of the clouds before its own).
#pragma once

// one wave per cloud; lu [Q] = slot of the row's window INSIDE its cloud, first [Q] = the row owns it, ucount [C] = slots of the cloud
__global__ __launch_bounds__(64) void window_index_kernel(const float* __restrict__ q, int N, int m, GridAxis ax, float* __restrict__ mask,
                                                           int32_t* __restrict__ vox, int32_t* __restrict__ lu,
                                                           int32_t* __restrict__ first, int32_t* __restrict__ ucount) {
    extern __shared__ int s_ix[];            // [N] voxel of the cloud's queries, then [N] slot of the rows that own one
    int* s_v = s_ix;
    int* s_slot = s_ix + N;
    const int c = blockIdx.x, lane = threadIdx.x;
    for (int n = lane; n < N; n += 64) {
        const size_t r = (size_t)c * N + n;
        const float qx = q[r * 3], qy = q[r * 3 + 1], qz = q[r * 3 + 2];
        int ix = cell_of(ax, m, qx), iy = cell_of(ax, m, qy), iz = cell_of(ax, m, qz);
        const bool valid = (ix >= 0) && (iy >= 0) && (iz >= 0);
        if (!valid) { ix = 0; iy = 0; iz = 0; }      // a masked query shares the window of voxel 0 (patch_rows_fwd_kernel)
        const int v = (iy * m + ix) * m + iz;
        s_v[n] = v;
        mask[r] = valid ? 1.f : 0.f;
        vox[r] = v;
    }
    __syncthreads();
    int running = 0;
    for (int n0 = 0; n0 < N; n0 += 64) {             // wave-uniform trip count
        const int n = n0 + lane;
        int f = n;
        if (n < N) {
            const int v = s_v[n];
            for (int j = n - 1; j >= 0; --j)
                if (s_v[j] == v) f = j;              // the FIRST row with this voxel
        }
        const bool own = n < N && f == n;
        const unsigned long long b = __ballot(own);
        if (own) s_slot[n] = running + __popcll(b & ((1ull << lane) - 1ull));
        running += __popcll(b);
        __syncthreads();                             // (one wave: orders the LDS writes before the reads below)
        if (n < N) {
            lu[(size_t)c * N + n] = s_slot[f];       // f <= n: written in this or an earlier round
            first[(size_t)c * N + n] = own ? 1 : 0;
        }
    }
    if (lane == 0) ucount[c] = running;
}

// patch_rows_fwd_lds_kernel with two kinds of workgroup, both on the cloud's scaled Fisher vector in LDS (same products, same bits):
//   blocks [0, x_rows / 8)          8 rows each, wave = row: the whole row of X (the weight gradient of layer 1 still contracts over
//                                   rows) and its Xt;
//   then kUqChunks blocks per cloud the cloud's slots as columns of XuT: wave = float4 unit of the window, lane = slot, four dword
//                                   stores of (slots of the cloud) x 4 contiguous bytes; chunk 0 also writes uid and the Xt of the rows
//                                   >= x_rows, cloud 0 the gap columns, its chunk 0 the counts.
constexpr int kUqChunks = 4;
struct UqRow {
    int own;          // offset of the row's own voxel in the cloud's vector
    unsigned vbits;   // validity bits of the displacements: axis a, d -> bit 8a + d
};
// ---- pieces of the LDS form shared by the gathers over distinct windows (this kernel and patch_rows_cross_kernel) ----
constexpr int kUqPre = 5;                                                     // m = 8: 2560 float4 of a cloud's vector = 5 per thread of 512
// the first kUqPre float4 per thread of a cloud's Fisher vector, requested before anything else
__device__ __forceinline__ void uq_prefetch(const float4* __restrict__ fvc, int nv, int tid, float4 (&pre)[kUqPre]) {
#pragma unroll
    for (int i = 0; i < kUqPre; ++i) {
        const int idx = tid + 512 * i;
        pre[i] = idx < nv ? fvc[idx] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}
// the cloud's vector into LDS, scaled per channel when scaled (fv * scale: the products of the plain gather)
__device__ __forceinline__ void uq_stage(float* s_fv, const float* s_sc, bool scaled, const float4* __restrict__ fvc, int nv, int tid,
                                         const float4 (&pre)[kUqPre]) {
    auto stage = [&](int idx, float4 x) {
        if (scaled) {
            const float4 sc = *reinterpret_cast<const float4*>(&s_sc[(idx % 5) * 4]);
            x.x *= sc.x; x.y *= sc.y; x.z *= sc.z; x.w *= sc.w;
        }
        *reinterpret_cast<float4*>(s_fv + 4 * idx) = x;
    };
#pragma unroll
    for (int i = 0; i < kUqPre; ++i)
        if (tid + 512 * i < nv) stage(tid + 512 * i, pre[i]);
    for (int idx = tid + 512 * kUqPre; idx < nv; idx += 512) stage(idx, fvc[idx]);
}
// unit table [U]: {offset in floats from the row's own voxel, d0 | d1 << 8 | d2 << 16 | kind << 24}; kind 0 window, 1 q - centre, 2 pad
__device__ __forceinline__ void uq_build_table(int2* s_tab, int U, int m, int k, unsigned mg_k, unsigned mg_kk, int tid) {
    const int E4 = k * k * k * (kF / 4), h = (k - 1) / 2;
    for (int j = tid; j < U; j += 512) {
        int2 e = make_int2(0, (j == E4 ? 1 : 2) << 24);
        if (j < E4) {
            const int nb = j / 5, part = j - 5 * nb;
            const int d0 = (int)(((unsigned)nb * mg_kk) >> 16), r = nb - d0 * k * k;
            const int d1 = (int)(((unsigned)r * mg_k) >> 16), d2 = r - d1 * k;
            e = make_int2((((d0 - h) * m + (d1 - h)) * m + (d2 - h)) * kF + part * 4, d0 | (d1 << 8) | (d2 << 16));
        }
        s_tab[j] = e;
    }
}
// window record of voxel (iy, ix, iz)
__device__ __forceinline__ UqRow uq_record(int iy, int ix, int iz, int m, int k) {
    const int h = (k - 1) / 2;
    unsigned vb = 0;
    for (int d = 0; d < k; ++d) {
        if ((unsigned)(iy - h + d) < (unsigned)m) vb |= 1u << d;
        if ((unsigned)(ix - h + d) < (unsigned)m) vb |= 1u << (8 + d);
        if ((unsigned)(iz - h + d) < (unsigned)m) vb |= 1u << (16 + d);
    }
    return UqRow{((iy * m + ix) * m + iz) * kF, vb};
}
// float4 unit with table entry e of the row with record (rw, dq)
__device__ __forceinline__ float4 uq_unit(const float* s_fv, const int2 e, const UqRow rw, const float4 dq) {
    const int kind = e.y >> 24;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (kind == 0) {
        if ((rw.vbits >> (e.y & 0xff)) & (rw.vbits >> (8 + ((e.y >> 8) & 0xff))) & (rw.vbits >> (16 + ((e.y >> 16) & 0xff))) & 1u)
            v = *reinterpret_cast<const float4*>(s_fv + rw.own + e.x);
    } else if (kind == 1) {
        v = dq;
    }
    return v;
}

__global__ __launch_bounds__(512) void patch_rows_fwd_unique_kernel(const float* __restrict__ q, const float* __restrict__ fv,
                                                                    float* __restrict__ X, int x_rows, float* __restrict__ XuT, int ldu,
                                                                    float* __restrict__ Xt, const int32_t* __restrict__ lu,
                                                                    const int32_t* __restrict__ first, const int32_t* __restrict__ ucount,
                                                                    int32_t* __restrict__ uid, int32_t* __restrict__ cnt, int Q, int N, int BN,
                                                                    int m, int k, int KP, GridAxis ax, const float* __restrict__ ssq, int nsl,
                                                                    unsigned mg_k, unsigned mg_kk) {
    extern __shared__ __attribute__((aligned(16))) int2 s_tab4[];             // [KP/4] unit table, the scaled vector [G*kF] fp32, then per row of the cloud
    const int U = KP / 4, UW = U - 8;                                         // float4 units of a row; of its XuT part
    const int G = m * m * m, GF = G * kF;
    float* s_fv = reinterpret_cast<float*>(s_tab4 + U);
    float4* s_dq = reinterpret_cast<float4*>(s_fv + GF);                      // [N] (q - centre, 0)        (row blocks use 8 entries)
    UqRow* s_row = reinterpret_cast<UqRow*>(s_dq + N);                        // [N]
    int* s_slotrow = reinterpret_cast<int*>(s_row + N);                       // [N] row (inside the cloud) that owns slot j
    __shared__ __attribute__((aligned(16))) float s_sc[kF];
    __shared__ int s_base[3];                                                 // slots before this cloud's; U_AB; slots of all clouds
    const int tid = threadIdx.x;
    const int clouds = Q / N, rgpc = N / 8, nrow = x_rows / 8;
    const bool rowblk = (int)blockIdx.x < nrow;
    int rg = blockIdx.x, cloud, chunk = 0;
    if (rowblk) {
        if (!((x_rows / N) & 7)) {                // cloud c on XCD c % 8 (one L2 per cloud), as in the plane form
            const int xcd = blockIdx.x & 7, i = blockIdx.x >> 3;
            rg = ((i / rgpc) * 8 + xcd) * rgpc + i % rgpc;
        }
        cloud = (8 * rg) / N;
    } else {                                      // consecutive blocks = consecutive clouds: the chunks of cloud c share an XCD when the counts are multiples of 8
        const int i = blockIdx.x - nrow;
        cloud = i % clouds; chunk = i / clouds;
    }
    const float4* fvc = reinterpret_cast<const float4*>(fv + (size_t)cloud * GF);
    const int nv = GF / 4;
    float4 pre[kUqPre];
    uq_prefetch(fvc, nv, tid, pre);
    if (tid < kF) s_sc[tid] = ssq ? fv_scale(ssq, nsl, cloud, tid) : 1.0f;
    // row records: the 8 rows of a row block, all N rows of a cloud block
    const int r_first = rowblk ? 8 * rg : cloud * N, r_count = rowblk ? 8 : N;
    for (int n = tid - 64; n >= 0 && n < r_count; n += 448) {                 // (threads 64 .. 511: the first wave fetches the scales)
        const int r = r_first + n;
        const float qx = q[(size_t)r * 3], qy = q[(size_t)r * 3 + 1], qz = q[(size_t)r * 3 + 2];
        int ix = cell_of(ax, m, qx), iy = cell_of(ax, m, qy), iz = cell_of(ax, m, qz);
        const bool valid = (ix >= 0) && (iy >= 0) && (iz >= 0);
        if (!valid) { ix = 0; iy = 0; iz = 0; }
        s_dq[n] = make_float4(qx - ax.c[ix], qy - ax.c[iy], qz - ax.c[iz], 0.f);       // point_cloud - Centers (:491)
        s_row[n] = uq_record(iy, ix, iz, m, k);
        if (!rowblk && first[r]) s_slotrow[lu[r]] = n;
    }
    if (!rowblk && tid < 64) {                    // one wave: slot counts of the clouds (integer sums: any order gives the same words)
        const int ab = BN / N;
        int before = 0, uab = 0, all = 0;
        for (int c = tid; c < clouds; c += 64) {
            const int n = ucount[c];
            before += (c < cloud) ? n : 0;
            uab += (c < ab) ? n : 0;
            all += n;
        }
        for (int off = 32; off; off >>= 1) {
            before += __shfl_xor(before, off, 64);
            uab += __shfl_xor(uab, off, 64);
            all += __shfl_xor(all, off, 64);
        }
        if (tid == 0) { s_base[0] = before; s_base[1] = uab; s_base[2] = all; }
    }
    uq_build_table(s_tab4, U, m, k, mg_k, mg_kk, tid);
    __syncthreads();
    uq_stage(s_fv, s_sc, ssq != nullptr, fvc, nv, tid, pre);
    __syncthreads();
    // float4 unit j of the row with record (rw, dq)
    auto unit = [&](int j, const UqRow rw, const float4 dq) { return uq_unit(s_fv, s_tab4[j], rw, dq); };
    const int wv = tid >> 6, lane = tid & 63;
    if (rowblk) {                                 // wave = row
        const int row = 8 * rg + wv;
        const UqRow rw = s_row[wv];
        const float4 dq = s_dq[wv];
        float* xr = X + (size_t)row * KP;
        for (int j = lane; j < U; j += 64) {
            const float4 v = unit(j, rw, dq);
            *reinterpret_cast<float4*>(xr + 4 * j) = v;
            if (j >= UW) *reinterpret_cast<float4*>(Xt + (size_t)row * 32 + 4 * (j - UW)) = v;
        }
        return;
    }
    const int u_ab = s_base[1], u_abp = (u_ab + 31) & ~31;
    const int r0 = cloud * N;
    const int base = s_base[0] + (r0 >= BN ? u_abp - u_ab : 0), nslots = ucount[cloud];
    if (chunk == 0) {
        for (int n = tid; n < N; n += 512) uid[r0 + n] = base + lu[r0 + n];
        for (int i = tid; i < 8 * N; i += 512) {                              // Xt of the rows no row block writes
            const int n = i >> 3, j = UW + (i & 7);
            if (r0 + n >= x_rows) *reinterpret_cast<float4*>(Xt + (size_t)(r0 + n) * 32 + 4 * (j - UW)) = unit(j, s_row[n], s_dq[n]);
        }
        if (cloud == 0 && tid == 0) { cnt[0] = u_ab; cnt[1] = u_abp + (s_base[2] - u_ab); cnt[2] = u_abp; cnt[3] = 0; }
    }
    const int per = (UW + kUqChunks - 1) / kUqChunks;
    const int j1 = min(UW, (chunk + 1) * per);
    for (int j = chunk * per + wv; j < j1; j += 8) {                          // wave = unit, lane = slot
        for (int s0 = 0; s0 < nslots; s0 += 64) {
            const int sl = s0 + lane;
            if (sl < nslots) {
                const int n = s_slotrow[sl];
                const float4 v = unit(j, s_row[n], s_dq[n]);
                float* d = XuT + (size_t)(4 * j) * ldu + base + sl;
                d[0] = v.x; d[ldu] = v.y; d[2 * (size_t)ldu] = v.z; d[3 * (size_t)ldu] = v.w;
            }
        }
        if (cloud == 0 && u_ab + lane < u_abp) {                              // the gap columns (< 32)
            float* d = XuT + (size_t)(4 * j) * ldu + u_ab + lane;
            d[0] = 0.f; d[ldu] = 0.f; d[2 * (size_t)ldu] = 0.f; d[3 * (size_t)ldu] = 0.f;
        }
    }
}

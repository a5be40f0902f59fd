// Window gather for the PER-POINT FIELD (exact fp32, forward; included by patch_rows.hip inside namespace dpd).
//
// Every cloud of a chunk (the SURFACE clouds, fv [n, m^3, 20]) against T queries of its OWN (q + c * q_cloud_stride; stride 0: one query
// set shared by all clouds): row (c, t) of the decoder is [window of surface c around the voxel of its query t | q - centre | pad].  The
// window depends on (cloud, voxel) only, so layer 1 runs over the sum of the clouds' occupied voxels U_c <= min(m^3, T) instead of over
// n T rows (decoder.hip: dpd_decoder_fwd_field, the chain of dpd_decoder_fwd_unique):
//   slot_of_vox [n, m^3]  dense slot INSIDE cloud c of an occupied voxel, in ascending voxel id, -1 otherwise; ucount [n] = U_c   (index)
//   Xu [KP - 32, ldu]     k-major: column base_c + s = columns [0, KP - 32) of the window of surface c around the voxel of its slot s,
//                         base_c = the sum of U_c' over c' < c (cloud-major); nothing else is written
//   Xt [rows_p, 32]       columns [KP - 32, KP) of row (c, t); uid [rows_p] = base_c + slot of the row's voxel; maskr [rows_p]
//   cnt [4]               {n, sum U_c, 0, 0}: cnt[1] is the live slot count layer 1 reads on the device
// rows_p = n T rounded up to 32: pad rows get uid 0, Xt 0, mask 0.
#pragma once

// One workgroup per cloud: voxel and mask of its T queries, then its occupied voxels in ascending id (index_query / index_slots of
// patch_rows_cross.h: integer only, one order).  qcounts (may be NULL): query t of the chunk is query t0 + t of its cloud, and is padding
// when t0 + t >= max(qcounts[c], 1): not read, masked, voxel 0 (as in cross_index_counts_kernel).
__global__ __launch_bounds__(1024) void field_index_kernel(const float* __restrict__ q, long q_cloud_stride, const int32_t* __restrict__ qcounts,
                                                           int t0, int T, int m, GridAxis ax, float* __restrict__ mask,
                                                           int32_t* __restrict__ vox, int32_t* __restrict__ slot_of_vox,
                                                           int32_t* __restrict__ ucount) {
    __shared__ int s_occ[1024];      // m <= 10: m^3 <= 1000
    __shared__ int s_wsum[16];
    const int tid = threadIdx.x, c = blockIdx.x, G = m * m * m;
    const float* qc = q + (size_t)c * q_cloud_stride;
    const int real_t = qcounts ? max(qcounts[c], 1) - t0 : T;      // queries [0, real_t) of the chunk are real
    s_occ[tid] = 0;
    __syncthreads();
    for (int t = tid; t < T; t += 1024) {
        bool valid;
        const int v = index_query(qc + (size_t)t * 3, t < real_t, m, ax, &valid);
        mask[(size_t)c * T + t] = valid ? 1.f : 0.f;
        vox[(size_t)c * T + t] = v;
        s_occ[v] = 1;
    }
    __syncthreads();
    index_slots(s_occ, s_wsum, G, slot_of_vox + (size_t)c * G, ucount + c);
}

// patch_rows_cross_kernel for clouds with their own queries and their own slots: `chunks` workgroups per cloud, each with the cloud's
// Fisher vector in LDS (the uq_* pieces of patch_rows_unique.h: same values, same bits as the plain gather).  Every workgroup adds up the
// slot counts of the clouds before its own (integer sums: any order gives the same words), as patch_rows_fwd_unique_kernel does.  Chunk
// i writes its share of the units of the cloud's columns of Xu (wave = float4 unit of the window, lane = slot) and its share of the
// cloud's rows of Xt, uid and maskr; workgroup 0 also writes the pad rows and the counts.  ucap = min(m^3, T) bounds a cloud's slots, so
// every column written lies below n ucap <= the capacity the host sized Xu for.
__global__ __launch_bounds__(512) void patch_rows_field_kernel(const float* __restrict__ q, long q_cloud_stride, const int32_t* __restrict__ vox,
                                                               const float* __restrict__ maskq, const int32_t* __restrict__ slot_of_vox,
                                                               const int32_t* __restrict__ ucount, int ucap, const float* __restrict__ fv,
                                                               float* __restrict__ XuT, int ldu, float* __restrict__ Xt,
                                                               int32_t* __restrict__ uid, float* __restrict__ maskr, int32_t* __restrict__ cnt,
                                                               int n, int T, int chunks, int rows_p, int m, int k, int KP, GridAxis ax,
                                                               unsigned mg_k, unsigned mg_kk) {
    extern __shared__ __attribute__((aligned(16))) int2 s_tabf[];             // [KP/4] unit table, the vector [G*kF] fp32, then per slot / per voxel
    const int U = KP / 4, UW = U - 8;                                         // float4 units of a row; of its Xu part
    const int G = m * m * m, GF = G * kF;
    float* s_fv = reinterpret_cast<float*>(s_tabf + U);
    UqRow* s_rec = reinterpret_cast<UqRow*>(s_fv + GF);                       // [G] window record of slot s
    int* s_slot = reinterpret_cast<int*>(s_rec + G);                          // [G] slot of voxel v
    __shared__ int s_base[2];                                                 // slots before this cloud's; slots of all clouds
    const int tid = threadIdx.x;
    const int cloud = blockIdx.x % n, chunk = blockIdx.x / n;                 // the chunks of a cloud share an XCD when n is a multiple of 8
    const float4* fvc = reinterpret_cast<const float4*>(fv + (size_t)cloud * GF);
    const int nv = GF / 4;
    float4 pre[kUqPre];
    uq_prefetch(fvc, nv, tid, pre);
    const int nslots = min(max(ucount[cloud], 0), ucap);
    if (tid < 64) {                               // one wave: slot counts of the clouds, each bounded like this cloud's
        int before = 0, all = 0;
        for (int c = tid; c < n; c += 64) {
            const int u = min(max(ucount[c], 0), ucap);
            before += (c < cloud) ? u : 0;
            all += u;
        }
        for (int off = 32; off; off >>= 1) {
            before += __shfl_xor(before, off, 64);
            all += __shfl_xor(all, off, 64);
        }
        if (tid == 0) { s_base[0] = before; s_base[1] = all; }
    }
    const int32_t* sov = slot_of_vox + (size_t)cloud * G;
    for (int v = tid; v < G; v += 512) {
        int sl = sov[v];
        if (sl >= nslots) sl = -1;
        s_slot[v] = sl;
        if (sl >= 0) {
            const int iy = v / (m * m), ix = (v / m) % m, iz = v % m;
            s_rec[sl] = uq_record(iy, ix, iz, m, k);
        }
    }
    uq_build_table(s_tabf, U, m, k, mg_k, mg_kk, tid);
    __syncthreads();
    uq_stage(s_fv, nullptr, false, fvc, nv, tid, pre);      // (the vectors are normalised: copied as they are)
    __syncthreads();
    const float4 no_dq = make_float4(0.f, 0.f, 0.f, 0.f);
    const int wv = tid >> 6, lane = tid & 63;
    const int base = s_base[0];
    // ---- the cloud's rows (c, t) of this chunk: Xt, uid, maskr ----
    {
        const float* qc = q + (size_t)cloud * q_cloud_stride;
        const int per = (T + chunks - 1) / chunks;
        const int n0 = min(T, chunk * per), n1 = min(T, n0 + per);
        for (int i = tid; i < 8 * (n1 - n0); i += 512) {
            const int t = n0 + (i >> 3), j = UW + (i & 7);
            const size_t row = (size_t)cloud * T + t;
            int v = vox[row];
            if ((unsigned)v >= (unsigned)G) v = 0;
            const int sl = max(s_slot[v], 0);
            const int2 e = s_tabf[j];
            float4 dq = no_dq;
            if ((e.y >> 24) == 1) {
                const int iy = v / (m * m), ix = (v / m) % m, iz = v % m;
                dq = make_float4(qc[(size_t)t * 3] - ax.c[ix], qc[(size_t)t * 3 + 1] - ax.c[iy], qc[(size_t)t * 3 + 2] - ax.c[iz], 0.f);   // point_cloud - Centers (:491)
            }
            const float4 x = uq_unit(s_fv, e, s_rec[sl], dq);
            *reinterpret_cast<float4*>(Xt + row * 32 + 4 * (j - UW)) = x;
            if ((i & 7) == 0) {
                uid[row] = base + sl;
                maskr[row] = maskq[row];
            }
        }
    }
    if (blockIdx.x == 0) {
        const size_t rows = (size_t)n * T;
        for (int i = tid; i < 8 * (int)(rows_p - rows); i += 512) {
            const size_t row = rows + (i >> 3);
            *reinterpret_cast<float4*>(Xt + row * 32 + 4 * (i & 7)) = make_float4(0.f, 0.f, 0.f, 0.f);
            if ((i & 7) == 0) { uid[row] = 0; maskr[row] = 0.f; }
        }
        if (tid == 0) { cnt[0] = n; cnt[1] = s_base[1]; cnt[2] = 0; cnt[3] = 0; }
    }
    // ---- the cloud's windows: wave = unit, lane = slot ----
    const int per = (UW + chunks - 1) / chunks;
    const int j1 = min(UW, (chunk + 1) * per);
    for (int j = chunk * per + wv; j < j1; j += 8) {
        const int2 e = s_tabf[j];
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

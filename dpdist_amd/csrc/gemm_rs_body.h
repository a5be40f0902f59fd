// The wave body of the register-streamed GEMM (gemm_rs.h), as TEXT: included inside a kernel, once per problem the kernel runs.
// In scope where it is included: the configuration as constants -- AK, BKC (bool), TM, TN, WR, WC, D (int), DM, DK, CS2 (bool), see
// gemm_rs.h -- a GemmArgs `g` the text may change, and `bid`, the workgroup's id among the workgroups of THIS problem.  A wave that
// has no output returns from the kernel.
// Why text and not a __device__ __forceinline__ function: behind a function boundary hipcc compiles the SAME statements differently
// (the 32x32-tile kernels come out with 119 VGPRs instead of 135, the NT forms with 176 / 146 / 142 instead of 185 / 148 / 152) and
// the training step measured 2.8 us SLOWER with those kernels and nothing else changed (docs/EXPERIMENTS.md G10).  Included like this,
// gemm_rs_kernel is the code it was.
    constexpr int BM = 32 * TM * WR, BN = 32 * TN * WC;
    if (DM) g.M = min(g.M, __builtin_amdgcn_readfirstlane(*g.M_dev));
    const int Kcap = g.K;      // what the operands hold: the buffer ranges below stay those of the capacity
    if (DK) g.K = max(0, min(g.K, __builtin_amdgcn_readfirstlane(*g.K_dev))) & ~31;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, half = lane >> 5;

    const int tilesM = (g.M + BM - 1) / BM, tilesN = (g.N + BN - 1) / BN;
    const int per_z = tilesM * tilesN;
    const int ngrp = g.A2 ? 2 : 1;
    // (the XCD map below is taken over the LIVE tile count: over the capacity, the dead tiles would be the high ids and whole XCDs idle)
    if (DM && bid >= per_z * g.split_k * ngrp) return;
    int grp = 0, z, t;
    unsigned kbeg, kend;
    if (g.tail_split > 1) {     // whole-K tiles first, then the K pieces of the last round's tiles
        const int sid = xcd_remap(bid, g.tail_first + (per_z - g.tail_first) * g.tail_split);
        if (sid < g.tail_first) { t = sid; z = 0; kbeg = 0; kend = g.K; }
        else {
            const int u = sid - g.tail_first;
            t = g.tail_first + u / g.tail_split; z = u % g.tail_split;
            kbeg = z * g.tail_chunk; kend = min(g.K, (int)kbeg + g.tail_chunk);
        }
    } else {
        const int sid = xcd_remap(bid, per_z * g.split_k * ngrp);
        grp = sid / (per_z * g.split_k);
        const int sid1 = sid % (per_z * g.split_k);
        z = sid1 / per_z; t = sid1 % per_z;
        kbeg = z * g.k_chunk; kend = min(g.K, (int)kbeg + g.k_chunk);
    }
    const int m0 = (t / tilesN) * BM + (wave / WC) * 32 * TM, n0 = (t % tilesN) * BN + (wave % WC) * 32 * TN;
    if (m0 >= g.M || n0 >= g.N) return;   // ragged edge: this wave has no output (no barriers anywhere, so it may leave)
    const int nt = (int)(kend - kbeg) / 32;
    const float* gA = grp ? g.A2 : g.A;
    const float* gB = grp ? g.B2 : g.B;
    const unsigned lda = g.lda, ldb = g.ldb;

    const __amdgpu_buffer_rsrc_t ra = rs_rsrc(gA, AK ? ((size_t)(g.M - 1) * lda + Kcap) * 4 : ((size_t)(Kcap - 1) * lda + g.M) * 4);
    const __amdgpu_buffer_rsrc_t rb = rs_rsrc(gB, BKC ? ((size_t)(g.N - 1) * ldb + Kcap) * 4 : ((size_t)(Kcap - 1) * ldb + g.N) * 4);
    unsigned va[TM], vb[TN];
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const unsigned r = min(m0 + 32 * i + l31, g.M - 1);
        va[i] = AK ? (r * lda + 16u * half) * 4u : (16u * half * lda + r) * 4u;
    }
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const unsigned c = min(n0 + 32 * j + l31, g.N - 1);
        vb[j] = BKC ? (c * ldb + 16u * half) * 4u : (16u * half * ldb + c) * 4u;
    }

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // ---- epilogue operands, requested before the main loop (they depend on nothing computed here): the bias value of this
    // lane's column and, for the ReLU-gate epilogue of the backward data GEMMs, the 16 gate values per accumulator tile.  Held
    // in registers when the wave tile is small enough (<= 2 accumulator tiles); otherwise fetched at the end like before.
    constexpr bool PRE = TM * TN <= 2;
    const int epi = g.epi;
    float ebias[TN], egate[PRE ? TM : 1][PRE ? TN : 1][16];
#pragma unroll
    for (int j = 0; j < TN; ++j)
        ebias[j] = (epi == EPI_BIAS || epi == EPI_BIAS_RELU) ? g.bias[min(n0 + 32 * j + l31, g.N - 1)] : 0.f;
    if (PRE && epi == EPI_GATE && g.split_k == 1) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = min(m0 + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * half, g.M - 1);
                    egate[i][j][r] = g.gate[(size_t)row * g.ldc + min(n0 + 32 * j + l31, g.N - 1)];
                }
    }
    RsFrag fa[D][TM], fb[D][TN];
    // all loads of K-tile kt (clamped to the last tile: a redundant reload instead of a branch) into register set d
    auto load_step = [&](int kt, int d, int b, int s) {
        const int ktc = DK ? max(min(kt, nt - 1), 0) : min(kt, nt - 1);      // (DK: no live K-tile at all -> tile 0 of the capacity, loaded and never used)
        const unsigned k0 = kbeg + 32u * ktc;
#pragma unroll
        for (int i = 0; i < TM; ++i) rs_load_step<AK>(ra, va[i], k0, lda, b, s, fa[d][i]);
#pragma unroll
        for (int j = 0; j < TN; ++j) rs_load_step<BKC>(rb, vb[j], k0, ldb, b, s, fb[d][j]);
    };
    // One K-tile: 16 steps of TM*TN MFMAs on register set `cur`; the loads of K-tile `kt_next` go into set `nxt` in the
    // same (b, s) order in which they will be consumed.  sched_barrier pins [loads of the step | MFMAs of the step]: left
    // alone, the machine scheduler sinks the loads to the end of the tile and halves the prefetch distance.
    auto tile = [&](int cur, int nxt, int kt_next, bool do_load) {
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                if (do_load) load_step(kt_next, nxt, b, s);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[cur][i].v[b][s], fb[cur][j].v[b][s], acc[i][j], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
    };

    // prologue: K-tiles 0 .. D-2 in flight
#pragma unroll
    for (int d = 0; d < D - 1; ++d)
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
            for (int s = 0; s < 4; ++s) load_step(d, d, b, s);
    // The loop body is branch-free on purpose: with a conditional load hipcc's waitcnt pass must assume the not-taken path
    // and waits for the loads it has just issued; a straight-line body gets the exact counted vmcnt.
    int kt = 0;
    for (; kt + D <= nt; kt += D) {
#pragma unroll
        for (int j = 0; j < D; ++j) tile(j, (j + D - 1) % D, kt + j + D - 1, true);
    }
    // remainder (< D tiles): their operands are already in flight in sets 0 .. rem-1
#pragma unroll
    for (int j = 0; j < D - 1; ++j)
        if (kt + j < nt) tile(j, 0, 0, false);

    GemmArgs gs = g;
    if (grp) gs.C = g.C2;
    if (g.tail_split > 1 && z > 0) {      // K piece of a tail tile: its own slab, dense [M, N]
        gs.C = g.tail_slab + (size_t)(z - 1) * g.M * g.N;
        gs.ldc = g.N;
    }
    const int zs = (g.tail_split > 1) ? 0 : z;     // slab index for put_tile (split-K slabs only)
    // Bias gradient, second step (see GemmArgs::colsum_part): the first row block's waves add the 32-row partial column sums an
    // EARLIER launch stored, in block order -> deterministic, no atomics, no extra launch.  (Adding them up inside the K loop of
    // this kernel instead was measured 25 % slower on the dW GEMMs: VALU work between the dependent MFMAs of a single accumulator.)
    float* csb_out = grp ? g.colsum_b2 : g.colsum_b;
    const float* csb_in = grp ? g.colsum_part_in2 : g.colsum_part_in;
    if (!CS2 && csb_out && csb_in && m0 == 0 && z == 0 && half == 0) {
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int col = n0 + 32 * j + l31;
            if (col < g.N) {
                float t = 0.f;
                for (int pb0 = 0; pb0 < g.colsum_nparts; pb0 += 16) {     // 16 loads in flight, added in block order
                    float v[16];
#pragma unroll
                    for (int u = 0; u < 16; ++u) v[u] = (pb0 + u < g.colsum_nparts) ? csb_in[(size_t)(pb0 + u) * g.N + col] : 0.f;
#pragma unroll
                    for (int u = 0; u < 16; ++u) t += v[u];
                }
                csb_out[col] = t;
            }
        }
    }
    // CS2 (a launch that is not grouped): both pairs of pointers -- the live-row chain's dW1 launch finishes db1 and db2: the same N
    // columns, each the same block-order sum as in the launch that finished it before.  The second sum belongs to the waves of the NEXT
    // 32 * TM rows, so that the two run side by side and no wave's tail carries both (one after the other they cost dW1 3.8 us,
    // docs/EXPERIMENTS.md G10)
    if (CS2 && z == 0 && half == 0) {
        const int m0_second = g.M > 32 * TM ? 32 * TM : 0;
        if (m0 == 0) rs_colsum_finish<TN>(g.colsum_b, g.colsum_part_in, g.colsum_nparts, g.N, n0, l31);
        if (m0 == m0_second) rs_colsum_finish<TN>(g.colsum_b2, g.colsum_part_in2, g.colsum_nparts, g.N, n0, l31);
    }
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            if (PRE && g.split_k == 1 && epi != EPI_NONE) {     // epilogue on the preloaded operands (same arithmetic as tile_values)
                float v[16];
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    float x = acc[i][j][r] + ebias[j];
                    if (epi == EPI_BIAS_RELU) x = fmaxf(x, 0.f);
                    if (epi == EPI_GATE) x = (egate[i][j][r] > 0.f) ? x : 0.f;
                    v[r] = x;
                }
                put_tile(gs, v, zs, m0 + 32 * i, n0 + 32 * j + l31, half);
            } else {
                store_tile(gs, acc[i][j], zs, m0 + 32 * i, n0 + 32 * j + l31, half);
            }
        }

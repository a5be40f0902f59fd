// The chunk workspace of the ALL-PAIRS engine, stated once (host only; included by patch_rows.hip and cross_bwd.hip, which hold the two
// workspace reports; dpd_cross_carve in patch_rows.hip hands the pointers out -- include/dpdist_capi.h: dpd_cross_chunk).
#pragma once
#include "common.h"

namespace dpd {

// the decoder rows of a chunk, rounded up to 32 (the finish kernel works on 32-row tiles)
inline size_t cross_rows_p(int Ca_chunk, int Cb, int N) { return ((size_t)Ca_chunk * Cb * N + 31) / 32 * 32; }
// the occupied voxels one surface cloud can have: U <= min(m^3, Cb N)
inline int cross_ucap(int Cb, int N, int m) {
    const long G = (long)m * m * m, qn = (long)Cb * N;
    return (int)(G < qn ? G : qn);
}

struct CrossMember {
    void* dpd_cross_chunk::*field;
    size_t bytes;
};
constexpr int kCrossMembers = 19;

// THE layout of a chunk: the members of the forward or of the backward form in order, each rounded up to 256 bytes when summed or
// carved.  The shape is taken as given (the predicates of the two reports come first).  -> the number of members
inline int cross_chunk_members(int Ca_chunk, int Cb, int N, int m, int KP, int H, bool backward, CrossMember out[kCrossMembers]) {
    using C = dpd_cross_chunk;
    const size_t cap = (size_t)dpd_cross_slot_capacity(Ca_chunk, Cb, N, m), rows_p = cross_rows_p(Ca_chunk, Cb, N);
    const size_t act = rows_p * H * 4, row3 = rows_p * 3 * 4, slots = cap * H * 4;
    int n = 0;
    auto put = [&](void* C::*f, size_t b) { out[n++] = CrossMember{f, b}; };
    put(&C::Xu, (size_t)(KP - 32) * cap * 4); put(&C::Xt, rows_p * 32 * 4); put(&C::uid, rows_p * 4); put(&C::maskr, rows_p * 4);
    put(&C::cnt, 16); put(&C::Pu, slots);
    if (!backward) {
        put(&C::act0, act); put(&C::act1, act); put(&C::y, row3); put(&C::pred, row3); put(&C::Dd, (size_t)Ca_chunk * Cb * 4);
    } else {
        put(&C::h1, act); put(&C::h2, act); put(&C::h3, act); put(&C::y, row3); put(&C::pred, row3);
        put(&C::dpred, row3); put(&C::dy, row3); put(&C::ga, act); put(&C::gb, act); put(&C::dq, row3); put(&C::gs, slots);
        put(&C::dXs, cap * (size_t)KP * 4); put(&C::dfv, (size_t)Ca_chunk * m * m * m * DPD_FV_CHANNELS * 4);
    }
    return n;
}

inline size_t cross_al256(size_t b) { return (b + 255) / 256 * 256; }

inline size_t cross_chunk_bytes(int Ca_chunk, int Cb, int N, int m, int KP, int H, bool backward) {
    CrossMember mem[kCrossMembers];
    const int n = cross_chunk_members(Ca_chunk, Cb, N, m, KP, H, backward, mem);
    size_t total = 0;
    for (int i = 0; i < n; ++i) total += cross_al256(mem[i].bytes);
    return total;
}

}  // namespace dpd

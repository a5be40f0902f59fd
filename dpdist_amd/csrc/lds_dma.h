// The LDS-DMA piece and its counted wait, and the accumulator type of the 32x32 MFMA: what the GEMM units (through gemm_shared.h) and the
// pose network's shared MLP (pose_point.hip, through pose_int.h) both build on.  One definition of the inline assembly.
#pragma once
#include "common.h"

namespace dpd {

typedef float f32x16 __attribute__((ext_vector_type(16)));

typedef __attribute__((address_space(3))) void* lds_ptr_t;

// One 1-KiB LDS-DMA piece: LDS[dst + lane*16] <- 16 bytes at this lane's source address.
// Inline asm on purpose: with the builtin, hipcc knows an LDS write is pending and drains vmcnt(0) before the next
// ds_read, which serialises the ring.  Here the pieces are invisible to its waitcnt bookkeeping and are retired by the
// counted s_waitcnt vmcnt(N) in the K-loop (every piece is one VM_CNT event).  M0 is written in the same statement
// that uses it and restored afterwards.
__device__ __forceinline__ void dma_piece(const void* src, unsigned dst_bytes) {
    unsigned keep;
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %2\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %1, off\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(src), "s"(dst_bytes)
        : "memory");
}

template <int N>
__device__ __forceinline__ void wait_vmcnt() {
    if (N == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    else if (N == 1) asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
    else if (N == 2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
    else if (N == 3) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
    else if (N == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else if (N == 6) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    else if (N == 8) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else if (N == 9) asm volatile("s_waitcnt vmcnt(9)" ::: "memory");
    else if (N == 12) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

}  // namespace dpd

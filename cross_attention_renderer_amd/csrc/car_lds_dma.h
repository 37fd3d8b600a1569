// car_lds_dma.h — the LDS-DMA instruction sequence and the vector-memory wait of the kernels that stream weights or rows L2 -> LDS
// (car_linear.hip, car_fused.hip, car_mma_tile.h and its users — car_fused_mma.h, car_row_sweep.h —, car_raychain.hip).  Included INSIDE the including file's anonymous
// namespace, like car_split.h.  The callers keep their own address arithmetic, readfirstlane and CAR_BOUNDS_TRAP checks: they know
// their extents.
#pragma once

typedef __attribute__((address_space(3))) void lds_void;

// LDS-DMA: 16 bytes per lane from global memory straight into LDS at M0 (lds_dst: a wave-uniform LDS byte address) + lane * 16.
// Issued through inline asm on purpose: hipcc orders every ds_read behind an LDS-DMA it knows about (s_waitcnt vmcnt(0) before the
// first ds_read of the chunk), which would serialise the weight stream with the MFMAs.  Hidden from the compiler, the DMA for chunk
// c + 1 flies under the MFMAs of chunk c; the caller's explicit wait_vm + barrier at the end of a chunk orders it before the next
// chunk's reads.
// gsrc: a 64-bit global address per lane
__device__ __forceinline__ void lds_dma16(const float* gsrc, unsigned lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
}
// sbase: a wave-uniform (scalar) global base, voff: the lane's byte offset from it — no 64-bit vector address arithmetic per piece
__device__ __forceinline__ void lds_dma16(const float* sbase, unsigned voff, unsigned lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %3\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(voff), "s"(lds_dst), "s"(sbase) : "memory");
}
// at most N of this wave's vector memory operations (LDS-DMA pieces included; they return in order) still outstanding
template <int N>
__device__ __forceinline__ void wait_vm() {
    static_assert(N >= 0 && N < 64, "vmcnt is a 6-bit count");
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

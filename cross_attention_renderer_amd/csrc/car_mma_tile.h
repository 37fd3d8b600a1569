// car_mma_tile.h — the v_mfma_f32_16x16x32_f16 tile pieces that need no chunk table: the vector types, one LDS-DMA piece of a weight
// chunk and the chunk barrier, the split-fp16 / fp16 B operands, the MFMA pair and the accumulator helpers.  The fused per-sample kernel
// takes them through car_fused_mma.h (which adds its chunk table and the chained layers), the row sweep of car_linear16.hip and
// car_conv.hip through car_row_sweep.h.
// Included INSIDE the kernel file's anonymous namespace, after it has defined kWaves (waves per workgroup = DMA participants).
//
// Split-fp16 arithmetic: x = hi + lo with fp16 halves, three products per term (hi*hi + hi*lo + lo*hi, fp32 accumulate; the
// dropped lo*lo is 2^-22 relative).  fp16 keeps 11 bits only between 2^-14 and 65504, so both operands are moved into that
// window by powers of two, undone exactly on the fp32 side: a layer's weights carry 2^shift chosen at pack time from the layer's
// largest weight (car_plan_build), the activations a power of two chosen from their largest magnitude — per sample for the
// chained layers (the whole input vector sits in registers), per launch for the first layer (bounded by the maxima of the
// projected maps) — so that the largest value lands in [2^13, 2^14): no overflow, and everything within 2^-17 of the largest
// value keeps its full 22 bits.
//
// F16 (the opt-in render precision, car_render_forward_f16): ONE product per term.  The weights come from the compact blob of
// car_plan_f16_build (hi-only tiles of 1 KB, each value rounded to nearest after the same 2^shift), the B operands are rounded to
// nearest by one v_cvt_pk_f16_f32 per pair after the same powers of two; accumulation stays fp32.
#pragma once

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 half8 __attribute__((ext_vector_type(8)));
#include "car_lds_dma.h"

#include "car_fused_layout.h"      // kTile, kTileHi: the packed floats per (K step, tile)

// Descriptor of the chunk to prefetch, resolved once per chunk with scalar branches so the per-piece issue is straight-line
struct NextChunk {
    const float* src; float* dst; int nkb;
#ifdef CAR_BOUNDS
    const float* lim = nullptr;        // one past the packed array the chunk lies in (nullptr: unknown to this kernel)
#endif
};
// piece p of the next chunk: wave w copies KB number kWaves p + w (wrapped into the chunk: re-copying identical bytes is harmless).
// LDS-DMA: car_lds_dma.h.  Must only run after the barrier that retired the buffer's previous chunk.
__device__ __forceinline__ void stream_issue_piece(const NextChunk& n, int p, int lane, int wave) {
    int kb = kWaves * p + wave;
    kb = kb < n.nkb ? kb : kb - n.nkb;
    kb = kb < n.nkb ? kb : kb - n.nkb;
    // a piece index that two subtractions do not bring back into the chunk would copy 1 KB from BEHIND it (the row sweep before 0d74f26:
    // three pieces issued for a four-KB chunk); and no piece may leave the packed array
    CAR_BOUNDS_TRAP(kb >= 0 && kb < n.nkb);
#ifdef CAR_BOUNDS
    {   // 32-bit arithmetic on the distance (a 64-bit pointer compare would move the address computation below into vector registers)
        const int room = n.lim ? (int)(n.lim - n.src) : 0x7fffffff;
        CAR_BOUNDS_TRAP((kb + 1) * 256 <= room);
    }
#endif
    // `wave` is scalar, so both addresses are: scalar base + the lane's 16 bytes (no 64-bit vector address arithmetic per piece)
    const unsigned lds_dst = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)(lds_void*)(n.dst + kb * 256));
    const float* gsrc = n.src + kb * 256;
#ifdef CAR_BOUNDS
    {   // the checks' branches make the compiler lose sight of the address being wave-uniform: say so again for the "s" operand below
        const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)gsrc), hi = __builtin_amdgcn_readfirstlane((unsigned)((uintptr_t)gsrc >> 32));
        gsrc = reinterpret_cast<const float*>(((uintptr_t)hi << 32) | lo);
    }
#endif
    const unsigned voff = 16u * (unsigned)lane;
    lds_dma16(gsrc, voff, lds_dst);
}
// end of a chunk: the DMA of the next chunk has landed and every wave is done reading the current one.  KEEP = number of
// vector loads this wave issued AFTER its last DMA piece and wants to leave in flight across the barrier (loads return in
// order, so "at most KEEP outstanding" still means every DMA piece has landed).
template <int KEEP = 0>
__device__ __forceinline__ void stream_sync() {
    wait_vm<(KEEP == 16 || KEEP == 8 || KEEP == 4 ? KEEP : 0)>();      // the counts the streams were tuned with; any other KEEP waits for all
    __syncthreads();
}

#include "car_split.h"

// F16: x * p (or x, already scaled) rounded to nearest fp16, one v_cvt_pk_f16_f32 per pair
typedef _Float16 half2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void cvt8_scaled(const float (&x)[8], half8& h) {
#pragma unroll
    for (int e = 0; e < 8; e += 2) {
        const half2v v = __builtin_convertvector(f32x2{x[e], x[e + 1]}, half2v);
        h[e] = v[0]; h[e + 1] = v[1];
    }
}
__device__ __forceinline__ void cvt8(const float (&x)[8], float p, half8& h) {
    float y[8];
    const f32x2 p2 = {p, p};
#pragma unroll
    for (int e = 0; e < 8; e += 2) {
        const f32x2 v = f32x2{x[e], x[e + 1]} * p2;
        y[e] = v[0]; y[e + 1] = v[1];
    }
    cvt8_scaled(y, h);
}
// B operand of one K step in the precision of the instance: split into (hi, lo), or rounded once into hi
template <bool F16>
__device__ __forceinline__ void operand8(const float (&x)[8], float p, half8& hi, half8& lo) {
    if constexpr (F16) cvt8(x, p, hi);
    else split8(x, p, hi, lo);
}

// largest magnitude of a sample's values: the sample's row is spread over NT x 4 registers of the four lanes (s, q = 0..3)
template <int NT, bool RELU>
__device__ __forceinline__ float sample_max(const f32x4 (&v)[NT]) {
    float m = 0.0f;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) m = fmaxf(m, RELU ? v[t][r] : fabsf(v[t][r]));
    m = fmaxf(m, __shfl_xor(m, 16, 64));
    return fmaxf(m, __shfl_xor(m, 32, 64));
}

// two output tiles x three split products, interleaved so consecutive MFMAs never share an accumulator.  F16: one product each, from
// the compact tiles (w0, w1 one KB apart), blo unused
template <bool F16 = false>
__device__ __forceinline__ void mfma_pair(f32x4& c0, f32x4& c1, const float* w0, const float* w1, const half8& bhi, const half8& blo) {
    if constexpr (F16) {
        const half8 a0 = __builtin_bit_cast(half8, *reinterpret_cast<const float4*>(w0));
        const half8 a1 = __builtin_bit_cast(half8, *reinterpret_cast<const float4*>(w1));
        c0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(a0, bhi, c0, 0, 0, 0);
        c1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1, bhi, c1, 0, 0, 0);
        return;
    }
    const half8 ah0 = __builtin_bit_cast(half8, *reinterpret_cast<const float4*>(w0));
    const half8 ah1 = __builtin_bit_cast(half8, *reinterpret_cast<const float4*>(w1));
    const half8 al0 = __builtin_bit_cast(half8, *reinterpret_cast<const float4*>(w0 + 256));
    const half8 al1 = __builtin_bit_cast(half8, *reinterpret_cast<const float4*>(w1 + 256));
    c0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah0, bhi, c0, 0, 0, 0);
    c1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah1, bhi, c1, 0, 0, 0);
    c0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah0, blo, c0, 0, 0, 0);
    c1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah1, blo, c1, 0, 0, 0);
    c0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(al0, bhi, c0, 0, 0, 0);
    c1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(al1, bhi, c1, 0, 0, 0);
}

// accumulators start at bias * scale: lane (s, q) register r of tile t holds channel 16 t + 4 q + r
template <int NT>
__device__ __forceinline__ void init_bias(f32x4 (&acc)[NT], const float* lbias, int q, float scale) {
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const float4 b4 = *reinterpret_cast<const float4*>(lbias + 16 * t + 4 * q);
        acc[t][0] = b4.x * scale; acc[t][1] = b4.y * scale; acc[t][2] = b4.z * scale; acc[t][3] = b4.w * scale;
    }
}
template <int NT>
__device__ __forceinline__ void scale_acc(f32x4 (&acc)[NT], float f) {
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] *= f;
}
template <int NT>
__device__ __forceinline__ void store_rows(const f32x4 (&acc)[NT], float* row, int q) {
#pragma unroll
    for (int t = 0; t < NT; ++t)
        *reinterpret_cast<float4*>(row + 16 * t + 4 * q) = make_float4(acc[t][0], acc[t][1], acc[t][2], acc[t][3]);
}

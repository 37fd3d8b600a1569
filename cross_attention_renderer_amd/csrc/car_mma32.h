// car_mma32.h — the 32x32x16 split-fp16 tile whose accumulators are the next layer's B operands ("chained"), stated once for the
// per-ray chains (car_raychain.hip) and the second round's per-sample layers (car_round2.hip, car_round2_logit.h).
// Weights are the A operand, the wave's 32 rows (rays, samples) the B operand: lane (s, h) = row s, channel half h.  Arithmetic: fp16
// hi / lo operand halves, three v_mfma_f32_32x32x16_f16 products per term, fp32 accumulation (car_fused_mma.h).
// Included INSIDE the including file's anonymous namespace, as car_split.h is.
#pragma once

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 half8 __attribute__((ext_vector_type(8)));
#include "car_split.h"

// packed floats of one 32-channel tile: a K = 32 chunk is [kg (2)][hi | lo][lane (64)][8 halves], a K = 16 layer [hi | lo][lane][8 halves]
// (car_pack.hip pack32_kernel; the packers know them as kTileFloats in car_chain_layout.h and kTile in car_round2_layout.h)
constexpr int kMma32Tile = 1024, kMma32TileK16 = kMma32Tile / 2;

// the accumulator layout: register r of tile t in a lane of half h holds this channel of the lane's row.  Registers 4 g .. 4 g + 3 are
// the four consecutive channels from mma32_channel(t, 4 g, h) = 32 t + 8 g + 4 h on (the float4 the epilogues read and write), and
// registers 8 kg .. 8 kg + 7 are the lane's B operand of K step (t, kg) of a layer packed in this ("chained") K order
constexpr int mma32_channel(int t, int r, int h) { return 32 * t + (r & 3) + 8 * (r >> 2) + 4 * h; }
// that float4 of a row of channels, for registers 4 g .. 4 g + 3 (the lane's part last: the constant part folds into the load's offset)
__device__ __forceinline__ float4 row4(const float* row, int t, int g, int h) {
    return *reinterpret_cast<const float4*>(row + mma32_channel(t, 4 * g, 0) + mma32_channel(0, 0, h));
}

// acc = f * b[channel], e.g. a bias in the product's units
template <int NT>
__device__ __forceinline__ void set_bias(f32x16 (&acc)[NT], const float* b, float f, int h) {
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = b[mma32_channel(t, r, h)] * f;
}
template <int NT>
__device__ __forceinline__ void zero(f32x16 (&acc)[NT]) {
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
}
template <int NT>
__device__ __forceinline__ void add_bias(f32x16 (&acc)[NT], const float* b, int h) {
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] += b[mma32_channel(t, r, h)];
}

// the A operands of one K step: w = the step's [hi | lo][lane][8 halves] + 4 * lane
__device__ __forceinline__ void read_a(const float* w, half8& ah, half8& al) {
    ah = __builtin_bit_cast(half8, *reinterpret_cast<const float4*>(w));
    al = __builtin_bit_cast(half8, *reinterpret_cast<const float4*>(w + 64 * 4));
}
// acc += (ah + al) (bhi + blo) without the lo . lo term: hi . hi, hi . lo, lo . hi, in this order
__device__ __forceinline__ void mma3(f32x16& acc, const half8& ah, const half8& al, const half8& bhi, const half8& blo) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bhi, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, blo, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bhi, acc, 0, 0, 0);
}

// one tile of a K = 16 layer (one K step, input rows in standard order: lane (s, h) feeds k = 8 h .. 8 h + 7): acc += W[tile t] . x,
// lw = the layer's [tile][hi | lo][lane][8 halves]
__device__ __forceinline__ void mma_k16(f32x16& acc, const float* lw, int t, int lane, const half8& xhi, const half8& xlo) {
    half8 ah, al;
    read_a(lw + t * kMma32TileK16 + 4 * lane, ah, al);
    mma3(acc, ah, al, xhi, xlo);
}

// one chunk (32 values of K = two K steps) of a layer: acc[t] += W[tile t][chunk] . x, wl = the chunk's tiles + 4 * lane, x8[kg] = this
// lane's 8 B-operand values of K step kg, multiplied into the fp16 window by p here
template <int NT>
__device__ __forceinline__ void mma_chunk(f32x16 (&acc)[NT], const float* wl, const float (&x8)[2][8], float p) {
    half8 bhi[2], blo[2];
#pragma unroll
    for (int kg = 0; kg < 2; ++kg) split8(x8[kg], p, bhi[kg], blo[kg]);
    // one wave per SIMD: nobody else hides an LDS round trip, so the A operands of step (t, kg) + 1 are read BEFORE the three products of
    // step (t, kg) are issued (the compiler, left alone, reads them into the same two registers right in front of their first use and
    // waits: ~100 cycles exposed per 96 cycles of MFMA — the chains ran at a third of their matrix time)
    auto read = [&](int i, half8& ah, half8& al) { read_a(wl + (i >> 1) * kMma32Tile + (i & 1) * (kMma32Tile / 2), ah, al); };
    half8 ah[2], al[2];
    read(0, ah[0], al[0]);
#pragma unroll
    for (int i = 0; i < 2 * NT; ++i) {
        const int t = i >> 1, kg = i & 1, cur = i & 1;
        if (i + 1 < 2 * NT) read(i + 1, ah[cur ^ 1], al[cur ^ 1]);
        __builtin_amdgcn_sched_barrier(0);
        mma3(acc[t], ah[cur], al[cur], bhi[kg], blo[kg]);
        __builtin_amdgcn_sched_barrier(0);
    }
}

// car_row_sweep.h — the row-streamed split-fp16 sweep of linear16_kernel (car_linear16.hip) and conv3x3_kernel (car_conv.hip: the 3x3
// convolutions of LPIPS, of the encoder's trunk and of its decoder): Y = X W^T over rows that arrive one 32-wide K step at a time.
// Both operands as fp16 hi / lo halves, three v_mfma_f32_16x16x32_f16 products per term, fp32 accumulation (car_mma_tile.h); the
// layer's weights carry a power of two chosen at pack time, every row a power
// of two that follows the largest magnitude seen so far along the row (when a later K step outgrows it, the row's accumulators are
// moved to the new power of two — an exact multiplication — so a row is read once, not twice), both undone exactly by the caller.
// A workgroup = 12 waves x 16 rows; a wave keeps NT tiles of 16 outputs (wider layers run as column groups of NT tiles); the weight
// chunks (one K step x the group's columns) stream L2 -> LDS by LDS-DMA, double buffered.
// The kernels differ in where a K step's eight values per lane come from, how the accumulators start and how far the row's exponent
// may fall.  What is stated here are the sweep's PIECES; the K loop's dozen lines that call them stand in each kernel's own frame (the
// skeleton at the end of this file).  A loop that lived in a function of its own here was optimised before it was inlined and came out
// scheduled differently, 1 - 2 % slower in some instances (profiles/row_sweep.md); with the skeleton in the kernel the convolution's six
// LPIPS instances and linear16_kernel's four plain ones compile to the very instructions they had when each unit carried the whole text
// (profiles/conv_once.md: the convolution's skeleton stands once, what its callers differ in comes from a compile-time form).
// This arithmetic is shared between exactly these two units — the only includers — and relies on their being compiled with the same flags
// (no extra flags in __graft_entry__.UNITS): a unit that contracted or vectorised differently would no longer give the other's bits.
// Included INSIDE the unit's anonymous namespace, like car_fused_mma.h.
#pragma once

constexpr int kWaves = 12, kRows = 16, kGroupRows = kWaves * kRows;
constexpr int kThreads = 64 * kWaves;
constexpr int kPieces = 3;                         // LDS-DMA pieces of the widest chunk (car_linear16.hip: 18 tiles = 36 KB over 12 waves); narrower
                                                   // column groups take fewer (pieces_of): a piece index past the chunk would copy from beyond it.
                                                   // Read by car_fused_mma.h's chunk_pieces (the KQ tail of car_linear16.hip) and by the text patch of
                                                   // tools/build_bounds.py --reintroduce-0d74f26; the sweep itself asks pieces_of
constexpr int pieces_of(int nt) { return (2 * nt + kWaves - 1) / kWaves; }

#include "car_mma_tile.h"

// ---- where a workgroup works ---------------------------------------------------------------------------------------------------------
// the column groups of a block of rows read the same rows of X: they sit on ONE XCD (workgroup b runs on XCD b % 8) in consecutive
// slots, so the second reader finds the rows in that XCD's L2 — as neighbours in launch order (rounds 4-6) they were on different
// XCDs and a 576-wide layer fetched X twice from the fabric (HBM-bound at 1.3-1.5 ms per 589 824 x 576 x 576 layer)
struct RowPlace {
    long row, lrow;                    // this lane's row, and the row it loads from (the last one where `row` lies beyond M)
    int slot, groups;
    template <int NT> __device__ __forceinline__ int tile0() const { return (slot % groups) * NT; }      // first output tile of the column group
};
// false: a workgroup of the grid's padding (sweep_grid), which has no rows
template <int NT>
__device__ __forceinline__ bool place_rows(int tiles_total, long M, int wave, int s, RowPlace& at) {
    at.groups = tiles_total / NT;
    const int xcd = blockIdx.x & 7;
    at.slot = blockIdx.x >> 3;
    const long rblock = (long)(at.slot / at.groups) * 8 + xcd;
    if (rblock * kGroupRows >= M) return false;                        // the grid is padded to whole rounds of eight row blocks
    at.row = rblock * kGroupRows + wave * kRows + s;
    at.lrow = at.row < M ? at.row : M - 1;
    return true;
}
inline unsigned sweep_grid(long M, int groups) { return car_div_up(car_div_up(M, kGroupRows), 8) * 8 * groups; }

// ---- the weight stream ---------------------------------------------------------------------------------------------------------------
// chunk c of the column group that starts at tile0, into LDS buffer c & 1 of [2][NT][512].  Args: the kernel's argument struct, of which
// this reads Wp ([K step][tiles_total][512]), tiles_total and chunks (K steps)
template <int NT, class Args>
__device__ __forceinline__ NextChunk chunk_desc(const Args& w, int tile0, float* lds, int c) {
    static_assert(kWaves * pieces_of(NT) <= 3 * 2 * NT, "stream_issue_piece wraps a piece index into the chunk with two subtractions");
    const int ce = c < w.chunks ? c : w.chunks - 1;
    NextChunk n;
    n.src = w.Wp + ((long)ce * w.tiles_total + tile0) * kTile;
    n.dst = lds + (ce & 1) * NT * kTile;
    n.nkb = 2 * NT;
#ifdef CAR_BOUNDS
    n.lim = w.Wp + (long)w.chunks * w.tiles_total * kTile;
#endif
    return n;
}
// slot qs of a K step's MFMAs carries piece qs of the next chunk, while there are pieces (pieces_of) and a next chunk (`more`).
// Nothing follows the last chunk: re-copying it onto itself would write the buffer this iteration's MFMAs are reading
template <int NT>
__device__ __forceinline__ void issue_next_piece(const NextChunk& nx, int qs, bool more, int lane, int wave) {
    if (qs < pieces_of(NT) && more) stream_issue_piece(nx, qs, lane, wave);
}

// largest magnitude of the row's values in a K step (the four lanes of a row hold eight each)
__device__ __forceinline__ float row_max(const float (&x)[8]) {
    float m = 0.0f;
#pragma unroll
    for (int e = 0; e < 8; ++e) m = fmaxf(m, fabsf(x[e]));
    m = fmaxf(m, __shfl_xor(m, 16, 64));
    return fmaxf(m, __shfl_xor(m, 32, 64));
}

// "keep where the activation is > 0" (car_relu_mask's rule), four columns at a time
__device__ __forceinline__ float4 keep_where_positive(const float4& v, const float4& act) {
    return make_float4(act.x > 0.0f ? v.x : 0.0f, act.y > 0.0f ? v.y : 0.0f, act.z > 0.0f ? v.z : 0.0f, act.w > 0.0f ? v.w : 0.0f);
}

// ---- the sweep's skeleton, as both kernels write it (conv3x3_kernel: issue_x, finish_x, the start, the clamp and the epilogue take what
// differs between its callers from its Form) ---------------------------------------------------------------------------------------------
//     chunk 0 = chunk_desc<NT>(a, tile0, lds, 0): its pieces_of(NT) pieces go out at once, so what the kernel sets up next (the GATHER
//         instance's taps) runs under the DMA
//     issue_x(0, raw); finish_x(0, raw, xc);            the kernel's row source.  issue only issues the loads of this lane's eight values
//         of K step c (k = 32 c + 8 q4 .. + 7) from valid addresses, finish turns them into values when they are consumed: touching
//         the loaded registers at the load would put the memory latency in front of the K step's MFMAs
//     mrun = max(row_max(xc), 1e-30); pow2_scale<clamp>(mrun, p, pinv); the accumulators' start (bias * p / dW, or zero); split8; stream_sync
//     for c in 0 .. chunks - 1:                          #pragma unroll 1
//         nx = chunk_desc<NT>(a, tile0, lds, c + 1); issue_x(next K step)          in flight under this step's MFMAs
//         for qs in 0 .. NT / 2 - 1: mfma_pair(acc[2 qs], acc[2 qs + 1], ...); issue_next_piece<NT>(nx, qs, c + 1 < chunks, ...); sched_barrier
//         finish_x; mn = row_max(xn); where a lane's mn > mrun (ballot): the row moves to the smaller power of two, scale_acc(pn * pinv), exactly
//         split8(xn, p, bhi, blo); stream_sync
//     the sums are in acc at the row's power of two p (pinv = 1 / p); the epilogue is the kernel's

// car_fused_mma.h — matrix-pipe pieces of the fused per-sample kernel (car_fused.hip) that go through a chunk TABLE: layer / blob
// constants, the weight stream over the table's chunks, the chained layers.  The tile pieces underneath (one LDS-DMA piece, the
// split-fp16 / fp16 operands and their arithmetic, the MFMA pair, the accumulator helpers) are car_mma_tile.h, which needs no table.
// Included INSIDE the kernel file's anonymous namespace, after it has defined kWaves (waves per workgroup = DMA participants)
// and kPieces (LDS-DMA pieces per chunk = ceil(36 / kWaves)); the kernel file then defines chunk_tile_offset / chunk_tiles
// (its order of the weight chunks) and carves its own LDS beyond the two weight buffers.
//
// F16 (the opt-in render precision, car_mma_tile.h): chunks are half the bytes, so the stream needs ceil(18 / kWaves) pieces per chunk
// and its two LDS buffers are half as far apart.
#pragma once

#include "car_mma_tile.h"

constexpr int kStageLd = 36;       // row stride of the wave-private h tile (floats)

// ---- dynamic LDS carve-up (floats) --------------------------------------------------------------------------------
constexpr int kLdsW = 0;                                        // [2][18][512]           weight chunks          72 KB (F16: [2][18][256] in front of it)

// floats per (K step, tile) of a blob and LDS-DMA pieces per chunk, per precision
template <bool F16> __host__ __device__ __forceinline__ constexpr int tile_floats() { return F16 ? kTileHi : kTile; }
template <bool F16> __host__ __device__ __forceinline__ constexpr int chunk_pieces() { return F16 ? (kChunkTiles + kWaves - 1) / kWaves : kPieces; }

__device__ __forceinline__ constexpr int chunk_tile_offset(int g);      // defined by the including kernel file
__device__ __forceinline__ constexpr int chunk_tiles(int g);

// the descriptor (NextChunk, car_mma_tile.h) of chunk g of this kernel file's table
template <bool F16 = false>
__device__ __forceinline__ NextChunk next_chunk(const float* __restrict__ blob, float* lds, int g) {
    constexpr int kTF = tile_floats<F16>();
    const int ge = g < kNumChunks ? g : kNumChunks - 1;            // past the end: re-copy the last chunk onto itself
    NextChunk n;
    n.src = blob + (long)chunk_tile_offset(ge) * kTF;
    n.dst = lds + kLdsW + (ge & 1) * kChunkTiles * kTF;
    n.nkb = (kTF / 256) * chunk_tiles(ge);
#ifdef CAR_BOUNDS
    n.lim = blob + (long)kBlobTiles * kTF;
#endif
    return n;
}
template <bool F16 = false>
__device__ __forceinline__ void stream_issue_all(const float* __restrict__ blob, float* lds, int g, int lane, int wave) {
    if (g >= kNumChunks) return;
    const NextChunk n = next_chunk<F16>(blob, lds, g);
#pragma unroll
    for (int p = 0; p < chunk_pieces<F16>(); ++p) stream_issue_piece(n, p, lane, wave);
}
// one chained layer with 128 outputs over NSRC source tiles (two per K step), weight chunks of two K steps; the source values
// are multiplied by the power of two p on their way into the fp16 split.  `after(m)` runs once K step m has been issued (its two
// source tiles are consumed by then); HOOK_OPS = the number of vector memory instructions it issues per call (they are younger
// than the chunk's DMA pieces and may stay in flight across the chunk barrier).
struct NoHook { __device__ __forceinline__ void operator()(int) const {} };
// G0: index of the layer's first weight chunk.  The chunk order is static, so every chunk's place in the blob, its size and its LDS
// buffer are constants here (resolving them at run time cost a chain of ~20 scalar branches per chunk).
template <int NSRC, bool RELU, int G0, bool F16 = false, int HOOK_OPS = 0, class Hook = NoHook>
__device__ __forceinline__ void chained_layer(f32x4 (&acc)[kTD], const f32x4 (&src)[NSRC], float p, const float* __restrict__ blob,
                                              float* lds, int lane, int wave, Hook after = Hook()) {
    constexpr int kSteps = NSRC / 2, kTF = tile_floats<F16>(), kP = chunk_pieces<F16>();
#pragma unroll
    for (int m0 = 0; m0 < kSteps; m0 += 2) {
        const int nks = m0 + 1 < kSteps ? 2 : 1;
        const int g = G0 + m0 / 2;
        const float* wl = lds + kLdsW + (g & 1) * kChunkTiles * kTF + 4 * lane;
        const NextChunk nx = next_chunk<F16>(blob, lds, g + 1);
#pragma unroll
        for (int kl = 0; kl < 2; ++kl) {
            if (kl < nks) {
                const int m = m0 + kl < kSteps ? m0 + kl : kSteps - 1;
                float x[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    x[e] = src[2 * m + (e >> 2)][e & 3];
                    if (RELU) x[e] = fmaxf(x[e], 0.f);
                }
                half8 bhi, blo;
                operand8<F16>(x, p, bhi, blo);
#pragma unroll
                for (int q = 0; q < kTD / 2; ++q) {
                    const float* w0 = wl + (kl * kTD + 2 * q) * kTF;
                    mfma_pair<F16>(acc[2 * q], acc[2 * q + 1], w0, w0 + kTF, bhi, blo);
                    // every DMA piece of the successor goes out in the first K step's four slots, ahead of the hook's memory
                    // operations: the chunk's closing "at most HOOK_OPS outstanding" must cover all of them
                    if (kl == 0) {
                        if (q < 3) { if (q < kP) stream_issue_piece(nx, q, lane, wave); }
                        else {
#pragma unroll
                            for (int p_ = 3; p_ < kP; ++p_) stream_issue_piece(nx, p_, lane, wave);
                        }
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
                after(m);
            }
        }
        if (nks == 2) stream_sync<2 * HOOK_OPS>(); else stream_sync<HOOK_OPS>();
    }
}

// a K = 16 (+ folded bias) layer with 128 outputs: one K step, B operand (ghi, glo) prepared by the caller
template <bool F16 = false>
__device__ __forceinline__ void small_layer(f32x4 (&acc)[kTD], const half8& ghi, const half8& glo, const float* wl) {
    constexpr int kTF = tile_floats<F16>();
#pragma unroll
    for (int q = 0; q < kTD / 2; ++q) {
        const float* w0 = wl + 2 * q * kTF;
        mfma_pair<F16>(acc[2 * q], acc[2 * q + 1], w0, w0 + kTF, ghi, glo);
    }
}


// car_mha_tile.h — what the attention of the encoder's transformer stage states once for its forward (car_vit.hip: car_mha) and its
// backward (car_vit_backward.hip: car_mha_backward): a tile of 32 rows of one (scene, head) laid out as hi / lo A operands of
// car_mma32.h's chained 32 x 32 x 16 tile in its two forms, the tile's largest magnitudes, the wave that owns 32 rows as B operands,
// and the epilogue of its accumulators.  The loops between prologue and epilogue are the kernels' own.
// Included INSIDE the including file's anonymous namespace, after car_mma32.h and car_vit_layout.h.
#pragma once

constexpr int kStep = kMma32TileK16;               // floats of one K step's A operand: [hi | lo][lane][8 halves]

__device__ __forceinline__ void zero1(f32x16& acc) {
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
}

// ---- the operand forms of a tile: 4 K steps each, thread (step, lane) writes the lane's 8 hi and 8 lo halves of K step `step` ----------
__device__ __forceinline__ void split_nearest(float x, _Float16& hi, _Float16& lo) {
    hi = (_Float16)x;
    lo = (_Float16)(x - (float)hi);
}
__device__ __forceinline__ void store_step(_Float16* form, int step, int lane, const float (&x)[8]) {
    half8 hi, lo;
#pragma unroll
    for (int e = 0; e < 8; ++e) { _Float16 u, l; split_nearest(x[e], u, l); hi[e] = u; lo[e] = l; }
    _Float16* dst = form + (long)step * (2 * kStep);                               // halves: kStep floats = 2 kStep halves
    *reinterpret_cast<half8*>(dst + lane * 8) = hi;
    *reinterpret_cast<half8*>(dst + kStep + lane * 8) = lo;
}
// RC, rows x channels — the A operand of a logit-shaped product: the lane's row is row lane % 32 of the tile, its 8 values channels
// 16 step + 8 (lane / 32) + e of `row`, that row's 64 channels, times the power of two `scale`.  row = null (beyond the scene): zeros.
__device__ __forceinline__ void write_rc(_Float16* form, int step, int lane, const float* row, float scale) {
    float x[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (row) {
        const float* src = row + 16 * step + 8 * (lane >> 5);
        const float4 a0 = *reinterpret_cast<const float4*>(src), a1 = *reinterpret_cast<const float4*>(src + 4);
        x[0] = a0.x * scale; x[1] = a0.y * scale; x[2] = a0.z * scale; x[3] = a0.w * scale;
        x[4] = a1.x * scale; x[5] = a1.y * scale; x[6] = a1.z * scale; x[7] = a1.w * scale;
    }
    store_step(form, step, lane, x);
}
// CR, channels x rows — the A operand of a value-shaped product: step = 2 t + kg, the lane's row is channel 32 t + lane % 32, its 8
// values the tile's rows 16 kg + mma32_channel(0, e, lane / 32), the order in which a logit-shaped product's accumulators hold them
// ("chained"), times `scale`.  at(r, c): channel c of the tile's row r, 0 for a row beyond the scene; a reader that captures by value
// (by reference the backward's pack kernel holds 68 registers in the place of 54 and loses a wave per SIMD, profiles/mha_tile_once.md)
template <class At>
__device__ __forceinline__ void write_cr(_Float16* form, int step, int lane, At at, float scale) {
    const int c = 32 * (step >> 1) + (lane & 31);
    float x[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) x[e] = at(16 * (step & 1) + mma32_channel(0, e, lane >> 5), c) * scale;
    store_step(form, step, lane, x);
}

// largest magnitudes of one tile (block) of T tensors -> maxes[block][T].  row_of(t): the 64 channels of this thread's row (8 threads
// per row, `row` of the scene) in tensor t; rows beyond the scene are not read
template <int T, class RowOf>
__device__ __forceinline__ void tile_absmax(int row, int S, RowOf row_of, float* maxes) {
    __shared__ float red[T][4];
    float m[T];
#pragma unroll
    for (int t = 0; t < T; ++t) m[t] = 0.0f;
    if (row < S) {
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const float* src = row_of(t) + (threadIdx.x & 7) * 8;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const float4 v = *reinterpret_cast<const float4*>(src + 4 * j);
                m[t] = fmaxf(m[t], fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
            }
        }
    }
#pragma unroll
    for (int t = 0; t < T; ++t) m[t] = wave_max(m[t]);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int t = 0; t < T; ++t) red[t][threadIdx.x >> 6] = m[t];
    }
    __syncthreads();
    if (threadIdx.x < T) {
        const float* r = red[threadIdx.x];
        maxes[(long)blockIdx.x * T + threadIdx.x] = fmaxf(fmaxf(r[0], r[1]), fmaxf(r[2], r[3]));
    }
}

// ---- the streaming kernels: one wave = 32 rows of one (scene, head) ---------------------------------------------------------------------
// wave -> its tile of its (scene, head), the lane's row `at` of the scene and `row`, the row it loads: rows beyond the scene are a copy
// of the scene's last row, never stored.  A wave() beyond the call's b heads tiles leaves first (no barrier in these kernels: it may
// leave alone); the check stays in the kernel, so that the decode is straight-line code
struct WaveRows {
    int tile, bh, h, sc, lane, s, hh, at, row;
    static __device__ __forceinline__ long wave() { return (long)blockIdx.x * 4 + (threadIdx.x >> 6); }
    __device__ __forceinline__ WaveRows(int S, int heads, int tiles) {
        tile = (int)(wave() % tiles), bh = (int)(wave() / tiles), h = bh % heads, sc = bh / heads;
        lane = threadIdx.x & 63, s = lane & 31, hh = lane >> 5;
        at = tile * kKeys + s, row = at < S ? at : S - 1;
    }
};
// the wave's own 32 rows of one tensor as B operands: the row's 64 channels (src = the row + 8 hh), one power of two per row -> inv = 1 / p
template <int LO>
__device__ __forceinline__ float load_rows_b(const float* src, half8 (&hi)[4], half8 (&lo)[4]) {
    float x8[4][8];
    float m = 0.0f;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
        const float4 a0 = *reinterpret_cast<const float4*>(src + 16 * ks), a1 = *reinterpret_cast<const float4*>(src + 16 * ks + 4);
        x8[ks][0] = a0.x; x8[ks][1] = a0.y; x8[ks][2] = a0.z; x8[ks][3] = a0.w;
        x8[ks][4] = a1.x; x8[ks][5] = a1.y; x8[ks][6] = a1.z; x8[ks][7] = a1.w;
#pragma unroll
        for (int e = 0; e < 8; ++e) m = fmaxf(m, fabsf(x8[ks][e]));
    }
    m = fmaxf(m, __shfl_xor(m, 32, 64));
    float p, inv;
    pow2_scale<LO>(fmaxf(m, 1e-30f), p, inv);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) split8(x8[ks], p, hi[ks], lo[ks]);
    return inv;
}
// the epilogue: the lane's 2 x 16 accumulators through f, as float4s at the 64 channels dst of the lane's row
template <class F>
__device__ __forceinline__ void store_rows(float* dst, const f32x16 (&acc)[2], int hh, F f) {
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int g = 0; g < 4; ++g)
            *reinterpret_cast<float4*>(dst + mma32_channel(t, 4 * g, hh)) =
                make_float4(f(acc[t][4 * g]), f(acc[t][4 * g + 1]), f(acc[t][4 * g + 2]), f(acc[t][4 * g + 3]));
}

// car_pack.hip — every weight packer of the library.  The split-fp16 operand format is stated here once: a layer's largest magnitude
// (absmax_kernel) gives its power of two (car_split.h pow2_scale), and one writer per MFMA tile shape (pack16_kernel, pack32_kernel) cuts the
// scaled weights into fp16 hi/lo A-operand tiles.  The packers of the C ABI defined here (include/car_hip.h: car_fused_pack,
// car_fused_pack_rows, car_kq_pack, car_round2_pack, car_round2q_pack) and the per-layer ones beside their kernels (car_linear_x3_pack,
// car_chain_pack, car_conv3x3_pack, car_conv3x3_backward_pack) all go through the car_pack_* launchers below (declared in car_common.h).
// Asynchronous, device side only.  car_plan_build / car_plan_f16_build (car_render.hip) and the stage route (engine.py) pack through these entries.
#include "car_common.h"

namespace {

#include "car_fused_layout.h"

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
#include "car_split.h"

constexpr int kTile16 = kTile;                     // floats per (K step, 16-channel tile) of the fused kernel's blob

__device__ __forceinline__ float block_max(float v, float* red) {
    v = wave_max(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float m = 0.0f;
    for (int w = 0; w < (int)(blockDim.x + 63) / 64; ++w) m = fmaxf(m, red[w]);
    __syncthreads();
    return m;
}

// ---- re-layout kernels ---------------------------------------------------------------------------------------------
// Largest |W (+ W2)| of an [N][K] matrix with row stride ldw (and |bias| where the bias is folded in as a column).  A grid of workgroups
// (s.max set): one atomicMax each into *s.max, zeroed by the caller — the bit pattern of a non-negative float orders like an integer.
// (One workgroup reading the whole matrix took 25 us per layer: 0.9 ms of a training step, which re-packs its ~36 forward and
// transposed layers after every optimizer step.)  One workgroup (s.max null; the plan-time packers): its maximum is the layer's, so it
// stores p = 2^shift in *s.p and 1 / p in *s.inv itself.
__global__ void absmax_kernel(const float* __restrict__ W, int ldw, const float* __restrict__ W2, const float* __restrict__ bias, int N, int K,
                              car_pack_scale s) {
    __shared__ float red[16];
    float m = 0.0f;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < (long)N * K; idx += (long)gridDim.x * blockDim.x) {
        const long at = (idx / K) * ldw + idx % K;
        m = fmaxf(m, fabsf(W2 ? W[at] + W2[at] : W[at]));
    }
    if (bias) for (int n = blockIdx.x * blockDim.x + threadIdx.x; n < N; n += gridDim.x * blockDim.x) m = fmaxf(m, fabsf(bias[n]));
    m = block_max(m, red);
    if (threadIdx.x != 0) return;
    if (s.max) {
        atomicMax(reinterpret_cast<unsigned*>(s.max), __float_as_uint(m));
    } else {
        pow2_scale(fmaxf(m, 1e-30f), *s.p, *s.inv);
    }
}
// The layer's power of two inside a tile writer: read from *s.p (stored by a one-workgroup absmax_kernel), or derived by every thread
// from *s.max, the first thread of the grid storing it and its inverse for the consuming kernel (s.max never aliases s.p or s.inv).
__device__ __forceinline__ float layer_pow2(const car_pack_scale& s) {
    if (!s.max) return *s.p;
    float p, inv;
    pow2_scale(fmaxf(*s.max, 1e-30f), p, inv);
    if (blockIdx.x == 0 && threadIdx.x == 0) { *s.p = p; *s.inv = inv; }
    return p;
}

// The scaled weight stays a value of its own in front of its rounding to fp16: left to the compiler, some instances of the writers fuse
// multiplication and rounding into v_fma_mixlo_f16 (x, p, +0), which packs a weight of -0.0 as +0.0, and some do not.
__device__ __forceinline__ void keep_product(float& w) { asm("" : "+v"(w)); }

// Where element (output n; K step ks, lane group q = lane >> 4, element e) of a 16-wide tile comes from.
// Rows of a matrix with stride ldw: k = 32 ks + 8 q + e, or chained over the accumulator order of the layer before,
// k = base + 16 (2 ks + e / 4) + 4 q + e % 4; k == K selects the bias, k > K and n >= N a zero.
struct RowSource {
    const float* W; int ldw; const float* bias; int N, K, chained, base;
    __device__ float operator()(int n, int ks, int q, int e) const {
        const int k = chained ? base + 16 * (2 * ks + e / 4) + 4 * q + e % 4 : 32 * ks + 8 * q + e;
        if (n >= N) return 0.0f;
        return k < K ? W[(long)n * ldw + k] : (k == K && bias ? bias[n] : 0.0f);
    }
};
// torch's [N][K][3][3] convolution weights with k = tap * K + channel.  flip (the data gradient's weights): Wt is the forward layer's
// [K][N][3][3] and the tile holds w'[n][k][tap] = Wt[k][n][8 - tap]
struct ConvSource {
    const float* Wt; int K, N; bool flip;
    __device__ float operator()(int n, int ks, int q, int e) const {
        const int k = 32 * ks + 8 * q + e, tap = k / K, ch = k % K;
        return flip ? Wt[((long)ch * N + n) * 9 + (8 - tap)] : Wt[((long)n * K + ch) * 9 + tap];
    }
};
// A-operand tiles of v_mfma_f32_16x16x32_f16 with fp16 hi/lo halves: [K step][tile][hi|lo][lane][8 halves]; lane l carries output
// 16 t + l % 16 and the eight k its source gives (K step, l >> 4, e).  Values are multiplied by the layer's power of two first.
// HI_ONLY: the compact tiles of the fp16 precision (car_plan_f16_build): the same values and order as the full instance's hi halves
// (rounded to nearest after the layer's power of two), without the lo halves: per (K step, tile) [lane][8 halves], 1 KB.
template <bool HI_ONLY, class Source>
__global__ void pack16_kernel(const Source src, int n_tiles, long total, car_pack_scale s, _Float16* __restrict__ out) {
    const float p = layer_pow2(s);
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int e = (int)(idx & 7), lane = (int)((idx >> 3) & 63);
        const long tile = idx >> 9;
        const int t = (int)(tile % n_tiles), ks = (int)(tile / n_tiles);
        float w = src(16 * t + (lane & 15), ks, lane >> 4, e) * p;
        keep_product(w);
        const _Float16 hi = (_Float16)w;
        if constexpr (HI_ONLY) {
            out[idx] = hi;
        } else {
            _Float16* o = out + tile * 1024 + lane * 8 + e;
            o[0] = hi;
            o[512] = (_Float16)(w - (float)hi);
        }
    }
}
// <Wa r + ba, Wb x + bb> = r^T (M x + v) + u^T x + c for two 128-wide layers that are only ever dotted with each other (the first round's
// key_map_2 / query_embed_2, the second round's query_repeat_embed_2 / query_embed_2; models.py:491, 529, 533, 553-556):
//     M[i][j] = sum_k Wa[k][i] Wb[k][j],  v[i] = sum_k Wa[k][i] bb[k],  u[j] = sum_k Wb[k][j] ba[k],  c = sum_k ba[k] bb[k]
// accumulated in fp64 in ascending k (every product of two fp32 values is exact there) and rounded once to fp32.  One workgroup per row i of M.
__global__ void bilinear_fold_kernel(const float* __restrict__ Wa, const float* __restrict__ ba, const float* __restrict__ Wb,
                                     const float* __restrict__ bb, int D, float* __restrict__ M, float* __restrict__ v, float* __restrict__ u,
                                     float* __restrict__ c) {
    const int i = blockIdx.x, j = threadIdx.x;
    if (j >= D) return;
    double m = 0.0;
    for (int k = 0; k < D; ++k) m += (double)Wa[k * D + i] * (double)Wb[k * D + j];
    M[i * D + j] = (float)m;
    if (j == 0) {
        double s = 0.0;
        for (int k = 0; k < D; ++k) s += (double)Wa[k * D + i] * (double)bb[k];
        v[i] = (float)s;
    }
    if (i == 0) {
        double s = 0.0;
        for (int k = 0; k < D; ++k) s += (double)Wb[k * D + j] * (double)ba[k];
        u[j] = (float)s;
        if (j == 0) {
            double t = 0.0;
            for (int k = 0; k < D; ++k) t += (double)ba[k] * (double)bb[k];
            c[0] = (float)t;
        }
    }
}
// A-operand tiles of v_mfma_f32_32x32x16_f16 (car_round2.hip: 4 tiles; car_raychain.hip: kgs = 2): [chunk][tile][K group kgs][hi|lo][lane]
// [8 halves]; lane l carries output 32 t + l % 32 and, chained, k = 32 c + (e & 3) + 8 (2 kg + (e >> 2)) + 4 (l >> 5) (the accumulator
// order of the layer before), else k = 16 kgs c + 16 kg + 8 (l >> 5) + e.  W2 (optional, same shape and stride) is added element-wise;
// outputs >= N and inputs >= K are zero.
__global__ void pack32_kernel(const float* __restrict__ W, int ldw, const float* __restrict__ W2, int N, int K, int tiles, int kgs, int chained,
                              long total, car_pack_scale s, _Float16* __restrict__ out) {
    const float p = layer_pow2(s);
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int e = (int)(idx & 7), lane = (int)((idx >> 3) & 63), hl = (int)((idx >> 9) & 1);
        long rest = idx >> 10;
        const int kg = (int)(rest % kgs); rest /= kgs;
        const int t = (int)(rest % tiles), c = (int)(rest / tiles);
        const int n = 32 * t + (lane & 31);
        const int k = chained ? 32 * c + (e & 3) + 8 * (2 * kg + (e >> 2)) + 4 * (lane >> 5) : 16 * kgs * c + 16 * kg + 8 * (lane >> 5) + e;
        float w = 0.0f;
        if (n < N && k < K) {
            const long at = (long)n * ldw + k;
            w = (W2 ? W[at] + W2[at] : W[at]) * p;
        }
        keep_product(w);
        const _Float16 hi = (_Float16)w;
        out[idx] = hl == 0 ? hi : (_Float16)(w - (float)hi);
    }
}
// [C][4] table (W1[:, C:C+3], b1) of the per-texel first layer, and the largest row sum of magnitudes (bounds the point / bias
// term of h because |tanh| <= 1).  One workgroup of kC threads.
__global__ void wpt_kernel(const float* __restrict__ w1, const float* __restrict__ b1, float* __restrict__ wpt, float* __restrict__ bound) {
    __shared__ float red[16];
    const int ch = threadIdx.x;
    float m = 0.0f;
    if (ch < kC) {
        const float x = w1[(long)ch * (kC + 3) + kC + 0], y = w1[(long)ch * (kC + 3) + kC + 1], z = w1[(long)ch * (kC + 3) + kC + 2], b = b1[ch];
        wpt[4 * ch + 0] = x; wpt[4 * ch + 1] = y; wpt[4 * ch + 2] = z; wpt[4 * ch + 3] = b;
        m = ((fabsf(x) + fabsf(y)) + fabsf(z)) + fabsf(b);
    }
    m = block_max(m, red);
    if (threadIdx.x == 0) bound[0] = m;
}

}  // namespace

// ---- the launchers every packer goes through (car_common.h) ----------------------------------------------------------------------------
void car_pack_absmax(hipStream_t st, int blocks, const float* W, int ldw, const float* W2, const float* bias, int N, int K, car_pack_scale s) {
    hipLaunchKernelGGL(absmax_kernel, dim3(blocks), dim3(blocks == 1 ? 1024 : 256), 0, st, W, ldw, W2, bias, N, K, s);
}
void car_pack_rows16(hipStream_t st, int blocks, const float* W, int ldw, const float* bias, int N, int K, int n_tiles, int ksteps, int chained,
                     int kbase, car_pack_scale s, _Float16* out, bool hi_only) {
    const RowSource src{W, ldw, bias, N, K, chained, kbase};
    const long total = (long)ksteps * n_tiles * 512;
    if (hi_only) hipLaunchKernelGGL((pack16_kernel<true, RowSource>), dim3(blocks), dim3(256), 0, st, src, n_tiles, total, s, out);
    else hipLaunchKernelGGL((pack16_kernel<false, RowSource>), dim3(blocks), dim3(256), 0, st, src, n_tiles, total, s, out);
}
void car_pack_conv16(hipStream_t st, int blocks, const float* w, int K, int N, bool flip, car_pack_scale s, _Float16* out) {
    hipLaunchKernelGGL((pack16_kernel<false, ConvSource>), dim3(blocks), dim3(256), 0, st, ConvSource{w, K, N, flip}, N / 16, (long)9 * K * N, s, out);
}
void car_pack_tiles32(hipStream_t st, int blocks, const float* W, int ldw, const float* W2, int N, int K, int tiles, int chunks, int kgs, int chained,
                      car_pack_scale s, _Float16* out) {
    hipLaunchKernelGGL(pack32_kernel, dim3(blocks), dim3(256), 0, st, W, ldw, W2, N, K, tiles, kgs, chained, (long)chunks * tiles * kgs * 1024, s, out);
}

namespace {

// ---- what the five packers here share: zero the bias table, one single-workgroup maximum per layer, the pack launches, CAR_CHECK_LAUNCH,
// then device-to-device bias copies ---------------------------------------------------------------------------------------------------
int zero_table(float* bias, size_t n, hipStream_t st, const char* who) {
    if (hipMemsetAsync(bias, 0, sizeof(float) * n, st) != hipSuccess) { car_set_error("%s: memset failed", who); return CAR_E_LAUNCH; }
    (void)hipGetLastError();
    return CAR_OK;
}
// the plan-time forms: one workgroup stores p = 2^shift in p_slot (read by the writers) and 1 / p in down_slot (read by the consuming kernel)
void layer_scale(hipStream_t st, const float* W, int ldw, int N, int K, const float* b, float* p_slot, float* down_slot) {
    car_pack_absmax(st, 1, W, ldw, nullptr, b, N, K, {nullptr, p_slot, down_slot});
}
template <bool HI_ONLY = false>
void pack16(hipStream_t st, int blocks, const float* W, int ldw, const float* b, int N, int K, int n_tiles, int ksteps, int chained, int kbase,
            float* p_slot, _Float16* out) {
    car_pack_rows16(st, blocks, W, ldw, b, N, K, n_tiles, ksteps, chained, kbase, {nullptr, p_slot, nullptr}, out, HI_ONLY);
}
void pack32(hipStream_t st, int blocks, const float* W, int ldw, int chunks, int kgs, int chained, float* p_slot, _Float16* out) {
    car_pack_tiles32(st, blocks, W, ldw, nullptr, kD, 16 * kgs * chunks, 4, chunks, kgs, chained, {nullptr, p_slot, nullptr}, out);
}
int copy_bias(float* dst, const float* src, int n, hipStream_t st, const char* who) {
    if (hipMemcpyAsync(dst, src, sizeof(float) * n, hipMemcpyDeviceToDevice, st) != hipSuccess) { car_set_error("%s: bias copy failed", who); return CAR_E_LAUNCH; }
    return CAR_OK;
}

// Packs the six layers of the fused per-sample kernel (csrc/car_fused.hip) into its operand order: fp16 hi/lo tiles, every layer
// times its own power of two (chosen from its largest weight; 1/p goes into the bias table).
// HI_ONLY: the compact blob of the fp16 precision (pack16_kernel<true>), same bias table and point table.
template <bool HI_ONLY>
int fused_pack(const car_weights* w, float* blob_f, float* bias, float* wpt, void* stream) {
    CAR_REQUIRE(w && blob_f && bias && wpt, "car_fused_pack: null pointer");
    CAR_REQUIRE(w->query_encode_latent_w && w->query_encode_latent_b && w->query_encode_latent_2_w && w->query_encode_latent_2_b &&
                w->key_map_w && w->key_map_b && w->key_map_2_w && w->key_map_2_b && w->query_embed_w && w->query_embed_b &&
                w->query_embed_2_w && w->query_embed_2_b, "car_fused_pack: a weight pointer of the fused layers is null");
    hipStream_t st = (hipStream_t)stream;
    CAR_TRY(zero_table(bias, kBiasFloats + kBiasScratch, st, "car_fused_pack"));
    _Float16* blob = reinterpret_cast<_Float16*>(blob_f);
    float* fdown = bias + kBiasScale;
    float* pscale = bias + kBiasScale + 8;                           // pack-time scratch: 2^shift per layer
    auto pack = [&](const float* W, int ldw, const float* b, int N, int K, int n_tiles, int ksteps, int mode, int kbase, int layer, int tile_off) {
        pack16<HI_ONLY>(st, 256, W, ldw, b, N, K, n_tiles, ksteps, mode, kbase, pscale + layer,
                        blob + (size_t)tile_off * (HI_ONLY ? kTileHi : kTile16) * 2);
    };
    // the closing pair key_map_2 / query_embed_2 folded into one layer (car_fused_layout.h): M in fp32 behind the bias table, v, u, c inside it
    float* Mf = bias + kBiasFloats;
    hipLaunchKernelGGL(bilinear_fold_kernel, dim3(kD), dim3(kD), 0, st, w->key_map_2_w, w->key_map_2_b, w->query_embed_2_w, w->query_embed_2_b, kD, Mf,
                       bias + kBiasV, bias + kBiasU, bias + kBiasConst);
    layer_scale(st, w->query_encode_latent_2_w, kC, kE, kC, nullptr, pscale + kLayerW2, fdown + kLayerW2);
    layer_scale(st, w->query_embed_w, 16, kD, 16, w->query_embed_b, pscale + kLayerQ1, fdown + kLayerQ1);
    layer_scale(st, Mf, kD, kD, kD, nullptr, pscale + kLayerM, fdown + kLayerM);
    layer_scale(st, w->key_map_w, kC, kD, kC, nullptr, pscale + kLayerK1, fdown + kLayerK1);
    pack(w->query_encode_latent_2_w, kC, nullptr, kE, kC, kTE, kKS, 0, 0, kLayerW2, kOffW2);
    pack(w->query_embed_w, 16, w->query_embed_b, kD, 16, kTD, 1, 0, 0, kLayerQ1, kOffQ1);
    pack(Mf, kD, nullptr, kD, kD, kTD, 4, 1, 0, kLayerM, kOffM);
    pack(w->key_map_w, kC, nullptr, kD, kC, kTD, 9, 1, 0, kLayerK1, kOffK1);
    pack(w->key_map_w, kC, nullptr, kD, kC, kTD, 9, 1, kE, kLayerK1, kOffK1 + 9 * kTD);
    hipLaunchKernelGGL(wpt_kernel, dim3(1), dim3(kC), 0, st, w->query_encode_latent_w, w->query_encode_latent_b, wpt, fdown + 5);
    CAR_CHECK_LAUNCH("car_fused_pack");
    CAR_TRY(copy_bias(bias + kBiasE, w->query_encode_latent_2_b, kE, st, "car_fused_pack"));
    return copy_bias(bias + kBiasK1, w->key_map_b, kD, st, "car_fused_pack");
}

}  // namespace

extern "C" int car_fused_pack(const car_weights* w, float* blob_f, float* bias, float* wpt, void* stream) {
    return fused_pack<false>(w, blob_f, bias, wpt, stream);
}
int car_fused_pack_hi(const car_weights* w, float* blob16, float* bias, float* wpt, void* stream) {
    return fused_pack<true>(w, blob16, bias, wpt, stream);
}

// The first two point-MLP layers alone, for car_fused_rows (the three-view exchange): W2 in the fused kernel's operand tiles with its power
// of two, b2 and the scales in the bias table, the [C][4] point / bias table of the first layer with its largest row sum.  Same formats
// as car_fused_pack; the other layers' regions of blob / bias stay zero.
extern "C" int car_fused_pack_rows(const float* w1, const float* b1, const float* w2, const float* b2, float* blob_f, float* bias, float* wpt, void* stream) {
    CAR_REQUIRE(w1 && b1 && w2 && b2 && blob_f && bias && wpt, "car_fused_pack_rows: null pointer");
    hipStream_t st = (hipStream_t)stream;
    CAR_TRY(zero_table(bias, kBiasFloats, st, "car_fused_pack_rows"));
    _Float16* blob = reinterpret_cast<_Float16*>(blob_f);
    float* fdown = bias + kBiasScale;
    float* pscale = bias + kBiasScale + 8;
    layer_scale(st, w2, kC, kE, kC, nullptr, pscale + kLayerW2, fdown + kLayerW2);
    pack16(st, 256, w2, kC, nullptr, kE, kC, kTE, kKS, 0, 0, pscale + kLayerW2, blob + (size_t)kOffW2 * kTile16 * 2);
    hipLaunchKernelGGL(wpt_kernel, dim3(1), dim3(kC), 0, st, w1, b1, wpt, fdown + 5);
    CAR_CHECK_LAUNCH("car_fused_pack_rows");
    return copy_bias(bias + kBiasE, b2, kE, st, "car_fused_pack_rows");
}

// Packs key_map_2, query_embed and query_embed_2 for car_key_query_logits (csrc/car_linear16.hip, the stage route's key / query chain): the
// fused kernel's operand formats — K2 and Q2 chained over the accumulator order of the layer before, Q1 standard with its bias folded in at
// k = 16 — in the order the kernel streams them: K2 (32 tiles) | Q1 (8) | Q2 (32).  bias: bk2 [128] | bq2 [128] | 2^-shift of K2, Q1, Q2.
extern "C" int car_kq_pack(const float* k2w, const float* k2b, const float* q1w, const float* q1b, const float* q2w, const float* q2b, float* tail,
                           float* bias, void* stream) {
    CAR_REQUIRE(k2w && k2b && q1w && q1b && q2w && q2b && tail && bias, "car_kq_pack: null pointer");
    hipStream_t st = (hipStream_t)stream;
    CAR_TRY(zero_table(bias, car_kq_bias_floats(), st, "car_kq_pack"));
    float* down = bias + 2 * kD;                                     // [0..2] 2^-shift of K2, Q1, Q2; [8..10] their 2^shift (pack-time scratch)
    _Float16* blob = reinterpret_cast<_Float16*>(tail);
    layer_scale(st, k2w, kD, kD, kD, nullptr, down + 8, down + 0);
    layer_scale(st, q1w, 16, kD, 16, q1b, down + 9, down + 1);
    layer_scale(st, q2w, kD, kD, kD, nullptr, down + 10, down + 2);
    pack16(st, 64, k2w, kD, nullptr, kD, kD, kTD, 4, 1, 0, down + 8, blob);
    pack16(st, 16, q1w, 16, q1b, kD, 16, kTD, 1, 0, 0, down + 9, blob + (size_t)32 * kTile16 * 2);
    pack16(st, 64, q2w, kD, nullptr, kD, kD, kTD, 4, 1, 0, down + 10, blob + (size_t)40 * kTile16 * 2);
    CAR_CHECK_LAUNCH("car_kq_pack");
    CAR_TRY(copy_bias(bias, k2b, kD, st, "car_kq_pack"));
    return copy_bias(bias + kD, q2b, kD, st, "car_kq_pack");
}

// Packs query_repeat_embed (its local_coords half, columns 128..143 of the (128, 144) matrix `wr1`) and query_repeat_embed_2 for
// csrc/car_round2.hip; same conventions as car_fused_pack.
extern "C" int car_round2_pack(const float* wr1, const float* br1, const float* wr2, const float* br2, float* wpacked, float* bias, void* stream) {
    CAR_REQUIRE(wr1 && br1 && wr2 && br2 && wpacked && bias, "car_round2_pack: null pointer");
    hipStream_t st = (hipStream_t)stream;
    CAR_TRY(zero_table(bias, car_round2_bias_floats(), st, "car_round2_pack"));
    float* down = bias + 2 * kD;                                     // [0] Wr1g, [1] Wr2; [2], [3]: their 2^shift (pack-time scratch)
    _Float16* out = reinterpret_cast<_Float16*>(wpacked);
    layer_scale(st, wr1 + kD, kD + 16, kD, 16, nullptr, down + 2, down + 0);
    layer_scale(st, wr2, kD, kD, kD, nullptr, down + 3, down + 1);
    pack32(st, 128, wr2, kD, 4, 2, 1, down + 3, out);
    pack32(st, 16, wr1 + kD, kD + 16, 1, 1, 0, down + 2, out + 4 * 4 * 2 * 2 * 64 * 8);
    CAR_CHECK_LAUNCH("car_round2_pack");
    CAR_TRY(copy_bias(bias, br1, kD, st, "car_round2_pack"));
    return copy_bias(bias + kD, br2, kD, st, "car_round2_pack");
}

// For car_round2_logits_from_g (csrc/car_round2.hip round2g_kernel, car_round2_logit.h): query_repeat_embed_2 and query_embed_2 folded into the one layer of the
// bilinear form <q2, qry> = y^T (M x + v) + u^T x + c (M = Wr2^T Wq2, v = Wr2^T bq2, u = Wq2^T br2, c = <br2, bq2>; bilinear_fold_kernel) and the
// two 16 -> 128 layers that make y and x from g.  wpacked [car_round2q_packed_floats()] = M (chained K order) | Wr1[:, 128:] | Wq1, each laid out
// as car_round2_pack lays out its own; bias [car_round2q_bias_floats()] = br1 | v | bq1 | u | 2^-shift of Wr1g, M, Wq1 | c | scratch (their
// 2^shift, then M in fp32).
extern "C" int car_round2q_pack(const float* wr1, const float* br1, const float* wr2, const float* br2, const float* wq1, const float* bq1,
                                const float* wq2, const float* bq2, float* wpacked, float* bias, void* stream) {
    CAR_REQUIRE(wr1 && br1 && wr2 && br2 && wq1 && bq1 && wq2 && bq2 && wpacked && bias, "car_round2q_pack: null pointer");
    hipStream_t st = (hipStream_t)stream;
    CAR_TRY(zero_table(bias, car_round2q_bias_floats(), st, "car_round2q_pack"));
    float* down = bias + 4 * kD;                                     // [0] Wr1g, [1] M, [2] Wq1, [3] c; [4..6]: the layers' 2^shift (pack-time scratch)
    float* Mf = bias + 4 * kD + 8;                                   // scratch: M in fp32
    _Float16* out = reinterpret_cast<_Float16*>(wpacked);
    const size_t first = (size_t)4 * 4 * 2 * 2 * 64 * 8, small = (size_t)4 * 2 * 64 * 8;                  // halves: the 128 x 128 layer, a 128 x 16 layer
    hipLaunchKernelGGL(bilinear_fold_kernel, dim3(kD), dim3(kD), 0, st, wr2, br2, wq2, bq2, kD, Mf, bias + kD, bias + 3 * kD, down + 3);
    layer_scale(st, wr1 + kD, kD + 16, kD, 16, nullptr, down + 4, down + 0);
    layer_scale(st, Mf, kD, kD, kD, nullptr, down + 5, down + 1);
    layer_scale(st, wq1, 16, kD, 16, nullptr, down + 6, down + 2);
    pack32(st, 128, Mf, kD, 4, 2, 1, down + 5, out);
    pack32(st, 16, wr1 + kD, kD + 16, 1, 1, 0, down + 4, out + first);
    pack32(st, 16, wq1, 16, 1, 1, 0, down + 6, out + first + small);
    CAR_CHECK_LAUNCH("car_round2q_pack");
    CAR_TRY(copy_bias(bias, br1, kD, st, "car_round2q_pack"));
    return copy_bias(bias + 2 * kD, bq1, kD, st, "car_round2q_pack");
}

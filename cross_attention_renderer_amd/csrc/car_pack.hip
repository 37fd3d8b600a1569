// car_pack.hip — the device-side weight packers of the C ABI (include/car_hip.h: car_fused_pack, car_fused_pack_rows, car_kq_pack,
// car_round2_pack, car_round2q_pack): small re-layout / reduction kernels that put a layer into the operand order of the kernel that
// consumes it, every layer times its own power of two.  Asynchronous, device side only.  car_plan_build / car_plan_f16_build
// (car_render.hip) and the stage route (engine.py) both pack through these entries.
#include "car_common.h"

namespace {

#include "car_fused_layout.h"

constexpr int kTile16 = kTile;                     // floats per (K step, 16-channel tile) of the fused kernel's blob

// power of two p with m p in [2^13, 2^14) (the window of the split-fp16 operands, car_fused_mma.h)
__device__ __forceinline__ float pow2_for(float m) {
    int e = (int)((__float_as_uint(m) >> 23) & 0xffu);
    e = e < 97 ? 97 : (e > 230 ? 230 : e);          // p in [2^-90, 2^43]: an all-zero vector or matrix must not push p_x * p_W past fp32
    return __uint_as_float((unsigned)(267 - e) << 23);
}
__device__ __forceinline__ float block_max(float v, float* red) {
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float m = 0.0f;
    for (int w = 0; w < (int)(blockDim.x + 63) / 64; ++w) m = fmaxf(m, red[w]);
    __syncthreads();
    return m;
}

// ---- re-layout kernels ---------------------------------------------------------------------------------------------
// Scale of a packed layer: p = 2^shift from the largest |weight| (and |bias| where the bias is folded in as a column);
// p goes to p_slot (read by the pack kernels), 1/p to down_slot (read by the consuming kernel).  One workgroup.
__global__ void layer_scale_kernel(const float* __restrict__ W, int ldw, int N, int K, const float* __restrict__ bias,
                                   float* __restrict__ p_slot, float* __restrict__ down_slot) {
    __shared__ float red[16];
    float m = 0.0f;
    for (long idx = threadIdx.x; idx < (long)N * K; idx += blockDim.x) m = fmaxf(m, fabsf(W[(idx / K) * ldw + idx % K]));
    if (bias) for (int n = threadIdx.x; n < N; n += blockDim.x) m = fmaxf(m, fabsf(bias[n]));
    m = block_max(m, red);
    if (threadIdx.x == 0) {
        const float p = pow2_for(fmaxf(m, 1e-30f));
        p_slot[0] = p;
        down_slot[0] = 1.0f / p;
    }
}
// A-operand tiles of v_mfma_f32_16x16x32_f16 with fp16 hi/lo halves: per (K step, tile) [hi|lo][lane][8 halves]; lane l carries
// output 16 t + l % 16 and k = 32 ks + 8 (l >> 4) + e (mode 0) or the accumulator order base + 16 (2 ks + e / 4) + 4 (l >> 4) + e % 4
// (mode 1); k == K selects the bias, k > K a zero.  Values are multiplied by the layer's power of two *p_slot.
// HI_ONLY: the compact tiles of the fp16 precision (car_plan_f16_build): the same values and order as the full instance's hi halves
// (rounded to nearest after the layer's power of two), without the lo halves: per (K step, tile) [lane][8 halves], 1 KB.
template <bool HI_ONLY>
__global__ void pack16_kernel(const float* __restrict__ W, int ldw, const float* __restrict__ bias, int N, int K, int n_tiles,
                              int ksteps, int mode, int base, const float* __restrict__ p_slot, _Float16* __restrict__ out) {
    const long total = (long)ksteps * n_tiles * 512;
    const float p = p_slot[0];
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int e = (int)(idx & 7), lane = (int)((idx >> 3) & 63);
        const long tile = idx >> 9;
        const int t = (int)(tile % n_tiles), ks = (int)(tile / n_tiles);
        const int n = 16 * t + (lane & 15), q = lane >> 4;
        const int k = mode == 0 ? 32 * ks + 8 * q + e : base + 16 * (2 * ks + e / 4) + 4 * q + e % 4;
        float w = 0.0f;
        if (n < N) {
            if (k < K) w = W[(long)n * ldw + k] * p;
            else if (k == K && bias) w = bias[n] * p;
        }
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
// A-operand tiles of v_mfma_f32_32x32x16_f16 for car_round2.hip: [chunk][tile 4][K group kgs][hi|lo][lane][8 halves], output
// 32 t + l % 32; chained = 1: k = 32 c + (e & 3) + 8 (2 kg + (e >> 2)) + 4 (l >> 5) (the accumulator order of the layer before),
// chained = 0: k = 16 c + 8 (l >> 5) + e with one K group per chunk.
__global__ void pack32_kernel(const float* __restrict__ W, int ldw, int chunks, int kgs, int chained, const float* __restrict__ p_slot,
                              _Float16* __restrict__ out) {
    const int total = chunks * 4 * kgs * 2 * 64 * 8;
    const float p = p_slot[0];
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
        const int e = idx & 7, lane = (idx >> 3) & 63, hl = (idx >> 9) & 1;
        int rest = idx >> 10;
        const int kg = rest % kgs; rest /= kgs;
        const int t = rest & 3, c = rest >> 2;
        const int n = 32 * t + (lane & 31);
        const int k = chained ? 32 * c + (e & 3) + 8 * (2 * kg + (e >> 2)) + 4 * (lane >> 5) : 16 * c + 8 * (lane >> 5) + e;
        const float w = W[n * ldw + k] * p;
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

// ---- what the five packers share: zero the bias table, one layer_scale_kernel per layer, the pack launches, CAR_CHECK_LAUNCH, then
// device-to-device bias copies -------------------------------------------------------------------------------------------------------
int zero_table(float* bias, size_t n, hipStream_t st, const char* who) {
    if (hipMemsetAsync(bias, 0, sizeof(float) * n, st) != hipSuccess) { car_set_error("%s: memset failed", who); return CAR_E_LAUNCH; }
    (void)hipGetLastError();
    return CAR_OK;
}
void layer_scale(hipStream_t st, const float* W, int ldw, int N, int K, const float* b, float* p_slot, float* down_slot) {
    hipLaunchKernelGGL(layer_scale_kernel, dim3(1), dim3(1024), 0, st, W, ldw, N, K, b, p_slot, down_slot);
}
template <bool HI_ONLY = false>
void pack16(hipStream_t st, int blocks, const float* W, int ldw, const float* b, int N, int K, int n_tiles, int ksteps, int mode, int kbase,
            const float* p_slot, _Float16* out) {
    hipLaunchKernelGGL(pack16_kernel<HI_ONLY>, dim3(blocks), dim3(256), 0, st, W, ldw, b, N, K, n_tiles, ksteps, mode, kbase, p_slot, out);
}
void pack32(hipStream_t st, int blocks, const float* W, int ldw, int chunks, int kgs, int chained, const float* p_slot, _Float16* out) {
    hipLaunchKernelGGL(pack32_kernel, dim3(blocks), dim3(256), 0, st, W, ldw, chunks, kgs, chained, p_slot, out);
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

// For car_round2_logits_from_g (csrc/car_round2.hip, G instance): query_repeat_embed_2 and query_embed_2 folded into the one layer of the
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

// car_round2.hip — per-sample part of the second attention round in one kernel (reference
// models.py:548-556):
//     ug    = Wr1[:,128:] g + br1                  g  = the sample's 16-channel geometric query (from the fused kernel)
//     q2    = Wr2 relu(ug + uh[ray]) + br2         uh = Wr1[:,:128] encode_latent(z1)   (per ray, car_ray_mid)
//     logit = <q2, qry> / 16
// Neither ug nor q2 exists in memory: ug is produced in the MFMA accumulators from the 64-byte g row (weights as A operand,
// samples as B operand), its registers — plus uh, loaded in the same accumulator layout — are the B operand of the second layer
// (the accumulator's channel permutation is baked into the packed Wr2, "chained" K order), and q2 is dotted with the sample's
// qry row straight out of the accumulators (round2_kernel) — or qry is never made: round2g_kernel evaluates the same logit as a
// bilinear form of g and uh alone (car_round2_layout.h, car_round2_logit.h).  f16 matrix pipe with fp16 hi/lo operand splits (three
// products per term: car_mma32.h); the activations of the second layer are scaled per sample by a power of two so that the split stays inside
// fp16's normal range whatever their magnitude.  Both layers (4 KB + 64 KB packed) sit in LDS, loaded once per workgroup
// (8 waves): no weight stream and no barrier in the main loop.  HBM-bound on the qry rows (512 B per sample) + g (64 B): they
// are loaded coalesced (8 lanes x 16 B per row = one 128-byte line) and turned through a wave-private LDS tile.
#include "car_common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
#include "car_mma32.h"
#include "car_round2_layout.h"
#include "car_round2_logit.h"

// both kernels: the packs and the bias table into LDS, once per workgroup
__device__ __forceinline__ void load_packs(float* lds, const float* wpacked, int n_packed, const float* bias, int n_bias, int tid) {
    for (int k = tid; k < n_packed / 4; k += 512)
        *reinterpret_cast<float4*>(lds + 4 * k) = *reinterpret_cast<const float4*>(wpacked + 4 * k);
    for (int k = tid; k < n_bias; k += 512) lds[n_packed + k] = bias[k];
    __syncthreads();
}
// the row of uh that sample row `srow` reads: uh is per (scene, ray), shared by the views
__device__ __forceinline__ const float* uh_row(const float* uh, long srow, int V, int R, int P) {
    const long nr = srow / P;                                      // (scene-view n, ray r)
    return uh + (((nr / R) / V) * R + nr % R) * kD;
}

// acc += W x for the 128 x 128 layer at lds (chained K order: K step (c, kg) takes registers 8 kg .. 8 kg + 7 of x's tile c), x times xp
__device__ __forceinline__ void layer_128(f32x16 (&acc)[kNT], const float* lds, const f32x16 (&x)[kNT], float xp, int lane) {
#pragma unroll
    for (int c = 0; c < kChunks; ++c) {
        float x8[2][8];
#pragma unroll
        for (int kg = 0; kg < 2; ++kg)
#pragma unroll
            for (int e = 0; e < 8; ++e) x8[kg][e] = x[c][8 * kg + e];
        mma_chunk<kNT>(acc, lds + c * kNT * kTile + 4 * lane, x8, xp);
    }
}

// The stored-query form: qry rows are read (the staged routes, which keep them)
__global__ void __launch_bounds__(512) round2_kernel(const float* __restrict__ g, const float* __restrict__ uh,
                                                     const float* __restrict__ qry, const float* __restrict__ wpacked,
                                                     const float* __restrict__ bias, int V, int R, int P, long S,
                                                     float* __restrict__ logit) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s = lane & 31, h = lane >> 5;
    const int qd = lane & 7, r8 = lane >> 3;                        // coalesced side: row r8 + 8 it, channel quad qd of a 32-wide chunk
    load_packs(lds, wpacked, kLdsBias, bias, 2 * kD + 4, tid);
    const float* lb = lds + kLdsBias;
    const float down1 = lb[2 * kD], down2 = lb[2 * kD + 1];
    float* stage = lds + kLdsStage + wave * 32 * kStageLd;

    for (long row0 = ((long)blockIdx.x * kWaves + wave) * 32; row0 < S; row0 += (long)gridDim.x * kWaves * 32) {
        // the HBM stream first: qry rows, coalesced (every load instruction covers 8 whole 128-byte lines)
        float4 qs[kChunks][4];
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const long row = row0 + r8 + 8 * it < S ? row0 + r8 + 8 * it : S - 1;
#pragma unroll
            for (int c = 0; c < kChunks; ++c) {                      // read once: non-temporal
                const f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(qry + row * kD + 32 * c + 4 * qd));
                qs[c][it] = make_float4(v[0], v[1], v[2], v[3]);
            }
        }
        // this lane's sample: its g half (B operand of the first layer) and the row of uh its ray owns
        const long srow = row0 + s < S ? row0 + s : S - 1;
        const float* uhrow = uh_row(uh, srow, V, R, P);
        half8 ghi, glo;
        float gp, ginv;
        split_g(*reinterpret_cast<const float4*>(g + srow * 16 + 8 * h), *reinterpret_cast<const float4*>(g + srow * 16 + 8 * h + 4), ghi, glo, gp, ginv);
        // ug = Wr1g g + br1 (the bias in the product's units, gp / down1); y = relu(ug + uh) in place
        f32x16 ug[kNT];
        set_bias<kNT>(ug, lb, gp / down1, h);
#pragma unroll
        for (int t = 0; t < kNT; ++t) mma_k16(ug[t], lds + kLdsW1, t, lane, ghi, glo);
        const float undo1 = down1 * ginv;
        float xm = 0.0f;
#pragma unroll
        for (int t = 0; t < kNT; ++t)
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
                const float4 u = row4(uhrow, t, gq, h);
                const float uu[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float x = fmaxf(fmaf(ug[t][4 * gq + r], undo1, uu[r]), 0.0f);
                    ug[t][4 * gq + r] = x;
                    xm = fmaxf(xm, x);
                }
            }
        xm = fmaxf(xm, __shfl_xor(xm, 32, 64));
        float xp, xinv;
        pow2_scale(fmaxf(xm, 1e-30f), xp, xinv);
        // q2 = Wr2 y + br2, times xp / down2: y's registers are the B operands (K step (c, kg) takes registers 8 kg .. 8 kg + 7 of tile c)
        f32x16 acc[kNT];
        set_bias<kNT>(acc, lb + kD, xp / down2, h);
        layer_128(acc, lds, ug, xp, lane);
        // <q2, qry>: lane (s, h) holds channels mma32_channel(t, 4 g', h) + (0..3) of its sample in acc[t][4g'..4g'+3]; qry comes through
        // the wave's tile, 32 channels at a time
        float dot = 0.0f;
#pragma unroll
        for (int t = 0; t < kNT; ++t) {
#pragma unroll
            for (int it = 0; it < 4; ++it) *reinterpret_cast<float4*>(stage + (r8 + 8 * it) * kStageLd + 4 * qd) = qs[t][it];
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
                const float4 qv = row4(stage + s * kStageLd, 0, gq, h);
                dot = fmaf(acc[t][4 * gq + 0], qv.x, dot); dot = fmaf(acc[t][4 * gq + 1], qv.y, dot);
                dot = fmaf(acc[t][4 * gq + 2], qv.z, dot); dot = fmaf(acc[t][4 * gq + 3], qv.w, dot);
            }
        }
        dot += __shfl_xor(dot, 32, 64);
        dot *= down2 * xinv;
        if (h == 0 && row0 + s < S) logit[row0 + s] = dot / 16.0f;
    }
}

// The folded form, from g and uh alone (car_round2_layout.h): x = relu(Wq1 g + bq1); <q2, qry> = y^T (M x + v) + u^T x + c.  The products,
// the sums and their order are sample_logit's (car_round2_logit.h: bit for bit the same logits, tests/test_round2_attend_hip.py), the
// live ranges are not: y and x are whole accumulator sets here and the 128 x 128 layer reads its A operands one step ahead
// (mma_chunk).  With this kernel's two waves per SIMD sample_logit itself measured 1.2 ms against 1.0 (profiles/second_round_pieces.md).
// The biases of all three layers are added AFTER the products, in true units (one fma each, where the product's scale is undone
// anyway), so the accumulators start from the matrix instruction's zero.  br1 + uh is read per sample: a tile of 32 samples may
// straddle rays here (any P)
__global__ void __launch_bounds__(512) round2g_kernel(const float* __restrict__ g, const float* __restrict__ uh, const float* __restrict__,
                                                      const float* __restrict__ wpacked, const float* __restrict__ bias, int V, int R, int P,
                                                      long S, float* __restrict__ logit) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s = lane & 31, h = lane >> 5;
    load_packs(lds, wpacked, kLdsBiasG, bias, kBiasFloatsG, tid);
    const float* lb = lds + kLdsBiasG;
    const float down1 = lb[4 * kD], down2 = lb[4 * kD + 1], downq = lb[4 * kD + 2];
    for (long row0 = ((long)blockIdx.x * kWaves + wave) * 32; row0 < S; row0 += (long)gridDim.x * kWaves * 32) {
        const long srow = row0 + s < S ? row0 + s : S - 1;
        const float* uhrow = uh_row(uh, srow, V, R, P);
        half8 ghi, glo;
        float gp, ginv;
        split_g(*reinterpret_cast<const float4*>(g + srow * 16 + 8 * h), *reinterpret_cast<const float4*>(g + srow * 16 + 8 * h + 4), ghi, glo, gp, ginv);
        // y = relu(Wr1g g + br1 + uh)
        f32x16 y[kNT];
        zero<kNT>(y);
#pragma unroll
        for (int t = 0; t < kNT; ++t) mma_k16(y[t], lds + kLdsW1, t, lane, ghi, glo);
        const float undo1 = down1 * ginv;
#pragma unroll
        for (int t = 0; t < kNT; ++t)
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
                const float4 u = row4(uhrow, t, gq, h), b = row4(lb, t, gq, h);
                const float uu[4] = {u.x + b.x, u.y + b.y, u.z + b.z, u.w + b.w};
#pragma unroll
                for (int r = 0; r < 4; ++r) y[t][4 * gq + r] = fmaxf(fmaf(y[t][4 * gq + r], undo1, uu[r]), 0.0f);
            }
        // x = relu(Wq1 g + bq1), its largest entry and u^T x
        f32x16 xq[kNT];
        zero<kNT>(xq);
#pragma unroll
        for (int t = 0; t < kNT; ++t) mma_k16(xq[t], lds + kLdsWq1, t, lane, ghi, glo);
        const float undoq = downq * ginv;
        float xqm = 0.0f, dot_u = 0.0f;
#pragma unroll
        for (int t = 0; t < kNT; ++t)
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
                const float4 u = row4(lb + 3 * kD, t, gq, h), b = row4(lb + 2 * kD, t, gq, h);
                const float uu[4] = {u.x, u.y, u.z, u.w}, bb[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float x = fmaxf(fmaf(xq[t][4 * gq + r], undoq, bb[r]), 0.0f);
                    xq[t][4 * gq + r] = x;
                    xqm = fmaxf(xqm, x);
                    dot_u = fmaf(uu[r], x, dot_u);
                }
            }
        xqm = fmaxf(xqm, __shfl_xor(xqm, 32, 64));
        float xp, xinv;
        pow2_scale(fmaxf(xqm, 1e-30f), xp, xinv);
        // M x, then y^T (M x) in the product's units and y^T v in true ones
        f32x16 acc[kNT];
        zero<kNT>(acc);
        layer_128(acc, lds, xq, xp, lane);
        float dot = 0.0f, dot_v = 0.0f;
#pragma unroll
        for (int t = 0; t < kNT; ++t)
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
                const float4 v4 = row4(lb + kD, t, gq, h);
                const float vv[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    dot = fmaf(y[t][4 * gq + r], acc[t][4 * gq + r], dot);
                    dot_v = fmaf(y[t][4 * gq + r], vv[r], dot_v);
                }
            }
        dot = fmaf(dot, down2 * xinv, dot_u + dot_v);
        dot += __shfl_xor(dot, 32, 64);
        dot += lb[4 * kD + 3];
        if (h == 0 && row0 + s < S) logit[row0 + s] = dot / 16.0f;
    }
}

}  // namespace

extern "C" size_t car_round2_packed_floats(void) { return (size_t)kLdsBias; }
extern "C" size_t car_round2_bias_floats(void) { return (size_t)(2 * kD + 4); }

extern "C" size_t car_round2q_packed_floats(void) { return (size_t)kLdsBiasG; }
extern "C" size_t car_round2q_bias_floats(void) { return (size_t)(kBiasFloatsG + kScratchG); }      // the table + car_round2q_pack's scratch

static int launch_round2(bool qg, const float* g, const float* uh, const float* qry, const float* wpacked, const float* bias,
                         int b, int V, int R, int P, float* logit, void* stream, const char* who) {
    CAR_REQUIRE(g && uh && (qg || qry) && wpacked && bias && logit, "%s: null pointer", who);
    CAR_REQUIRE(b > 0 && V > 0 && R > 0 && P > 0, "%s: bad sizes", who);
    const long S = (long)b * V * R * P;
    void (*kern)(const float*, const float*, const float*, const float*, const float*, int, int, int, long, float*) =
        qg ? round2g_kernel : round2_kernel;
    const size_t lds_bytes = qg ? kLdsBytesG : kLdsBytes;
    const long groups = (S + 255) / 256;
    const unsigned blocks = (unsigned)(groups < 1024 ? groups : 1024);       // one 8-wave workgroup per CU x 256 CUs x 4: grid-stride
    CAR_LAUNCH_LDS(who, kern, dim3(blocks), dim3(512), lds_bytes, (hipStream_t)stream, g, uh, qry, wpacked, bias, V, R, P, S, logit);
    return CAR_OK;
}

extern "C" int car_round2_logits(const float* g, const float* uh, const float* qry, const float* wpacked, const float* bias,
                                 int b, int V, int R, int P, float* logit, void* stream) {
    return launch_round2(false, g, uh, qry, wpacked, bias, b, V, R, P, logit, stream, "car_round2_logits");
}

// The same logits without the qry rows: the bilinear form of y and x = relu(query_embed(g)) described above.  wpacked / bias: car_round2q_pack.
extern "C" int car_round2_logits_from_g(const float* g, const float* uh, const float* wpacked, const float* bias, int b, int V, int R, int P,
                                        float* logit, void* stream) {
    return launch_round2(true, g, uh, nullptr, wpacked, bias, b, V, R, P, logit, stream, "car_round2_logits_from_g");
}

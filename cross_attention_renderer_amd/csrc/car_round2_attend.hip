// car_round2_attend.hip — the whole second attention round in one kernel: the folded bilinear logits of car_round2.hip's round2g_kernel
// (car_round2_logit.h; matrix pipe only) computed UNDER the value stream of car_attention.hip's sample-row instance (HBM only).  The two ran one after the other
// on an otherwise idle chip, with the logits making a round trip through memory in between.
//
// One persistent 12-wave workgroup per compute unit, grid-stride over batches of two rays:
//   waves 0-7  "stream": four waves per ray with attend_kernel<false, 9>'s thread mapping (16 groups of 16 lanes, a group reads a whole
//              576-wide row as nine non-temporal float4 loads per lane), softmax and reduction order: w_out and z_out come out bit for bit
//              as car_attend writes them.  Two rows per lane are in flight at any time, also across the batch boundary.
//   waves 8-11 "matrix": one per SIMD; they compute the NEXT batch's logits into an LDS double buffer while the current one streams.
//              A sample's logit is car_round2_logit.h's sample_logit: round2g_kernel's products and sums in its order (bit for bit its
//              logits), with short live ranges, because the kernel must share its register budget with the stream waves.
// One __syncthreads() closes each batch.  A stream wave needs no other barrier: it computes the ray's softmax for itself (each of the four
// waves evaluates all four waves' partial sums, in the two-kernel form's order), and the four waves' partial value sums meet in an LDS
// double buffer that is folded after the barrier.  The packs of car_round2q_pack (82 KB) sit in LDS for the workgroup's life.
#include "car_common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
#include "car_mma32.h"
#include "car_round2_layout.h"
#include "car_round2_logit.h"

constexpr int kC = 576, kSeg = kC / 64;                             // the value rows: nine 64-channel segments
constexpr int kMaxSamples = CAR_MAX_VIEWS * 256;                    // car_attention.hip's limit on V * P
constexpr int kStreamWaves = 8, kMatrixWaves = 4, kThreads = 64 * (kStreamWaves + kMatrixWaves);
constexpr int kLdsLogit = kLdsBiasG + kBiasFloatsG;                 // [2 buffers][2 rays][kMaxSamples]
constexpr int kLdsWt = kLdsLogit + 2 * 2 * kMaxSamples;             // [2 rays][kMaxSamples]: the softmax weights
constexpr int kLdsZ = kLdsWt + 2 * kMaxSamples;                     // [2 buffers][2 rays][4 waves][576]: per-wave partial value sums
constexpr int kLdsUh = kLdsZ + 2 * 2 * 4 * kC;                      // [4 matrix waves][128]: br1 + the uh row of the wave's tile
constexpr int kLdsFloats = kLdsUh + kMatrixWaves * kD;
static_assert(kLdsZ % 4 == 0 && kLdsUh % 4 == 0 && kLdsFloats * sizeof(float) <= 160 * 1024, "LDS layout");

struct Args {
    const float *g, *uh, *wpacked, *bias, *val;
    int b, V, R, P;
    float *w_out, *z_out;
    int ld_z;
    float* logit_out;
};

__global__ void __launch_bounds__(kThreads) round2_attend_kernel(const Args a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int k = tid; k < kLdsBiasG / 4; k += kThreads)
        *reinterpret_cast<float4*>(lds + 4 * k) = *reinterpret_cast<const float4*>(a.wpacked + 4 * k);
    for (int k = tid; k < kBiasFloatsG; k += kThreads) lds[kLdsBiasG + k] = a.bias[k];

    const int V = a.V, R = a.R, P = a.P, S = V * P;
    const long BR = (long)a.b * R, nbatch = (BR + 1) / 2, rows = BR * S;
    const bool matrix = wave >= kStreamWaves;
    auto row_of = [&](int ray, int s) -> long {
        const long row = car_sample_row(ray / R, ray % R, s, V, R, P);
        CAR_BOUNDS_TRAP(ray >= 0 && ray < BR && s >= 0 && s < S && row >= 0 && row < rows);
        return row;
    };

    // ---- stream side: ray slot q of the batch, wave wl of its four, group grp of its sixteen
    const int q = (wave >> 2) & 1, wl = wave & 3;
    const int tl = wl * 64 + lane, sub = tl & 15, grp = tl >> 4;
    const int nit = S / 16;                                         // even: P % 32 == 0
    f32x4 bufA[kSeg], bufB[kSeg];
    // the rows of iteration `it` of batch `batch`; iterations past the batch's end are the first ones of the workgroup's next batch (past
    // the last batch and past the last ray the addresses are clamped to rows that exist: loaded, never used)
    auto issue = [&](f32x4 (&buf)[kSeg], long batch, int it) {
        if (it >= nit) { batch += gridDim.x; it -= nit; }
        if (batch >= nbatch) batch -= gridDim.x;
        const int ray = (int)(2 * batch + q < BR ? 2 * batch + q : BR - 1);
        const float* rowp = a.val + row_of(ray, 16 * it + grp) * kC + 4 * sub;
        CAR_BOUNDS_TRAP(rowp >= a.val && rowp + 64 * (kSeg - 1) + 4 <= a.val + rows * kC);
#pragma unroll
        for (int j = 0; j < kSeg; ++j) buf[j] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(rowp + 64 * j));   // read once
    };
    __syncthreads();

    // iteration k streams batch `cur` from logit buffer k & 1 while the matrix waves fill buffer (k + 1) & 1 for batch `nxt`; k = -1 is the
    // prologue (the first batch's logits, nothing to stream yet).  The two roles run the same iterations in loops of their own, each
    // with the batch's one barrier, so that neither carries the other's registers.
    if (matrix) {
        const int s = lane & 31, h = lane >> 5;
        const int tpr = S / 32;
        float* ub = lds + kLdsUh + (wave - kStreamWaves) * kD;
        for (int k = -1;; ++k) {
            const long cur = (long)blockIdx.x + (long)k * gridDim.x, nxt = cur + gridDim.x;
            if (k >= 0 && cur >= nbatch) break;
            if (nxt < nbatch) {
                const int ntile = (2 * nxt + 1 < BR ? 2 : 1) * tpr;
                float* lg = lds + kLdsLogit + ((k + 1) & 1) * 2 * kMaxSamples;
                for (int tile = wave - kStreamWaves; tile < ntile; tile += kMatrixWaves) {
                    const int slot = tile / tpr, si = 32 * (tile % tpr) + s;
                    const int ray = (int)(2 * nxt) + slot;
                    const long srow = row_of(ray, si);
                    // one trip to memory per tile: the g rows and the ray's uh row together; br1 + uh goes through the wave's LDS row
                    const float4 g0 = *reinterpret_cast<const float4*>(a.g + srow * 16 + 8 * h);
                    const float4 g1 = *reinterpret_cast<const float4*>(a.g + srow * 16 + 8 * h + 4);
                    __builtin_amdgcn_wave_barrier();                 // the previous tile's reads of `ub` are done
                    if (lane < 32) {
                        const float4 u = *reinterpret_cast<const float4*>(a.uh + (long)ray * kD + 4 * lane);
                        const float4 b1 = *reinterpret_cast<const float4*>(lds + kLdsBiasG + 4 * lane);
                        *reinterpret_cast<float4*>(ub + 4 * lane) = make_float4(u.x + b1.x, u.y + b1.y, u.z + b1.z, u.w + b1.w);
                    }
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                    // a tile of 32 samples lies inside one ray: P % 32 == 0
                    const float logit = sample_logit(lds, g0, g1, ub, lane, h);
                    if (h == 0) {
                        CAR_BOUNDS_TRAP(si < kMaxSamples);
                        lg[slot * kMaxSamples + si] = logit;
                        if (a.logit_out) a.logit_out[srow] = logit;
                    }
                }
            }
            __syncthreads();
        }
        return;
    }
    issue(bufA, blockIdx.x, 0);
    issue(bufB, blockIdx.x, 1);
    for (int k = -1;; ++k) {
        const long cur = (long)blockIdx.x + (long)k * gridDim.x;
        if (k >= 0 && cur >= nbatch) break;
        const bool on = k >= 0 && 2 * cur + q < BR;                  // the last batch may hold one ray
        const int ray = (int)(2 * cur) + q;
        if (on) {
            const float* lg = lds + kLdsLogit + ((k & 1) * 2 + q) * kMaxSamples;
            float* wt = lds + kLdsWt + q * kMaxSamples;
            // the softmax, by every wave for itself, in attend_kernel's order: thread tid' = 64 w + lane of its 256 sums the samples
            // tid' + 256 i, a wave folds its lanes, and the four waves' sums meet as (0 + 1) + (2 + 3)
            float m = -INFINITY;
            for (int s = lane; s < S; s += 64) m = fmaxf(m, lg[s]);
            m = wave_max(m);
            float tot[4];
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                float sacc = 0.0f;
                for (int s = 64 * w + lane; s < S; s += 256) sacc += expf(lg[s] - m);
                tot[w] = wave_sum(sacc);
            }
            const float sum = (tot[0] + tot[1]) + (tot[2] + tot[3]);
            for (int s0 = 0; s0 < S; s0 += 64) {
                const int s = s0 + lane;
                if (s < S) {
                    const float w = expf(lg[s] - m) / sum;
                    wt[s] = w;                                       // the ray's four waves write the same values
                    if (((s0 >> 6) & 3) == wl) a.w_out[row_of(ray, s)] = w;
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            // z = sum_s w_s val[s]: group grp takes the samples 16 it + grp
            float4 part[kSeg];
#pragma unroll
            for (int j = 0; j < kSeg; ++j) part[j] = make_float4(0.f, 0.f, 0.f, 0.f);
            auto consume = [&](const f32x4 (&buf)[kSeg], float w) {
#pragma unroll
                for (int j = 0; j < kSeg; ++j) {
                    part[j].x = fmaf(w, buf[j][0], part[j].x); part[j].y = fmaf(w, buf[j][1], part[j].y);
                    part[j].z = fmaf(w, buf[j][2], part[j].z); part[j].w = fmaf(w, buf[j][3], part[j].w);
                }
            };
            for (int it = 0; it < nit; it += 2) {
                const float w0 = wt[16 * it + grp], w1 = wt[16 * it + 16 + grp];
                // a buffer is requested again as soon as it is consumed, while the other one is still in flight (kept in this order)
                consume(bufA, w0);
                __builtin_amdgcn_sched_barrier(0);
                issue(bufA, cur, it + 2);
                __builtin_amdgcn_sched_barrier(0);
                consume(bufB, w1);
                __builtin_amdgcn_sched_barrier(0);
                issue(bufB, cur, it + 3);
                __builtin_amdgcn_sched_barrier(0);
            }
            // the four groups of a wave hold different samples of the same channels: fold them; the four waves meet after the barrier
            float* sz = lds + kLdsZ + (((k & 1) * 2 + q) * 4 + wl) * kC;
#pragma unroll
            for (int j = 0; j < kSeg; ++j) {
                float4 v4 = part[j];
                v4.x += __shfl_xor(v4.x, 16, 64); v4.y += __shfl_xor(v4.y, 16, 64); v4.z += __shfl_xor(v4.z, 16, 64); v4.w += __shfl_xor(v4.w, 16, 64);
                v4.x += __shfl_xor(v4.x, 32, 64); v4.y += __shfl_xor(v4.y, 32, 64); v4.z += __shfl_xor(v4.z, 32, 64); v4.w += __shfl_xor(v4.w, 32, 64);
                if (lane < 16) *reinterpret_cast<float4*>(sz + 64 * j + 4 * sub) = v4;
            }
        }
        __syncthreads();
        if (on) {
            const float* sz = lds + kLdsZ + ((k & 1) * 2 + q) * 4 * kC;
            CAR_BOUNDS_TRAP(ray < BR);
            for (int d = tl; d < kC; d += 256) a.z_out[(long)ray * a.ld_z + d] = (sz[d] + sz[kC + d]) + (sz[2 * kC + d] + sz[3 * kC + d]);
        }
    }
}

}  // namespace

CAR_INTERNAL bool car_attend_round2_supports(int D, int V, int P) {
    return D == kC && V > 0 && V <= CAR_MAX_VIEWS && P > 0 && P % 32 == 0 && V * P <= kMaxSamples;
}

extern "C" int car_attend_round2(const float* g, const float* uh, const float* wpacked, const float* bias, const float* val, int D, int b, int V,
                                 int R, int P, float* w_out, float* z_out, int ld_z, float* logit_out, void* stream) {
    CAR_REQUIRE(g && uh && wpacked && bias && val && w_out && z_out, "car_attend_round2: null pointer");
    CAR_REQUIRE(b > 0 && V > 0 && V <= CAR_MAX_VIEWS && R > 0 && P > 0 && V * P <= kMaxSamples && (long)b * V * R < (1l << 30),
                "car_attend_round2: bad sizes");
    CAR_REQUIRE(car_attend_round2_supports(D, V, P) && ld_z >= D,
                "car_attend_round2: D = %d, P = %d, ld_z = %d: the merged round takes D = 576 and P %% 32 == 0 (car_round2_logits_from_g + car_attend take the rest)",
                D, P, ld_z);
    static int cus = 0;                                             // one persistent workgroup per compute unit
    if (cus <= 0) {
        const int n = car_device_cu_count();
        if (n <= 0) return n < 0 ? n : CAR_E_LAUNCH;
        cus = n;
    }
    const long nbatch = ((long)b * R + 1) / 2;
    const size_t lds_bytes = (size_t)kLdsFloats * sizeof(float);
    const Args a{g, uh, wpacked, bias, val, b, V, R, P, w_out, z_out, ld_z, logit_out};
    CAR_LAUNCH_LDS("car_attend_round2", round2_attend_kernel, dim3((unsigned)(nbatch < cus ? nbatch : cus)), dim3(kThreads), lds_bytes, (hipStream_t)stream, a);
    return CAR_OK;
}

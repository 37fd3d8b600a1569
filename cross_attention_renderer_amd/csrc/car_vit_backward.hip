// car_vit_backward.hip — the backward of the encoder's transformer stage (include/car_encoder_train.h): LayerNorm, exact
// GELU and multi-head attention backwards, the pack with the transposed matrices, and the stage's backward as a sequence of these entries,
// car_linear_x3 (dX = dY W on the transposed matrix) and car_linear_wgrad.  The recorded forward is car_vit.hip's.
//
// car_mha_backward is the one hot kernel pair.  Both stand on what car_mha stands on (car_mha_tile.h: the operand forms, the wave's rows as
// B operands, the epilogue): a wave owns 32 rows of one (scene, head) and streams tiles of 32 rows as A operands; the two logit-shaped
// products (s and dp) leave, per lane, 16 values of the lane's own row, which — multiplied out to p and ds, scaled and split in
// registers — ARE the B operand of the two value-shaped products.  mha_bwd_dq_kernel: the wave's rows are queries, the stream is the keys (s^T = K Q^T as the forward forms it,
// dp^T = V dO^T, dq^T += K^T ds^T).  mha_bwd_dkv_kernel: the wave's rows are keys, the stream is the queries (s = Q K^T, dp = dO V^T,
// dv^T += dO^T p, dk^T += Q^T ds).  Nothing is summed across waves: no atomics, every reduction in a fixed order.
// mha_bwd_absmax_kernel, mha_bwd_rows_kernel and mha_bwd_pack_kernel lay the seven A-operand forms of a tile out first.
#include "car_common.h"
#include <math.h>
#include <stdint.h>

namespace {

#include "car_mma32.h"
#include "car_vit_layout.h"
#include "car_mha_tile.h"

constexpr int kForm = 4 * kStep;                   // one operand form of a tile: 4 K steps
// the forms of a tile record, RC (rows x channels) and CR (channels x rows) as car_mha_tile.h writes them.  Powers of two: one per
// (scene, head) and tensor, except Q_RC, whose rows carry the forward's own per-row power (so that the logits are the forward's).
enum { F_K_RC, F_V_RC, F_K_CR, F_Q_RC, F_D_RC, F_Q_CR, F_D_CR, kForms };
constexpr int kTileBwd = kForms * kForm;
enum { T_Q, T_K, T_V, T_D, kTensors };

struct BwdArgs {
    const float* qkv; int ld;
    const float* out; int ldo;
    const float* dout; int ldd;
    const float* stats;    // [b heads][S][2]: the forward's running maximum and sum
    float* dqkv; int lddq;
    int b, S, heads, tiles;
    float* maxes;          // [b heads][tiles][4]: largest |q|, |k|, |v|, |dout| of a tile
    float* scales;         // [b heads][4]: 1 / p of q, k, v, dout
    float4* rows;          // [b heads][S]: 1 / p_q of the row, the forward's maximum and sum, D = sum_c dout out
    float* packed;         // [b heads][tiles][kTileBwd]
};

__device__ __forceinline__ const float* tensor_row(const BwdArgs& a, int t, int sc, int h, int row) {
    const int dim = a.heads * kHead;
    return t == T_D ? a.dout + ((long)sc * a.S + row) * a.ldd + h * kHead : a.qkv + ((long)sc * a.S + row) * a.ld + t * dim + h * kHead;
}

// largest magnitudes of one tile's q, k, v and dout (rows beyond the scene are not read)
__global__ void __launch_bounds__(256) mha_bwd_absmax_kernel(BwdArgs a) {
    const int tile = blockIdx.x % a.tiles, bh = blockIdx.x / a.tiles, h = bh % a.heads, sc = bh / a.heads;
    const int row = tile * kKeys + (threadIdx.x >> 3);
    tile_absmax<kTensors>(row, a.S, [&](int t) { return tensor_row(a, t, sc, h, row); }, a.maxes);
}

// one thread per (scene, head, row): the row's own power of two of q (as car_mha's wave takes it), the saved statistics, D
__global__ void __launch_bounds__(256) mha_bwd_rows_kernel(BwdArgs a) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)a.b * a.heads * a.S) return;
    const int row = (int)(i % a.S), bh = (int)(i / a.S), h = bh % a.heads, sc = bh / a.heads;
    const float* q = tensor_row(a, T_Q, sc, h, row);
    const float* d = tensor_row(a, T_D, sc, h, row);
    const float* o = a.out + ((long)sc * a.S + row) * a.ldo + h * kHead;
    float m = 0.0f, D = 0.0f;
    for (int c = 0; c < kHead; c += 4) {
        const float4 q4 = *reinterpret_cast<const float4*>(q + c), d4 = *reinterpret_cast<const float4*>(d + c), o4 = *reinterpret_cast<const float4*>(o + c);
        m = fmaxf(m, fmaxf(fmaxf(fabsf(q4.x), fabsf(q4.y)), fmaxf(fabsf(q4.z), fabsf(q4.w))));
        D = fmaf(d4.x, o4.x, D); D = fmaf(d4.y, o4.y, D); D = fmaf(d4.z, o4.z, D); D = fmaf(d4.w, o4.w, D);
    }
    float pq, iq;
    pow2_scale(fmaxf(m, 1e-30f), pq, iq);
    a.rows[i] = make_float4(iq, a.stats[i * 2], a.stats[i * 2 + 1], D);
}

// one tile record: thread (step, lane) writes the lane's halves of K step `step` of every form.  Rows beyond the scene are zeros and
// are not read.
__global__ void __launch_bounds__(256) mha_bwd_pack_kernel(BwdArgs a) {
    const int tile = blockIdx.x % a.tiles, bh = blockIdx.x / a.tiles, h = bh % a.heads, sc = bh / a.heads;
    const int step = threadIdx.x >> 6, lane = threadIdx.x & 63, row = tile * kKeys + (lane & 31);
    float p[kTensors];
#pragma unroll
    for (int t = 0; t < kTensors; ++t) {
        float m = 0.0f, inv;
        for (int k = 0; k < a.tiles; ++k) m = fmaxf(m, a.maxes[((long)bh * a.tiles + k) * kTensors + t]);
        if (t == T_D) pow2_scale<kPow2LoWide>(fmaxf(m, 1e-30f), p[t], inv);
        else pow2_scale(fmaxf(m, 1e-30f), p[t], inv);
        if (tile == 0 && threadIdx.x == 0) a.scales[bh * kTensors + t] = inv;
    }
    _Float16* rec = reinterpret_cast<_Float16*>(a.packed + ((long)bh * a.tiles + tile) * kTileBwd);
    const int rc_form[4] = {F_Q_RC, F_K_RC, F_V_RC, F_D_RC}, cr_form[4] = {F_Q_CR, F_K_CR, -1, F_D_CR};
#pragma unroll
    for (int t = 0; t < kTensors; ++t) {
        const float* src = row < a.S ? tensor_row(a, t, sc, h, row) : nullptr;
        const float s = t == T_Q && src ? 1.0f / a.rows[(long)bh * a.S + row].x : p[t];       // a power of two: the reciprocal is exact
        write_rc(rec + (long)rc_form[t] * (2 * kForm), step, lane, src, s);
        // the power of two inside the reader's row test, as this kernel always had it: multiplied in by write_cr, a step's eight loads are
        // in flight together and the kernel holds 70 registers in the place of 54, a wave per SIMD less
        if (cr_form[t] >= 0)
            write_cr(rec + (long)cr_form[t] * (2 * kForm), step, lane,
                     [=](int r, int c) { return tile * kKeys + r < a.S ? tensor_row(a, t, sc, h, tile * kKeys + r)[c] * p[t] : 0.0f; }, 1.0f);
    }
}

// the lane's 16 values of p or ds as the B operand of a value-shaped product: one power of two per row and tile, taken from the largest
// magnitude -> inv = 1 / p.  kPow2LoTiny: p in [2^-90, 2^126] — a key that a dominant one leaves a weight of e^-80 still gets ITS dv and
// dk to fp32-class accuracy (its own bound is as small as its weight), where the forward's fixed 2^13 would flush it to zero
constexpr int kPow2LoTiny = 14;
__device__ __forceinline__ float split_ds(const float (&ds)[16], half8 (&hi)[2], half8 (&lo)[2]) {
    float m = 0.0f;
#pragma unroll
    for (int r = 0; r < 16; ++r) m = fmaxf(m, fabsf(ds[r]));
    m = fmaxf(m, __shfl_xor(m, 32, 64));
    float p, inv;
    pow2_scale<kPow2LoTiny>(fmaxf(m, 1e-37f), p, inv);
#pragma unroll
    for (int kg = 0; kg < 2; ++kg) {
        float x8[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) x8[e] = ds[8 * kg + e];
        split8(x8, p, hi[kg], lo[kg]);
    }
    return inv;
}

// acc[t] (+)= form^T-shaped product: A = the CR form's 4 K steps, B = the lane's 16 values
__device__ __forceinline__ void mma_cr(f32x16 (&acc)[2], const float* form, const half8 (&bhi)[2], const half8 (&blo)[2]) {
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int kg = 0; kg < 2; ++kg) {
            half8 ah, al;
            read_a(form + (2 * t + kg) * kStep, ah, al);
            mma3(acc[t], ah, al, bhi[kg], blo[kg]);
        }
}
// acc += A B^T-shaped product over the 64 channels: A = the RC form's 4 K steps, B = the wave's rows
__device__ __forceinline__ void mma_rc(f32x16& acc, const float* form, const half8 (&bhi)[4], const half8 (&blo)[4]) {
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
        half8 ah, al;
        read_a(form + ks * kStep, ah, al);
        mma3(acc, ah, al, bhi[ks], blo[ks]);
    }
}

// ---- dq: one wave = 32 query rows of one (scene, head), streaming the key tiles ---------------------------------------------------------
__global__ void __launch_bounds__(256) mha_bwd_dq_kernel(BwdArgs a) {
    if (WaveRows::wave() >= (long)a.b * a.heads * a.tiles) return;
    const WaveRows w(a.S, a.heads, a.tiles);
    const int bh = w.bh, lane = w.lane, hh = w.hh;
    half8 qhi[4], qlo[4], dhi[4], dlo[4];
    const float iq = load_rows_b<kPow2Lo>(tensor_row(a, T_Q, w.sc, w.h, w.row) + 8 * hh, qhi, qlo);  // mha_kernel's call: the forward's split of q
    const float id = load_rows_b<kPow2LoWide>(tensor_row(a, T_D, w.sc, w.h, w.row) + 8 * hh, dhi, dlo);
    const float4 st = a.rows[(long)bh * a.S + w.row];
    const float ik = a.scales[bh * kTensors + T_K], iv = a.scales[bh * kTensors + T_V];
    const float cq = 0.125f * iq;
    f32x16 dq[2];
    zero(dq);
    const float* tw = a.packed + (long)bh * a.tiles * kTileBwd + 4 * lane;
    for (int kt = 0; kt < a.tiles; ++kt, tw += kTileBwd) {
        f32x16 sacc, dpacc;
        zero1(sacc); zero1(dpacc);
        mma_rc(sacc, tw + F_K_RC * kForm, qhi, qlo);
        mma_rc(dpacc, tw + F_V_RC * kForm, dhi, dlo);
        const int left = a.S - kt * kKeys;
        float ds[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float p = expf((sacc[r] * ik) * cq - st.y) / st.z;
            ds[r] = mma32_channel(0, r, hh) < left ? p * ((dpacc[r] * iv) * id - st.w) : 0.0f;       // a key beyond the scene: by its index
        }
        half8 shi[2], slo[2];
        const float is = split_ds(ds, shi, slo);
        f32x16 part[2];
        zero(part);
        mma_cr(part, tw + F_K_CR * kForm, shi, slo);
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) dq[t][r] = fmaf(part[t][r], is, dq[t][r]);
    }
    if (w.at >= a.S) return;
    store_rows(a.dqkv + ((long)w.sc * a.S + w.at) * a.lddq + w.h * kHead, dq, hh, [&](float x) { return (x * ik) * 0.125f; });
}

// ---- dk, dv: one wave = 32 keys of one (scene, head), streaming the query tiles -----------------------------------------------------------
__global__ void __launch_bounds__(256) mha_bwd_dkv_kernel(BwdArgs a) {
    if (WaveRows::wave() >= (long)a.b * a.heads * a.tiles) return;
    const WaveRows w(a.S, a.heads, a.tiles);
    const int bh = w.bh, lane = w.lane, hh = w.hh;
    half8 khi[4], klo[4], vhi[4], vlo[4];
    const float ik = load_rows_b<kPow2Lo>(tensor_row(a, T_K, w.sc, w.h, w.row) + 8 * hh, khi, klo);
    const float iv = load_rows_b<kPow2Lo>(tensor_row(a, T_V, w.sc, w.h, w.row) + 8 * hh, vhi, vlo);
    const float iqs = a.scales[bh * kTensors + T_Q], idd = a.scales[bh * kTensors + T_D];
    const float ck = 0.125f * ik;
    f32x16 dk[2], dv[2];
    zero(dk); zero(dv);
    const float* tw = a.packed + (long)bh * a.tiles * kTileBwd + 4 * lane;
    const float4* rows = a.rows + (long)bh * a.S;
    for (int qt = 0; qt < a.tiles; ++qt, tw += kTileBwd) {
        f32x16 sacc, dpacc;
        zero1(sacc); zero1(dpacc);
        mma_rc(sacc, tw + F_Q_RC * kForm, khi, klo);
        mma_rc(dpacc, tw + F_D_RC * kForm, vhi, vlo);
        float p[16], ds[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int qi = qt * kKeys + mma32_channel(0, r, hh);
            const float4 st = rows[qi < a.S ? qi : a.S - 1];
            const float w = expf((sacc[r] * st.x) * ck - st.y) / st.z;
            p[r] = qi < a.S ? w : 0.0f;                                                 // a query beyond the scene: by its index
            ds[r] = qi < a.S ? w * ((dpacc[r] * idd) * iv - st.w) : 0.0f;
        }
        half8 bhi[2], blo[2];
        f32x16 part[2];
        const float ip = split_ds(p, bhi, blo);
        zero(part);
        mma_cr(part, tw + F_D_CR * kForm, bhi, blo);
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) dv[t][r] = fmaf(part[t][r], ip, dv[t][r]);
        const float is = split_ds(ds, bhi, blo);
        zero(part);
        mma_cr(part, tw + F_Q_CR * kForm, bhi, blo);
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) dk[t][r] = fmaf(part[t][r], is, dk[t][r]);
    }
    if (w.at >= a.S) return;
    const int dim = a.heads * kHead;
    float* dst = a.dqkv + ((long)w.sc * a.S + w.at) * a.lddq + w.h * kHead;
    store_rows(dst + dim, dk, hh, [&](float x) { return (x * iqs) * 0.125f; });
    store_rows(dst + 2 * dim, dv, hh, [&](float x) { return x * idd; });
}

// car_mha_backward's workspace: pieces of whole 64 floats, the last one as long as it is
struct MhaBwdLayout { float *maxes, *scales; float4* rows; float* packed; size_t total; int tiles; };
MhaBwdLayout mha_bwd_layout(int b, int S, int heads, void* work = nullptr) {
    const int tiles = (S + kKeys - 1) / kKeys;
    const size_t bh = (size_t)b * heads;
    Carver c(work, 64);
    return {c.take<float>(bh * tiles * kTensors), c.take<float>(bh * kTensors), c.take<float4>(bh * S), c.take<float>(bh * tiles * kTileBwd, 1),
            c.bytes(), tiles};
}

// ---- LayerNorm backward: one wave per row, the row and its fp64 statistics from the forward's LnRow -----------------------------------
constexpr int kLnSlab = 64;
__global__ void __launch_bounds__(256) ln_bwd_kernel(const float* __restrict__ X, int ldx, const float* __restrict__ gamma, int C, double eps,
                                                      const float* dY, int lddy, float* dX, int lddx, long M, int accum, double* __restrict__ rowstat) {
    const long m = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= M) return;
    const int lane = threadIdx.x & 63;
    LnRow r;
    r.load(X + m * ldx, C, eps, lane);
    const float4 (&v)[LnRow::kVec] = r.v;
    const double mean = r.mean, rstd = r.rstd;
    if (rowstat && lane == 0) { rowstat[2 * m] = mean; rowstat[2 * m + 1] = rstd; }
    // a = gamma dy; s1 = sum a, s2 = sum a xhat
    const float* dy = dY + m * lddy;
    float4 a4[LnRow::kVec];
    double s1 = 0.0, s2 = 0.0;
#pragma unroll
    for (int i = 0; i < LnRow::kVec; ++i) {
        const int c = (i * 64 + lane) * 4;
        a4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c < C) {
            const float4 g = *reinterpret_cast<const float4*>(gamma + c), d = *reinterpret_cast<const float4*>(dy + c);
            a4[i] = make_float4(g.x * d.x, g.y * d.y, g.z * d.z, g.w * d.w);
            s1 += ((double)a4[i].x + (double)a4[i].y) + ((double)a4[i].z + (double)a4[i].w);
            s2 += ((double)a4[i].x * (((double)v[i].x - mean) * rstd) + (double)a4[i].y * (((double)v[i].y - mean) * rstd)) +
                  ((double)a4[i].z * (((double)v[i].z - mean) * rstd) + (double)a4[i].w * (((double)v[i].w - mean) * rstd));
        }
    }
    const double m1 = wave_sum(s1) / (double)C, m2 = wave_sum(s2) / (double)C;
    float* dx = dX + m * lddx;
#pragma unroll
    for (int i = 0; i < LnRow::kVec; ++i) {
        const int c = (i * 64 + lane) * 4;
        if (c < C) {
            float4 o;
            o.x = (float)(rstd * ((double)a4[i].x - m1 - (((double)v[i].x - mean) * rstd) * m2));
            o.y = (float)(rstd * ((double)a4[i].y - m1 - (((double)v[i].y - mean) * rstd) * m2));
            o.z = (float)(rstd * ((double)a4[i].z - m1 - (((double)v[i].z - mean) * rstd) * m2));
            o.w = (float)(rstd * ((double)a4[i].w - m1 - (((double)v[i].w - mean) * rstd) * m2));
            if (accum) {
                const float4 old = *reinterpret_cast<const float4*>(dx + c);
                o.x += old.x; o.y += old.y; o.z += old.z; o.w += old.w;
            }
            *reinterpret_cast<float4*>(dx + c) = o;
        }
    }
}
// dgamma, dbeta, first level: one thread per column sums a slab of kLnSlab rows in row order -> part[slab][2][C]
__global__ void __launch_bounds__(256) ln_bwd_slab_kernel(const float* __restrict__ X, int ldx, const float* __restrict__ dY, int lddy, int C, long M,
                                                           const double* __restrict__ rowstat, double* __restrict__ part) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const long m0 = (long)blockIdx.y * kLnSlab, m1 = m0 + kLnSlab < M ? m0 + kLnSlab : M;
    double sg = 0.0, sb = 0.0;
    for (long m = m0; m < m1; ++m) {
        const double d = (double)dY[m * lddy + c];
        sg += d * (((double)X[m * ldx + c] - rowstat[2 * m]) * rowstat[2 * m + 1]);
        sb += d;
    }
    part[((long)blockIdx.y * 2) * C + c] = sg;
    part[((long)blockIdx.y * 2 + 1) * C + c] = sb;
}
// second level: one thread per column sums the slabs in slab order; the result is WRITTEN
__global__ void __launch_bounds__(256) ln_bwd_sum_kernel(const double* __restrict__ part, int C, int slabs, float* __restrict__ dgamma, float* __restrict__ dbeta) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    double sg = 0.0, sb = 0.0;
    for (int s = 0; s < slabs; ++s) { sg += part[((long)s * 2) * C + c]; sb += part[((long)s * 2 + 1) * C + c]; }
    dgamma[c] = (float)sg;
    dbeta[c] = (float)sb;
}
struct LnBwdLayout { double *rowstat, *part; size_t total; int slabs; };
LnBwdLayout ln_bwd_layout(long M, int C, void* work = nullptr) {
    const int slabs = (int)((M + kLnSlab - 1) / kLnSlab);
    Carver c(work, 8);
    return {c.take<double>(2 * (size_t)M), c.take<double>((size_t)slabs * 2 * C, 1), c.bytes(), slabs};
}

// ---- exact GELU backward, in place on dy ----------------------------------------------------------------------------------------------
__device__ __forceinline__ float gelu_grad1(float u) {
    return fmaf(u * 0.39894228040143267794f, expf(-0.5f * u * u), 0.5f * erfcf(-0.70710678118654752440f * u));
}
__global__ void __launch_bounds__(256) gelu_bwd_kernel(const float* __restrict__ U, int ldu, float* __restrict__ dY, int lddy, long M, int N4) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= M * N4) return;
    const float4 u = *reinterpret_cast<const float4*>(U + (i / N4) * ldu + (i % N4) * 4);
    float4* p = reinterpret_cast<float4*>(dY + (i / N4) * lddy + (i % N4) * 4);
    float4 v = *p;
    v.x *= gelu_grad1(u.x); v.y *= gelu_grad1(u.y); v.z *= gelu_grad1(u.z); v.w *= gelu_grad1(u.w);
    *p = v;
}

// ---- the transposed matrices of car_vit_pack_train -----------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) transpose_kernel(const float* __restrict__ W, int N, int K, float* __restrict__ T) {   // W [N][K] -> T [K][N]
    __shared__ float tile[32][33];
    const int n0 = blockIdx.y * 32, k0 = blockIdx.x * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int r = ty; r < 32; r += 8)
        if (n0 + r < N && k0 + tx < K) tile[r][tx] = W[(long)(n0 + r) * K + k0 + tx];
    __syncthreads();
    for (int r = ty; r < 32; r += 8)
        if (k0 + r < K && n0 + tx < N) T[(long)(k0 + r) * N + n0 + tx] = tile[tx][r];
}

// car_vit_blocks_backward's workspace: the maps of whole 64 floats, then the two nested workspaces
struct VitBwdWork { float *norm, *small, *wide, *dwide; void *mha, *ln; size_t mha_bytes, ln_bytes, total; };
VitBwdWork vit_bwd_work(int b, int S, int dim, void* work = nullptr) {
    const size_t rows = (size_t)b * S, d = (size_t)dim;
    const size_t mha_bytes = mha_bwd_layout(b, S, dim / kHead).total, ln_bytes = ln_bwd_layout((long)rows, dim).total;
    Carver c(work, 64);
    float *norm = c.take<float>(rows * d), *small = c.take<float>(rows * d), *wide = c.take<float>(rows * 4 * d), *dwide = c.take<float>(rows * 4 * d);
    void* mha = c.sub(mha_bytes).take<char>(mha_bytes);
    c.align(256);
    void* ln = c.sub(ln_bytes).take<char>(ln_bytes);
    return {norm, small, wide, dwide, mha, ln, mha_bytes, ln_bytes, c.bytes()};
}

}  // namespace

extern "C" size_t car_layernorm_backward_workspace_bytes(long M, int C) {
    if (M < 1 || M > (1L << 31) || !ln_shape_ok(C, "car_layernorm_backward_workspace_bytes")) {      // this entry's text names M too
        car_set_error("car_layernorm_backward_workspace_bytes: M = %ld, C = %d: C must be a multiple of 4 in 4..%d", M, C, kLnMax);
        return 0;
    }
    return ln_bwd_layout(M, C).total;
}

extern "C" int car_layernorm_backward(const float* X, int ldx, const float* gamma, int C, double eps, const float* dY, int lddy, float* dX, int lddx,
                                      long M, int flags, float* dgamma, float* dbeta, void* work, size_t work_bytes, void* stream) {
    const char* who = "car_layernorm_backward";
    CAR_REQUIRE(X && gamma && dY && dX && (!dgamma == !dbeta) && (!dgamma || work), "%s: null pointer", who);
    if (!ln_shape_ok(C, who)) return CAR_E_ARG;
    CAR_REQUIRE(M > 0 && M <= (1L << 31) && eps >= 0.0, "%s: bad sizes (M = %ld, eps = %g)", who, M, eps);
    CAR_REQUIRE((flags & ~CAR_LIN_ACCUM) == 0, "%s: flags = %d: CAR_LIN_ACCUM is the only one", who, flags);
    CAR_REQUIRE(ldx >= C && lddy >= C && lddx >= C && ldx % 4 == 0 && lddy % 4 == 0 && lddx % 4 == 0,
                "%s: the row strides (%d, %d, %d) must hold C = %d and be multiples of 4", who, ldx, lddy, lddx, C);
    CAR_REQUIRE(aligned16(X) && aligned16(gamma) && aligned16(dY) && aligned16(dX) && aligned16(work), "%s: X, gamma, dY, dX and work must be 16-byte aligned", who);
    const LnBwdLayout l = ln_bwd_layout(M, C, work);
    if (dgamma) CAR_REQUIRE(work_bytes >= l.total, "%s: the workspace is too small (%zu bytes, car_layernorm_backward_workspace_bytes says %zu)", who, work_bytes, l.total);
    hipStream_t st = (hipStream_t)stream;
    (void)hipGetLastError();
    hipLaunchKernelGGL(ln_bwd_kernel, dim3(car_div_up(M, 4)), dim3(256), 0, st, X, ldx, gamma, C, eps, dY, lddy, dX, lddx, M, flags & CAR_LIN_ACCUM,
                       dgamma ? l.rowstat : (double*)nullptr);
    if (dgamma) {
        hipLaunchKernelGGL(ln_bwd_slab_kernel, dim3(car_div_up(C, 256), l.slabs), dim3(256), 0, st, X, ldx, dY, lddy, C, M, l.rowstat, l.part);
        hipLaunchKernelGGL(ln_bwd_sum_kernel, dim3(car_div_up(C, 256)), dim3(256), 0, st, l.part, C, l.slabs, dgamma, dbeta);
    }
    CAR_CHECK_LAUNCH(who);
    return CAR_OK;
}

extern "C" int car_gelu_backward(const float* U, int ldu, float* dY, int lddy, long M, int N, void* stream) {
    const char* who = "car_gelu_backward";
    CAR_REQUIRE(U && dY, "%s: null pointer", who);
    CAR_REQUIRE(M > 0 && N > 0 && N % 4 == 0 && (M * (N / 4)) / 256 < (1L << 31), "%s: bad sizes (M = %ld, N = %d: N must be a multiple of 4)", who, M, N);
    CAR_REQUIRE(ldu >= N && lddy >= N && ldu % 4 == 0 && lddy % 4 == 0, "%s: the row strides (%d, %d) must hold N = %d and be multiples of 4", who, ldu, lddy, N);
    CAR_REQUIRE(aligned16(U) && aligned16(dY), "%s: U and dY must be 16-byte aligned", who);
    (void)hipGetLastError();
    hipLaunchKernelGGL(gelu_bwd_kernel, dim3(car_div_up(M * (N / 4), 256)), dim3(256), 0, (hipStream_t)stream, U, ldu, dY, lddy, M, N / 4);
    CAR_CHECK_LAUNCH(who);
    return CAR_OK;
}

extern "C" size_t car_mha_backward_workspace_bytes(int b, int S, int heads) {
    return mha_shape_ok(b, S, heads, "car_mha_backward_workspace_bytes") ? mha_bwd_layout(b, S, heads).total : 0;
}

extern "C" int car_mha_backward(const float* qkv, int ld, const float* stats, const float* out, int ldo, const float* dout, int ldd, int b, int S,
                                int heads, float* dqkv, int lddq, void* work, size_t work_bytes, void* stream) {
    const char* who = "car_mha_backward";
    CAR_REQUIRE(qkv && stats && out && dout && dqkv && work, "%s: null pointer", who);
    if (!mha_shape_ok(b, S, heads, who)) return CAR_E_ARG;
    const int dim = heads * kHead;
    CAR_REQUIRE(ld >= 3 * dim && ld % 4 == 0 && lddq >= 3 * dim && lddq % 4 == 0,
                "%s: the row strides of qkv and dqkv (%d, %d) must hold 3 x %d columns and be multiples of 4", who, ld, lddq, dim);
    CAR_REQUIRE(ldo >= dim && ldo % 4 == 0 && ldd >= dim && ldd % 4 == 0,
                "%s: the row strides of out and dout (%d, %d) must hold %d columns and be multiples of 4", who, ldo, ldd, dim);
    CAR_REQUIRE(aligned16(qkv) && aligned16(stats) && aligned16(out) && aligned16(dout) && aligned16(dqkv) && aligned16(work),
                "%s: qkv, stats, out, dout, dqkv and work must be 16-byte aligned", who);
    const MhaBwdLayout l = mha_bwd_layout(b, S, heads, work);
    CAR_REQUIRE(work_bytes >= l.total, "%s: the workspace is too small (%zu bytes, car_mha_backward_workspace_bytes says %zu)", who, work_bytes, l.total);
    BwdArgs a{qkv, ld, out, ldo, dout, ldd, stats, dqkv, lddq, b, S, heads, l.tiles, l.maxes, l.scales, l.rows, l.packed};
    hipStream_t st = (hipStream_t)stream;
    const unsigned tiles_all = (unsigned)(b * heads * l.tiles);
    (void)hipGetLastError();
    hipLaunchKernelGGL(mha_bwd_absmax_kernel, dim3(tiles_all), dim3(256), 0, st, a);
    hipLaunchKernelGGL(mha_bwd_rows_kernel, dim3(car_div_up((long)b * heads * S, 256)), dim3(256), 0, st, a);
    hipLaunchKernelGGL(mha_bwd_pack_kernel, dim3(tiles_all), dim3(256), 0, st, a);
    hipLaunchKernelGGL(mha_bwd_dq_kernel, dim3(car_div_up(tiles_all, 4)), dim3(256), 0, st, a);
    hipLaunchKernelGGL(mha_bwd_dkv_kernel, dim3(car_div_up(tiles_all, 4)), dim3(256), 0, st, a);
    CAR_CHECK_LAUNCH(who);
    return CAR_OK;
}

extern "C" size_t car_vit_packed_train_floats(int dim, int depth) {
    const char* who = "car_vit_packed_train_floats";
    if (!vit_dim_ok(dim, who) || !vit_depth_ok(depth, who)) return 0;
    return vit_train_layout(dim, depth).total;
}

extern "C" size_t car_vit_packed_train_offset(int dim, int depth, int item) {
    const char* who = "car_vit_packed_train_offset";
    if (!vit_dim_ok(dim, who) || !vit_depth_ok(depth, who)) return 0;
    if (item < 0 || item > 5) { car_set_error("%s: item %d is outside 0..5", who, item); return 0; }
    const VitTrainLayout l = vit_train_layout(dim, depth);
    return item == 5 ? l.tr : l.off[item];
}

extern "C" int car_vit_pack_train(const float* const* params, int n_params, int dim, int depth, float* packed, void* stream) {
    const char* who = "car_vit_pack_train";
    CAR_REQUIRE(params && packed, "%s: null pointer", who);
    if (!vit_dim_ok(dim, who) || !vit_depth_ok(depth, who)) return CAR_E_ARG;
    CAR_REQUIRE(n_params == 12 * depth, "%s: %d parameter arrays do not fit depth %d (12 per block)", who, n_params, depth);
    for (int i = 0; i < n_params; ++i) CAR_REQUIRE(params[i], "%s: null pointer (parameter %d)", who, i);
    CAR_REQUIRE(aligned16(packed), "%s: packed must be 16-byte aligned", who);
    CAR_TRY(car_vit_pack(params, n_params, dim, depth, packed, stream));
    const VitTrainLayout l = vit_train_layout(dim, depth);
    const VitShapes s = vit_shapes(dim);
    const int mats[4] = {2, 4, 8, 10};
    float* scratch = packed + l.scratch;
    for (int blk = 0; blk < depth; ++blk)
        for (int t = 0; t < 4; ++t) {
            const int N = s.n[mats[t]], K = s.k[mats[t]];
            (void)hipGetLastError();
            hipLaunchKernelGGL(transpose_kernel, dim3(car_div_up(K, 32), car_div_up(N, 32)), dim3(256), 0, (hipStream_t)stream, params[blk * 12 + mats[t]], N, K,
                               scratch);
            CAR_CHECK_LAUNCH(who);
            // W^T is a [K][N] matrix: a layer with N inputs and K outputs
            CAR_TRY(car_linear_x3_pack(scratch, N, N, K, packed + l.tr + (size_t)blk * l.off[4] + l.off[t], stream));
        }
    return CAR_OK;
}

extern "C" size_t car_vit_grad_offset(int dim, int item) {
    if (!vit_dim_ok(dim, "car_vit_grad_offset")) return 0;
    if (item < 0 || item > 12) { car_set_error("car_vit_grad_offset: item %d is outside 0..12", item); return 0; }
    return vit_grad_layout(dim).off[item];
}

extern "C" size_t car_vit_backward_workspace_bytes(int b, int S, int dim) {
    const char* who = "car_vit_backward_workspace_bytes";
    if (!vit_dim_ok(dim, who) || !mha_shape_ok(b, S, dim / kHead, who)) return 0;
    return vit_bwd_work(b, S, dim).total;
}

extern "C" int car_vit_blocks_backward(float* dtok, int b, int S, int dim, const float* packed, int depth, const int* taps, int n_taps,
                                       const float* const* dtaps, const void* saved, size_t saved_bytes, float* dparams, int flags, void* work,
                                       size_t work_bytes, void* stream) {
    const char* who = "car_vit_blocks_backward";
    CAR_REQUIRE(dtok && packed && saved && dparams && work && (n_taps == 0 || (taps && dtaps)), "%s: null pointer", who);
    if (!vit_dim_ok(dim, who) || !mha_shape_ok(b, S, dim / kHead, who) || !vit_depth_ok(depth, who)) return CAR_E_ARG;
    CAR_REQUIRE(n_taps >= 0 && n_taps <= depth, "%s: %d taps for %d blocks", who, n_taps, depth);
    for (int i = 0; i < n_taps; ++i) {
        CAR_REQUIRE(taps[i] >= 0 && taps[i] < depth && (i == 0 || taps[i] > taps[i - 1]),
                    "%s: taps must be strictly increasing block indices below depth = %d (tap %d is %d)", who, depth, i, taps[i]);
        CAR_REQUIRE(aligned16(dtaps[i]), "%s: dtaps %d must be 16-byte aligned", who, i);
    }
    CAR_REQUIRE((flags & ~CAR_WGRAD_FP32) == 0, "%s: flags = %d: CAR_WGRAD_FP32 is the only one", who, flags);
    CAR_REQUIRE(aligned16(dtok) && aligned16(packed) && aligned16(saved) && aligned16(dparams) && aligned16(work),
                "%s: dtok, packed, saved, dparams and work must be 16-byte aligned", who);
    const VitBwdWork w = vit_bwd_work(b, S, dim, work);
    CAR_REQUIRE(work_bytes >= w.total, "%s: the workspace is too small (%zu bytes, car_vit_backward_workspace_bytes says %zu)", who, work_bytes, w.total);
    const size_t need = vit_saved(b, S, dim, depth).total;
    CAR_REQUIRE(saved_bytes >= need, "%s: the saved buffer is too small (%zu bytes, car_vit_saved_bytes says %zu)", who, saved_bytes, need);
    const VitLayout l = vit_layout(dim), gl = vit_grad_layout(dim);
    const VitTrainLayout tl = vit_train_layout(dim, depth);
    const long rows = (long)b * S;
    const int heads = dim / kHead, d3 = 3 * dim, d4 = 4 * dim;
    float *g = dtok, *norm = w.norm, *small = w.small, *wide = w.wide, *dwide = w.dwide;
    hipStream_t st = (hipStream_t)stream;
    int next_tap = n_taps - 1;
    for (int blk = depth - 1; blk >= 0; --blk) {
        const float* p = packed + (size_t)blk * l.off[12];
        const float* pt = packed + tl.tr + (size_t)blk * tl.off[4];
        float* dp = dparams + (size_t)blk * gl.off[12];
        const VitSaved sv = vit_saved(b, S, dim, depth, blk, saved);
        if (next_tap >= 0 && taps[next_tap] == blk) {                   // the tap was taken here: its gradient joins the stream here
            if (dtaps[next_tap]) CAR_TRY(car_add(g, dim, g, dim, 1.0f, dtaps[next_tap], dim, 1.0f, rows, dim, stream));
            --next_tap;
        }
        // the MLP half: x2 = x1 + fc2(gelu(fc1(LN2(x1))))
        CAR_TRY(car_layernorm(sv.x1, dim, p + l.off[6], p + l.off[7], dim, 1e-6, norm, dim, rows, stream));
        CAR_CHECK_HIP(hipMemcpyAsync(wide, sv.u, sizeof(float) * rows * d4, hipMemcpyDeviceToDevice, st), "%s: copy failed", who);
        CAR_TRY(car_gelu(wide, d4, rows, d4, stream));
        CAR_TRY(car_linear_wgrad(g, dim, wide, d4, rows, dim, d4, flags, dp + gl.off[10], d4, dp + gl.off[11], stream));
        CAR_TRY(car_linear_x3(g, dim, pt + tl.off[3], nullptr, dim, d4, dwide, d4, rows, 0, stream));
        CAR_TRY(car_gelu_backward(sv.u, d4, dwide, d4, rows, d4, stream));
        CAR_TRY(car_linear_wgrad(dwide, d4, norm, dim, rows, d4, dim, flags, dp + gl.off[8], dim, dp + gl.off[9], stream));
        CAR_TRY(car_linear_x3(dwide, d4, pt + tl.off[2], nullptr, d4, dim, small, dim, rows, 0, stream));
        CAR_TRY(car_layernorm_backward(sv.x1, dim, p + l.off[6], dim, 1e-6, small, dim, g, dim, rows, CAR_LIN_ACCUM, dp + gl.off[6], dp + gl.off[7], w.ln,
                                       w.ln_bytes, stream));
        // the attention half: x1 = x0 + proj(mha(qkv(LN1(x0))))
        CAR_TRY(car_linear_wgrad(g, dim, sv.att, dim, rows, dim, dim, flags, dp + gl.off[4], dim, dp + gl.off[5], stream));
        CAR_TRY(car_linear_x3(g, dim, pt + tl.off[1], nullptr, dim, dim, small, dim, rows, 0, stream));
        CAR_TRY(car_mha_backward(sv.qkv, d3, sv.stats, sv.att, dim, small, dim, b, S, heads, dwide, d3, w.mha, w.mha_bytes, stream));
        CAR_TRY(car_layernorm(sv.x0, dim, p + l.off[0], p + l.off[1], dim, 1e-6, norm, dim, rows, stream));
        CAR_TRY(car_linear_wgrad(dwide, d3, norm, dim, rows, d3, dim, flags, dp + gl.off[2], dim, dp + gl.off[3], stream));
        CAR_TRY(car_linear_x3(dwide, d3, pt + tl.off[0], nullptr, d3, dim, small, dim, rows, 0, stream));
        CAR_TRY(car_layernorm_backward(sv.x0, dim, p + l.off[0], dim, 1e-6, small, dim, g, dim, rows, CAR_LIN_ACCUM, dp + gl.off[0], dp + gl.off[1], w.ln,
                                       w.ln_bytes, stream));
    }
    return CAR_OK;
}

// car_vit.hip — the transformer stage of get_z's image encoder (include/car_encoder.h; encoder.py MultiViewDPTEncoder.forward, the 12
// pre-norm blocks over the concatenated tokens of a scene's views): LayerNorm, exact GELU, multi-head attention with head width 64, the
// pack of a stage's parameters and the stage itself as a sequence of these entries and car_linear_x3; car_mha_stats and car_vit_blocks_train are the same kernels
// with what the backward (car_vit_backward.hip, include/car_encoder_train.h) needs written down.
//
// car_mha is the one hot kernel here.  One wave owns 32 query rows of one (scene, head) as the B operand of car_mma32.h's chained
// 32 x 32 x 16 tile; per tile of 32 keys it forms S^T = K Q^T (the keys are the A "weights", K = 64 head channels = 4 K steps), whose
// accumulators hold, per lane, 16 of the 32 logits of the lane's query — the other 16 live in lane ^ 32 — and, once exponentiated and split
// in registers, ARE the B operand of O^T += V^T P (A = the V tile transposed, K = the 32 keys in the chained order).  The running maximum
// and sum of a query row and the 32 x 64 output accumulators follow the online softmax.  mha_absmax_kernel and mha_pack_kernel lay k and v of the whole
// call out as hi / lo A-operand tiles first, one power of two per (scene, head), the padding keys zero.  The two operand forms, the
// wave's rows as B operands and the epilogue are car_mha_tile.h's, which the backward shares; LayerNorm's row pass is car_vit_layout.h's.
#include "car_common.h"
#include <math.h>
#include <stdint.h>

namespace {

#include "car_mma32.h"
#include "car_vit_layout.h"
#include "car_mha_tile.h"

constexpr int kTileK = 4 * kStep;                  // the K part of a tile record: 4 K steps over the 64 channels
constexpr int kTileFloats = 2 * kTileK;            // + the V part: [channel tile (2)][kg (2)] K steps over the 32 keys
constexpr float kPScale = 8192.0f;                 // the numerators' power of two: p in [0, 1] -> [0, 2^13]

// ---- LayerNorm: one wave per row, the row in registers, statistics in fp64 ------------------------------------------------------------
__global__ void __launch_bounds__(256) layernorm_kernel(const float* __restrict__ X, int ldx, const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, int C, double eps, float* __restrict__ Y, int ldy, long M) {
    const long m = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= M) return;
    const int lane = threadIdx.x & 63;
    LnRow r;
    r.load(X + m * ldx, C, eps, lane);
    float* y = Y + m * ldy;
#pragma unroll
    for (int i = 0; i < LnRow::kVec; ++i) {
        const int c = (i * 64 + lane) * 4;
        if (c < C) {
            const float4 g = *reinterpret_cast<const float4*>(gamma + c), b = *reinterpret_cast<const float4*>(beta + c), v = r.v[i];
            float4 o;
            o.x = fmaf((float)(((double)v.x - r.mean) * r.rstd), g.x, b.x);
            o.y = fmaf((float)(((double)v.y - r.mean) * r.rstd), g.y, b.y);
            o.z = fmaf((float)(((double)v.z - r.mean) * r.rstd), g.z, b.z);
            o.w = fmaf((float)(((double)v.w - r.mean) * r.rstd), g.w, b.w);
            *reinterpret_cast<float4*>(y + c) = o;
        }
    }
}

// ---- exact GELU, in place --------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float gelu1(float x) { return 0.5f * x * erfcf(-0.70710678118654752440f * x); }
__global__ void __launch_bounds__(256) gelu_kernel(float* __restrict__ Y, int ldy, long M, int N4) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= M * N4) return;
    float4* p = reinterpret_cast<float4*>(Y + (i / N4) * ldy + (i % N4) * 4);
    float4 v = *p;
    v.x = gelu1(v.x); v.y = gelu1(v.y); v.z = gelu1(v.z); v.w = gelu1(v.w);
    *p = v;
}

// ---- attention: the operand tiles of k and v -------------------------------------------------------------------------------------------
struct MhaArgs {
    const float* qkv; int ld; int b, S, heads, tiles;
    float* out; int ldo;
    float* maxes;          // [b heads][tiles][2]: largest |k|, |v| of a tile
    float* scales;         // [b heads][2]: 1 / p_k, 1 / p_v
    float* packed;         // [b heads][tiles][kTileFloats]
    float* stats;          // null, or [b heads][S][2]: the running maximum and sum a query row ends with (car_mha_stats)
};

// largest magnitudes of one tile's k and v (rows beyond the scene are not read)
__global__ void __launch_bounds__(256) mha_absmax_kernel(MhaArgs a) {
    const int tile = blockIdx.x % a.tiles, bh = blockIdx.x / a.tiles, h = bh % a.heads, sc = bh / a.heads;
    const int key = tile * kKeys + (threadIdx.x >> 3), dim = a.heads * kHead;
    tile_absmax<2>(key, a.S, [&](int t) { return a.qkv + ((long)sc * a.S + key) * a.ld + h * kHead + (t + 1) * dim; }, a.maxes);
}

// one tile record: the K part is k in car_mha_tile.h's rows x channels form, the V part v in its channels x rows form
__global__ void __launch_bounds__(256) mha_pack_kernel(MhaArgs a) {
    const int tile = blockIdx.x % a.tiles, bh = blockIdx.x / a.tiles, h = bh % a.heads, sc = bh / a.heads;
    const int dim = a.heads * kHead, step = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float mk = 0.0f, mv = 0.0f;
    for (int t = 0; t < a.tiles; ++t) {
        mk = fmaxf(mk, a.maxes[((long)bh * a.tiles + t) * 2]);
        mv = fmaxf(mv, a.maxes[((long)bh * a.tiles + t) * 2 + 1]);
    }
    float pk, ik, pv, iv;
    pow2_scale(fmaxf(mk, 1e-30f), pk, ik);
    pow2_scale(fmaxf(mv, 1e-30f), pv, iv);
    if (tile == 0 && threadIdx.x == 0) { a.scales[bh * 2] = ik; a.scales[bh * 2 + 1] = iv; }
    const float* base = a.qkv + (long)sc * a.S * a.ld + h * kHead;
    _Float16* rec = reinterpret_cast<_Float16*>(a.packed + ((long)bh * a.tiles + tile) * kTileFloats);
    const int key = tile * kKeys + (lane & 31);
    write_rc(rec, step, lane, key < a.S ? base + (long)key * a.ld + dim : nullptr, pk);
    write_cr(rec + 2 * kTileK, step, lane, [=](int r, int c) { return tile * kKeys + r < a.S ? base[(long)(tile * kKeys + r) * a.ld + 2 * dim + c] : 0.0f; }, pv);
}

// ---- attention: one wave = 32 query rows of one (scene, head) --------------------------------------------------------------------------
__global__ void __launch_bounds__(256) mha_kernel(MhaArgs a) {
    if (WaveRows::wave() >= (long)a.b * a.heads * a.tiles) return;
    const WaveRows w(a.S, a.heads, a.tiles);
    const int bh = w.bh, lane = w.lane, hh = w.hh;
    half8 qhi[4], qlo[4];
    const float iq = load_rows_b<kPow2Lo>(a.qkv + ((long)w.sc * a.S + w.row) * a.ld + w.h * kHead + 8 * hh, qhi, qlo);
    const float ik = a.scales[bh * 2], iv = a.scales[bh * 2 + 1];
    const float cq = 0.125f * iq;                                                       // 1 / sqrt(64), with the query row's power of two

    f32x16 o[2];
    zero(o);
    float mrun = -INFINITY, lrun = 0.0f;
    const float* tw = a.packed + (long)bh * a.tiles * kTileFloats + 4 * lane;
    // one wave per SIMD at the eval shape: nobody else hides a load, so the K operands of tile kt + 1 are requested while tile kt's softmax
    // runs, and the V operands of tile kt before its logits are formed
    half8 kh[4], kl[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) read_a(tw + ks * kStep, kh[ks], kl[ks]);
    for (int kt = 0; kt < a.tiles; ++kt, tw += kTileFloats) {
        half8 vh[4], vl[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) read_a(tw + kTileK + i * kStep, vh[i], vl[i]);
        f32x16 sacc;
        zero1(sacc);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) mma3(sacc, kh[ks], kl[ks], qhi[ks], qlo[ks]);
        if (kt + 1 < a.tiles) {
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) read_a(tw + kTileFloats + ks * kStep, kh[ks], kl[ks]);
        }
        // the lane's 16 logits: keys kt 32 + mma32_channel(0, r, hh); a key beyond the scene is masked by its index
        const int left = a.S - kt * kKeys;
        float p[16], tm = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            p[r] = mma32_channel(0, r, hh) < left ? (sacc[r] * ik) * cq : -INFINITY;
            tm = fmaxf(tm, p[r]);
        }
        tm = fmaxf(tm, __shfl_xor(tm, 32, 64));
        const float mnew = fmaxf(mrun, tm), alpha = expf(mrun - mnew);
        float psum = 0.0f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            p[r] = mma32_channel(0, r, hh) < left ? expf(p[r] - mnew) : 0.0f;
            psum += p[r];
        }
        psum += __shfl_xor(psum, 32, 64);
        lrun = lrun * alpha + psum;
        mrun = mnew;
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[t][r] *= alpha;
        half8 phi[2], plo[2];
#pragma unroll
        for (int kg = 0; kg < 2; ++kg) {
            float p8[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) p8[e] = p[8 * kg + e];
            split8(p8, kPScale, phi[kg], plo[kg]);
        }
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int kg = 0; kg < 2; ++kg) mma3(o[t], vh[2 * t + kg], vl[2 * t + kg], phi[kg], plo[kg]);
    }
    if (w.at >= a.S) return;
    if (a.stats && hh == 0) *reinterpret_cast<float2*>(a.stats + ((long)bh * a.S + w.at) * 2) = make_float2(mrun, lrun);
    const float c = iv * (1.0f / kPScale);
    store_rows(a.out + ((long)w.sc * a.S + w.at) * a.ldo + w.h * kHead, o, hh, [&](float x) { return (x * c) / lrun; });
}

// car_mha's workspace: pieces of whole 64 floats, the last one as long as it is
struct MhaLayout { float *maxes, *scales, *packed; size_t total; int tiles; };
MhaLayout mha_layout(int b, int S, int heads, void* work = nullptr) {
    const int tiles = (S + kKeys - 1) / kKeys;
    const size_t bh = (size_t)b * heads;
    Carver c(work, 64);
    return {c.take<float>(bh * tiles * 2), c.take<float>(bh * 2), c.take<float>(bh * tiles * kTileFloats, 1), c.bytes(), tiles};
}
// car_vit_blocks' workspace: three maps of whole 64 floats, then car_mha's own workspace as a range nested in this one
struct VitWork { float *norm, *att, *wide, *mha; size_t mha_bytes, total; };
VitWork vit_work(int b, int S, int dim, void* work = nullptr) {
    const size_t rows = (size_t)b * S, d = (size_t)dim, mha_bytes = mha_layout(b, S, dim / kHead).total;
    Carver c(work, 64);                                                 // wide: qkv [rows][3 dim], then the hidden rows [rows][4 dim]
    return {c.take<float>(rows * d), c.take<float>(rows * d), c.take<float>(rows * 4 * d), c.sub(mha_bytes).take<float>(mha_bytes / sizeof(float)),
            mha_bytes, c.bytes()};
}

}  // namespace

extern "C" int car_layernorm(const float* X, int ldx, const float* gamma, const float* beta, int C, double eps, float* Y, int ldy, long M,
                             void* stream) {
    CAR_REQUIRE(X && gamma && beta && Y, "car_layernorm: null pointer");
    if (!ln_shape_ok(C, "car_layernorm")) return CAR_E_ARG;
    CAR_REQUIRE(M > 0 && M <= (1L << 31) && eps >= 0.0, "car_layernorm: bad sizes (M = %ld, eps = %g)", M, eps);
    CAR_REQUIRE(ldx >= C && ldy >= C && ldx % 4 == 0 && ldy % 4 == 0, "car_layernorm: the row strides (%d, %d) must hold C = %d and be multiples of 4",
                ldx, ldy, C);
    CAR_REQUIRE(aligned16(X) && aligned16(Y) && aligned16(gamma) && aligned16(beta), "car_layernorm: X, Y, gamma and beta must be 16-byte aligned");
    (void)hipGetLastError();
    hipLaunchKernelGGL(layernorm_kernel, dim3(car_div_up(M, 4)), dim3(256), 0, (hipStream_t)stream, X, ldx, gamma, beta, C, eps, Y, ldy, M);
    CAR_CHECK_LAUNCH("car_layernorm");
    return CAR_OK;
}

extern "C" int car_gelu(float* Y, int ldy, long M, int N, void* stream) {
    CAR_REQUIRE(Y, "car_gelu: null pointer");
    CAR_REQUIRE(M > 0 && N > 0 && N % 4 == 0 && (M * (N / 4)) / 256 < (1L << 31), "car_gelu: bad sizes (M = %ld, N = %d: N must be a multiple of 4)", M, N);
    CAR_REQUIRE(ldy >= N && ldy % 4 == 0, "car_gelu: the row stride (%d) must hold N = %d and be a multiple of 4", ldy, N);
    CAR_REQUIRE(aligned16(Y), "car_gelu: Y must be 16-byte aligned");
    (void)hipGetLastError();
    hipLaunchKernelGGL(gelu_kernel, dim3(car_div_up(M * (N / 4), 256)), dim3(256), 0, (hipStream_t)stream, Y, ldy, M, N / 4);
    CAR_CHECK_LAUNCH("car_gelu");
    return CAR_OK;
}

extern "C" size_t car_mha_workspace_bytes(int b, int S, int heads) {
    return mha_shape_ok(b, S, heads, "car_mha_workspace_bytes") ? mha_layout(b, S, heads).total : 0;
}

namespace {
// car_mha and car_mha_stats: the same checks, the same three launches; stats (or null) is the only difference
int mha_run(const char* who, const float* qkv, int ld, int b, int S, int heads, float* out, int ldo, float* stats, void* work, size_t work_bytes,
            void* stream) {
    CAR_REQUIRE(qkv && out && work, "%s: null pointer", who);
    if (!mha_shape_ok(b, S, heads, who)) return CAR_E_ARG;
    const int dim = heads * kHead;
    CAR_REQUIRE(ld >= 3 * dim && ld % 4 == 0, "%s: the row stride of qkv (%d) must hold 3 x %d columns and be a multiple of 4", who, ld, dim);
    CAR_REQUIRE(ldo >= dim && ldo % 4 == 0, "%s: the row stride of out (%d) must hold %d columns and be a multiple of 4", who, ldo, dim);
    CAR_REQUIRE(aligned16(qkv) && aligned16(out) && aligned16(work) && aligned16(stats), "%s: qkv, out, stats and work must be 16-byte aligned", who);
    const MhaLayout l = mha_layout(b, S, heads, work);
    CAR_REQUIRE(work_bytes >= l.total, "%s: the workspace is too small (%zu bytes, car_mha_workspace_bytes says %zu)", who, work_bytes, l.total);
    MhaArgs a{qkv, ld, b, S, heads, l.tiles, out, ldo, l.maxes, l.scales, l.packed, stats};
    hipStream_t st = (hipStream_t)stream;
    const unsigned tiles_all = (unsigned)(b * heads * l.tiles);
    (void)hipGetLastError();
    hipLaunchKernelGGL(mha_absmax_kernel, dim3(tiles_all), dim3(256), 0, st, a);
    hipLaunchKernelGGL(mha_pack_kernel, dim3(tiles_all), dim3(256), 0, st, a);
    hipLaunchKernelGGL(mha_kernel, dim3(car_div_up(tiles_all, 4)), dim3(256), 0, st, a);
    CAR_CHECK_LAUNCH(who);
    return CAR_OK;
}
}  // namespace

extern "C" int car_mha(const float* qkv, int ld, int b, int S, int heads, float* out, int ldo, void* work, size_t work_bytes, void* stream) {
    return mha_run("car_mha", qkv, ld, b, S, heads, out, ldo, nullptr, work, work_bytes, stream);
}

extern "C" size_t car_mha_stats_floats(int b, int S, int heads) {
    return mha_shape_ok(b, S, heads, "car_mha_stats_floats") ? (size_t)b * heads * S * 2 : 0;
}

extern "C" int car_mha_stats(const float* qkv, int ld, int b, int S, int heads, float* out, int ldo, float* stats, void* work, size_t work_bytes,
                             void* stream) {
    CAR_REQUIRE(stats, "car_mha_stats: null pointer");
    return mha_run("car_mha_stats", qkv, ld, b, S, heads, out, ldo, stats, work, work_bytes, stream);
}

extern "C" size_t car_vit_packed_offset(int dim, int item) {
    if (!vit_dim_ok(dim, "car_vit_packed_offset")) return 0;
    if (item < 0 || item > 12) { car_set_error("car_vit_packed_offset: item %d is outside 0..12", item); return 0; }
    return vit_layout(dim).off[item];
}

extern "C" size_t car_vit_packed_floats(int dim, int depth) {
    if (!vit_dim_ok(dim, "car_vit_packed_floats")) return 0;
    if (depth < 1 || depth > 32) { car_set_error("car_vit_packed_floats: depth = %d is outside 1..32", depth); return 0; }
    return vit_layout(dim).off[12] * (size_t)depth;
}

extern "C" int car_vit_pack(const float* const* params, int n_params, int dim, int depth, float* packed, void* stream) {
    CAR_REQUIRE(params && packed, "car_vit_pack: null pointer");
    if (!vit_dim_ok(dim, "car_vit_pack")) return CAR_E_ARG;
    CAR_REQUIRE(depth >= 1 && depth <= 32, "car_vit_pack: depth = %d is outside 1..32", depth);
    CAR_REQUIRE(n_params == 12 * depth, "car_vit_pack: %d parameter arrays do not fit depth %d (12 per block)", n_params, depth);
    for (int i = 0; i < n_params; ++i) CAR_REQUIRE(params[i], "car_vit_pack: null pointer (parameter %d)", i);
    CAR_REQUIRE(aligned16(packed), "car_vit_pack: packed must be 16-byte aligned");
    const VitLayout l = vit_layout(dim);
    hipStream_t st = (hipStream_t)stream;
    const int mk[12] = {0, 0, dim, 0, dim, 0, 0, 0, dim, 0, 4 * dim, 0};                // a matrix's K (0: a vector)
    const int mn[12] = {dim, dim, 3 * dim, 3 * dim, dim, dim, dim, dim, 4 * dim, 4 * dim, dim, dim};
    for (int blk = 0; blk < depth; ++blk) {
        float* base = packed + (size_t)blk * l.off[12];
        for (int i = 0; i < 12; ++i) {
            const float* src = params[blk * 12 + i];
            if (mk[i]) CAR_TRY(car_linear_x3_pack(src, mk[i], mk[i], mn[i], base + l.off[i], stream));
            else CAR_CHECK_HIP(hipMemcpyAsync(base + l.off[i], src, sizeof(float) * mn[i], hipMemcpyDeviceToDevice, st), "car_vit_pack: copy failed");
        }
    }
    return CAR_OK;
}

extern "C" size_t car_vit_workspace_bytes(int b, int S, int dim) {
    if (!vit_dim_ok(dim, "car_vit_workspace_bytes") || !mha_shape_ok(b, S, dim / kHead, "car_vit_workspace_bytes")) return 0;
    return vit_work(b, S, dim).total;
}

namespace {
// car_vit_blocks and car_vit_blocks_train: the same checks and the same sequence of entries on the same strides; with `saved` the
// intermediates the backward reads are written where it will find them (vit_saved) instead of into the workspace's maps
int vit_run(const char* who, float* tok, int b, int S, int dim, const float* packed, int depth, const int* taps, int n_taps, float* const* tap_out,
            void* saved, size_t saved_bytes, bool train, void* work, size_t work_bytes, void* stream) {
    CAR_REQUIRE(tok && packed && work && (n_taps == 0 || (taps && tap_out)) && (!train || saved), "%s: null pointer", who);
    if (!vit_dim_ok(dim, who) || !mha_shape_ok(b, S, dim / kHead, who) || !vit_depth_ok(depth, who)) return CAR_E_ARG;
    CAR_REQUIRE(n_taps >= 0 && n_taps <= depth, "%s: %d taps for %d blocks", who, n_taps, depth);
    for (int i = 0; i < n_taps; ++i) {
        CAR_REQUIRE(taps[i] >= 0 && taps[i] < depth && (i == 0 || taps[i] > taps[i - 1]),
                    "%s: taps must be strictly increasing block indices below depth = %d (tap %d is %d)", who, depth, i, taps[i]);
        CAR_REQUIRE(tap_out[i], "%s: null pointer (tap_out %d)", who, i);
        CAR_REQUIRE(aligned16(tap_out[i]), "%s: tap_out %d must be 16-byte aligned", who, i);
    }
    CAR_REQUIRE(aligned16(tok) && aligned16(packed) && aligned16(work) && aligned16(saved), "%s: tok, packed, saved and work must be 16-byte aligned", who);
    const VitWork w = vit_work(b, S, dim, work);
    CAR_REQUIRE(work_bytes >= w.total, "%s: the workspace is too small (%zu bytes, car_vit_workspace_bytes says %zu)", who, work_bytes, w.total);
    if (train) {
        const size_t need = vit_saved(b, S, dim, depth).total;
        CAR_REQUIRE(saved_bytes >= need, "%s: the saved buffer is too small (%zu bytes, car_vit_saved_bytes says %zu)", who, saved_bytes, need);
    }
    const VitLayout l = vit_layout(dim);
    const long rows = (long)b * S;
    const size_t map = sizeof(float) * rows * dim;
    const int heads = dim / kHead;
    hipStream_t st = (hipStream_t)stream;
    int next_tap = 0;
    for (int blk = 0; blk < depth; ++blk) {
        const float* p = packed + (size_t)blk * l.off[12];
        const VitSaved sv = train ? vit_saved(b, S, dim, depth, blk, saved) : VitSaved{};
        float *norm = w.norm, *att = train ? sv.att : w.att, *qkv = train ? sv.qkv : w.wide, *wide = w.wide;
        if (train) CAR_CHECK_HIP(hipMemcpyAsync(sv.x0, tok, map, hipMemcpyDeviceToDevice, st), "%s: copy failed", who);
        CAR_TRY(car_layernorm(tok, dim, p + l.off[0], p + l.off[1], dim, 1e-6, norm, dim, rows, stream));
        CAR_TRY(car_linear_x3(norm, dim, p + l.off[2], p + l.off[3], dim, 3 * dim, qkv, 3 * dim, rows, 0, stream));
        if (train) CAR_TRY(car_mha_stats(qkv, 3 * dim, b, S, heads, att, dim, sv.stats, w.mha, w.mha_bytes, stream));
        else CAR_TRY(car_mha(qkv, 3 * dim, b, S, heads, att, dim, w.mha, w.mha_bytes, stream));
        CAR_TRY(car_linear_x3(att, dim, p + l.off[4], p + l.off[5], dim, dim, tok, dim, rows, CAR_LIN_ACCUM, stream));
        if (train) CAR_CHECK_HIP(hipMemcpyAsync(sv.x1, tok, map, hipMemcpyDeviceToDevice, st), "%s: copy failed", who);
        CAR_TRY(car_layernorm(tok, dim, p + l.off[6], p + l.off[7], dim, 1e-6, norm, dim, rows, stream));
        if (train) {                                                    // the pre-activation stays; GELU runs on a copy
            CAR_TRY(car_linear_x3(norm, dim, p + l.off[8], p + l.off[9], dim, 4 * dim, sv.u, 4 * dim, rows, 0, stream));
            CAR_CHECK_HIP(hipMemcpyAsync(wide, sv.u, 4 * map, hipMemcpyDeviceToDevice, st), "%s: copy failed", who);
        } else {
            CAR_TRY(car_linear_x3(norm, dim, p + l.off[8], p + l.off[9], dim, 4 * dim, wide, 4 * dim, rows, 0, stream));
        }
        CAR_TRY(car_gelu(wide, 4 * dim, rows, 4 * dim, stream));
        CAR_TRY(car_linear_x3(wide, 4 * dim, p + l.off[10], p + l.off[11], 4 * dim, dim, tok, dim, rows, CAR_LIN_ACCUM, stream));
        if (next_tap < n_taps && taps[next_tap] == blk) {
            CAR_CHECK_HIP(hipMemcpyAsync(tap_out[next_tap], tok, map, hipMemcpyDeviceToDevice, st), "%s: copy failed", who);
            ++next_tap;
        }
    }
    return CAR_OK;
}
}  // namespace

extern "C" int car_vit_blocks(float* tok, int b, int S, int dim, const float* packed, int depth, const int* taps, int n_taps, float* const* tap_out,
                              void* work, size_t work_bytes, void* stream) {
    return vit_run("car_vit_blocks", tok, b, S, dim, packed, depth, taps, n_taps, tap_out, nullptr, 0, false, work, work_bytes, stream);
}

extern "C" size_t car_vit_saved_bytes(int b, int S, int dim, int depth) {
    const char* who = "car_vit_saved_bytes";
    if (!vit_dim_ok(dim, who) || !mha_shape_ok(b, S, dim / kHead, who) || !vit_depth_ok(depth, who)) return 0;
    return vit_saved(b, S, dim, depth).total;
}

extern "C" int car_vit_blocks_train(float* tok, int b, int S, int dim, const float* packed, int depth, const int* taps, int n_taps,
                                    float* const* tap_out, void* saved, size_t saved_bytes, void* work, size_t work_bytes, void* stream) {
    return vit_run("car_vit_blocks_train", tok, b, S, dim, packed, depth, taps, n_taps, tap_out, saved, saved_bytes, true, work, work_bytes, stream);
}

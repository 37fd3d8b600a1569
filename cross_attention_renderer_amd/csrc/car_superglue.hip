// car_superglue.hip — SuperGlue's forward for the unposed pair (estimate_pose/superglue.py:51-285).
//
// Every layer of the network is a 1 x 1 convolution over at most 1024 keypoints per image: a car_linear call on channel-last rows (fp32
// matrix pipe, bias folded into the pack).  Both images' rows lie in one array, image 0's N0 rows first, and share every launch whose
// weights they share.  What is new here:
//   pack       every eval-mode BatchNorm1d folded into the convolution in front of it (fp64: s = gamma / sqrt(var + 1e-5), W' = s W,
//              b' = (b - mean) s + beta, rounded once); the three projections of a layer packed as ONE 256 -> 768 layer (q | k | v).
//              HEAD PERMUTATION: MultiHeadedAttention splits channels by view(b, 64, 4, n), so head h owns the torch channels h, h + 4,
//              h + 8, ...; the projections' rows and merge's columns are permuted at pack time (device channel h * 64 + d = torch channel
//              d * 4 + h) so that a head is 64 contiguous floats here.
//   attention  softmax(q k^T / 8) v for 4 heads of 64: one workgroup per query row, one wave per head, the logits of the row in LDS, the
//              maximum subtracted, fp32 accumulation in a fixed order (dot products by ascending channel, sums by ascending key per
//              lane and the fixed butterfly across lanes).
//   transport  the (m + 1) x (n + 1) couplings with bin_score on the dustbin row and column; one launch per half-iteration, one wave
//              per row (or column), the log-sum-exp in fp64 in a fixed order.  No workgroup waits for another.
//   matches    row and column arg-max over Z[:-1, :-1] (ties to the lowest index), the mutual check, exp(max), the threshold.
#include "car_common.h"
#include <math.h>
#include <stdint.h>

namespace {

constexpr int kD = 256, kHeads = 4, kHeadDim = 64;
constexpr int kMaxKeypoints = 1024, kMaxLayers = 64;
constexpr int kKenc[6] = {3, 32, 64, 128, 256, 256};
constexpr int kKencParams = 26, kLayerParams = 16;
constexpr size_t kScratch = 512 * 512 + 512;                  // the widest folded layer and its bias

// slots of the packed array: 0..4 the keypoint encoder, then per layer qkv | merge | mlp0 | mlp3, then final_proj, then the scratch
struct Slot { int K, N; };
Slot slot_of(int layers, int s) {
    if (s < 5) return {kKenc[s], kKenc[s + 1]};
    s -= 5;
    if (s < 4 * layers) {
        constexpr Slot kLayer[4] = {{256, 768}, {256, 256}, {512, 512}, {512, 256}};
        return kLayer[s % 4];
    }
    return {256, 256};
}
size_t slot_offset(int layers, int s) {
    size_t off = 0;
    for (int i = 0; i < s; ++i) {
        const Slot t = slot_of(layers, i);
        off += car_linear_packed_floats(t.K, t.N);
    }
    return off;
}
int n_slots(int layers) { return 5 + 4 * layers + 1; }

// ---- pack: BatchNorm fold and head permutation, fp64, rounded once ---------------------------------------------------------------------
struct PrepArgs {
    const float *W, *b, *gamma, *beta, *mean, *var;          // gamma null: no BatchNorm behind the layer
    int N, K, row_perm, col_perm;
    float *outW, *outb;
};
__device__ __forceinline__ int head_major(int c) { return (c % kHeadDim) * kHeads + c / kHeadDim; }      // device channel -> torch channel
__global__ void __launch_bounds__(256) prep_kernel(const PrepArgs a) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)a.N * (a.K + 1)) return;
    const int ro = (int)(idx / (a.K + 1)), co = (int)(idx % (a.K + 1));
    const int r = a.row_perm ? head_major(ro) : ro;
    const double s = a.gamma ? (double)a.gamma[r] / sqrt((double)a.var[r] + 1e-5) : 1.0;
    if (co < a.K) {
        const int c = a.col_perm ? head_major(co) : co;
        a.outW[(long)ro * a.K + co] = (float)((double)a.W[(long)r * a.K + c] * s);
    } else {
        a.outb[ro] = a.gamma ? (float)(((double)a.b[r] - (double)a.mean[r]) * s + (double)a.beta[r]) : a.b[r];
    }
}
int prep(const float* const* p, bool bn, int N, int K, int row_perm, int col_perm, float* outW, float* outb, hipStream_t st) {
    PrepArgs a;
    a.W = p[0]; a.b = p[1];
    a.gamma = bn ? p[2] : nullptr; a.beta = bn ? p[3] : nullptr; a.mean = bn ? p[4] : nullptr; a.var = bn ? p[5] : nullptr;
    a.N = N; a.K = K; a.row_perm = row_perm; a.col_perm = col_perm; a.outW = outW; a.outb = outb;
    hipLaunchKernelGGL(prep_kernel, dim3(car_div_up((long)N * (K + 1), 256)), dim3(256), 0, st, a);
    CAR_CHECK_LAUNCH("car_superglue_pack");
    return CAR_OK;
}

// ---- the rows' start: normalize_keypoints and the copy of the descriptors into the [rows, 512] buffer ---------------------------------
// kin [rows, 4] = ((x - W / 2) / (0.7 max(W, H)), (y - H / 2) / (0.7 max(W, H)), score, 0); cat[:, 0:256] = desc
__global__ void __launch_bounds__(256) rows_kernel(const float* __restrict__ kpts, const float* __restrict__ scores, const float* __restrict__ desc, int N,
                                                   float cx, float cy, float scale, float* __restrict__ kin, float* __restrict__ cat) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= N) return;
    if (lane == 0) reinterpret_cast<float4*>(kin)[r] = make_float4((kpts[2 * r] - cx) / scale, (kpts[2 * r + 1] - cy) / scale, scores[r], 0.0f);
    reinterpret_cast<float4*>(cat + (long)r * 512)[lane] = reinterpret_cast<const float4*>(desc + (long)r * kD)[lane];
}

// ---- attention: one workgroup per query row, one wave per head ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) attention_kernel(const float* __restrict__ q, int ldq, const float* __restrict__ k, int ldk,
                                                        const float* __restrict__ v, int ldv, int M, float* __restrict__ out, int ldo) {
    __shared__ float sq[kD];
    __shared__ float logit[kHeads][kMaxKeypoints];
    const int lane = threadIdx.x & 63, h = threadIdx.x >> 6;
    const long row = blockIdx.x;
    sq[threadIdx.x] = q[row * ldq + threadIdx.x];
    __syncthreads();
    const float* qh = sq + h * kHeadDim;
    float mx = -INFINITY;
    for (int m = lane; m < M; m += 64) {
        const float4* kr = reinterpret_cast<const float4*>(k + (long)m * ldk + h * kHeadDim);
        float acc = 0.0f;
#pragma unroll
        for (int d = 0; d < kHeadDim / 4; ++d) {
            const float4 t = kr[d];
            acc = fmaf(qh[4 * d], t.x, acc);
            acc = fmaf(qh[4 * d + 1], t.y, acc);
            acc = fmaf(qh[4 * d + 2], t.z, acc);
            acc = fmaf(qh[4 * d + 3], t.w, acc);
        }
        acc *= 0.125f;
        logit[h][m] = acc;
        mx = fmaxf(mx, acc);
    }
    mx = wave_max(mx);
    float sum = 0.0f;
    for (int m = lane; m < M; m += 64) {
        const float e = expf(logit[h][m] - mx);
        logit[h][m] = e;
        sum += e;
    }
    sum = wave_sum(sum);
    __syncthreads();                                  // the wave's own writes to logit[h] are read across lanes below
    float acc = 0.0f;
    const float* vh = v + h * kHeadDim + lane;
    for (int m = 0; m < M; ++m) acc = fmaf(logit[h][m], vh[(long)m * ldv], acc);
    out[row * ldo + h * kHeadDim + lane] = acc / sum;
}

// ---- the couplings: S = mdesc0 mdesc1^T / 16 with bin_score on the dustbin row and column ------------------------------------------------
__global__ void __launch_bounds__(256) couplings_kernel(const float* __restrict__ d0, const float* __restrict__ d1, int m, int n, float bin,
                                                        float* __restrict__ Zc) {
    __shared__ float sq[kD];
    const int i = blockIdx.x;                          // 0..m
    float* row = Zc + (long)i * (n + 1);
    if (i == m) {
        for (int j = threadIdx.x; j <= n; j += 256) row[j] = bin;
        return;
    }
    sq[threadIdx.x] = d0[(long)i * kD + threadIdx.x];
    __syncthreads();
    for (int j = threadIdx.x; j <= n; j += 256) {
        if (j == n) { row[j] = bin; continue; }
        const float4* r = reinterpret_cast<const float4*>(d1 + (long)j * kD);
        float acc = 0.0f;
#pragma unroll 8
        for (int d = 0; d < kD / 4; ++d) {
            const float4 t = r[d];
            acc = fmaf(sq[4 * d], t.x, acc);
            acc = fmaf(sq[4 * d + 1], t.y, acc);
            acc = fmaf(sq[4 * d + 2], t.z, acc);
            acc = fmaf(sq[4 * d + 3], t.w, acc);
        }
        row[j] = acc / 16.0f;
    }
}
// one half-iteration: out[l] = log_marginal(l) - logsumexp_e(Z[l, e] + add[e]), one wave per line l; fp64, lane-strided then the butterfly.
// stride_l / stride_e: rows (n + 1, 1) or columns (1, n + 1) of the couplings.
__global__ void __launch_bounds__(256) sinkhorn_kernel(const float* __restrict__ Zc, int lines, int len, long stride_l, long stride_e,
                                                       const double* __restrict__ add, double lm, double lm_last, double* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int l = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (l >= lines) return;
    const float* z = Zc + l * stride_l;
    double mx = -INFINITY;
    for (int e = lane; e < len; e += 64) mx = fmax(mx, (double)z[e * stride_e] + add[e]);
    mx = wave_max(mx);
    double sum = 0.0;
    for (int e = lane; e < len; e += 64) sum += exp((double)z[e * stride_e] + add[e] - mx);
    sum = wave_sum(sum);
    if (lane == 0) out[l] = (l == lines - 1 ? lm_last : lm) - (mx + log(sum));
}
__global__ void __launch_bounds__(256) transport_out_kernel(const float* __restrict__ Zc, const double* __restrict__ u, const double* __restrict__ v,
                                                            double norm, int rows, int cols, float* __restrict__ Z) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)rows * cols) return;
    Z[idx] = (float)((double)Zc[idx] + u[idx / cols] + v[idx % cols] - norm);
}

// ---- matches -------------------------------------------------------------------------------------------------------------------------------
// arg-max of every line over its first `len` entries, ties to the lowest index: one wave per line
__global__ void __launch_bounds__(256) argmax_kernel(const float* __restrict__ Z, int lines, int len, long stride_l, long stride_e, float* __restrict__ best,
                                                     int* __restrict__ at) {
    const int lane = threadIdx.x & 63;
    const int l = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (l >= lines) return;
    const float* z = Z + l * stride_l;
    float b = -INFINITY;
    int bi = 0x7fffffff;
    for (int e = lane; e < len; e += 64) {
        const float t = z[e * stride_e];
        if (bi == 0x7fffffff || t > b) { b = t; bi = e; }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(b, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (oi != 0x7fffffff && (bi == 0x7fffffff || ob > b || (ob == b && oi < bi))) { b = ob; bi = oi; }
    }
    if (lane == 0) { best[l] = b; at[l] = bi; }
}
__global__ void __launch_bounds__(256) decide_kernel(const float* __restrict__ max0, const int* __restrict__ idx0, const int* __restrict__ idx1, int m, int n,
                                                     float thr, int* __restrict__ m0, int* __restrict__ m1, float* __restrict__ s0, float* __restrict__ s1) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < m) {
        const bool mutual = idx1[idx0[t]] == t;
        const float s = mutual ? (float)exp((double)max0[t]) : 0.0f;
        s0[t] = s;
        m0[t] = mutual && s > thr ? idx0[t] : -1;
    } else if (t < m + n) {
        const int j = t - m, i = idx1[j];
        const bool mutual1 = idx0[i] == j;                                       // then idx1[idx0[i]] == i too: i's own check holds
        const float s = mutual1 ? (float)exp((double)max0[i]) : 0.0f;
        s1[j] = s;
        m1[j] = mutual1 && s > thr ? i : -1;
    }
}

// car_superglue_descriptors' workspace, per row of both images: the [x | message] buffer (512), q | k | v (768), the attention's output
// (256), the hidden layer (512), the encoder's input (4)
struct DescWork { float *cat, *qkv, *att, *hid, *kin; size_t bytes; };
DescWork desc_work(int N0, int N1, void* work = nullptr) {
    const size_t R = (size_t)N0 + N1;
    Carver c(work);
    return {c.take<float>(R * 512), c.take<float>(R * 768), c.take<float>(R * 256), c.take<float>(R * 512), c.take<float>(R * 4), c.bytes()};
}
// car_superglue_transport's: the couplings (fp32), then u and v (fp64, cleared in one go: everything from u on), each of whole 64 elements
struct TransportWork { float* Zc; double *u, *v; size_t bytes; };
TransportWork transport_work(int m, int n, void* work = nullptr) {
    Carver c(work, 64);
    return {c.take<float>((size_t)(m + 1) * (n + 1)), c.take<double>(m + 1), c.take<double>(n + 1), c.bytes()};
}
// car_superglue_matches': max0 [N0] floats, then idx0 [N0] and idx1 [N1] ints, then max1 [N1] floats
struct MatchWork { float* max0; int *idx0, *idx1; float* max1; size_t bytes; };
MatchWork match_work(int N0, int N1, void* work = nullptr) {
    Carver c(work);
    return {c.take<float>(N0), c.take<int>(N0), c.take<int>(N1), c.take<float>(N1), c.bytes()};
}

bool pair_ok(int N0, int N1, const char* who) {
    if (N0 >= 1 && N1 >= 1 && N0 <= kMaxKeypoints && N1 <= kMaxKeypoints) return true;
    car_set_error("%s: %d and %d keypoints, need 1..%d of each", who, N0, N1, kMaxKeypoints);
    return false;
}

}  // namespace

extern "C" size_t car_superglue_packed_floats(int layers) {
    if (layers < 1 || layers > kMaxLayers) {
        car_set_error("car_superglue_packed_floats: %d layers, need 1..%d", layers, kMaxLayers);
        return 0;
    }
    return slot_offset(layers, n_slots(layers)) + kScratch;
}

extern "C" int car_superglue_pack(const float* const* params, int n_params, int layers, float* packed, void* stream) {
    CAR_REQUIRE(params && packed, "car_superglue_pack: null pointer");
    CAR_REQUIRE(layers >= 1 && layers <= kMaxLayers, "car_superglue_pack: %d layers, need 1..%d", layers, kMaxLayers);
    const int want = kKencParams + kLayerParams * layers + 2;
    CAR_REQUIRE(n_params == want, "car_superglue_pack: %d parameter arrays, %d layers need %d", n_params, layers, want);
    for (int i = 0; i < n_params; ++i) CAR_REQUIRE(params[i], "car_superglue_pack: null pointer (parameter %d)", i);
    CAR_REQUIRE(aligned16(packed), "car_superglue_pack: packed must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    float* scratch = packed + slot_offset(layers, n_slots(layers));
    (void)hipGetLastError();
    int s = 0;
    auto emit = [&](int K, int N, const float* bias) { return car_linear_pack(scratch, K, bias, K, N, packed + slot_offset(layers, s++), stream); };
    const float* const* p = params;
    for (int i = 0; i < 5; ++i, p += i < 5 ? 6 : 2) {                            // the keypoint encoder: BatchNorm behind the first four
        const int K = kKenc[i], N = kKenc[i + 1];
        CAR_TRY(prep(p, i < 4, N, K, 0, 0, scratch, scratch + (size_t)N * K, st));
        CAR_TRY(emit(K, N, scratch + (size_t)N * K));
    }
    for (int l = 0; l < layers; ++l, p += kLayerParams) {
        float* bias = scratch + 768 * 256;
        for (int j = 0; j < 3; ++j) CAR_TRY(prep(p + 2 * j, false, 256, 256, 1, 0, scratch + (size_t)j * 256 * 256, bias + j * 256, st));
        CAR_TRY(emit(256, 768, bias));                                            // q | k | v, rows head-major
        CAR_TRY(prep(p + 6, false, 256, 256, 0, 1, scratch, scratch + 256 * 256, st));
        CAR_TRY(emit(256, 256, scratch + 256 * 256));                             // merge, columns head-major
        CAR_TRY(prep(p + 8, true, 512, 512, 0, 0, scratch, scratch + 512 * 512, st));
        CAR_TRY(emit(512, 512, scratch + 512 * 512));                             // mlp.0 with mlp.1 folded in
        CAR_TRY(prep(p + 14, false, 256, 512, 0, 0, scratch, scratch + 256 * 512, st));
        CAR_TRY(emit(512, 256, scratch + 256 * 512));                             // mlp.3
    }
    CAR_TRY(prep(p, false, 256, 256, 0, 0, scratch, scratch + 256 * 256, st));
    CAR_TRY(emit(256, 256, scratch + 256 * 256));                                 // final_proj
    return CAR_OK;
}

extern "C" int car_superglue_attention(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, int N, int M, float* out, int ldo,
                                       void* stream) {
    CAR_REQUIRE(q && k && v && out, "car_superglue_attention: null pointer");
    CAR_REQUIRE(N >= 1 && N <= kMaxKeypoints && M >= 1 && M <= kMaxKeypoints, "car_superglue_attention: %d queries against %d keys, need 1..%d of each", N, M,
                kMaxKeypoints);
    CAR_REQUIRE(ldq >= kD && ldo >= kD && ldk >= kD && ldv >= kD && ldk % 4 == 0, "car_superglue_attention: row strides %d %d %d %d, need >= 256 (keys: a multiple of 4)",
                ldq, ldk, ldv, ldo);
    CAR_REQUIRE(aligned16(k), "car_superglue_attention: the keys must be 16-byte aligned");
    (void)hipGetLastError();
    hipLaunchKernelGGL(attention_kernel, dim3((unsigned)N), dim3(256), 0, (hipStream_t)stream, q, ldq, k, ldk, v, ldv, M, out, ldo);
    CAR_CHECK_LAUNCH("car_superglue_attention");
    return CAR_OK;
}

extern "C" size_t car_superglue_workspace_bytes(int N0, int N1) {
    return pair_ok(N0, N1, "car_superglue_workspace_bytes") ? desc_work(N0, N1).bytes : 0;
}

extern "C" int car_superglue_descriptors(const float* kpts0, const float* scores0, const float* desc0, int N0, int H0, int W0, const float* kpts1,
                                         const float* scores1, const float* desc1, int N1, int H1, int W1, const float* packed, int layers,
                                         const int* cross, float* mdesc, void* work, size_t work_bytes, void* stream) {
    CAR_REQUIRE(kpts0 && scores0 && desc0 && kpts1 && scores1 && desc1 && packed && cross && mdesc && work, "car_superglue_descriptors: null pointer");
    CAR_REQUIRE(layers >= 1 && layers <= kMaxLayers, "car_superglue_descriptors: %d layers, need 1..%d", layers, kMaxLayers);
    CAR_REQUIRE(N0 >= 1 && N1 >= 1 && N0 <= kMaxKeypoints && N1 <= kMaxKeypoints, "car_superglue_descriptors: %d and %d keypoints, need 1..%d of each", N0, N1,
                kMaxKeypoints);
    CAR_REQUIRE(H0 >= 1 && W0 >= 1 && H1 >= 1 && W1 >= 1, "car_superglue_descriptors: image shapes %d x %d and %d x %d", H0, W0, H1, W1);
    const size_t need = car_superglue_workspace_bytes(N0, N1);
    CAR_REQUIRE(work_bytes >= need, "car_superglue_descriptors: workspace holds %zu bytes, need %zu (car_superglue_workspace_bytes)", work_bytes, need);
    CAR_REQUIRE(aligned16(packed) && aligned16(work) && aligned16(mdesc) && aligned16(desc0) && aligned16(desc1),
                "car_superglue_descriptors: packed, the descriptors, mdesc and the workspace must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const long R = N0 + N1;
    const auto [cat, qkv, att, hid, kin, work_end] = desc_work(N0, N1, work);      // [R, 512]: x | message, [R, 768], [R, 256], [R, 512], [R, 4]
    (void)hipGetLastError();
    const float s0 = 0.7f * (float)(W0 > H0 ? W0 : H0), s1 = 0.7f * (float)(W1 > H1 ? W1 : H1);
    hipLaunchKernelGGL(rows_kernel, dim3(car_div_up(N0, 4)), dim3(256), 0, st, kpts0, scores0, desc0, N0, W0 / 2.0f, H0 / 2.0f, s0, kin, cat);
    CAR_CHECK_LAUNCH("car_superglue_descriptors");
    hipLaunchKernelGGL(rows_kernel, dim3(car_div_up(N1, 4)), dim3(256), 0, st, kpts1, scores1, desc1, N1, W1 / 2.0f, H1 / 2.0f, s1, kin + (long)N0 * 4,
                       cat + (long)N0 * 512);
    CAR_CHECK_LAUNCH("car_superglue_descriptors");
    auto W = [&](int s) { return packed + slot_offset(layers, s); };
    // the keypoint encoder: 3 -> 32 -> 64 -> 128 -> 256 -> 256, the last layer added onto the descriptors
    CAR_TRY(car_linear(kin, 4, W(0), 3, 32, qkv, 32, R, CAR_LIN_RELU_OUT, stream));
    CAR_TRY(car_linear(qkv, 32, W(1), 32, 64, hid, 64, R, CAR_LIN_RELU_OUT, stream));
    CAR_TRY(car_linear(hid, 64, W(2), 64, 128, qkv, 128, R, CAR_LIN_RELU_OUT, stream));
    CAR_TRY(car_linear(qkv, 128, W(3), 128, 256, hid, 256, R, CAR_LIN_RELU_OUT, stream));
    CAR_TRY(car_linear(hid, 256, W(4), 256, 256, cat, 512, R, CAR_LIN_ACCUM, stream));
    for (int l = 0; l < layers; ++l) {
        const int s = 5 + 4 * l;
        CAR_TRY(car_linear(cat, 512, W(s), 256, 768, qkv, 768, R, 0, stream));
        const float* src0 = cross[l] ? qkv + (long)N0 * 768 : qkv;               // the rows image 0 attends to
        const float* src1 = cross[l] ? qkv : qkv + (long)N0 * 768;
        CAR_TRY(car_superglue_attention(qkv, 768, src0 + 256, 768, src0 + 512, 768, N0, cross[l] ? N1 : N0, att, 256, stream));
        CAR_TRY(car_superglue_attention(qkv + (long)N0 * 768, 768, src1 + 256, 768, src1 + 512, 768, N1, cross[l] ? N0 : N1, att + (long)N0 * 256, 256, stream));
        CAR_TRY(car_linear(att, 256, W(s + 1), 256, 256, cat + 256, 512, R, 0, stream));                 // message = merge(...), beside x
        CAR_TRY(car_linear(cat, 512, W(s + 2), 512, 512, hid, 512, R, CAR_LIN_RELU_OUT, stream));
        CAR_TRY(car_linear(hid, 512, W(s + 3), 512, 256, cat, 512, R, CAR_LIN_ACCUM, stream));           // x += delta
    }
    CAR_TRY(car_linear(cat, 512, W(5 + 4 * layers), 256, 256, mdesc, 256, R, 0, stream));
    return CAR_OK;
}

extern "C" size_t car_superglue_transport_workspace_bytes(int N0, int N1) {
    return pair_ok(N0, N1, "car_superglue_transport_workspace_bytes") ? transport_work(N0, N1).bytes : 0;
}

extern "C" int car_superglue_transport(const float* mdesc0, int N0, const float* mdesc1, int N1, float bin_score, int iters, float* Z, void* work,
                                       size_t work_bytes, void* stream) {
    CAR_REQUIRE(mdesc0 && mdesc1 && Z && work, "car_superglue_transport: null pointer");
    CAR_REQUIRE(N0 >= 1 && N1 >= 1 && N0 <= kMaxKeypoints && N1 <= kMaxKeypoints, "car_superglue_transport: %d and %d keypoints, need 1..%d of each", N0, N1,
                kMaxKeypoints);
    CAR_REQUIRE(iters >= 0 && iters <= 1000, "car_superglue_transport: %d iterations, need 0..1000", iters);
    CAR_REQUIRE(bin_score == bin_score, "car_superglue_transport: bin_score is NaN");
    const size_t need = car_superglue_transport_workspace_bytes(N0, N1);
    CAR_REQUIRE(work_bytes >= need, "car_superglue_transport: workspace holds %zu bytes, need %zu (car_superglue_transport_workspace_bytes)", work_bytes, need);
    CAR_REQUIRE(aligned16(mdesc0) && aligned16(mdesc1) && aligned16(work), "car_superglue_transport: mdesc0, mdesc1 and the workspace must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int m = N0, n = N1;
    const auto [Zc, u, v, work_end] = transport_work(m, n, work);
    (void)hipGetLastError();
    CAR_CHECK_HIP(hipMemsetAsync(u, 0, work_end - ((char*)u - (char*)work), st), "car_superglue_transport: memset failed");
    hipLaunchKernelGGL(couplings_kernel, dim3((unsigned)(m + 1)), dim3(256), 0, st, mdesc0, mdesc1, m, n, bin_score, Zc);
    CAR_CHECK_LAUNCH("car_superglue_transport");
    const double norm = -log((double)m + (double)n), lmu_last = log((double)n) + norm, lnu_last = log((double)m) + norm;
    for (int it = 0; it < iters; ++it) {
        hipLaunchKernelGGL(sinkhorn_kernel, dim3(car_div_up(m + 1, 4)), dim3(256), 0, st, Zc, m + 1, n + 1, (long)(n + 1), 1L, v, norm, lmu_last, u);
        CAR_CHECK_LAUNCH("car_superglue_transport");
        hipLaunchKernelGGL(sinkhorn_kernel, dim3(car_div_up(n + 1, 4)), dim3(256), 0, st, Zc, n + 1, m + 1, 1L, (long)(n + 1), u, norm, lnu_last, v);
        CAR_CHECK_LAUNCH("car_superglue_transport");
    }
    hipLaunchKernelGGL(transport_out_kernel, dim3(car_div_up((long)(m + 1) * (n + 1), 256)), dim3(256), 0, st, Zc, u, v, norm, m + 1, n + 1, Z);
    CAR_CHECK_LAUNCH("car_superglue_transport");
    return CAR_OK;
}

extern "C" size_t car_superglue_matches_workspace_bytes(int N0, int N1) {
    return pair_ok(N0, N1, "car_superglue_matches_workspace_bytes") ? match_work(N0, N1).bytes : 0;
}

extern "C" int car_superglue_matches(const float* Z, int N0, int N1, float match_threshold, int* matches0, int* matches1, float* scores0, float* scores1,
                                     void* work, size_t work_bytes, void* stream) {
    CAR_REQUIRE(Z && matches0 && matches1 && scores0 && scores1 && work, "car_superglue_matches: null pointer");
    CAR_REQUIRE(N0 >= 1 && N1 >= 1 && N0 <= kMaxKeypoints && N1 <= kMaxKeypoints, "car_superglue_matches: %d and %d keypoints, need 1..%d of each", N0, N1,
                kMaxKeypoints);
    CAR_REQUIRE(match_threshold == match_threshold, "car_superglue_matches: the threshold is NaN");
    const size_t need = car_superglue_matches_workspace_bytes(N0, N1);
    CAR_REQUIRE(work_bytes >= need, "car_superglue_matches: workspace holds %zu bytes, need %zu (car_superglue_matches_workspace_bytes)", work_bytes, need);
    CAR_REQUIRE(((uintptr_t)work & 3) == 0, "car_superglue_matches: the workspace must be 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const auto [max0, idx0, idx1, max1, work_end] = match_work(N0, N1, work);
    (void)hipGetLastError();
    hipLaunchKernelGGL(argmax_kernel, dim3(car_div_up(N0, 4)), dim3(256), 0, st, Z, N0, N1, (long)(N1 + 1), 1L, max0, idx0);
    CAR_CHECK_LAUNCH("car_superglue_matches");
    hipLaunchKernelGGL(argmax_kernel, dim3(car_div_up(N1, 4)), dim3(256), 0, st, Z, N1, N0, 1L, (long)(N1 + 1), max1, idx1);
    CAR_CHECK_LAUNCH("car_superglue_matches");
    hipLaunchKernelGGL(decide_kernel, dim3(car_div_up(N0 + N1, 256)), dim3(256), 0, st, max0, idx0, idx1, N0, N1, match_threshold, matches0, matches1, scores0,
                       scores1);
    CAR_CHECK_LAUNCH("car_superglue_matches");
    return CAR_OK;
}

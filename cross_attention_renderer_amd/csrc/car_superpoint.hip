// car_superpoint.hip — SuperPoint's forward for the unposed pair (estimate_pose/superpoint.py:47-202).
//
// Stages, each an entry of include/car_match.h:
//   dense    conv1a (1 -> 64, the fp32 vector kernel below), then the nine 64 / 128 / 256 layers and three pools through car_conv3x3 /
//            car_maxpool2x2 (csrc/car_lpips.hip, csrc/car_conv.hip: split fp16 on the matrix pipe, ReLU in the store), the two 1 x 1 heads through
//            car_linear (fp32 matrix pipe, bias folded into the pack, no ReLU); softmax over the 65 channels of a cell with the dustbin
//            dropped and the other 64 laid out as the cell's 8 x 8 pixels; descriptors x / max(|x|, 1e-12).
//   nms      simple_nms: the (2r+1)^2 maximum with the window clipped at the edges (-inf padding), two suppress-and-recover passes.
//            Comparisons of fp32 values only, so the result has the reference's bits.
//   select   score > threshold, at least `border` from every edge, the max_keypoints largest when more survive.  One workgroup per image:
//            tiled prefix sums compact the candidates in row-major order, a four-pass radix selection on the ordered bit pattern of the
//            score finds the cut, the survivors are ranked among themselves.  Integer counters only; nothing depends on the schedule.
//   sample   sample_descriptors: bilinear, align_corners = True, zero padding, then L2 normalisation; one wave per keypoint.
// Everything is channel-last; a descriptor set is [N, 256] where the reference holds [256, N].
#include "car_common.h"
#include <math.h>
#include <stdint.h>

namespace {

constexpr int kConvs = 12;                           // conv1a 1b 2a 2b 3a 3b 4a 4b Pa Pb Da Db, the reference's declaration order
constexpr int kFirstFloats = 9 * 64 + 64;            // conv1a: [tap][64] weights, then the bias
constexpr long kMaxPixels = 1L << 22;                // n H W: every offset of the [n, H, W, 64] maps stays inside 32 bits
constexpr int kMaxKeypoints = 4096;
constexpr int kLogitLd = 68;                         // the 65 logits of a cell, rows 16-byte aligned
constexpr int kDesc = 256;
struct Layer { int K, N; };                          // the 3 x 3 layers behind conv1a, in pack order
constexpr Layer kLayer[9] = {{64, 64}, {64, 64}, {64, 64}, {64, 128}, {128, 128}, {128, 128}, {128, 128}, {128, 256}, {128, 256}};
constexpr int kLayerConv[9] = {1, 2, 3, 4, 5, 6, 7, 8, 10};       // their index among the twelve convolutions

bool shape_ok(int n, int H, int W) {
    return n >= 1 && H >= 8 && W >= 8 && H % 8 == 0 && W % 8 == 0 && (double)n * H * W <= (double)kMaxPixels;
}
bool map_ok(int n, int H, int W) { return n >= 1 && H >= 1 && W >= 1 && (double)n * H * W <= (double)kMaxPixels; }

size_t layer_offset(int l) {                         // of 3 x 3 layer l (9: convPb, 10: convDb, 11: the end) inside the packed array
    size_t off = kFirstFloats;
    for (int i = 0; i < l && i < 9; ++i) off += car_conv3x3_packed_floats(kLayer[i].K, kLayer[i].N);
    if (l >= 10) off += car_linear_packed_floats(256, 65);
    if (l >= 11) off += car_linear_packed_floats(256, 256);
    return off;
}

// ---- conv1a: 1 -> 64, zero padding, ReLU, fp32 ----------------------------------------------------------------------------------------
// a wave = the 64 output channels of one pixel at a time (the pixel is wave-uniform), 16 pixels per wave; taps in row-major order
constexpr int kFirstPix = 16;
__global__ void first_pack_kernel(const float* __restrict__ Wt, const float* __restrict__ bias, float* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < 9 * 64) out[i] = Wt[(i % 64) * 9 + i / 64];
    else if (i < kFirstFloats) out[i] = bias[i - 9 * 64];
}
__global__ void __launch_bounds__(256) conv1a_kernel(const float* __restrict__ X, const float* __restrict__ packed, float* __restrict__ Y, int H, int W,
                                                     long M) {
    const int c = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    float w[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) w[t] = packed[t * 64 + c];
    const float b = packed[9 * 64 + c];
    const long p0 = ((long)blockIdx.x * 4 + wave) * kFirstPix;
    for (int i = 0; i < kFirstPix; ++i) {
        const long p = p0 + i;
        if (p >= M) return;
        const int pix = (int)(p % ((long)H * W)), py = pix / W, px = pix % W;
        float acc = b;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int yy = py + t / 3 - 1, xx = px + t % 3 - 1;
            if ((unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W) acc = fmaf(X[p + (long)(t / 3 - 1) * W + (t % 3 - 1)], w[t], acc);
        }
        Y[p * 64 + c] = fmaxf(acc, 0.0f);
    }
}

// ---- the two heads' closing arithmetic: one wave per feature cell --------------------------------------------------------------------
// scores: softmax over the cell's 65 logits (maximum subtracted), lane c keeps channel c = pixel (c / 8, c % 8) of the cell, the dustbin
// only enters the sum
__global__ void __launch_bounds__(256) score_kernel(const float* __restrict__ logits, float* __restrict__ scores, int h, int w, long cells) {
    const int lane = threadIdx.x & 63;
    const long cell = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (cell >= cells) return;
    const float* row = logits + cell * kLogitLd;
    const float v = row[lane], bin = row[64];
    const float m = fmaxf(wave_max(v), bin);
    const float e = expf(v - m);
    const float sum = wave_sum(e) + expf(bin - m);
    const int cx = (int)(cell % w), cy = (int)((cell / w) % h);
    const long img = cell / ((long)w * h);
    scores[(img * h * 8 + cy * 8 + lane / 8) * ((long)w * 8) + cx * 8 + lane % 8] = e / sum;
}
// descriptors: x / max(|x|, 1e-12) over the 256 channels of a row, four per lane
__device__ __forceinline__ float4 normalised(float4 v) {
    const float n = sqrtf(wave_sum(v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w));
    const float d = fmaxf(n, 1e-12f);
    return make_float4(v.x / d, v.y / d, v.z / d, v.w / d);
}
__global__ void __launch_bounds__(256) normalise_kernel(const float* __restrict__ X, float* __restrict__ Y, long rows) {
    const int lane = threadIdx.x & 63;
    const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    reinterpret_cast<float4*>(Y + r * kDesc)[lane] = normalised(reinterpret_cast<const float4*>(X + r * kDesc)[lane]);
}

// ---- simple_nms: a thread per pixel, the window clipped to the image -------------------------------------------------------------------
__device__ __forceinline__ float window_max(const float* __restrict__ s, int H, int W, int y, int x, int r) {
    const int y0 = max(y - r, 0), y1 = min(y + r, H - 1), x0 = max(x - r, 0), x1 = min(x + r, W - 1);
    float m = -INFINITY;
    for (int yy = y0; yy <= y1; ++yy)
        for (int xx = x0; xx <= x1; ++xx) m = fmaxf(m, s[(long)yy * W + xx]);
    return m;
}
// mask = s == max(s)
__global__ void __launch_bounds__(256) nms_first_kernel(const float* __restrict__ s, float* __restrict__ mask, int H, int W, int r, long total) {
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= total) return;
    const long hw = (long)H * W, img = p / hw;
    const int pix = (int)(p % hw);
    mask[p] = s[p] == window_max(s + img * hw, H, W, pix / W, pix % W, r) ? 1.0f : 0.0f;
}
// supp = max(mask) > 0, ss = supp ? 0 : s
__global__ void __launch_bounds__(256) nms_suppress_kernel(const float* __restrict__ s, const float* __restrict__ mask, float* __restrict__ supp,
                                                           float* __restrict__ ss, int H, int W, int r, long total) {
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= total) return;
    const long hw = (long)H * W, img = p / hw;
    const int pix = (int)(p % hw);
    const bool on = window_max(mask + img * hw, H, W, pix / W, pix % W, r) > 0.0f;
    supp[p] = on ? 1.0f : 0.0f;
    ss[p] = on ? 0.0f : s[p];
}
// mask |= (ss == max(ss)) & !supp; with `out`, the last pass: out = mask ? s : 0
__global__ void __launch_bounds__(256) nms_recover_kernel(const float* __restrict__ s, const float* __restrict__ supp, const float* __restrict__ ss,
                                                          float* __restrict__ mask, float* __restrict__ out, int H, int W, int r, long total) {
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= total) return;
    const long hw = (long)H * W, img = p / hw;
    const int pix = (int)(p % hw);
    const bool fresh = ss[p] == window_max(ss + img * hw, H, W, pix / W, pix % W, r) && !(supp[p] > 0.0f);
    const bool on = mask[p] > 0.0f || fresh;
    if (out) out[p] = on ? s[p] : 0.0f;
    else mask[p] = on ? 1.0f : 0.0f;
}

// ---- selection: one workgroup of 1024 per image ----------------------------------------------------------------------------------------
constexpr int kSelThreads = 1024;
// exclusive prefix sum of v over the workgroup in thread order, and the total; every thread calls it
__device__ __forceinline__ int block_scan(int v, int* sh, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    __syncthreads();                                  // the previous call's readers are done with sh
    if (lane == 63) sh[wave] = inc;
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < kSelThreads / 64; ++k) {
        const int x = sh[k];
        if (k < wave) base += x;
        tot += x;
    }
    total = tot;
    return base + inc - v;
}
// a key that orders as the score does (-0 and +0 being one value)
__device__ __forceinline__ unsigned score_key(float s) {
    if (s == 0.0f) s = 0.0f;
    const unsigned u = __float_as_uint(s);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__global__ void __launch_bounds__(kSelThreads) select_kernel(const float* __restrict__ nms, int H, int W, float thr, int border, int maxk,
                                                             int* __restrict__ cand, float* __restrict__ kpts, float* __restrict__ scores,
                                                             int* __restrict__ count) {
    __shared__ int sh[kSelThreads / 64];
    __shared__ int hist[256];
    __shared__ int pick[2];
    __shared__ int sel_idx[kMaxKeypoints];
    __shared__ unsigned sel_key[kMaxKeypoints];
    const int tid = threadIdx.x, HW = H * W;
    const float* s = nms + (long)blockIdx.x * HW;
    int* cd = cand + (long)blockIdx.x * HW;
    float* kp = kpts + (long)blockIdx.x * maxk * 2;
    float* sc = scores + (long)blockIdx.x * maxk;

    int C = 0;                                        // the candidates, row-major
    for (int t0 = 0; t0 < HW; t0 += kSelThreads) {
        const int p = t0 + tid;
        int flag = 0;
        if (p < HW) {
            const int y = p / W, x = p % W;
            flag = s[p] > thr && y >= border && y < H - border && x >= border && x < W - border;
        }
        int total;
        const int at = block_scan(flag, sh, total);
        if (flag) cd[C + at] = p;
        C += total;
    }
    __syncthreads();                                  // cd is read by other threads from here on
    if (C <= maxk) {
        for (int i = tid; i < C; i += kSelThreads) {
            const int p = cd[i];
            kp[2 * i] = (float)(p % W);
            kp[2 * i + 1] = (float)(p / W);
            sc[i] = s[p];
        }
        if (tid == 0) count[blockIdx.x] = C;
        return;
    }

    unsigned prefix = 0, mask = 0;                    // the maxk-th largest key, eight bits at a time from the top
    int need = maxk;
    for (int shift = 24; shift >= 0; shift -= 8) {
        if (tid < 256) hist[tid] = 0;
        __syncthreads();
        for (int i = tid; i < C; i += kSelThreads) {
            const unsigned k = score_key(s[cd[i]]);
            if ((k & mask) == prefix) atomicAdd(&hist[(k >> shift) & 255], 1);
        }
        __syncthreads();
        if (tid == 0) {
            int above = 0, b = 255;
            for (; b > 0 && above + hist[b] < need; --b) above += hist[b];
            pick[0] = b;
            pick[1] = need - above;
        }
        __syncthreads();
        prefix |= (unsigned)pick[0] << shift;
        mask |= 255u << shift;
        need = pick[1];
        __syncthreads();
    }

    int n_sel = 0, n_tie = 0;                         // every key above the cut, and the first `need` of the keys on it
    for (int t0 = 0; t0 < C; t0 += kSelThreads) {
        const int i = t0 + tid;
        int p = 0, gt = 0, eq = 0;
        unsigned k = 0;
        if (i < C) {
            p = cd[i];
            k = score_key(s[p]);
            gt = k > prefix;
            eq = k == prefix;
        }
        int eq_total, total;
        const int eq_at = block_scan(eq, sh, eq_total);
        const int take = gt || (eq && n_tie + eq_at < need);
        const int at = n_sel + block_scan(take, sh, total);
        if (take && at < maxk) {
            sel_idx[at] = p;
            sel_key[at] = k;
        }
        n_sel += total;
        n_tie += eq_total;
    }
    __syncthreads();
    for (int j = tid; j < maxk; j += kSelThreads) {    // descending score, equal scores in row-major order
        const unsigned kj = sel_key[j];
        int rank = 0;
        for (int i = 0; i < maxk; ++i) {
            const unsigned ki = sel_key[i];
            rank += ki > kj || (ki == kj && i < j);
        }
        const int p = sel_idx[j];
        kp[2 * rank] = (float)(p % W);
        kp[2 * rank + 1] = (float)(p / W);
        sc[rank] = s[p];
    }
    if (tid == 0) count[blockIdx.x] = maxk;
}

// ---- sample_descriptors: one wave per keypoint -----------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) sample_kernel(const float* __restrict__ kpts, int N, const float* __restrict__ desc, int h, int w,
                                                     float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= N) return;
    // (k - s / 2 + 0.5) / (w s - s / 2 - 0.5) to [-1, 1], then grid_sample's align_corners = True pixel coordinate
    const float gx = (kpts[2 * k] - 4.0f + 0.5f) / ((float)(w * 8) - 4.0f - 0.5f) * 2.0f - 1.0f;
    const float gy = (kpts[2 * k + 1] - 4.0f + 0.5f) / ((float)(h * 8) - 4.0f - 0.5f) * 2.0f - 1.0f;
    const float ix = (gx + 1.0f) / 2.0f * (float)(w - 1), iy = (gy + 1.0f) / 2.0f * (float)(h - 1);
    float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (isfinite(ix) && isfinite(iy) && ix > -2.0f && iy > -2.0f && ix < (float)w + 1.0f && iy < (float)h + 1.0f) {
        const float fx = floorf(ix), fy = floorf(iy);
        const int x0 = (int)fx, y0 = (int)fy;
        const float wx1 = ix - fx, wx0 = (fx + 1.0f) - ix, wy1 = iy - fy, wy0 = (fy + 1.0f) - iy;
        const float wt[4] = {wx0 * wy0, wx1 * wy0, wx0 * wy1, wx1 * wy1};        // nw, ne, sw, se
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int xx = x0 + (t & 1), yy = y0 + (t >> 1);
            if ((unsigned)xx < (unsigned)w && (unsigned)yy < (unsigned)h) {
                const float4 v = reinterpret_cast<const float4*>(desc + ((long)yy * w + xx) * kDesc)[lane];
                acc.x = fmaf(v.x, wt[t], acc.x);
                acc.y = fmaf(v.y, wt[t], acc.y);
                acc.z = fmaf(v.z, wt[t], acc.z);
                acc.w = fmaf(v.w, wt[t], acc.w);
            }
        }
    }
    reinterpret_cast<float4*>(out + (long)k * kDesc)[lane] = normalised(acc);
}

int conv1a(const float* gray, int n, int H, int W, const float* packed, float* Y, hipStream_t st, const char* who) {
    const long M = (long)n * H * W;
    hipLaunchKernelGGL(conv1a_kernel, dim3(car_div_up(M, 4 * kFirstPix)), dim3(256), 0, st, gray, packed, Y, H, W, M);
    CAR_CHECK_LAUNCH(who);
    return CAR_OK;
}

// car_superpoint_dense's workspace: two [n, H, W, 64] maps A and B that the layers alternate between.  The ten moves up to conv4b leave
// x in A, so the heads' [cells, 256] hidden map and the 1 x 1 layer's rows behind it (kLogitLd = 68 wide, or 256 channels) take B:
// a range of its own, whose capacity ok says they fit
struct DenseWork { float *A, *B, *rows; size_t bytes; bool ok; };      // head is B's own start
DenseWork dense_work(int n, int H, int W, void* work = nullptr) {
    const size_t map = (size_t)n * H * W * 64, cells = (size_t)n * (H / 8) * (W / 8);
    Carver c(work);
    float* A = c.take<float>(map);
    Carver inB = c.sub(map * sizeof(float));
    return {A, inB.take<float>(cells * 256), inB.take<float>(cells * 256), c.bytes(), inB.ok()};
}
// car_superpoint_nms': the mask, the suppression mask and the suppressed scores
struct NmsWork { float *mask, *supp, *ss; size_t bytes; };
NmsWork nms_work(size_t total, void* work = nullptr) {
    Carver c(work);
    return {c.take<float>(total), c.take<float>(total), c.take<float>(total), c.bytes()};
}

}  // namespace

extern "C" size_t car_superpoint_packed_floats(void) { return layer_offset(11); }

extern "C" int car_superpoint_pack(const float* const* conv_w, const float* const* conv_b, float* packed, void* stream) {
    CAR_REQUIRE(conv_w && conv_b && packed, "car_superpoint_pack: null pointer");
    for (int l = 0; l < kConvs; ++l) CAR_REQUIRE(conv_w[l] && conv_b[l], "car_superpoint_pack: null pointer (convolution %d)", l);
    CAR_REQUIRE(aligned16(packed), "car_superpoint_pack: packed must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    (void)hipGetLastError();
    hipLaunchKernelGGL(first_pack_kernel, dim3(car_div_up(kFirstFloats, 256)), dim3(256), 0, st, conv_w[0], conv_b[0], packed);
    CAR_CHECK_LAUNCH("car_superpoint_pack");
    for (int l = 0; l < 9; ++l) {
        const int c = kLayerConv[l];
        CAR_TRY(car_conv3x3_pack(conv_w[c], conv_b[c], kLayer[l].K, kLayer[l].N, packed + layer_offset(l), stream));
    }
    CAR_TRY(car_linear_pack(conv_w[9], 256, conv_b[9], 256, 65, packed + layer_offset(9), stream));
    CAR_TRY(car_linear_pack(conv_w[11], 256, conv_b[11], 256, 256, packed + layer_offset(10), stream));
    return CAR_OK;
}

extern "C" int car_superpoint_conv1a(const float* gray, int n, int H, int W, const float* packed, float* Y, void* stream) {
    CAR_REQUIRE(gray && packed && Y, "car_superpoint_conv1a: null pointer");
    CAR_REQUIRE(map_ok(n, H, W), "car_superpoint_conv1a: %d images of %d x %d, need at least one pixel and at most 2^22", n, H, W);
    (void)hipGetLastError();
    return conv1a(gray, n, H, W, packed, Y, (hipStream_t)stream, "car_superpoint_conv1a");
}

extern "C" size_t car_superpoint_workspace_bytes(int n, int H, int W) {
    if (!shape_ok(n, H, W)) {
        car_set_error("car_superpoint_workspace_bytes: %d images of %d x %d, need H and W multiples of 8, at least 8, and n H W <= 2^22", n, H, W);
        return 0;
    }
    return dense_work(n, H, W).bytes;
}

extern "C" int car_superpoint_dense(const float* gray, int n, int H, int W, const float* packed, float* scores, float* desc, void* work,
                                    size_t work_bytes, void* stream) {
    CAR_REQUIRE(gray && packed && scores && desc && work, "car_superpoint_dense: null pointer");
    CAR_REQUIRE(shape_ok(n, H, W), "car_superpoint_dense: %d images of %d x %d, need H and W multiples of 8, at least 8, and n H W <= 2^22", n, H, W);
    const size_t need = car_superpoint_workspace_bytes(n, H, W);
    CAR_REQUIRE(work_bytes >= need, "car_superpoint_dense: workspace holds %zu bytes, need %zu (car_superpoint_workspace_bytes)", work_bytes, need);
    CAR_REQUIRE(aligned16(packed) && aligned16(work) && aligned16(desc), "car_superpoint_dense: packed, desc and the workspace must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const DenseWork dw = dense_work(n, H, W, work);
    CAR_REQUIRE(dw.ok, "car_superpoint_dense: the heads' maps do not fit the second map of the workspace");
    (void)hipGetLastError();
    CAR_TRY(conv1a(gray, n, H, W, packed, dw.A, st, "car_superpoint_dense"));
    float *src = dw.A, *dst = dw.B;
    int h = H, w = W, l = 0;
    auto conv = [&]() {                              // layer l: src -> dst, then the two change places
        const int rc = car_conv3x3(src, n, h, w, kLayer[l].K, kLayer[l].N, packed + layer_offset(l), dst, stream);
        float* t = src; src = dst; dst = t;
        ++l;
        return rc;
    };
    auto pool = [&](int C) {
        const int rc = car_maxpool2x2(src, n, h, w, C, dst, stream);
        float* t = src; src = dst; dst = t;
        h /= 2; w /= 2;
        return rc;
    };
    CAR_TRY(conv());                                 // conv1b
    CAR_TRY(pool(64));
    CAR_TRY(conv());                                 // conv2a
    CAR_TRY(conv());                                 // conv2b
    CAR_TRY(pool(64));
    CAR_TRY(conv());                                 // conv3a
    CAR_TRY(conv());                                 // conv3b
    CAR_TRY(pool(128));
    CAR_TRY(conv());                                 // conv4a
    CAR_TRY(conv());                                 // conv4b: x [n, h, w, 128] in src
    const long cells = (long)n * h * w;
    float *head = dw.B, *rows = dw.rows;             // [cells, 256] and the 1 x 1 layer's rows behind it, in B, which is dst here
    CAR_TRY(car_conv3x3(src, n, h, w, 128, 256, packed + layer_offset(7), head, stream));                    // convPa
    CAR_TRY(car_linear(head, 256, packed + layer_offset(9), 256, 65, rows, kLogitLd, cells, 0, stream));     // convPb
    hipLaunchKernelGGL(score_kernel, dim3(car_div_up(cells, 4)), dim3(256), 0, st, rows, scores, h, w, cells);
    CAR_CHECK_LAUNCH("car_superpoint_dense");
    CAR_TRY(car_conv3x3(src, n, h, w, 128, 256, packed + layer_offset(8), head, stream));                    // convDa
    CAR_TRY(car_linear(head, 256, packed + layer_offset(10), 256, 256, rows, 256, cells, 0, stream));        // convDb
    hipLaunchKernelGGL(normalise_kernel, dim3(car_div_up(cells, 4)), dim3(256), 0, st, rows, desc, cells);
    CAR_CHECK_LAUNCH("car_superpoint_dense");
    return CAR_OK;
}

extern "C" size_t car_superpoint_nms_workspace_bytes(int n, int H, int W) {
    if (!map_ok(n, H, W)) {
        car_set_error("car_superpoint_nms_workspace_bytes: %d maps of %d x %d, need at least one pixel and at most 2^22", n, H, W);
        return 0;
    }
    return nms_work((size_t)n * H * W).bytes;
}

extern "C" int car_superpoint_nms(const float* scores, int n, int H, int W, int radius, float* out, void* work, size_t work_bytes, void* stream) {
    CAR_REQUIRE(scores && out && work, "car_superpoint_nms: null pointer");
    CAR_REQUIRE(map_ok(n, H, W), "car_superpoint_nms: %d maps of %d x %d, need at least one pixel and at most 2^22", n, H, W);
    CAR_REQUIRE(radius >= 0 && radius <= 8, "car_superpoint_nms: radius %d, need 0..8", radius);
    CAR_REQUIRE(scores != out, "car_superpoint_nms: out must not be the score map");
    const size_t need = car_superpoint_nms_workspace_bytes(n, H, W);
    CAR_REQUIRE(work_bytes >= need, "car_superpoint_nms: workspace holds %zu bytes, need %zu (car_superpoint_nms_workspace_bytes)", work_bytes, need);
    CAR_REQUIRE(((uintptr_t)work & 3) == 0, "car_superpoint_nms: the workspace must be 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const long total = (long)n * H * W;
    const auto [mask, supp, ss, work_end] = nms_work((size_t)total, work);
    const dim3 grid(car_div_up(total, 256)), block(256);
    (void)hipGetLastError();
    hipLaunchKernelGGL(nms_first_kernel, grid, block, 0, st, scores, mask, H, W, radius, total);
    CAR_CHECK_LAUNCH("car_superpoint_nms");
    for (int pass = 0; pass < 2; ++pass) {
        hipLaunchKernelGGL(nms_suppress_kernel, grid, block, 0, st, scores, mask, supp, ss, H, W, radius, total);
        CAR_CHECK_LAUNCH("car_superpoint_nms");
        hipLaunchKernelGGL(nms_recover_kernel, grid, block, 0, st, scores, supp, ss, mask, pass == 1 ? out : (float*)nullptr, H, W, radius, total);
        CAR_CHECK_LAUNCH("car_superpoint_nms");
    }
    return CAR_OK;
}

extern "C" size_t car_superpoint_select_workspace_bytes(int n, int H, int W) {
    if (!map_ok(n, H, W)) {
        car_set_error("car_superpoint_select_workspace_bytes: %d maps of %d x %d, need at least one pixel and at most 2^22", n, H, W);
        return 0;
    }
    return (size_t)n * H * W * sizeof(int);           // the candidates' pixel indices, row-major
}

extern "C" int car_superpoint_select(const float* nms, int n, int H, int W, float threshold, int border, int max_keypoints, float* kpts,
                                     float* scores, int* count, void* work, size_t work_bytes, void* stream) {
    CAR_REQUIRE(nms && kpts && scores && count && work, "car_superpoint_select: null pointer");
    CAR_REQUIRE(map_ok(n, H, W), "car_superpoint_select: %d maps of %d x %d, need at least one pixel and at most 2^22", n, H, W);
    CAR_REQUIRE(max_keypoints != -1, "car_superpoint_select: max_keypoints = -1 (the reference's \"all\") is not served, name a cap of 1..%d", kMaxKeypoints);
    CAR_REQUIRE(max_keypoints >= 1 && max_keypoints <= kMaxKeypoints, "car_superpoint_select: max_keypoints = %d, need 1..%d", max_keypoints, kMaxKeypoints);
    CAR_REQUIRE(border >= 0, "car_superpoint_select: border %d, need >= 0", border);
    CAR_REQUIRE(threshold == threshold, "car_superpoint_select: the threshold is NaN");
    const size_t need = car_superpoint_select_workspace_bytes(n, H, W);
    CAR_REQUIRE(work_bytes >= need, "car_superpoint_select: workspace holds %zu bytes, need %zu (car_superpoint_select_workspace_bytes)", work_bytes, need);
    CAR_REQUIRE(((uintptr_t)work & 3) == 0, "car_superpoint_select: the workspace must be 4-byte aligned");
    (void)hipGetLastError();
    hipLaunchKernelGGL(select_kernel, dim3((unsigned)n), dim3(kSelThreads), 0, (hipStream_t)stream, nms, H, W, threshold, border, max_keypoints,
                       static_cast<int*>(work), kpts, scores, count);
    CAR_CHECK_LAUNCH("car_superpoint_select");
    return CAR_OK;
}

extern "C" int car_superpoint_sample(const float* kpts, int N, const float* desc, int h, int w, float* out, void* stream) {
    CAR_REQUIRE(kpts && desc && out, "car_superpoint_sample: null pointer");
    CAR_REQUIRE(N >= 1 && N <= kMaxKeypoints, "car_superpoint_sample: %d keypoints, need 1..%d", N, kMaxKeypoints);
    CAR_REQUIRE(map_ok(1, h, w), "car_superpoint_sample: a %d x %d descriptor map, need at least one cell and at most 2^22", h, w);
    CAR_REQUIRE(aligned16(desc) && aligned16(out), "car_superpoint_sample: desc and out must be 16-byte aligned");
    (void)hipGetLastError();
    hipLaunchKernelGGL(sample_kernel, dim3(car_div_up(N, 4)), dim3(256), 0, (hipStream_t)stream, kpts, N, desc, h, w, out);
    CAR_CHECK_LAUNCH("car_superpoint_sample");
    return CAR_OK;
}

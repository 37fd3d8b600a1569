// car_lpips.hip — LPIPS v0.1, net = 'vgg' (include/car_hip.h: car_conv3x3, car_maxpool2x2, car_lpips_head, car_lpips),
// and its gradient with respect to the images for the training loss (car_lpips_forward_train, car_lpips_backward and their stages: the
// second half of this file).
//
// The metric is a fixed network: a per-channel scaling of the [-1, 1] image, the 13 3x3 convolutions of VGG16's `features` (ReLU behind
// each, 2x2 max-pool in front of blocks 2-5), and at the five taps relu1_2 .. relu5_3 the channel-normalised squared difference of the two
// images' features, weighted by a 1x1 layer, averaged over the tap's pixels and summed over the taps.  Weights come from the caller.
//
// The 12 convolutions with K >= 64 and their data gradients are car_conv.hip's conv3x3_kernel in its two LPIPS forms (the row sweep of
// car_row_sweep.h as an implicit GEMM over 9 K), packed by its packer: this unit calls car_conv3x3_lpips and car_conv3x3_pack_tiles.
// The first layer (K = 3) is a plain fp32 vector kernel with the scaling layer folded in: the weights carry 1 / scale at pack time and
// the shift is subtracted from a pixel as it is loaded, so a padded tap stays the exact zero of the scaled image's padding.
// The max-pool is a kernel of its own (profiles/lpips.md).  The head runs in fp64 with every sum in a fixed order.
#include "car_common.h"
#include <math.h>
#include <stdint.h>

namespace {

// ---- the network ---------------------------------------------------------------------------------------------------------------------
constexpr int kLayers = 13, kTaps = 5;
constexpr int kWidth[kLayers] = {64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512};
constexpr int kTapWidth[kTaps] = {64, 128, 256, 512, 512};
constexpr int kLinFloats = 64 + 128 + 256 + 512 + 512;
constexpr bool layer_ends_block(int l) { return l == 1 || l == 3 || l == 6 || l == 9 || l == 12; }
constexpr bool pool_in_front(int l) { return l == 2 || l == 4 || l == 7 || l == 10; }
constexpr int kFirstFloats = 27 * 64 + 64;         // first layer: [tap * 3 + channel][64] weights / scale, then the bias
#define CAR_LPIPS_SHIFT {-0.030f, -0.088f, -0.188f}       // the scaling layer: (v - shift) / scale per channel
#define CAR_LPIPS_SCALE {0.458, 0.448, 0.450}
constexpr long kMaxPixels = 1L << 27;              // 2 B H W: keeps every row count, grid and per-image offset far inside 32 bits

// ---- first layer: 3 -> 64, fp32, scaling layer folded in ---------------------------------------------------------------------------
// a wave = 64 output channels of one pixel at a time (the pixel is wave-uniform: its 27 inputs are scalar loads), 16 pixels per wave
constexpr int kFirstPix = 16;
__global__ void __launch_bounds__(256) conv_first_kernel(const float* __restrict__ X, const float* __restrict__ packed, float* __restrict__ Y,
                                                         int H, int W, long M) {
    constexpr float kShift[3] = CAR_LPIPS_SHIFT;
    const int n = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    float w[27];
#pragma unroll
    for (int k = 0; k < 27; ++k) w[k] = packed[k * 64 + n];
    const float b = packed[27 * 64 + n];
    const long p0 = ((long)blockIdx.x * 4 + wave) * kFirstPix;
    for (int i = 0; i < kFirstPix; ++i) {
        const long p = p0 + i;
        if (p >= M) return;
        const int pix = (int)(p % ((long)H * W)), py = pix / W, px = pix % W;
        float acc = b;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int yy = py + t / 3 - 1, xx = px + t % 3 - 1;
            if ((unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W) {
                const float* v = X + (p + (long)(t / 3 - 1) * W + (t % 3 - 1)) * 3;
#pragma unroll
                for (int c = 0; c < 3; ++c) acc = fmaf(v[c] - kShift[c], w[3 * t + c], acc);
            }
        }
        Y[p * 64 + n] = fmaxf(acc, 0.0f);
    }
}

// ---- 2x2 max-pool, stride 2, floor ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) maxpool_kernel(const float* __restrict__ X, float* __restrict__ Y, int H, int W, int C4, long total) {
    const int Ho = H / 2, Wo = W / 2;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int c = (int)(idx % C4);
        long r = idx / C4;
        const int ox = (int)(r % Wo); r /= Wo;
        const int oy = (int)(r % Ho);
        const long img = r / Ho;
        const float4* src = reinterpret_cast<const float4*>(X) + ((img * H + 2 * oy) * W + 2 * ox) * C4 + c;
        const float4 a = src[0], b = src[C4], d = src[(long)W * C4], e = src[(long)W * C4 + C4];
        reinterpret_cast<float4*>(Y)[idx] = make_float4(fmaxf(fmaxf(a.x, b.x), fmaxf(d.x, e.x)), fmaxf(fmaxf(a.y, b.y), fmaxf(d.y, e.y)),
                                                        fmaxf(fmaxf(a.z, b.z), fmaxf(d.z, e.z)), fmaxf(fmaxf(a.w, b.w), fmaxf(d.w, e.w)));
    }
}

// ---- packing the first layer (the other layers: car_conv3x3_pack_tiles) -------------------------------------------------------------
__global__ void first_pack_kernel(const float* __restrict__ Wt, const float* __restrict__ bias, float* __restrict__ out) {
    constexpr double kScale[3] = CAR_LPIPS_SCALE;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < 27 * 64) {
        const int n = i % 64, k = i / 64, tap = k / 3, c = k % 3;
        out[i] = (float)((double)Wt[(n * 3 + c) * 9 + tap] / kScale[c]);
    } else if (i < kFirstFloats) out[i] = bias[i - 27 * 64];
}

// ---- the head ------------------------------------------------------------------------------------------------------------------------
constexpr int kHeadPix = 64;                       // pixels per workgroup: 4 waves x 16
struct HeadArgs {
    const float* f[kTaps];                         // [2 B, npix, C]: images 0 .. B-1 against images B .. 2 B-1
    const float* lin[kTaps];
    int npix[kTaps], C[kTaps], blk0[kTaps + 1];    // blk0: first workgroup of a tap inside a pair's run of workgroups
    int B;
    double* partial;                               // [B, blk0[5]]
};
__global__ void __launch_bounds__(256) lpips_head_kernel(const HeadArgs a) {
    __shared__ double red[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int per_pair = a.blk0[kTaps];
    const int pair = blockIdx.x / per_pair, blk = blockIdx.x % per_pair;
    int k = 0;
#pragma unroll
    for (int t = 1; t < kTaps; ++t) k += blk >= a.blk0[t] ? 1 : 0;
    const int C = a.C[k], npix = a.npix[k], per = C / 64;
    const int p0 = (blk - a.blk0[k]) * kHeadPix + wave * 16;
    const float* f0 = a.f[k] + (size_t)pair * npix * C;
    const float* f1 = a.f[k] + (size_t)(a.B + pair) * npix * C;
    double w[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) w[j] = j < per ? (double)a.lin[k][lane + 64 * j] : 0.0;
    double acc = 0.0;
    for (int i = 0; i < 16; ++i) {
        const int p = p0 + i;
        if (p >= npix) break;                                          // wave-uniform
        double u[8], v[8], s0 = 0.0, s1 = 0.0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            u[j] = j < per ? (double)f0[(size_t)p * C + lane + 64 * j] : 0.0;
            v[j] = j < per ? (double)f1[(size_t)p * C + lane + 64 * j] : 0.0;
            s0 += u[j] * u[j];
            s1 += v[j] * v[j];
        }
        const double n0 = sqrt(wave_sum(s0)) + 1e-10, n1 = sqrt(wave_sum(s1)) + 1e-10;
        double d = 0.0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const double t = u[j] / n0 - v[j] / n1;
            d += w[j] * (t * t);
        }
        acc += wave_sum(d);
    }
    if (lane == 0) red[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) a.partial[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}
// one wave per pair: lane l adds workgroups l, l + 64, ... of a tap in order, then the fixed butterfly
__global__ void __launch_bounds__(64) lpips_mean_kernel(const HeadArgs a, double* lpips, double* per_tap) {
    const int pair = blockIdx.x, lane = threadIdx.x;
    const double* part = a.partial + (size_t)pair * a.blk0[kTaps];
    double total = 0.0;
    for (int k = 0; k < kTaps; ++k) {
        double s = 0.0;
        for (int b = a.blk0[k] + lane; b < a.blk0[k + 1]; b += 64) s += part[b];
        const double L = wave_sum(s) / (double)a.npix[k];
        if (per_tap && lane == 0) per_tap[pair * kTaps + k] = L;
        total += L;
    }
    if (lane == 0) lpips[pair] = total;
}

bool lpips_shape_ok(int B, int H, int W) {
    return B >= 1 && H >= 16 && W >= 16 && 2.0 * B * H * W <= (double)kMaxPixels;
}
int head_blocks(int H, int W) {
    int n = 0;
    for (int k = 0; k < kTaps; ++k) n += ((H >> k) * (W >> k) + kHeadPix - 1) / kHeadPix;
    return n;
}
bool conv_shape_ok(int K, int N) {
    return (K == 3 && N == 64) || ((K == 64 || K == 128 || K == 256 || K == 512) && (N == 64 || N == 128 || N == 256 || N == 512));
}

// the 13 convolutions and 4 pools over the workspace's buffers: 0..4 the taps, 5 and 6 two scratch maps, -1 the input images.  The
// workspace: those seven maps, each as large as its largest tenant, then the head's partial sums; pieces of whole 64 elements
struct Step { bool pool; int layer, K, N, h, w, src, dst; };
struct Plan { Step step[kLayers + 4]; int steps; float* buf[7]; double* scratch; size_t bytes; };
Plan make_plan(int B, int H, int W, void* work = nullptr) {
    Plan pl{};
    size_t floats[7] = {};
    int cur = -1, h = H, w = W, K = 3, tap = 0;
    auto need = [&](int b, size_t n) { if (floats[b] < n) floats[b] = n; };
    for (int l = 0; l < kLayers; ++l) {
        if (pool_in_front(l)) {
            pl.step[pl.steps++] = Step{true, l, K, K, h, w, cur, 6};
            h /= 2; w /= 2; cur = 6;
            need(6, (size_t)2 * B * h * w * K);
        }
        const int N = kWidth[l], dst = layer_ends_block(l) ? tap++ : (cur == 5 ? 6 : 5);
        pl.step[pl.steps++] = Step{false, l, K, N, h, w, cur, dst};
        need(dst, (size_t)2 * B * h * w * N);
        cur = dst; K = N;
    }
    Carver c(work, 64);
    for (int b = 0; b < 7; ++b) pl.buf[b] = c.take<float>(floats[b]);
    pl.scratch = c.take<double>(car_lpips_head_scratch_doubles(B, H, W));
    pl.bytes = c.bytes();
    return pl;
}
size_t layer_offset(int l) {                                          // of layer l inside car_lpips_pack's array (l = 13: the lin weights)
    size_t off = 0;
    for (int i = 0, K = 3; i < l; K = kWidth[i], ++i) off += car_conv3x3_packed_floats(K, kWidth[i]);
    return off;
}

HeadArgs head_args(const float* const* feats, int B, int H, int W, const float* lin) {
    HeadArgs a{};
    int blk = 0, off = 0;
    for (int k = 0; k < kTaps; ++k) {
        a.f[k] = feats[k];
        a.lin[k] = lin + off;
        off += kTapWidth[k];
        a.npix[k] = (H >> k) * (W >> k);
        a.C[k] = kTapWidth[k];
        a.blk0[k] = blk;
        blk += (a.npix[k] + kHeadPix - 1) / kHeadPix;
    }
    a.blk0[kTaps] = blk;
    a.B = B;
    return a;
}
int head(const float* const* feats, int B, int H, int W, const float* lin, double* lpips, double* per_tap, double* scratch, hipStream_t st,
         const char* who) {
    HeadArgs a = head_args(feats, B, H, W, lin);
    a.partial = scratch;
    hipLaunchKernelGGL(lpips_head_kernel, dim3((unsigned)((long)B * a.blk0[kTaps])), dim3(256), 0, st, a);
    CAR_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(lpips_mean_kernel, dim3((unsigned)B), dim3(64), 0, st, a, lpips, per_tap);
    CAR_CHECK_LAUNCH(who);
    return CAR_OK;
}

int conv(const float* X, int n, int H, int W, int K, int N, const float* packed, float* Y, hipStream_t st) {
    const long M = (long)n * H * W;
    if (K == 3) {
        hipLaunchKernelGGL(conv_first_kernel, dim3(car_div_up(M, 4 * kFirstPix)), dim3(256), 0, st, X, packed, Y, H, W, M);
        CAR_CHECK_LAUNCH("car_conv3x3");
        return CAR_OK;
    }
    return car_conv3x3_lpips(X, packed, nullptr, nullptr, Y, H, W, K, N, M, false, st);
}

int pool(const float* X, int n, int H, int W, int C, float* Y, hipStream_t st) {
    const long total = (long)n * (H / 2) * (W / 2) * (C / 4);
    const long blocks = (total + 255) / 256;
    hipLaunchKernelGGL(maxpool_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, st, X, Y, H, W, C / 4, total);
    CAR_CHECK_LAUNCH("car_maxpool2x2");
    return CAR_OK;
}


// ==== the backward: d LPIPS / d image, weights frozen (profiles/lpips_backward.md) ============================
// Every kernel is gather-form — an output element is written once, by the thread that summed it in a fixed order — so the gradient is
// bit-reproducible and an image's gradient does not depend on where its pair sits in the batch.

// ---- first layer's data gradient: 64 -> 3, fp32 ------------------------------------------------------------------------------------
// gx[p][c] = sum over taps t and channels n of w[t][c][n] / scale[c] * D[p - offset(t)][n], over the taps whose output pixel lies inside
// the image; `packed` is the forward's first-layer array, which already carries 1 / scale.  A wave takes one pixel at a time: lane n
// holds channel n's 27 weights, the nine 64-float rows of D are coalesced loads, the three sums close with the fixed butterfly.
__global__ void __launch_bounds__(256) conv_first_backward_kernel(const float* __restrict__ D, const float* __restrict__ packed, float* __restrict__ gx,
                                                                  int H, int W, long M) {
    const int n = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    float w[27];
#pragma unroll
    for (int k = 0; k < 27; ++k) w[k] = packed[k * 64 + n];
    const long p0 = ((long)blockIdx.x * 4 + wave) * kFirstPix;
    for (int i = 0; i < kFirstPix; ++i) {
        const long p = p0 + i;
        if (p >= M) return;
        const int pix = (int)(p % ((long)H * W)), py = pix / W, px = pix % W;
        float acc[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int yy = py - (t / 3 - 1), xx = px - (t % 3 - 1);
            if ((unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W) {
                const long src = p - ((long)(t / 3 - 1) * W + (t % 3 - 1));
                CAR_BOUNDS_TRAP(src >= 0 && src < M);
                const float d = D[src * 64 + n];
#pragma unroll
                for (int c = 0; c < 3; ++c) acc[c] = fmaf(d, w[3 * t + c], acc[c]);
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] = wave_sum(acc[c]);
        if (n < 3) gx[p * 3 + n] = n == 0 ? acc[0] : n == 1 ? acc[1] : acc[2];
    }
}

// ---- max-pool backward, gather form --------------------------------------------------------------------------------------------------
// out[y][x] = (routed + add) * (act > 0): routed is the pooled gradient T[y / 2][x / 2] where (y, x) is the FIRST maximal element of its
// window in row-major order (torch's rule), else 0; a last odd row or column lies in no window.  Four channels per thread.
__device__ __forceinline__ float route1(float a, float b, float d, float e, int pos, float t) {
    int arg = 0;
    float m = a;
    if (b > m) { m = b; arg = 1; }
    if (d > m) { m = d; arg = 2; }
    if (e > m) { m = e; arg = 3; }
    return arg == pos ? t : 0.0f;
}
__global__ void __launch_bounds__(256) maxpool_backward_kernel(const float* __restrict__ T, const float* __restrict__ act, const float* __restrict__ add,
                                                               float* __restrict__ out, int H, int W, int C4, long total) {
    const int Ho = H / 2, Wo = W / 2;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int c = (int)(idx % C4);
        long r = idx / C4;
        const int x = (int)(r % W); r /= W;
        const int y = (int)(r % H);
        const long img = r / H;
        const float4 own = reinterpret_cast<const float4*>(act)[idx];
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        const int oy = y >> 1, ox = x >> 1;
        if (oy < Ho && ox < Wo) {
            const long win = ((img * H + 2 * oy) * W + 2 * ox) * C4 + c, pooled = ((img * Ho + oy) * Wo + ox) * C4 + c;
            // act holds `total` float4s, T only the pooled map's: total / (H W) = images x C4 of them per pooled pixel
            CAR_BOUNDS_TRAP(win + (long)W * C4 + C4 < total && pooled < total / ((long)H * W) * Ho * Wo);
            const float4* src = reinterpret_cast<const float4*>(act) + win;
            const float4 a = src[0], b = src[C4], d = src[(long)W * C4], e = src[(long)W * C4 + C4];
            const float4 t = reinterpret_cast<const float4*>(T)[pooled];
            const int pos = 2 * (y & 1) + (x & 1);
            v = make_float4(route1(a.x, b.x, d.x, e.x, pos, t.x), route1(a.y, b.y, d.y, e.y, pos, t.y), route1(a.z, b.z, d.z, e.z, pos, t.z),
                            route1(a.w, b.w, d.w, e.w, pos, t.w));
        }
        if (add) {
            const float4 g = reinterpret_cast<const float4*>(add)[idx];
            v.x += g.x; v.y += g.y; v.z += g.z; v.w += g.w;
        }
        reinterpret_cast<float4*>(out)[idx] = make_float4(own.x > 0.0f ? v.x : 0.0f, own.y > 0.0f ? v.y : 0.0f, own.z > 0.0f ? v.z : 0.0f,
                                                          own.w > 0.0f ? v.w : 0.0f);
    }
}
// out = g * (act > 0): the last layer's ReLU, which no convolution's epilogue reaches
__global__ void __launch_bounds__(256) relu_mask_kernel(const float* __restrict__ g, const float* __restrict__ act, float* __restrict__ out, long total4) {
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total4; idx += (long)gridDim.x * blockDim.x) {
        const float4 v = reinterpret_cast<const float4*>(g)[idx], m = reinterpret_cast<const float4*>(act)[idx];
        reinterpret_cast<float4*>(out)[idx] = make_float4(m.x > 0.0f ? v.x : 0.0f, m.y > 0.0f ? v.y : 0.0f, m.z > 0.0f ? v.z : 0.0f, m.w > 0.0f ? v.w : 0.0f);
    }
}

// ---- the head's backward -----------------------------------------------------------------------------------------------------------------
// Per pixel of a tap, in fp64 with the forward head's sums: u = f0 / (n0 + 1e-10), v = f1 / (n1 + 1e-10), q_c = 2 w_c (u_c - v_c),
//   ds / df0_c =  q_c / (n0 + 1e-10) - (sum_j q_j f0_j) f0_c / (n0 (n0 + 1e-10)^2),
//   ds / df1_c = -q_c / (n1 + 1e-10) + (sum_j q_j f1_j) f1_c / (n1 (n1 + 1e-10)^2),
// times the pair's cotangent / npix, stored as fp32.  At n = 0 the norm's derivative is taken as 0.  Identical features give q = 0 exactly.
struct HeadBwdArgs {
    HeadArgs h;                                    // f, lin, npix, C, blk0, B as in the forward; partial unused
    const double* g;                               // [B]
    float* gf0[kTaps];                             // [B, npix, C] per tap, or all nullptr
    float* gf1[kTaps];
};
__global__ void __launch_bounds__(256) lpips_head_backward_kernel(const HeadBwdArgs b) {
    const HeadArgs& a = b.h;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int per_pair = a.blk0[kTaps];
    const int pair = blockIdx.x / per_pair, blk = blockIdx.x % per_pair;
    int k = 0;
#pragma unroll
    for (int t = 1; t < kTaps; ++t) k += blk >= a.blk0[t] ? 1 : 0;
    const int C = a.C[k], npix = a.npix[k], per = C / 64;
    const int p0 = (blk - a.blk0[k]) * kHeadPix + wave * 16;
    const float* f0 = a.f[k] + (size_t)pair * npix * C;
    const float* f1 = a.f[k] + (size_t)(a.B + pair) * npix * C;
    float* o0 = b.gf0[k] ? b.gf0[k] + (size_t)pair * npix * C : nullptr;
    float* o1 = b.gf1[k] ? b.gf1[k] + (size_t)pair * npix * C : nullptr;
    const double cot = b.g[pair] / (double)npix;
    double w[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) w[j] = j < per ? (double)a.lin[k][lane + 64 * j] : 0.0;
    for (int i = 0; i < 16; ++i) {
        const int p = p0 + i;
        if (p >= npix) break;                                          // wave-uniform
        double u[8], v[8], s0 = 0.0, s1 = 0.0;
        // a pixel's row of C floats, inside the pair's map and the pair inside the stack of 2 B images
        CAR_BOUNDS_TRAP(pair < a.B && k < kTaps && (size_t)p * C + lane + 64 * (per - 1) < (size_t)npix * C);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            u[j] = j < per ? (double)f0[(size_t)p * C + lane + 64 * j] : 0.0;
            v[j] = j < per ? (double)f1[(size_t)p * C + lane + 64 * j] : 0.0;
            s0 += u[j] * u[j];
            s1 += v[j] * v[j];
        }
        const double r0 = sqrt(wave_sum(s0)), r1 = sqrt(wave_sum(s1)), n0 = r0 + 1e-10, n1 = r1 + 1e-10;
        double q[8], a0 = 0.0, a1 = 0.0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            q[j] = 2.0 * w[j] * (u[j] / n0 - v[j] / n1);
            a0 += q[j] * u[j];
            a1 += q[j] * v[j];
        }
        const double t0 = wave_sum(a0), t1 = wave_sum(a1);
        const double c0 = r0 > 0.0 ? t0 / (r0 * (n0 * n0)) : 0.0, c1 = r1 > 0.0 ? t1 / (r1 * (n1 * n1)) : 0.0;
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (j < per) {
                if (o0) o0[(size_t)p * C + lane + 64 * j] = (float)((q[j] / n0 - c0 * u[j]) * cot);
                if (o1) o1[(size_t)p * C + lane + 64 * j] = (float)((c1 * v[j] - q[j] / n1) * cot);
            }
    }
}

int head_backward(const float* const* feats, int B, int H, int W, const float* lin, const double* g, float* const* gf0, float* const* gf1,
                  hipStream_t st, const char* who) {
    HeadBwdArgs b;
    b.h = head_args(feats, B, H, W, lin);
    b.g = g;
    for (int k = 0; k < kTaps; ++k) { b.gf0[k] = gf0 ? gf0[k] : nullptr; b.gf1[k] = gf1 ? gf1[k] : nullptr; }
    hipLaunchKernelGGL(lpips_head_backward_kernel, dim3((unsigned)((long)B * b.h.blk0[kTaps])), dim3(256), 0, st, b);
    CAR_CHECK_LAUNCH(who);
    return CAR_OK;
}

// K, N: the FORWARD layer's channel counts; D [n, H, W, N] -> out [n, H, W, K]
int conv_backward(const float* D, int n, int H, int W, int K, int N, const float* packed, const float* act, const float* add, float* out,
                  hipStream_t st) {
    const long M = (long)n * H * W;
    if (K == 3) {
        hipLaunchKernelGGL(conv_first_backward_kernel, dim3(car_div_up(M, 4 * kFirstPix)), dim3(256), 0, st, D, packed, out, H, W, M);
        CAR_CHECK_LAUNCH("car_conv3x3_backward");
        return CAR_OK;
    }
    return car_conv3x3_lpips(D, packed, act, add, out, H, W, N, K, M, true, st);      // the sweep runs N -> K
}
int pool_backward(const float* T, const float* act, const float* add, int n, int H, int W, int C, float* out, hipStream_t st) {
    const long total = (long)n * H * W * (C / 4);
    const long blocks = (total + 255) / 256;
    hipLaunchKernelGGL(maxpool_backward_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, st, T, act, add, out, H, W, C / 4, total);
    CAR_CHECK_LAUNCH("car_maxpool2x2_backward");
    return CAR_OK;
}
bool conv_backward_shape_ok(int K, int N) { return conv_shape_ok(K, N) && K != 3; }
size_t backward_layer_offset(int l) {                                  // of layer l >= 1 inside car_lpips_pack_backward's array
    size_t off = 0;
    for (int i = 1; i < l; ++i) off += car_conv3x3_backward_packed_floats(kWidth[i - 1], kWidth[i]);
    return off;
}

// the training workspace (floats): the 13 retained activation maps [2 B, h, w, C] in layer order, the pooled map in flight, the head's
// partial sums, then what only the backward touches: the five head gradients and two maps the gradient alternates between
struct TrainPlan { size_t act[kLayers]; int h[kLayers], w[kLayers]; size_t pooled, scratch, hg[kTaps], ping[2], floats; };
TrainPlan make_train_plan(int B, int H, int W) {
    TrainPlan tp{};
    Carver c(nullptr, 64);
    size_t pooled = 0;
    int h = H, w = W;
    for (int l = 0; l < kLayers; ++l) {
        if (pool_in_front(l)) {
            h /= 2; w /= 2;
            const size_t n = (size_t)2 * B * h * w * kWidth[l - 1];
            pooled = n > pooled ? n : pooled;
        }
        tp.act[l] = c.at<float>((size_t)2 * B * h * w * kWidth[l]); tp.h[l] = h; tp.w[l] = w;
    }
    tp.pooled = c.at<float>(pooled);
    tp.scratch = c.at<double>(car_lpips_head_scratch_doubles(B, H, W)) * (sizeof(double) / sizeof(float));
    for (int k = 0; k < kTaps; ++k) tp.hg[k] = c.at<float>((size_t)2 * B * (H >> k) * (W >> k) * kTapWidth[k]);
    for (int i = 0; i < 2; ++i) tp.ping[i] = c.at<float>((size_t)2 * B * H * W * 64);
    tp.floats = c.bytes() / sizeof(float);
    return tp;
}
constexpr int kTapLayer[kTaps] = {1, 3, 6, 9, 12};

}  // namespace

// One layer's packed weights: K = 3 (N = 64; the network's first layer, scaling layer folded in) 27 x 64 fp32 weights and the bias;
// otherwise 9 K / 32 x N / 16 tiles of 512 floats, 64 floats of scale, the bias.  0 for a shape car_conv3x3 refuses.
extern "C" size_t car_conv3x3_packed_floats(int K, int N) {
    if (!conv_shape_ok(K, N)) return 0;
    return K == 3 ? (size_t)kFirstFloats : car_conv3x3_tile_floats(K, N) + 64 + (size_t)N;
}

extern "C" int car_conv3x3_pack(const float* w, const float* bias, int K, int N, float* packed, void* stream) {
    CAR_REQUIRE(w && bias && packed, "car_conv3x3_pack: null pointer");
    CAR_REQUIRE(conv_shape_ok(K, N), "car_conv3x3_pack: %d -> %d channels, need 3 -> 64 or K and N among 64, 128, 256, 512", K, N);
    CAR_REQUIRE(aligned16(packed), "car_conv3x3_pack: packed must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    (void)hipGetLastError();
    if (K == 3) {
        hipLaunchKernelGGL(first_pack_kernel, dim3(car_div_up(kFirstFloats, 256)), dim3(256), 0, st, w, bias, packed);
        CAR_CHECK_LAUNCH("car_conv3x3_pack");
        return CAR_OK;
    }
    return car_conv3x3_pack_tiles("car_conv3x3_pack", w, bias, K, N, false, packed, st);
}

extern "C" int car_conv3x3(const float* X, int n, int H, int W, int K, int N, const float* packed, float* Y, void* stream) {
    CAR_REQUIRE(X && packed && Y, "car_conv3x3: null pointer");
    CAR_REQUIRE(conv_shape_ok(K, N), "car_conv3x3: %d -> %d channels, need 3 -> 64 or K and N among 64, 128, 256, 512", K, N);
    CAR_REQUIRE(n >= 1 && H >= 1 && W >= 1, "car_conv3x3: %d images of %d x %d, need at least one pixel", n, H, W);
    CAR_REQUIRE((double)n * H * W <= (double)kMaxPixels, "car_conv3x3: %d x %d x %d is too large", n, H, W);
    CAR_REQUIRE(aligned16(X) && aligned16(packed) && aligned16(Y), "car_conv3x3: X, packed and Y must be 16-byte aligned");
    return conv(X, n, H, W, K, N, packed, Y, (hipStream_t)stream);
}

extern "C" int car_maxpool2x2(const float* X, int n, int H, int W, int C, float* Y, void* stream) {
    CAR_REQUIRE(X && Y, "car_maxpool2x2: null pointer");
    CAR_REQUIRE(n >= 1 && H >= 2 && W >= 2 && C >= 4 && C % 4 == 0, "car_maxpool2x2: %d x %d x %d x %d, need H, W >= 2 and C a multiple of 4", n, H, W, C);
    CAR_REQUIRE((double)n * H * W <= (double)kMaxPixels && C <= 4096, "car_maxpool2x2: %d x %d x %d x %d is too large", n, H, W, C);
    CAR_REQUIRE(aligned16(X) && aligned16(Y), "car_maxpool2x2: X and Y must be 16-byte aligned");
    return pool(X, n, H, W, C, Y, (hipStream_t)stream);
}

extern "C" size_t car_lpips_head_scratch_doubles(int B, int H, int W) {
    return lpips_shape_ok(B, H, W) ? (size_t)B * head_blocks(H, W) : 0;
}

extern "C" int car_lpips_head(const float* const* feats, int B, int H, int W, const float* lin, double* lpips, double* per_tap, double* scratch,
                              size_t scratch_doubles, void* stream) {
    CAR_REQUIRE(feats && lin && lpips && scratch, "car_lpips_head: null pointer");
    for (int k = 0; k < kTaps; ++k) CAR_REQUIRE(feats[k], "car_lpips_head: null pointer (tap %d)", k);
    CAR_REQUIRE(B >= 1, "car_lpips_head: B = %d, need at least one image pair", B);
    CAR_REQUIRE(H >= 16 && W >= 16, "car_lpips_head: %d x %d image, the last tap needs H >= 16 and W >= 16", H, W);
    CAR_REQUIRE(lpips_shape_ok(B, H, W), "car_lpips_head: %d x %d x %d is too large", B, H, W);
    const size_t need = car_lpips_head_scratch_doubles(B, H, W);
    CAR_REQUIRE(scratch_doubles >= need, "car_lpips_head: scratch holds %zu doubles, need %zu (car_lpips_head_scratch_doubles)", scratch_doubles, need);
    (void)hipGetLastError();
    return head(feats, B, H, W, lin, lpips, per_tap, scratch, (hipStream_t)stream, "car_lpips_head");
}

extern "C" size_t car_lpips_packed_floats(void) { return layer_offset(kLayers) + kLinFloats; }

extern "C" int car_lpips_pack(const float* const* conv_w, const float* const* conv_b, const float* const* lin_w, float* packed, void* stream) {
    CAR_REQUIRE(conv_w && conv_b && lin_w && packed, "car_lpips_pack: null pointer");
    for (int l = 0; l < kLayers; ++l) CAR_REQUIRE(conv_w[l] && conv_b[l], "car_lpips_pack: null pointer (layer %d)", l);
    for (int k = 0; k < kTaps; ++k) CAR_REQUIRE(lin_w[k], "car_lpips_pack: null pointer (lin%d)", k);
    CAR_REQUIRE(aligned16(packed), "car_lpips_pack: packed must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    size_t off = 0;
    for (int l = 0, K = 3; l < kLayers; K = kWidth[l], ++l) {
        const int code = car_conv3x3_pack(conv_w[l], conv_b[l], K, kWidth[l], packed + off, stream);
        if (code != CAR_OK) return code;
        off += car_conv3x3_packed_floats(K, kWidth[l]);
    }
    for (int k = 0; k < kTaps; ++k) {
        if (hipMemcpyAsync(packed + off, lin_w[k], kTapWidth[k] * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess) {
            car_set_error("car_lpips_pack: copying lin%d failed: %s", k, hipGetErrorString(hipGetLastError()));
            return CAR_E_LAUNCH;
        }
        off += kTapWidth[k];
    }
    return CAR_OK;
}

extern "C" size_t car_lpips_workspace_bytes(int B, int H, int W) {
    if (!lpips_shape_ok(B, H, W)) return 0;
    return make_plan(B, H, W).bytes;
}

extern "C" int car_lpips(const float* x, const float* y, int B, int H, int W, const float* packed, double* lpips, double* per_tap, void* work,
                         size_t work_bytes, void* stream) {
    CAR_REQUIRE(x && y && packed && lpips && work, "car_lpips: null pointer");
    CAR_REQUIRE(B >= 1, "car_lpips: B = %d, need at least one image pair", B);
    CAR_REQUIRE(H >= 16 && W >= 16, "car_lpips: %d x %d image, the last tap needs H >= 16 and W >= 16", H, W);
    CAR_REQUIRE(lpips_shape_ok(B, H, W), "car_lpips: %d x %d x %d is too large", B, H, W);
    const size_t need = car_lpips_workspace_bytes(B, H, W);
    CAR_REQUIRE(work_bytes >= need, "car_lpips: workspace holds %zu bytes, need %zu (car_lpips_workspace_bytes)", work_bytes, need);
    CAR_REQUIRE(aligned16(packed) && aligned16(work), "car_lpips: packed and the workspace must be 16-byte aligned");

    const Plan pl = make_plan(B, H, W, work);
    float* const* buf = pl.buf;
    hipStream_t st = (hipStream_t)stream;
    (void)hipGetLastError();
    for (int i = 0; i < pl.steps; ++i) {
        const Step& s = pl.step[i];
        int code;
        if (s.pool) code = pool(buf[s.src], 2 * B, s.h, s.w, s.K, buf[s.dst], st);
        else if (s.src < 0) {                                           // the two image stacks become one batch of 2 B here
            code = conv(x, B, H, W, 3, 64, packed, buf[s.dst], st);
            if (code == CAR_OK) code = conv(y, B, H, W, 3, 64, packed, buf[s.dst] + (size_t)B * H * W * 64, st);
        } else code = conv(buf[s.src], 2 * B, s.h, s.w, s.K, s.N, packed + layer_offset(s.layer), buf[s.dst], st);
        if (code != CAR_OK) return code;
    }
    return head(buf, B, H, W, packed + layer_offset(kLayers), lpips, per_tap, pl.scratch, st, "car_lpips");
}

// ---- the backward's entries (include/car_hip.h) ------------------------------------------------------------------------------------------
// K, N are the FORWARD layer's channel counts throughout.  The data gradient's weights: 9 N / 32 x K / 16 tiles and 64 floats of scale;
// 0 for a refused shape and for the first layer, whose data gradient reads car_conv3x3_pack's array.
extern "C" size_t car_conv3x3_backward_packed_floats(int K, int N) {
    return conv_backward_shape_ok(K, N) ? car_conv3x3_tile_floats(N, K) + 64 : 0;
}

extern "C" int car_conv3x3_backward_pack(const float* w, int K, int N, float* packed, void* stream) {
    CAR_REQUIRE(w && packed, "car_conv3x3_backward_pack: null pointer");
    CAR_REQUIRE(conv_backward_shape_ok(K, N), "car_conv3x3_backward_pack: %d -> %d channels, need K and N among 64, 128, 256, 512", K, N);
    CAR_REQUIRE(aligned16(packed), "car_conv3x3_backward_pack: packed must be 16-byte aligned");
    return car_conv3x3_pack_tiles("car_conv3x3_backward_pack", w, nullptr, N, K, true, packed, (hipStream_t)stream);
}

extern "C" int car_conv3x3_backward(const float* D, int n, int H, int W, int K, int N, const float* packed, const float* act, const float* add,
                                    float* out, void* stream) {
    CAR_REQUIRE(D && packed && out, "car_conv3x3_backward: null pointer");
    CAR_REQUIRE(conv_shape_ok(K, N), "car_conv3x3_backward: %d -> %d channels, need 3 -> 64 or K and N among 64, 128, 256, 512", K, N);
    CAR_REQUIRE(K != 3 || (!act && !add), "car_conv3x3_backward: the first layer's gradient lands on the image: act and add must be NULL");
    CAR_REQUIRE(n >= 1 && H >= 1 && W >= 1, "car_conv3x3_backward: %d images of %d x %d, need at least one pixel", n, H, W);
    CAR_REQUIRE((double)n * H * W <= (double)kMaxPixels, "car_conv3x3_backward: %d x %d x %d is too large", n, H, W);
    CAR_REQUIRE(aligned16(D) && aligned16(packed) && aligned16(out) && aligned16(act) && aligned16(add),
                "car_conv3x3_backward: D, packed, act, add and out must be 16-byte aligned");
    (void)hipGetLastError();
    return conv_backward(D, n, H, W, K, N, packed, act, add, out, (hipStream_t)stream);
}

extern "C" int car_maxpool2x2_backward(const float* T, const float* act, const float* add, int n, int H, int W, int C, float* out, void* stream) {
    CAR_REQUIRE(T && act && out, "car_maxpool2x2_backward: null pointer");
    CAR_REQUIRE(n >= 1 && H >= 2 && W >= 2 && C >= 4 && C % 4 == 0, "car_maxpool2x2_backward: %d x %d x %d x %d, need H, W >= 2 and C a multiple of 4", n, H, W, C);
    CAR_REQUIRE((double)n * H * W <= (double)kMaxPixels && C <= 4096, "car_maxpool2x2_backward: %d x %d x %d x %d is too large", n, H, W, C);
    CAR_REQUIRE(aligned16(T) && aligned16(act) && aligned16(add) && aligned16(out), "car_maxpool2x2_backward: T, act, add and out must be 16-byte aligned");
    (void)hipGetLastError();
    return pool_backward(T, act, add, n, H, W, C, out, (hipStream_t)stream);
}

extern "C" int car_lpips_head_backward(const float* const* feats, int B, int H, int W, const float* lin, const double* g, float* const* gf0,
                                       float* const* gf1, void* stream) {
    CAR_REQUIRE(feats && lin && g, "car_lpips_head_backward: null pointer");
    CAR_REQUIRE(gf0 || gf1, "car_lpips_head_backward: null pointer (neither gf0 nor gf1 is given)");
    for (int k = 0; k < kTaps; ++k)
        CAR_REQUIRE(feats[k] && (!gf0 || gf0[k]) && (!gf1 || gf1[k]), "car_lpips_head_backward: null pointer (tap %d)", k);
    CAR_REQUIRE(B >= 1, "car_lpips_head_backward: B = %d, need at least one image pair", B);
    CAR_REQUIRE(H >= 16 && W >= 16, "car_lpips_head_backward: %d x %d image, the last tap needs H >= 16 and W >= 16", H, W);
    CAR_REQUIRE(lpips_shape_ok(B, H, W), "car_lpips_head_backward: %d x %d x %d is too large", B, H, W);
    (void)hipGetLastError();
    return head_backward(feats, B, H, W, lin, g, gf0, gf1, (hipStream_t)stream, "car_lpips_head_backward");
}

extern "C" size_t car_lpips_backward_packed_floats(void) { return backward_layer_offset(kLayers); }

extern "C" int car_lpips_pack_backward(const float* const* conv_w, float* packed, void* stream) {
    CAR_REQUIRE(conv_w && packed, "car_lpips_pack_backward: null pointer");
    for (int l = 0; l < kLayers; ++l) CAR_REQUIRE(conv_w[l], "car_lpips_pack_backward: null pointer (layer %d)", l);
    CAR_REQUIRE(aligned16(packed), "car_lpips_pack_backward: packed must be 16-byte aligned");
    for (int l = 1; l < kLayers; ++l)
        CAR_TRY(car_conv3x3_backward_pack(conv_w[l], kWidth[l - 1], kWidth[l], packed + backward_layer_offset(l), stream));
    return CAR_OK;
}

extern "C" size_t car_lpips_train_workspace_bytes(int B, int H, int W) {
    return lpips_shape_ok(B, H, W) ? make_train_plan(B, H, W).floats * sizeof(float) : 0;
}

// byte offset of layer l's retained map [2 B, h, w, C_l] (h = H >> pools in front of l) in the training workspace; (size_t)-1 when refused
extern "C" size_t car_lpips_train_layer_offset(int B, int H, int W, int l) {
    if (!lpips_shape_ok(B, H, W) || l < 0 || l >= kLayers) return (size_t)-1;
    return make_train_plan(B, H, W).act[l] * sizeof(float);
}

extern "C" int car_lpips_forward_train(const float* x, const float* y, int B, int H, int W, const float* packed, double* lpips, double* per_tap,
                                       void* work, size_t work_bytes, void* stream) {
    CAR_REQUIRE(x && y && packed && lpips && work, "car_lpips_forward_train: null pointer");
    CAR_REQUIRE(B >= 1, "car_lpips_forward_train: B = %d, need at least one image pair", B);
    CAR_REQUIRE(H >= 16 && W >= 16, "car_lpips_forward_train: %d x %d image, the last tap needs H >= 16 and W >= 16", H, W);
    CAR_REQUIRE(lpips_shape_ok(B, H, W), "car_lpips_forward_train: %d x %d x %d is too large", B, H, W);
    const size_t need = car_lpips_train_workspace_bytes(B, H, W);
    CAR_REQUIRE(work_bytes >= need, "car_lpips_forward_train: workspace holds %zu bytes, need %zu (car_lpips_train_workspace_bytes)", work_bytes, need);
    CAR_REQUIRE(aligned16(packed) && aligned16(work), "car_lpips_forward_train: packed and the workspace must be 16-byte aligned");

    const TrainPlan tp = make_train_plan(B, H, W);
    float* base = static_cast<float*>(work);
    hipStream_t st = (hipStream_t)stream;
    (void)hipGetLastError();
    CAR_TRY(conv(x, B, H, W, 3, 64, packed, base + tp.act[0], st));
    CAR_TRY(conv(y, B, H, W, 3, 64, packed, base + tp.act[0] + (size_t)B * H * W * 64, st));
    for (int l = 1; l < kLayers; ++l) {
        const float* src = base + tp.act[l - 1];
        if (pool_in_front(l)) {
            CAR_TRY(pool(src, 2 * B, tp.h[l - 1], tp.w[l - 1], kWidth[l - 1], base + tp.pooled, st));
            src = base + tp.pooled;
        }
        CAR_TRY(conv(src, 2 * B, tp.h[l], tp.w[l], kWidth[l - 1], kWidth[l], packed + layer_offset(l), base + tp.act[l], st));
    }
    const float* feats[kTaps];
    for (int k = 0; k < kTaps; ++k) feats[k] = base + tp.act[kTapLayer[k]];
    return head(feats, B, H, W, packed + layer_offset(kLayers), lpips, per_tap, reinterpret_cast<double*>(base + tp.scratch), st, "car_lpips_forward_train");
}

extern "C" int car_lpips_backward(const double* g, float* gx, float* gy, int B, int H, int W, const float* packed, const float* packed_backward,
                                  void* work, size_t work_bytes, void* stream) {
    CAR_REQUIRE(g && packed && packed_backward && work, "car_lpips_backward: null pointer");
    CAR_REQUIRE(gx || gy, "car_lpips_backward: null pointer (neither gx nor gy is given)");
    CAR_REQUIRE(B >= 1, "car_lpips_backward: B = %d, need at least one image pair", B);
    CAR_REQUIRE(H >= 16 && W >= 16, "car_lpips_backward: %d x %d image, the last tap needs H >= 16 and W >= 16", H, W);
    CAR_REQUIRE(lpips_shape_ok(B, H, W), "car_lpips_backward: %d x %d x %d is too large", B, H, W);
    const size_t need = car_lpips_train_workspace_bytes(B, H, W);
    CAR_REQUIRE(work_bytes >= need, "car_lpips_backward: workspace holds %zu bytes, need %zu (car_lpips_train_workspace_bytes)", work_bytes, need);
    CAR_REQUIRE(aligned16(packed) && aligned16(packed_backward) && aligned16(work),
                "car_lpips_backward: packed, packed_backward and the workspace must be 16-byte aligned");

    const TrainPlan tp = make_train_plan(B, H, W);
    float* base = static_cast<float*>(work);
    hipStream_t st = (hipStream_t)stream;
    (void)hipGetLastError();
    // the image stacks that need a gradient: images i0 .. i0 + n - 1 of every retained map
    const int i0 = gx ? 0 : B, n = (gx && gy) ? 2 * B : B;
    auto act = [&](int l) { return base + tp.act[l] + (size_t)i0 * tp.h[l] * tp.w[l] * kWidth[l]; };
    const float* feats[kTaps];
    float *hg0[kTaps], *hg1[kTaps];
    for (int k = 0; k < kTaps; ++k) {
        feats[k] = base + tp.act[kTapLayer[k]];
        hg0[k] = base + tp.hg[k];
        hg1[k] = base + tp.hg[k] + (gx ? (size_t)B * (H >> k) * (W >> k) * kTapWidth[k] : 0);
    }
    CAR_TRY(head_backward(feats, B, H, W, packed + layer_offset(kLayers), g, gx ? hg0 : nullptr, gy ? hg1 : nullptr, st, "car_lpips_backward"));
    float* cur = base + tp.ping[0];
    float* other = base + tp.ping[1];
    {
        const long total4 = (long)n * tp.h[12] * tp.w[12] * (kWidth[12] / 4), blocks = (total4 + 255) / 256;
        hipLaunchKernelGGL(relu_mask_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, st, base + tp.hg[4], act(12), cur, total4);
        CAR_CHECK_LAUNCH("car_lpips_backward");
    }
    int tap = kTaps - 2;
    for (int l = kLayers - 1; l >= 1; --l) {                             // cur holds the gradient at layer l's pre-activation
        const float* pk = packed_backward + backward_layer_offset(l);
        if (pool_in_front(l)) {                                          // layer l - 1 is a tap: its head gradient joins behind the pool's routing
            CAR_TRY(conv_backward(cur, n, tp.h[l], tp.w[l], kWidth[l - 1], kWidth[l], pk, nullptr, nullptr, other, st));
            CAR_TRY(pool_backward(other, act(l - 1), base + tp.hg[tap--], n, tp.h[l - 1], tp.w[l - 1], kWidth[l - 1], cur, st));
        } else {
            CAR_TRY(conv_backward(cur, n, tp.h[l], tp.w[l], kWidth[l - 1], kWidth[l], pk, act(l - 1), nullptr, other, st));
            float* t = cur; cur = other; other = t;
        }
    }
    const size_t img = (size_t)B * H * W;
    if (gx) CAR_TRY(conv_backward(cur, B, H, W, 3, 64, packed, nullptr, nullptr, gx, st));
    if (gy) CAR_TRY(conv_backward(cur + (gx ? img * 64 : 0), B, H, W, 3, 64, packed, nullptr, nullptr, gy, st));
    return CAR_OK;
}

// car_conv.hip — the library's dense convolutions, each stated once: the 3x3 implicit GEMM on the f16 matrix pipe that LPIPS (car_lpips.hip:
// car_conv3x3, car_conv3x3_backward), the encoder's trunk (car_trunk.hip: car_conv3x3_same) and its decoder (car_decoder.hip:
// car_conv3x3_pad1) run, its packer and size rule, and the fp32 7x7 first layer 3 -> 64 of the trunk's stem and of conv_map (car_stem7x7,
// car_conv7x7_pad3).  Those units keep their networks, layouts, chains, argument checks and C entries and call the launchers at the end of
// this file (declared in car_common.h).
//
// conv3x3_kernel is the row sweep of car_row_sweep.h (split-fp16 operands, three v_mfma_f32_16x16x32_f16 products per term, fp32
// accumulation, weight chunks streamed L2 -> LDS by LDS-DMA) run as an implicit GEMM over 9 K in ONE sweep, the K loop's skeleton in the
// kernel's own frame as that file prescribes: a row of the A operand is an output pixel, a K step reads 32 channels of one tap — the address
// of the input pixel under the window's centre plus one of nine offsets — and a tap outside the image contributes zeros.  The row's power
// of two follows the largest magnitude seen so far along the 9 K values: the sweep's rule.  A row's result depends on its own nine pixels
// and the weights only, never on its neighbours in the launch: an image gives the same bits wherever it sits in the batch, which is what
// makes LPIPS of two identical images exactly 0.  A compile-time Form supplies what differs between the callers and nothing else.
// The sweep's arithmetic relies on this unit being compiled as car_linear16.hip is (no extra flags in __graft_entry__.UNITS).
#include "car_common.h"
#include <math.h>
#include <stdint.h>

namespace {

#include "car_row_sweep.h"

// ---- the forms -------------------------------------------------------------------------------------------------------------------------
// A form states, for output row `lrow`: centre() — the input pixel under the window's centre (its coordinates and its index among the
// call's input pixels; always inside its image) and in_pixels(), the input's extent; Step — how K step c maps to (tap, 32-channel step
// within it); relu_in() and loaded() — whether finish_x applies a ReLU, and the value it takes; kClamp — how far the row's exponent may
// fall; start() — how the accumulators start; store() — the epilogue over the sums, which arrive at the row's power of two p (pinv = 1 / p)
// times the layer's (dW = 2^-shift).  Offset: the type a tap's offset W K is formed in.
// Two things are shaped by what keeps the six LPIPS instances the instructions they were (profiles/conv_once.md): loaded() is a member
// because a ReLU selected by a constant false inside finish_x still reordered them, and store() is handed the output's base and width by
// value because address arithmetic on a.Y and a.N read through the reference came out scheduled differently in the data gradient.

// LPIPS (stride 1, padding 1, K a power of two): the output pixel is its own input pixel, tap = c >> lgk
struct LpipsArgs {
    const float* X;                        // [n, H, W, K]
    const float* Wp; int tiles_total;      // [K step][tiles_total][512]: k = tap * K + channel
    const float* bias;                     // N floats (forward only)
    const float* down;                     // 2^-shift of the packed layer
    float* Y;                              // [n, H, W, N]
    const float* act;                      // data gradient only: [n, H, W, N] forward activation whose sign masks Y, or nullptr
    const float* add;                      // data gradient only: [n, H, W, N] added in front of the mask, or nullptr
    int H, W, K, N, lgk, chunks;           // lgk = log2(K / 32)
    long M;                                // n H W output pixels
};
// BWD: the data gradient of the same convolution.  The same sweep over weights packed transposed and flipped
// (car_pack.hip ConvSource), no bias, and the epilogue Y = (sum + add) * (act > 0) in the place of bias + ReLU.
// A gradient row's power of two: pow2_scale with the exponent clamped far lower (car_split.h kPow2LoWide).  When a later K step raises the
// row's maximum, the accumulators move by pn * pinv, a power of two as small as 2^-190: what was summed so far may then lose low bits or
// flush to 0.  It is below 2^-150 of the row's new scale, so the accuracy bound is untouched, but "a cotangent scaled by 2^k scales every
// entry exactly" holds only while no row's magnitude crosses the clamp span inside one sweep.
template <bool BWD>
struct LpipsForm {
    using Args = LpipsArgs;
    using Offset = int;
    static constexpr int kClamp = BWD ? kPow2LoWide : kPow2Lo;
    struct Step {
        int tap = 0, kc = 0;
        __device__ __forceinline__ void next(const Args& a, int c) {
            const int cn = c + 1 < a.chunks ? c + 1 : c;
            tap = cn >> a.lgk; kc = cn & ((1 << a.lgk) - 1);
        }
    };
    static __device__ __forceinline__ long centre(const Args& a, long lrow, int& cy, int& cx) {
        const int pix = (int)(lrow % ((long)a.H * a.W));
        cy = pix / a.W; cx = pix % a.W;
        return lrow;
    }
    static __device__ __forceinline__ long in_pixels(const Args& a) { return a.M; }
    static __device__ __forceinline__ bool relu_in(const Args&) { return false; }
    static __device__ __forceinline__ float loaded(bool, float e) { return e; }
    template <int NT>
    static __device__ __forceinline__ void start(f32x4 (&acc)[NT], const Args& a, int tile0, int q4, float p, float dW) {
        if constexpr (BWD) {
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        } else init_bias<NT>(acc, a.bias + 16 * tile0, q4, p / dW);
    }
    template <int NT>
    static __device__ __forceinline__ void store(f32x4 (&acc)[NT], const Args& a, float* Y, int N, long row, int tile0, int q4, float dW, float pinv) {
        float* yrow = Y + row * N + 16 * tile0 + 4 * q4;
        if constexpr (BWD) {
            scale_acc<NT>(acc, dW);                                        // two steps: dW * pinv may lie below fp32's normal range
            scale_acc<NT>(acc, pinv);
            const long at = row * N + 16 * tile0 + 4 * q4;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                float4 v = make_float4(acc[t][0], acc[t][1], acc[t][2], acc[t][3]);
                if (a.add) {
                    CAR_BOUNDS_TRAP(at + 16 * t + 4 <= a.M * a.N);
                    const float4 d = *reinterpret_cast<const float4*>(a.add + at + 16 * t);
                    v.x += d.x; v.y += d.y; v.z += d.z; v.w += d.w;
                }
                if (a.act) {
                    CAR_BOUNDS_TRAP(at + 16 * t + 4 <= a.M * a.N);
                    v = keep_where_positive(v, *reinterpret_cast<const float4*>(a.act + at + 16 * t));
                }
                *reinterpret_cast<float4*>(yrow + 16 * t) = v;
            }
        } else {
            scale_acc<NT>(acc, dW * pinv);
#pragma unroll
            for (int t = 0; t < NT; ++t)
                *reinterpret_cast<float4*>(yrow + 16 * t) =
                    make_float4(fmaxf(acc[t][0], 0.0f), fmaxf(acc[t][1], 0.0f), fmaxf(acc[t][2], 0.0f), fmaxf(acc[t][3], 0.0f));
        }
    }
};

// General (car_conv3x3_same, car_conv3x3_pad1): stride 1 or 2, the padding in front (pt, pl) the caller's — TF "SAME" pads 0 or 1, torch's
// symmetric padding 1 — so the window's centre is input pixel (stride oy + 1 - pt, stride ox + 1 - pl) of an image whose extents differ from
// the output's.  K = 768 is 24 K steps per tap, no power of two, so the tap and the step within it are counted along.  The input may go
// through a ReLU on load (the padding stays zeros: a tap outside the image is dropped by index behind the activation); the epilogue is
// act_out((sum + bias) + add) + Y by run-time flags, each part optional.
// EPILOGUE false: the instance of a caller that has none of it (the trunk) — no ReLU on load, the plain store.  As ONE instance with the
// flags at run time the trunk's layers were 8 to 12 % slower and the decoder's about 1 % (profiles/conv_once.md): the ReLU select of every
// K step and the epilogue's branches are paid by a 25 us kernel that needs neither, so the epilogue is a parameter of the form.
struct GeneralArgs {
    const float* X;                        // [n, H, W, K]
    const float* Wp; int tiles_total;      // [K step][tiles_total][512]: k = tap * K + channel
    const float* down;                     // 2^-shift of the packed layer
    const float* bias;                     // [N] or null
    const float* add;                      // [n, Ho, Wo, N] or null
    float* Y;                              // [n, Ho, Wo, N]
    int H, W, Ho, Wo, stride, pt, pl;      // pt, pl: the padding in front (top, left)
    int K, N, ksteps, chunks, flags;       // ksteps = K / 32 K steps per tap, chunks = 9 ksteps; flags: CAR_LIN_RELU_IN | _RELU_OUT | _ACCUM
    long M, Min;                           // n Ho Wo output pixels, n H W input pixels
};
template <bool EPILOGUE>
struct GeneralForm {
    using Args = GeneralArgs;
    using Offset = long;                   // W K may pass 2^31 in a wide image
    static constexpr int kClamp = kPow2Lo;
    struct Step {
        int tap = 0, kc = 0;
        __device__ __forceinline__ void next(const Args& a, int c) {          // the last K step once more behind the end
            if (c + 1 < a.chunks && ++kc == a.ksteps) { kc = 0; ++tap; }
        }
    };
    static __device__ __forceinline__ long centre(const Args& a, long lrow, int& cy, int& cx) {
        const int pix = (int)(lrow % ((long)a.Ho * a.Wo)), oy = pix / a.Wo, ox = pix % a.Wo;
        const long img = lrow / ((long)a.Ho * a.Wo);
        cy = oy * a.stride + 1 - a.pt; cx = ox * a.stride + 1 - a.pl;
        return (img * a.H + cy) * a.W + cx;
    }
    static __device__ __forceinline__ long in_pixels(const Args& a) { return a.Min; }
    static __device__ __forceinline__ bool relu_in(const Args& a) { return EPILOGUE && (a.flags & CAR_LIN_RELU_IN) != 0; }
    static __device__ __forceinline__ float loaded(bool relu, float e) {
        if constexpr (EPILOGUE) return relu ? fmaxf(e, 0.0f) : e;
        else return e;
    }
    template <int NT>
    static __device__ __forceinline__ void start(f32x4 (&acc)[NT], const Args&, int, int, float, float) {
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    }
    // ((sum + bias) + add), the ReLU (a NaN stays a NaN, as F.relu leaves it), then + Y
    template <int NT>
    static __device__ __forceinline__ void store(f32x4 (&acc)[NT], const Args& a, float* Y, int N, long row, int tile0, int q4, float dW, float pinv) {
        if constexpr (!EPILOGUE) {
            float* yrow = Y + row * N + 16 * tile0 + 4 * q4;
            scale_acc<NT>(acc, dW * pinv);
#pragma unroll
            for (int t = 0; t < NT; ++t) *reinterpret_cast<float4*>(yrow + 16 * t) = make_float4(acc[t][0], acc[t][1], acc[t][2], acc[t][3]);
        } else {                                                           // a.Y, a.N: as the decoder's kernel read them; by value the
                                                                           // epilogue came out scheduled differently (same count)
            const bool relu_out = (a.flags & CAR_LIN_RELU_OUT) != 0, accum = (a.flags & CAR_LIN_ACCUM) != 0;
            const long at = row * a.N + 16 * tile0 + 4 * q4;
            scale_acc<NT>(acc, dW * pinv);
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                float4 v = make_float4(acc[t][0], acc[t][1], acc[t][2], acc[t][3]);
                if (a.bias) {
                    CAR_BOUNDS_TRAP(16 * (tile0 + t) + 4 * q4 + 4 <= a.N);
                    const float4 b = *reinterpret_cast<const float4*>(a.bias + 16 * (tile0 + t) + 4 * q4);
                    v.x += b.x; v.y += b.y; v.z += b.z; v.w += b.w;
                }
                CAR_BOUNDS_TRAP(at + 16 * t + 4 <= a.M * a.N);
                if (a.add) {
                    const float4 d = *reinterpret_cast<const float4*>(a.add + at + 16 * t);
                    v.x += d.x; v.y += d.y; v.z += d.z; v.w += d.w;
                }
                if (relu_out) { v.x = v.x < 0.0f ? 0.0f : v.x; v.y = v.y < 0.0f ? 0.0f : v.y; v.z = v.z < 0.0f ? 0.0f : v.z; v.w = v.w < 0.0f ? 0.0f : v.w; }
                float4* dst = reinterpret_cast<float4*>(a.Y + at + 16 * t);
                if (accum) { const float4 o = *dst; v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w; }
                *dst = v;
            }
        }
    }
};

// ---- the kernel ------------------------------------------------------------------------------------------------------------------------
// Instances: LPIPS forward and data gradient at NT 4, 8, 16 (N = 64, 128, wider), the general form's two at NT 4 alone.  The trunk's and the
// decoder's layers are small — 128 pixels to 8192 at one pair — and a 256-wide layer as four column groups of four tiles is four
// workgroups per block of 192 pixels: a wider group only leaves more of the device idle there (512 pixels as one group of 16 tiles are
// three working workgroups, as four groups twelve).  No shape of theirs has the 25 000 pixels at which a wider group would still fill 256
// CUs, so no wider general instance is built.
template <int NT, class Form>
__global__ void __launch_bounds__(kThreads) conv3x3_kernel(const typename Form::Args a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];      // [2][NT][512]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int s = lane & 15, q4 = lane >> 4;
    RowPlace pl;                                                       // one XCD per block of pixels: car_row_sweep.h
    if (!place_rows<NT>(a.tiles_total, a.M, wave, s, pl)) return;
    const long row = pl.row, lrow = pl.lrow;
    const int tile0 = pl.tile0<NT>();
    const int K = a.K;
    const bool relu_in = Form::relu_in(a);
    // the input pixel under the window's centre, and which of the nine taps lie inside its image
    int cy, cx;
    const long centre = Form::centre(a, lrow, cy, cx);
    unsigned inside = 0;
#pragma unroll
    for (int t = 0; t < 9; ++t)
        if ((unsigned)(cy + t / 3 - 1) < (unsigned)a.H && (unsigned)(cx + t % 3 - 1) < (unsigned)a.W) inside |= 1u << t;
    const float* xpix = a.X + centre * K + 8 * q4;

    {   // chunk 0 goes out now: what follows runs under the DMA
        const NextChunk n0 = chunk_desc<NT>(a, tile0, lds, 0);
#pragma unroll
        for (int p = 0; p < pieces_of(NT); ++p) stream_issue_piece(n0, p, lane, wave);
    }
    // this lane's eight values of step kc of tap t: channels 32 kc + 8 q4 .. + 7 of input pixel (cy + t / 3 - 1, cx + t % 3 - 1).  issue_x only
    // issues the loads — from the centre pixel when the tap is outside, a valid address whose values are dropped; finish_x turns them into
    // values when they are consumed (car_row_sweep.h): the ReLU first, then the tap's index, so the padding is zeros whatever was loaded
    auto issue_x = [&](int t, int kc, float4 (&raw)[2]) {
        const typename Form::Offset off = ((typename Form::Offset)(t / 3 - 1) * a.W + (t % 3 - 1)) * K;
        const float* src = xpix + (((inside >> t) & 1u) ? off : 0) + 32 * kc;
        CAR_BOUNDS_TRAP(src >= a.X && src + 8 <= a.X + Form::in_pixels(a) * K);
        raw[0] = *reinterpret_cast<const float4*>(src);
        raw[1] = *reinterpret_cast<const float4*>(src + 4);
    };
    auto finish_x = [&](int t, const float4 (&raw)[2], float (&x)[8]) {
        const bool in = ((inside >> t) & 1u) != 0;
        const float e[8] = {raw[0].x, raw[0].y, raw[0].z, raw[0].w, raw[1].x, raw[1].y, raw[1].z, raw[1].w};
#pragma unroll
        for (int i = 0; i < 8; ++i) x[i] = in ? Form::loaded(relu_in, e[i]) : 0.0f;
    };
    const float dW = a.down[0];
    float xc[8];
    {
        float4 raw[2];
        issue_x(0, 0, raw);
        finish_x(0, raw, xc);
    }
    float mrun = fmaxf(row_max(xc), 1e-30f), p, pinv;
    pow2_scale<Form::kClamp>(mrun, p, pinv);

    f32x4 acc[NT];
    Form::template start<NT>(acc, a, tile0, q4, p, dW);
    half8 bhi, blo;
    split8(xc, p, bhi, blo);
    stream_sync();                                                     // weight chunk 0 landed

    // the sweep's skeleton (car_row_sweep.h); ks = the tap and the step within it of the K step whose values are in bhi / blo
    typename Form::Step ks;
#pragma unroll 1
    for (int c = 0; c < a.chunks; ++c) {
        const float* wl = lds + (c & 1) * NT * kTile + 4 * lane;
        const NextChunk nx = chunk_desc<NT>(a, tile0, lds, c + 1);
        ks.next(a, c);                                                 // the next K step (the last one once more behind the end)
        float4 rawn[2];
        issue_x(ks.tap, ks.kc, rawn);                                  // its values: in flight under this step's MFMAs
#pragma unroll
        for (int qs = 0; qs < NT / 2; ++qs) {
            const float* w0 = wl + (2 * qs * 2) * 256;
            mfma_pair(acc[2 * qs], acc[2 * qs + 1], w0, w0 + 512, bhi, blo);
            issue_next_piece<NT>(nx, qs, c + 1 < a.chunks, lane, wave);
            __builtin_amdgcn_sched_barrier(0);
        }
        // the next K step may outgrow the row's power of two: move the row (accumulators and scale) to the smaller one, exactly
        float xn[8];
        finish_x(ks.tap, rawn, xn);
        const float mn = row_max(xn);
        if (__builtin_amdgcn_ballot_w64(mn > mrun) != 0) {
            float pn, pninv;
            mrun = fmaxf(mrun, mn);
            pow2_scale<Form::kClamp>(mrun, pn, pninv);
            scale_acc<NT>(acc, pn * pinv);
            p = pn; pinv = pninv;
        }
        split8(xn, p, bhi, blo);
        stream_sync();
    }
    if (row >= a.M) return;
    Form::template store<NT>(acc, a, a.Y, a.N, row, tile0, q4, dW, pinv);
}

template <int NT, class Form>
int launch_conv(const char* who, const typename Form::Args& a, hipStream_t st) {
    const size_t lds_bytes = (size_t)2 * NT * kTile * sizeof(float);
    CAR_LAUNCH_LDS(who, (conv3x3_kernel<NT, Form>), dim3(sweep_grid(a.M, a.tiles_total / NT)), dim3(kThreads), lds_bytes, st, a);
    return CAR_OK;
}

// ---- the first layer 3 -> 64, 7x7, fp32 on the vector pipe --------------------------------------------------------------------------------
// a wave = the 64 output channels of one pixel at a time (the pixel is wave-uniform: its inputs are scalar loads), 8 pixels per wave;
// lane n keeps channel n's 147 weights.  The accumulator starts at the bias, or at zero without one; the terms are added in the order
// (channel, row, column) of the window by fmaf; a tap in the padding adds nothing.  X is [n, 3, H, W], Y [n, Ho, Wo, 64].
constexpr int k7Pix = 8, k7Terms = 147;
template <int STRIDE>
__global__ void __launch_bounds__(256) conv7x7_kernel(const float* __restrict__ X, const float* __restrict__ Wt, const float* __restrict__ bias,
                                                      float* __restrict__ Y, int H, int W, int Ho, int Wo, int pt, int pl, long M, long Min) {
    const int n = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    float w[k7Terms];
#pragma unroll
    for (int k = 0; k < k7Terms; ++k) w[k] = Wt[n * k7Terms + k];
    const float b = bias ? bias[n] : 0.0f;
    const long p0 = ((long)blockIdx.x * 4 + wave) * k7Pix;
    for (int i = 0; i < k7Pix; ++i) {
        const long p = p0 + i;
        if (p >= M) return;
        const int pix = (int)(p % ((long)Ho * Wo)), oy = pix / Wo, ox = pix % Wo;
        const float* img = X + (p / ((long)Ho * Wo)) * 3 * H * W;
        float acc = b;
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int ky = 0; ky < 7; ++ky) {
                const int iy = STRIDE * oy + ky - pt;
                if ((unsigned)iy >= (unsigned)H) continue;
#pragma unroll
                for (int kx = 0; kx < 7; ++kx) {
                    const int ix = STRIDE * ox + kx - pl;
                    if ((unsigned)ix < (unsigned)W) {
                        CAR_BOUNDS_TRAP(img + ((long)c * H + iy) * W + ix < X + Min * 3);
                        acc = fmaf(img[((long)c * H + iy) * W + ix], w[(c * 7 + ky) * 7 + kx], acc);
                    }
                }
            }
        Y[p * 64 + n] = acc;
    }
}

}  // namespace

// ---- what the three units call (car_common.h) ---------------------------------------------------------------------------------------------
size_t car_conv3x3_tile_floats(int K, int N) { return (size_t)(9 * K / 32) * (N / 16) * kTile; }

int car_conv3x3_pack_tiles(const char* who, const float* w, const float* bias, int K, int N, bool flip, float* packed, hipStream_t st) {
    float* scale = packed + car_conv3x3_tile_floats(K, N);
    (void)hipGetLastError();
    CAR_CHECK_HIP(hipMemsetAsync(scale, 0, 64 * sizeof(float), st), "%s: memset failed", who);
    const car_pack_scale s{scale + 2, scale, scale + 1};
    car_pack_absmax(st, 64, w, 9 * K * N, nullptr, nullptr, 1, 9 * K * N, s);
    car_pack_conv16(st, 512, w, K, N, flip, s, reinterpret_cast<_Float16*>(packed));
    if (bias) CAR_CHECK_HIP(hipMemcpyAsync(scale + 64, bias, sizeof(float) * N, hipMemcpyDeviceToDevice, st), "%s: bias copy failed", who);
    CAR_CHECK_LAUNCH(who);
    return CAR_OK;
}

int car_conv3x3_lpips(const float* X, const float* packed, const float* act, const float* add, float* Y, int H, int W, int K, int N, long M,
                      bool backward, hipStream_t st) {
    LpipsArgs a;
    a.X = X; a.Wp = packed; a.tiles_total = N / 16;
    a.down = packed + car_conv3x3_tile_floats(K, N) + 1;
    a.bias = backward ? nullptr : packed + car_conv3x3_tile_floats(K, N) + 64;
    a.Y = Y; a.act = act; a.add = add;
    a.H = H; a.W = W; a.K = K; a.N = N; a.chunks = 9 * K / 32; a.M = M;
    a.lgk = K == 64 ? 1 : K == 128 ? 2 : K == 256 ? 3 : 4;
    if (backward) {
        if (N == 64) return launch_conv<4, LpipsForm<true>>("car_conv3x3_backward", a, st);
        if (N == 128) return launch_conv<8, LpipsForm<true>>("car_conv3x3_backward", a, st);
        return launch_conv<16, LpipsForm<true>>("car_conv3x3_backward", a, st);
    }
    if (N == 64) return launch_conv<4, LpipsForm<false>>("car_conv3x3", a, st);
    if (N == 128) return launch_conv<8, LpipsForm<false>>("car_conv3x3", a, st);
    return launch_conv<16, LpipsForm<false>>("car_conv3x3", a, st);
}

int car_conv3x3_general(const char* who, bool epilogue, const float* X, int n, int H, int W, int K, int N, int stride, int pt, int pl, int Ho, int Wo,
                        const float* packed, const float* bias, const float* add, int flags, float* Y, hipStream_t st) {
    GeneralArgs a;
    a.X = X; a.Wp = packed; a.tiles_total = N / 16; a.down = packed + car_conv3x3_tile_floats(K, N) + 1; a.bias = bias; a.add = add; a.Y = Y;
    a.H = H; a.W = W; a.Ho = Ho; a.Wo = Wo; a.stride = stride; a.pt = pt; a.pl = pl;
    a.K = K; a.N = N; a.ksteps = K / 32; a.chunks = 9 * a.ksteps; a.flags = flags;
    a.M = (long)n * Ho * Wo; a.Min = (long)n * H * W;
    if (epilogue) return launch_conv<4, GeneralForm<true>>(who, a, st);
    return launch_conv<4, GeneralForm<false>>(who, a, st);
}

int car_conv7x7(const char* who, const float* x, int n, int H, int W, int stride, int pt, int pl, int Ho, int Wo, const float* w,
                const float* bias, float* Y, hipStream_t st) {
    const long M = (long)n * Ho * Wo, Min = (long)n * H * W;
    const auto kernel = stride == 2 ? conv7x7_kernel<2> : conv7x7_kernel<1>;
    (void)hipGetLastError();
    hipLaunchKernelGGL(kernel, dim3(car_div_up(M, 4 * k7Pix)), dim3(256), 0, st, x, w, bias, Y, H, W, Ho, Wo, pt, pl, M, Min);
    CAR_CHECK_LAUNCH(who);
    return CAR_OK;
}

// car_summary.hip — the training loop's summaries on the device (include/car_hip.h: car_attention_entropy, car_colormap,
// car_epipolar_overlay, car_image_grid).
//
// The reference builds these on the host: summaries.py:15-141 pulls pixel_val and the depth to the CPU and paints the epipolar panel in
// a Python loop over scenes x views x samples, and training.py:110-115 evaluates the attention entropy as a chain of full-size
// elementwise kernels at every step.  Here the per-step entropy is one small reduction whose result stays on the device, and the
// panels are built where the frames already are.
//
// All four are memory-bound kernels on small data.  Images are fp32 channel-last, the stream is the last argument, scratch is the
// caller's.  No float atomics; every sum has a fixed order, so the same input gives the same bits.  Built with -ffp-contract=off: the
// colour map, the overlay and the grid are pinned bit for bit to their restatements (tests/summary_restatement.py), which needs the
// fp32 products, differences and quotients below rounded one at a time.
#include "car_common.h"
#include <math.h>

namespace {

constexpr int kMaxSamples = 768;                 // samples per ray the entropy and the overlay accept
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kEntropyMaxBlocks = 1024;

// ---- (a) attention entropy -------------------------------------------------------------------------------------------------------------
// Stage 1: one wave per row at a time.  Lane l forms the fp32 terms w * logf(w + 1e-5f) of samples l, l + 64, ... as the reference's
// torch expression does and adds them in fp64 in that order; a fixed butterfly joins the lanes.  A wave walks rows wave, wave + n_waves,
// ... and adds their entropies in that order; thread 0 adds the block's four wave sums in order into partial[block].  The grid is a
// function of `rows` alone, so nothing depends on launch timing.
__global__ __launch_bounds__(kThreads) void entropy_rows_kernel(const float* __restrict__ w, long rows, int S, int nan_rows_zero,
                                                                double* __restrict__ partial) {
    __shared__ double wave_acc[kWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long n_waves = (long)gridDim.x * kWaves;
    double acc = 0.0;
    for (long row = (long)blockIdx.x * kWaves + wave; row < rows; row += n_waves) {
        const float* p = w + (size_t)row * S;
        double s = 0.0;
        for (int j = lane; j < S; j += 64) {
            const float wj = p[j];
            const float term = wj * logf(wj + 1e-5f);
            s += (double)term;
        }
        double ent = -wave_sum(s);
        if (nan_rows_zero && ent != ent) ent = 0.0;                  // training.py:113: ent[torch.isnan(ent)] = 0
        acc += ent;
    }
    if (lane == 0) wave_acc[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = wave_acc[0];
        for (int i = 1; i < kWaves; ++i) t += wave_acc[i];
        partial[blockIdx.x] = t;
    }
}

// Stage 2: one wave adds the blocks' sums, lane l taking l, l + 64, ... in order, then the same butterfly.
__global__ __launch_bounds__(64) void entropy_sum_kernel(const double* __restrict__ partial, int n, double* __restrict__ out) {
    const int lane = threadIdx.x;
    double s = 0.0;
    for (int i = lane; i < n; i += 64) s += partial[i];
    s = wave_sum(s);
    if (lane == 0) out[0] = s;
}

bool entropy_shape_ok(long rows, int S) { return rows >= 1 && S >= 1 && S <= kMaxSamples && (double)rows * S < 9.0e15; }

int entropy_blocks(long rows) {
    const long b = (rows + kWaves - 1) / kWaves;
    return (int)(b < kEntropyMaxBlocks ? b : kEntropyMaxBlocks);
}

// ---- (b) colour map ---------------------------------------------------------------------------------------------------------------------
// matplotlib's Colormap.__call__ on a float array with a 256-entry table: t * 256 truncated, t == 1 -> 255, t > 1 -> "over" (entry 255),
// t < 0 -> "under" (entry 0), NaN -> "bad" (0, 0, 0).  t * 256 is exact in fp32 (or overflows to inf, which is "over").
__global__ __launch_bounds__(kThreads) void colormap_kernel(const float* __restrict__ x, size_t n, float scale, const float* __restrict__ lut,
                                                            float* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const float t = x[i] / scale;                                    // summaries.py:36: depth / 10. in fp32
    float r = 0.0f, g = 0.0f, b = 0.0f;
    if (t == t) {
        const float a = t * 256.0f;
        int idx;
        if (a < 0.0f) idx = 0;
        else if (a >= 256.0f) idx = 255;                             // a == 256 is "not out of range" and maps to 255, as "over" does
        else idx = (int)a;
        r = lut[3 * idx];
        g = lut[3 * idx + 1];
        b = lut[3 * idx + 2];
    }
    out[3 * i] = r;
    out[3 * i + 1] = g;
    out[3 * i + 2] = b;
}

// ---- (c) epipolar overlay ---------------------------------------------------------------------------------------------------------------
// summaries.py:72-136 in gather form.  The panel holds the B target tiles, then the context tiles view-major (view 0 of every scene, view 1
// of every scene, ...: summaries.py:134-136).  A block owns 256 pixels of one panel tile; it puts the tile's sample centres into LDS
// once, and every pixel then decides its own value: -1 inside the arg-max sample's square, else 0 inside any sample's square, else the
// input — the reference's paint order without a write race.
struct OverlayArgs {
    const float* trgt;                            // [B][H][W][3]
    const float* ctxt;                            // [B * V][H][W][3], scene-major view-minor
    const float* pixel_val;                       // [B * V][rays][S][2]
    const long long* at_wt_max;                   // [B * V][rays]
    const float* uv;                              // [B][rays][2]
    float* panel;                                 // [B + B * V][H][W][3]
    int B, V, H, W, rays, probe, S, pix;
};

constexpr int kNoSample = -(1 << 24);             // a centre whose square is empty whatever the image size

__device__ __forceinline__ int trunc_to_int(float v) {               // int(v) of a finite v, kept inside int's range
    return (int)fminf(fmaxf(v, -1.0e9f), 1.0e9f);
}

__device__ __forceinline__ bool in_square(int py, int px, int y, int x, int pix, int H, int W) {
    // rows [max(y - pix, 0), min(y + pix, H - 1)), columns likewise with W: the upper end is exclusive (summaries.py:113-116)
    const int ymin = max(y - pix, 0), ymax = min(y + pix, H - 1);
    const int xmin = max(x - pix, 0), xmax = min(x + pix, W - 1);
    return py >= ymin && py < ymax && px >= xmin && px < xmax;
}

__global__ __launch_bounds__(kThreads) void overlay_kernel(OverlayArgs a) {
    __shared__ int sx[kMaxSamples], sy[kMaxSamples];
    __shared__ int s_best;
    const int tile = blockIdx.y, tid = threadIdx.x;
    const bool target = tile < a.B;
    const float* src;
    int n_samples;
    if (target) {                                                    // the probe pixel itself: one -1 square (summaries.py:98-102)
        src = a.trgt + (size_t)tile * a.H * a.W * 3;
        n_samples = 1;
        if (tid == 0) {
            const float* c = a.uv + ((size_t)tile * a.rays + a.probe) * 2;
            const bool ok = c[0] == c[0] && c[1] == c[1];
            sx[0] = ok ? trunc_to_int(c[0]) : kNoSample;
            sy[0] = ok ? trunc_to_int(c[1]) : kNoSample;
            s_best = 0;
        }
    } else {
        const int k = tile - a.B, view = k / a.B, scene = k % a.B;
        const size_t row = (size_t)scene * a.V + view;               // view k's samples paint only that scene's k-th context tile
        src = a.ctxt + row * a.H * a.W * 3;
        n_samples = a.S;
        const float* pv = a.pixel_val + (row * a.rays + a.probe) * (size_t)a.S * 2;
        for (int j = tid; j < a.S; j += kThreads) {
            float vx = (pv[2 * j] + 1.0f) / 2.0f, vy = (pv[2 * j + 1] + 1.0f) / 2.0f;
            const bool ok = vx == vx && vy == vy;                    // a NaN sample paints nothing (the reference's int() raises on it)
            vx = fminf(fmaxf(vx, 0.0f), 1.0f);
            vy = fminf(fmaxf(vy, 0.0f), 1.0f);
            sx[j] = ok ? (int)(vx * (float)(a.W - 1)) : kNoSample;
            sy[j] = ok ? (int)(vy * (float)(a.H - 1)) : kNoSample;
        }
        if (tid == 0) {
            const long long best = a.at_wt_max[row * a.rays + a.probe];
            s_best = (best >= 0 && best < a.S) ? (int)best : -1;     // an index outside [0, S) marks nothing
        }
    }
    __syncthreads();
    const int p = blockIdx.x * kThreads + tid;
    if (p >= a.H * a.W) return;
    const int py = p / a.W, px = p % a.W;
    const float* in = src + (size_t)p * 3;
    float* out = a.panel + ((size_t)tile * a.H * a.W + p) * 3;
    const int best = s_best;
    if (best >= 0 && in_square(py, px, sy[best], sx[best], a.pix, a.H, a.W)) {
        out[0] = out[1] = out[2] = -1.0f;
        return;
    }
    if (!target) {
        for (int j = 0; j < n_samples; ++j) {
            if (in_square(py, px, sy[j], sx[j], a.pix, a.H, a.W)) {
                out[0] = out[1] = out[2] = 0.0f;
                return;
            }
        }
    }
    out[0] = in[0];
    out[1] = in[1];
    out[2] = in[2];
}

// ---- (d) image grid ---------------------------------------------------------------------------------------------------------------------
// torchvision.utils.make_grid(x, normalize=True, scale_each=...) with nrow = 8, padding = 2, pad_value = 0.  Launch 1: one workgroup per
// image takes the min and max of its (clamped) values into scratch [N][2]; an image that holds a NaN gets NaN for both, as torch's min /
// max give.  Launch 2: one thread per output element; it reads its image's range, or folds all N ranges in order, and writes
// (clamp(x, low, high) - low) / max(high - low, 1e-5), or 0 on the padding.
constexpr int kRangeThreads = 1024;

__device__ __forceinline__ float clamped(float v, int clamp, float lo, float hi) {
    return clamp ? fminf(fmaxf(v, lo), hi) : v;                      // a NaN is caught by the range, not here
}

__global__ __launch_bounds__(kRangeThreads) void grid_range_kernel(const float* __restrict__ x, size_t per_image, int clamp, float lo, float hi,
                                                                   float* __restrict__ range) {
    __shared__ float smin[kRangeThreads / 64], smax[kRangeThreads / 64];
    __shared__ int snan[kRangeThreads / 64];
    const float* p = x + (size_t)blockIdx.x * per_image;
    float mn = INFINITY, mx = -INFINITY;
    int bad = 0;
    for (size_t i = threadIdx.x; i < per_image; i += kRangeThreads) {
        const float raw = p[i];
        bad |= raw != raw;
        const float v = clamped(raw, clamp, lo, hi);
        mn = fminf(mn, v);
        mx = fmaxf(mx, v);
    }
    for (int o = 32; o > 0; o >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, o, 64));
        mx = fmaxf(mx, __shfl_xor(mx, o, 64));
        bad |= __shfl_xor(bad, o, 64);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        smin[wave] = mn;
        smax[wave] = mx;
        snan[wave] = bad;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < kRangeThreads / 64; ++i) {
            mn = fminf(mn, smin[i]);
            mx = fmaxf(mx, smax[i]);
            bad |= snan[i];
        }
        range[2 * blockIdx.x] = bad ? NAN : mn;
        range[2 * blockIdx.x + 1] = bad ? NAN : mx;
    }
}

struct GridArgs {
    const float* x;                               // [N][H][W][3]
    const float* range;                           // [N][2]
    float* out;                                   // [3][Hg][Wg]
    int N, H, W, Hg, Wg, xm, scale_each, clamp;
    float lo, hi;
};

__global__ __launch_bounds__(kThreads) void grid_write_kernel(GridArgs a) {
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    const size_t plane = (size_t)a.Hg * a.Wg;
    if (i >= 3 * plane) return;
    const int ch = (int)(i / plane), gy = (int)((i % plane) / a.Wg), gx = (int)(i % a.Wg);
    int k, y, x;
    if (a.N == 1) {                                                  // make_grid returns the normalised image itself, unpadded
        k = 0;
        y = gy;
        x = gx;
    } else {
        const int cy = gy / (a.H + 2), cx = gx / (a.W + 2);
        y = gy - cy * (a.H + 2) - 2;
        x = gx - cx * (a.W + 2) - 2;
        k = cy * a.xm + cx;
        // the last cell row / column holds only the closing padding; cells past image N - 1 stay empty
        if (y < 0 || x < 0 || cx >= a.xm || k >= a.N) {
            a.out[i] = 0.0f;
            return;
        }
    }
    float low, high;
    if (a.scale_each) {
        low = a.range[2 * k];
        high = a.range[2 * k + 1];
    } else {
        low = a.range[0];
        high = a.range[1];
        bool bad = low != low;
        for (int j = 1; j < a.N; ++j) {
            const float l = a.range[2 * j], h = a.range[2 * j + 1];
            bad |= l != l;
            low = fminf(low, l);
            high = fmaxf(high, h);
        }
        if (bad) low = high = NAN;
    }
    if (low != low) {
        a.out[i] = NAN;
        return;
    }
    const float v = clamped(a.x[(((size_t)k * a.H + y) * a.W + x) * 3 + ch], a.clamp, a.lo, a.hi);
    // make_grid's norm_ip: low and high are Python floats, so the span is formed in fp64 and handed to div_ as an fp32 scalar
    const float span = (float)fmax((double)high - (double)low, 1e-5);
    a.out[i] = (fminf(fmaxf(v, low), high) - low) / span;
}

bool grid_shape(int N, int H, int W, int* Hg, int* Wg, int* xm_out) {
    if (N < 1 || H < 1 || W < 1) return false;
    const int xm = N < 8 ? N : 8, ym = (N + xm - 1) / xm;
    const double hg = N == 1 ? H : ((double)H + 2) * ym + 2, wg = N == 1 ? W : ((double)W + 2) * xm + 2;
    if (3.0 * hg * wg >= 2147483648.0 || (double)N * H * W * 3 >= 9.0e15) return false;
    *Hg = (int)hg;
    *Wg = (int)wg;
    *xm_out = xm;
    return true;
}
size_t grid_scratch_floats(int N) { return 2 * (size_t)N; }          // grid_range_kernel leaves every image's low and high

}  // namespace

extern "C" size_t car_attention_entropy_scratch_doubles(long rows, int S) {
    if (!entropy_shape_ok(rows, S)) {
        car_set_error("car_attention_entropy_scratch_doubles: rows = %ld, S = %d, need rows >= 1 and 1 <= S <= %d", rows, S, kMaxSamples);
        return 0;
    }
    return (size_t)entropy_blocks(rows);
}

extern "C" int car_attention_entropy(const float* at_wt, long rows, int S, int nan_rows_zero, double* sum, double* scratch,
                                     size_t scratch_doubles, void* stream) {
    CAR_REQUIRE(at_wt && sum && scratch, "car_attention_entropy: null pointer");
    CAR_REQUIRE(S >= 1 && S <= kMaxSamples, "car_attention_entropy: S = %d, need 1 <= S <= %d samples per row", S, kMaxSamples);
    CAR_REQUIRE(rows >= 1, "car_attention_entropy: rows = %ld, need at least one row", rows);
    CAR_REQUIRE(entropy_shape_ok(rows, S), "car_attention_entropy: %ld x %d is too large", rows, S);
    const int blocks = entropy_blocks(rows);
    CAR_REQUIRE(scratch_doubles >= (size_t)blocks, "car_attention_entropy: scratch holds %zu doubles, need %d (car_attention_entropy_scratch_doubles)",
                scratch_doubles, blocks);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(entropy_rows_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, st, at_wt, rows, S, nan_rows_zero ? 1 : 0, scratch);
    CAR_CHECK_LAUNCH("car_attention_entropy");
    hipLaunchKernelGGL(entropy_sum_kernel, dim3(1), dim3(64), 0, st, (const double*)scratch, blocks, sum);
    CAR_CHECK_LAUNCH("car_attention_entropy");
    return CAR_OK;
}

extern "C" int car_colormap(const float* x, int N, int H, int W, float scale, const float* lut, float* out, void* stream) {
    CAR_REQUIRE(x && lut && out, "car_colormap: null pointer");
    CAR_REQUIRE(N >= 1 && H >= 1 && W >= 1, "car_colormap: %d maps of %d x %d, need N >= 1, H >= 1 and W >= 1", N, H, W);
    CAR_REQUIRE(scale == scale && scale != 0.0f && !isinf(scale), "car_colormap: scale = %g, need a finite value other than 0", (double)scale);
    const double n = (double)N * H * W;
    CAR_REQUIRE(n < 4294967296.0 * kThreads / 4, "car_colormap: %d x %d x %d is too large", N, H, W);
    const size_t count = (size_t)N * H * W;
    hipLaunchKernelGGL(colormap_kernel, dim3(car_div_up((long)count, kThreads)), dim3(kThreads), 0, (hipStream_t)stream, x, count, scale, lut, out);
    CAR_CHECK_LAUNCH("car_colormap");
    return CAR_OK;
}

extern "C" int car_epipolar_overlay(const float* trgt, const float* ctxt, const float* pixel_val, const long long* at_wt_max, const float* uv,
                                    int B, int V, int H, int W, int rays, int probe, int S, float* panel, void* stream) {
    CAR_REQUIRE(trgt && ctxt && pixel_val && at_wt_max && uv && panel, "car_epipolar_overlay: null pointer");
    CAR_REQUIRE(B >= 1 && V >= 1, "car_epipolar_overlay: B = %d, n_view = %d, need at least one scene and one view", B, V);
    CAR_REQUIRE(H >= 1 && W >= 1 && H <= 16384 && W <= 16384, "car_epipolar_overlay: %d x %d tiles, need 1 <= H, W <= 16384", H, W);
    CAR_REQUIRE(S >= 1 && S <= kMaxSamples, "car_epipolar_overlay: S = %d, need 1 <= S <= %d samples per ray", S, kMaxSamples);
    CAR_REQUIRE(rays >= 1, "car_epipolar_overlay: rays = %d, need at least one ray", rays);
    CAR_REQUIRE(probe >= 0 && probe < rays, "car_epipolar_overlay: probe ray %d of a frame with %d rays (the reference's probe is ray 2065)", probe, rays);
    CAR_REQUIRE((double)B * (1 + V) <= 65535.0, "car_epipolar_overlay: %d scenes x %d views are too many tiles", B, V);
    OverlayArgs a;
    a.trgt = trgt;
    a.ctxt = ctxt;
    a.pixel_val = pixel_val;
    a.at_wt_max = at_wt_max;
    a.uv = uv;
    a.panel = panel;
    a.B = B;
    a.V = V;
    a.H = H;
    a.W = W;
    a.rays = rays;
    a.probe = probe;
    a.S = S;
    a.pix = H / 64 + 1;                                              // summaries.py:90
    hipLaunchKernelGGL(overlay_kernel, dim3(car_div_up((long)H * W, kThreads), (unsigned)(B * (1 + V))), dim3(kThreads), 0, (hipStream_t)stream, a);
    CAR_CHECK_LAUNCH("car_epipolar_overlay");
    return CAR_OK;
}

extern "C" size_t car_image_grid_scratch_floats(int N, int H, int W) {
    int hg, wg, xm;
    if (!grid_shape(N, H, W, &hg, &wg, &xm)) {
        car_set_error("car_image_grid_scratch_floats: %d images of %d x %d, need N >= 1, H >= 1, W >= 1 and a grid below 2^31 elements", N, H, W);
        return 0;
    }
    return grid_scratch_floats(N);
}

extern "C" int car_image_grid(const float* x, int N, int H, int W, int scale_each, int clamp, float lo, float hi, float* out, float* scratch,
                              size_t scratch_floats, void* stream) {
    CAR_REQUIRE(x && out && scratch, "car_image_grid: null pointer");
    GridArgs a;
    CAR_REQUIRE(grid_shape(N, H, W, &a.Hg, &a.Wg, &a.xm),
                "car_image_grid: %d images of %d x %d, need N >= 1, H >= 1, W >= 1 and a grid below 2^31 elements", N, H, W);
    CAR_REQUIRE(N <= 65535, "car_image_grid: N = %d images are too many", N);
    CAR_REQUIRE(!clamp || lo <= hi, "car_image_grid: clamp range [%g, %g] is empty or NaN", (double)lo, (double)hi);
    CAR_REQUIRE(scratch_floats >= grid_scratch_floats(N), "car_image_grid: scratch holds %zu floats, need %zu (car_image_grid_scratch_floats)",
                scratch_floats, grid_scratch_floats(N));
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(grid_range_kernel, dim3((unsigned)N), dim3(kRangeThreads), 0, st, x, (size_t)H * W * 3, clamp ? 1 : 0, lo, hi, scratch);
    CAR_CHECK_LAUNCH("car_image_grid");
    a.x = x;
    a.range = scratch;
    a.out = out;
    a.N = N;
    a.H = H;
    a.W = W;
    a.scale_each = scale_each ? 1 : 0;
    a.clamp = clamp ? 1 : 0;
    a.lo = lo;
    a.hi = hi;
    hipLaunchKernelGGL(grid_write_kernel, dim3(car_div_up(3L * a.Hg * a.Wg, kThreads)), dim3(kThreads), 0, st, a);
    CAR_CHECK_LAUNCH("car_image_grid");
    return CAR_OK;
}

// car_metrics.hip — image metrics of the evaluation scripts (include/car_hip.h: car_ssim_scratch_doubles, car_ssim).
//
// car_ssim is the SSIM of the reference's eval_realestate10k.py:194, scikit-image 0.18.3
// structural_similarity(x, y, win_size=11, multichannel=True, gaussian_weights=True), restated on the device:
// per channel, float64 moments ux uy uxx uyy uxy through the 11-tap Gaussian (sigma 1.5, truncate 3.5) applied along axis 0 and
// then axis 1 as scipy.ndimage.gaussian_filter does, sample covariances (cov_norm = 121/120), the per-pixel S, and the mean of S
// over the pixels 5 or more away from every edge — exactly the pixels whose whole window lies inside the image, so no padding rule
// is ever read.  The image's value is the mean of its channels' means.
//
// Two launches.  ssim_tile_kernel: one workgroup per (image, channel, 32 x 16 output tile) stages the tile and its 5-pixel halo in
// LDS, runs both filter passes in fp64 and writes the sum of S over its pixels to the caller's scratch.  ssim_mean_kernel: one
// wave per image adds its tiles' sums in a fixed order.  Every sum has a fixed order, so the result is bitwise reproducible and an
// image gives the same bits alone as inside a batch.  Built with -ffp-contract=off: identical inputs must give exactly 1.0, which
// needs S's numerator and denominator evaluated in the same rounding sequence (an FMA in one and not the other breaks the tie).
#include "car_common.h"
#include <math.h>

namespace {

constexpr int kRad = 5;                          // scipy's radius int(truncate * sigma + 0.5) = int(3.5 * 1.5 + 0.5)
constexpr int kWin = 2 * kRad + 1;               // 11 taps, skimage's win_size
constexpr int kTW = 32, kTH = 16;                // output tile (columns, rows)
constexpr int kSW = kTW + 2 * kRad, kSH = kTH + 2 * kRad;
constexpr int kThreads = 256;

struct SsimArgs {
    const float* x;
    const float* y;
    double* partial;                             // [B, C, tiles_y, tiles_x] sums of S
    int H, W, C, tiles_x, tiles_y;
    double w[kRad + 1];                          // w[0] centre tap, w[j] the taps at -j and +j
    double c1, c2, cov_norm;
};

// scipy's symmetric correlate1d: centre * w[0], then the pairs from the outermost inwards
__device__ __forceinline__ double taps(const double* p, const double* w) {
    double s = p[0] * w[0];
#pragma unroll
    for (int j = kRad; j >= 1; --j) s += (p[-j] + p[j]) * w[j];
    return s;
}

__global__ __launch_bounds__(kThreads) void ssim_tile_kernel(SsimArgs a) {
    __shared__ float sx[kSH * kSW], sy[kSH * kSW];
    __shared__ double mom[5][kTH * kSW];         // axis-0 pass: ux uy uxx uyy uxy over the tile's rows and the halo's columns
    __shared__ double red[kThreads];
    const int tid = threadIdx.x;
    const int tx = blockIdx.x % a.tiles_x, ty = (blockIdx.x / a.tiles_x) % a.tiles_y;
    const int plane = blockIdx.x / (a.tiles_x * a.tiles_y);          // image * C + channel
    const int img = plane / a.C, ch = plane % a.C;
    // output pixel (oy, ox) of the cropped (H-10) x (W-10) map is image pixel (oy+5, ox+5); its window is rows oy..oy+10, cols ox..ox+10
    const int oy0 = ty * kTH, ox0 = tx * kTW;
    const int out_h = a.H - 2 * kRad, out_w = a.W - 2 * kRad;
    const size_t base = (size_t)img * a.H * a.W;

    for (int i = tid; i < kSH * kSW; i += kThreads) {
        const int r = i / kSW, c = i % kSW, gy = oy0 + r, gx = ox0 + c;
        const bool in = gy < a.H && gx < a.W;                        // outside only for pixels no kept output reads
        const size_t at = (base + (size_t)gy * a.W + gx) * a.C + ch;
        sx[i] = in ? a.x[at] : 0.0f;
        sy[i] = in ? a.y[at] : 0.0f;
    }
    __syncthreads();

    for (int i = tid; i < kTH * kSW; i += kThreads) {
        const int r = i / kSW, c = i % kSW;
        const float* px = sx + (r + kRad) * kSW + c;
        const float* py = sy + (r + kRad) * kSW + c;
        const double x0 = px[0], y0 = py[0];
        double ux = x0 * a.w[0], uy = y0 * a.w[0], uxx = (x0 * x0) * a.w[0], uyy = (y0 * y0) * a.w[0], uxy = (x0 * y0) * a.w[0];
#pragma unroll
        for (int j = kRad; j >= 1; --j) {
            const double xa = px[-j * kSW], xb = px[j * kSW], ya = py[-j * kSW], yb = py[j * kSW], wj = a.w[j];
            ux += (xa + xb) * wj;
            uy += (ya + yb) * wj;
            uxx += (xa * xa + xb * xb) * wj;
            uyy += (ya * ya + yb * yb) * wj;
            uxy += (xa * ya + xb * yb) * wj;
        }
        mom[0][i] = ux;
        mom[1][i] = uy;
        mom[2][i] = uxx;
        mom[3][i] = uyy;
        mom[4][i] = uxy;
    }
    __syncthreads();

    double acc = 0.0;
    for (int i = tid; i < kTH * kTW; i += kThreads) {
        const int r = i / kTW, c = i % kTW;
        if (oy0 + r >= out_h || ox0 + c >= out_w) continue;
        const int at = r * kSW + c + kRad;
        const double ux = taps(&mom[0][at], a.w), uy = taps(&mom[1][at], a.w);
        const double uxx = taps(&mom[2][at], a.w), uyy = taps(&mom[3][at], a.w), uxy = taps(&mom[4][at], a.w);
        // skimage 0.18.3 _structural_similarity.py, term for term and in numpy's evaluation order
        const double vx = a.cov_norm * (uxx - ux * ux);
        const double vy = a.cov_norm * (uyy - uy * uy);
        const double vxy = a.cov_norm * (uxy - ux * uy);
        const double A1 = 2.0 * ux * uy + a.c1, A2 = 2.0 * vxy + a.c2;
        const double B1 = ux * ux + uy * uy + a.c1, B2 = vx + vy + a.c2;
        acc += (A1 * A2) / (B1 * B2);
    }
    red[tid] = acc;
    __syncthreads();
    for (int s = kThreads / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    if (tid == 0) a.partial[blockIdx.x] = red[0];
}

// one wave per image: lane l adds tiles l, l + 64, ... of a channel in order, then a fixed butterfly; lane 0's result is kept
__global__ __launch_bounds__(64) void ssim_mean_kernel(const double* partial, int C, int tiles, double npix, double* mssim) {
    const int img = blockIdx.x, lane = threadIdx.x;
    double total = 0.0;
    for (int ch = 0; ch < C; ++ch) {
        const double* p = partial + ((size_t)img * C + ch) * tiles;
        double s = 0.0;
        for (int t = lane; t < tiles; t += 64) s += p[t];
        total += wave_sum(s) / npix;                                          // crop(S, 5).mean() of the channel
    }
    if (lane == 0) mssim[img] = total / C;                           // mean over the channels (multichannel=True)
}

size_t ssim_tiles(int H, int W) {
    return (size_t)((H - 2 * kRad + kTH - 1) / kTH) * ((W - 2 * kRad + kTW - 1) / kTW);
}

// the tile launch's grid is B * C * tiles workgroups of 256 lanes, and its lane count must fit the 32-bit dispatch size
bool ssim_shape_ok(int B, int H, int W, int C) {
    if (B < 1 || H < kWin || W < kWin || C < 1 || C > 4) return false;
    return (double)B * C * ssim_tiles(H, W) * kThreads < 4294967296.0;
}

}  // namespace

extern "C" size_t car_ssim_scratch_doubles(int B, int H, int W, int C) {
    return ssim_shape_ok(B, H, W, C) ? (size_t)B * C * ssim_tiles(H, W) : 0;
}

extern "C" int car_ssim(const float* x, const float* y, int B, int H, int W, int C, double data_range, double* mssim, double* scratch,
                        size_t scratch_doubles, void* stream) {
    CAR_REQUIRE(x && y && mssim && scratch, "car_ssim: null pointer");
    CAR_REQUIRE(B >= 1, "car_ssim: B = %d, need at least one image pair", B);
    CAR_REQUIRE(H >= kWin && W >= kWin, "car_ssim: %d x %d image, the 11 x 11 window needs H >= 11 and W >= 11", H, W);
    CAR_REQUIRE(C >= 1 && C <= 4, "car_ssim: C = %d, need 1 to 4 channels", C);
    CAR_REQUIRE(data_range > 0.0 && isfinite(data_range), "car_ssim: data_range = %g, need a finite value > 0", data_range);
    CAR_REQUIRE(ssim_shape_ok(B, H, W, C), "car_ssim: %d x %d x %d x %d is too large", B, H, W, C);
    const size_t need = car_ssim_scratch_doubles(B, H, W, C);
    CAR_REQUIRE(scratch_doubles >= need, "car_ssim: scratch holds %zu doubles, need %zu (car_ssim_scratch_doubles)", scratch_doubles, need);

    SsimArgs a;
    a.x = x;
    a.y = y;
    a.partial = scratch;
    a.H = H;
    a.W = W;
    a.C = C;
    a.tiles_x = (W - 2 * kRad + kTW - 1) / kTW;
    a.tiles_y = (H - 2 * kRad + kTH - 1) / kTH;
    // scipy.ndimage._gaussian_kernel1d(1.5, 0, 5): exp(-0.5 / sigma^2 * k^2) normalised to sum 1
    double g[kWin], sum = 0.0;
    for (int k = -kRad; k <= kRad; ++k) sum += (g[k + kRad] = exp(-0.5 / (1.5 * 1.5) * (double)(k * k)));
    for (int j = 0; j <= kRad; ++j) a.w[j] = g[kRad + j] / sum;
    a.c1 = (0.01 * data_range) * (0.01 * data_range);
    a.c2 = (0.03 * data_range) * (0.03 * data_range);
    a.cov_norm = (double)(kWin * kWin) / (double)(kWin * kWin - 1);

    hipStream_t st = (hipStream_t)stream;
    const int tiles = a.tiles_x * a.tiles_y;
    hipLaunchKernelGGL(ssim_tile_kernel, dim3((unsigned)((long)B * C * tiles)), dim3(kThreads), 0, st, a);
    CAR_CHECK_LAUNCH("car_ssim");
    hipLaunchKernelGGL(ssim_mean_kernel, dim3((unsigned)B), dim3(64), 0, st, (const double*)scratch, C, tiles,
                       (double)(H - 2 * kRad) * (double)(W - 2 * kRad), mssim);
    CAR_CHECK_LAUNCH("car_ssim");
    return CAR_OK;
}

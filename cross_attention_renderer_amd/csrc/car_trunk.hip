// car_trunk.hip — what stands in front of the transformer blocks in get_z's image encoder (include/car_trunk.h; encoder.py ResNetV2Trunk and the
// token lines of MultiViewDPTEncoder.forward): the weight standardisation of timm's StdConv2dSame (once, at pack time, in fp64),
// the 7x7 stem, GroupNorm with an optional residual and ReLU, the SAME max-pool, the strided 3x3 convolution with TF "SAME" padding, the
// pixel copy of a stride-2 1x1 convolution, the trunk as a sequence of these entries and car_linear_x3, and the assembly of the token rows
// car_vit_blocks reads.  Inference only.  Activations are channel-last fp32 rows [n][H W][C].
//
// The two dense convolutions are car_conv.hip's: the 3x3 one is conv3x3_kernel in its general form (car_conv3x3_general) with the padding
// of TF "SAME" and no bias, residual or activation, the stem conv7x7_kernel at stride 2 (car_conv7x7); this unit works out the padding
// and the output's extents.
// GroupNorm's statistics are two passes in fp64 (the mean, then the squared distances from it), each split over slabs of pixels whose partial
// sums are combined in one fixed order by every reader: no atomics, an image's result does not depend on the other images of the call.
#include "car_common.h"
#include <math.h>
#include <stdint.h>

namespace {

constexpr long kMaxPixels = 1L << 27;              // n H W: keeps every row count, grid and per-image offset far inside 32 bits
constexpr int kMaxImages = 65535;

// TF "SAME": total padding max((ceil(i / s) - 1) s + k - i, 0), the odd pixel behind
inline int same_out(int i, int s) { return (i + s - 1) / s; }
inline int same_pad_front(int i, int k, int s) {
    const int total = (same_out(i, s) - 1) * s + k - i;
    return total > 0 ? total / 2 : 0;
}

// ---- weight standardisation: one workgroup per output channel, fp64 ------------------------------------------------------------------
__device__ __forceinline__ double block_sum256(double v, double* red) {              // fixed order: the butterfly, then waves 0..3
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}
__global__ void __launch_bounds__(256) weight_std_kernel(const float* __restrict__ w, int fan_in, double eps, float* __restrict__ out) {
    __shared__ double red[4];
    const float* row = w + (long)blockIdx.x * fan_in;
    double s = 0.0;
    for (int i = threadIdx.x; i < fan_in; i += 256) s += (double)row[i];
    const double mean = block_sum256(s, red) / (double)fan_in;
    double q = 0.0;
    for (int i = threadIdx.x; i < fan_in; i += 256) { const double d = (double)row[i] - mean; q += d * d; }
    const double rstd = 1.0 / sqrt(block_sum256(q, red) / (double)fan_in + eps);
    for (int i = threadIdx.x; i < fan_in; i += 256) out[(long)blockIdx.x * fan_in + i] = (float)(((double)row[i] - mean) * rstd);
}

// ---- GroupNorm ------------------------------------------------------------------------------------------------------------------------
// A workgroup = one slab of an image: kGnVec float4 of it, i.e. 4 kGnVec / C pixels over all C channels.  Thread t owns float4 column
// t % (C / 4) in every pass (C / 4 divides 256), so its fp64 sums belong to one group — or, where a group is two channels wide, to the two
// groups its float4 spans (acc[0]: .x .y, acc[1]: .z .w).  The threads' sums meet in LDS and one thread per group adds them in thread order.
constexpr int kGnVec = 2048;
struct GnArgs {
    const float* X; const float* gamma; const float* beta; const float* add; float* Y;
    double* psum; double* psq;             // [n][groups][slabs]
    int HW, C, groups, slabs, slab_rows, relu;
    double eps;
};
inline int gn_slab_rows(int C) { return kGnVec / (C / 4); }
// this thread's sums of f(x) over its column of the slab -> the groups' sums of the slab, into dst[(img groups + g) slabs + slab]
template <class F>
__device__ __forceinline__ void gn_slab_reduce(const GnArgs& a, double (*lds)[2], double* dst, F f) {
    const int C4 = a.C >> 2, cpg = a.C / a.groups;
    const int slab = blockIdx.x % a.slabs, img = blockIdx.x / a.slabs;
    const int c4 = threadIdx.x % C4, rsub = threadIdx.x / C4, rstep = 256 / C4;
    const int r0 = slab * a.slab_rows, r1 = min(r0 + a.slab_rows, a.HW);
    const float4* x = reinterpret_cast<const float4*>(a.X) + ((long)img * a.HW) * C4 + c4;
    double acc[2] = {0.0, 0.0};
    for (int r = r0 + rsub; r < r1; r += rstep) {
        const float4 v = x[(long)r * C4];
        const double s01 = f((double)v.x, 0) + f((double)v.y, 0), s23 = f((double)v.z, 1) + f((double)v.w, 1);
        if (cpg == 2) { acc[0] += s01; acc[1] += s23; }
        else acc[0] += s01 + s23;
    }
    lds[threadIdx.x][0] = acc[0]; lds[threadIdx.x][1] = acc[1];
    __syncthreads();
    for (int g = threadIdx.x; g < a.groups; g += 256) {
        const int first = (g * cpg) >> 2, width = cpg == 2 ? 1 : cpg >> 2, half = cpg == 2 ? (g & 1) : 0;
        double s = 0.0;
        for (int r = 0; r < rstep; ++r)
            for (int j = 0; j < width; ++j) s += lds[r * C4 + first + j][half];
        dst[((long)img * a.groups + g) * a.slabs + slab] = s;
    }
}
// The totals of one partial array for every group of image img, into out[groups] (LDS).  A group's slabs are added by 256 / min(groups, 256)
// threads, each over its own stride in slab order, and one thread adds those sums in thread order: a fixed order, the same in every
// workgroup that asks — and a chain of slabs / 8 dependent additions per thread at 32 groups, not of all the slabs
__device__ __forceinline__ void gn_totals(const double* __restrict__ part, int img, int groups, int slabs, double* tmp, double* out) {
    const int gc = groups < 256 ? groups : 256, per = 256 / gc;
    for (int gb = 0; gb < groups; gb += gc) {
        const int g = gb + threadIdx.x / per, j = threadIdx.x % per;
        const double* p = part + ((long)img * groups + g) * slabs;
        double s = 0.0;
        for (int i = j; i < slabs; i += per) s += p[i];
        tmp[threadIdx.x] = s;
        __syncthreads();
        if (j == 0) {
            double t = 0.0;
            for (int k = 0; k < per; ++k) t += tmp[threadIdx.x + k];
            out[g] = t;
        }
        __syncthreads();
    }
}
constexpr int kGnMaxGroups = 512;                  // C / 2 at C = 1024
__global__ void __launch_bounds__(256) gn_sum_kernel(const GnArgs a) {
    __shared__ double lds[256][2];
    gn_slab_reduce(a, lds, a.psum, [](double v, int) { return v; });
}
__global__ void __launch_bounds__(256) gn_sq_kernel(const GnArgs a) {
    __shared__ double lds[256][2];
    __shared__ double tot[kGnMaxGroups];
    const int C4 = a.C >> 2, cpg = a.C / a.groups, img = blockIdx.x / a.slabs, c4 = threadIdx.x % C4;
    gn_totals(a.psum, img, a.groups, a.slabs, &lds[0][0], tot);
    const double count = (double)a.HW * cpg;
    const int g0 = (4 * c4) / cpg;
    const double m0 = tot[g0] / count, m1 = cpg == 2 ? tot[g0 + 1] / count : m0;
    gn_slab_reduce(a, lds, a.psq, [m0, m1](double v, int h) { const double d = v - (h ? m1 : m0); return d * d; });
}
__global__ void __launch_bounds__(256) gn_apply_kernel(const GnArgs a) {
    __shared__ double tmp[256];
    __shared__ double tot[kGnMaxGroups], totq[kGnMaxGroups];
    const int C4 = a.C >> 2, cpg = a.C / a.groups;
    const int slab = blockIdx.x % a.slabs, img = blockIdx.x / a.slabs;
    const int c4 = threadIdx.x % C4, rsub = threadIdx.x / C4, rstep = 256 / C4;
    gn_totals(a.psum, img, a.groups, a.slabs, tmp, tot);
    gn_totals(a.psq, img, a.groups, a.slabs, tmp, totq);
    const double count = (double)a.HW * cpg;
    const int g0 = (4 * c4) / cpg, g1 = cpg == 2 ? g0 + 1 : g0;
    const double mean[2] = {tot[g0] / count, tot[g1] / count};
    const double rstd[2] = {1.0 / sqrt(totq[g0] / count + a.eps), 1.0 / sqrt(totq[g1] / count + a.eps)};
    const float4 g = reinterpret_cast<const float4*>(a.gamma)[c4], b = reinterpret_cast<const float4*>(a.beta)[c4];
    const int r0 = slab * a.slab_rows, r1 = min(r0 + a.slab_rows, a.HW);
    const long base = ((long)img * a.HW) * C4 + c4;
    for (int r = r0 + rsub; r < r1; r += rstep) {
        const long at = base + (long)r * C4;
        const float4 v = reinterpret_cast<const float4*>(a.X)[at];
        float4 o;
        o.x = fmaf((float)(((double)v.x - mean[0]) * rstd[0]), g.x, b.x);
        o.y = fmaf((float)(((double)v.y - mean[0]) * rstd[0]), g.y, b.y);
        o.z = fmaf((float)(((double)v.z - mean[1]) * rstd[1]), g.z, b.z);
        o.w = fmaf((float)(((double)v.w - mean[1]) * rstd[1]), g.w, b.w);
        if (a.add) {
            const float4 d = reinterpret_cast<const float4*>(a.add)[at];
            o.x += d.x; o.y += d.y; o.z += d.z; o.w += d.w;
        }
        if (a.relu) {                                                  // a NaN stays a NaN, as F.relu leaves it
            o.x = o.x < 0.0f ? 0.0f : o.x; o.y = o.y < 0.0f ? 0.0f : o.y; o.z = o.z < 0.0f ? 0.0f : o.z; o.w = o.w < 0.0f ? 0.0f : o.w;
        }
        reinterpret_cast<float4*>(a.Y)[at] = o;
    }
}
struct GnLayout { double *psum, *psq; size_t total; int slabs; };
GnLayout gn_layout(int n, int HW, int C, int groups, void* work = nullptr) {
    const int slabs = (HW + gn_slab_rows(C) - 1) / gn_slab_rows(C);
    const size_t each = (size_t)n * groups * slabs;
    Carver c(work, 8);
    return {c.take<double>(each), c.take<double>(each), c.bytes(), slabs};
}
bool gn_shape_ok(int n, int HW, int C, int groups, const char* who) {
    if (n < 1 || n > kMaxImages || HW < 1 || (double)n * HW > (double)kMaxPixels) {
        car_set_error("%s: %d images of %d pixels, need 1..%d images and at most 2^27 pixels in all", who, n, HW, kMaxImages);
        return false;
    }
    if (C < 8 || C > 1024 || (C & (C - 1))) { car_set_error("%s: C = %d must be a power of two in 8..1024", who, C); return false; }
    if (groups < 1 || C % groups) { car_set_error("%s: %d groups do not divide C = %d", who, groups, C); return false; }
    const int cpg = C / groups;
    if (cpg != 2 && cpg % 4) { car_set_error("%s: %d channels per group, need 2 or a multiple of 4", who, cpg); return false; }
    return true;
}

// ---- 3x3 max-pool, stride 2, SAME with -inf: the maximum over the window's taps inside the image ---------------------------------------
__device__ __forceinline__ float max_nan(float m, float v) { return (v > m || v != v) ? v : m; }     // a NaN is taken and then kept
__global__ void __launch_bounds__(256) maxpool_same_kernel(const float* __restrict__ X, float* __restrict__ Y, int H, int W, int Ho, int Wo, int pt,
                                                           int pl, int C4, long total) {
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int c = (int)(idx % C4);
        long r = idx / C4;
        const int ox = (int)(r % Wo); r /= Wo;
        const int oy = (int)(r % Ho);
        const long img = r / Ho;
        float4 m = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int iy = 2 * oy + t / 3 - pt, ix = 2 * ox + t % 3 - pl;
            if ((unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W) {
                const float4 v = reinterpret_cast<const float4*>(X)[((img * H + iy) * W + ix) * C4 + c];
                m.x = max_nan(m.x, v.x); m.y = max_nan(m.y, v.y); m.z = max_nan(m.z, v.z); m.w = max_nan(m.w, v.w);
            }
        }
        reinterpret_cast<float4*>(Y)[idx] = m;
    }
}

// ---- the pixels at even coordinates ----------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) pixels_stride2_kernel(const float* __restrict__ X, float* __restrict__ Y, int H, int W, int Ho, int Wo, int C4,
                                                             long total) {
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int c = (int)(idx % C4);
        long r = idx / C4;
        const int ox = (int)(r % Wo); r /= Wo;
        const int oy = (int)(r % Ho);
        const long img = r / Ho;
        reinterpret_cast<float4*>(Y)[idx] = reinterpret_cast<const float4*>(X)[((img * H + 2 * oy) * W + 2 * ox) * C4 + c];
    }
}

// ---- the convolutions (car_conv.hip) -----------------------------------------------------------------------------------------------------
constexpr int kStemTerms = 147;                    // the stem's 3 x 7 x 7 weights per output channel
bool same_width_ok(int c) { return c == 64 || c == 128 || c == 256; }

// ---- the trunk's layout ----------------------------------------------------------------------------------------------------------------
constexpr int kStages = 3, kMaxDepth = 16, kGroups = 32;
constexpr int kStageOut[kStages] = {256, 512, 1024};
constexpr double kGnEps = 1e-5, kStemEps = 1e-6, kStageEps = 1e-8;
bool depths_ok(const int* depths, const char* who) {
    if (!depths) { car_set_error("%s: null pointer", who); return false; }
    for (int s = 0; s < kStages; ++s)
        if (depths[s] < 1 || depths[s] > kMaxDepth) { car_set_error("%s: depth %d of stage %d is outside 1..%d", who, depths[s], s, kMaxDepth); return false; }
    return true;
}
int trunk_param_count(const int* depths) {
    int n = 3;
    for (int s = 0; s < kStages; ++s) n += 9 * depths[s] + 3;
    return n;
}
// one block's packed items (offsets in floats from the start of car_trunk_pack's array)
struct BlockPack { size_t down_w, down_g, down_b, w1, g1, b1, w2, g2, b2, w3, g3, b3; int cin, mid, cout, stride; bool project; };
struct TrunkPack { size_t stem_w, stem_g, stem_b; BlockPack blk[kStages * kMaxDepth]; int blocks; size_t scratch, floats; };
TrunkPack trunk_pack_layout(const int* depths) {
    TrunkPack t{};
    Carver c(nullptr, 4);
    t.stem_w = c.at<float>(64 * kStemTerms); t.stem_g = c.at<float>(64); t.stem_b = c.at<float>(64);
    int cin = 64;
    for (int s = 0; s < kStages; ++s)
        for (int i = 0; i < depths[s]; ++i) {
            BlockPack& b = t.blk[t.blocks++];
            b.cin = cin; b.cout = kStageOut[s]; b.mid = b.cout / 4; b.stride = (i == 0 && s > 0) ? 2 : 1; b.project = i == 0;
            if (b.project) {
                b.down_w = c.at<float>(car_linear_x3_packed_floats(b.cin, b.cout)); b.down_g = c.at<float>(b.cout); b.down_b = c.at<float>(b.cout);
            }
            b.w1 = c.at<float>(car_linear_x3_packed_floats(b.cin, b.mid)); b.g1 = c.at<float>(b.mid); b.b1 = c.at<float>(b.mid);
            b.w2 = c.at<float>(car_conv3x3_tile_floats(b.mid, b.mid) + 64); b.g2 = c.at<float>(b.mid); b.b2 = c.at<float>(b.mid);
            b.w3 = c.at<float>(car_linear_x3_packed_floats(b.mid, b.cout)); b.g3 = c.at<float>(b.cout); b.b3 = c.at<float>(b.cout);
            cin = b.cout;
        }
    t.scratch = c.at<float>((size_t)9 * 256 * 256);                    // the packer's own: a standardised weight on its way to its packer
    t.floats = c.bytes() / sizeof(float);
    return t;
}
// car_trunk_forward's workspace: two maps a block's result alternates between (the stem's too), the shortcut, the two narrow maps of a
// block (the second one also holds the strided pixels of a projecting shortcut), then car_groupnorm's workspace as a nested range
struct TrunkWork { float *u, *v, *sc, *ma, *mb; void* gn; size_t gn_bytes, total; };
TrunkWork trunk_work(int n, int H, int W, const int* depths, void* work = nullptr) {
    size_t u = 0, sc = 0, ma = 0, mb = 0, gn = 0;
    auto need = [](size_t& slot, size_t v) { if (slot < v) slot = v; };
    int h = same_out(H, 2), w = same_out(W, 2);
    need(u, (size_t)n * h * w * 64); need(gn, gn_layout(n, h * w, 64, kGroups).total);
    h = same_out(h, 2); w = same_out(w, 2);
    need(u, (size_t)n * h * w * 64);
    int cin = 64;
    for (int s = 0; s < kStages; ++s)
        for (int i = 0; i < depths[s]; ++i) {
            const int cout = kStageOut[s], mid = cout / 4, stride = (i == 0 && s > 0) ? 2 : 1;
            const int ho = same_out(h, stride), wo = same_out(w, stride);
            need(ma, (size_t)n * h * w * mid); need(gn, gn_layout(n, h * w, mid, kGroups).total);
            need(mb, (size_t)n * ho * wo * mid); need(gn, gn_layout(n, ho * wo, mid, kGroups).total);
            if (i == 0) { need(sc, (size_t)n * ho * wo * cout); need(mb, (size_t)n * ho * wo * cin); }
            need(u, (size_t)n * ho * wo * cout); need(gn, gn_layout(n, ho * wo, cout, kGroups).total);
            h = ho; w = wo; cin = cout;
        }
    Carver c(work, 64);
    TrunkWork t;
    t.u = c.take<float>(u); t.v = c.take<float>(u); t.sc = c.take<float>(sc); t.ma = c.take<float>(ma); t.mb = c.take<float>(mb);
    t.gn = c.sub(gn).take<double>(gn / sizeof(double));
    t.gn_bytes = gn; t.total = c.bytes();
    return t;
}
bool trunk_shape_ok(int n, int H, int W, const char* who) {
    if (n < 1 || n > kMaxImages || H < 1 || W < 1 || (double)n * H * W > (double)kMaxPixels) {
        car_set_error("%s: %d images of %d x %d, need 1..%d images of at least one pixel and at most 2^27 pixels in all", who, n, H, W, kMaxImages);
        return false;
    }
    return true;
}

// ---- the token rows ----------------------------------------------------------------------------------------------------------------------
constexpr int kTokDim = 768, kTokIn = 1024, kMaxGrid = 64;
struct TokPack { size_t proj, bias, cls, pos, pose_w, pose_b, floats; };
TokPack tok_pack_layout(int gh, int gw) {
    TokPack t;
    Carver c(nullptr, 4);
    t.proj = c.at<float>(car_linear_x3_packed_floats(kTokIn, kTokDim)); t.bias = c.at<float>(kTokDim); t.cls = c.at<float>(kTokDim);
    t.pos = c.at<float>((size_t)(1 + gh * gw) * kTokDim); t.pose_w = c.at<float>(16 * kTokDim); t.pose_b = c.at<float>(kTokDim);
    t.floats = c.bytes() / sizeof(float);
    return t;
}
struct TokWork { float *proj, *pose; size_t total; };
TokWork tok_work(int BV, int gh, int gw, void* work = nullptr) {
    Carver c(work, 64);
    TokWork t;
    t.proj = c.take<float>((size_t)BV * gh * gw * kTokDim); t.pose = c.take<float>((size_t)BV * kTokDim);
    t.total = c.bytes();
    return t;
}
bool tok_shape_ok(int gh, int gw, const char* who) {
    if (gh < 1 || gh > kMaxGrid || gw < 1 || gw > kMaxGrid) { car_set_error("%s: a grid of %d x %d patches is outside 1..%d", who, gh, gw, kMaxGrid); return false; }
    return true;
}
// the position embedding's grid entries, bilinear from grid x grid to gh x gw with align_corners = False (F.interpolate as
// MultiViewViT.resized_pos_embed calls it): source coordinate max((d + 0.5) grid / g - 0.5, 0); fp64, rounded once.  Entry 0 is copied.
__global__ void __launch_bounds__(256) pos_resize_kernel(const float* __restrict__ pos, int grid, int gh, int gw, float* __restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)(1 + gh * gw) * kTokDim) return;
    const int c = (int)(i % kTokDim), r = (int)(i / kTokDim);
    if (r == 0) { out[i] = pos[c]; return; }
    const int oy = (r - 1) / gw, ox = (r - 1) % gw;
    const double sy = fmax(((double)oy + 0.5) * ((double)grid / gh) - 0.5, 0.0), sx = fmax(((double)ox + 0.5) * ((double)grid / gw) - 0.5, 0.0);
    const int y0 = min((int)sy, grid - 1), x0 = min((int)sx, grid - 1), y1 = min(y0 + 1, grid - 1), x1 = min(x0 + 1, grid - 1);
    const double ly = sy - y0, lx = sx - x0;
    auto at = [&](int y, int x) { return (double)pos[(long)(1 + y * grid + x) * kTokDim + c]; };
    out[i] = (float)((1.0 - ly) * ((1.0 - lx) * at(y0, x0) + lx * at(y0, x1)) + ly * ((1.0 - lx) * at(y1, x0) + lx * at(y1, x1)));
}
// pose_embed: Linear(16, 768) of a view's pose, the 16 terms then the bias in fp64, rounded once
__global__ void __launch_bounds__(256) pose_embed_kernel(const float* __restrict__ pose16, const float* __restrict__ w, const float* __restrict__ b, int BV,
                                                         float* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= BV * kTokDim) return;
    const int c = i % kTokDim, v = i / kTokDim;
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 16; ++k) s += (double)pose16[v * 16 + k] * (double)w[c * 16 + k];
    out[i] = (float)(s + (double)b[c]);
}
// tok[v][0] = (cls + pos[0]) + pose[v]; tok[v][1 + p] = (proj[v][p] + pos[1 + p]) + pose[v], proj with its bias already in
__global__ void __launch_bounds__(256) tokens_kernel(const float* __restrict__ proj, const float* __restrict__ cls, const float* __restrict__ pos,
                                                     const float* __restrict__ pose, int T, long total4, float* __restrict__ tok) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total4) return;
    constexpr int D4 = kTokDim / 4;
    const int c = (int)(i % D4), r = (int)((i / D4) % T);
    const long v = i / ((long)D4 * T);
    const float4 a = r == 0 ? reinterpret_cast<const float4*>(cls)[c] : reinterpret_cast<const float4*>(proj)[(v * (T - 1) + r - 1) * D4 + c];
    const float4 p = reinterpret_cast<const float4*>(pos)[(long)r * D4 + c], e = reinterpret_cast<const float4*>(pose)[v * D4 + c];
    reinterpret_cast<float4*>(tok)[i] = make_float4((a.x + p.x) + e.x, (a.y + p.y) + e.y, (a.z + p.z) + e.z, (a.w + p.w) + e.w);
}

unsigned grid_for(long total) { const long blocks = (total + 255) / 256; return (unsigned)(blocks < 65536 ? blocks : 65536); }

}  // namespace

extern "C" int car_weight_standardize(const float* w, int N, int fan_in, double eps, float* out, void* stream) {
    CAR_REQUIRE(w && out, "car_weight_standardize: null pointer");
    CAR_REQUIRE(N >= 1 && N <= (1 << 20) && fan_in >= 1 && fan_in <= (1 << 24) && eps >= 0.0,
                "car_weight_standardize: bad sizes (N = %d, fan_in = %d, eps = %g)", N, fan_in, eps);
    CAR_REQUIRE(aligned16(w) && aligned16(out), "car_weight_standardize: w and out must be 16-byte aligned");
    (void)hipGetLastError();
    hipLaunchKernelGGL(weight_std_kernel, dim3((unsigned)N), dim3(256), 0, (hipStream_t)stream, w, fan_in, eps, out);
    CAR_CHECK_LAUNCH("car_weight_standardize");
    return CAR_OK;
}

extern "C" int car_stem7x7(const float* x, int n, int H, int W, const float* w_std, float* Y, void* stream) {
    CAR_REQUIRE(x && w_std && Y, "car_stem7x7: null pointer");
    if (!trunk_shape_ok(n, H, W, "car_stem7x7")) return CAR_E_ARG;
    CAR_REQUIRE(aligned16(x) && aligned16(w_std) && aligned16(Y), "car_stem7x7: x, w_std and Y must be 16-byte aligned");
    return car_conv7x7("car_stem7x7", x, n, H, W, 2, same_pad_front(H, 7, 2), same_pad_front(W, 7, 2), same_out(H, 2), same_out(W, 2), w_std, nullptr, Y,
                       (hipStream_t)stream);
}

extern "C" size_t car_groupnorm_workspace_bytes(int n, int HW, int C, int groups) {
    return gn_shape_ok(n, HW, C, groups, "car_groupnorm_workspace_bytes") ? gn_layout(n, HW, C, groups).total : 0;
}

extern "C" int car_groupnorm(const float* X, int n, int HW, int C, int groups, const float* gamma, const float* beta, double eps, const float* add,
                             int flags, float* Y, void* work, size_t work_bytes, void* stream) {
    CAR_REQUIRE(X && gamma && beta && Y && work, "car_groupnorm: null pointer");
    if (!gn_shape_ok(n, HW, C, groups, "car_groupnorm")) return CAR_E_ARG;
    CAR_REQUIRE(eps >= 0.0 && (flags & ~CAR_GN_RELU) == 0, "car_groupnorm: bad eps (%g) or flags (%d: CAR_GN_RELU or 0)", eps, flags);
    CAR_REQUIRE(aligned16(X) && aligned16(gamma) && aligned16(beta) && aligned16(add) && aligned16(Y) && aligned16(work),
                "car_groupnorm: X, gamma, beta, add, Y and work must be 16-byte aligned");
    const GnLayout l = gn_layout(n, HW, C, groups, work);
    CAR_REQUIRE(work_bytes >= l.total, "car_groupnorm: the workspace is too small (%zu bytes, car_groupnorm_workspace_bytes says %zu)", work_bytes, l.total);
    GnArgs a{X, gamma, beta, add, Y, l.psum, l.psq, HW, C, groups, l.slabs, gn_slab_rows(C), (flags & CAR_GN_RELU) != 0, eps};
    hipStream_t st = (hipStream_t)stream;
    const unsigned blocks = (unsigned)((long)n * l.slabs);
    (void)hipGetLastError();
    hipLaunchKernelGGL(gn_sum_kernel, dim3(blocks), dim3(256), 0, st, a);
    hipLaunchKernelGGL(gn_sq_kernel, dim3(blocks), dim3(256), 0, st, a);
    hipLaunchKernelGGL(gn_apply_kernel, dim3(blocks), dim3(256), 0, st, a);
    CAR_CHECK_LAUNCH("car_groupnorm");
    return CAR_OK;
}

extern "C" int car_maxpool3x3s2_same(const float* X, int n, int H, int W, int C, float* Y, void* stream) {
    CAR_REQUIRE(X && Y, "car_maxpool3x3s2_same: null pointer");
    if (!trunk_shape_ok(n, H, W, "car_maxpool3x3s2_same")) return CAR_E_ARG;
    CAR_REQUIRE(C >= 4 && C <= 4096 && C % 4 == 0, "car_maxpool3x3s2_same: C = %d must be a multiple of 4 in 4..4096", C);
    CAR_REQUIRE(aligned16(X) && aligned16(Y), "car_maxpool3x3s2_same: X and Y must be 16-byte aligned");
    const int Ho = same_out(H, 2), Wo = same_out(W, 2);
    const long total = (long)n * Ho * Wo * (C / 4);
    (void)hipGetLastError();
    hipLaunchKernelGGL(maxpool_same_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, X, Y, H, W, Ho, Wo, same_pad_front(H, 3, 2),
                       same_pad_front(W, 3, 2), C / 4, total);
    CAR_CHECK_LAUNCH("car_maxpool3x3s2_same");
    return CAR_OK;
}

extern "C" int car_pixels_stride2(const float* X, int n, int H, int W, int C, float* Y, void* stream) {
    CAR_REQUIRE(X && Y, "car_pixels_stride2: null pointer");
    if (!trunk_shape_ok(n, H, W, "car_pixels_stride2")) return CAR_E_ARG;
    CAR_REQUIRE(C >= 4 && C <= 4096 && C % 4 == 0, "car_pixels_stride2: C = %d must be a multiple of 4 in 4..4096", C);
    CAR_REQUIRE(aligned16(X) && aligned16(Y), "car_pixels_stride2: X and Y must be 16-byte aligned");
    const int Ho = same_out(H, 2), Wo = same_out(W, 2);
    const long total = (long)n * Ho * Wo * (C / 4);
    (void)hipGetLastError();
    hipLaunchKernelGGL(pixels_stride2_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, X, Y, H, W, Ho, Wo, C / 4, total);
    CAR_CHECK_LAUNCH("car_pixels_stride2");
    return CAR_OK;
}

// the packed 3x3 layer: car_conv3x3's tiles — 9 K / 32 x N / 16 tiles of 512 floats, [K step][tile][hi | lo][lane][8 halves] with
// k = tap * K + channel — then 64 floats of scale (2^shift, 2^-shift, the largest magnitude, zeros).  No bias.
extern "C" size_t car_conv3x3_same_packed_floats(int K, int N) {
    if (!same_width_ok(K) || !same_width_ok(N)) { car_set_error("car_conv3x3_same_packed_floats: %d -> %d channels, need K and N among 64, 128, 256", K, N); return 0; }
    return car_conv3x3_tile_floats(K, N) + 64;
}

extern "C" int car_conv3x3_same_pack(const float* w_std, int K, int N, float* packed, void* stream) {
    CAR_REQUIRE(w_std && packed, "car_conv3x3_same_pack: null pointer");
    CAR_REQUIRE(same_width_ok(K) && same_width_ok(N), "car_conv3x3_same_pack: %d -> %d channels, need K and N among 64, 128, 256", K, N);
    CAR_REQUIRE(aligned16(w_std) && aligned16(packed), "car_conv3x3_same_pack: w_std and packed must be 16-byte aligned");
    return car_conv3x3_pack_tiles("car_conv3x3_same_pack", w_std, nullptr, K, N, false, packed, (hipStream_t)stream);
}

extern "C" int car_conv3x3_same(const float* X, int n, int H, int W, int K, int N, int stride, const float* packed, float* Y, void* stream) {
    CAR_REQUIRE(X && packed && Y, "car_conv3x3_same: null pointer");
    CAR_REQUIRE(same_width_ok(K) && same_width_ok(N), "car_conv3x3_same: %d -> %d channels, need K and N among 64, 128, 256", K, N);
    CAR_REQUIRE(stride == 1 || stride == 2, "car_conv3x3_same: stride = %d, need 1 or 2", stride);
    if (!trunk_shape_ok(n, H, W, "car_conv3x3_same")) return CAR_E_ARG;
    CAR_REQUIRE(aligned16(X) && aligned16(packed) && aligned16(Y), "car_conv3x3_same: X, packed and Y must be 16-byte aligned");
    return car_conv3x3_general("car_conv3x3_same", false, X, n, H, W, K, N, stride, same_pad_front(H, 3, stride), same_pad_front(W, 3, stride), same_out(H, stride),
                               same_out(W, stride), packed, nullptr, nullptr, 0, Y, (hipStream_t)stream);
}

extern "C" size_t car_trunk_packed_floats(const int* depths) {
    return depths_ok(depths, "car_trunk_packed_floats") ? trunk_pack_layout(depths).floats : 0;
}

extern "C" int car_trunk_pack(const float* const* params, int n_params, const int* depths, float* packed, void* stream) {
    CAR_REQUIRE(params && packed, "car_trunk_pack: null pointer");
    if (!depths_ok(depths, "car_trunk_pack")) return CAR_E_ARG;
    CAR_REQUIRE(n_params == trunk_param_count(depths), "car_trunk_pack: %d parameter arrays do not fit depths (%d, %d, %d), which have %d", n_params,
                depths[0], depths[1], depths[2], trunk_param_count(depths));
    for (int i = 0; i < n_params; ++i) {
        CAR_REQUIRE(params[i], "car_trunk_pack: null pointer (parameter %d)", i);
        CAR_REQUIRE(aligned16(params[i]), "car_trunk_pack: parameter %d must be 16-byte aligned", i);
    }
    CAR_REQUIRE(aligned16(packed), "car_trunk_pack: packed must be 16-byte aligned");
    const TrunkPack t = trunk_pack_layout(depths);
    hipStream_t st = (hipStream_t)stream;
    float* scratch = packed + t.scratch;
    int at = 0;
    auto vec = [&](size_t off, int count) -> int {
        CAR_CHECK_HIP(hipMemcpyAsync(packed + off, params[at++], sizeof(float) * count, hipMemcpyDeviceToDevice, st), "car_trunk_pack: copy failed");
        return CAR_OK;
    };
    auto lin = [&](size_t off, int K, int N) -> int {                    // a 1x1 layer: standardised, then laid out for car_linear_x3
        CAR_TRY(car_weight_standardize(params[at++], N, K, kStageEps, scratch, stream));
        return car_linear_x3_pack(scratch, K, K, N, packed + off, stream);
    };
    CAR_TRY(car_weight_standardize(params[at++], 64, kStemTerms, kStemEps, packed + t.stem_w, stream));
    CAR_TRY(vec(t.stem_g, 64)); CAR_TRY(vec(t.stem_b, 64));
    for (int i = 0; i < t.blocks; ++i) {
        const BlockPack& b = t.blk[i];
        if (b.project) { CAR_TRY(lin(b.down_w, b.cin, b.cout)); CAR_TRY(vec(b.down_g, b.cout)); CAR_TRY(vec(b.down_b, b.cout)); }
        CAR_TRY(lin(b.w1, b.cin, b.mid)); CAR_TRY(vec(b.g1, b.mid)); CAR_TRY(vec(b.b1, b.mid));
        CAR_TRY(car_weight_standardize(params[at++], b.mid, 9 * b.mid, kStageEps, scratch, stream));
        CAR_TRY(car_conv3x3_same_pack(scratch, b.mid, b.mid, packed + b.w2, stream));
        CAR_TRY(vec(b.g2, b.mid)); CAR_TRY(vec(b.b2, b.mid));
        CAR_TRY(lin(b.w3, b.mid, b.cout)); CAR_TRY(vec(b.g3, b.cout)); CAR_TRY(vec(b.b3, b.cout));
    }
    return CAR_OK;
}

extern "C" size_t car_trunk_workspace_bytes(int n, int H, int W, const int* depths) {
    if (!depths_ok(depths, "car_trunk_workspace_bytes") || !trunk_shape_ok(n, H, W, "car_trunk_workspace_bytes")) return 0;
    return trunk_work(n, H, W, depths).total;
}

extern "C" int car_trunk_forward(const float* x, int n, int H, int W, const float* packed, const int* depths, float* layer1, float* layer2, float* feat,
                                 void* work, size_t work_bytes, void* stream) {
    CAR_REQUIRE(x && packed && layer1 && layer2 && feat && work, "car_trunk_forward: null pointer");
    if (!depths_ok(depths, "car_trunk_forward") || !trunk_shape_ok(n, H, W, "car_trunk_forward")) return CAR_E_ARG;
    CAR_REQUIRE(aligned16(x) && aligned16(packed) && aligned16(layer1) && aligned16(layer2) && aligned16(feat) && aligned16(work),
                "car_trunk_forward: x, packed, layer1, layer2, feat and work must be 16-byte aligned");
    const TrunkWork k = trunk_work(n, H, W, depths, work);
    CAR_REQUIRE(work_bytes >= k.total, "car_trunk_forward: the workspace is too small (%zu bytes, car_trunk_workspace_bytes says %zu)", work_bytes, k.total);
    const TrunkPack t = trunk_pack_layout(depths);
    float* const stage_out[kStages] = {layer1, layer2, feat};
    auto gn = [&](float* X, int HW, int C, size_t g, size_t b, const float* add, int flags) {
        return car_groupnorm(X, n, HW, C, kGroups, packed + g, packed + b, kGnEps, add, flags, X, k.gn, k.gn_bytes, stream);
    };
    int h = same_out(H, 2), w = same_out(W, 2);
    CAR_TRY(car_stem7x7(x, n, H, W, packed + t.stem_w, k.u, stream));
    CAR_TRY(gn(k.u, h * w, 64, t.stem_g, t.stem_b, nullptr, CAR_GN_RELU));
    CAR_TRY(car_maxpool3x3s2_same(k.u, n, h, w, 64, k.v, stream));
    h = same_out(h, 2); w = same_out(w, 2);
    float* cur = k.v;
    int blk = 0;
    for (int s = 0; s < kStages; ++s)
        for (int i = 0; i < depths[s]; ++i, ++blk) {
            const BlockPack& b = t.blk[blk];
            const int ho = same_out(h, b.stride), wo = same_out(w, b.stride);
            const long rows_in = (long)n * h * w, rows_out = (long)n * ho * wo;
            const float* shortcut = cur;
            if (b.project) {
                const float* src = cur;
                if (b.stride == 2) { CAR_TRY(car_pixels_stride2(cur, n, h, w, b.cin, k.mb, stream)); src = k.mb; }
                CAR_TRY(car_linear_x3(src, b.cin, packed + b.down_w, nullptr, b.cin, b.cout, k.sc, b.cout, rows_out, 0, stream));
                CAR_TRY(gn(k.sc, ho * wo, b.cout, b.down_g, b.down_b, nullptr, 0));
                shortcut = k.sc;
            }
            CAR_TRY(car_linear_x3(cur, b.cin, packed + b.w1, nullptr, b.cin, b.mid, k.ma, b.mid, rows_in, 0, stream));
            CAR_TRY(gn(k.ma, h * w, b.mid, b.g1, b.b1, nullptr, CAR_GN_RELU));
            CAR_TRY(car_conv3x3_same(k.ma, n, h, w, b.mid, b.mid, b.stride, packed + b.w2, k.mb, stream));
            CAR_TRY(gn(k.mb, ho * wo, b.mid, b.g2, b.b2, nullptr, CAR_GN_RELU));
            float* out = i == depths[s] - 1 ? stage_out[s] : (cur == k.u ? k.v : k.u);
            CAR_TRY(car_linear_x3(k.mb, b.mid, packed + b.w3, nullptr, b.mid, b.cout, out, b.cout, rows_out, 0, stream));
            CAR_TRY(gn(out, ho * wo, b.cout, b.g3, b.b3, shortcut, CAR_GN_RELU));
            cur = out; h = ho; w = wo;
        }
    return CAR_OK;
}

extern "C" size_t car_vit_tokens_packed_floats(int gh, int gw) {
    return tok_shape_ok(gh, gw, "car_vit_tokens_packed_floats") ? tok_pack_layout(gh, gw).floats : 0;
}

extern "C" int car_vit_tokens_pack(const float* proj_w, const float* proj_b, const float* cls, const float* pos_embed, int grid, const float* pose_w,
                                   const float* pose_b, int gh, int gw, float* packed, void* stream) {
    CAR_REQUIRE(proj_w && proj_b && cls && pos_embed && pose_w && pose_b && packed, "car_vit_tokens_pack: null pointer");
    if (!tok_shape_ok(gh, gw, "car_vit_tokens_pack")) return CAR_E_ARG;
    CAR_REQUIRE(grid >= 1 && grid <= 1024, "car_vit_tokens_pack: the position embedding's grid (%d) is outside 1..1024", grid);
    CAR_REQUIRE(aligned16(proj_w) && aligned16(proj_b) && aligned16(cls) && aligned16(pos_embed) && aligned16(pose_w) && aligned16(pose_b) && aligned16(packed),
                "car_vit_tokens_pack: every array must be 16-byte aligned");
    const TokPack t = tok_pack_layout(gh, gw);
    hipStream_t st = (hipStream_t)stream;
    CAR_TRY(car_linear_x3_pack(proj_w, kTokIn, kTokIn, kTokDim, packed + t.proj, stream));
    CAR_CHECK_HIP(hipMemcpyAsync(packed + t.bias, proj_b, sizeof(float) * kTokDim, hipMemcpyDeviceToDevice, st), "car_vit_tokens_pack: copy failed");
    CAR_CHECK_HIP(hipMemcpyAsync(packed + t.cls, cls, sizeof(float) * kTokDim, hipMemcpyDeviceToDevice, st), "car_vit_tokens_pack: copy failed");
    CAR_CHECK_HIP(hipMemcpyAsync(packed + t.pose_w, pose_w, sizeof(float) * 16 * kTokDim, hipMemcpyDeviceToDevice, st), "car_vit_tokens_pack: copy failed");
    CAR_CHECK_HIP(hipMemcpyAsync(packed + t.pose_b, pose_b, sizeof(float) * kTokDim, hipMemcpyDeviceToDevice, st), "car_vit_tokens_pack: copy failed");
    (void)hipGetLastError();
    hipLaunchKernelGGL(pos_resize_kernel, dim3(car_div_up((long)(1 + gh * gw) * kTokDim, 256)), dim3(256), 0, st, pos_embed, grid, gh, gw, packed + t.pos);
    CAR_CHECK_LAUNCH("car_vit_tokens_pack");
    return CAR_OK;
}

extern "C" size_t car_vit_tokens_workspace_bytes(int BV, int gh, int gw) {
    if (!tok_shape_ok(gh, gw, "car_vit_tokens_workspace_bytes")) return 0;
    if (BV < 1 || BV > 4096) { car_set_error("car_vit_tokens_workspace_bytes: BV = %d is outside 1..4096", BV); return 0; }
    return tok_work(BV, gh, gw).total;
}

extern "C" int car_vit_tokens(const float* feat, int BV, int gh, int gw, const float* pose16, const float* packed, float* tok, void* work,
                              size_t work_bytes, void* stream) {
    CAR_REQUIRE(feat && pose16 && packed && tok && work, "car_vit_tokens: null pointer");
    if (!tok_shape_ok(gh, gw, "car_vit_tokens")) return CAR_E_ARG;
    CAR_REQUIRE(BV >= 1 && BV <= 4096, "car_vit_tokens: BV = %d is outside 1..4096", BV);
    CAR_REQUIRE(aligned16(feat) && aligned16(pose16) && aligned16(packed) && aligned16(tok) && aligned16(work),
                "car_vit_tokens: feat, pose16, packed, tok and work must be 16-byte aligned");
    const TokWork k = tok_work(BV, gh, gw, work);
    CAR_REQUIRE(work_bytes >= k.total, "car_vit_tokens: the workspace is too small (%zu bytes, car_vit_tokens_workspace_bytes says %zu)", work_bytes, k.total);
    const TokPack t = tok_pack_layout(gh, gw);
    hipStream_t st = (hipStream_t)stream;
    const int T = 1 + gh * gw;
    CAR_TRY(car_linear_x3(feat, kTokIn, packed + t.proj, packed + t.bias, kTokIn, kTokDim, k.proj, kTokDim, (long)BV * gh * gw, 0, stream));
    (void)hipGetLastError();
    hipLaunchKernelGGL(pose_embed_kernel, dim3(car_div_up((long)BV * kTokDim, 256)), dim3(256), 0, st, pose16, packed + t.pose_w, packed + t.pose_b, BV, k.pose);
    const long total4 = (long)BV * T * (kTokDim / 4);
    hipLaunchKernelGGL(tokens_kernel, dim3(car_div_up(total4, 256)), dim3(256), 0, st, k.proj, packed + t.cls, packed + t.pos, k.pose, T, total4, tok);
    CAR_CHECK_LAUNCH("car_vit_tokens");
    return CAR_OK;
}

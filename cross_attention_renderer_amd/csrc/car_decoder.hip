// car_decoder.hip — what stands behind the transformer blocks in get_z's image encoder, and get_z as one call (include/car_decoder.h; the
// last 45 lines of encoder.py MultiViewDPTEncoder.forward and the normalisation and conv_map lines of models.CrossAttentionRenderer.get_z;
// DESIGN.md §17): ProjectReadout in its split form, the 3x3 convolution with torch's symmetric padding of 1 and a bias / residual / ReLU
// epilogue, the bilinear 2x upsampling with align_corners = True, conv_map's 7x7 convolution, the image normalisation, the decoder as a
// sequence of these entries and car_linear_x3, and car_getz as the sequence normalise -> trunk -> tokens -> blocks -> decoder -> conv_map.
// Inference only.  Activations are channel-last fp32 rows [n][H W][C].
//
// The two dense convolutions are car_conv.hip's: the 3x3 one is conv3x3_kernel in its general form (car_conv3x3_general), the form the
// trunk runs, here with a padding of 1 in front — so the window's centre (stride oy, stride ox) is always inside the image — and the bias,
// residual, ReLU and accumulation of its epilogue; conv_map is conv7x7_kernel at stride 1 with a padding of 3 and a bias (car_conv7x7).
#include "car_common.h"
#include <math.h>
#include <stdint.h>

namespace {

constexpr long kMaxPixels = 1L << 27;              // n H W of the largest map of a call: keeps every row count, grid and per-image offset inside 32 bits
constexpr int kMaxImages = 4096, kMaxGrid = 64;
constexpr int kDim = 768, kFuse = 256;             // the token width and the fusion width of the product (car_decoder_* and car_getz)
constexpr int kDecoderParams = 50;

inline int pad1_out(int i, int s) { return (i - 1) / s + 1; }
unsigned grid_for(long total) { const long blocks = (total + 255) / 256; return (unsigned)(blocks < 65536 ? blocks : 65536); }
bool image_shape_ok(int n, int H, int W, const char* who) {
    if (n < 1 || n > kMaxImages || H < 1 || W < 1 || (double)n * H * W > (double)kMaxPixels) {
        car_set_error("%s: %d images of %d x %d, need 1..%d images of at least one pixel and at most 2^27 pixels in all", who, n, H, W, kMaxImages);
        return false;
    }
    return true;
}

// ---- the 3x3 convolution with zero padding 1 (car_conv.hip) ---------------------------------------------------------------------------------
bool pad1_widths_ok(int K, int N) { return (K == 256 || K == 512 || K == 768) && (N == 256 || N == 768); }
size_t pad1_floats(int K, int N) { return car_conv3x3_tile_floats(K, N) + 64; }

// ---- bilinear 2x upsampling, align_corners = True -------------------------------------------------------------------------------------------
// output o of an extent E reads source coordinate o (E - 1) / (2 E - 1), taken exactly: i0 = o (E - 1) div (2 E - 1), the fraction
// l = (o (E - 1) mod (2 E - 1)) / (2 E - 1) rounded once, i1 = min(i0 + 1, E - 1).  The corners have l = 0 and an extent of 1 has i0 = i1 = 0
// and l = 0: nothing outside the image is read.  top = fma(lx, v01 - v00, v00), bot = fma(lx, v11 - v10, v10), out = fma(ly, bot - top, top):
// a constant image comes back exactly, a pixel with l = 0 is its source's bits
__global__ void __launch_bounds__(256) upsample2x_kernel(const float* __restrict__ X, float* __restrict__ Y, int H, int W, int C4, long total, long in4) {
    const int Ho = 2 * H, Wo = 2 * W;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int c = (int)(idx % C4);
        long r = idx / C4;
        const int ox = (int)(r % Wo); r /= Wo;
        const int oy = (int)(r % Ho);
        const long img = r / Ho;
        const int ny = oy * (H - 1), dy = Ho - 1, nx = ox * (W - 1), dx = Wo - 1;
        const int y0 = ny / dy, x0 = nx / dx, y1 = min(y0 + 1, H - 1), x1 = min(x0 + 1, W - 1);
        const float ly = (float)(ny % dy) / (float)dy, lx = (float)(nx % dx) / (float)dx;
        const float4* src = reinterpret_cast<const float4*>(X) + img * H * W * C4 + c;
        const long i00 = ((long)y0 * W + x0) * C4, i01 = ((long)y0 * W + x1) * C4, i10 = ((long)y1 * W + x0) * C4, i11 = ((long)y1 * W + x1) * C4;
        CAR_BOUNDS_TRAP(img * H * W * C4 + c + i11 < in4 && i00 >= 0);
        const float4 v00 = src[i00], v01 = src[i01], v10 = src[i10], v11 = src[i11];
        auto mix = [&](float a, float b, float e, float f) {
            const float top = fmaf(lx, b - a, a), bot = fmaf(lx, f - e, e);
            return fmaf(ly, bot - top, top);
        };
        reinterpret_cast<float4*>(Y)[idx] = make_float4(mix(v00.x, v01.x, v10.x, v11.x), mix(v00.y, v01.y, v10.y, v11.y), mix(v00.z, v01.z, v10.z, v11.z),
                                                        mix(v00.w, v01.w, v10.w, v11.w));
    }
}

// ---- the read-out: Y[v][p] = gelu(prod[v][1 + p] + r[v]) ---------------------------------------------------------------------------------------
// prod [BV T][dim] = Wa t over ALL token rows (the class row's product is not used), r [BV][dim] = Wb t[v][0] + b; car_gelu's formula
__device__ __forceinline__ float gelu1(float x) { return 0.5f * x * erfcf(-0.70710678118654752440f * x); }
__global__ void __launch_bounds__(256) readout_kernel(const float* __restrict__ prod, const float* __restrict__ r, float* __restrict__ Y, int T, int D4,
                                                      long total4, long prod4, long r4) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total4) return;
    const int c = (int)(i % D4), p = (int)((i / D4) % (T - 1));
    const long v = i / ((long)D4 * (T - 1));
    CAR_BOUNDS_TRAP((v * T + 1 + p) * D4 + c < prod4 && v * D4 + c < r4);
    const float4 a = reinterpret_cast<const float4*>(prod)[(v * T + 1 + p) * D4 + c], e = reinterpret_cast<const float4*>(r)[v * D4 + c];
    reinterpret_cast<float4*>(Y)[i] = make_float4(gelu1(a.x + e.x), gelu1(a.y + e.y), gelu1(a.z + e.z), gelu1(a.w + e.w));
}
bool readout_dim_ok(int dim) { return dim >= 64 && dim <= 1024 && dim % 32 == 0; }
struct ReadoutPack { size_t wa, wb, bias, floats; };
ReadoutPack readout_pack_layout(int dim) {
    ReadoutPack t;
    Carver c(nullptr, 4);
    t.wa = c.at<float>(car_linear_x3_packed_floats(dim, dim)); t.wb = c.at<float>(car_linear_x3_packed_floats(dim, dim)); t.bias = c.at<float>(dim);
    t.floats = c.bytes() / sizeof(float);
    return t;
}
struct ReadoutWork { float *prod, *r; size_t total; };
ReadoutWork readout_work(int BV, int P, int dim, void* work = nullptr) {
    Carver c(work, 64);
    ReadoutWork t;
    t.prod = c.take<float>((size_t)BV * (1 + P) * dim); t.r = c.take<float>((size_t)BV * dim);
    t.total = c.bytes();
    return t;
}
bool readout_shape_ok(int BV, int P, int dim, const char* who) {
    if (BV < 1 || BV > kMaxImages || P < 1 || P > kMaxGrid * kMaxGrid) { car_set_error("%s: %d views of %d patches, need 1..%d views of 1..%d patches", who, BV, P, kMaxImages, kMaxGrid * kMaxGrid); return false; }
    if (!readout_dim_ok(dim)) { car_set_error("%s: dim = %d must be a multiple of 32 in 64..1024", who, dim); return false; }
    return true;
}

// ---- the image normalisation of get_z: ((v + 1) / 2 - mean_c) / std_c, its operations in its order, nothing contracted -------------------------
__global__ void __launch_bounds__(256) normalize_kernel(const float* __restrict__ rgb, float* __restrict__ x, long HW, long total) {
#pragma clang fp contract(off)
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const long pix = idx % HW, r = idx / HW;
        const int c = (int)(r % 3);
        const long img = r / 3;
        const float mean = c == 0 ? 0.485f : c == 1 ? 0.456f : 0.406f, sd = c == 0 ? 0.229f : c == 1 ? 0.224f : 0.225f;
        CAR_BOUNDS_TRAP((img * HW + pix) * 3 + c < total);
        const float v = rgb[(img * HW + pix) * 3 + c];
        const float half = (v + 1.0f) / 2.0f;
        const float centred = half - mean;
        x[idx] = centred / sd;
    }
}

// ---- the decoder's layouts ---------------------------------------------------------------------------------------------------------------------
// car_decoder_pack's array, in floats from its start.  A 3x3 layer is car_conv3x3_pad1_pack's array, a 1x1 layer car_linear_x3_pack's, a
// read-out car_readout_pack's; every bias is copied behind its layer
struct Lin { size_t w, b; };
struct RefinePack { Lin out, rcu1[2], rcu2[2]; };
struct DecoderPack { size_t ro3, ro4; Lin lin3, lin4, conv4; size_t rn[4]; RefinePack refine[4]; size_t floats; };
constexpr int kRnIn[4] = {256, 512, 768, 768};
DecoderPack decoder_pack_layout() {
    DecoderPack t{};
    Carver c(nullptr, 4);
    auto lin = [&](size_t wfloats, int N) { Lin l; l.w = c.at<float>(wfloats); l.b = c.at<float>(N); return l; };
    t.ro3 = c.at<float>(readout_pack_layout(kDim).floats);
    t.lin3 = lin(car_linear_x3_packed_floats(kDim, kDim), kDim);
    t.ro4 = c.at<float>(readout_pack_layout(kDim).floats);
    t.lin4 = lin(car_linear_x3_packed_floats(kDim, kDim), kDim);
    t.conv4 = lin(pad1_floats(kDim, kDim), kDim);
    for (int i = 0; i < 4; ++i) t.rn[i] = c.at<float>(pad1_floats(kRnIn[i], kFuse));
    for (int i = 0; i < 4; ++i) {
        RefinePack& r = t.refine[i];
        r.out = lin(car_linear_x3_packed_floats(kFuse, kFuse), kFuse);
        if (i < 3)                                                       // refinenet4 has no skip: its resConfUnit1 is never evaluated
            for (int j = 0; j < 2; ++j) r.rcu1[j] = lin(pad1_floats(kFuse, kFuse), kFuse);
        for (int j = 0; j < 2; ++j) r.rcu2[j] = lin(pad1_floats(kFuse, kFuse), kFuse);
    }
    t.floats = c.bytes() / sizeof(float);
    return t;
}
// car_decoder_forward's workspace: the read-out's result, layer_3, the 1x1 result of tap 4 and layer_4 (768 wide); the skip, the path and a
// residual unit's middle map (256 wide, at the finest level's pixels); the upsampled map; then car_readout's workspace as a nested range
struct DecoderWork { float *ro, *l3, *l4a, *l4, *skip, *path, *mid, *up; void* ro_work; size_t ro_bytes, total; };
DecoderWork decoder_work(int BV, int gh, int gw, void* work = nullptr) {
    const size_t P = (size_t)gh * gw, P4 = (size_t)(gh / 2) * (gw / 2), fine = (size_t)BV * 16 * P;
    Carver c(work, 64);
    DecoderWork t;
    t.ro = c.take<float>(BV * P * kDim); t.l3 = c.take<float>(BV * P * kDim); t.l4a = c.take<float>(BV * P * kDim); t.l4 = c.take<float>(BV * P4 * kDim);
    t.skip = c.take<float>(fine * kFuse); t.path = c.take<float>(fine * kFuse); t.mid = c.take<float>(fine * kFuse); t.up = c.take<float>(4 * fine * kFuse);
    t.ro_bytes = readout_work(BV, (int)P, kDim).total;
    t.ro_work = c.sub(t.ro_bytes).take<float>(t.ro_bytes / sizeof(float));
    t.total = c.bytes();
    return t;
}
bool decoder_shape_ok(int BV, int gh, int gw, const char* who) {
    if (BV < 1 || BV > kMaxImages) { car_set_error("%s: BV = %d is outside 1..%d", who, BV, kMaxImages); return false; }
    if (gh < 2 || gh > kMaxGrid || gw < 2 || gw > kMaxGrid || (gh & 1) || (gw & 1)) {
        car_set_error("%s: a grid of %d x %d patches, need even extents in 2..%d (the halved map is doubled back onto the grid)", who, gh, gw, kMaxGrid);
        return false;
    }
    if ((double)BV * 64 * gh * gw > (double)kMaxPixels) { car_set_error("%s: %d views of %d x %d patches pass 2^27 pixels at the finest level", who, BV, gh, gw); return false; }
    return true;
}

// ---- car_getz's layout ---------------------------------------------------------------------------------------------------------------------------
// the normalised images, the trunk's three stage ends, the token rows, the two tapped states, then ONE range that the five stages' own
// workspaces share (each is done with it when the next begins)
struct GetzWork { float *x, *layer1, *layer2, *feat, *tok, *tap[2]; void* stage; size_t stage_bytes, total; };
GetzWork getz_work(int BV, int H, int W, int gh, int gw, int nviews, const int* depths, void* work = nullptr) {
    const size_t P = (size_t)gh * gw, T = 1 + P;
    size_t stage = car_trunk_workspace_bytes(BV, H, W, depths);
    auto need = [&](size_t v) { if (stage < v) stage = v; };
    need(car_vit_tokens_workspace_bytes(BV, gh, gw));
    need(car_vit_workspace_bytes(BV / nviews, nviews * (int)T, kDim));
    need(decoder_work(BV, gh, gw).total);
    Carver c(work, 64);
    GetzWork t;
    t.x = c.take<float>((size_t)BV * 3 * H * W);
    t.layer1 = c.take<float>((size_t)BV * 16 * P * 256); t.layer2 = c.take<float>((size_t)BV * 4 * P * 512); t.feat = c.take<float>((size_t)BV * P * 1024);
    t.tok = c.take<float>((size_t)BV * T * kDim); t.tap[0] = c.take<float>((size_t)BV * T * kDim); t.tap[1] = c.take<float>((size_t)BV * T * kDim);
    t.stage_bytes = stage;
    t.stage = c.sub(stage).take<float>(stage / sizeof(float));
    t.total = c.bytes();
    return t;
}
bool getz_shape_ok(int BV, int H, int W, int gh, int gw, int nviews, const int* depths, int vit_depth, const char* who) {
    if (!depths) { car_set_error("%s: null pointer", who); return false; }
    if (!decoder_shape_ok(BV, gh, gw, who) || !image_shape_ok(BV, H, W, who)) return false;
    if (nviews < 1 || BV % nviews) { car_set_error("%s: BV = %d is not a multiple of nviews = %d", who, BV, nviews); return false; }
    auto up = [](int v, int k) { return (v + k - 1) / k; };
    if (up(H, 16) != gh || up(W, 16) != gw || up(H, 8) != 2 * gh || up(W, 8) != 2 * gw || up(H, 4) != 4 * gh || up(W, 4) != 4 * gw) {
        car_set_error("%s: a %d x %d image gives %d x %d trunk features (and %d x %d, %d x %d before them), not the %d x %d token grid and its doubles", who,
                      H, W, up(H, 16), up(W, 16), up(H, 8), up(W, 8), up(H, 4), up(W, 4), gh, gw);
        return false;
    }
    if ((long)nviews * (1 + gh * gw) > 1024) { car_set_error("%s: %d views of %d tokens pass car_mha's 1024 rows per scene", who, nviews, 1 + gh * gw); return false; }
    if (vit_depth < 1 || vit_depth > 32) { car_set_error("%s: %d transformer blocks, need 1..32", who, vit_depth); return false; }
    if (car_trunk_workspace_bytes(BV, H, W, depths) == 0) return false;          // the trunk's own message (a depth outside 1..16)
    return true;
}

}  // namespace

// the packed 3x3 layer: car_conv3x3_same_pack's tile layout — 9 K / 32 x N / 16 tiles of 512 floats, [K step][tile][hi | lo][lane][8 halves]
// with k = tap * K + channel — then 64 floats of scale (2^shift, 2^-shift, the largest magnitude, zeros).  The bias is the call's.
extern "C" size_t car_conv3x3_pad1_packed_floats(int K, int N) {
    if (!pad1_widths_ok(K, N)) { car_set_error("car_conv3x3_pad1_packed_floats: %d -> %d channels, need K among 256, 512, 768 and N among 256, 768", K, N); return 0; }
    return pad1_floats(K, N);
}

extern "C" int car_conv3x3_pad1_pack(const float* w, int K, int N, float* packed, void* stream) {
    CAR_REQUIRE(w && packed, "car_conv3x3_pad1_pack: null pointer");
    CAR_REQUIRE(pad1_widths_ok(K, N), "car_conv3x3_pad1_pack: %d -> %d channels, need K among 256, 512, 768 and N among 256, 768", K, N);
    CAR_REQUIRE(aligned16(w) && aligned16(packed), "car_conv3x3_pad1_pack: w and packed must be 16-byte aligned");
    return car_conv3x3_pack_tiles("car_conv3x3_pad1_pack", w, nullptr, K, N, false, packed, (hipStream_t)stream);
}

extern "C" int car_conv3x3_pad1(const float* X, int n, int H, int W, int K, int N, int stride, const float* packed, const float* bias, const float* add,
                                int flags, float* Y, void* stream) {
    CAR_REQUIRE(X && packed && Y, "car_conv3x3_pad1: null pointer");
    CAR_REQUIRE(pad1_widths_ok(K, N), "car_conv3x3_pad1: %d -> %d channels, need K among 256, 512, 768 and N among 256, 768", K, N);
    CAR_REQUIRE(stride == 1 || stride == 2, "car_conv3x3_pad1: stride = %d, need 1 or 2", stride);
    CAR_REQUIRE((flags & ~(CAR_LIN_RELU_IN | CAR_LIN_RELU_OUT | CAR_LIN_ACCUM)) == 0, "car_conv3x3_pad1: flags = %d, need CAR_LIN_RELU_IN, CAR_LIN_RELU_OUT, CAR_LIN_ACCUM or 0", flags);
    if (!image_shape_ok(n, H, W, "car_conv3x3_pad1")) return CAR_E_ARG;
    CAR_REQUIRE(aligned16(X) && aligned16(packed) && aligned16(bias) && aligned16(add) && aligned16(Y),
                "car_conv3x3_pad1: X, packed, bias, add and Y must be 16-byte aligned");
    return car_conv3x3_general("car_conv3x3_pad1", true, X, n, H, W, K, N, stride, 1, 1, pad1_out(H, stride), pad1_out(W, stride), packed, bias, add, flags, Y,
                               (hipStream_t)stream);
}

extern "C" int car_upsample2x_bilinear(const float* X, int n, int H, int W, int C, float* Y, void* stream) {
    CAR_REQUIRE(X && Y, "car_upsample2x_bilinear: null pointer");
    if (!image_shape_ok(n, H, W, "car_upsample2x_bilinear")) return CAR_E_ARG;
    CAR_REQUIRE(H <= 16384 && W <= 16384 && (double)n * 4 * H * W <= (double)kMaxPixels,
                "car_upsample2x_bilinear: %d images of %d x %d pass 16384 a side or 2^27 output pixels in all", n, H, W);
    CAR_REQUIRE(C >= 4 && C <= 4096 && C % 4 == 0, "car_upsample2x_bilinear: C = %d must be a multiple of 4 in 4..4096", C);
    CAR_REQUIRE(aligned16(X) && aligned16(Y), "car_upsample2x_bilinear: X and Y must be 16-byte aligned");
    const long total = (long)n * 4 * H * W * (C / 4);
    (void)hipGetLastError();
    hipLaunchKernelGGL(upsample2x_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, X, Y, H, W, C / 4, total, (long)n * H * W * (C / 4));
    CAR_CHECK_LAUNCH("car_upsample2x_bilinear");
    return CAR_OK;
}

extern "C" size_t car_readout_packed_floats(int dim) {
    if (!readout_dim_ok(dim)) { car_set_error("car_readout_packed_floats: dim = %d must be a multiple of 32 in 64..1024", dim); return 0; }
    return readout_pack_layout(dim).floats;
}

extern "C" int car_readout_pack(const float* w, const float* bias, int dim, float* packed, void* stream) {
    CAR_REQUIRE(w && bias && packed, "car_readout_pack: null pointer");
    CAR_REQUIRE(readout_dim_ok(dim), "car_readout_pack: dim = %d must be a multiple of 32 in 64..1024", dim);
    CAR_REQUIRE(aligned16(w) && aligned16(bias) && aligned16(packed), "car_readout_pack: w, bias and packed must be 16-byte aligned");
    const ReadoutPack t = readout_pack_layout(dim);
    CAR_TRY(car_linear_x3_pack(w, 2 * dim, dim, dim, packed + t.wa, stream));              // Wa: the columns of the patch token
    CAR_TRY(car_linear_x3_pack(w + dim, 2 * dim, dim, dim, packed + t.wb, stream));        // Wb: the columns of the class token
    CAR_CHECK_HIP(hipMemcpyAsync(packed + t.bias, bias, sizeof(float) * dim, hipMemcpyDeviceToDevice, (hipStream_t)stream), "car_readout_pack: copy failed");
    return CAR_OK;
}

extern "C" size_t car_readout_workspace_bytes(int BV, int P, int dim) {
    return readout_shape_ok(BV, P, dim, "car_readout_workspace_bytes") ? readout_work(BV, P, dim).total : 0;
}

extern "C" int car_readout(const float* tok, int BV, int P, int dim, const float* packed, float* Y, void* work, size_t work_bytes, void* stream) {
    CAR_REQUIRE(tok && packed && Y && work, "car_readout: null pointer");
    if (!readout_shape_ok(BV, P, dim, "car_readout")) return CAR_E_ARG;
    CAR_REQUIRE(aligned16(tok) && aligned16(packed) && aligned16(Y) && aligned16(work), "car_readout: tok, packed, Y and work must be 16-byte aligned");
    const ReadoutWork k = readout_work(BV, P, dim, work);
    CAR_REQUIRE(work_bytes >= k.total, "car_readout: the workspace is too small (%zu bytes, car_readout_workspace_bytes says %zu)", work_bytes, k.total);
    const ReadoutPack t = readout_pack_layout(dim);
    const int T = 1 + P;
    CAR_TRY(car_linear_x3(tok, T * dim, packed + t.wb, packed + t.bias, dim, dim, k.r, dim, BV, 0, stream));          // r[v] = Wb t[v][0] + b
    CAR_TRY(car_linear_x3(tok, dim, packed + t.wa, nullptr, dim, dim, k.prod, dim, (long)BV * T, 0, stream));           // Wa t, every row
    const long total4 = (long)BV * P * (dim / 4);
    (void)hipGetLastError();
    hipLaunchKernelGGL(readout_kernel, dim3(car_div_up(total4, 256)), dim3(256), 0, (hipStream_t)stream, k.prod, k.r, Y, T, dim / 4, total4,
                       (long)BV * T * (dim / 4), (long)BV * (dim / 4));
    CAR_CHECK_LAUNCH("car_readout");
    return CAR_OK;
}

extern "C" int car_conv7x7_pad3(const float* x, int n, int H, int W, const float* w, const float* bias, float* Y, void* stream) {
    CAR_REQUIRE(x && w && bias && Y, "car_conv7x7_pad3: null pointer");
    if (!image_shape_ok(n, H, W, "car_conv7x7_pad3")) return CAR_E_ARG;
    CAR_REQUIRE(aligned16(x) && aligned16(w) && aligned16(bias) && aligned16(Y), "car_conv7x7_pad3: x, w, bias and Y must be 16-byte aligned");
    return car_conv7x7("car_conv7x7_pad3", x, n, H, W, 1, 3, 3, H, W, w, bias, Y, (hipStream_t)stream);
}

extern "C" int car_normalize_rgb(const float* rgb, int n, int H, int W, float* x, void* stream) {
    CAR_REQUIRE(rgb && x, "car_normalize_rgb: null pointer");
    if (!image_shape_ok(n, H, W, "car_normalize_rgb")) return CAR_E_ARG;
    CAR_REQUIRE(aligned16(rgb) && aligned16(x), "car_normalize_rgb: rgb and x must be 16-byte aligned");
    const long total = (long)n * H * W * 3;
    (void)hipGetLastError();
    hipLaunchKernelGGL(normalize_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, rgb, x, (long)H * W, total);
    CAR_CHECK_LAUNCH("car_normalize_rgb");
    return CAR_OK;
}

extern "C" size_t car_decoder_packed_floats(void) { return decoder_pack_layout().floats; }

extern "C" int car_decoder_pack(const float* const* params, int n_params, float* packed, void* stream) {
    CAR_REQUIRE(params && packed, "car_decoder_pack: null pointer");
    CAR_REQUIRE(n_params == kDecoderParams, "car_decoder_pack: %d parameter arrays, the decoder evaluates %d", n_params, kDecoderParams);
    for (int i = 0; i < n_params; ++i) {
        CAR_REQUIRE(params[i], "car_decoder_pack: null pointer (parameter %d)", i);
        CAR_REQUIRE(aligned16(params[i]), "car_decoder_pack: parameter %d must be 16-byte aligned", i);
    }
    CAR_REQUIRE(aligned16(packed), "car_decoder_pack: packed must be 16-byte aligned");
    const DecoderPack t = decoder_pack_layout();
    hipStream_t st = (hipStream_t)stream;
    int at = 0;
    auto vec = [&](size_t off, int count) -> int {
        CAR_CHECK_HIP(hipMemcpyAsync(packed + off, params[at++], sizeof(float) * count, hipMemcpyDeviceToDevice, st), "car_decoder_pack: copy failed");
        return CAR_OK;
    };
    auto readout = [&](size_t off) -> int { at += 2; return car_readout_pack(params[at - 2], params[at - 1], kDim, packed + off, stream); };
    auto lin = [&](const Lin& l, int K, int N) -> int { CAR_TRY(car_linear_x3_pack(params[at++], K, K, N, packed + l.w, stream)); return vec(l.b, N); };
    auto conv = [&](const Lin& l, int K, int N) -> int { CAR_TRY(car_conv3x3_pad1_pack(params[at++], K, N, packed + l.w, stream)); return vec(l.b, N); };
    CAR_TRY(readout(t.ro3)); CAR_TRY(lin(t.lin3, kDim, kDim));
    CAR_TRY(readout(t.ro4)); CAR_TRY(lin(t.lin4, kDim, kDim)); CAR_TRY(conv(t.conv4, kDim, kDim));
    for (int i = 0; i < 4; ++i) CAR_TRY(car_conv3x3_pad1_pack(params[at++], kRnIn[i], kFuse, packed + t.rn[i], stream));
    for (int i = 0; i < 4; ++i) {
        const RefinePack& r = t.refine[i];
        CAR_TRY(lin(r.out, kFuse, kFuse));
        if (i < 3)
            for (int j = 0; j < 2; ++j) CAR_TRY(conv(r.rcu1[j], kFuse, kFuse));
        for (int j = 0; j < 2; ++j) CAR_TRY(conv(r.rcu2[j], kFuse, kFuse));
    }
    return CAR_OK;
}

extern "C" size_t car_decoder_workspace_bytes(int BV, int gh, int gw) {
    return decoder_shape_ok(BV, gh, gw, "car_decoder_workspace_bytes") ? decoder_work(BV, gh, gw).total : 0;
}

extern "C" int car_decoder_forward(const float* tap3, const float* tap4, const float* layer1, const float* layer2, int BV, int gh, int gw,
                                   const float* packed, float* path_2, float* path_1, void* work, size_t work_bytes, void* stream) {
    CAR_REQUIRE(tap3 && tap4 && layer1 && layer2 && packed && path_2 && path_1 && work, "car_decoder_forward: null pointer");
    if (!decoder_shape_ok(BV, gh, gw, "car_decoder_forward")) return CAR_E_ARG;
    CAR_REQUIRE(aligned16(tap3) && aligned16(tap4) && aligned16(layer1) && aligned16(layer2) && aligned16(packed) && aligned16(path_2) && aligned16(path_1) &&
                aligned16(work), "car_decoder_forward: every array must be 16-byte aligned");
    const DecoderWork k = decoder_work(BV, gh, gw, work);
    CAR_REQUIRE(work_bytes >= k.total, "car_decoder_forward: the workspace is too small (%zu bytes, car_decoder_workspace_bytes says %zu)", work_bytes, k.total);
    const DecoderPack t = decoder_pack_layout();
    hipStream_t st = (hipStream_t)stream;
    const int P = gh * gw;
    const long rows = (long)BV * P;
    const int RELU_IN = CAR_LIN_RELU_IN;
    auto conv = [&](const float* X, int h, int w, int K, int N, int stride, size_t wt, const float* bias, const float* add, int flags, float* Y) {
        return car_conv3x3_pad1(X, BV, h, w, K, N, stride, packed + wt, bias, add, flags, Y, stream);
    };
    // the two re-assembled maps: layer_3 [BV][gh gw][768], layer_4 [BV][gh / 2 gw / 2][768]
    CAR_TRY(car_readout(tap3, BV, P, kDim, packed + t.ro3, k.ro, k.ro_work, k.ro_bytes, stream));
    CAR_TRY(car_linear_x3(k.ro, kDim, packed + t.lin3.w, packed + t.lin3.b, kDim, kDim, k.l3, kDim, rows, 0, stream));
    CAR_TRY(car_readout(tap4, BV, P, kDim, packed + t.ro4, k.ro, k.ro_work, k.ro_bytes, stream));
    CAR_TRY(car_linear_x3(k.ro, kDim, packed + t.lin4.w, packed + t.lin4.b, kDim, kDim, k.l4a, kDim, rows, 0, stream));
    CAR_TRY(conv(k.l4a, gh, gw, kDim, kDim, 2, t.conv4.w, packed + t.conv4.b, nullptr, 0, k.l4));
    // refinenet4 .. refinenet1.  Level i works at h x w pixels; its layerN_rn goes into the path (level 4, which has no skip) or the skip
    const float* level_in[4] = {layer1, layer2, k.l3, k.l4};
    float* const level_out[4] = {path_1, path_2, k.path, k.path};
    int h = gh / 2, w = gw / 2;
    for (int i = 3; i >= 0; --i) {
        const RefinePack& r = t.refine[i];
        CAR_TRY(conv(level_in[i], h, w, kRnIn[i], kFuse, 1, t.rn[i], nullptr, nullptr, 0, i == 3 ? k.path : k.skip));
        if (i < 3) {                                                     // path = path + resConfUnit1(skip)
            CAR_TRY(conv(k.skip, h, w, kFuse, kFuse, 1, r.rcu1[0].w, packed + r.rcu1[0].b, nullptr, RELU_IN, k.mid));
            CAR_TRY(conv(k.mid, h, w, kFuse, kFuse, 1, r.rcu1[1].w, packed + r.rcu1[1].b, k.skip, RELU_IN | CAR_LIN_ACCUM, k.path));
        }
        CAR_TRY(conv(k.path, h, w, kFuse, kFuse, 1, r.rcu2[0].w, packed + r.rcu2[0].b, nullptr, RELU_IN, k.mid));
        CAR_TRY(conv(k.mid, h, w, kFuse, kFuse, 1, r.rcu2[1].w, packed + r.rcu2[1].b, k.path, RELU_IN, k.skip));
        CAR_TRY(car_upsample2x_bilinear(k.skip, BV, h, w, kFuse, k.up, stream));
        h *= 2; w *= 2;
        const long up_rows = (long)BV * h * w;
        CAR_TRY(car_linear_x3(k.up, kFuse, packed + r.out.w, packed + r.out.b, kFuse, kFuse, level_out[i], kFuse, up_rows, 0, stream));
        if (i == 1)                                                      // path_2 is an output AND the next level's path
            CAR_CHECK_HIP(hipMemcpyAsync(k.path, path_2, sizeof(float) * up_rows * kFuse, hipMemcpyDeviceToDevice, st), "car_decoder_forward: copy failed");
    }
    return CAR_OK;
}

extern "C" size_t car_getz_workspace_bytes(int BV, int H, int W, int gh, int gw, int nviews, const int* depths, int vit_depth) {
    return getz_shape_ok(BV, H, W, gh, gw, nviews, depths, vit_depth, "car_getz_workspace_bytes") ? getz_work(BV, H, W, gh, gw, nviews, depths).total : 0;
}

extern "C" int car_getz(const float* rgb, const float* pose16, int BV, int H, int W, int gh, int gw, int nviews, const int* depths, const float* trunk_packed,
                        const float* tokens_packed, const float* vit_packed, int vit_depth, const int* taps, const float* decoder_packed,
                        const float* map_w, const float* map_b, int no_high_freq, float* z0, float* z1, float* z2, void* work, size_t work_bytes,
                        void* stream) {
    CAR_REQUIRE(rgb && pose16 && trunk_packed && tokens_packed && vit_packed && taps && decoder_packed && map_w && map_b && z0 && z1 && z2 && work,
                "car_getz: null pointer");
    if (!getz_shape_ok(BV, H, W, gh, gw, nviews, depths, vit_depth, "car_getz")) return CAR_E_ARG;
    CAR_REQUIRE(taps[0] >= 0 && taps[0] < taps[1] && taps[1] < vit_depth, "car_getz: taps (%d, %d) must increase inside the %d blocks", taps[0], taps[1], vit_depth);
    CAR_REQUIRE(aligned16(rgb) && aligned16(pose16) && aligned16(trunk_packed) && aligned16(tokens_packed) && aligned16(vit_packed) && aligned16(decoder_packed) &&
                aligned16(map_w) && aligned16(map_b) && aligned16(z0) && aligned16(z1) && aligned16(z2) && aligned16(work),
                "car_getz: every array must be 16-byte aligned");
    const GetzWork k = getz_work(BV, H, W, gh, gw, nviews, depths, work);
    CAR_REQUIRE(work_bytes >= k.total, "car_getz: the workspace is too small (%zu bytes, car_getz_workspace_bytes says %zu)", work_bytes, k.total);
    const int T = 1 + gh * gw;
    float* const tap_out[2] = {k.tap[0], k.tap[1]};
    CAR_TRY(car_normalize_rgb(rgb, BV, H, W, k.x, stream));
    CAR_TRY(car_trunk_forward(k.x, BV, H, W, trunk_packed, depths, k.layer1, k.layer2, k.feat, k.stage, k.stage_bytes, stream));
    CAR_TRY(car_vit_tokens(k.feat, BV, gh, gw, pose16, tokens_packed, k.tok, k.stage, k.stage_bytes, stream));
    CAR_TRY(car_vit_blocks(k.tok, BV / nviews, nviews * T, kDim, vit_packed, vit_depth, taps, 2, tap_out, k.stage, k.stage_bytes, stream));
    CAR_TRY(car_decoder_forward(k.tap[0], k.tap[1], k.layer1, k.layer2, BV, gh, gw, decoder_packed, z0, z1, k.stage, k.stage_bytes, stream));
    if (no_high_freq) {
        CAR_CHECK_HIP(hipMemsetAsync(z2, 0, sizeof(float) * (size_t)BV * H * W * 64, (hipStream_t)stream), "car_getz: memset failed");
        return CAR_OK;
    }
    return car_conv7x7_pad3(k.x, BV, H, W, map_w, map_b, z2, stream);
}

// car_frames.hip — the pixel chain of the RealEstate10K training reader on the device (include/car_hip.h: car_frames_table_ints,
// car_frames_table_slot, car_frames_resize_u8, car_frames_resize_f32).
//
// One kernel, two instances.  An image's record names a rectangle of a stored uint8 frame, the size it is resized to and the columns of
// the result that are kept; the arithmetic is dataio.resize_linear_u8's (OpenCV's 8-bit INTER_LINEAR: 11-bit coefficients, an int32
// horizontal pass, the vertical pass ((b0 (S0 >> 4)) >> 16) + ((b1 (S1 >> 4)) >> 16) + 2) >> 2, clip) on coefficient tables the host
// made, so the kernel holds integer arithmetic only and equals the host bit for bit.  The uint8 instance is the reader's first resize
// (360 x 640 -> the 256 x 256 window of 256 x 455), the float32 instance its second (flip, crop, 256 x 256) followed by the host's
// uint8 -> float32 / 127.5 - 1 as a 256-entry table.
//
// Work: a thread owns four consecutive output pixels (dense: of one row; sparse: of the index list), i.e. twelve values — three 16-byte
// stores as float32, three 4-byte stores as uint8.  Its sources are at most 2 x 2 taps per pixel, read as bytes: neighbouring threads
// read neighbouring bytes of the same two rows.  A workgroup of 256 threads owns 1024 pixels; the grid strides over (image, group).
// The launchers validate every record on the host before anything is launched; the kernel clamps table indices to the rectangle, so a
// wrong table gives wrong pixels, never a read outside the frame the record was validated for.
#include "car_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kQuad = 4;                                   // output pixels per thread
constexpr int kSlotInts = CAR_FRAMES_SLOT_ENTRIES * 4;
constexpr int kLutAt = CAR_FRAMES_SLOTS * kSlotInts;       // the grey-level table follows the slots
constexpr int kMaxIndex = 65536;

__host__ __device__ inline int table_slot(int n_src, int n_dst) {
    if (n_dst == 256 && n_src <= 256 && n_src >= 256 - 2 * 31 && (n_src & 1) == 0) return (256 - n_src) / 2;
    if (n_dst == 256 && n_src == 360) return 32;
    if (n_dst == 455 && n_src == 640) return 33;
    return -1;
}

struct FrameArgs {
    const unsigned char* src;
    const car_frame_rec* recs;
    const int* idx;
    const int4* tables;
    void* dst;
    int n_images, groups_per_image;
};

// a whole quad: `at` is a multiple of 4 elements (dst_off, win_w and the quad's first pixel are)
__device__ __forceinline__ void store12(float* dst, long long at, const int* v, const float* lut) {
    float4* p = reinterpret_cast<float4*>(dst + at);
    p[0] = make_float4(lut[v[0]], lut[v[1]], lut[v[2]], lut[v[3]]);
    p[1] = make_float4(lut[v[4]], lut[v[5]], lut[v[6]], lut[v[7]]);
    p[2] = make_float4(lut[v[8]], lut[v[9]], lut[v[10]], lut[v[11]]);
}

__device__ __forceinline__ void store12(unsigned char* dst, long long at, const int* v, const float*) {
    unsigned* p = reinterpret_cast<unsigned*>(dst + at);
#pragma unroll
    for (int k = 0; k < 3; ++k)
        p[k] = (unsigned)v[4 * k] | ((unsigned)v[4 * k + 1] << 8) | ((unsigned)v[4 * k + 2] << 16) | ((unsigned)v[4 * k + 3] << 24);
}

__device__ __forceinline__ void store1(float* dst, long long at, int v, const float* lut) { dst[at] = lut[v]; }
__device__ __forceinline__ void store1(unsigned char* dst, long long at, int v, const float*) { dst[at] = (unsigned char)v; }

template <typename OutT>
__global__ __launch_bounds__(kThreads) void frames_resize_kernel(FrameArgs a) {
    __shared__ float lut[256];
    if (sizeof(OutT) == 4) {
        lut[threadIdx.x] = reinterpret_cast<const float*>(a.tables)[kLutAt + threadIdx.x];   // kThreads == 256
        __syncthreads();
    }
    OutT* const dst = static_cast<OutT*>(a.dst);
    const int items = a.n_images * a.groups_per_image;
    for (int item = blockIdx.x; item < items; item += gridDim.x) {
        const car_frame_rec r = a.recs[item / a.groups_per_image];
        const int group = item % a.groups_per_image;
        const int n_pix = r.n_idx ? r.n_idx : r.dst_h * r.win_w;
        const int first = (group * kThreads + threadIdx.x) * kQuad;
        if (first >= n_pix) continue;
        const int count = min(kQuad, n_pix - first);
        const bool identity = r.rw == r.dst_w && r.rh == r.dst_h;
        const int4* xtab = a.tables + table_slot(r.rw, r.dst_w) * CAR_FRAMES_SLOT_ENTRIES;
        const int4* ytab = a.tables + table_slot(r.rh, r.dst_h) * CAR_FRAMES_SLOT_ENTRIES;
        const unsigned char* img = a.src + r.src_off;
        int v[3 * kQuad];
#pragma unroll
        for (int j = 0; j < kQuad; ++j) {
            if (j >= count) {
                v[3 * j] = v[3 * j + 1] = v[3 * j + 2] = 0;
                continue;
            }
            int p = first + j;
            if (r.n_idx) p = min(a.idx[r.idx_off + p], r.dst_h * r.win_w - 1);          // validated on the host; clamped all the same
            const int oy = p / r.win_w, ox = r.win_x0 + p % r.win_w;
            if (identity) {
                const int sx = r.x0 + (r.flip ? r.rw - 1 - ox : ox);
                const unsigned char* s = img + (long long)(r.y0 + oy) * r.src_pitch + 3 * sx;
                v[3 * j] = s[0], v[3 * j + 1] = s[1], v[3 * j + 2] = s[2];
                continue;
            }
            const int4 cx = xtab[ox], cy = ytab[oy];                                    // {i0, i1, w0, w1}
            int x0 = min(max(cx.x, 0), r.rw - 1), x1 = min(max(cx.y, 0), r.rw - 1);
            if (r.flip) x0 = r.rw - 1 - x0, x1 = r.rw - 1 - x1;
            const int y0 = min(max(cy.x, 0), r.rh - 1), y1 = min(max(cy.y, 0), r.rh - 1);
            const unsigned char* row0 = img + (long long)(r.y0 + y0) * r.src_pitch + 3 * r.x0;
            const unsigned char* row1 = img + (long long)(r.y0 + y1) * r.src_pitch + 3 * r.x0;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int s0 = (int)row0[3 * x0 + c] * cx.z + (int)row0[3 * x1 + c] * cx.w;      // horizontal pass: values x 2048
                const int s1 = (int)row1[3 * x0 + c] * cx.z + (int)row1[3 * x1 + c] * cx.w;
                const int o = (((cy.z * (s0 >> 4)) >> 16) + ((cy.w * (s1 >> 4)) >> 16) + 2) >> 2;
                v[3 * j + c] = min(max(o, 0), 255);
            }
        }
        const long long at = r.dst_off + 3LL * first;
        if (count == kQuad) {
            store12(dst, at, v, lut);
        } else {
            for (int k = 0; k < 3 * count; ++k) store1(dst, at + k, v[k], lut);
        }
    }
}

// Every field of every record against the extents the caller states; nothing is launched unless all of them pass.
int validate(const char* who, const unsigned char* src, size_t src_bytes, const car_frame_rec* recs_host, const car_frame_rec* recs_dev,
             int n_images, const int* idx_host, const int* idx_dev, size_t n_idx_total, const int* tables, const void* dst, size_t dst_elems,
             size_t elem_bytes, int* groups_per_image) {
    CAR_REQUIRE(src && recs_host && recs_dev && tables && dst, "%s: null pointer", who);
    CAR_REQUIRE(n_images >= 1 && n_images <= 65536, "%s: n_images = %d is outside 1 .. 65536", who, n_images);
    CAR_REQUIRE(((uintptr_t)dst & 15) == 0 && ((uintptr_t)tables & 15) == 0 && ((uintptr_t)recs_dev & 7) == 0,
                "%s: dst and tables must be 16-byte aligned, the records 8-byte", who);
    // blocks read src while others write dst: the two ranges may share an allocation, never a byte
    const uintptr_t s0 = (uintptr_t)src, d0 = (uintptr_t)dst;
    CAR_REQUIRE(d0 + dst_elems * elem_bytes <= s0 || s0 + src_bytes <= d0, "%s: dst (%zu elements) overlaps src (%zu bytes)", who, dst_elems, src_bytes);
    int max_pix = 0;
    for (int i = 0; i < n_images; ++i) {
        const car_frame_rec& r = recs_host[i];
        CAR_REQUIRE(r.src_h >= 1 && r.src_w >= 1 && r.src_w <= 65536 && r.src_h <= 65536 && r.src_pitch >= 3 * r.src_w && r.src_off >= 0,
                    "%s: image %d: bad stored size %d x %d, pitch %d, offset %lld", who, i, r.src_h, r.src_w, r.src_pitch, r.src_off);
        CAR_REQUIRE((size_t)r.src_off + (size_t)(r.src_h - 1) * r.src_pitch + 3 * (size_t)r.src_w <= src_bytes,
                    "%s: image %d: the stored image ends outside src (%zu bytes)", who, i, src_bytes);
        CAR_REQUIRE(r.x0 >= 0 && r.y0 >= 0 && r.rw >= 1 && r.rh >= 1 && (long long)r.x0 + r.rw <= r.src_w && (long long)r.y0 + r.rh <= r.src_h,
                    "%s: image %d: the rectangle (%d, %d) + %d x %d lies outside its %d x %d source", who, i, r.x0, r.y0, r.rw, r.rh, r.src_w,
                    r.src_h);
        CAR_REQUIRE(r.flip == 0 || r.flip == 1, "%s: image %d: flip must be 0 or 1", who, i);
        CAR_REQUIRE(r.reserved == 0, "%s: image %d: reserved must be 0", who, i);
        CAR_REQUIRE(table_slot(r.rw, r.dst_w) >= 0 && table_slot(r.rh, r.dst_h) >= 0,
                    "%s: image %d: no table for %d x %d -> %d x %d (destination size)", who, i, r.rw, r.rh, r.dst_w, r.dst_h);
        CAR_REQUIRE(r.win_x0 >= 0 && r.win_w >= 4 && r.win_w % 4 == 0 && r.win_x0 + r.win_w <= r.dst_w,
                    "%s: image %d: the written columns %d + %d must lie in the result's %d and be a multiple of 4", who, i, r.win_x0, r.win_w, r.dst_w);
        CAR_REQUIRE(r.dst_off >= 0 && r.dst_off % 4 == 0, "%s: image %d: dst_off must be a non-negative multiple of 4", who, i);
        const long long window = (long long)r.dst_h * r.win_w;
        long long n_pix = window;
        if (r.n_idx != 0) {
            CAR_REQUIRE(idx_host && idx_dev, "%s: image %d: sparse form without an index list (null pointer)", who, i);
            CAR_REQUIRE(r.n_idx > 0 && r.idx_off >= 0 && (size_t)r.idx_off + (size_t)r.n_idx <= n_idx_total,
                        "%s: image %d: its %d indices at %lld lie outside the list of %zu", who, i, r.n_idx, r.idx_off, n_idx_total);
            for (int k = 0; k < r.n_idx; ++k) {
                const int p = idx_host[r.idx_off + k];
                CAR_REQUIRE(p >= 0 && p < kMaxIndex && p < window, "%s: image %d: pixel index %d (entry %d) is outside the written window", who, i, p, k);
            }
            n_pix = r.n_idx;
        }
        CAR_REQUIRE((size_t)r.dst_off + 3 * (size_t)n_pix <= dst_elems, "%s: image %d: its output ends outside dst (%zu elements)", who, i, dst_elems);
        CAR_REQUIRE(n_pix <= (1 << 24), "%s: image %d: too many pixels", who, i);
        if (n_pix > max_pix) max_pix = (int)n_pix;
    }
    *groups_per_image = (int)car_div_up(max_pix, kThreads * kQuad);
    return CAR_OK;
}

template <typename OutT>
int launch(const char* who, const unsigned char* src, const car_frame_rec* recs_dev, int n_images, const int* idx_dev, const int* tables, OutT* dst,
           int groups_per_image, void* stream) {
    FrameArgs a;
    a.src = src, a.recs = recs_dev, a.idx = idx_dev, a.tables = reinterpret_cast<const int4*>(tables), a.dst = dst;
    a.n_images = n_images, a.groups_per_image = groups_per_image;
    const long items = (long)n_images * groups_per_image;
    const unsigned grid = (unsigned)(items < 8192 ? items : 8192);
    hipLaunchKernelGGL(frames_resize_kernel<OutT>, dim3(grid), dim3(kThreads), 0, (hipStream_t)stream, a);
    CAR_CHECK_LAUNCH(who);
    return CAR_OK;
}

}  // namespace

extern "C" size_t car_frames_table_ints(void) { return (size_t)kLutAt + 256; }

extern "C" int car_frames_table_slot(int n_src, int n_dst) { return table_slot(n_src, n_dst); }

extern "C" int car_frames_resize_u8(const unsigned char* src, size_t src_bytes, const car_frame_rec* recs_host, const car_frame_rec* recs_dev,
                                    int n_images, const int* tables, unsigned char* dst, size_t dst_elems, void* stream) {
    int groups = 0;
    CAR_TRY(validate("car_frames_resize_u8", src, src_bytes, recs_host, recs_dev, n_images, nullptr, nullptr, 0, tables, dst, dst_elems, sizeof(unsigned char),
                     &groups));
    return launch<unsigned char>("car_frames_resize_u8", src, recs_dev, n_images, nullptr, tables, dst, groups, stream);
}

extern "C" int car_frames_resize_f32(const unsigned char* src, size_t src_bytes, const car_frame_rec* recs_host, const car_frame_rec* recs_dev,
                                     int n_images, const int* idx_host, const int* idx_dev, size_t n_idx_total, const int* tables, float* dst,
                                     size_t dst_elems, void* stream) {
    int groups = 0;
    CAR_TRY(validate("car_frames_resize_f32", src, src_bytes, recs_host, recs_dev, n_images, idx_host, idx_dev, n_idx_total, tables, dst, dst_elems,
                     sizeof(float), &groups));
    return launch<float>("car_frames_resize_f32", src, recs_dev, n_images, idx_dev, tables, dst, groups, stream);
}

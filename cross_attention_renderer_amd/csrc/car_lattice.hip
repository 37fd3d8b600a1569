// car_lattice.hip — the merged lattice of a feature pyramid: every projected level summed onto the levels' common lattice, which the fused
// per-sample kernel (car_fused.hip) gathers from.  car_project_maps (car_render.hip) merges through car_launch_merge; car_merge_lattice and
// car_merge_lattice_max are the entries of hosts that project the levels themselves (include/car_hip.h).
#include "car_common.h"

namespace {

#include "car_fused_layout.h"

// The merged lattice (car_geom.h car_lattice_taps): node (jy, jx) of map (m, mode) = sum over the levels of the bilinear
// interpolation of the projected level G_l[m] at lattice coordinate u = j - pad, i.e. at texel coordinate (u + 1 - r_l) / (2 r_l) of
// a level r_l times coarser than the finest, with the level's own padding rule (mode 0 border, 1 zeros).
// A 16-lane group owns one node of one map and writes BOTH padding modes of it: the taps and weights of every level are worked out
// once per node (per 16-lane group, not per float4 of channels: that arithmetic used to be most of the kernel's time); a source row
// both modes read with a non-zero weight — every tap of an interior node — is loaded once; taps of weight zero (three of four on
// the finest level's own texel centres) get an out-of-range buffer offset: the load returns zeros without touching memory, and an
// instruction whose lanes are all out of range costs the texture path nothing (profiles/round3_fused_experiments.md).  No branch
// per tap, so a whole channel step's loads are in flight together.  Lane `sub` takes the channel quads sub + 16 j: a load / store
// instruction of the group moves 256 contiguous bytes.  The sums run in the order the one-mode kernel used (levels from the last
// index down, taps nw ne sw se, one fused multiply-add each; a skipped tap had weight zero), so the values are the same up to the
// sign of an exact zero.
// gmax (optional): the largest |lattice value| goes there (atomic max of the bit pattern: non-negative floats order like integers; the
// caller zeroes it) — one atomic per workgroup of a grid-stride launch; it bounds h in the fused kernel's fp16 split.
struct MergeArgs {
    const float* g[CAR_MAX_LEVELS];   // level l of the launch's first map
    unsigned bytes[CAR_MAX_LEVELS];   // the launch's maps of level l: range of the buffer loads (< 2 GiB, car_project_maps slices the maps)
    int h[CAR_MAX_LEVELS], w[CAR_MAX_LEVELS], r[CAR_MAX_LEVELS];
    int n_levels, lh, lw, pad;
    long nodes;                       // maps of the launch * lh * lw
    long per;                         // consecutive nodes per workgroup
    int ny;                           // lattice rows a workgroup's nodes can span (its y-axis table)
    float* lat;                       // [maps][2][lh][lw][kC] of the launch's first map
};
typedef float mf32x4 __attribute__((ext_vector_type(4)));
typedef float mf32x2 __attribute__((ext_vector_type(2)));
constexpr unsigned kNoTap = 0xc0000000u;          // beyond any sliced level: the load returns zeros
// Level l's four taps at node (jx, jy) of the launch's map m, for the lane that owns channel quad `sub`: ob = byte offset of the load
// that serves border mode — or, where border mode's weight is zero and zeros mode's is not, zeros mode's texel (e.g. on the ring just
// outside the map) — kNoTap when neither needs it; wb the border weight of what that load returns, ws the zeros weight.  Should both
// modes ever need DIFFERENT texels for one tap, `second` is set and (oz, wn) describe the extra load of the slow path.
struct LevelTaps { unsigned ob[4], oz[4]; float wb[4], ws[4], wn[4]; bool second; };
// One axis of car_bilinear_taps_px (car_geom.h): the two clamped texel indices of texel coordinate i and their weights, a weight forced to
// zero where its texel lies outside the level.  The 2-D weights are the products of the two axes' — the products car_bilinear_taps_px forms,
// zero exactly where it masks — so a node's taps come from one entry per axis, level and padding mode: 2 (lw + rows) entries per level
// instead of a page of arithmetic per node.
struct AxisTap { int c0, c1; float w0, w1; };
__device__ __forceinline__ AxisTap axis_tap(float i, int W, int mode) {
    if (mode == 0) i = fminf(fmaxf(i, 0.0f), (float)(W - 1));
    if (!(i > -4.0f)) i = -4.0f;
    if (i > (float)W + 4.0f) i = (float)W + 4.0f;
    const float f0 = floorf(i), f1 = f0 + 1.0f;
    const int x0 = (int)f0, x1 = x0 + 1;
    AxisTap t;
    t.w0 = (x0 >= 0 && x0 < W) ? f1 - i : 0.0f;
    t.w1 = (x1 >= 0 && x1 < W) ? i - f0 : 0.0f;
    t.c0 = x0 < 0 ? 0 : (x0 >= W ? W - 1 : x0);
    t.c1 = x1 < 0 ? 0 : (x1 >= W ? W - 1 : x1);
    return t;
}
__device__ __forceinline__ float lattice_to_texel(int j, int pad, int r) { return (float)(j - pad + 1 - r) / (float)(2 * r); }
__device__ __forceinline__ float4 axis_entry(const AxisTap& t) { return make_float4(__int_as_float(t.c0), __int_as_float(t.c1), t.w0, t.w1); }
__device__ __forceinline__ AxisTap axis_of(const float4& e) { return AxisTap{__float_as_int(e.x), __float_as_int(e.y), e.z, e.w}; }
// the level's four taps of both padding modes (xb / yb: border, xz / yz: zeros) -> what the node's loads and sums need
__device__ __forceinline__ LevelTaps level_taps(const AxisTap& xb, const AxisTap& yb, const AxisTap& xz, const AxisTap& yz, int W, unsigned mbase, int sub) {
    LevelTaps T;
    const int tb[4] = {yb.c0 * W + xb.c0, yb.c0 * W + xb.c1, yb.c1 * W + xb.c0, yb.c1 * W + xb.c1};
    const int tz[4] = {yz.c0 * W + xz.c0, yz.c0 * W + xz.c1, yz.c1 * W + xz.c0, yz.c1 * W + xz.c1};
    const float wz[4] = {xz.w0 * yz.w0, xz.w1 * yz.w0, xz.w0 * yz.w1, xz.w1 * yz.w1};
    T.wb[0] = xb.w0 * yb.w0; T.wb[1] = xb.w1 * yb.w0; T.wb[2] = xb.w0 * yb.w1; T.wb[3] = xb.w1 * yb.w1;
    T.second = false;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const bool on0 = T.wb[t] != 0.0f, on1 = wz[t] != 0.0f;
        const bool borrow = on1 && !on0, second = on1 && on0 && tz[t] != tb[t];
        T.ob[t] = (on0 || borrow) ? (mbase + (unsigned)(borrow ? tz[t] : tb[t])) * (unsigned)(kC * 4) + 16u * sub : kNoTap;
        T.oz[t] = second ? (mbase + (unsigned)tz[t]) * (unsigned)(kC * 4) + 16u * sub : kNoTap;
        T.ws[t] = (on1 && !second) ? wz[t] : 0.0f;
        T.wn[t] = second ? wz[t] : 0.0f;
        T.second = T.second || second;
    }
    return T;
}
__device__ __forceinline__ void merge_fma(float w, const mf32x4& v, mf32x2& lo, mf32x2& hi) {
    const mf32x2 w2 = {w, w};
    lo = __builtin_elementwise_fma(w2, mf32x2{v[0], v[1]}, lo);
    hi = __builtin_elementwise_fma(w2, mf32x2{v[2], v[3]}, hi);
}
// TAB: a workgroup owns `per` consecutive nodes (a few lattice rows) and keeps the axis entries of its columns and rows in LDS;
// otherwise (lattices too wide for that) the nodes are dealt out 16 at a time and every node works its entries out itself.
template <int NL, bool TAB>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 3))) merge_kernel(const MergeArgs a, unsigned* __restrict__ gmax) {
    __shared__ float red[4];
    extern __shared__ __attribute__((aligned(16))) float4 tab[];       // TAB: x axis [NL][2 modes][lw], then y axis [NL][2][a.ny]
    const int sub = threadIdx.x & 15;
    const long plane = (long)a.lh * a.lw;
    __amdgpu_buffer_rsrc_t rs[NL];
#pragma unroll
    for (int l = 0; l < NL; ++l) rs[l] = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.g[l]), 0, (int)a.bytes[l], 0x00027000);
    const long first = TAB ? (long)blockIdx.x * a.per : (long)blockIdx.x * 16;
    const long last = TAB ? (first + a.per < a.nodes ? first + a.per : a.nodes) : a.nodes;
    const long stride = TAB ? 16 : (long)gridDim.x * 16;
    const long row0 = first / a.lw;                                   // first lattice row (counted through the maps) of this workgroup
    float4* ytab = tab + NL * 2 * a.lw;
    if constexpr (TAB) {
        for (int i = threadIdx.x; i < NL * 2 * a.lw; i += 256) {
            const int l = i / (2 * a.lw), md = (i / a.lw) & 1, jx = i % a.lw;
            tab[i] = axis_entry(axis_tap(lattice_to_texel(jx, a.pad, a.r[l]), a.w[l], md));
        }
        for (int i = threadIdx.x; i < NL * 2 * a.ny; i += 256) {
            const int l = i / (2 * a.ny), md = (i / a.ny) & 1, jy = (int)((row0 + i % a.ny) % a.lh);
            ytab[i] = axis_entry(axis_tap(lattice_to_texel(jy, a.pad, a.r[l]), a.h[l], md));
        }
        __syncthreads();
    }
    float mx = 0.0f;
    // Tried and dropped (round 5, tools/bench_merge.py): a wave's four nodes 8 apart, so that they agree on which taps carry weight zero and a
    // dead tap is an instruction whose lanes are ALL out of range: 1.08 -> 1.5 ms (the wave's stores then fall on four distant rows); 64 lanes
    // per node (1 KB contiguous per load / store instruction, the third step a quarter full): 1.15 -> 1.46 ms = the extra instructions.
    for (long node = first + (threadIdx.x >> 4); node < last; node += stride) {
        const long row = node / a.lw;
        const int m = (int)(row / a.lh);
        const int jy = (int)(row - (long)m * a.lh), jx = (int)(node - row * a.lw);
        auto taps_of = [&](int l) {
            const unsigned mbase = (unsigned)m * (unsigned)(a.h[l] * a.w[l]);
            if constexpr (TAB) {
                const int ry = (int)(row - row0);
                return level_taps(axis_of(tab[(l * 2 + 0) * a.lw + jx]), axis_of(ytab[(l * 2 + 0) * a.ny + ry]), axis_of(tab[(l * 2 + 1) * a.lw + jx]),
                                  axis_of(ytab[(l * 2 + 1) * a.ny + ry]), a.w[l], mbase, sub);
            } else {
                const float ix = lattice_to_texel(jx, a.pad, a.r[l]), iy = lattice_to_texel(jy, a.pad, a.r[l]);
                return level_taps(axis_tap(ix, a.w[l], 0), axis_tap(iy, a.h[l], 0), axis_tap(ix, a.w[l], 1), axis_tap(iy, a.h[l], 1), a.w[l], mbase, sub);
            }
        };
        unsigned ob[NL][4];
        float wb[NL][4], ws[NL][4];
        bool second = false;
#pragma unroll
        for (int l = 0; l < NL; ++l) {
            const LevelTaps T = taps_of(l);
#pragma unroll
            for (int t = 0; t < 4; ++t) { ob[l][t] = T.ob[t]; wb[l][t] = T.wb[t]; ws[l][t] = T.ws[t]; }
            second = second || T.second;
        }
        float* out0 = a.lat + (((long)m * 2 + 0) * plane + (long)jy * a.lw + jx) * kC + 4 * sub;
        float* out1 = out0 + plane * kC;
        const bool slow = __builtin_amdgcn_ballot_w64(second) != 0;   // wave-uniform
        // three channel steps per trip: a trip's loads (up to 36 per lane) are in flight together
#pragma unroll 3
        for (int j = 0; j < kC / 64; ++j) {
            mf32x2 a0l = {0.f, 0.f}, a0h = {0.f, 0.f}, a1l = {0.f, 0.f}, a1h = {0.f, 0.f};
            if (!slow) {                                               // one load per live tap serves both modes; every level's in flight together
                mf32x4 v[NL][4];
#pragma unroll
                for (int l = 0; l < NL; ++l)
#pragma unroll
                    for (int t = 0; t < 4; ++t) v[l][t] = __builtin_bit_cast(mf32x4, __builtin_amdgcn_raw_buffer_load_b128(rs[l], (int)ob[l][t], 256 * j, 0));
#pragma unroll
                for (int l = NL - 1; l >= 0; --l)
#pragma unroll
                    for (int t = 0; t < 4; ++t) { merge_fma(wb[l][t], v[l][t], a0l, a0h); merge_fma(ws[l][t], v[l][t], a1l, a1h); }
            } else {                                                   // never seen with the two padding rules of grid_sample; kept for safety
#pragma unroll 1
                for (int l = NL - 1; l >= 0; --l) {
                    const LevelTaps T = taps_of(l);
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        const mf32x4 v = __builtin_bit_cast(mf32x4, __builtin_amdgcn_raw_buffer_load_b128(rs[l], (int)T.ob[t], 256 * j, 0));
                        const mf32x4 u = __builtin_bit_cast(mf32x4, __builtin_amdgcn_raw_buffer_load_b128(rs[l], (int)T.oz[t], 256 * j, 0));
                        merge_fma(T.wb[t], v, a0l, a0h); merge_fma(T.ws[t], v, a1l, a1h); merge_fma(T.wn[t], u, a1l, a1h);
                    }
                }
            }
            *reinterpret_cast<float4*>(out0 + 64 * j) = make_float4(a0l[0], a0l[1], a0h[0], a0h[1]);
            *reinterpret_cast<float4*>(out1 + 64 * j) = make_float4(a1l[0], a1l[1], a1h[0], a1h[1]);
            mx = fmaxf(fmaxf(mx, fmaxf(fmaxf(fabsf(a0l[0]), fabsf(a0l[1])), fmaxf(fabsf(a0h[0]), fabsf(a0h[1])))),
                       fmaxf(fmaxf(fabsf(a1l[0]), fabsf(a1l[1])), fmaxf(fabsf(a1h[0]), fabsf(a1h[1]))));
        }
    }
    if (gmax) {
        mx = wave_max(mx);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
        __syncthreads();
        if (threadIdx.x == 0) atomicMax(gmax, __float_as_uint(fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]))));
    }
}
// as many workgroups as the chip holds at once (three 4-wave workgroups per compute unit at this kernel's 168 registers: a grid that
// needs a partial second helping of workgroups per compute unit ends on a half-empty chip)
inline long merge_resident_blocks() {
    static int cus = 0;
    if (cus == 0) {
        int dev = 0;
        hipDeviceProp_t p;
        cus = (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&p, dev) == hipSuccess && p.multiProcessorCount > 0) ? p.multiProcessorCount : 256;
    }
    return 3L * cus;
}
}  // namespace

// the merge over n_maps maps, in launches whose widest level stays below the 2 GiB a buffer load addresses
int car_launch_merge(const float* const* levels, const int* hs, const int* ws, const int* rs, int n_levels, int lh, int lw, int pad, int n_maps,
                     float* lattice, unsigned* gmax, hipStream_t st, const char* who) {
    long widest = 0;
    for (int l = 0; l < n_levels; ++l) widest = (long)hs[l] * ws[l] > widest ? (long)hs[l] * ws[l] : widest;
    const long per = 0x7fffffffL / (widest * kC * 4);
    CAR_REQUIRE(per >= 1, "%s: one map of the widest level exceeds 2 GiB", who);
    for (int m0 = 0; m0 < n_maps; m0 += (int)per) {
        const int nm = n_maps - m0 < per ? n_maps - m0 : (int)per;
        MergeArgs a{};
        for (int l = 0; l < n_levels; ++l) {
            a.g[l] = levels[l] + (long)m0 * hs[l] * ws[l] * kC;
            a.bytes[l] = (unsigned)((long)nm * hs[l] * ws[l] * kC * 4);
            a.h[l] = hs[l]; a.w[l] = ws[l]; a.r[l] = rs[l];
        }
        a.n_levels = n_levels; a.lh = lh; a.lw = lw; a.pad = pad;
        a.nodes = (long)nm * lh * lw;
        a.lat = lattice + (long)m0 * 2 * lh * lw * kC;
        // consecutive nodes per workgroup (a multiple of the 16 a workgroup takes per step), the rows they span, the tables' LDS
        const long groups = (a.nodes + 15) / 16, resident = merge_resident_blocks();
        long blocks = groups < resident ? groups : resident;
        a.per = ((a.nodes + blocks - 1) / blocks + 15) / 16 * 16;
        blocks = (a.nodes + a.per - 1) / a.per;
        a.ny = (int)(a.per / lw) + 2;
        const size_t tab_bytes = (size_t)n_levels * 2 * (lw + a.ny) * sizeof(float4);
        const bool tables = tab_bytes <= 52 * 1024;                   // three workgroups per compute unit keep theirs in the 160 KB
#define CAR_MERGE_KERNEL(T) (n_levels == 1 ? merge_kernel<1, T> : n_levels == 2 ? merge_kernel<2, T> : n_levels == 3 ? merge_kernel<3, T> : merge_kernel<4, T>)
        void (*kern)(const MergeArgs, unsigned*) = tables ? CAR_MERGE_KERNEL(true) : CAR_MERGE_KERNEL(false);
#undef CAR_MERGE_KERNEL
        CAR_LAUNCH_LDS(who, kern, dim3((unsigned)blocks), dim3(256), tables ? tab_bytes : 0, st, a, gmax);
    }
    return CAR_OK;
}
// Every level is summed on the lattice: it must be an integer factor r_l coarser than the widest level, the same factor in both
// directions; lat = 2 W_max + 2 r_max + 1 nodes, pad = r_max + 1 (521 x 521 nodes, pad 5, for the 64 / 128 / 256 pyramid of a 256 x 256
// frame: 2.5 GB per scene for two views and two padding modes).
car_lattice car_lattice_of(const car_dims& d) {
    car_lattice L{};
    int hm = 0, wm = 0, rmax = 1;
    for (int l = 0; l < d.n_levels; ++l) {
        hm = d.level_h[l] > hm ? d.level_h[l] : hm; wm = d.level_w[l] > wm ? d.level_w[l] : wm;
    }
    L.ok = d.n_levels > 0;
    for (int l = 0; l < d.n_levels && L.ok; ++l) {
        const int h = d.level_h[l], w = d.level_w[l];
        L.ok = h > 0 && w > 0 && hm % h == 0 && wm % w == 0 && hm / h == wm / w;
        if (L.ok) { L.r[l] = hm / h; rmax = L.r[l] > rmax ? L.r[l] : rmax; }
    }
    L.pad = rmax + 1;
    L.h = 2 * hm + 2 * rmax + 1; L.w = 2 * wm + 2 * rmax + 1;
    return L;
}

// The body of both entries: the argument checks, the levels' common lattice (written to lat_h / lat_w / lat_pad where given; lattice NULL:
// nothing else), then the merge, with the lattice's largest magnitude in the same pass where gmax is given (zeroed here).
static int merge_entry(const char* who, const float* const* levels, const int* level_h, const int* level_w, int n_levels, int n_maps, float* lattice,
                       int* lat_h, int* lat_w, int* lat_pad, float* gmax, void* stream) {
    CAR_REQUIRE(levels && level_h && level_w && n_levels > 0 && n_levels <= CAR_MAX_LEVELS && n_maps > 0, "%s: bad arguments", who);
    car_dims d{};
    d.b = n_maps; d.V = 1; d.n_levels = n_levels;
    for (int l = 0; l < n_levels; ++l) { d.level_h[l] = level_h[l]; d.level_w[l] = level_w[l]; }
    const car_lattice L = car_lattice_of(d);
    CAR_REQUIRE(L.ok, "%s: every level must be an integer factor coarser than the widest one, the same factor in both directions", who);
    if (lat_h) *lat_h = L.h;
    if (lat_w) *lat_w = L.w;
    if (lat_pad) *lat_pad = L.pad;
    if (!lattice) return CAR_OK;
    for (int l = 0; l < n_levels; ++l) CAR_REQUIRE(levels[l], "%s: level %d is null", who, l);
    if (gmax && hipMemsetAsync(gmax, 0, sizeof(float), (hipStream_t)stream) != hipSuccess) { car_set_error("%s: memset failed", who); return CAR_E_LAUNCH; }
    return car_launch_merge(levels, level_h, level_w, L.r, n_levels, L.h, L.w, L.pad, n_maps, lattice, reinterpret_cast<unsigned*>(gmax), (hipStream_t)stream, who);
}

// The lattice alone, for hosts that project the levels themselves (engine.py: the three-view exchange, which has no plan): levels[l] =
// the projected level [n_maps, level_h[l], level_w[l], 576] channel-last; lattice = [n_maps][2 padding modes][lat_h][lat_w][576] (NULL: only
// the shape is returned).
extern "C" int car_merge_lattice(const float* const* levels, const int* level_h, const int* level_w, int n_levels, int n_maps, float* lattice,
                                 int* lat_h, int* lat_w, int* lat_pad, void* stream) {
    return merge_entry("car_merge_lattice", levels, level_h, level_w, n_levels, n_maps, lattice, lat_h, lat_w, lat_pad, nullptr, stream);
}
// The same, and the lattice's largest magnitude in the same pass (gmax [1]: zeroed here, then one atomic per workgroup of the merge) — what
// car_fused_rows takes as `gmeta`; no separate reduction over the gigabyte of lattice.
extern "C" int car_merge_lattice_max(const float* const* levels, const int* level_h, const int* level_w, int n_levels, int n_maps, float* lattice,
                                     float* gmax, void* stream) {
    CAR_REQUIRE(lattice && gmax, "car_merge_lattice_max: bad arguments");
    return merge_entry("car_merge_lattice_max", levels, level_h, level_w, n_levels, n_maps, lattice, nullptr, nullptr, nullptr, gmax, stream);
}

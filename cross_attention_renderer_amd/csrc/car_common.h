// car_common.h — error plumbing and the library-internal prototypes shared by the translation units of libcar_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include "../../include/car_hip.h"
#include "car_workspace.h"

void car_set_error(const char* fmt, ...);

#define CAR_REQUIRE(cond, ...)                         \
    do {                                               \
        if (!(cond)) {                                 \
            car_set_error(__VA_ARGS__);                \
            return CAR_E_ARG;                          \
        }                                              \
    } while (0)

// Checks the launch itself (configuration / missing code object); never synchronises.
#define CAR_CHECK_LAUNCH(name)                                                        \
    do {                                                                              \
        hipError_t e_ = hipGetLastError();                                            \
        if (e_ != hipSuccess) {                                                       \
            car_set_error("%s: launch failed: %s", name, hipGetErrorString(e_));      \
            return CAR_E_LAUNCH;                                                      \
        }                                                                             \
    } while (0)

// -DCAR_BOUNDS (tools/build_bounds.py; tests/oob_runner.py with CAR_OOB_LIB): a debug build in which every LDS-DMA / buffer-load / row-load
// helper of the kernels compares the range it is about to read with the extent its launcher passed in the args struct and TRAPS when it
// leaves it — the one way to see a read whose value nobody uses (the NaN-margin harness only sees reads that reach a result).  The
// product build compiles these to nothing.
#ifdef CAR_BOUNDS
#define CAR_BOUNDS_TRAP(cond) do { if (!(cond)) __builtin_trap(); } while (0)
#else
#define CAR_BOUNDS_TRAP(cond) do { } while (0)
#endif

static inline unsigned car_div_up(long a, long b) { return (unsigned)((a + b - 1) / b); }
static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// ---- device side: what several units' kernels share ----
// Reduction over the wave's 64 lanes by a fixed xor butterfly (32, 16, .. 1): every lane ends with the same bits, and the order of the
// additions is part of what the bit-for-bit suites pin.  T: float, double, unsigned (wave_max: float, double)
template <class T>
__device__ __forceinline__ T wave_sum(T v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
template <class T>
__device__ __forceinline__ T wave_max(T v) {
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}
// sample s = v P + p of ray (sc, r) lives at row ((sc V + v) R + r) P + p of the per-sample arrays (logits, weights, value rows, pt)
__device__ __forceinline__ long car_sample_row(int sc, int r, int s, int V, int R, int P) { return ((long)(sc * V + s / P) * R + r) * P + (s % P); }

// a C++ function that one unit defines for another: kept out of the library's dynamic symbols
#define CAR_INTERNAL __attribute__((visibility("hidden")))

#define CAR_TRY(call)                 \
    do {                              \
        const int rc_ = (call);       \
        if (rc_ != CAR_OK) return rc_; \
    } while (0)

// A HIP runtime call (memset, copy, event) that must succeed: the error text is the caller's
#define CAR_CHECK_HIP(call, ...)              \
    do {                                      \
        if ((call) != hipSuccess) {           \
            car_set_error(__VA_ARGS__);       \
            return CAR_E_LAUNCH;              \
        }                                     \
    } while (0)

// The launch of a kernel with dynamic LDS: reserve, clear the sticky error, launch, check (returns from the calling function on failure).
// car_reserve_lds (car_api.hip): the reservation is a per-device attribute of the kernel, set once per (kernel, device) — not on each of
// the dozens of launches of a step — and again when a call asks for more than the largest reserved so far.  Its refusal is CAR_E_LAUNCH
// with the one error text worded there: a contract, engine._lds_refused lets a route step down to its next kernel on this code and text.
CAR_INTERNAL int car_reserve_lds(const void* kernel, size_t bytes, const char* entry);
#define CAR_LAUNCH_LDS(entry, kernel, grid, block, lds_bytes, stream, ...)            \
    do {                                                                              \
        CAR_TRY(car_reserve_lds((const void*)(kernel), lds_bytes, entry));            \
        (void)hipGetLastError();                                                      \
        hipLaunchKernelGGL(kernel, grid, block, lds_bytes, stream, __VA_ARGS__);      \
        CAR_CHECK_LAUNCH(entry);                                                      \
    } while (0)

// ---- library-internal functions that one unit defines and another calls.  Declared here and nowhere else: the defining and the calling
// unit both include this header, so a parameter list that drifts on one side is a compile error, not a call that links and runs. ----
// car_fused.hip: the fp16 instance of the fused per-sample kernel and its compact blob's size.  Reached through car_render_forward_f16;
// exported (C linkage) for tools/bench_fused.py, not part of include/car_hip.h.  Arguments as car_fused_samples_parts.
extern "C" size_t car_fused_blob16_floats(void);
extern "C" int car_fused_samples_f16(const float* poses, const float* rays, const float* steps, const float* lattice, int lat_h, int lat_w,
                                     int lat_pad, const float* gmeta, const float* wpt, const float* blob16, const float* bias, int b, int V, int R,
                                     int P, int H, int W, int no_sample, float* e, float* g, float* logit, float* pt, float* pixel_val,
                                     float* part, void* stream);
// car_pack.hip: car_fused_pack with the compact (hi halves only) blob of the fp16 precision; same bias table and point table
CAR_INTERNAL int car_fused_pack_hi(const car_weights* w, float* blob16, float* bias, float* wpt, void* stream);
// car_pack.hip: the layer maximum and the two tile writers that every packed layer goes through (formats: the kernels' comments there).
// car_pack_scale says where a layer's power of two comes from and goes to.  max set: car_pack_absmax (any grid) raises *max, zeroed by
// the caller, to the largest magnitude as a bit pattern; the tile writer derives p = 2^shift from it and stores p and 1 / p.  max null:
// car_pack_absmax (ONE workgroup) stores p and 1 / p itself, and the tile writer reads *p (inv may then be null).
struct car_pack_scale { float* max; float* p; float* inv; };
CAR_INTERNAL void car_pack_absmax(hipStream_t st, int blocks, const float* W, int ldw, const float* W2, const float* bias, int N, int K, car_pack_scale s);
CAR_INTERNAL void car_pack_rows16(hipStream_t st, int blocks, const float* W, int ldw, const float* bias, int N, int K, int n_tiles, int ksteps,
                                  int chained, int kbase, car_pack_scale s, _Float16* out, bool hi_only = false);
CAR_INTERNAL void car_pack_conv16(hipStream_t st, int blocks, const float* w, int K, int N, bool flip, car_pack_scale s, _Float16* out);
// car_conv.hip: a packed 3x3 layer is car_conv3x3_tile_floats(K, N) floats of tiles — 9 K / 32 x N / 16 tiles of 512 floats, [K step][tile]
// [hi | lo][lane][8 halves] with k = tap * K + channel — then 64 floats of scale (2^shift, 2^-shift, the largest magnitude, zeros) and, where
// `bias` is given, its N floats behind them.  flip: the data gradient's weights, transposed and with the taps reversed.  K, N: the packed
// matrix's inputs per tap and outputs.  who: the entry named in an error
CAR_INTERNAL size_t car_conv3x3_tile_floats(int K, int N);
CAR_INTERNAL int car_conv3x3_pack_tiles(const char* who, const float* w, const float* bias, int K, int N, bool flip, float* packed, hipStream_t st);
// car_conv.hip: the launchers of the 3x3 sweep's three forms and of the 7x7 first layer; the callers have checked shapes and alignment.
// car_conv3x3_lpips: M = n H W pixels, K -> N the SWEEP's widths (the data gradient's are the forward layer's exchanged; it has no bias and
// takes act and add).  car_conv3x3_general and car_conv7x7: pt, pl the padding in front, Ho x Wo the output's extents; who names the
// launch; epilogue chooses between the general form's two instances (false: no bias, residual or flag is read)
CAR_INTERNAL int car_conv3x3_lpips(const float* X, const float* packed, const float* act, const float* add, float* Y, int H, int W, int K, int N, long M,
                                   bool backward, hipStream_t st);
CAR_INTERNAL int car_conv3x3_general(const char* who, bool epilogue, const float* X, int n, int H, int W, int K, int N, int stride, int pt, int pl, int Ho, int Wo,
                                     const float* packed, const float* bias, const float* add, int flags, float* Y, hipStream_t st);
CAR_INTERNAL int car_conv7x7(const char* who, const float* x, int n, int H, int W, int stride, int pt, int pl, int Ho, int Wo, const float* w,
                             const float* bias, float* Y, hipStream_t st);
CAR_INTERNAL void car_pack_tiles32(hipStream_t st, int blocks, const float* W, int ldw, const float* W2, int N, int K, int tiles, int chunks, int kgs,
                                   int chained, car_pack_scale s, _Float16* out);
// car_lattice.hip: the common lattice of a pyramid's levels (only n_levels, level_h, level_w of d are read), and the merge onto it
struct car_lattice { int h, w, pad, r[CAR_MAX_LEVELS]; bool ok; };
CAR_INTERNAL car_lattice car_lattice_of(const car_dims& d);
CAR_INTERNAL int car_launch_merge(const float* const* levels, const int* hs, const int* ws, const int* rs, int n_levels, int lh, int lw, int pad, int n_maps,
                                  float* lattice, unsigned* gmax, hipStream_t st, const char* who);
// car_round2_attend.hip: whether car_attend_round2 takes the shape (the one-call forward asks before it chooses between the merged second
// round and the two launches)
CAR_INTERNAL bool car_attend_round2_supports(int D, int V, int P);

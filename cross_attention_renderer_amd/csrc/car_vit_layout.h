// car_vit_layout.h — the shapes and layouts the forward (car_vit.hip) and the backward (car_vit_backward.hip) of the encoder's transformer
// stage share: the accepted ranges, LayerNorm's row pass (LnRow), one block of car_vit_pack, the transposed matrices car_vit_pack_train lays out behind it, and the
// record car_vit_blocks_train saves per block (profiles/workspace_layout.md, "the transformer stage's backward").  Each layout is ONE
// function over a Carver: its total is what the size entry returns, its pieces are what the launchers use.
// Included INSIDE the including file's anonymous namespace, after car_common.h.
#pragma once

constexpr int kHead = 64;                          // head width
constexpr int kKeys = 32;                          // keys per tile = query rows per wave

bool mha_shape_ok(int b, int S, int heads, const char* who) {
    if (b < 1 || b > 4096) { car_set_error("%s: b = %d is outside 1..4096", who, b); return false; }
    if (S < 1 || S > 1024) { car_set_error("%s: S = %d is outside 1..1024", who, S); return false; }
    if (heads < 1 || heads > 16) { car_set_error("%s: heads = %d is outside 1..16", who, heads); return false; }
    return true;
}
// LayerNorm, forward and backward: a row of at most kLnMax floats lives in one wave's registers, kLnVec float4 per lane
constexpr int kLnMax = 4096, kLnVec = kLnMax / (64 * 4);
bool ln_shape_ok(int C, const char* who) {
    if (C < 4 || C > kLnMax || C % 4) { car_set_error("%s: C = %d must be a multiple of 4 in 4..%d", who, C, kLnMax); return false; }
    return true;
}
// one row in its wave's registers with its statistics in fp64: the mean first, then the variance from the squared distances to it.
// layernorm_kernel and ln_bwd_kernel both start here, so the backward's mean and rstd ARE the forward's
struct LnRow {
    static constexpr int kVec = kLnVec;
    float4 v[kVec];
    double mean, rstd;
    __device__ __forceinline__ void load(const float* x, int C, double eps, int lane) {
        double sum = 0.0;
#pragma unroll
        for (int i = 0; i < kVec; ++i) {
            const int c = (i * 64 + lane) * 4;
            v[i] = c < C ? *reinterpret_cast<const float4*>(x + c) : make_float4(0.f, 0.f, 0.f, 0.f);
            sum += ((double)v[i].x + (double)v[i].y) + ((double)v[i].z + (double)v[i].w);
        }
        mean = wave_sum(sum) / (double)C;
        double sq = 0.0;
#pragma unroll
        for (int i = 0; i < kVec; ++i) {
            if ((i * 64 + lane) * 4 < C) {
                const double a = (double)v[i].x - mean, b = (double)v[i].y - mean, c = (double)v[i].z - mean, d = (double)v[i].w - mean;
                sq += (a * a + b * b) + (c * c + d * d);
            }
        }
        rstd = 1.0 / sqrt(wave_sum(sq) / (double)C + eps);
    }
};
bool vit_dim_ok(int dim, const char* who) {
    if (dim < 64 || dim > 1024 || dim % 64) { car_set_error("%s: dim = %d must be a multiple of 64 in 64..1024", who, dim); return false; }
    return true;
}
bool vit_depth_ok(int depth, const char* who) {
    if (depth < 1 || depth > 32) { car_set_error("%s: depth = %d is outside 1..32", who, depth); return false; }
    return true;
}

// the layout of one block of car_vit_pack: item i of the 12 parameters at off[i], the block's size at off[12] (floats)
struct VitLayout { size_t off[13]; };
VitLayout vit_layout(int dim) {
    const size_t d = (size_t)dim;
    const size_t n[12] = {d, d, car_linear_x3_packed_floats(dim, 3 * dim), 3 * d, car_linear_x3_packed_floats(dim, dim), d, d, d,
                          car_linear_x3_packed_floats(dim, 4 * dim), 4 * d, car_linear_x3_packed_floats(4 * dim, dim), d};
    VitLayout l;
    Carver c(nullptr, 4);
    for (int i = 0; i < 12; ++i) l.off[i] = c.at<float>(n[i]);
    l.off[12] = c.bytes() / sizeof(float);
    return l;
}
// the parameters' shapes in car_vit_pack's order: a matrix's K (0: a vector) and every item's N
struct VitShapes { int k[12], n[12]; };
VitShapes vit_shapes(int dim) {
    return {{0, 0, dim, 0, dim, 0, 0, 0, dim, 0, 4 * dim, 0}, {dim, dim, 3 * dim, 3 * dim, dim, dim, dim, dim, 4 * dim, 4 * dim, dim, dim}};
}
// one block of a parameter gradient in torch layout: item i (N x K or N floats) at off[i], the block's size at off[12] (floats)
VitLayout vit_grad_layout(int dim) {
    const VitShapes s = vit_shapes(dim);
    VitLayout l;
    Carver c(nullptr, 4);
    for (int i = 0; i < 12; ++i) l.off[i] = c.at<float>((size_t)s.n[i] * (s.k[i] ? s.k[i] : 1));
    l.off[12] = c.bytes() / sizeof(float);
    return l;
}
// car_vit_pack_train: car_vit_pack's blocks first (every offset of theirs as it was), then per block the four TRANSPOSED matrices as
// car_linear_x3_pack lays them out — item t of qkv, proj, fc1, fc2 at off[t], the block's size at off[4] — then the scratch one
// transpose is written to before it is packed (4 dim x dim floats)
struct VitTrainLayout { size_t tr, off[5], scratch, total; };          // tr: where the transposed blocks start
VitTrainLayout vit_train_layout(int dim, int depth) {
    const size_t d = (size_t)dim;
    const size_t n[4] = {car_linear_x3_packed_floats(3 * dim, dim), car_linear_x3_packed_floats(dim, dim), car_linear_x3_packed_floats(4 * dim, dim),
                         car_linear_x3_packed_floats(dim, 4 * dim)};
    VitTrainLayout l;
    Carver b(nullptr, 4);
    for (int i = 0; i < 4; ++i) l.off[i] = b.at<float>(n[i]);
    l.off[4] = b.bytes() / sizeof(float);
    Carver c(nullptr, 4);
    c.at<float>(vit_layout(dim).off[12] * (size_t)depth);               // car_vit_pack's blocks, from 0
    l.tr = c.at<float>(l.off[4] * (size_t)depth);
    l.scratch = c.at<float>(4 * d * d);
    l.total = c.bytes() / sizeof(float);
    return l;
}
// what car_vit_blocks_train saves per block, pieces of whole 64 floats: the block's input, qkv, the attention output, the residual stream
// after the attention half, the fc1 pre-activation, and the softmax's (maximum, sum) per (scene, head, query row)
struct VitSaved { float *x0, *qkv, *att, *x1, *u, *stats; size_t block_bytes, total; };
VitSaved vit_saved(int b, int S, int dim, int depth, int blk = 0, const void* saved = nullptr) {
    const size_t rows = (size_t)b * S, d = (size_t)dim;
    Carver sz(nullptr, 64);
    sz.take<float>(rows * d); sz.take<float>(rows * 3 * d); sz.take<float>(rows * d); sz.take<float>(rows * d); sz.take<float>(rows * 4 * d);
    sz.take<float>(rows * (d / kHead) * 2);
    const size_t block = sz.bytes();
    Carver c(saved ? (const char*)saved + block * blk : nullptr, 64);
    VitSaved s{c.take<float>(rows * d), c.take<float>(rows * 3 * d), c.take<float>(rows * d), c.take<float>(rows * d), c.take<float>(rows * 4 * d),
               c.take<float>(rows * (d / kHead) * 2), block, block * (size_t)depth};
    return s;
}

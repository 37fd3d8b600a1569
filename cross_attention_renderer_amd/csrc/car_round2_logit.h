// car_round2_logit.h — the folded second-round logit of one sample, <q2, qry> / 16 = (y^T (M x + v) + u^T x + c) / 16 (car_round2_layout.h),
// in the form with short live ranges that the matrix waves of car_round2_attend.hip need.  car_round2.hip's round2g_kernel
// (car_round2_logits_from_g) makes the same products and sums in the same order from whole accumulator sets, which is faster where a
// kernel has the registers to itself; both take the sample's operand from split_g and the tile pieces from car_mma32.h, and
// tests/test_round2_attend_hip.py holds the two to the same bits.
// Included INSIDE the including file's anonymous namespace, behind car_mma32.h and car_round2_layout.h.
#pragma once

static_assert(kTile == kMma32Tile && kD == 32 * kNT && kD == 32 * kChunks, "the packers' tile is the one car_mma32.h reads");

// the lane's half of its sample's g row (lane (s, h): k = 8 h .. 8 h + 7) as the B operand of the K = 16 layers: g gp = ghi + glo,
// gp the sample's power of two, ginv = 1 / gp
__device__ __forceinline__ void split_g(const float4 g0, const float4 g1, half8& ghi, half8& glo, float& gp, float& ginv) {
    const float gx[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
    float m = 0.0f;
#pragma unroll
    for (int k = 0; k < 8; ++k) m = fmaxf(m, fabsf(gx[k]));
    m = fmaxf(m, __shfl_xor(m, 32, 64));
    pow2_scale(fmaxf(m, 1e-30f), gp, ginv);
    split8(gx, gp, ghi, glo);
}

// logit of this lane's sample (lane (s, h): sample s of the wave's 32, channel half h; both halves return it); the biases of all three
// layers are added AFTER the products, in true units, so the accumulators start from the matrix instruction's zero.  lds: the packs of
// car_round2q_pack at car_round2_layout.h's offsets; g0, g1: the lane's half of the sample's g row; ub: br1 + uh of the sample's
// ray (in LDS: the caller's tile of 32 samples lies inside one ray).  x is kept as its fp16 hi / lo operand halves (64 registers), M x and
// y are produced one 32-channel tile at a time (16 registers each) and dotted at once, in the order (t, gq, r).
__device__ __forceinline__ float sample_logit(const float* lds, const float4 g0, const float4 g1, const float* ub, int lane, int h) {
    const float* lb = lds + kLdsBiasG;
    const float down1 = lb[4 * kD], down2 = lb[4 * kD + 1], downq = lb[4 * kD + 2];
    half8 ghi, glo;
    float gp, ginv;
    split_g(g0, g1, ghi, glo, gp, ginv);
    // x = relu(Wq1 g + bq1), u^T x, and x's fp16 halves: the B operands of the folded layer (K step (c, kg) takes entries 8 kg .. 8 kg + 7 of tile c)
    half8 bhi[kChunks][2], blo[kChunks][2];
    float dot_u = 0.0f, xinv;
    {
        f32x16 xq[kNT];
#pragma unroll
        for (int t = 0; t < kNT; ++t) {
#pragma unroll
            for (int r = 0; r < 16; ++r) xq[t][r] = 0.0f;
            mma_k16(xq[t], lds + kLdsWq1, t, lane, ghi, glo);
        }
        const float undoq = downq * ginv;
        const float* lu = lb + 3 * kD;
        const float* lq = lb + 2 * kD;
        float xqm = 0.0f;
#pragma unroll
        for (int t = 0; t < kNT; ++t)
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
                const float4 u = row4(lu, t, gq, h);
                const float4 b = row4(lq, t, gq, h);
                const float uu[4] = {u.x, u.y, u.z, u.w}, bb[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float x = fmaxf(fmaf(xq[t][4 * gq + r], undoq, bb[r]), 0.0f);
                    xq[t][4 * gq + r] = x;
                    xqm = fmaxf(xqm, x);
                    dot_u = fmaf(uu[r], x, dot_u);
                }
            }
        xqm = fmaxf(xqm, __shfl_xor(xqm, 32, 64));
        float xp;
        pow2_scale(fmaxf(xqm, 1e-30f), xp, xinv);
#pragma unroll
        for (int c = 0; c < kChunks; ++c)
#pragma unroll
            for (int kg = 0; kg < 2; ++kg) {
                float x8[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) x8[e] = xq[c][8 * kg + e];
                split8(x8, xp, bhi[c][kg], blo[c][kg]);
            }
    }
    // per 32-channel tile t: y = relu(Wr1g g + br1 + uh) (K = 16), (M x) of the same channels (K = 128), and their products
    const float undo1 = down1 * ginv;
    const float* lv = lb + kD;
    float dot = 0.0f, dot_v = 0.0f;
#pragma unroll
    for (int t = 0; t < kNT; ++t) {
        f32x16 y, acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) { y[r] = 0.0f; acc[r] = 0.0f; }
        mma_k16(y, lds + kLdsW1, t, lane, ghi, glo);
#pragma unroll
        for (int c = 0; c < kChunks; ++c)
#pragma unroll
            for (int kg = 0; kg < 2; ++kg) {
                half8 ah, al;
                read_a(lds + (c * kNT + t) * kTile + kg * (kTile / 2) + 4 * lane, ah, al);
                mma3(acc, ah, al, bhi[c][kg], blo[c][kg]);
            }
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
            const float4 u = row4(ub, t, gq, h);
            const float4 v4 = row4(lv, t, gq, h);
            const float uu[4] = {u.x, u.y, u.z, u.w}, vv[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float yy = fmaxf(fmaf(y[4 * gq + r], undo1, uu[r]), 0.0f);
                dot = fmaf(yy, acc[4 * gq + r], dot);
                dot_v = fmaf(yy, vv[r], dot_v);
            }
        }
    }
    // y^T (M x) in the product's units, y^T v and u^T x in true ones
    dot = fmaf(dot, down2 * xinv, dot_u + dot_v);
    dot += __shfl_xor(dot, 32, 64);
    dot += lb[4 * kD + 3];
    return dot / 16.0f;
}

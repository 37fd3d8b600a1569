// car_chain_layout.h — the layer table of the two per-ray chain kernels (car_raychain.hip), shared by the kernels, their launcher and the
// host code that lays out, packs and walks the plan (car_render.hip).  Plain constants and constexpr functions only.
// Included INSIDE the including file's anonymous namespace, behind car_fused_layout.h (kC, kE, kD).
#pragma once

// ---- packed-tile geometry: a layer is [chunk (K = 32)][tile (32 output channels)][kg (2)][hi | lo][lane (64)][8 halves] ----------------
constexpr int kChunkK = 32, kTileN = 32;
constexpr int kTileFloats = 1024;                  // packed floats per (chunk, tile)
constexpr int kTileCounts[] = {1, 4, 9};           // tiles per chunk that Stream::landed has a counted wait for
constexpr int kMaxNT = 9;                          // the largest of them
constexpr int kRing = 3;                           // weight buffers: the chunk being multiplied and the two behind it
constexpr int kBufFloats = kMaxNT * kTileFloats;   // one weight buffer: 36 KB
constexpr int kMaxChunks = 96;                     // ChainArgs::chunk
constexpr int kMaxLayers = 16;                     // ChainArgs::layer, and the scale slots of a plan
constexpr int kScaleFloats = 2 * kMaxLayers;       // 2^shift of every slot, then 2^-shift (car_chain_pack)
constexpr int chain_chunks_of(int K) { return (K + kChunkK - 1) / kChunkK; }
constexpr int chain_tiles_of(int N) { return (N + kTileN - 1) / kTileN; }
constexpr size_t chain_packed_floats(int K, int N) { return (size_t)chain_chunks_of(K) * chain_tiles_of(N) * kTileFloats; }
constexpr bool chain_tile_count_ok(int nt) { return nt == kTileCounts[0] || nt == kTileCounts[1] || nt == kTileCounts[2]; }

// ---- the layers of a plan, by scale slot ------------------------------------------------------------------------------------------
constexpr int kPhiIn = 18, kPhiLd = 20;            // the decoder's ray input (phi_x): columns used, row stride
constexpr int kBlocks = 3;                         // residual blocks of the decoder: lin_z_i, fc_0_i, fc_1_i
enum {
    kSlotLatentValue = 0, kSlotEncodeLatent, kSlotQueryRepeat /* query_repeat_embed[:, :128] */, kSlotLinIn,
    kSlotBlocks,                                   // + 3 i + j: lin_z_i (j = 0), fc_0_i (1), fc_1_i (2)
    kSlotLinOut = kSlotBlocks + 3 * kBlocks,
    kChainLayers
};
constexpr int chain_block_slot(int i, int j) { return kSlotBlocks + 3 * i + j; }
// chained: the input is the previous layer's accumulator set (its K order), else rows from memory.  halves: the layer sees its input twice
// (lin_z_i([z, z])), its weight rows are 2 K wide and the two halves are added at pack time.  bias: the layer has a place in the bias tables
struct ChainLayer { int K, N; bool chained, halves, bias; };
constexpr ChainLayer kChainLayer[kChainLayers] = {
    {kC, kE, false, false, true},                  // latent_value
    {kE, kD, true, false, true},                   // encode_latent
    {kD, kD, true, false, false},                  // query_repeat_embed[:, :128]: its bias rides with the per-sample half (car_round2.hip)
    {kPhiIn, kD, false, false, true},              // lin_in
    {kE, kD, true, true, true}, {kD, kD, true, false, true}, {kD, kD, true, false, true},      // lin_z_0, fc_0_0, fc_1_0
    {kE, kD, true, true, true}, {kD, kD, true, false, true}, {kD, kD, true, false, true},      // block 1
    {kE, kD, true, true, true}, {kD, kD, true, false, true}, {kD, kD, true, false, true},      // block 2
    {kD, 3, true, false, true},                    // lin_out
};
constexpr int chain_chunks(int slot) { return chain_chunks_of(kChainLayer[slot].K); }
constexpr int chain_tiles(int slot) { return chain_tiles_of(kChainLayer[slot].N); }
constexpr size_t chain_floats(int slot) { return chain_packed_floats(kChainLayer[slot].K, kChainLayer[slot].N); }

// the order in which a plan holds the layers' tiles (car_render.hip, plan_layout): a plan's bytes depend on it, the kernels do not
constexpr int kPlanOrder[kChainLayers] = {kSlotLatentValue, kSlotLinIn, kSlotEncodeLatent, kSlotQueryRepeat, 4, 5, 6, 7, 8, 9, 10, 11, 12, kSlotLinOut};

// ---- the order in which each kernel consumes its layers ------------------------------------------------------------------------------
constexpr int kMidSeq[] = {kSlotLatentValue, kSlotEncodeLatent, kSlotQueryRepeat};
constexpr int kTailSeq[] = {kSlotLatentValue, kSlotLinIn, 4, 5, 6, 7, 8, 9, 10, 11, 12, kSlotLinOut};
constexpr int kMidLayers = sizeof(kMidSeq) / sizeof(int), kTailLayers = sizeof(kTailSeq) / sizeof(int);
// position of the tail's block layers and of lin_out in kTailSeq (what the kernel hands to ChainArgs::layer)
constexpr int kTailPosBlocks = 2, kTailPosLinOut = kTailPosBlocks + 3 * kBlocks;
constexpr int tail_block_pos(int i, int j) { return kTailPosBlocks + 3 * i + j; }
constexpr int chain_seq_chunks(const int* seq, int n_layers) {
    int n = 0;
    for (int i = 0; i < n_layers; ++i) n += chain_chunks(seq[i]);
    return n;
}

// ---- bias tables: the biases of a kernel's layers back to back in consumption order, each over whole tiles (add_bias reads 32 a tile) ----
constexpr int chain_bias_at(const int* seq, int pos) {
    int o = 0;
    for (int i = 0; i < pos; ++i) o += kChainLayer[seq[i]].bias ? chain_tiles(seq[i]) * kTileN : 0;
    return o;
}
constexpr int kMidBiasEncodeLatent = kE, kMidBiasFloats = kE + kD;
constexpr int kTailBiasLinIn = kE;
constexpr int tail_block_bias(int i, int j) { return kE + kD * (1 + 3 * i + j); }
constexpr int kTailBiasLinOut = kE + kD * (1 + 3 * kBlocks), kTailBiasFloats = kTailBiasLinOut + kTileN;   // lin_out's three, padded to a tile

// ---- drift is a compile error ------------------------------------------------------------------------------------------------------
constexpr bool chain_tiles_ok() {                  // every chunk fits a ring buffer and has a counted wait in Stream::landed
    for (int s = 0; s < kChainLayers; ++s)
        if (!chain_tile_count_ok(chain_tiles(s)) || chain_tiles(s) > kMaxNT) return false;
    return true;
}
constexpr bool chain_plan_order_ok() {             // kPlanOrder names every slot once
    int seen = 0;
    for (int s = 0; s < kChainLayers; ++s) seen |= 1 << kPlanOrder[s];
    return seen == (1 << kChainLayers) - 1;
}
constexpr bool chain_seq_ok(const int* seq, int n_layers) {
    for (int i = 0; i < n_layers; ++i)
        if (seq[i] < 0 || seq[i] >= kChainLayers) return false;
    return chain_seq_chunks(seq, n_layers) <= kMaxChunks;
}
constexpr bool chain_blocks_ok() {                 // the closed forms the tail kernel's unrolled loop uses are the table's
    for (int i = 0; i < kBlocks; ++i)
        for (int j = 0; j < 3; ++j)
            if (kTailSeq[tail_block_pos(i, j)] != chain_block_slot(i, j) || chain_bias_at(kTailSeq, tail_block_pos(i, j)) != tail_block_bias(i, j) ||
                kChainLayer[chain_block_slot(i, j)].halves != (j == 0))
                return false;
    return true;
}
static_assert(kChainLayers == 14 && kChainLayers <= kMaxLayers, "the plan's layers are its scale slots: 14, all below kMaxLayers");
static_assert(kMaxNT == kTileCounts[2] && chain_tiles_ok(), "a layer's tile count is 1, 4 or 9 (Stream::landed) and at most a ring buffer's");
static_assert(chain_plan_order_ok(), "kPlanOrder is a permutation of the slots");
static_assert(chain_seq_ok(kMidSeq, kMidLayers) && chain_seq_ok(kTailSeq, kTailLayers), "a sequence names plan slots and has at most kMaxChunks chunks");
static_assert(chain_seq_chunks(kMidSeq, kMidLayers) == 31 && chain_seq_chunks(kTailSeq, kTailLayers) == 74, "chunks per kernel");
static_assert(kMidSeq[1] == kSlotEncodeLatent && chain_bias_at(kMidSeq, 1) == kMidBiasEncodeLatent && chain_bias_at(kMidSeq, kMidLayers) == kMidBiasFloats,
              "mid bias table");
static_assert(kTailSeq[1] == kSlotLinIn && chain_bias_at(kTailSeq, 1) == kTailBiasLinIn && chain_blocks_ok() && kTailLayers == kTailPosLinOut + 1 &&
              kTailSeq[kTailPosLinOut] == kSlotLinOut && chain_bias_at(kTailSeq, kTailPosLinOut) == kTailBiasLinOut &&
              chain_bias_at(kTailSeq, kTailLayers) == kTailBiasFloats, "tail sequence and bias table");

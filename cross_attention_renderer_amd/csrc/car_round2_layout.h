// car_round2_layout.h — LDS / packed-weight layout of the second round's per-sample layers, shared by the kernels that hold the packs
// in LDS at these float offsets (car_round2.hip, car_round2_attend.hip and, for both, car_round2_logit.h) and by the packers that write
// them (car_pack.hip: car_round2_pack, car_round2q_pack).
// Included INSIDE the including file's anonymous namespace.
#pragma once

constexpr int kD = 128, kNT = 4, kTile = 1024, kChunks = 4;
constexpr int kWaves = 8, kStageLd = 36;
constexpr int kLdsW1 = kChunks * kNT * kTile;                       // Wr1g tiles after the 64 KB of Wr2: [4 tiles][hi|lo][64 lanes][8 halves]
constexpr int kLdsBias = kLdsW1 + kNT * 512;                        // br1 [128] | br2 [128] | 2^-shift of Wr1g, Wr2
constexpr int kLdsStage = kLdsBias + 2 * kD + 4;                    // [8 waves][32 rows][36]
constexpr size_t kLdsBytes = (size_t)(kLdsStage + kWaves * 32 * kStageLd) * sizeof(float);
// The folded form (car_round2_logits_from_g, car_attend_round2; car_round2_logit.h): no qry rows.  <q2, qry> with q2 = Wr2 y + br2, qry = Wq2 x + bq2 (y = relu(Wr1g g + br1 + uh),
// x = relu(Wq1 g + bq1), models.py:529, 549-556) is the bilinear form y^T (M x + v) + u^T x + c with M = Wr2^T Wq2, v = Wr2^T bq2,
// u = Wq2^T br2, c = <br2, bq2> folded once per checkpoint (car_round2q_pack): ONE 128 x 128 layer per sample, as many matrix operations as
// the stored-query form needs for q2 alone, and nothing 128 wide is read.  Packed: M (chained over x, 64 KB) | Wr1g | Wq1 (8 KB each).
constexpr int kLdsWq1 = kLdsBias;                                   // Wq1 tiles behind Wr1g's
constexpr int kLdsBiasG = kLdsWq1 + kNT * 512;                      // br1 | v | bq1 | u | 2^-shift of Wr1g, M, Wq1 | c
constexpr int kBiasFloatsG = 4 * kD + 8;
constexpr int kScratchG = kD * kD;                                  // car_round2q_pack's scratch behind the bias table: M in fp32
constexpr size_t kLdsBytesG = (size_t)(kLdsBiasG + kBiasFloatsG) * sizeof(float);

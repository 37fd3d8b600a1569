/* car_encoder_train.h — training through the transformer stage of get_z's encoder: the recorded forward and the backward of the 12 pre-norm
 * blocks of car_encoder.h (csrc/car_vit.hip, csrc/car_vit_backward.hip).  Included by car_hip.h, inside its extern "C" block,
 * behind car_decoder.h; include that file, not this one.  cross_attention_renderer_amd/_lib.py mirrors these prototypes in
 * ENCODER_TRAIN_SIGNATURES (tests/test_vit_backward_reference.py compares them type by type).  The conventions are car_encoder.h's:
 * channel-last fp32 rows; a status entry returns CAR_OK, CAR_E_ARG (nothing launched) or CAR_E_LAUNCH with a message in car_last_error; a
 * size entry returns 0, with a message, for a refused shape; caller-owned workspaces; 16-byte alignment; strides multiples of 4.  Nothing
 * beyond a row's width or a scene's rows is read.  No kernel of this file uses a float atomic: two runs give bit-identical DATA gradients
 * and LayerNorm gradients.  The matrices' weight and bias gradients go through car_linear_wgrad as it stands and inherit its fp32 atomics:
 * their last bits depend on the order in which its workgroups arrive.
 *
 * car_mha_stats: car_mha (same kernels, same arguments, `out` bit-identical) which also writes, per (scene, head, query row), the running
 *   maximum m and sum l its online softmax ends with: stats [b heads][S][2], car_mha_stats_floats(b, S, heads) floats, 16-byte aligned.
 *   m + log l is the row's log-sum-exp of q . k_j / 8.
 * car_mha_backward: from qkv, stats, out (car_mha_stats' own) and dout [b S][ldd] to dqkv [b S][lddq] in qkv's column order, WRITTEN (the
 *   3 dim columns of every row; not accumulated).  Per (scene, head), s_ij = q_i . k_j / 8, p_ij = exp(s_ij - m_i) / l_i:
 *     D_i = sum_c dout_ic out_ic    dv_j = sum_i p_ij dout_i    dp_ij = dout_i . v_j    ds_ij = p_ij (dp_ij - D_i)
 *     dq_i = sum_j ds_ij k_j / 8    dk_j = sum_i ds_ij q_i / 8
 *   Arithmetic: all five products in the library's fp32-class split fp16 (fp16 hi / lo halves of both operands, three
 *   v_mfma_f32_32x32x16_f16 products per term, fp32 accumulation) on the chained 32 x 32 x 16 tile; D in fp32; exp is the accurate one.
 *   Two kernels, no atomics: in one a wave owns 32 query rows and streams the key tiles (car_mha's loop; the logits are formed from the
 *   same packed k tiles, the same split of q and the same powers of two as the forward's, so p there is the forward's weight) and gives
 *   dq; in the other a wave owns 32 keys and streams the query tiles and gives dk and dv (its logits are the transposed product: the
 *   forward's to rounding).  Powers of two, all undone exactly: q, k, v, dout one per (scene, head) as A operands — q as the logits' A
 *   operand one per row, the forward's — and one per row as B operands; p and ds one per row and tile, taken from the largest
 *   magnitude there.  The powers of dout reach down to magnitudes of 2^-87, those of p and ds to 2^-113: a gradient of 1e-8 per unit is
 *   not flushed, and a key that a dominant one leaves a weight of e^-80 gets its own dv and dk to fp32-class accuracy.  Keys and queries
 *   that pad the last tile are masked by INDEX.  A scene's result does not depend on the other scenes of the call.  Shapes and
 *   refusals as car_mha; dqkv must not overlap an input.  work: car_mha_backward_workspace_bytes(b, S, heads) bytes (7 operand
 *   forms per tile of 32 rows: 56 KB, against car_mha's 16).
 * car_layernorm_backward: dx = rstd (g dy - mean(g dy) - xhat mean(g dy xhat)), xhat = (x - mean) rstd, the statistics recomputed in fp64
 *   over the row's registers exactly as car_layernorm takes them (nothing is saved).  One wave per row.  flags: CAR_LIN_ACCUM adds dx
 *   into dX (the residual branch), 0 writes it.  dgamma[c] = sum_m dy xhat, dbeta[c] = sum_m dy (both or neither; null: not computed):
 *   slabs of 64 rows summed in row order into the workspace, then the slabs in slab order, in fp64 — WRITTEN, no atomics.  C a multiple
 *   of 4 in 4..4096; strides >= C and multiples of 4; dX may be dY.  work: car_layernorm_backward_workspace_bytes(M, C) bytes (needed
 *   with dgamma only).
 * car_gelu_backward: dY[m][n] *= Phi(u) + u phi(u), u = U[m][n] the saved pre-activation; Phi(u) = erfc(-u / sqrt 2) / 2 as the forward
 *   takes it (no cancellation in the lower tail), phi(u) = exp(-u^2 / 2) / sqrt(2 pi).  u = +-0 gives 1/2; a large u gives 1 exactly, a
 *   large negative u gives 0 (both terms underflow, no NaN); +-inf give NaN (inf times 0, as the formula does); a NaN stays a NaN.
 * car_vit_pack_train: car_vit_pack, followed in the same buffer by the four TRANSPOSED matrices of every block (the operands of
 *   dX = dY W through car_linear_x3).  packed: car_vit_packed_train_floats(dim, depth) floats; its first car_vit_packed_floats are
 *   car_vit_pack's own, bit for bit, at car_vit_packed_offset's offsets.  car_vit_packed_train_offset(dim, depth, item): item 0..3 the
 *   transposed qkv, proj, fc1, fc2 from a block's transposed record, item 4 that record's size, item 5 where the records start.
 * car_vit_blocks_train: car_vit_blocks (same sequence, tok and the taps bit-identical) which saves what the backward reads.  saved:
 *   car_vit_saved_bytes(b, S, dim, depth) bytes, 16-byte aligned; per block, in pieces of whole 64 floats: the block's input [rows][dim],
 *   qkv [rows][3 dim], the attention output [rows][dim], the stream after the attention half [rows][dim], the fc1 pre-activation
 *   [rows][4 dim], the statistics [b heads][S][2] — 10 dim floats a row: 189.5 MB per block at b = 12, S = 514, dim = 768.  The
 *   LayerNorm outputs and gelu(u) are recomputed by the backward.  work: car_vit_workspace_bytes.
 * car_vit_blocks_backward: the blocks in reverse.  dtok [b S][dim]: on entry the gradient of the stage's output tok, on return the
 *   gradient of its input.  dtaps: a HOST array of n_taps device pointers ([b S][dim], read only), the gradient of tap i, added to the
 *   stream where the tap was taken; a null entry is a zero gradient.  dparams: the parameter gradients in car_vit_pack's order and torch
 *   layout, one flat buffer the CALLER ZEROES: block i at i car_vit_grad_offset(dim, 12), item j at car_vit_grad_offset(dim, j).  The
 *   LayerNorm items are written; the matrices and their biases are added by car_linear_wgrad (flags: CAR_WGRAD_FP32 or 0, passed on).
 *   dtok is bit-identical to the same sequence issued through the stage entries.  packed: car_vit_pack_train's.
 *   work: car_vit_backward_workspace_bytes(b, S, dim) bytes.
 * Refusals (CAR_E_ARG, nothing launched): those of car_encoder.h's entries, a saved buffer that is too small, flags other than the ones
 *   named. */
#ifndef CAR_ENCODER_TRAIN_H
#define CAR_ENCODER_TRAIN_H

size_t car_mha_stats_floats(int b, int S, int heads);
int car_mha_stats(const float* qkv, int ld, int b, int S, int heads, float* out, int ldo, float* stats, void* work, size_t work_bytes,
                  void* stream);
size_t car_mha_backward_workspace_bytes(int b, int S, int heads);
int car_mha_backward(const float* qkv, int ld, const float* stats, const float* out, int ldo, const float* dout, int ldd, int b, int S,
                     int heads, float* dqkv, int lddq, void* work, size_t work_bytes, void* stream);
size_t car_layernorm_backward_workspace_bytes(long M, int C);
int car_layernorm_backward(const float* X, int ldx, const float* gamma, int C, double eps, const float* dY, int lddy, float* dX, int lddx,
                           long M, int flags, float* dgamma, float* dbeta, void* work, size_t work_bytes, void* stream);
int car_gelu_backward(const float* U, int ldu, float* dY, int lddy, long M, int N, void* stream);
size_t car_vit_packed_train_floats(int dim, int depth);
size_t car_vit_packed_train_offset(int dim, int depth, int item);
int car_vit_pack_train(const float* const* params, int n_params, int dim, int depth, float* packed, void* stream);
size_t car_vit_saved_bytes(int b, int S, int dim, int depth);
int car_vit_blocks_train(float* tok, int b, int S, int dim, const float* packed, int depth, const int* taps, int n_taps,
                         float* const* tap_out, void* saved, size_t saved_bytes, void* work, size_t work_bytes, void* stream);
size_t car_vit_grad_offset(int dim, int item);
size_t car_vit_backward_workspace_bytes(int b, int S, int dim);
int car_vit_blocks_backward(float* dtok, int b, int S, int dim, const float* packed, int depth, const int* taps, int n_taps,
                            const float* const* dtaps, const void* saved, size_t saved_bytes, float* dparams, int flags, void* work,
                            size_t work_bytes, void* stream);

#endif /* CAR_ENCODER_TRAIN_H */

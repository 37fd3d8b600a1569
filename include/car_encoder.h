/* car_encoder.h — the image encoder's part of the C ABI of libcar_hip.so: the transformer stage of get_z's multi-view DPT encoder
 * (csrc/car_vit.hip).  Included by car_hip.h, inside its extern "C" block and after its codes and conventions (CAR_OK,
 * CAR_E_ARG, CAR_E_LAUNCH, car_last_error, `void* stream`, flags of car_linear); include that file, not this one.
 * cross_attention_renderer_amd/_lib.py mirrors these prototypes in ENCODER_SIGNATURES (tests/test_vit_reference.py compares them type by
 * type).
 *
 * What is here: the 12 pre-norm blocks over the concatenated tokens of a scene's views (encoder.py MultiViewDPTEncoder.forward; reference
 * midas/vit.py:183-202, vit_models.py:10-97 with timm 0.5.4's Block / Attention / Mlp).  What stands in front of them — the ResNetV2 trunk
 * and the token assembly (projection, class token, position and pose embeddings) — is on the device too, in car_trunk.h, which car_hip.h
 * includes behind this file.  What stands behind them — the read-out and re-assembly, the RefineNet fusion, conv_map and the image
 * normalisation — is on the device as well, in car_decoder.h, behind car_trunk.h; its car_getz is the whole of get_z in one call, so a host
 * without PyTorch has a route from two images to z (the relative pose and the checkpoint stay its own).  The entries of this file are forwards;
 * the recorded forward of the blocks and their backward (LayerNorm, GELU, attention, the stage) are in car_encoder_train.h, behind car_decoder.h.
 *
 * Everything is channel-last fp32 rows.  Every status entry returns CAR_OK, CAR_E_ARG (nothing launched) or CAR_E_LAUNCH with a message in
 * car_last_error; a size entry returns 0, with a message, for a refused shape.
 *
 * car_layernorm: Y[m][c] = (X[m][c] - mean_m) rsqrt(var_m + eps) gamma[c] + beta[c], var the BIASED variance over the row's C channels.
 *   One wave per row; the row is read once into registers, mean and variance are taken in fp64 over them (two passes: the mean first, then
 *   the squared distances from it), so a row of 1e4 + noise does not cancel and a constant row gives beta exactly.  C a multiple of 4 in
 *   4..4096; ldx, ldy >= C and multiples of 4; X, Y, gamma, beta 16-byte aligned; Y may be X.  Columns beyond C are never read or written.
 * car_gelu: Y[m][n] = x Phi(x), the exact GELU x (1 + erf(x / sqrt 2)) / 2 evaluated as x erfc(-x / sqrt 2) / 2 (no cancellation in the
 *   lower tail), in place.  +-0 stay +-0, +inf stays +inf, a NaN stays a NaN, -inf gives NaN (-inf times 0, as the formula does).
 *   N and ldy multiples of 4, ldy >= N, Y 16-byte aligned.
 * car_mha: multi-head self-attention with head width 64 over b scenes of S rows.  qkv [b S][ld] in timm's column order: with dim = 64 heads,
 *   q of head h at column 64 h, k at dim + 64 h, v at 2 dim + 64 h.  out [b S][ldo]: column 64 h + c = sum_j softmax_j(q . k_j / 8) v_j[c],
 *   the keys j being the S rows of the query's own scene.  S in 1..1024, heads in 1..16, b in 1..4096; ld >= 3 dim, ldo >= dim, both
 *   multiples of 4; qkv, out, work 16-byte aligned; out must not overlap qkv.
 *   Arithmetic: the library's fp32-class split fp16 for BOTH products — fp16 hi / lo halves of q, k, the softmax numerators and v, three
 *   v_mfma_f32_32x32x16_f16 products per term (hi hi, hi lo, lo hi), fp32 accumulation.  k and v carry one power of two per (scene, head),
 *   a query row one of its own, the numerators 2^13; all are undone exactly.  The softmax is fp32 with the running maximum subtracted
 *   (online softmax over tiles of 32 keys: K and V of one head do not fit LDS at S = 771 and are streamed); exp is the accurate one.
 *   The keys that pad the last tile are given weight 0 by their INDEX, never by a value: nothing beyond a scene's rows or beyond the 3 dim
 *   columns of a row is read, so NaN there can not reach a sum.  Fixed order of every reduction, no atomics: two runs are bit-identical, and a
 *   scene's result does not depend on the other scenes of the call.
 *   work: car_mha_workspace_bytes(b, S, heads) bytes, caller-owned (the k / v operand tiles of the whole call and their scales).
 * car_vit_pack: params = a HOST array of device arrays in torch layout, 12 per block in this order: norm1.weight, norm1.bias,
 *   attn.qkv.weight [3 dim][dim], attn.qkv.bias, attn.proj.weight [dim][dim], attn.proj.bias, norm2.weight, norm2.bias, mlp.fc1.weight
 *   [4 dim][dim], mlp.fc1.bias, mlp.fc2.weight [dim][4 dim], mlp.fc2.bias; n_params = 12 depth.  The four matrices are laid out by
 *   car_linear_x3_pack, the eight vectors are copied.  dim a multiple of 64 in 64..1024 (heads = dim / 64), the hidden width is 4 dim,
 *   depth in 1..32.  packed: car_vit_packed_floats(dim, depth) floats, 16-byte aligned.  Per block, in floats from the block's start:
 *   car_vit_packed_offset(dim, i) for i = 0..11 in the order above (vectors and matrices alike), the block's size for i = 12.
 * car_vit_blocks: runs blocks 0 .. depth - 1 IN PLACE on tok [b S][dim] (contiguous rows, 16-byte aligned).  Per block:
 *   car_layernorm (eps 1e-6) -> car_linear_x3 (qkv) -> car_mha -> car_linear_x3 (proj, CAR_LIN_ACCUM into tok) -> car_layernorm ->
 *   car_linear_x3 (fc1) -> car_gelu -> car_linear_x3 (fc2, CAR_LIN_ACCUM into tok).  After block taps[i] tok is copied to tap_out[i]
 *   ([b S][dim]); taps: a HOST array of n_taps strictly increasing ints in 0 .. depth - 1, tap_out a HOST array of n_taps device pointers
 *   (n_taps may be 0, with both null).  The result is bit-identical to the same sequence issued through the stage entries.
 *   work: car_vit_workspace_bytes(b, S, dim) bytes, 16-byte aligned, caller-owned.
 * Refusals (CAR_E_ARG, nothing launched): a null pointer, S outside 1..1024, heads outside 1..16, dim not a multiple of 64 or above 1024,
 *   depth outside 1..32, a parameter count that does not fit the depth, taps not increasing or >= depth, a stride below the width or not a
 *   multiple of 4, a pointer not 16-byte aligned, a workspace that is too small. */
#ifndef CAR_ENCODER_H
#define CAR_ENCODER_H

int car_layernorm(const float* X, int ldx, const float* gamma, const float* beta, int C, double eps, float* Y, int ldy, long M, void* stream);
int car_gelu(float* Y, int ldy, long M, int N, void* stream);
size_t car_mha_workspace_bytes(int b, int S, int heads);
int car_mha(const float* qkv, int ld, int b, int S, int heads, float* out, int ldo, void* work, size_t work_bytes, void* stream);
size_t car_vit_packed_floats(int dim, int depth);
size_t car_vit_packed_offset(int dim, int item);
int car_vit_pack(const float* const* params, int n_params, int dim, int depth, float* packed, void* stream);
size_t car_vit_workspace_bytes(int b, int S, int dim);
int car_vit_blocks(float* tok, int b, int S, int dim, const float* packed, int depth, const int* taps, int n_taps, float* const* tap_out,
                   void* work, size_t work_bytes, void* stream);

#endif /* CAR_ENCODER_H */

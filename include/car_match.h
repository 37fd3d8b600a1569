/* car_match.h — the matcher's part of the C ABI of libcar_hip.so: SuperPoint (csrc/car_superpoint.hip) and SuperGlue
 * (csrc/car_superglue.hip).  Included by car_hip.h, inside its extern "C" block and after its codes and conventions (CAR_OK, CAR_E_ARG,
 * CAR_E_LAUNCH, car_last_error, `void* stream`, flags of car_linear); include that file, not this one.
 * cross_attention_renderer_amd/_lib.py mirrors these prototypes in MATCH_SIGNATURES (tests/test_matcher_reference.py compares them type
 * by type). */
#ifndef CAR_MATCH_H
#define CAR_MATCH_H

/* ---- keypoints of an unposed pair: SuperPoint's forward (estimate_pose/superpoint.py:47-202; csrc/car_superpoint.hip).
 * The weights are the caller's: the twelve convolutions in the reference's declaration order (conv1a 1b 2a 2b 3a 3b 4a 4b Pa Pb Da Db),
 * torch layout [N][K][kh][kw] and biases [N], device arrays named by HOST arrays of pointers.  car_superpoint_pack lays them out once
 * (car_superpoint_packed_floats floats, 16-byte aligned): conv1a as fp32 [tap][64] with its bias, the nine 3 x 3 layers of 64 / 128 / 256
 * channels by car_conv3x3_pack, convPb (256 -> 65) and convDb (256 -> 256) by car_linear_pack.  Everything is channel-last: a descriptor
 * set is [N, 256] where the reference holds [256, N].
 * car_superpoint_dense: gray [n, H, W] fp32 in [0, 1], H and W multiples of 8 and >= 8, n H W <= 2^22.  scores [n, H, W]: the softmax
 *   over a cell's 65 channels (maximum subtracted, fp32), the dustbin dropped, channel c at pixel (c / 8, c % 8) of the cell (:163-166),
 *   BEFORE the non-maximum suppression.  desc [n, H / 8, W / 8, 256], 16-byte aligned: x / max(|x|, 1e-12) per cell (F.normalize).  The
 *   3 x 3 layers and pools are car_conv3x3 / car_maxpool2x2 calls, the two 1 x 1 heads car_linear calls.  work:
 *   car_superpoint_workspace_bytes bytes, 16-byte aligned, caller-owned (0, with a message, for a refused shape).
 * car_superpoint_conv1a: the first layer alone, Y [n, H, W, 64] = relu(conv3x3(gray) + bias), zero padding, any H, W >= 1; `packed` is
 *   car_superpoint_pack's array.
 * car_superpoint_nms: simple_nms (:47-62) on n maps [H, W]: the (2 radius + 1)^2 maximum with -inf padding and the two
 *   suppress-and-recover passes, radius 0..8.  Only comparisons of fp32 values: bit-identical to the reference's function on the same
 *   finite map, plateaus and exact ties included.  out != scores.  work: car_superpoint_nms_workspace_bytes bytes.
 * car_superpoint_select (:170-187): keeps the pixels with score > threshold that lie at least `border` from every edge (border <= y <
 *   H - border, likewise x); when more than max_keypoints (1..4096) survive, the max_keypoints largest.  Per map i: kpts [i][k] = (x, y)
 *   as fp32 and scores [i][k] for k < count [i], the arrays being [n][max_keypoints][2] and [n][max_keypoints]; entries >= count [i] are
 *   not written.  Order: row-major when nothing is cut, descending score when the top-k cuts (the reference's two orders).  Equal scores:
 *   the lower row-major index is kept first and comes first — torch.topk leaves that case open, this is the library's choice (-0 and +0
 *   are one score).  The result depends on the inputs alone, never on the schedule: prefix sums and integer counters, no float atomics.
 *   The reference's max_keypoints = -1 ("all") is refused.  work: car_superpoint_select_workspace_bytes bytes.
 * car_superpoint_sample (sample_descriptors, :80-92): kpts [N][2] (x, y) of ONE image, N in 1..4096, desc [h, w, 256] its dense
 *   descriptors; coordinates (k - 4 + 0.5) / (8 w - 4 - 0.5) mapped to [-1, 1], bilinear with align_corners = True and zero padding,
 *   then x / max(|x|, 1e-12).  out [N, 256].  desc and out 16-byte aligned.
 * Refusals (CAR_E_ARG, nothing launched): a null pointer, H or W no multiple of 8 (dense), a map above 2^22 pixels, a radius outside
 *   0..8, max_keypoints outside 1..4096, a NaN threshold, a workspace that is too small. */
size_t car_superpoint_packed_floats(void);
int car_superpoint_pack(const float* const* conv_w, const float* const* conv_b, float* packed, void* stream);
size_t car_superpoint_workspace_bytes(int n, int H, int W);
int car_superpoint_dense(const float* gray, int n, int H, int W, const float* packed, float* scores, float* desc, void* work,
                         size_t work_bytes, void* stream);
int car_superpoint_conv1a(const float* gray, int n, int H, int W, const float* packed, float* Y, void* stream);
size_t car_superpoint_nms_workspace_bytes(int n, int H, int W);
int car_superpoint_nms(const float* scores, int n, int H, int W, int radius, float* out, void* work, size_t work_bytes, void* stream);
size_t car_superpoint_select_workspace_bytes(int n, int H, int W);
int car_superpoint_select(const float* nms, int n, int H, int W, float threshold, int border, int max_keypoints, float* kpts, float* scores,
                          int* count, void* work, size_t work_bytes, void* stream);
int car_superpoint_sample(const float* kpts, int N, const float* desc, int h, int w, float* out, void* stream);

/* ---- matches of an unposed pair: SuperGlue's forward (estimate_pose/superglue.py:51-285; csrc/car_superglue.hip).
 * Keypoints [N][2] (x, y), scores [N], descriptors [N][256] per image, as car_superpoint_select / car_superpoint_sample leave them; at most
 * 1024 keypoints per image.  An empty set is the host's business (all -1 and zeros, nothing launched; :235-242): every entry refuses N < 1.
 * car_superglue_pack: params = a HOST array of device arrays in torch layout, in this order: the keypoint encoder's five convolutions
 *   (weight, bias), each of the first four followed by its BatchNorm1d (weight, bias, running_mean, running_var) — 26 arrays; per GNN layer
 *   attn.proj.0 / 1 / 2, attn.merge, mlp.0 (weight, bias each), mlp.1 (weight, bias, running_mean, running_var), mlp.3 (weight, bias) — 16
 *   arrays; final_proj (weight, bias).  n_params = 26 + 16 layers + 2, layers in 1..64 (the published network has 18, `self` and `cross`
 *   alternating; the pattern is an argument of car_superglue_descriptors).  Every eval-mode BatchNorm is folded into the convolution in front
 *   of it at pack time, in fp64, rounded once: s = weight / sqrt(running_var + 1e-5), W' = s W, b' = (b - running_mean) s + bias.
 *   HEAD PERMUTATION: MultiHeadedAttention splits its 256 channels by view(b, 64, 4, n), so head h owns the torch channels h, h + 4, h + 8,
 *   ..., not a contiguous block.  The rows of the three projections and the columns of merge are permuted at pack time — device channel
 *   h * 64 + d is torch channel d * 4 + h — so that a head is 64 contiguous floats on the device; the three projections are packed as one
 *   256 -> 768 layer (q | k | v).  packed: car_superglue_packed_floats(layers) floats, 16-byte aligned (the packer's scratch behind the layers).
 * car_superglue_descriptors: normalize_keypoints with the centre (W / 2, H / 2) and the scale 0.7 max(W, H) of each image; the keypoint
 *   encoder [x, y, score] -> 32 -> 64 -> 128 -> 256 -> 256 added to the descriptors; per layer l the projections, the attention of each image's
 *   rows against its own (cross[l] = 0) or the other image's (cross[l] != 0; `cross` is a HOST array of `layers` ints), merge, the
 *   512 -> 512 -> 256 MLP on [x | message] (a column offset into one [rows, 512] buffer, not a copy) and the residual add; final_proj.
 *   mdesc [N0 + N1][256]: image 0's rows, then image 1's.  All layers are car_linear calls over the rows of both images.
 * car_superglue_attention: out [N][ldo] = softmax(q k^T / 8) v for 4 heads of 64 contiguous channels, q [N][ldq], k, v [M][ldk], [M][ldv],
 *   N and M in 1..1024, strides >= 256 (ldk a multiple of 4, k 16-byte aligned).  The maximum is subtracted; fp32 accumulation in a fixed order.
 * car_superglue_transport: Z [(N0 + 1)][(N1 + 1)] = log_optimal_transport (:143-172) of mdesc0 mdesc1^T / 16 with bin_score on the dustbin
 *   row and column; `iters` (0..1000) alternating u / v updates, one launch per half-iteration, the log-sum-exp sums in fp64 in a fixed
 *   order; Z = couplings + u + v - norm, norm = -log(N0 + N1).  No launch waits for another workgroup.
 * car_superglue_matches (:267-285): the row and column arg-max over Z[:-1, :-1] (ties to the lowest index), the mutual check, score =
 *   exp(max) where mutual, else 0; matches0 [N0], matches1 [N1] int32 with -1 for no match (not mutual, or score <= match_threshold),
 *   scores0 [N0], scores1 [N1].
 * Workspaces are caller-owned, 16-byte aligned; a size entry returns 0, with a message, for a refused shape.  Refusals (CAR_E_ARG, nothing
 * launched): a null pointer, fewer than 1 or more than 1024 keypoints, layers outside 1..64, a parameter count that does not fit the layers,
 * a workspace that is too small, a NaN threshold or bin_score. */
size_t car_superglue_packed_floats(int layers);
int car_superglue_pack(const float* const* params, int n_params, int layers, float* packed, void* stream);
size_t car_superglue_workspace_bytes(int N0, int N1);
int car_superglue_descriptors(const float* kpts0, const float* scores0, const float* desc0, int N0, int H0, int W0, const float* kpts1,
                              const float* scores1, const float* desc1, int N1, int H1, int W1, const float* packed, int layers,
                              const int* cross, float* mdesc, void* work, size_t work_bytes, void* stream);
int car_superglue_attention(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, int N, int M, float* out, int ldo,
                            void* stream);
size_t car_superglue_transport_workspace_bytes(int N0, int N1);
int car_superglue_transport(const float* mdesc0, int N0, const float* mdesc1, int N1, float bin_score, int iters, float* Z, void* work,
                            size_t work_bytes, void* stream);
size_t car_superglue_matches_workspace_bytes(int N0, int N1);
int car_superglue_matches(const float* Z, int N0, int N1, float match_threshold, int* matches0, int* matches1, float* scores0, float* scores1,
                          void* work, size_t work_bytes, void* stream);

#endif /* CAR_MATCH_H */

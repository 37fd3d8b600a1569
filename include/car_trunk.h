/* car_trunk.h — the image encoder's front half in the C ABI of libcar_hip.so: the weight-standardised ResNetV2 trunk of get_z's multi-view
 * DPT encoder and the assembly of the token rows its transformer stage reads (csrc/car_trunk.hip).  Included by car_hip.h,
 * inside its extern "C" block and after its codes and conventions (CAR_OK, CAR_E_ARG, CAR_E_LAUNCH, car_last_error, `void* stream`) and
 * after car_encoder.h; include that file, not this one.  cross_attention_renderer_amd/_lib.py mirrors these prototypes in TRUNK_SIGNATURES
 * (tests/test_trunk_reference.py compares them type by type).
 *
 * What is here: everything in front of car_vit_blocks (encoder.py ResNetV2Trunk — timm 0.5.4's resnetv2 Bottleneck, StdConv2dSame,
 * GroupNormAct, MaxPool2dSame as restated there — and the token lines of MultiViewDPTEncoder.forward: the 1x1 projection, the class token,
 * the resized position embedding, the pose embedding).  With car_encoder.h the path from an image to the tapped states of the blocks is one
 * run of C-ABI calls.  What is NOT here — the read-out and re-assembly, the RefineNet fusion, conv_map and the image normalisation — is in
 * car_decoder.h, which car_hip.h includes behind this file and whose car_getz strings the whole of get_z together.  Inference only: no
 * entry here has a backward.
 *
 * Activations are channel-last fp32 rows [n][H W][C].  Every status entry returns CAR_OK, CAR_E_ARG (nothing launched) or CAR_E_LAUNCH with
 * a message in car_last_error; a size entry returns 0, with a message, for a refused shape.  Every reduction has a fixed order and uses no
 * float atomics: two runs are bit-identical, and an image's result does not depend on the other images of the call.  Every pointer is
 * 16-byte aligned.  TF "SAME" padding of a window k at stride s over an extent i: ceil(i / s) outputs, total padding
 * max((ceil(i / s) - 1) s + k - i, 0), the odd pixel behind (bottom / right).
 *
 * car_weight_standardize: out[c][j] = (w[c][j] - mean_c) / sqrt(var_c + eps) over the fan_in values of output channel c (N channels), var the
 *   BIASED variance.  Mean, squared distances from it and the division in fp64, rounded to fp32 once; a constant filter gives exact zeros.
 *   eps: 1e-6 for the stem, 1e-8 for the stages (encoder.py).  The output, still in torch layout, feeds car_linear_x3_pack (1x1 layers) and
 *   car_conv3x3_same_pack.
 * car_stem7x7: x [n][3][H][W] (NCHW, the image as get_z normalises it), w_std [64][3][7][7], Y [n][ceil(H/2)][ceil(W/2)][64]; stride 2, SAME
 *   padding with zeros.  fp32 on the vector pipe, one fmaf per term in the order (channel, window row, window column); a tap in the padding
 *   adds nothing.
 * car_groupnorm: Y = act(gn(X) gamma + beta (+ add)); X, Y, add [n][HW][C], add NULL or a residual that is summed after the affine step and
 *   before the ReLU (flags: CAR_GN_RELU or 0).  Statistics per (image, group) over HW C / groups values in fp64, two passes (the mean, then
 *   the squared distances from it): a group of 1e4 + noise comes out with the rounding of the result, a constant group gives beta exactly.
 *   Each pass is split over slabs of 8192 / C pixels whose partial sums every reader adds in the same fixed order.  C a power of two in 8..1024,
 *   groups divides C, C / groups 2 or a multiple of 4; n in 1..65535.  Y may be X.  work: car_groupnorm_workspace_bytes(n, HW, C, groups)
 *   bytes, caller-owned (the slabs' partial sums).
 * car_maxpool3x3s2_same: Y [n][ceil(H/2)][ceil(W/2)][C] = the maximum over the 3x3 window's taps inside the image (SAME padding with -inf);
 *   a NaN in the window gives NaN.  C a multiple of 4 in 4..4096.
 * car_conv3x3_same: Y [n][Ho][Wo][N] = the 3x3 convolution of X [n][H][W][K] at stride 1 or 2 with SAME padding (zeros); no bias, no
 *   activation.  At stride 2 an even extent pads 0 in front and 1 behind, an odd one 1 and 1.  K and N among 64, 128, 256.  An implicit GEMM
 *   over 9 K on the f16 matrix pipe in the library's split-fp16 arithmetic (car_linear_x3's: fp16 hi / lo halves of both operands, three
 *   products per term, fp32 accumulation, one power of two per layer and one per output pixel, undone exactly).  packed:
 *   car_conv3x3_same_packed_floats(K, N) floats written by car_conv3x3_same_pack from w_std [N][K][3][3]: 9 K / 32 x N / 16 tiles of 512
 *   floats, [K step][tile][hi | lo][lane][8 halves] with k = tap K + channel (car_conv3x3's tiles), then 64 floats of scale.
 * car_pixels_stride2: Y [n][ceil(H/2)][ceil(W/2)][C] = X at the even coordinates: the stride-2 1x1 convolution of a projecting shortcut
 *   (whose SAME padding is zero) is this copy followed by car_linear_x3.  C a multiple of 4 in 4..4096.
 * car_trunk_pack: depths = a HOST array of three ints in 1..16 (the product's: 3, 4, 9); widths are fixed at 64 -> 256 / 512 / 1024 with
 *   mid = out / 4, 32 groups.  params = a HOST array of device arrays in torch layout, in state_dict order of ResNetV2Trunk: stem.conv.weight,
 *   stem.norm.weight, stem.norm.bias, then per block (downsample.conv.weight, downsample.norm.weight, downsample.norm.bias in a stage's
 *   first block,) conv1.weight, norm1.weight, norm1.bias, conv2 .., conv3 ..; n_params = 3 + sum over stages of (9 depth + 3).  Every
 *   convolution weight is standardised and laid out for its consumer, the GroupNorm vectors are copied.  packed:
 *   car_trunk_packed_floats(depths) floats (the packer's scratch included).
 * car_trunk_forward: x [n][3][H][W] -> layer1 [n][H/4 W/4][256], layer2 [n][H/8 W/8][512], feat [n][H/16 W/16][1024] (the three stage ends;
 *   with SAME padding every halving is a ceiling).  Nothing but this sequence of exported entries, to which its result is bit-identical:
 *   car_stem7x7 -> car_groupnorm (ReLU) -> car_maxpool3x3s2_same; per block: (first of a stage: [car_pixels_stride2 at stride 2 ->]
 *   car_linear_x3 -> car_groupnorm = the shortcut;) car_linear_x3 (conv1) -> car_groupnorm (ReLU) -> car_conv3x3_same (the stage's stride in its
 *   first block) -> car_groupnorm (ReLU) -> car_linear_x3 (conv3) -> car_groupnorm (add = shortcut, ReLU).  GroupNorm eps 1e-5, bias NULL in
 *   every linear.  work: car_trunk_workspace_bytes(n, H, W, depths) bytes, caller-owned.
 * car_vit_tokens_pack: proj_w [768][1024], proj_b [768], cls [768], pos_embed [1 + grid grid][768], pose_w [768][16], pose_b [768].  The
 *   position embedding is resized here, once: entry 0 kept, the grid entries bilinear from grid x grid to gh x gw with align_corners = False
 *   (fp64, rounded once).  gh, gw in 1..64.  packed: car_vit_tokens_packed_floats(gh, gw) floats.
 * car_vit_tokens: feat [BV][gh gw][1024], pose16 [BV][16] -> tok [BV][1 + gh gw][768], the rows car_vit_blocks reads.  Per view v:
 *   row 0 = (cls + pos[0]) + pose_embed(pose16[v]); row 1 + p = ((proj(feat[v][p]) + bias) + pos[1 + p]) + pose_embed(pose16[v]); the sums
 *   in fp32 in this order.  The projection is car_linear_x3 with its bias; pose_embed is the 16 terms and the bias in fp64, rounded once.
 *   work: car_vit_tokens_workspace_bytes(BV, gh, gw) bytes, caller-owned.  BV in 1..4096.
 * Refusals (CAR_E_ARG, nothing launched): a null pointer, a pointer not 16-byte aligned, a width outside the sets above, groups that do not
 *   divide C, C / groups neither 2 nor a multiple of 4, n, H or W below 1 or beyond the caps (2^27 pixels in all), a stride other than 1 or
 *   2, a depth outside 1..16, a parameter count that does not fit the depths, a workspace that is too small. */
#ifndef CAR_TRUNK_H
#define CAR_TRUNK_H

#define CAR_GN_RELU 1            /* car_groupnorm's flags: ReLU behind the affine step and the residual */

int car_weight_standardize(const float* w, int N, int fan_in, double eps, float* out, void* stream);
int car_stem7x7(const float* x, int n, int H, int W, const float* w_std, float* Y, void* stream);
size_t car_groupnorm_workspace_bytes(int n, int HW, int C, int groups);
int car_groupnorm(const float* X, int n, int HW, int C, int groups, const float* gamma, const float* beta, double eps, const float* add,
                  int flags, float* Y, void* work, size_t work_bytes, void* stream);
int car_maxpool3x3s2_same(const float* X, int n, int H, int W, int C, float* Y, void* stream);
size_t car_conv3x3_same_packed_floats(int K, int N);
int car_conv3x3_same_pack(const float* w_std, int K, int N, float* packed, void* stream);
int car_conv3x3_same(const float* X, int n, int H, int W, int K, int N, int stride, const float* packed, float* Y, void* stream);
int car_pixels_stride2(const float* X, int n, int H, int W, int C, float* Y, void* stream);
size_t car_trunk_packed_floats(const int* depths);
int car_trunk_pack(const float* const* params, int n_params, const int* depths, float* packed, void* stream);
size_t car_trunk_workspace_bytes(int n, int H, int W, const int* depths);
int car_trunk_forward(const float* x, int n, int H, int W, const float* packed, const int* depths, float* layer1, float* layer2, float* feat,
                      void* work, size_t work_bytes, void* stream);
size_t car_vit_tokens_packed_floats(int gh, int gw);
int car_vit_tokens_pack(const float* proj_w, const float* proj_b, const float* cls, const float* pos_embed, int grid, const float* pose_w,
                        const float* pose_b, int gh, int gw, float* packed, void* stream);
size_t car_vit_tokens_workspace_bytes(int BV, int gh, int gw);
int car_vit_tokens(const float* feat, int BV, int gh, int gw, const float* pose16, const float* packed, float* tok, void* work,
                   size_t work_bytes, void* stream);

#endif /* CAR_TRUNK_H */

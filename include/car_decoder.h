/* car_decoder.h — the image encoder's back half in the C ABI of libcar_hip.so, and get_z as one call: the read-out and re-assembly of the
 * two tapped block states, the RefineNet fusion, conv_map and the image normalisation (csrc/car_decoder.hip).  Included by
 * car_hip.h, inside its extern "C" block and after its codes and conventions (CAR_OK, CAR_E_ARG, CAR_E_LAUNCH, car_last_error, `void* stream`,
 * the CAR_LIN_* flags) and after car_trunk.h; include that file, not this one.  cross_attention_renderer_amd/_lib.py mirrors these
 * prototypes in DECODER_SIGNATURES (tests/test_decoder_reference.py compares them type by type).  16 entries.
 *
 * What is here: the last 45 lines of encoder.py MultiViewDPTEncoder.forward (ProjectReadout, the 1x1 and strided 3x3 layers of
 * act_postprocess3 / 4, scratch.layerN_rn, the four FeatureFusionBlocks) and the normalisation and conv_map lines of
 * models.CrossAttentionRenderer.get_z.  With car_trunk.h and car_encoder.h the path from two images in [-1, 1] and their relative poses to
 * the feature pyramid z is one run of C-ABI calls, and car_getz is that run.  What stays the caller's: the 4x4 inverse and product of the
 * relative pose, and reading a checkpoint.  Inference only: no entry here has a backward.
 *
 * Activations are channel-last fp32 rows [n][H W][C]; z comes out channel-last, the layout the render engine takes as a view.  Every status
 * entry returns CAR_OK, CAR_E_ARG (nothing launched) or CAR_E_LAUNCH with a message in car_last_error; a size entry returns 0, with a
 * message, for a refused shape.  Every reduction has a fixed order and uses no float atomics: two runs are bit-identical, and an image's
 * result does not depend on the other images of the call.  Every pointer is 16-byte aligned.
 *
 * car_conv3x3_pad1: Y [n][Ho][Wo][N] = act_out((conv3x3(act_in(X [n][H][W][K])) + bias) + add) (+ Y), stride 1 or 2, torch's symmetric zero
 *   padding of 1: Ho = (H - 1) / stride + 1 by integer division.  bias: N floats or NULL; add: NULL or a [n][Ho][Wo][N] residual.  flags:
 *   CAR_LIN_RELU_IN (the input through a ReLU on load; the padding stays zeros), CAR_LIN_RELU_OUT (a NaN stays a NaN), CAR_LIN_ACCUM (+ Y,
 *   behind the output ReLU), applied in the order of the formula.  K among 256, 512, 768; N among 256, 768.  An implicit GEMM over 9 K on the
 *   f16 matrix pipe in the library's split-fp16 arithmetic (car_linear_x3's: fp16 hi / lo halves of both operands, three products per term,
 *   fp32 accumulation, one power of two per layer and one per output pixel, undone exactly); bias, residual, ReLU and accumulation in fp32
 *   on the finished sum.  add must not be Y; X must not be Y.  packed: car_conv3x3_pad1_packed_floats(K, N) floats written by
 *   car_conv3x3_pad1_pack from w [N][K][3][3]: car_conv3x3_same_pack's layout — 9 K / 32 x N / 16 tiles of 512 floats, [K step][tile]
 *   [hi | lo][lane][8 halves] with k = tap K + channel, then 64 floats of scale.
 * car_upsample2x_bilinear: Y [n][2H][2W][C] from X [n][H][W][C], align_corners = True: output o of an extent E reads source coordinate
 *   o (E - 1) / (2 E - 1), taken exactly in integers: i0 = o (E - 1) div (2 E - 1), i1 = min(i0 + 1, E - 1), the fraction l =
 *   (o (E - 1) mod (2 E - 1)) / (2 E - 1) rounded to fp32 once.  In fp32: top = fma(lx, v01 - v00, v00), bot = fma(lx, v11 - v10, v10),
 *   out = fma(ly, bot - top, top).  A constant image comes back exactly, the corners are the input's corners bit for bit; a border row or
 *   column and an extent of 1 read nothing outside the image.  C a multiple of 4 in 4..4096, H and W at most 16384.
 * car_readout: ProjectReadout without the concatenation.  tok [BV][1 + P][dim] (row 0 the class token), Y [BV][P][dim].  With W = [Wa | Wb]
 *   of the Linear(2 dim, dim) (Wa the columns of the patch token): r[v] = Wb tok[v][0] + b (car_linear_x3 over the class rows, ldx =
 *   (1 + P) dim, with the bias), prod = Wa tok over every row (car_linear_x3, no bias; the class row's product is not used), Y[v][p] =
 *   gelu(prod[v][1 + p] + r[v]): one fp32 sum of the two, then car_gelu's formula x erfc(-x / sqrt 2) / 2.  Half the MACs of the literal
 *   form and no 2 dim wide staging buffer.  dim a multiple of 32 in 64..1024, P in 1..4096, BV in 1..4096.  packed:
 *   car_readout_packed_floats(dim) floats written by car_readout_pack from w [dim][2 dim] and bias [dim] (Wa's and Wb's car_linear_x3_pack
 *   arrays, then the bias).  work: car_readout_workspace_bytes(BV, P, dim) bytes, caller-owned.
 * car_conv7x7_pad3: conv_map.  x [n][3][H][W] (NCHW, the normalised image, as car_stem7x7 reads it), w [64][3][7][7], bias [64] ->
 *   Y [n][H][W][64]; stride 1, zero padding 3.  fp32 on the vector pipe: the accumulator STARTS at the bias, then one fmaf per term in
 *   car_stem7x7's order (channel, window row, window column); a tap in the padding adds nothing.
 * car_normalize_rgb: rgb [n][H][W][3] in [-1, 1] -> x [n][3][H][W] = ((v + 1) / 2 - mean_c) / std_c in fp32, get_z's operations in its order
 *   with its constants (0.485, 0.456, 0.406; 0.229, 0.224, 0.225) rounded to fp32, nothing contracted: the bits of those lines of
 *   models.get_z run by torch on the CPU.
 * car_decoder_pack: params = a HOST array of the 50 device arrays the decoder evaluates, in torch layout and in state_dict order of
 *   MultiViewDPTEncoder: pretrained.act_postprocess3 .0.project.0.weight [768][1536], .bias, .3.weight [768][768][1][1], .bias;
 *   pretrained.act_postprocess4 the same four, then .4.weight [768][768][3][3], .bias; scratch.layer{1,2,3,4}_rn.weight [256][256 / 512 /
 *   768 / 768][3][3]; then per scratch.refinenet{1,2,3,4}: out_conv.weight [256][256][1][1], .bias, resConfUnit1.conv1.weight
 *   [256][256][3][3], .bias, resConfUnit1.conv2 .., resConfUnit2.conv1 .., resConfUnit2.conv2 .. — WITHOUT refinenet4.resConfUnit1 (four
 *   arrays) and scratch.output_conv, which are in the checkpoint and never evaluated.  packed: car_decoder_packed_floats() floats.
 * car_decoder_forward: tap3, tap4 [BV][1 + gh gw][768] (the states behind blocks 8 and 11, as car_vit_blocks hands them out), layer1
 *   [BV][4gh 4gw][256], layer2 [BV][2gh 2gw][512] (as car_trunk_forward writes them) -> path_2 [BV][4gh 4gw][256], path_1 [BV][8gh 8gw][256].
 *   gh, gw even in 2..64 (the halved map of tap 4 is doubled back onto the grid).  Nothing but this sequence of exported entries, to which
 *   its result is bit-identical:
 *     layer_3 = car_linear_x3 (act_postprocess3[3], bias) of car_readout(tap3);
 *     layer_4 = car_conv3x3_pad1 (act_postprocess4[4], stride 2, bias) of car_linear_x3 (act_postprocess4[3], bias) of car_readout(tap4);
 *     then for level N = 4, 3, 2, 1 at h x w = gh / 2 x gw / 2, doubling: car_conv3x3_pad1 (layerN_rn, no bias) of layer_N -> the path
 *     (N = 4) or the skip; (N < 4, resConfUnit1 and the sum:) mid = car_conv3x3_pad1 (conv1, bias, RELU_IN) of the skip, path =
 *     car_conv3x3_pad1 (conv2, bias, add = skip, RELU_IN | ACCUM into the path) of mid; (resConfUnit2:) mid = car_conv3x3_pad1 (conv1, bias,
 *     RELU_IN) of the path, u = car_conv3x3_pad1 (conv2, bias, add = path, RELU_IN) of mid; car_upsample2x_bilinear of u; the next path =
 *     car_linear_x3 (out_conv, bias) of the upsampled map — AFTER the upsampling, as encoder.py has it.  The result of level 2 is path_2
 *     (copied into the next level's path, which the sum overwrites), that of level 1 path_1.
 *   work: car_decoder_workspace_bytes(BV, gh, gw) bytes, caller-owned.
 * car_getz: the whole of get_z.  rgb [BV][H][W][3] in [-1, 1], pose16 [BV][16] (the relative poses, the caller's to compute; no_multiview is
 *   a zero pose16) -> z0 = path_2 [BV][4gh 4gw][256], z1 = path_1 [BV][8gh 8gw][256], z2 = conv_map [BV][H W][64] (zeros when no_high_freq
 *   is not 0).  trunk_packed, tokens_packed (for gh x gw), vit_packed (dim 768, vit_depth blocks), decoder_packed: the arrays of
 *   car_trunk_pack, car_vit_tokens_pack, car_vit_pack, car_decoder_pack; map_w [64][3][7][7], map_b [64]: conv_map's.  depths: a HOST
 *   array of the trunk's three depths; taps: a HOST array of the two tapped blocks, increasing, below vit_depth (the product: 8, 11 of 12).
 *   Nothing but car_normalize_rgb -> car_trunk_forward -> car_vit_tokens -> car_vit_blocks (b = BV / nviews scenes of S = nviews (1 + gh gw)
 *   rows) -> car_decoder_forward -> car_conv7x7_pad3 (or the memset) over one workspace, bit-identical to that sequence.
 *   work: car_getz_workspace_bytes(BV, H, W, gh, gw, nviews, depths, vit_depth) bytes, caller-owned.
 * Refusals (CAR_E_ARG, nothing launched): a null pointer, a pointer not 16-byte aligned, a width outside the sets above, a stride other than
 *   1 or 2, unknown flags, n, H, W, BV, P, gh or gw below 1 or beyond the caps (4096 images, 2^27 pixels in the largest map of a call, a grid
 *   of 64 x 64), an odd gh or gw in the decoder, a parameter count other than 50, BV not a multiple of nviews, nviews (1 + gh gw) beyond
 *   car_mha's 1024 rows, an image whose halvings (ceil(H / 4), ceil(H / 8), ceil(H / 16)) are not (4 gh, 2 gh, gh), and the same for W,
 *   taps that do not increase inside the blocks, a workspace that is too small. */
#ifndef CAR_DECODER_H
#define CAR_DECODER_H

size_t car_conv3x3_pad1_packed_floats(int K, int N);
int car_conv3x3_pad1_pack(const float* w, int K, int N, float* packed, void* stream);
int car_conv3x3_pad1(const float* X, int n, int H, int W, int K, int N, int stride, const float* packed, const float* bias, const float* add,
                     int flags, float* Y, void* stream);
int car_upsample2x_bilinear(const float* X, int n, int H, int W, int C, float* Y, void* stream);
size_t car_readout_packed_floats(int dim);
int car_readout_pack(const float* w, const float* bias, int dim, float* packed, void* stream);
size_t car_readout_workspace_bytes(int BV, int P, int dim);
int car_readout(const float* tok, int BV, int P, int dim, const float* packed, float* Y, void* work, size_t work_bytes, void* stream);
int car_conv7x7_pad3(const float* x, int n, int H, int W, const float* w, const float* bias, float* Y, void* stream);
int car_normalize_rgb(const float* rgb, int n, int H, int W, float* x, void* stream);
size_t car_decoder_packed_floats(void);
int car_decoder_pack(const float* const* params, int n_params, float* packed, void* stream);
size_t car_decoder_workspace_bytes(int BV, int gh, int gw);
int car_decoder_forward(const float* tap3, const float* tap4, const float* layer1, const float* layer2, int BV, int gh, int gw,
                        const float* packed, float* path_2, float* path_1, void* work, size_t work_bytes, void* stream);
size_t car_getz_workspace_bytes(int BV, int H, int W, int gh, int gw, int nviews, const int* depths, int vit_depth);
int car_getz(const float* rgb, const float* pose16, int BV, int H, int W, int gh, int gw, int nviews, const int* depths, const float* trunk_packed,
             const float* tokens_packed, const float* vit_packed, int vit_depth, const int* taps, const float* decoder_packed, const float* map_w,
             const float* map_b, int no_high_freq, float* z0, float* z1, float* z2, void* work, size_t work_bytes, void* stream);

#endif /* CAR_DECODER_H */

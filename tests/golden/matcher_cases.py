"""The seeded inputs of the matcher fixture (tests/golden/matcher_expected.npz): the weight recipe, the image pairs and the crafted
score maps.  Shared by the generator (make_matcher_golden.py) and by the tests, which rebuild the weights from the seed — only inputs
and results are stored, never weights."""
import numpy as np
import torch

# the reference's declaration order (estimate_pose/superpoint.py:119-134): name, input channels, output channels, kernel size
SUPERPOINT_CONVS = (("conv1a", 1, 64, 3), ("conv1b", 64, 64, 3), ("conv2a", 64, 64, 3), ("conv2b", 64, 64, 3), ("conv3a", 64, 128, 3),
                    ("conv3b", 128, 128, 3), ("conv4a", 128, 128, 3), ("conv4b", 128, 128, 3), ("convPa", 128, 256, 3), ("convPb", 256, 65, 1),
                    ("convDa", 128, 256, 3), ("convDb", 256, 256, 1))
WEIGHT_SEED = 11


def superpoint_state(seed: int = WEIGHT_SEED):
    """He-scaled convolution weights (std = sqrt(2 / fan_in)) and biases of std 0.1, float32, drawn in declaration order."""
    g = torch.Generator().manual_seed(seed)
    state = {}
    for name, k, n, ks in SUPERPOINT_CONVS:
        state[f"{name}.weight"] = torch.randn(n, k, ks, ks, generator=g) * (2.0 / (k * ks * ks)) ** 0.5
        state[f"{name}.bias"] = torch.randn(n, generator=g) * 0.1
    return state


# name -> (H, W, shift of the second image (dy, dx), nms_radius, keypoint_threshold, max_keypoints, remove_borders)
PAIRS = {
    "rowmajor": (48, 64, (2, 3), 4, 0.005, 1024, 4),      # max_keypoints above the count: nothing is cut, row-major order
    "topk": (40, 56, (1, 2), 4, 0.005, 24, 4),            # the top-k cuts: descending score
    "unequal": (56, 64, (3, 5), 3, 0.05, 1024, 4),       # a threshold inside the scores' range: the two sides keep different counts
}
IMAGE_SEED = 3


def pair_images(name: str):
    """Two float32 grey images in [0, 1]: windows of one seed-3 noise field, the second shifted by a few pixels."""
    H, W, (dy, dx) = PAIRS[name][:3]
    rng = np.random.default_rng([IMAGE_SEED, sorted(PAIRS).index(name)])
    field = rng.random((H + 16, W + 16)).astype(np.float32)
    return np.stack([field[8:8 + H, 8:8 + W], field[8 + dy:8 + dy + H, 8 + dx:8 + dx + W]])


def crafted_maps():
    """Score maps [H, W] float32 for the decision stages: plateaus, exact ties, everything under the threshold, everything inside the
    border, and a noise map whose values are all distinct."""
    rng = np.random.default_rng(5)
    H, W = 24, 40
    maps = {}
    noise = rng.permutation(H * W).astype(np.float32).reshape(H, W) / (H * W)          # distinct values
    maps["distinct"] = noise
    plateau = np.zeros((H, W), np.float32)
    plateau[3:9, 4:12] = 0.5                                                            # a flat block larger than the window of radius 1
    plateau[15, 20:30] = 0.25                                                           # a flat line
    plateau[20, 35] = 0.75
    maps["plateau"] = plateau
    maps["ties"] = (rng.integers(0, 4, (H, W)) / 4.0).astype(np.float32)               # four levels: ties everywhere
    maps["constant"] = np.full((H, W), 0.125, np.float32)
    maps["low"] = (noise * 0.004).astype(np.float32)                                    # everything under the default threshold 0.005
    edge = np.zeros((H, W), np.float32)
    edge[0, :] = noise[0, :] + 0.1
    edge[:, 0] = noise[:, 0] + 0.1
    edge[H - 1, 7] = 0.9
    edge[2, W - 2] = 0.8
    maps["border"] = edge                                                               # every maximum lies inside a border of 4
    maps["one"] = rng.random((1, 1)).astype(np.float32)
    maps["row"] = rng.random((1, 19)).astype(np.float32)
    return maps


NMS_RADII = (0, 1, 4, 8)
# selections on the crafted maps that the reference decides (no equal scores at a cut): map, radius, threshold, border, max_keypoints
SELECTIONS = (("distinct", 0, 0.5, 0, 4096), ("distinct", 0, 0.5, 3, 100), ("distinct", 2, 0.005, 4, 1024), ("distinct", 2, 0.005, 4, 7),
              ("low", 4, 0.005, 4, 1024), ("border", 4, 0.005, 4, 1024), ("plateau", 1, 0.005, 0, 1024), ("distinct", 4, 0.005, 12, 1024),
              ("one", 0, 0.005, 0, 5), ("row", 1, 0.005, 0, 3))

GNN_LAYERS = ("self", "cross", "self", "cross")       # the fixtures' network; the published one has nine such pairs
SINKHORN_ITERATIONS, MATCH_THRESHOLD, BIN_SCORE = 20, 0.2, 2.37
GLUE_SEED = 401
MDESC_PROBE = 16                                      # rows of mdesc the fixture keeps per image
FINAL_SCALE = 0.17                                   # on final_proj: keeps mdesc0 mdesc1^T / 16 in the range where the dustbin (2.37) competes


def superglue_state(layers: int = len(GNN_LAYERS), seed: int = GLUE_SEED):
    """He-scaled 1 x 1 convolutions (std = sqrt(2 / fan_in), biases of std 0.1), BatchNorm with non-trivial running statistics and affine
    pairs, final_proj scaled by FINAL_SCALE, bin_score = 2.37; the reference module's parameter names, in its state dict's order."""
    g = torch.Generator().manual_seed(seed)
    state = {}

    def conv(name, k, n):
        state[name + ".weight"] = torch.randn(n, k, 1, generator=g) * (2.0 / k) ** 0.5
        state[name + ".bias"] = torch.randn(n, generator=g) * 0.1

    def bn(name, n):
        state[name + ".weight"] = 0.5 + torch.rand(n, generator=g)
        state[name + ".bias"] = torch.randn(n, generator=g) * 0.1
        state[name + ".running_mean"] = torch.randn(n, generator=g) * 0.2
        state[name + ".running_var"] = 0.5 + torch.rand(n, generator=g)
        state[name + ".num_batches_tracked"] = torch.tensor(0)
    widths = (3, 32, 64, 128, 256, 256)
    for i, idx in enumerate((0, 3, 6, 9, 12)):
        conv(f"kenc.encoder.{idx}", widths[i], widths[i + 1])
        if i < 4:
            bn(f"kenc.encoder.{idx + 1}", widths[i + 1])
    for l in range(layers):
        pre = f"gnn.layers.{l}"
        conv(f"{pre}.attn.merge", 256, 256)
        for j in range(3):
            conv(f"{pre}.attn.proj.{j}", 256, 256)
        conv(f"{pre}.mlp.0", 512, 512)
        bn(f"{pre}.mlp.1", 512)
        conv(f"{pre}.mlp.3", 512, 256)
    conv("final_proj", 256, 256)
    state["final_proj.weight"], state["final_proj.bias"] = state["final_proj.weight"] * FINAL_SCALE, state["final_proj.bias"] * FINAL_SCALE
    state["bin_score"] = torch.tensor(BIN_SCORE)
    return state

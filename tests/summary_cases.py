"""The seeded inputs of the summary fixture (tests/golden/summary_expected.npz): regenerated here by the generator and by the tests, never
stored.  Image values are multiples of 1/32 so that the fixture compresses; the probe ray's samples are set by hand so that some
project outside [-1, 1] and the arg-max sample sits near a border."""
import os

import numpy as np
import torch

PROBE = 2065
SAMPLES = 16
# name -> (B, n_view, H, W).  48 x 48: pix = 1 and ray 2065 is row 43, column 1 (the left-edge clip); 64 x 64: pix = 2 and, with one
# scene and one view, make_grid's single-image form for every panel but the epipolar one
CASES = {"b2v2_48": (2, 2, 48, 48), "b1v1_64": (1, 1, 64, 64)}
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "summary_expected.npz")


def _grid(H, W):
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    return torch.stack([xs, ys], dim=-1).reshape(H * W, 2)


def build(name):
    """(model_input, model_output) of a case as CPU tensors, in the shapes the renderer returns them."""
    B, V, H, W = CASES[name]
    g = torch.Generator().manual_seed(sorted(CASES).index(name) + 20)
    R, S, n = H * W, SAMPLES, B * V

    def image(*shape, span=32):
        return torch.randint(-span, span + 1, shape, generator=g).float() / 32

    rgb = image(B, 1, R, 3, span=48)                                  # beyond [-1, 1]: the clamp matters
    depth = torch.rand(B, R, 1, generator=g) * 12 - 1                 # below 0 and above 10 included
    depth[0, :6, 0] = torch.tensor([0.0, 10.0, -0.5, 25.0, float("nan"), 9.999999])
    at_wt = torch.softmax(2 * torch.randn(n, R, S, generator=g), dim=-1)   # may differ in the last ulp between hosts: the entropy's bound covers it
    pixel_val = torch.rand(n, R, S, 2, generator=g) * 2.6 - 1.3       # some samples outside [-1, 1]
    best = torch.randint(0, S, (n, R, 1), generator=g)
    for row in range(n):                                              # the probe ray: a line across the tile that leaves it on both sides
        t = (torch.arange(S, dtype=torch.float32) * 52 - 400) / 320     # -1.25 ... 1.1875, formed from exact integers
        pixel_val[row, PROBE, :, 0] = t
        pixel_val[row, PROBE, :, 1] = 0.35 * t + 0.1 * row - 0.2
        best[row, PROBE, 0] = (1, S - 2, 2, 8)[row % 4]               # first / last sample inside the tile sit on a border
    pixel_val[0, PROBE, 5] = torch.tensor([0.999, -0.999])            # top-right corner: the square is cut on two sides
    model_output = {"rgb": rgb, "depth_ray": depth, "at_wt": at_wt, "pixel_val": pixel_val, "at_wt_max": best,
                    "uv": _grid(H, W)[None, None].expand(B, 1, R, 2).contiguous()}
    model_input = {"context": {"rgb": image(B, V, H, W, 3)}, "query": {"rgb": image(B, 1, R, 3)}}
    return model_input, model_output


def checksum(model_input, model_output) -> np.ndarray:
    ts = [model_input["context"]["rgb"], model_input["query"]["rgb"]] + [model_output[k] for k in sorted(model_output)]
    return np.array([torch.nan_to_num(t.double()).sum().item() for t in ts])


def load(name):
    """(model_input, model_output, the case's fixture arrays), after checking that the regenerated inputs are the fixture's."""
    fx = np.load(FIXTURE)
    model_input, model_output = build(name)
    np.testing.assert_allclose(checksum(model_input, model_output), fx[f"{name}.checksum"], rtol=1e-6, err_msg="summary input RNG drift")
    return model_input, model_output, {k[len(name) + 1:]: fx[k] for k in fx.files if k.startswith(name + ".")}

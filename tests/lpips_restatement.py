"""Float64 torch restatement of LPIPS v0.1 with net = 'vgg', the checker of ``car_lpips`` (tests/test_lpips.py).

Written from the metric's specification, not from the package (which does not exist offline) and not from the code under test:
  1. scaling layer, per channel: (v - shift) / scale, shift = (-0.030, -0.088, -0.188), scale = (0.458, 0.448, 0.450), on images in [-1, 1];
  2. VGG16 ``features``: 3x3 convolutions, stride 1, zero padding 1, bias, ReLU behind each; 2x2 / stride 2 max-pool (floor) in front of
     blocks 2-5; widths 64 64 | 128 128 | 256 256 256 | 512 512 512 | 512 512 512; taps relu1_2 relu2_2 relu3_3 relu4_3 relu5_3;
  3. per tap and pixel: n0 = sqrt(sum_c f0_c^2), n1 likewise, d_c = (f0_c / (n0 + 1e-10) - f1_c / (n1 + 1e-10))^2, s = sum_c w[c] d_c with
     the 1x1 layer's weights w (no bias); the tap's term is the mean of s over its pixels;
  4. LPIPS = the sum of the five terms.
Its pin against the ``lpips`` package itself is tests/golden/make_lpips_golden.py --lpips, run where the package exists.  torch only."""
import math

import torch
import torch.nn.functional as F

SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)
WIDTHS = (64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512)
FEATURES = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)          # torchvision vgg16().features indices of the convolutions
SLICE = (1, 1, 2, 2, 3, 3, 3, 4, 4, 4, 5, 5, 5)                       # the package's net.slice{n} holding each convolution
POOL_BEFORE = (2, 4, 7, 10)                                           # a max-pool sits in front of these layers
TAP_AFTER = (1, 3, 6, 9, 12)
TAP_WIDTHS = (64, 128, 256, 512, 512)


def scale_image(x, dtype=torch.float64):
    """[B, H, W, 3] in [-1, 1], channel-last -> the scaled image, [B, 3, H, W]."""
    x = x.to(dtype).permute(0, 3, 1, 2)
    return (x - torch.tensor(SHIFT, dtype=dtype).view(1, 3, 1, 1)) / torch.tensor(SCALE, dtype=dtype).view(1, 3, 1, 1)


def layers(x, conv_w, conv_b, dtype=torch.float64):
    """Every ReLU output of the network, [B, C, h, w] each, for images x [B, H, W, 3] in [-1, 1]."""
    h, outs = scale_image(x, dtype), []
    for l in range(13):
        if l in POOL_BEFORE:
            h = F.max_pool2d(h, 2, 2)
        h = F.relu(F.conv2d(h, conv_w[l].to(dtype), conv_b[l].to(dtype), stride=1, padding=1))
        outs.append(h)
    return outs


def taps(x, conv_w, conv_b, dtype=torch.float64):
    outs = layers(x, conv_w, conv_b, dtype)
    return [outs[l] for l in TAP_AFTER]


def head(f0, f1, lin, dtype=torch.float64):
    """Step 3 and 4 for lists of five [B, C, h, w] maps: (total [B], per tap [B, 5])."""
    terms = []
    for a, b, w in zip(f0, f1, lin):
        a, b, w = a.to(dtype), b.to(dtype), w.to(dtype).view(1, -1, 1, 1)
        n0 = a.pow(2).sum(1, keepdim=True).sqrt()
        n1 = b.pow(2).sum(1, keepdim=True).sqrt()
        d = (a / (n0 + 1e-10) - b / (n1 + 1e-10)).pow(2)
        terms.append((w * d).sum(1).mean(dim=(1, 2)))
    per_tap = torch.stack(terms, 1)
    return per_tap.sum(1), per_tap


def lpips(x, y, conv_w, conv_b, lin, dtype=torch.float64):
    """x, y [B, H, W, 3] in [-1, 1] -> (LPIPS [B], per tap [B, 5]) computed in `dtype`."""
    return head(taps(x, conv_w, conv_b, dtype), taps(y, conv_w, conv_b, dtype), lin, dtype)


# ---- the tests' inputs --------------------------------------------------------------------------------------------------------------

def seeded_weights(seed=0):
    """Convolutions He-normal (std = sqrt(2 / (9 K))), biases 0.01 x normal, lin weights |normal| / C_k; float32."""
    g = torch.Generator().manual_seed(seed)
    conv_w, conv_b, k = [], [], 3
    for n in WIDTHS:
        conv_w.append((torch.randn(n, k, 3, 3, generator=g, dtype=torch.float64) * math.sqrt(2.0 / (9 * k))).float())
        conv_b.append((0.01 * torch.randn(n, generator=g, dtype=torch.float64)).float())
        k = n
    lin = [(torch.randn(c, generator=g, dtype=torch.float64).abs() / c).float() for c in TAP_WIDTHS]
    return conv_w, conv_b, lin


def make_image(seed, b, h, w):
    """A smooth field plus noise in [0, 1], [b, h, w, 3] float32."""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, h, dtype=torch.float64), torch.linspace(0, 1, w, dtype=torch.float64), indexing="ij")
    ph = 6.0 * torch.rand(b, 1, 1, 3, generator=g, dtype=torch.float64)
    fx, fy = (1.0 + 4.0 * torch.rand(b, 1, 1, 3, generator=g, dtype=torch.float64) for _ in range(2))
    smooth = 0.5 + 0.3 * torch.sin(fx * xx[None, ..., None] * 3 + fy * yy[None, ..., None] * 2 + ph)
    return (smooth + 0.1 * torch.randn(b, h, w, 3, generator=g, dtype=torch.float64)).clamp(0, 1).float()


def state_dicts(conv_w, conv_b, lin, layout):
    """The weights written as the two file layouts: 'split' -> (torchvision state dict, lin state dict), 'single' -> (package state dict, None)."""
    if layout == "split":
        vgg = {}
        for i, w, b in zip(FEATURES, conv_w, conv_b):
            vgg[f"features.{i}.weight"], vgg[f"features.{i}.bias"] = w.clone(), b.clone()
        return vgg, {f"lin{k}.model.1.weight": w.clone().view(1, -1, 1, 1) for k, w in enumerate(lin)}
    sd = {"scaling_layer.shift": torch.tensor(SHIFT).view(1, 3, 1, 1), "scaling_layer.scale": torch.tensor(SCALE).view(1, 3, 1, 1)}
    for i, s, w, b in zip(FEATURES, SLICE, conv_w, conv_b):
        sd[f"net.slice{s}.{i}.weight"], sd[f"net.slice{s}.{i}.bias"] = w.clone(), b.clone()
    for k, w in enumerate(lin):
        sd[f"lin{k}.model.1.weight"] = w.clone().view(1, -1, 1, 1)
        sd[f"lins.{k}.model.1.weight"] = w.clone().view(1, -1, 1, 1)
    return sd, None

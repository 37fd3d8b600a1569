"""Closes the one pin the LPIPS tests cannot close offline: tests/lpips_restatement.py against the ``lpips`` package itself.

    python tests/golden/make_lpips_golden.py --lpips

Runs on a machine that ALREADY has ``lpips`` and ``torchvision`` installed.  It downloads nothing and installs nothing: when a package is
missing it says so and stops, and it builds ``lpips.LPIPS(net='vgg', pnet_rand=True)`` — the package's own network code and its own
linear layers (shipped inside the package), with a randomly initialised VGG16 trunk, so that torchvision never looks for pretrained weights.
What is pinned is the DEFINITION (scaling layer, taps, normalisation, linear layers, means and sum), which does not depend on the trunk's
values.  It reads the network's state dict through ``harness.lpips_arrays`` (the loader the scripts use), evaluates the package and the
float64 restatement on one seeded pair of 256 x 256 images and on a noisy copy, and prints both values and their relative difference; more
than 1e-5 (the package computes in float32) is an error.  It is never run by the tests."""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    if "--lpips" not in sys.argv:
        sys.exit(__doc__)
    try:
        import lpips
        import torchvision  # noqa: F401
    except ImportError as e:
        sys.exit(f"make_lpips_golden.py --lpips: {e.name} is not installed here; run this on a machine that has lpips and torchvision")
    import lpips_restatement as LR
    from cross_attention_renderer_amd import harness
    try:
        torch.manual_seed(0)
        net = lpips.LPIPS(net="vgg", pretrained=True, pnet_rand=True, verbose=False).eval()      # pretrained: the package's own lin layers
    except Exception as e:
        sys.exit(f"make_lpips_golden.py --lpips: lpips.LPIPS(net='vgg', pnet_rand=True) could not be built: {e}")
    state = {k: v.detach().clone() for k, v in net.state_dict().items()}
    conv_w, conv_b, lin = harness.lpips_arrays(state)
    worst = 0.0
    for name, noise in (("unrelated", None), ("noisy copy", 0.05)):
        x = LR.make_image(1, 1, 256, 256)
        y = LR.make_image(2, 1, 256, 256) if noise is None else (x + noise * torch.randn(x.shape, generator=torch.Generator().manual_seed(3)))
        x11, y11 = (x - 0.5) * 2, (y - 0.5) * 2
        with torch.no_grad():
            theirs = net(x11.permute(0, 3, 1, 2), y11.permute(0, 3, 1, 2)).item()
        mine = LR.lpips(x11, y11, conv_w, conv_b, lin)[0].item()
        rel = abs(mine - theirs) / abs(theirs)
        worst = max(worst, rel)
        print(f"{name}: lpips package {theirs:.8f}, restatement {mine:.8f}, relative difference {rel:.2e}")
    if worst > 1e-5:
        sys.exit(f"the restatement and the lpips package differ by {worst:.2e} (> 1e-5): the pin is NOT closed")
    print("the restatement agrees with the lpips package: pin closed")


if __name__ == "__main__":
    main()

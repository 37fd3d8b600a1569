"""Float64 vector-Jacobian product of the LPIPS restatement (tests/lpips_restatement.py), written out layer by layer, the checker of
``car_lpips_backward`` (tests/test_lpips_backward.py).

It takes the LINEARISATION POINT as an argument: the 13 activation maps.  Every ReLU mask and every pool choice is read from those maps
and nothing is recomputed, so the device's gradient can be held against the exact float64 gradient of the network linearised where the
device itself stood.  With the restatement's own float64 maps it is ``torch.autograd`` of ``LR.lpips`` (a CPU test); against plain
autograd a ReLU or pool decision that flips between arithmetics would otherwise move whole entries and have to be budgeted.
  1. head, per tap and pixel, u = f0 / (n0 + 1e-10), v = f1 / (n1 + 1e-10), q_c = 2 w_c (u_c - v_c):
       ds/df0_c =  q_c / (n0 + 1e-10) - (sum_j q_j f0_j) f0_c / (n0 (n0 + 1e-10)^2),
       ds/df1_c = -q_c / (n1 + 1e-10) + (sum_j q_j f1_j) f1_c / (n1 (n1 + 1e-10)^2),  times cotangent / npix; the norm term is 0 at n = 0;
  2. ReLU: times (activation > 0);
  3. convolution: ``conv_transpose2d`` with the same weights, stride 1, padding 1;
  4. max-pool: the gradient goes to the first maximal element of the window in row-major order (torch's rule);
  5. scaling layer: divide by scale.
torch only."""
import torch
import torch.nn.functional as F

import lpips_restatement as LR


def head_backward(f0, f1, w, g):
    """One tap: f0, f1 [B, C, h, w], w [C], g [B] -> (d sum_b g_b s_b / d f0, / d f1), float64."""
    f0, f1, w, g = f0.double(), f1.double(), w.double().view(1, -1, 1, 1), g.double().view(-1, 1, 1, 1)
    r0, r1 = f0.pow(2).sum(1, keepdim=True).sqrt(), f1.pow(2).sum(1, keepdim=True).sqrt()
    n0, n1 = r0 + 1e-10, r1 + 1e-10
    q = 2 * w * (f0 / n0 - f1 / n1)
    c0 = torch.where(r0 > 0, (q * f0).sum(1, keepdim=True) / (r0 * n0 * n0), torch.zeros_like(r0))
    c1 = torch.where(r1 > 0, (q * f1).sum(1, keepdim=True) / (r1 * n1 * n1), torch.zeros_like(r1))
    cot = g / (f0.shape[2] * f0.shape[3])
    return (q / n0 - c0 * f0) * cot, (c1 * f1 - q / n1) * cot


def pool_choice(act):
    """Index 0..3 (row-major in the window) of the first maximal element of every 2x2 window of act [n, C, H, W] -> [n, C, H/2, W/2]."""
    n, c, h, w = act.shape
    ho, wo = h // 2, w // 2
    win = act[:, :, :2 * ho, :2 * wo].reshape(n, c, ho, 2, wo, 2).permute(0, 1, 2, 4, 3, 5).reshape(n, c, ho, wo, 4)
    best = win.max(-1, keepdim=True).values
    return (win == best).to(torch.uint8).argmax(-1)                    # argmax returns the first of equal values


def pool_backward(t, act):
    """Routes t [n, C, H/2, W/2] to the chosen element of each window of act [n, C, H, W]; a last odd row or column gets 0."""
    n, c, h, w = act.shape
    ho, wo = h // 2, w // 2
    onehot = F.one_hot(pool_choice(act).long(), 4).to(t.dtype) * t[..., None]
    out = torch.zeros(n, c, h, w, dtype=t.dtype)
    out[:, :, :2 * ho, :2 * wo] = onehot.reshape(n, c, ho, wo, 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(n, c, 2 * ho, 2 * wo)
    return out


def vjp(acts, conv_w, lin, g):
    """acts: the 13 maps [2 B, C, h, w] (x's B images, then y's); g [B].  Returns (gx, gy), [B, H, W, 3] float64 each: the gradient of
    sum_b g_b LPIPS_b with respect to the two [-1, 1] channel-last images, for the network linearised at `acts`."""
    acts = [a.double() for a in acts]
    b = acts[0].shape[0] // 2
    hg = {}
    for k, l in enumerate(LR.TAP_AFTER):
        hg[l] = torch.cat(head_backward(acts[l][:b], acts[l][b:], lin[k], g))
    grad = hg[12] * (acts[12] > 0)
    for l in range(12, 0, -1):
        t = F.conv_transpose2d(grad, conv_w[l].double(), stride=1, padding=1)
        if l in LR.POOL_BEFORE:
            t = pool_backward(t, acts[l - 1])
        if l - 1 in hg:
            t = t + hg[l - 1]
        grad = t * (acts[l - 1] > 0)
    gimg = F.conv_transpose2d(grad, conv_w[0].double(), stride=1, padding=1) / torch.tensor(LR.SCALE, dtype=torch.float64).view(1, 3, 1, 1)
    gimg = gimg.permute(0, 2, 3, 1).contiguous()
    return gimg[:b], gimg[b:]


def autograd(x, y, conv_w, conv_b, lin, g, dtype=torch.float64):
    """torch.autograd of the restatement run in `dtype`: (gx, gy) [B, H, W, 3], the plain gradient with its own ReLU and pool decisions."""
    x, y = x.to(dtype).clone().requires_grad_(True), y.to(dtype).clone().requires_grad_(True)
    total, _ = LR.lpips(x, y, conv_w, conv_b, lin, dtype)
    (total * g.to(dtype)).sum().backward()
    return x.grad, y.grad


def worst(got, want):
    """Largest deviation of got from want [B, ...] as a fraction of each image's largest entry of want (tests/golden/grad_cases.py's rule)."""
    got, want = got.double(), want.double()
    top = want.flatten(1).abs().max(1).values.clamp_min(1e-300)
    return ((got - want).flatten(1).abs().max(1).values / top).max().item()

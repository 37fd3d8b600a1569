"""numpy restatements of the four summary operations (csrc/car_summary.hip), written from the reference's lines and from the documented
behaviour of the packages it calls — the yardsticks of tests/test_summaries_cpu.py and tests/test_summaries_hip.py.

  entropy_mean   training.py:110-114 / summaries.py:24-26, in float64
  jet_table      matplotlib's lookup-table construction for "jet" (colors._create_lookup_table on _cm._jet_data), float64
  colormap       matplotlib's Colormap.__call__ on a float32 array, as summaries.py:35-38 calls it
  overlay        summaries.py:72-136, the paint loop itself (the kernel is its gather form)
  make_grid      torchvision.utils.make_grid(x, normalize=True, scale_each=...) with its defaults nrow=8, padding=2, pad_value=0.
                 torchvision is not installed where these tests run: this follows its documented behaviour and is not checked
                 against the package.
Images are channel-last (N, H, W, 3) float32 here, as the kernels take them; make_grid returns the planar (3, Hg, Wg) grid."""
import math

import numpy as np

PROBE = 2065                                       # summaries.py:96


def entropy_mean(at_wt, nan_rows_zero):
    w = np.asarray(at_wt, dtype=np.float64).reshape(-1, np.shape(at_wt)[-1])
    with np.errstate(invalid="ignore", divide="ignore"):
        ent = -(w * np.log(w + 1e-5)).sum(axis=-1)
    if nan_rows_zero:
        ent[np.isnan(ent)] = 0
    return float(ent.mean())


def entropy_tolerance(S):
    """Per mean, against the float64 value: each fp32 term carries a few ulp of relative error on w * log plus about 2^-24 absolute error
    on the log from rounding its argument; a row's weights sum to 1, so a row's error is at most about 3u H + 2u with H <= ln S; the
    factor 8 leaves 2x for logf's own error."""
    return 8 * 2.0 ** -24 * (math.log(S) + 1)


_JET = {"red": ((0.00, 0, 0), (0.35, 0, 0), (0.66, 1, 1), (0.89, 1, 1), (1.00, 0.5, 0.5)),
        "green": ((0.000, 0, 0), (0.125, 0, 0), (0.375, 1, 1), (0.640, 1, 1), (0.910, 0, 0), (1.000, 0, 0)),
        "blue": ((0.00, 0.5, 0.5), (0.11, 1, 1), (0.34, 1, 1), (0.65, 0, 0), (1.00, 0, 0))}


def jet_table(n=256):
    cols = []
    for name in ("red", "green", "blue"):
        seg = np.array(_JET[name], dtype=np.float64)
        x, y0, y1 = seg[:, 0] * (n - 1), seg[:, 1], seg[:, 2]
        xind = (n - 1) * np.linspace(0, 1, n)
        ind = np.searchsorted(x, xind)[1:-1]
        frac = (xind[1:-1] - x[ind - 1]) / (x[ind] - x[ind - 1])
        cols.append(np.clip(np.concatenate([[y1[0]], frac * (y0[ind] - y1[ind - 1]) + y1[ind - 1], [y0[-1]]]), 0.0, 1.0))
    return np.stack(cols, axis=-1)


def colormap(x, scale, lut):
    """x (..., ) float32 -> (..., 3) float32 through lut (256, 3)."""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        t = np.asarray(x, dtype=np.float32) / np.float32(scale)
        a = t * np.float32(256)
        a[a == 256] = 255
        under, over, bad = a < 0, a >= 256, np.isnan(a)
        idx = np.where(bad | under | over, 0, a).astype(np.int64)
    idx[under] = 0
    idx[over] = 255
    out = np.asarray(lut, dtype=np.float32)[idx]
    out[bad] = 0
    return out


def _square(img, y, x, pix, value):
    H, W = img.shape[:2]
    # an upper end below 0 (a centre far outside the image, which the reference never meets) is an empty range, not an index from the end
    img[max(y - pix, 0):max(min(y + pix, H - 1), 0), max(x - pix, 0):max(min(x + pix, W - 1), 0)] = value


def overlay(trgt, ctxt, pixel_val, at_wt_max, uv, n_view, probe=PROBE):
    """trgt (B, H, W, 3); ctxt (B * n_view, H, W, 3) scene-major; pixel_val (B * n_view, R, S, 2); at_wt_max (B * n_view, R[, 1]);
    uv (B, 1, R, 2) or (B, R, 2).  Returns the panel (B + B * n_view, H, W, 3): targets, then the context tiles view-major."""
    trgt, ctxt = np.array(trgt, dtype=np.float32), np.array(ctxt, dtype=np.float32)
    B, H, W, _ = trgt.shape
    pixel_val = np.asarray(pixel_val, dtype=np.float32)
    at_wt_max = np.asarray(at_wt_max).reshape(B * n_view, -1)
    uv = np.asarray(uv, dtype=np.float32).reshape(B, -1, 2)
    pix = H // 64 + 1
    for i in range(B):
        _square(trgt[i], int(uv[i, probe, 1]), int(uv[i, probe, 0]), pix, -1.0)
        for k in range(n_view):
            tile, row = ctxt[i * n_view + k], pixel_val[i * n_view + k, probe]
            centres = []
            for j in range(row.shape[0]):
                val = np.clip((row[j] + np.float32(1)) / np.float32(2), 0, 1)
                centres.append((int(val[1] * np.float32(H - 1)), int(val[0] * np.float32(W - 1))))
                _square(tile, *centres[-1], pix, 0.0)
            _square(tile, *centres[int(at_wt_max[i * n_view + k, probe])], pix, -1.0)
    ctxt = ctxt.reshape(B, n_view, H, W, 3).transpose(1, 0, 2, 3, 4).reshape(B * n_view, H, W, 3)
    return np.concatenate([trgt, ctxt], axis=0)


def grid_shape(N, H, W):
    if N == 1:
        return H, W
    xm = min(8, N)
    ym = -(-N // xm)
    return (H + 2) * ym + 2, (W + 2) * xm + 2


def make_grid(x, scale_each=False, clamp=None):
    x = np.array(x, dtype=np.float32)
    if clamp is not None:
        x = np.where(np.isnan(x), x, np.clip(x, np.float32(clamp[0]), np.float32(clamp[1])))
    N, H, W, _ = x.shape

    def norm(t):                                   # norm_ip with low = float(t.min()), high = float(t.max())
        low, high = float(t.min()), float(t.max())              # numpy's min / max give NaN when any value is NaN, as torch's do
        if math.isnan(low) or math.isnan(high):
            return np.full_like(t, np.nan)
        span = np.float32(max(high - low, 1e-5))
        return (np.clip(t, np.float32(low), np.float32(high)) - np.float32(low)) / span
    with np.errstate(invalid="ignore"):
        x = np.stack([norm(t) for t in x]) if scale_each else norm(x)
    x = x.transpose(0, 3, 1, 2)
    if N == 1:
        return x[0]
    xm = min(8, N)
    Hg, Wg = grid_shape(N, H, W)
    grid = np.zeros((3, Hg, Wg), dtype=np.float32)
    for k in range(N):
        r, c = (k // xm) * (H + 2) + 2, (k % xm) * (W + 2) + 2
        grid[:, r:r + H, c:c + W] = x[k]
    return grid

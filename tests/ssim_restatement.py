"""Float64 numpy restatement of the SSIM the reference's eval script reports, the checker of ``car_ssim`` (tests/test_ssim.py).

The reference (experiment_scripts/eval_realestate10k.py:192-194) calls scikit-image 0.18.3
``structural_similarity(rgb_np, target_np, win_size=11, multichannel=True, gaussian_weights=True)`` on float32 (H, W, 3) images.
scikit-image is not obtainable offline, so this module restates that call from its source, step by step; it is checked against
analytic cases and ``scipy.ndimage.gaussian_filter`` (tests/test_ssim.py), never against scikit-image itself.  numpy only.
"""
import numpy as np

SIGMA, TRUNCATE = 1.5, 3.5                 # skimage: sigma=1.5 default; gaussian_weights=True sets truncate = 3.5
RADIUS = int(TRUNCATE * SIGMA + 0.5)       # scipy.ndimage.gaussian_filter1d: lw = int(truncate * sd + 0.5) = 5
WIN = 2 * RADIUS + 1                       # skimage: win_size = 2 * r + 1 = 11 (the caller's win_size=11 agrees)
K1, K2 = 0.01, 0.03                        # skimage defaults


def gaussian_weights():
    """scipy.ndimage._gaussian_kernel1d(sigma, 0, radius): exp(-0.5 / sigma**2 * x**2) for x = -r..r, normalised to sum 1."""
    x = np.arange(-RADIUS, RADIUS + 1)
    phi = np.exp(-0.5 / (SIGMA * SIGMA) * x ** 2)
    return phi / phi.sum()


def filter_valid(img):
    """gaussian_filter(img, sigma=1.5, truncate=3.5) restricted to the pixels whose 11 x 11 window lies inside the image,
    (H-10, W-10): scipy filters axis 0 then axis 1 with the separable 1-D kernel.  Only these pixels reach the mean (crop below),
    so the 'reflect' padding of the full filter never matters."""
    w = gaussian_weights()
    img = np.asarray(img, dtype=np.float64)
    H, W = img.shape
    a0 = sum(w[k] * img[k:H - 2 * RADIUS + k, :] for k in range(WIN))
    return sum(w[k] * a0[:, k:W - 2 * RADIUS + k] for k in range(WIN))


def ssim_map(x, y, data_range=2.0):
    """Per-pixel S of one 2-D channel over the kept (H-10, W-10) pixels (skimage 0.18.3 _structural_similarity.py)."""
    x = np.asarray(x, dtype=np.float64)    # X.astype(np.float64), Y.astype(np.float64)
    y = np.asarray(y, dtype=np.float64)
    if x.shape != y.shape or min(x.shape) < WIN:
        raise ValueError("win_size exceeds image extent")
    NP = WIN ** 2
    cov_norm = NP / (NP - 1)               # use_sample_covariance=True
    ux, uy = filter_valid(x), filter_valid(y)
    uxx, uyy, uxy = filter_valid(x * x), filter_valid(y * y), filter_valid(x * y)
    vx = cov_norm * (uxx - ux * ux)
    vy = cov_norm * (uyy - uy * uy)
    vxy = cov_norm * (uxy - ux * uy)
    R = data_range                          # data_range=None: dtype_range[float32] = (-1, 1) -> 2.0
    C1, C2 = (K1 * R) ** 2, (K2 * R) ** 2
    A1, A2, B1, B2 = 2 * ux * uy + C1, 2 * vxy + C2, ux ** 2 + uy ** 2 + C1, vx + vy + C2
    return (A1 * A2) / (B1 * B2)


def ssim(x, y, data_range=2.0):
    """Mean SSIM of two (H, W) or (H, W, C) images: crop(S, 5).mean() per channel, then the mean over channels
    (multichannel=True)."""
    x = np.asarray(x)
    y = np.asarray(y)
    if x.ndim == 2:
        return float(ssim_map(x, y, data_range).mean())
    return float(np.mean([ssim_map(x[..., c], y[..., c], data_range).mean() for c in range(x.shape[-1])]))


def constant_pair(c1, c2, data_range=2.0):
    """Closed form for two constant images: the variances vanish, S = (2 c1 c2 + C1) / (c1**2 + c2**2 + C1)."""
    C1 = (K1 * data_range) ** 2
    return (2 * c1 * c2 + C1) / (c1 * c1 + c2 * c2 + C1)

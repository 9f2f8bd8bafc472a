"""Numpy restatement of the MS-SSIM definition the device kernels implement (Wang et al. 2003
with the choices of tf.image.ssim_multiscale), in float64 by default and in float32 on request:
sliding weighted sums, no scipy.  Also the seeded image kinds the MS-SSIM tests share."""
import numpy as np

C1, C2 = 6.5025, 58.5225
WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def window(dtype=np.float64):
    k = np.arange(11, dtype=np.float64)
    g = np.exp(-(k - 5.0) ** 2 / (2 * 1.5 ** 2))
    return (g / g.sum()).astype(dtype)


def _filt(x, g):
    """Separable 'valid' 11-tap filter of [h, w, 3] along w, then along h."""
    h, w, _ = x.shape
    t = sum(g[k] * x[:, k:k + w - 10] for k in range(11))
    return sum(g[k] * t[k:k + h - 10] for k in range(11))


def _pool(x):
    """2x2 mean, stride 2; an odd last row / column is paired with itself."""
    h, w, _ = x.shape
    ya, xa = np.arange(0, h, 2), np.arange(0, w, 2)
    yb, xb = np.minimum(ya + 1, h - 1), np.minimum(xa + 1, w - 1)
    return (x[ya][:, xa] + x[ya][:, xb] + x[yb][:, xa] + x[yb][:, xb]) * x.dtype.type(0.25)


def sums(a, b, dtype=np.float64):
    """[5, 3, 2]: per scale and channel the sum (float64) of cs and of l*cs (computed in dtype)."""
    x, y = np.asarray(a).astype(dtype), np.asarray(b).astype(dtype)
    g = window(dtype)
    c1, c2, two = dtype(C1), dtype(C2), dtype(2)
    out = np.zeros((5, 3, 2), np.float64)
    for j in range(5):
        mx, my = _filt(x, g), _filt(y, g)
        sxx, syy, sxy = _filt(x * x, g) - mx * mx, _filt(y * y, g) - my * my, _filt(x * y, g) - mx * my
        cs = (two * sxy + c2) / (sxx + syy + c2)
        l = (two * mx * my + c1) / (mx * mx + my * my + c1)
        out[j, :, 0] = cs.astype(np.float64).sum(axis=(0, 1))
        out[j, :, 1] = (l * cs).astype(np.float64).sum(axis=(0, 1))
        if j < 4:
            x, y = _pool(x), _pool(y)
    return out


def counts(H, W):
    n, h, w = [], H, W
    for _ in range(5):
        n.append((h - 10) * (w - 10))
        h, w = (h + 1) // 2, (w + 1) // 2
    return np.asarray(n, np.float64)


def means(s, H, W):
    return np.asarray(s, np.float64) / counts(H, W)[:, None, None]


def combine(s, H, W):
    m = means(s, H, W)
    terms = np.concatenate([m[:4, :, 0], m[4:, :, 1]])
    return float(np.mean(np.prod(np.maximum(terms, 0.0) ** np.asarray(WEIGHTS)[:, None], axis=0)))


def msssim(a, b, dtype=np.float64):
    return combine(sums(a, b, dtype), *np.asarray(a).shape[:2])


# ---------------------------------------------------------------------------- image kinds
def image(kind, H, W, seed):
    r = np.random.default_rng(seed)
    if kind == "smooth":  # test_gpu_image_batch._image without its noise term
        yy, xx = np.mgrid[0:H, 0:W]
        base = 128 + 60 * np.sin(xx / 17.0)[..., None] * np.cos(yy / 23.0)[..., None] + np.zeros((H, W, 3))
        return np.clip(base, 0, 255).astype(np.uint8)
    if kind == "noise":
        return r.integers(0, 256, (H, W, 3), dtype=np.uint8)
    if kind == "flat":
        return np.full((H, W, 3), 250, np.uint8)
    raise ValueError(kind)


def distort(a, n, seed):
    """b = clip(a + U{-n..n})."""
    r = np.random.default_rng(seed)
    return np.clip(a.astype(np.int64) + r.integers(-n, n + 1, a.shape), 0, 255).astype(np.uint8)

"""Rate / distortion evaluation, mirroring processing_utils/evaluate.py (same names and
formulas) with the per-image squared error optionally computed on the GPU.

* ``mse(a, b)``          evaluate.py:10-11 — the SUM of squared differences (the reference
                          names it mse; the division by the pixel count happens later).
* ``mse2psnr(m)``        :14-15 — 20 log10(255) - 10 log10(m).
* ``evaluate(pairs)``    :18-32 — dataset PSNR = mse2psnr(sum of SSE / sum of dims).
* ``get_code_size`` / ``calc_bpp`` / ``calc_psnr``  :35-66.

``sse_device(codec, d_a, d_b, n)`` is the GPU form of ``mse`` for uint8 images already in
HBM (exact integer sum, tic_sse_u8_device); the sharded dataset run and the benchmark
reduce it over ranks with the one stats all-gather.

MS-SSIM (the second measure of the CLIC challenge the codec was built for; not in the
reference's evaluate.py) follows Wang et al. 2003 with the choices of
``tf.image.ssim_multiscale``; the moments and the per-scale sums are computed on the GPU
(tic_msssim_images_device), the combination over scales is host float64:

* ``msssim_from_sums(sums, H, W)``  the 30 device sums of one image -> MS-SSIM.
* ``msssim_device(codec, d_a, d_b, offsets, sizes)``  image pairs already in HBM.
* ``msssim(a, b, codec)``           two host arrays.
* ``estimated_bits(counts, cum_freq)``  the ideal code length of a symbol histogram under
  the range coder's table (encode.py:77-97), known before any file is written.
* ``estimated_bits_ctx(counts, tables)``  the same under the ``K`` tables of a periodic context
  model (entropy.py), from the per-context histogram ``counts[K, Q]``.

As elsewhere there is no CPU fallback for the device parts.
"""
from __future__ import annotations

import os
from os.path import getsize, isfile, join

import numpy as np


def mse(image0, image1):
    return np.sum(np.square(np.asarray(image1, np.float32) - np.asarray(image0, np.float32)))


def mse2psnr(m):
    return 20.0 * np.log10(255.0) - 10.0 * np.log10(m)


def _read(path):
    from PIL import Image
    return np.asarray(Image.open(path), dtype=np.float32)


def evaluate(image_files):
    """image_files: iterable of (original, reconstruction) — paths or arrays."""
    num_dims = 0
    sq = []
    for a, b in image_files:
        img = _read(a) if isinstance(a, str) else np.asarray(a, np.float32)
        rec = _read(b) if isinstance(b, str) else np.asarray(b, np.float32)
        num_dims += img.size
        sq.append(mse(img, rec))
    return mse2psnr(np.sum(sq) / num_dims)


def get_code_size(folder):
    return sum(getsize(join(folder, f)) for f in os.listdir(folder)
               if isfile(join(folder, f)) and ".png" not in f)


def calc_bpp(code_dir, pixel_num):
    return get_code_size(code_dir) * 8.0 / pixel_num


def calc_psnr(ori_images_dir, recons_images_dir):
    pairs = [(join(ori_images_dir, f), join(recons_images_dir, f)) for f in os.listdir(ori_images_dir)]
    return evaluate(pairs)


def sse_device(codec, d_a, d_b, n: int, d_acc=None) -> int:
    """Exact sum of squared differences of two uint8 device buffers of n bytes."""
    own = d_acc is None
    if own:
        d_acc = codec.alloc(8)
    codec.memset_device(d_acc, 0, 8)
    codec.sse_u8_device(d_a, d_b, n, d_acc)
    v = int(d_acc.download((1,), np.uint64)[0])
    if own:
        d_acc.free()
    return v


MSSSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
MSSSIM_MIN_SIDE = 161  # 161 -> 81 -> 41 -> 21 -> 11: one 11x11 window at the fifth scale


def msssim_counts(H: int, W: int) -> np.ndarray:
    """Valid window positions (h_j - 10)(w_j - 10) of the five scales; scale j + 1 is the
    ceil half of scale j."""
    n = []
    h, w = int(H), int(W)
    for _ in MSSSIM_WEIGHTS:
        n.append((h - 10) * (w - 10))
        h, w = (h + 1) // 2, (w + 1) // 2
    return np.asarray(n, np.float64)


def msssim_from_sums(sums, H: int, W: int) -> float:
    """sums: float64 [5, 3, 2] — per scale and channel the sum of cs and of l*cs over the
    valid positions (tic_msssim_images_device).  MS(c) = prod_{j<4} max(mean cs_j, 0)^w_j *
    max(mean ssim_4, 0)^w_4; the result is the mean of MS(c) over the three channels."""
    if min(int(H), int(W)) < MSSSIM_MIN_SIDE:
        raise ValueError(f"MS-SSIM needs both sides >= {MSSSIM_MIN_SIDE}, got {H}x{W}")
    means = np.asarray(sums, np.float64).reshape(5, 3, 2) / msssim_counts(H, W)[:, None, None]
    w = np.asarray(MSSSIM_WEIGHTS, np.float64)
    terms = np.concatenate([means[:4, :, 0], means[4:, :, 1]])          # [5, 3]
    ms = np.prod(np.maximum(terms, 0.0) ** w[:, None], axis=0)         # [3]
    return float(np.mean(ms))


def msssim_sums_device(codec, d_a, d_b, offsets, sizes) -> np.ndarray:
    """The raw device sums, float64 [n, 5, 3, 2], of n uint8 image pairs in two arenas."""
    sizes = [(int(H), int(W)) for H, W in sizes]
    n = len(sizes)
    if n == 0:
        return np.zeros((0, 5, 3, 2), np.float64)
    d_scr = codec.alloc(max(codec.msssim_scratch_bytes(sizes), 16))
    d_out = codec.alloc(n * 30 * 8)
    try:
        codec.msssim_images_device(d_a, d_b, offsets, sizes, d_scr, d_out)
        return d_out.download((n, 5, 3, 2), np.float64)
    finally:
        d_scr.free()
        d_out.free()


def msssim_device(codec, d_a, d_b, offsets, sizes) -> np.ndarray:
    """MS-SSIM of every uint8 HWC image pair of two device arenas (image i of both at byte
    ``offsets[i]``), as float64 [n]."""
    sums = msssim_sums_device(codec, d_a, d_b, offsets, sizes)
    return np.asarray([msssim_from_sums(s, H, W) for s, (H, W) in zip(sums, sizes)], np.float64)


def msssim(a, b, codec) -> float:
    """MS-SSIM of two uint8 [H, W, 3] host arrays, computed on ``codec``'s device."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape != b.shape or b.dtype != np.uint8:
        raise ValueError(f"images must be uint8 [H, W, 3] of one shape, got {a.dtype} {a.shape} / {b.dtype} {b.shape}")
    d_a, d_b = codec.alloc(a.nbytes), codec.alloc(b.nbytes)
    try:
        d_a.upload(a)
        d_b.upload(b)
        return float(msssim_device(codec, d_a, d_b, [0], [a.shape[:2]])[0])
    finally:
        d_a.free()
        d_b.free()


def estimated_bits(counts, cum_freq) -> float:
    """-sum counts[s] * log2(freq[s] / total) for a cumulative table as
    range_coder.symbol_table builds it: the length the range coder approaches."""
    c = np.asarray(counts, np.float64).reshape(-1)
    cf = np.asarray(cum_freq, np.float64).reshape(-1)
    if cf.size != c.size + 1:
        raise ValueError(f"{c.size} counts for a table of {cf.size - 1} symbols")
    freq = np.diff(cf)
    used = c > 0
    if np.any(freq[used] <= 0):
        raise ValueError("a symbol with a count has zero frequency in the table")
    return float(-np.sum(c[used] * np.log2(freq[used] / cf[-1])))


def estimated_bits_ctx(counts, tables) -> float:
    """sum over the contexts k of estimated_bits(counts[k], tables[k]): ``counts[K, Q]`` is the
    per-context histogram (tic_histogram_ctx_device), ``tables[K, Q + 1]`` the cumulative tables."""
    c = np.asarray(counts, np.float64)
    cf = np.asarray(tables, np.float64)
    if c.ndim != 2 or cf.ndim != 2 or cf.shape != (c.shape[0], c.shape[1] + 1):
        raise ValueError(f"counts {c.shape} do not fit context tables {cf.shape}")
    freq = np.diff(cf, axis=1)
    used = c > 0
    if np.any(freq[used] <= 0):
        raise ValueError("a symbol with a count has zero frequency in its context's table")
    p = freq / cf[:, -1:]
    return float(-np.sum(c[used] * np.log2(p[used])))

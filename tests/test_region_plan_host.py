"""CPU tests of tic_region_plan (include/tic.h): the patch box a region of an image is decoded
from, against a brute-force boolean-mask model of what the region's pixels depend on: the crop,
every second-pass window of the post-filter that intersects it, and every first-pass window that
intersects that set (window grids as tic_rmbe_image_device lays them out)."""
import numpy as np
import pytest

from tf_image_compression_amd.codec import Codec


def windows(H, W, S, which):
    """(r, c) of the top-left corners of one pass's windows: pass 1 at column offset S/2, pass 2 at
    row offset S/2; a pass without a full row or column of windows has none."""
    o = S // 2
    r0, c0 = (0, o) if which == 1 else (o, 0)
    hn, wn = max(0, (H - r0) // S), max(0, (W - c0) // S)
    return [(r0 + a * S, c0 + b * S) for a in range(hn) for b in range(wn)]


def dependency_mask(H, W, S, y, x, h, w):
    m = np.zeros((H, W), bool)
    m[y:y + h, x:x + w] = True
    if S:
        for which in (2, 1):
            add = [(r, c) for r, c in windows(H, W, S, which) if m[r:r + S, c:c + S].any()]
            for r, c in add:
                m[r:r + S, c:c + S] = True
    return m


def check(H, W, P, y, x, h, w, S):
    py0, py1, px0, px1 = Codec.region_plan(H, W, P, y, x, h, w, S)
    hn, wn = -(-H // P), -(-W // P)
    assert 0 <= py0 < py1 <= hn and 0 <= px0 < px1 <= wn, (py0, py1, px0, px1)
    m = dependency_mask(H, W, S, y, x, h, w)
    rows, cols = np.flatnonzero(m.any(axis=1)), np.flatnonzero(m.any(axis=0))
    box = (py0 * P, min(py1 * P, H), px0 * P, min(px1 * P, W))
    assert box[0] <= rows[0] and rows[-1] < box[1] and box[2] <= cols[0] and cols[-1] < box[3], \
        ((H, W, P, y, x, h, w, S), box, (rows[0], rows[-1], cols[0], cols[-1]))
    own = ((y // P) * P, min(-(-(y + h) // P) * P, H), (x // P) * P, min(-(-(x + w) // P) * P, W))
    assert own[0] - box[0] < 2 * S + P and box[1] - own[1] < 2 * S + P
    assert own[2] - box[2] < 2 * S + P and box[3] - own[3] < 2 * S + P
    assert box[0] <= own[0] and own[1] <= box[1] and box[2] <= own[2] and own[3] <= box[3]
    if S == 0:
        assert (py0, py1, px0, px1) == (y // P, -(-(y + h) // P), x // P, -(-(x + w) // P))
    return py0, py1, px0, px1


@pytest.mark.parametrize("seed", range(6))
def test_random_regions_against_the_mask_model(seed):
    rng = np.random.default_rng(seed)
    for _ in range(120):
        H, W = (int(v) for v in rng.integers(1, 701, size=2))
        P = int(rng.choice([64, 128, 256]))
        h, w = int(rng.integers(1, H + 1)), int(rng.integers(1, W + 1))
        if rng.random() < 0.5:  # small regions are the use
            h, w = min(h, int(rng.integers(1, 40))), min(w, int(rng.integers(1, 40)))
        y, x = int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1))
        for S in (0, 128):
            check(H, W, P, y, x, h, w, S)


@pytest.mark.parametrize("P", [64, 128, 256])
@pytest.mark.parametrize("S", [0, 128])
def test_named_regions(P, S):
    H, W = 330, 460
    assert check(H, W, P, 0, 0, H, W, S) == (0, -(-H // P), 0, -(-W // P))  # the whole image
    for y, x in [(0, 0), (150, 200), (H - 1, W - 1), (63, 64), (64, 63), (191, 192), (192, 191)]:
        check(H, W, P, y, x, 1, 1, S)  # 1 x 1
    # 330 = 2 * 128 + 74, 460 = 3 * 128 + 76: rows >= 320 lie in no second-pass window and rows
    # >= 256 in no first-pass one; columns >= 448 in no first-pass window, >= 384 in no second-pass
    check(H, W, P, 322, 100, 8, 50, S)   # the bottom strip
    check(H, W, P, 100, 450, 50, 10, S)  # the right strip
    got = check(H, W, P, 322, 450, 8, 10, S)  # the corner no window covers
    assert got == (322 // P, -(-330 // P), 450 // P, -(-460 // P))  # the post-filter adds nothing
    check(H, W, P, 60, 60, 10, 10, S)    # across the first window borders
    check(H, W, P, 120, 120, 20, 20, S)
    # sizes below 128 and below 64: no window fits at all, or none in one direction
    for Hs, Ws in [(100, 100), (50, 50), (127, 300), (300, 127), (63, 63), (1, 1), (64, 192), (192, 64)]:
        for y, x, h, w in [(0, 0, Hs, Ws), (Hs - 1, Ws - 1, 1, 1), (Hs // 2, Ws // 3, 1, 1)]:
            got = check(Hs, Ws, P, y, x, h, w, S)
            if Hs < 128 and Ws < 128:
                assert got == check(Hs, Ws, P, y, x, h, w, 0)  # no band on either axis: nothing to add


def test_the_post_filter_widens_an_interior_region():
    # (200, 200) 8 x 8 in a 512 x 512 image: pass-2 rows [192, 320), columns [128, 256); pass 1
    # over that: rows [128, 384), columns [64, 320)
    assert Codec.region_plan(512, 512, 64, 200, 200, 8, 8, 0) == (3, 4, 3, 4)
    assert Codec.region_plan(512, 512, 64, 200, 200, 8, 8, 128) == (2, 6, 1, 5)
    assert Codec.region_plan(512, 512, 256, 200, 200, 8, 8, 128) == (0, 2, 0, 2)


def test_argument_errors():
    for y, x, h, w in [(0, 0, 0, 5), (0, 0, 5, 0), (0, 0, -1, 5), (-1, 0, 5, 5), (0, -1, 5, 5), (96, 0, 5, 5),
                       (0, 196, 5, 5), (0, 0, 101, 5), (0, 0, 5, 201), (100, 200, 1, 1)]:
        with pytest.raises(ValueError):
            Codec.region_plan(100, 200, 64, y, x, h, w, 0)
    for H, W, P, S in [(0, 10, 64, 0), (10, 0, 64, 0), (10, 10, 0, 0), (10, 10, 64, -128), (10, 10, 64, 127)]:
        with pytest.raises(ValueError):
            Codec.region_plan(H, W, P, 0, 0, 1, 1, S)
    assert Codec.region_plan(100, 200, 64, 95, 195, 5, 5, 0) == (1, 2, 3, 4)

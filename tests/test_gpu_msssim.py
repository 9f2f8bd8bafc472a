"""GPU tests of MS-SSIM on the device (tic_msssim.cpp), ImageCodec.evaluate_images and
evaluate_codec.py, against the float64 numpy restatement of the definition in
tests/msssim_ref.py.

Bars: every per-scale, per-channel mean within 5e-4 of float64 and the combined value within
1e-4.  On the 18 list inputs below the plain float32 numpy restatement itself deviates from
float64 by at most 1.65e-4 (per-scale mean) and 3.3e-5 (combined), both on the flat kind (every
other kind stays below 3e-5 / 1e-6); the bars are about 3x that.  The first test prints the
float32 restatement's deviation beside the GPU's (measured: 6.6e-5 / 5.2e-6; DESIGN.md §6b
records both).
"""
import json
import math

import numpy as np
import pytest

import msssim_ref as ref

pytestmark = pytest.mark.gpu

MEAN_BAR, MS_BAR = 5e-4, 1e-4
SIZES = [(161, 161), (177, 203), (256, 320)]
KINDS = ["smooth", "noise", "flat"]
NOISE = [2, 20]


@pytest.fixture(scope="module")
def codec():
    from tf_image_compression_amd.codec import Codec
    from tf_image_compression_amd.weights import synthetic_params, SYNTH_MEAN, SYNTH_STD
    c = Codec(0, synthetic_params(0, seed=0), SYNTH_MEAN, SYNTH_STD, patch_size=64)
    yield c
    c.close()


def _packed(sizes, gap=0, reverse=False):
    order = range(len(sizes) - 1, -1, -1) if reverse else range(len(sizes))
    offs, end = [0] * len(sizes), 0
    for i in order:
        offs[i] = end + gap
        end = offs[i] + sizes[i][0] * sizes[i][1] * 3
    return offs, end + gap


def _sums(codec, pairs, offs=None, total=None):
    """Device sums [n, 5, 3, 2] of the pairs laid out at `offs` (default: back to back)."""
    from tf_image_compression_amd.evaluate import msssim_sums_device
    sizes = [a.shape[:2] for a, _ in pairs]
    if offs is None:
        offs, total = _packed(sizes)
    arena_a, arena_b = np.full(total, 0xA5, np.uint8), np.full(total, 0x5A, np.uint8)
    for (a, b), off in zip(pairs, offs):
        arena_a[off:off + a.size] = a.reshape(-1)
        arena_b[off:off + b.size] = b.reshape(-1)
    d_a, d_b = codec.alloc(total), codec.alloc(total)
    d_a.upload(arena_a)
    d_b.upload(arena_b)
    try:
        return msssim_sums_device(codec, d_a, d_b, offs, sizes)
    finally:
        d_a.free()
        d_b.free()


def _check(got, a, b, want=None):
    """Both bars for one pair; returns (worst mean deviation, combined deviation)."""
    from tf_image_compression_amd.evaluate import msssim_from_sums
    H, W = a.shape[:2]
    want = ref.sums(a, b) if want is None else want
    dm = float(np.max(np.abs(ref.means(got, H, W) - ref.means(want, H, W))))
    dc = abs(msssim_from_sums(got, H, W) - ref.combine(want, H, W))
    return dm, dc


@pytest.fixture(scope="module")
def list_cases():
    """The 18 pairs of the list test with their float64 and float32 restatement sums."""
    cases = []
    for H, W in SIZES:
        for kind in KINDS:
            for n in NOISE:
                a = ref.image(kind, H, W, seed=H + W)
                b = ref.distort(a, n, seed=H * W + n)
                cases.append((f"{H}x{W} {kind} n={n}", a, b, ref.sums(a, b), ref.sums(a, b, np.float32)))
    return cases


def test_list_against_float64(codec, list_cases):
    pairs = [(a, b) for _, a, b, _, _ in list_cases]
    offs, _ = _packed([a.shape[:2] for a, _ in pairs])
    assert any(o % 2 for o in offs)  # 161 * 161 * 3 is odd: the later images start at odd bytes
    got = _sums(codec, pairs)
    worst = [0.0, 0.0, 0.0, 0.0]
    fails = []
    for (name, a, b, s64, s32), g in zip(list_cases, got):
        dm, dc = _check(g, a, b, s64)
        H, W = a.shape[:2]
        fm = float(np.max(np.abs(ref.means(s32, H, W) - ref.means(s64, H, W))))
        fc = abs(ref.combine(s32, H, W) - ref.combine(s64, H, W))
        print(f"{name}: gpu mean {dm:.2e} combined {dc:.2e} | float32 numpy mean {fm:.2e} combined {fc:.2e}")
        worst = [max(worst[0], dm), max(worst[1], dc), max(worst[2], fm), max(worst[3], fc)]
        if dm > MEAN_BAR or dc > MS_BAR:
            fails.append(name)
    print(f"worst: gpu mean {worst[0]:.2e} combined {worst[1]:.2e} | float32 numpy mean {worst[2]:.2e} "
          f"combined {worst[3]:.2e}")
    assert not fails, fails


def test_many_workgroups_against_float64(codec):
    a = ref.image("smooth", 600, 900, seed=1)
    b = ref.distort(a, 8, seed=2)
    dm, dc = _check(_sums(codec, [(a, b)])[0], a, b)
    print(f"600x900 smooth: gpu mean {dm:.2e} combined {dc:.2e}")
    assert dm <= MEAN_BAR and dc <= MS_BAR


def test_odd_last_row_and_column(codec):
    """The inverted last 4 rows / columns of a 177x203 image reach the coarser scales only
    through the odd last row / column paired with itself: dropping it moves the value by 2.0e-3,
    zero-padding it by 1.35e-3."""
    a = ref.image("noise", 177, 203, seed=9)
    b = a.copy()
    b[-4:] = 255 - b[-4:]
    b[:, -4:] = 255 - b[:, -4:]
    dm, dc = _check(_sums(codec, [(a, b)])[0], a, b)
    print(f"odd edges: gpu mean {dm:.2e} combined {dc:.2e}")
    assert dc <= MS_BAR


def test_negative_means_clamp_to_zero(codec):
    from tf_image_compression_amd.evaluate import msssim_from_sums
    a = ref.image("noise", 161, 161, seed=5)
    b = 255 - a
    got = _sums(codec, [(a, b)])[0]
    dm, _ = _check(got, a, b)
    assert np.all(ref.means(got, 161, 161)[:4, :, 0] < 0)
    assert dm <= MEAN_BAR
    assert msssim_from_sums(got, 161, 161) == 0.0


@pytest.mark.parametrize("H,W", [(161, 161), (177, 203)])
def test_identity_is_exact(codec, H, W):
    """b = a: cs = l = 1 at every position, so every sum is its position count exactly.  The
    scale-4 count of 161x161 is 1 (ceil sizes; floor sizes would leave 10x10, below the window)."""
    from tf_image_compression_amd.evaluate import msssim_from_sums
    a = ref.image("noise", H, W, seed=3)
    got = _sums(codec, [(a, a.copy())])[0]
    want = np.broadcast_to(ref.counts(H, W)[:, None, None], (5, 3, 2))
    if (H, W) == (161, 161):
        assert want[4, 0, 0] == 1
    assert np.array_equal(got, want)
    assert msssim_from_sums(got, H, W) == 1.0


def test_independent_of_list_position_and_offset(codec):
    a = ref.image("smooth", 177, 203, seed=11)
    b = ref.distort(a, 20, seed=12)
    other = [(ref.image("noise", 161, 161, seed=13), ref.image("noise", 161, 161, seed=14)),
             (ref.image("flat", 200, 163, seed=15), ref.image("smooth", 200, 163, seed=16))]
    alone = _sums(codec, [(a, b)])[0]
    three = [other[0], (a, b), other[1]]
    mid = _sums(codec, three)
    offs, total = _packed([p[0].shape[:2] for p in three], gap=5, reverse=True)
    assert offs[0] > offs[-1]
    rev = _sums(codec, three, offs, total)
    again = _sums(codec, [(a, b)])[0]
    assert np.array_equal(alone, mid[1])
    assert np.array_equal(alone, rev[1])
    assert np.array_equal(alone, again)
    assert np.array_equal(mid, rev)


def test_more_images_than_one_launch_holds(codec):
    """70 pairs run as two launch sequences (64 images per table); each equals its own
    single-image result bit for bit."""
    r = np.random.default_rng(70)
    base = ref.image("smooth", 161, 161, seed=20)
    pairs = []
    for k in range(70):
        a = np.roll(base, k, axis=1)
        pairs.append((a, np.clip(a.astype(np.int64) + r.integers(-1 - k, 2 + k, a.shape), 0, 255).astype(np.uint8)))
    got = _sums(codec, pairs)
    assert len({g.tobytes() for g in got}) == 70  # 70 different inputs, 70 different results
    for k in range(70):
        assert np.array_equal(got[k], _sums(codec, [pairs[k]])[0]), k


def test_errors_leave_the_output_untouched(codec):
    total = 200 * 200 * 3
    d_a, d_b = codec.alloc(total), codec.alloc(total)
    codec.memset_device(d_a, 7, total)
    codec.memset_device(d_b, 9, total)
    need = codec.msssim_scratch_bytes([(200, 200)])
    d_scr, d_short, d_out = codec.alloc(need), codec.alloc(need - 1), codec.alloc(2 * 240)
    codec.memset_device(d_out, 0xC3, 2 * 240)
    try:
        with pytest.raises(ValueError, match="161"):
            codec.msssim_images_device(d_a, d_b, [0], [(160, 250)], d_scr, d_out)
        with pytest.raises(ValueError, match="too small"):
            codec.msssim_images_device(d_a, d_b, [0], [(200, 200)], d_short, d_out)
        with pytest.raises(ValueError, match="offsets for"):
            codec.msssim_images_device(d_a, d_b, [0, 0], [(200, 200)], d_scr, d_out)
        codec.synchronize()
        assert np.all(d_out.download((2 * 240,), np.uint8) == 0xC3)
        codec.msssim_images_device(d_a, d_b, [0], [(200, 200)], d_scr, d_out)  # the same buffers do work
        out = d_out.download((2 * 240,), np.uint8)
        assert np.all(out[240:] == 0xC3) and not np.all(out[:240] == 0xC3)
    finally:
        for d in (d_a, d_b, d_scr, d_short, d_out):
            d.free()


EVAL_SIZES = [(200, 170), (161, 300), (100, 130)]


def _eval_image(H, W, seed):
    r = np.random.default_rng(seed)
    return np.clip(ref.image("smooth", H, W, seed).astype(np.float64) + r.normal(0, 12, (H, W, 3)), 0, 255).astype(
        np.uint8)


@pytest.mark.parametrize("post", [False, True])
def test_evaluate_images(codec, post):
    from tf_image_compression_amd import evaluate as ev
    from tf_image_compression_amd.codec import Codec
    from tf_image_compression_amd.image_codec import ImageCodec
    from tf_image_compression_amd.range_coder import symbol_table
    from tf_image_compression_amd.topology import RMBE_ID
    from tf_image_compression_amd.weights import synthetic_params, SYNTH_MEAN, SYNTH_STD
    cr = Codec(RMBE_ID, synthetic_params(RMBE_ID, seed=0), SYNTH_MEAN, SYNTH_STD, patch_size=128) if post else None
    ic = ImageCodec(codec, cr)
    try:
        imgs = [_eval_image(H, W, 30 + k) for k, (H, W) in enumerate(EVAL_SIZES)]
        cum = symbol_table([0.6, 0.4], 4096)
        res = ic.evaluate_images(imgs, post_filter=post, cum_freq=cum)
        sym = ic.encode_images(imgs)
        rec = ic.decode_images(sym, EVAL_SIZES, post_filter=post)
        assert len(res) == 3
        for k, (im, s, rc, r) in enumerate(zip(imgs, sym, rec, res)):
            # the device sum is the exact integer; evaluate.mse sums float32 squares pairwise, good to
            # about eps * log2(n) = 6e-8 * 17 of the sum
            sse = int(np.sum(np.square(im.astype(np.int64) - rc.astype(np.int64))))
            assert r["sse"] == sse and isinstance(r["sse"], int)
            assert r["sse"] == pytest.approx(float(ev.mse(im, rc)), rel=2e-6)
            assert r["psnr"] == pytest.approx(float(ev.mse2psnr(np.float64(sse) / im.size)), rel=1e-12)
            assert r["psnr"] == pytest.approx(float(ev.mse2psnr(np.float64(ev.mse(im, rc)) / im.size)), rel=1e-6)
            assert r["counts"].dtype == np.uint64
            assert np.array_equal(r["counts"], np.bincount(s.reshape(-1), minlength=2))
            assert r["n_symbols"] == s.size
            assert r["est_bits"] == ev.estimated_bits(r["counts"], cum)
            if k < 2:
                assert r["msssim"] == ev.msssim(im, rc, codec) and 0.0 < r["msssim"] < 1.0
            else:
                assert math.isnan(r["msssim"])
        assert ic.evaluate_images(imgs[:1], post_filter=post)[0]["est_bits"] is None
        assert ic.evaluate_images([]) == []
    finally:
        ic.close()
        if cr is not None:
            cr.close()


def test_cli(tmp_path, capsys):
    import evaluate_codec as ec
    from tf_image_compression_amd import utils
    paths = []
    for k, (H, W) in enumerate(EVAL_SIZES):
        p = str(tmp_path / f"img{k}.png")
        utils.imsave(p, _eval_image(H, W, 50 + k))
        paths.append(p)
    lst = tmp_path / "list.txt"
    lst.write_text("\n".join(paths) + "\n")
    dist = str(tmp_path / "dist.npy")
    np.save(dist, np.asarray([0.6, 0.4]))
    results = {}
    model = None
    for nb in ("4", "1"):
        out = str(tmp_path / f"eval{nb}.json")
        args = ec.my_parse_args(["-m", "0", "-g", "0", "--synthetic-weights", "--norm", "/nonexistent", "--dist", dist,
                                 "-v", str(lst), "--batch-images", nb, "--json", out])
        model = model or ec.load_model(args, ec.load_config("0"))
        ec.run(model, args)
        lines = capsys.readouterr().out.splitlines()
        assert sum(ln.startswith(tuple(paths)) for ln in lines) == 3 and lines[-1].startswith("dataset: psnr ")
        with open(out) as f:
            results[nb] = json.load(f)
    r = results["4"]
    assert [im["path"] for im in r["images"]] == paths
    for im in r["images"]:
        for key in ("height", "width", "sse", "psnr", "msssim", "msssim_db", "est_bits", "est_bpp", "n_symbols", "counts"):
            assert key in im
        assert im["est_bpp"] == im["est_bits"] / (im["height"] * im["width"])
    assert math.isnan(r["images"][2]["msssim"]) and 0 < r["images"][0]["msssim"] < 1
    d = r["dataset"]
    assert d["n_images"] == 3 and d["n_msssim"] == 2 and d["pixels"] == sum(H * W for H, W in EVAL_SIZES)
    assert d["msssim"] == pytest.approx((r["images"][0]["msssim"] + r["images"][1]["msssim"]) / 2, rel=1e-15)
    assert d["est_bpp"] == pytest.approx(sum(im["est_bits"] for im in r["images"]) / d["pixels"], rel=1e-15)
    # NaN != NaN: compare the text
    assert json.dumps(results["1"], sort_keys=True) == json.dumps(results["4"], sort_keys=True)
    assert list(tmp_path.glob("**/*.encoded")) == []

"""GPU parity of the whole-image path (BASELINE config 5) and the symbol histogram,
through the C-ABI, against the oracle's restatement of the reference's host code:

* tiling (utils/utils.py:96-133, np.pad 'reflect' incl. pads longer than the image),
  stitching (:136-167), rounding (decode.py:249) and the histogram
  (get_encoded_distribution.py:113-126) are integer/byte work: bit-exact;
* rmbe on a whole image (submit/2/rmbe/rmbe.py:15-111): the direct form within 4 E32 of the
  oracle and the default F(4x4,3x3) within twice the direct form's error floored at 1e-3
  (gpu_checks.float_bar / wino4_float_bar; test_gpu_rmbe.py holds the other geometries);
* image encode -> decode (-> rmbe): symbols bit-exact outside the decision band, uint8
  within 1 and only on .5 rounding edges, as test_gpu_parity.py.
"""
import numpy as np
import pytest

from gpu_checks import float_bar, rmbe_image_reference, wino4_float_bar
from oracle import tic_oracle as o

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def codecs():
    from tf_image_compression_amd.codec import Codec
    from tf_image_compression_amd.weights import synthetic_params, SYNTH_MEAN, SYNTH_STD
    from tf_image_compression_amd.topology import RMBE_ID
    p0 = synthetic_params(0, seed=0)
    pr = synthetic_params(RMBE_ID, seed=0)
    c0 = Codec(0, p0, SYNTH_MEAN, SYNTH_STD, patch_size=64)
    cr = Codec(RMBE_ID, pr, SYNTH_MEAN, SYNTH_STD, patch_size=128)
    yield c0, cr, p0, pr
    c0.close()
    cr.close()


def _image(H, W, seed):
    r = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    base = 128 + 60 * np.sin(xx / 17.0)[..., None] * np.cos(yy / 23.0)[..., None] + r.normal(0, 12, (H, W, 3))
    return np.clip(base, 0, 255).astype(np.uint8)


@pytest.mark.parametrize("H,W,P", [(100, 130, 64), (64, 128, 64), (20, 37, 64), (1, 9, 4), (130, 70, 32)])
def test_tile_reflect_bit_exact(codecs, H, W, P):
    c0 = codecs[0]
    img = _image(H, W, H * 7 + W)
    ref = np.stack(o.crop_image_input_patches(img, P))
    d_img = c0.alloc(img.nbytes)
    d_img.upload(img)
    d_pat = c0.alloc(ref.nbytes)
    c0.image_to_patches_device(d_img, H, W, P, d_pat)
    got = d_pat.download(ref.shape, np.uint8)
    d_img.free()
    d_pat.free()
    assert np.array_equal(got, ref)


@pytest.mark.parametrize("H,W,P", [(100, 130, 64), (128, 64, 64), (5, 70, 32)])
def test_stitch_bit_exact(codecs, H, W, P):
    c0 = codecs[0]
    hn, wn = -(-H // P), -(-W // P)
    pat = np.random.default_rng(H + W).random((hn * wn, P, P, 3), dtype=np.float32) * 255
    ref = o.concat_patches(pat, H, W, P)
    d_pat = c0.alloc(pat.nbytes)
    d_pat.upload(pat)
    d_img = c0.alloc(H * W * 3 * 4)
    c0.patches_to_image_device(d_pat, H, W, P, d_img)
    got = d_img.download((H, W, 3), np.float32)
    d_pat.free()
    d_img.free()
    assert np.array_equal(got, ref)


def test_round_u8_half_even(codecs):
    c0 = codecs[0]
    x = np.concatenate([np.arange(0, 255.5, 0.5, dtype=np.float32),
                        np.random.default_rng(1).random(1001, dtype=np.float32) * 255]).astype(np.float32)
    d_x = c0.alloc(x.nbytes)
    d_x.upload(x)
    d_y = c0.alloc(x.size)
    c0.round_u8_device(d_x, x.size, d_y)
    got = d_y.download(x.shape, np.uint8)
    assert np.array_equal(got, o.around_u8(x))


@pytest.mark.parametrize("Q,n", [(2, 1 << 16), (2, 1003), (5, 4099), (256, 100001), (3, 3)])
def test_histogram_matches_numpy(codecs, Q, n):
    from tf_image_compression_amd.image_codec import symbol_histogram
    c0 = codecs[0]
    top = min(255, Q + 2)  # include values == Q (closed last bin) and > Q (ignored)
    s = np.random.default_rng(Q + n).integers(0, top + 1, n).astype(np.uint8)
    d_s = c0.alloc(n)
    d_s.upload(s)
    got = symbol_histogram(c0, d_s, n, Q)
    ref, _ = np.histogram(s, list(range(Q + 1)))
    assert np.array_equal(got.astype(np.int64), ref)


def test_rmbe_whole_image(codecs):
    _, cr, _, pr = codecs
    H, W = 200, 330  # pass 1: 1 x 2 windows, pass 2: 1 x 2; edge strips untouched
    img = _image(H, W, 11).astype(np.float32)
    ref, e32 = rmbe_image_reference(pr, img)
    d = cr.alloc(img.nbytes)
    d.upload(img)
    cr.rmbe_image_device(d, H, W)
    cr.synchronize()
    got = d.download(img.shape, np.float32)
    # the bars of test_gpu_rmbe.py: the direct form within 4 E32 (the two-pass E32 of the reference
    # accumulated in f32), the default F(4x4,3x3) within wino4_float_bar of the direct form's error
    assert any("wino4" in k for k in cr.layer_kernels(1))
    try:
        cr.set_option("s1_form", 0)
        d.upload(img)
        cr.rmbe_image_device(d, H, W)
        cr.synchronize()
        direct = d.download(img.shape, np.float32)
    finally:
        cr.set_option("s1_form", -1)
    err_direct = float(np.max(np.abs(direct.astype(np.float64) - ref)))
    err = float(np.max(np.abs(got.astype(np.float64) - ref)))
    print(f"\nrmbe whole image: E32 {e32:.3e} direct {err_direct:.3e} default {err:.3e}")
    assert err_direct <= float_bar(e32), (err_direct, e32)
    assert err <= wino4_float_bar(err_direct), (err, err_direct)
    # untouched strips are bit-identical to the input
    assert np.array_equal(got[192:], img[192:])
    assert np.array_equal(got[:64, :64], img[:64, :64])
    assert np.array_equal(got[128:, 256:], img[128:, 256:])
    assert np.array_equal(got[:128, 320:], img[:128, 320:])


@pytest.mark.parametrize("post", [False, True])
def test_image_roundtrip(codecs, post):
    from tf_image_compression_amd.image_codec import ImageCodec
    from tf_image_compression_amd.weights import SYNTH_MEAN, SYNTH_STD
    c0, cr, p0, pr = codecs
    H, W, P = 200, 330, 64
    img = _image(H, W, 5)
    ic = ImageCodec(c0, cr if post else None)
    sym = ic.encode_image(img)
    patches = np.stack(o.crop_image_input_patches(img, P))
    pre, ref_sym = o.encoder(p0, SYNTH_MEAN, SYNTH_STD, patches, P, 2, 0)
    scale = max(1.0, float(np.abs(pre).max()))
    safe = o.decision_margin(pre, 2) > 1e-5 * scale
    assert sym.shape == ref_sym.shape
    assert int(np.count_nonzero((sym != ref_sym) & safe)) == 0
    rec = ic.decode_image(sym, H, W, post_filter=post)
    f, _ = o.decoder(p0, SYNTH_MEAN, SYNTH_STD, sym, 2, 0)   # decoder fed the SAME symbols
    fimg = o.concat_patches(f, H, W, P)
    if post:
        fimg = o.rmbe(fimg, pr, SYNTH_MEAN, SYNTH_STD)
    ref = o.around_u8(fimg)
    du = np.abs(rec.astype(np.int16) - ref.astype(np.int16))
    assert int(du.max()) <= 1
    edge = np.abs(np.abs(fimg - np.floor(fimg)) - 0.5) < 1e-2
    assert not np.any((du > 0) & ~edge)
    ic.close()


@pytest.mark.parametrize("n", [1, 7, 4096 + 3, 3 * 256 * 256 * 5])
def test_sse_u8_exact(codecs, n):
    from tf_image_compression_amd.evaluate import sse_device, mse
    c0 = codecs[0]
    r = np.random.default_rng(n)
    a = r.integers(0, 256, n, dtype=np.uint8)
    b = r.integers(0, 256, n, dtype=np.uint8)
    da, db = c0.alloc(n), c0.alloc(n)
    da.upload(a)
    db.upload(b)
    got = sse_device(c0, da, db, n)
    ref = int(np.sum(np.square(a.astype(np.int64) - b.astype(np.int64))))
    assert got == ref
    assert np.isclose(float(mse(a, b)), float(ref), rtol=1e-5)


def test_get_encoded_distribution_tool(codecs, tmp_path):
    """get_encoded_distribution.py on 66 PNG patches (two batches of <= 64): the GPU
    histogram equals np.histogram of the encoder's symbols (get_encoded_distribution.py:113-129)."""
    import importlib.util
    import os
    from PIL import Image
    from conftest import ROOT, structured_patches
    spec = importlib.util.spec_from_file_location("ged", os.path.join(ROOT, "get_encoded_distribution.py"))
    ged = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ged)
    c0 = codecs[0]  # model_0 at P = 64
    pats = structured_patches(66, 64, seed=21)
    paths = []
    for i, p in enumerate(pats):
        f = str(tmp_path / f"p{i}.png")
        Image.fromarray(p).save(f)
        paths.append(f)
    freq = ged.encoded_frequencies(c0, ged.patch_batches(paths, 64), 2)
    sym = c0.encode(pats)
    ref, _ = np.histogram(sym, [0, 1, 2])
    assert np.array_equal(freq, ref.astype(np.float64))


def test_image_pipeline_back_to_back(codecs):
    """Three images enqueued back to back (no host synchronisation): the codec of image
    i+1 overlaps the rmbe passes of image i through the two stitch buffers and named
    events; results equal images decoded one at a time."""
    from tf_image_compression_amd.image_codec import ImageCodec
    c0, cr, _, _ = codecs
    H, W = 200, 330
    imgs = [_image(H, W, 30 + k) for k in range(3)]
    ic = ImageCodec(c0, cr)
    ref = [ic.decode_image(ic.encode_image(im), H, W, post_filter=True) for im in imgs]
    eh, ew, ec = c0.code_shape
    n = ic.num_patches(H, W)
    d_img = [c0.alloc(H * W * 3) for _ in imgs]
    d_sym = [c0.alloc(n * eh * ew * ec) for _ in imgs]
    d_out = [c0.alloc(H * W * 3) for _ in imgs]
    for d, im in zip(d_img, imgs):
        d.upload(im)
    for k in range(3):
        ic.roundtrip_device(d_img[k], H, W, d_sym[k], d_out[k], post_filter=True)
    ic.synchronize()
    for k in range(3):
        assert np.array_equal(d_out[k].download((H, W, 3), np.uint8), ref[k])
    # the same output buffer reused for consecutive images: the last write wins
    for k in (0, 1, 2):
        ic.roundtrip_device(d_img[k], H, W, d_sym[0], d_out[0], post_filter=True)
    ic.synchronize()
    assert np.array_equal(d_out[0].download((H, W, 3), np.uint8), ref[2])
    ic.close()

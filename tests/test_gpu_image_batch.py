"""GPU tests of the image-list path (tic_image_batch.cpp, ImageCodec.*_images*, the CLIs'
--batch-images): several images of different sizes as ONE patch batch.

* ragged tiling and stitching are byte / word movement: bit-exact against the oracle's
  restatement of utils.crop_image_input_patches / concat_patches per image, for offsets of any
  alignment, order and gaps, and nothing outside the images is written;
* the ragged rmbe passes give every image bit-identically what tic_rmbe_image_device gives it
  alone (patches are independent of how a batch is split), and stay within the whole-image bars
  of test_gpu_image.py (gpu_checks.float_bar / wino4_float_bar of the two-pass E32) of the oracle;
* the list forms and the CLIs with --batch-images > 1 give byte for byte what the single-image
  forms give.
"""
import filecmp
import os

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


def _packed(sizes, gap=0, reverse=False):
    """Offsets of the images laid out in list order (or in reversed order) with `gap` elements
    in front of each, and the arena's length."""
    order = range(len(sizes) - 1, -1, -1) if reverse else range(len(sizes))
    offs, end = [0] * len(sizes), 0
    for i in order:
        offs[i] = end + gap
        end = offs[i] + sizes[i][0] * sizes[i][1] * 3
    return offs, end + gap


def _tile_case(c0, sizes, P, offs, total):
    imgs = [_image(H, W, 7 * H + W) for H, W in sizes]
    arena = np.full(total, 0xA5, np.uint8)
    for im, off in zip(imgs, offs):
        arena[off:off + im.size] = im.reshape(-1)
    ref = np.concatenate([np.stack(o.crop_image_input_patches(im, P)) for im in imgs])
    d_img = c0.alloc(total)
    d_img.upload(arena)
    d_pat = c0.alloc(ref.nbytes + 64)
    c0.memset_device(d_pat, 0x5A, ref.nbytes + 64)
    n = c0.images_to_patches_device(d_img, offs, sizes, P, d_pat)
    got = d_pat.download((ref.nbytes + 64,), np.uint8)
    d_img.free()
    d_pat.free()
    assert n == ref.shape[0]
    assert np.array_equal(got[:ref.nbytes].reshape(ref.shape), ref)
    assert np.all(got[ref.nbytes:] == 0x5A)  # nothing behind the last patch is written


TILE_SIZES = [(100, 130), (64, 128), (20, 37), (1, 9), (130, 70), (64, 64)]


def test_ragged_tiling_packed_odd_offsets(codecs):
    offs, total = _packed(TILE_SIZES)
    assert any(off % 2 for off in offs)  # the 27-byte image makes the later offsets odd
    _tile_case(codecs[0], TILE_SIZES, 64, offs, total)


def test_ragged_tiling_reversed_offsets_with_gaps(codecs):
    offs, total = _packed(TILE_SIZES, gap=5, reverse=True)
    assert offs[0] > offs[-1]
    _tile_case(codecs[0], TILE_SIZES, 64, offs, total)


def test_ragged_tiling_tiny_patches(codecs):
    sizes = [(1, 9), (3, 1), (9, 2)]
    offs, total = _packed(sizes)
    _tile_case(codecs[0], sizes, 4, offs, total)


def test_ragged_tiling_more_images_than_one_launch_holds(codecs):
    """A launch carries the table of at most 64 images: 131 images run as three launches."""
    sizes = [(1 + (3 * k) % 11, 1 + (5 * k) % 13) for k in range(131)]
    offs, total = _packed(sizes, gap=1)
    _tile_case(codecs[0], sizes, 4, offs, total)


def test_ragged_tiling_single_image_equals_single_entry(codecs):
    c0 = codecs[0]
    H, W, P = 100, 130, 64
    img = _image(H, W, 3)
    n = -(-H // P) * -(-W // P)
    d_img = c0.alloc(img.nbytes)
    d_img.upload(img)
    d_a, d_b = c0.alloc(n * P * P * 3), c0.alloc(n * P * P * 3)
    c0.image_to_patches_device(d_img, H, W, P, d_a)
    assert c0.images_to_patches_device(d_img, [0], [(H, W)], P, d_b) == n
    a = d_a.download((n, P, P, 3), np.uint8)
    b = d_b.download((n, P, P, 3), np.uint8)
    for d in (d_img, d_a, d_b):
        d.free()
    assert np.array_equal(a, b)


def _stitch_case(c0, sizes, P, offs, total):
    r = np.random.default_rng(len(sizes) + P)
    pats = [r.random((-(-H // P) * -(-W // P), P, P, 3), dtype=np.float32) * 255 for H, W in sizes]
    sentinel = np.float32(-12345.5)
    ref = np.full(total, sentinel, np.float32)
    for pat, (H, W), off in zip(pats, sizes, offs):
        ref[off:off + H * W * 3] = o.concat_patches(pat, H, W, P).reshape(-1)
    allp = np.concatenate(pats)
    d_pat = c0.alloc(allp.nbytes)
    d_pat.upload(allp)
    d_img = c0.alloc(total * 4)
    d_img.upload(np.full(total, sentinel, np.float32))
    c0.patches_to_images_device(d_pat, offs, sizes, P, d_img)
    got = d_img.download((total,), np.float32)
    d_pat.free()
    d_img.free()
    assert np.array_equal(got, ref)  # the images bit-exact, every other element still the sentinel


def test_ragged_stitching_with_gaps(codecs):
    sizes = [(100, 130), (128, 64), (5, 70)]
    offs, total = _packed(sizes, gap=7)
    _stitch_case(codecs[0], sizes, 64, offs, total)
    offs, total = _packed(sizes, gap=3, reverse=True)
    _stitch_case(codecs[0], sizes, 64, offs, total)


def test_ragged_stitching_more_images_than_one_launch_holds(codecs):
    sizes = [(1 + (3 * k) % 11, 1 + (5 * k) % 13) for k in range(131)]
    offs, total = _packed(sizes, gap=1)
    _stitch_case(codecs[0], sizes, 4, offs, total)


def test_ragged_stitching_rejects_overlap(codecs):
    c0 = codecs[0]
    d = c0.alloc(1 << 16)
    with pytest.raises(ValueError, match="overlap"):
        c0.patches_to_images_device(d, [0, 299], [(10, 10), (4, 5)], 64, d)
    with pytest.raises(ValueError, match="overlap"):
        codecs[1].rmbe_images_device(d, [299, 0], [(4, 5), (10, 10)])
    d.free()


def _rmbe_case(cr, sizes, gap, check=None):
    """Ragged rmbe over an arena against tic_rmbe_image_device per image; returns the images
    before and after."""
    imgs = [_image(H, W, 11 + k).astype(np.float32) for k, (H, W) in enumerate(sizes)]
    offs, total = _packed(sizes, gap=gap)
    sentinel = np.float32(-777.25)
    arena = np.full(total, sentinel, np.float32)
    for im, off in zip(imgs, offs):
        arena[off:off + im.size] = im.reshape(-1)
    d = cr.alloc(total * 4)
    d.upload(arena)
    cr.rmbe_images_device(d, offs, sizes)
    cr.synchronize()
    got = d.download((total,), np.float32)
    d.free()
    inside = np.zeros(total, bool)
    outs = []
    for im, (H, W), off in zip(imgs, sizes, offs):
        inside[off:off + im.size] = True
        outs.append(got[off:off + im.size].reshape(H, W, 3))
    assert np.all(got[~inside] == sentinel)
    for k, (im, out) in enumerate(zip(imgs, outs)):
        if check is not None and k not in check:
            continue
        H, W = sizes[k]
        d1 = cr.alloc(im.nbytes)
        d1.upload(im)
        cr.rmbe_image_device(d1, H, W)
        cr.synchronize()
        alone = d1.download(im.shape, np.float32)
        d1.free()
        assert np.array_equal(out, alone), f"image {k} {sizes[k]}"
    return imgs, outs


def test_ragged_rmbe(codecs):
    _, cr, _, pr = codecs
    # (128,192): a pass-1 window only; (100,500) and (64,700): no window in either pass
    # ((64-64)//128 == 0 rows); (256,256): 2x1 then 1x2 windows
    sizes = [(200, 330), (128, 192), (100, 500), (256, 256), (64, 700)]
    imgs, outs = _rmbe_case(cr, sizes, gap=3)
    assert np.array_equal(outs[2], imgs[2]) and np.array_equal(outs[4], imgs[4])
    assert not np.array_equal(outs[1], imgs[1])
    assert np.array_equal(outs[1][:, :64], imgs[1][:, :64])
    # the bars of test_gpu_rmbe.py: the direct form of the same ragged call within 4 E32, the
    # default F(4x4,3x3) within wino4_float_bar of the direct form's error
    ref, e32 = rmbe_image_reference(pr, imgs[0])
    assert any("wino4" in k for k in cr.layer_kernels(1))
    try:
        cr.set_option("s1_form", 0)
        _, direct = _rmbe_case(cr, sizes, gap=3, check=set())
    finally:
        cr.set_option("s1_form", -1)
    err_direct = float(np.max(np.abs(direct[0].astype(np.float64) - ref)))
    err = float(np.max(np.abs(outs[0].astype(np.float64) - ref)))
    print(f"\nragged rmbe: E32 {e32:.3e} direct {err_direct:.3e} default {err:.3e}")
    assert err_direct <= float_bar(e32), (err_direct, e32)
    assert err <= wino4_float_bar(err_direct), (err, err_direct)


def test_ragged_rmbe_more_images_than_one_launch_holds(codecs):
    """67 images, windows only in images 0, 63, 64 and 66: the window batch of a pass is
    gathered and written back by two launches."""
    _, cr, _, _ = codecs
    sizes = [(16, 24)] * 67
    for k, s in {0: (128, 192), 63: (200, 200), 64: (192, 128), 66: (128, 320)}.items():
        sizes[k] = s
    imgs, outs = _rmbe_case(cr, sizes, gap=1, check={0, 63, 64, 66})
    for k in range(67):
        if k not in (0, 63, 64, 66):
            assert np.array_equal(outs[k], imgs[k])


E2E_SIZES = [(200, 330), (40, 50), (64, 64), (130, 257), (300, 70)]


@pytest.fixture(scope="module")
def e2e(codecs):
    """The per-image results every end-to-end case compares with, computed once (chunk 8: the
    patch batch of a list is cut inside an image)."""
    from tf_image_compression_amd.image_codec import ImageCodec
    c0, cr, _, _ = codecs
    imgs = [_image(H, W, 40 + k) for k, (H, W) in enumerate(E2E_SIZES)]
    c0.set_option("chunk", 8)
    cr.set_option("chunk", 8)
    ic = ImageCodec(c0, cr)
    sym = [ic.encode_image(im) for im in imgs]
    rec = {post: [ic.decode_image(s, H, W, post_filter=post) for s, (H, W) in zip(sym, E2E_SIZES)]
           for post in (False, True)}
    yield ic, imgs, sym, rec
    ic.close()
    c0.set_option("chunk", 256)
    cr.set_option("chunk", 256)


def test_encode_images_equals_per_image(e2e):
    ic, imgs, sym, _ = e2e
    got = ic.encode_images(imgs)
    assert len(got) == len(sym)
    for a, b in zip(got, sym):
        assert a.shape == b.shape and a.dtype == b.dtype
        assert np.array_equal(a, b)
    assert ic.encode_images([]) == []


@pytest.mark.parametrize("post", [False, True])
def test_decode_images_equals_per_image(e2e, post):
    ic, _, sym, rec = e2e
    got = ic.decode_images(sym, E2E_SIZES, post_filter=post)
    assert len(got) == len(sym)
    for a, b in zip(got, rec[post]):
        assert a.shape == b.shape and a.dtype == np.uint8
        assert np.array_equal(a, b)
    with pytest.raises(ValueError, match="patches of symbols"):
        ic.decode_images(sym[:2], [E2E_SIZES[1], E2E_SIZES[0]], post_filter=post)


def test_two_groups_back_to_back_on_the_device(e2e):
    """Two groups through the device forms with no host synchronisation in between: both read
    one input arena, write one symbol arena and one output arena (each its own part), and share
    ImageCodec's internal patch buffers and stitch arenas.  Then two more calls that write the
    SAME part of a second output arena back to back: the last write wins, as
    test_gpu_image.py::test_image_pipeline_back_to_back pins for single images."""
    ic, imgs, _, rec = e2e
    c0 = ic.codec
    eh, ew, ec = c0.code_shape
    groups = [[0, 1, 2], [3, 4]]
    assert ic.plan_batches(E2E_SIZES, 64, 3) == groups
    offs, total = ic.packed_offsets(E2E_SIZES)
    counts = [ic.num_patches(H, W) for H, W in E2E_SIZES]
    code = eh * ew * ec
    d_in, d_sym, d_out, d_out2 = c0.alloc(total), c0.alloc(sum(counts) * code), c0.alloc(total), c0.alloc(total)
    d_in.upload(np.concatenate([im.reshape(-1) for im in imgs]))
    c0.memset_device(d_out, 0xEE, total)
    c0.synchronize()
    sym_views = []
    for g in groups:
        sizes = [E2E_SIZES[i] for i in g]
        goffs = [offs[i] for i in g]
        sv = d_sym.view(sum(counts[:g[0]]) * code)
        sym_views.append(sv)
        assert ic.encode_images_device(d_in, goffs, sizes, sv) == sum(counts[i] for i in g)
        ic.decode_images_device(sv, goffs, sizes, d_out, post_filter=True)
    # group 2, then group 1, both from the front of the second arena: group 1 is longer and wins
    for k in (1, 0):
        sizes = [E2E_SIZES[i] for i in groups[k]]
        ic.decode_images_device(sym_views[k], ic.packed_offsets(sizes)[0], sizes, d_out2, post_filter=True)
    ic.synchronize()
    flat = d_out.download((total,), np.uint8)
    flat2 = d_out2.download((offs[3],), np.uint8)
    for d in (d_in, d_sym, d_out, d_out2):
        d.free()
    for i, (H, W) in enumerate(E2E_SIZES):
        assert np.array_equal(flat[offs[i]:offs[i] + H * W * 3].reshape(H, W, 3), rec[True][i]), i
    assert np.array_equal(flat2, np.concatenate([rec[True][i].reshape(-1) for i in groups[0]]))


def _write_pngs(tmp_path, sizes):
    from tf_image_compression_amd import utils
    paths = []
    for k, (h, w) in enumerate(sizes):
        p = str(tmp_path / f"img{k}.png")
        utils.imsave(p, _image(h, w, 60 + k))
        paths.append(p)
    lst = tmp_path / "list.txt"
    lst.write_text("\n".join(paths) + "\n")
    return str(lst)


@pytest.mark.parametrize("model_num,rmbe", [("0", False), ("3", True)])
def test_cli_batch_images_writes_identical_files(tmp_path, capsys, model_num, rmbe):
    import encode
    import decode
    from tf_image_compression_amd.topology import RMBE_ID
    from tf_image_compression_amd.weights import save_params, synthetic_params
    sizes = [(300, 200), (130, 257), (64, 64), (256, 300), (200, 330)]
    lst = _write_pngs(tmp_path, sizes)
    common = ["-m", model_num, "-g", "0", "--synthetic-weights", "--norm", "/nonexistent", "--raw"]
    post = []
    if rmbe:
        w = str(tmp_path / "rmbe.npz")
        save_params(w, synthetic_params(RMBE_ID))
        post = ["--rmbe", w, "--rmbe-norm", "/nonexistent"]
    cfg = encode.load_config(model_num)
    runs = {nb: (str(tmp_path / f"enc{nb}"), str(tmp_path / f"rec{nb}")) for nb in ("1", "3")}
    lines = {nb: [] for nb in runs}
    capsys.readouterr()
    model = None
    for nb, (enc_dir, _) in runs.items():
        eargs = encode.my_parse_args(common + ["-v", lst, "-o", enc_dir, "--batch-images", nb])
        model = model or encode.load_model(eargs, cfg)
        encode.compress(model, eargs)
        lines[nb].append([ln.replace(enc_dir, "ENC") for ln in capsys.readouterr().out.splitlines()
                          if ln.startswith("encodepath: ")])
    model = None
    for nb, (enc_dir, rec_dir) in runs.items():
        dargs = decode.my_parse_args(common + post + ["-i", enc_dir, "-o", rec_dir, "--batch-images", nb])
        model = model or decode.load_model(dargs, cfg)
        decode.uncompress(model, dargs)
        lines[nb].append([ln.replace(rec_dir, "REC") for ln in capsys.readouterr().out.splitlines()
                          if ln.startswith("recons_image_path: ")])
    assert len(lines["1"][0]) == 5 and len(lines["1"][1]) == 5
    assert lines["1"] == lines["3"]  # the printed path lines, order included
    for kind, count_suffix in (("enc", ".encoded"), ("rec", ".png")):
        a, b = str(tmp_path / f"{kind}1"), str(tmp_path / f"{kind}3")
        names = sorted(os.listdir(a))
        assert names == sorted(os.listdir(b))
        assert len(names) == 5 and all(n.endswith(count_suffix) for n in names)
        match, mismatch, errors = filecmp.cmpfiles(a, b, names, shallow=False)
        assert (sorted(match), mismatch, errors) == (names, [], [])

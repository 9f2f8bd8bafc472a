"""The rmbe post-filter against the oracle: the window network in every form it can run, and the
whole-image driver over several chunks and lanes (submit/2/rmbe/model.py:113-197: normalise,
conv_1 .. conv6, denormalise + clip, float in and float out; rmbe.py:15-111: pass 1 filters the
128 x 128 windows at column offset 64, writes them back, pass 2 those at row offset 64).

The net has paths no codec has: f32 input into enc01_kernel / conv_rgb_s2_kernel, f32 output from
dec10_kernel and the last-layer kernels without rounding, and F(4x4,3x3) as its default form.

(a) the net on gpu_checks.rmbe_net_windows() — two structured crops, Gaussian noise, all 0, all
    255 — fully unfused in each stride-1 form, in the F(2x2,3x3) chain at both workgroup sizes, in
    the default options and in the shipped state, every launch asserted by name.  Bars: the
    reference's own f32 error E32 of the call (gpu_checks.rmbe_reference); direct, F(2x2,3x3) and
    the chain within float_bar(E32) = 4 E32, whatever runs F(4x4,3x3) within
    wino4_float_bar(direct form's error), as the codecs.  The all-255 window, whose
    oracle output clips at 0 in 12.6 % of its values, is held to the bar of its own E32 apart from
    the others, so neither hides behind the other's error;
(b) every TIC_ENC01_VARIANT, TIC_DEC10_VARIANT and TIC_RGB_OUT_TILE bit-identical to the unfused run;
(c) tic_rmbe_image_device on the float images of gpu_checks.RMBE_IMAGES — no window in one pass,
    in either, one each and overlapping, 2 x 3 and 3 x 2 — at chunk 256 and 4, one and two lanes:
    within the form's bar of the two-pass E32, every pixel outside the windows bit-identical to
    the input, nothing behind the image written, all four runs bit-identical;
(d) the same images in one arena with gaps through tic_rmbe_images_device at chunk 4.
Every handle runs with option "poison" on.  The input conditions (nothing clipped, window counts,
E32 > 0) are asserted on the CPU by test_parity_inputs_host.py."""
import re

import numpy as np
import pytest

import gpu_checks as g

pytestmark = pytest.mark.gpu

UNFUSED = dict(chain=0, fuse01=0, fuse_tail=0)
S1_KERNEL = {0: r"conv3x3<0,64,64,", 1: r"conv3x3_wino_kernel<64,64,", 2: r"conv3x3_wino4_kernel<64,64,"}
L = 6  # conv_1, conv_2 (stride 2), conv_3, conv_4 (stride 1, 64 -> 64), conv_5, conv6 (transposed)
SENTINEL = np.float32(-777.25)


def _unfused_plan(form):
    return [r"conv_rgb_s2_kernel<32,\d+,false>", r"conv3x3<1,32,64,", S1_KERNEL[form], S1_KERNEL[form],
            r"conv3x3<2,64,32,", r"convT_rgb_valu_kernel<32,\d+>"]


FUSED_HEAD, FUSED_TAIL = [r"enc01_kernel<32,64,\d,false,", r"$"], [r"dec10_kernel<64,32,false,", r"$"]


def _assert_plan(c, plan, batches):
    for n in batches:
        kern = c.layer_kernels(n)
        assert len(kern) == len(plan) == L, kern
        for k, pat in zip(kern, plan):
            assert re.match(pat, k), (n, pat, kern)


@pytest.fixture(scope="module")
def rmbe():
    """(plain, shipped, params): a handle with the runtime's defaults and one made the product way
    (the shipped tuning applied), both poisoned."""
    from tf_image_compression_amd.codec import Codec
    from tf_image_compression_amd.topology import RMBE_ID
    params = g.rmbe_params()
    plain = g.poisoned(Codec(RMBE_ID, params, g.codec_mean(), g.codec_std(), patch_size=128, tuning="none"))
    shipped = g.poisoned(Codec(RMBE_ID, params, g.codec_mean(), g.codec_std(), patch_size=128))
    src = shipped.tuning_source
    assert src.startswith("shipped tuning:") and "model100_p128_b256_s2.json" in src, src
    yield plain, shipped, params
    plain.close()
    shipped.close()


@pytest.fixture(scope="module")
def net_ref():
    """The oracle of the five windows, computed once: (windows, ref, E32 of the float bar's
    windows, E32 of the all-255 window)."""
    params = g.rmbe_params()
    w = g.rmbe_net_windows()
    ref, e32 = g.rmbe_reference(params, w[g.RMBE_NET_FLOAT])
    ref255, e255 = g.rmbe_reference(params, w[g.RMBE_NET_FLAT255])
    w.setflags(write=False)
    return w, np.concatenate([ref, ref255]), e32, e255


def _net_errors(got, ref):
    d = np.abs(got.astype(np.float64) - ref)
    return float(d[g.RMBE_NET_FLOAT].max()), float(d[g.RMBE_NET_FLAT255].max())


# ---------------------------------------------------------------------------- (a) the net, per form
def test_net_forms_vs_oracle(rmbe, net_ref):
    plain, shipped, _ = rmbe
    w, ref, e32, e255 = net_ref
    lanes = (3, 2)  # five windows on two lanes
    # the direct form first: F(4x4,3x3)'s bar is stated against its error
    g.set_options(plain, **dict(UNFUSED, s1_form=0, s2_form=0))
    _assert_plan(plain, _unfused_plan(0), lanes)
    direct = plain.rmbe_windows(w)
    err_direct, err_direct255 = _net_errors(direct, ref)
    print(f"\nrmbe net: E32 {e32:.3e} (all-255 window {e255:.3e}); direct {err_direct:.3e} ({err_direct / e32:.2f} E32), "
          f"all-255 {err_direct255:.3e} ({err_direct255 / e255:.2f} E32)")
    assert err_direct <= g.float_bar(e32), (err_direct, e32)
    assert err_direct255 <= g.float_bar(e255), (err_direct255, e255)
    chain = [r"conv_rgb_s2_kernel<32,\d+,false>", r"conv3x3<1,32,64,", None, r"$", r"conv3x3<2,64,32,",
             r"convT_rgb_valu_kernel<32,\d+>"]
    cases = [("unfused F(2x2,3x3)", plain, dict(UNFUSED, s1_form=1, s2_form=0), _unfused_plan(1), False),
             ("unfused F(4x4,3x3)", plain, dict(UNFUSED, s1_form=2, s2_form=0), _unfused_plan(2), True)]
    for wh in (1, 2):
        plan = list(chain)
        plan[2] = rf"wino_chain_kernel<0,0,{wh},0>$"
        cases.append((f"chain wh {wh}", plain, dict(UNFUSED, chain=1, chain_wh=wh, s1_form=1, s2_form=0), plan, False))
    fused = FUSED_HEAD + [S1_KERNEL[2], S1_KERNEL[2]] + FUSED_TAIL
    cases.append(("default options", plain, {}, fused, True))
    cases.append(("shipped state", shipped, None, fused, True))
    same_form = {}
    try:
        for tag, c, opts, plan, wino4 in cases:
            if opts is not None:  # the shipped handle runs as the product made it
                g.set_options(c, **opts)
            _assert_plan(c, plan, lanes)
            got = c.rmbe_windows(w)
            assert not np.isnan(got).any(), tag
            err, err255 = _net_errors(got, ref)
            bar = g.wino4_float_bar(err_direct) if wino4 else g.float_bar(e32)
            bar255 = g.wino4_float_bar(err_direct255) if wino4 else g.float_bar(e255)
            print(f"  {tag}: {err:.3e} ({err / e32:.2f} E32) bar {bar:.3e}; all-255 {err255:.3e} "
                  f"({err255 / e255:.2f} E32) bar {bar255:.3e}")
            assert err <= bar, (tag, err, e32, bar)
            assert err255 <= bar255, (tag, err255, e255, bar255)
            # within a form every fusion is bit-identical: chain == unfused F(2x2,3x3); default
            # options == shipped state == unfused F(4x4,3x3)
            key = "F(4x4,3x3)" if wino4 else "F(2x2,3x3)"
            if key in same_form:
                assert np.array_equal(got, same_form[key][1]), (tag, same_form[key][0])
            else:
                same_form[key] = (tag, got)
    finally:
        g.set_options(plain)


# ---------------------------------------------------------------------------- (b) variants
def test_net_head_tail_and_last_layer_variants(rmbe, net_ref, monkeypatch):
    """Every TIC_ENC01_VARIANT, TIC_DEC10_VARIANT and TIC_RGB_OUT_TILE the rmbe handle accepts
    (f32 input into the head, f32 output from the tail and the last layer) against the unfused run
    of the default form, each launch asserted by name."""
    plain, _, _ = rmbe
    w = net_ref[0]
    lanes = (3, 2)
    try:
        g.set_options(plain, **UNFUSED)
        _assert_plan(plain, _unfused_plan(2), lanes)
        ref = plain.rmbe_windows(w)
        assert not np.isnan(ref).any()
        g.set_options(plain, **dict(UNFUSED, fuse01=1))
        names = set()
        for v in g.ENC01_VARIANTS:
            monkeypatch.setenv("TIC_ENC01_VARIANT", str(v))
            _assert_plan(plain, FUSED_HEAD + _unfused_plan(2)[2:], lanes)
            names.add(plain.layer_kernels(3)[0])
            assert np.array_equal(plain.rmbe_windows(w), ref), v
        assert len(names) == len(g.ENC01_VARIANTS), names
        monkeypatch.delenv("TIC_ENC01_VARIANT")
        g.set_options(plain, **dict(UNFUSED, fuse_tail=1))
        names = set()
        for v in g.DEC10_VARIANTS:
            monkeypatch.setenv("TIC_DEC10_VARIANT", str(v))
            _assert_plan(plain, _unfused_plan(2)[:4] + FUSED_TAIL, lanes)
            names.add(plain.layer_kernels(3)[L - 2])
            assert np.array_equal(plain.rmbe_windows(w), ref), v
        assert len(names) == len(g.DEC10_VARIANTS), names
        monkeypatch.delenv("TIC_DEC10_VARIANT")
        g.set_options(plain, **UNFUSED)
        names = set()
        for t in g.RGB_OUT_TILES:
            monkeypatch.setenv("TIC_RGB_OUT_TILE", str(t))
            kern = plain.layer_kernels(3)
            assert re.fullmatch(r"convT_rgb_valu(_persist)?_kernel<32,\d+>", kern[L - 1]), kern
            persistent = t >= g.RGB_OUT_PERSISTENT_FROM
            assert ("_persist" in kern[L - 1]) == persistent, kern
            names.add(kern[L - 1])
            for grid in ((0, 7) if persistent else (0,)):  # 7: several tiles per workgroup
                plain.set_option("persist_grid", grid)
                got = plain.rmbe_windows(w)
                plain.set_option("persist_grid", 0)
                assert np.array_equal(got, ref), (t, grid)
        assert len(names) == len(g.RGB_OUT_TILES), names
    finally:
        g.set_options(plain)


# ---------------------------------------------------------------------------- (c), (d) whole images
SIZES = list(g.RMBE_IMAGES)
SIZE_IDS = [f"{H}x{W}" for H, W in SIZES]
TAIL = 4096  # floats behind the image that no run may write


def _run_image(c, img, chunk, streams):
    H, W, _ = img.shape
    c.set_option("chunk", chunk)
    c.set_option("streams", streams)
    d = c.alloc((img.size + TAIL) * 4)
    try:
        d.upload(np.concatenate([img.reshape(-1), np.full(TAIL, SENTINEL, np.float32)]))
        c.rmbe_image_device(d, H, W)
        c.synchronize()
        got = d.download((img.size + TAIL,), np.float32)
    finally:
        d.free()
        c.set_option("chunk", 256)
        c.set_option("streams", 2)
    assert np.all(got[img.size:] == SENTINEL)
    return got[:img.size].reshape(img.shape)


@pytest.fixture(scope="module")
def image_cases(rmbe):
    """Per (H, W), computed once and shared by (c) and (d): the image, the oracle and its two-pass
    E32, the direct form's result at chunk 256 on two lanes and its error."""
    plain, _, params = rmbe
    cache = {}

    def get(H, W):
        if (H, W) not in cache:
            img = g.rmbe_image(H, W)
            ref, e32 = g.rmbe_image_reference(params, img)
            g.set_options(plain, **dict(UNFUSED, s1_form=0, s2_form=0))
            try:
                direct = _run_image(plain, img, 256, 2)
            finally:
                g.set_options(plain)
            err = float(np.max(np.abs(direct.astype(np.float64) - ref)))
            for a in (img, ref, direct):
                a.setflags(write=False)
            cache[(H, W)] = (img, ref, e32, direct, err)
        return cache[(H, W)]

    return get


def _check_image(tag, got, img, ref, bar, H, W):
    cov = g.rmbe_covered(H, W)
    assert not np.isnan(got).any(), tag
    assert np.array_equal(got[~cov], img[~cov]), tag  # what the oracle leaves unchanged
    err = float(np.max(np.abs(got.astype(np.float64) - ref)))
    assert err <= bar, (tag, err, bar)
    return err


@pytest.mark.parametrize("H,W", SIZES, ids=SIZE_IDS)
def test_image_two_passes_vs_oracle(rmbe, image_cases, H, W):
    plain, shipped, _ = rmbe
    img, ref, e32, direct, err_direct = image_cases(H, W)
    counts = g.rmbe_window_counts(H, W)
    assert [a * b for a, b in counts] == [a * b for a, b in g.RMBE_IMAGES[(H, W)]]
    nwin = sum(a * b for a, b in counts)
    print(f"\nrmbe image {H}x{W}: windows {counts} E32 {e32:.3e} direct {err_direct:.3e}"
          + (f" ({err_direct / e32:.2f} E32)" if nwin else ""))
    if nwin == 0:
        # no window in either pass: no launch, nothing gathered, nothing written back
        assert e32 == 0 and np.array_equal(ref, img)
    for form, c, opts in (("direct", plain, dict(UNFUSED, s1_form=0, s2_form=0)), ("shipped", shipped, None)):
        if opts is not None:
            g.set_options(c, **opts)
        try:
            if form == "shipped":
                assert any("wino4" in k for k in c.layer_kernels(2))
            bar = g.float_bar(e32) if form == "direct" else g.wino4_float_bar(err_direct)
            first = None
            for chunk in (256, 4):
                for streams in (2, 1):
                    got = _run_image(c, img, chunk, streams)
                    if nwin == 0:
                        assert np.array_equal(got, img), (form, chunk, streams)
                        continue
                    err = _check_image((form, chunk, streams), got, img, ref, bar, H, W)
                    if first is None:
                        first = got
                        print(f"  {form}: {err:.3e} ({err / e32:.2f} E32) bar {bar:.3e}")
                        if form == "direct":
                            assert np.array_equal(got, direct)
                    else:
                        assert np.array_equal(got, first), (form, chunk, streams)
        finally:
            if opts is not None:
                g.set_options(c)


def test_images_in_one_arena_vs_oracle(rmbe, image_cases):
    """tic_rmbe_images_device on the seven images in one arena with gaps, chunk 4: 15 windows in
    pass 1 and 15 in pass 2, cut inside images; the shipped state at its bar per image, and
    bit-identical to tic_rmbe_image_device of each image alone."""
    _, shipped, _ = rmbe
    cases = [image_cases(H, W) for H, W in SIZES]
    offs, end = [], 5
    for H, W in SIZES:
        offs.append(end)
        end += H * W * 3 + 3
    arena = np.full(end, SENTINEL, np.float32)
    inside = np.zeros(end, bool)
    for (img, *_), off in zip(cases, offs):
        arena[off:off + img.size] = img.reshape(-1)
        inside[off:off + img.size] = True
    shipped.set_option("chunk", 4)
    d = shipped.alloc(end * 4)
    try:
        d.upload(arena)
        shipped.rmbe_images_device(d, offs, SIZES)
        shipped.synchronize()
        got = d.download((end,), np.float32)
    finally:
        d.free()
        shipped.set_option("chunk", 256)
    assert np.all(got[~inside] == SENTINEL)
    for (H, W), (img, ref, e32, _, err_direct), off in zip(SIZES, cases, offs):
        out = got[off:off + img.size].reshape(img.shape)
        if sum(a * b for a, b in g.rmbe_window_counts(H, W)) == 0:
            assert np.array_equal(out, img), (H, W)
            continue
        err = _check_image(("arena", H, W), out, img, ref, g.wino4_float_bar(err_direct), H, W)
        print(f"\nrmbe arena {H}x{W}: {err:.3e} ({err / e32:.2f} E32)")
        assert np.array_equal(out, _run_image(shipped, img, 256, 2)), (H, W)

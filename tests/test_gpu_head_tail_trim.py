"""The fused encoder head (enc01_kernel) and decoder tail (dec10_kernel) after their address,
byte-packing and staging work was trimmed: still bit-identical to the unfused kernels at the
smallest shapes that reach every staging and store path, and the byte conversion of the last
layer (shared by the fused and the unfused form, so the first check cannot see it) still rounds
half to even like np.around: at P = 128 through the 16-byte chunk path (one v_cvt_pk_u8_f32 per
byte), at P = 16 through the element-wise path (rintf) — and likewise in the last layer's two
MFMA forms (scatter, dense) and for model_2 / model_3, whose last layer is decode_1.

Shapes (model_0, tiles of 64 x 16 RGB pixels per enc01 workgroup at TH1 = 4, 16 x 64 output
pixels per dec10 workgroup at TA = 4):
* P = 16: one workgroup holds all four image borders, a partial tile in both directions;
* P = 80: a full tile plus a partial one each way, no interior tile;
* P = 208: the smallest size with an interior u8 tile beside partial ones;
* model_1 at P = 32: the 16-channel head / tail instances.
3 patches on two lanes: one launch with image indices 0 and 1, one with a single image."""
import numpy as np
import pytest

from conftest import structured_patches
from gpu_checks import poisoned

pytestmark = pytest.mark.gpu

SHAPES = [(0, 16), (0, 80), (0, 208), (1, 32)]


@pytest.fixture(scope="module")
def lib_codec():
    from tf_image_compression_amd.codec import Codec
    from tf_image_compression_amd.weights import synthetic_params, SYNTH_MEAN, SYNTH_STD
    cache = {}

    def get(model_id, P):
        if (model_id, P) not in cache:
            c = poisoned(Codec(model_id, synthetic_params(model_id, seed=0), SYNTH_MEAN, SYNTH_STD, patch_size=P))
            c.set_option("streams", 2)
            cache[model_id, P] = c
        return cache[model_id, P]

    yield get
    for c in cache.values():
        c.close()


@pytest.mark.parametrize("model_id,P", SHAPES)
def test_head_equals_unfused(lib_codec, monkeypatch, model_id, P):
    """Every TIC_ENC01_VARIANT with fuse01 = 1 == fuse01 = 0, pre-activations and symbols."""
    codec = lib_codec(model_id, P)
    x = structured_patches(3, P, seed=150 + model_id + P)
    try:
        codec.set_option("fuse01", 0)
        idx0, pre0 = codec.encode(x, return_preact=True)
        codec.set_option("fuse01", 1)
        for v in range(5):
            monkeypatch.setenv("TIC_ENC01_VARIANT", str(v))
            idx1, pre1 = codec.encode(x, return_preact=True)
            assert np.array_equal(pre0, pre1) and np.array_equal(idx0, idx1), v
    finally:
        codec.set_option("fuse01", -1)


@pytest.mark.parametrize("model_id,P", SHAPES)
def test_tail_equals_unfused(lib_codec, monkeypatch, model_id, P):
    """Every TIC_DEC10_VARIANT with fuse_tail = 1 == fuse_tail = 0, bytes and floats."""
    codec = lib_codec(model_id, P)
    idx = codec.encode(structured_patches(3, P, seed=180 + model_id + P))
    try:
        codec.set_option("fuse_tail", 0)
        u0, f0 = codec.decode(idx, return_float=True)
        codec.set_option("fuse_tail", 1)
        outs = []
        for v in range(16):
            monkeypatch.setenv("TIC_DEC10_VARIANT", str(v))
            outs.append(codec.decode(idx, return_float=True))
    finally:
        codec.set_option("fuse_tail", -1)
    for v, (u1, f1) in enumerate(outs):
        assert np.array_equal(u0, u1) and np.array_equal(f0, f1), v


# P = 16: the output is 16 pixels wide, narrower than any tile (64 output pixels for dec10,
# 32 to 128 for the unfused VALU form), so rgb_out_store writes element-wise with rintf.
# P = 128: the output is 128 pixels wide — whole tiles in every tiling of both forms, rows of
# 384 bytes — so every byte goes through the 16-byte chunk path and its v_cvt_pk_u8_f32.
@pytest.mark.parametrize("P", [16, 128])
@pytest.mark.parametrize("bias,want", [((0.0, 1.0, 254.0), (0, 2, 254)),        # ties: 0.5, 1.5, 254.5
                                       ((-3.0, 300.0, 127.25), (0, 255, 128))])  # clip ends, a non-tie
def test_byte_rounding_is_half_to_even(bias, want, P):
    """decode_0 with zero weights, std = 1, mean = 0.5: every output is bias + 0.5 exactly (then
    clipped to [0, 255]); the bytes are np.rint of the floats, ties to even — in the unfused
    form (convT_rgb_valu_kernel) and the fused one (dec10_kernel)."""
    _check_byte_rounding(0, "decode_0", bias, want, P, "convT_rgb_valu")


def _check_byte_rounding(model_id, last, bias, want, P, kernel):
    from tf_image_compression_amd.codec import Codec
    from tf_image_compression_amd.weights import synthetic_params
    params = dict(synthetic_params(model_id, seed=0))
    params[f"{last}/kernel"] = np.zeros_like(params[f"{last}/kernel"])
    params[f"{last}/bias"] = np.asarray(bias, np.float32)
    with poisoned(Codec(model_id, params, [0.5, 0.5, 0.5], [1.0, 1.0, 1.0], patch_size=P)) as c:
        assert c.layers()[-1][0] == last
        idx = c.encode(structured_patches(3, P, seed=7))
        try:
            for fuse in (0, 1):
                c.set_option("fuse_tail", fuse)
                if fuse == 0:
                    assert all(c.layer_kernels(n)[-1].startswith(kernel) for n in (2, 1)), c.layer_kernels(2)
                u, f = c.decode(idx, return_float=True)
                expect = np.clip(np.asarray(bias, np.float32) + np.float32(0.5), 0, 255)
                assert np.array_equal(f, np.broadcast_to(expect, f.shape)), fuse
                assert np.array_equal(u, np.rint(f).astype(np.uint8)), fuse
                assert np.array_equal(u, np.broadcast_to(np.asarray(want, np.uint8), u.shape)), fuse
        finally:
            c.set_option("fuse_tail", -1)


# The MFMA forms of the last layer (TIC_RGB_OUT_FORM; the fused tail only exists beside the
# VALU form, so both passes run them unfused): scatter (convT_rgb_scatter_kernel, the col2im
# store's rintf) and dense (convT_rgb_kernel, the sub-pixel store's rintf).  And model_2 /
# model_3, whose last layer is decode_1 (32 -> 3 as model_0's decode_0, behind a 64 -> 32
# decode_2): P = 32 is narrower than any tile of either form, P = 128 is whole tiles in all.
@pytest.mark.parametrize("model_id,form,P", [(0, "scatter", 16), (0, "scatter", 128), (0, "dense", 16),
                                             (0, "dense", 128), (2, None, 32), (2, None, 128), (3, None, 32),
                                             (3, None, 128), (2, "scatter", 32), (3, "dense", 128)])
@pytest.mark.parametrize("bias,want", [((0.0, 1.0, 254.0), (0, 2, 254)), ((-3.0, 300.0, 127.25), (0, 255, 128))])
def test_byte_rounding_forms_and_models(monkeypatch, bias, want, model_id, form, P):
    """test_byte_rounding_is_half_to_even for the other byte stores of the last layer."""
    if form:
        monkeypatch.setenv("TIC_RGB_OUT_FORM", form)
    kernel = {None: "convT_rgb_valu", "scatter": "convT_rgb_scatter_kernel<", "dense": "convT_rgb_kernel<"}[form]
    _check_byte_rounding(model_id, "decode_0" if model_id == 0 else "decode_1", bias, want, P, kernel)

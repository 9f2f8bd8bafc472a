"""The quantiser round_half_even(sigmoid(x) * (Q-1)) (quant1, csrc/conv3x3.h; the reference's
model_0/model.py:136-138, tf.round = half to even) on its own, in every epilogue it is inlined
into: direct stride-1 / stride-2 (conv3x3.h), Winograd F(2x2,3x3) (conv3x3_wino.h), F(4x4,3x3)
(conv3x3_wino4.h), polyphase (conv3x3_pwino.h), the chain's last layer and the joined launch's
junction (wino_chain.h).

1. Exact vectors.  The encoder's last layer gets a zero kernel and a chosen bias b, so every
   pre-activation is b[c] exactly in every form; the symbols must be the f64 oracle's of b, which
   are unambiguous: b holds the exact tie (+-0), the clamp and expf-overflow values, and points a
   quarter level from the thresholds of levels spread over the whole range
   (gpu_checks.quant_bias_vector; margins asserted in test_parity_inputs_host.py).  Neighbouring
   channels hold different symbols, so a permuted lane or byte of the packed store fails.
2. The whole level range on real convolution output: model_0 with its last encoder layer's
   gain at 4 (and model_3 as it is) reaches all 256 levels at Q = 256; besides check_codec's
   bars the symbols must be rint(sigmoid_f64(pre) * 255) of the GPU's own returned
   pre-activation wherever that is farther than 8 * 2^-24 * 255 levels from a threshold, which
   separates the quantiser's arithmetic from the convolution's error.

3 patches on two lanes (launches of 2 and 1).  Which kernel ran is read from tic_layer_kernel /
tic_codec_kernel, never trusted to the option."""
import re

import numpy as np
import pytest

from conftest import structured_patches
import gpu_checks as g
from test_gpu_parity import TILES

pytestmark = pytest.mark.gpu

N = 3
LANE_BATCHES = (2, 1)
JOINED = re.compile(r"wino_chain_kernel<0,1,2,(\d+)>")


@pytest.fixture(scope="module")
def handles():
    """Codec handles per (model, P, Q, params tag): creating one dominates a test's time."""
    from tf_image_compression_amd.codec import Codec
    cache = {}

    def get(model_id, P, Q, tag, make_params):
        key = (model_id, P, Q, tag)
        if key not in cache:
            params = make_params()
            c = Codec(model_id, params, g.codec_mean(), g.codec_std(), patch_size=P, quan_scale=Q)
            cache[key] = (g.poisoned(c), params)
        return cache[key]

    yield get
    for c, _ in cache.values():
        c.close()


def _vector_codec(handles, model_id, P, Q):
    eh_c = 80 if model_id == 3 else 64
    b, _ = g.quant_bias_vector(Q, eh_c)
    c, _ = handles(model_id, P, Q, "vector", lambda: g.quantiser_params(model_id, b))
    assert c.code_shape[2] == eh_c
    return c, b, g.quantize_f64(b, Q)


def _check_exact(c, x, b, want, what):
    idx, pre = c.encode(x, return_preact=True)
    assert np.array_equal(pre, np.broadcast_to(b, pre.shape)), what
    bad = np.argwhere(idx != np.broadcast_to(want, idx.shape))
    assert bad.size == 0, (what, len(bad), [(tuple(i), float(b[i[3]]), int(idx[tuple(i)]), int(want[i[3]]))
                                            for i in bad[:8]])


def _enc_kernels(c, codec_step=False):
    last = g.layer_index(c, g.last_encoder_layer(c.model_id))
    return [g.launched_kernel(c, last, n, codec_step) for n in LANE_BATCHES]


def _expect_kernel(c, pattern):
    for k in _enc_kernels(c):
        assert re.fullmatch(pattern, k), (k, pattern)


def _direct(c, x, b, want, monkeypatch, mode, cin, cout, **opts):
    """The direct form as the planner picks it, then every compiled tiling of TILES forced."""
    from tf_image_compression_amd._lib import TicError
    pattern = rf"conv3x3<{mode},{cin},{cout},(\d+),\d+,(\d+),(\d+),0,false,0,1>"
    g.set_options(c, **opts)
    _expect_kernel(c, pattern)
    _check_exact(c, x, b, want, ("direct", opts))
    ran = 0
    for tile in TILES:
        monkeypatch.setenv("TIC_FORCE_TILE", "%d,%d,%d" % tile)
        try:
            kern = _enc_kernels(c)
        except TicError as e:
            assert "no compiled" in str(e)
            continue
        for k in kern:
            m = re.fullmatch(pattern, k)
            assert m and tuple(int(v) for v in m.groups()) == tile, (k, tile)
        _check_exact(c, x, b, want, ("direct", opts, tile))
        ran += 1
    monkeypatch.delenv("TIC_FORCE_TILE")
    assert ran >= 1, "no forced tiling ran"


def _joined(c, x, want):
    """codec_device with the two chain launches (chain_j 0) and with the joined one: the symbols,
    and the bytes against decode() of those symbols on the unfused path — the junction hands the
    decoder what its LDS copy of the dequantiser table holds."""
    lane_batches = sorted({-(-len(x) // 2), len(x) // 2} - {0}, reverse=True)
    for j in (0, 1):
        g.set_options(c, s1_form=1, chain=1, chain_wh=2, chain_x=2, chain_j=j)
        last = g.layer_index(c, g.last_encoder_layer(c.model_id))
        for n in lane_batches:
            m = JOINED.fullmatch(g.launched_kernel(c, last, n, codec_step=True))
            assert m and bool(int(m[1]) & 16) == bool(j) and int(m[1]) & 1, (j, n, c.codec_kernels(n))
        idx, rgb = g.device_codec(c, x)
        assert np.array_equal(idx, np.broadcast_to(want, idx.shape)), j
        g.set_options(c, s1_form=1, chain=0)
        assert not any("wino_chain" in k for k in c.layer_kernels(lane_batches[0]))
        assert np.array_equal(rgb, c.decode(idx)), j


@pytest.mark.parametrize("Q", g.QUANT_QS)
@pytest.mark.parametrize("model_id,P", [(0, 64), (1, 32)])
def test_exact_vectors_stride1(handles, monkeypatch, model_id, P, Q):
    """encode_4 of model_0 / model_1 (64 -> 64, stride 1): direct in every tiling, F(2x2,3x3),
    F(4x4,3x3), the chain's last layer in every chain shape, the joined launch's junction."""
    c, b, want = _vector_codec(handles, model_id, P, Q)
    x = structured_patches(N, P, seed=300 + model_id)
    _direct(c, x, b, want, monkeypatch, 0, 64, 64, s1_form=0)
    g.set_options(c, s1_form=1)
    _expect_kernel(c, r"conv3x3_wino_kernel<64,64,\d+,\d+,\d+,0,false,0,1>")
    _check_exact(c, x, b, want, "F(2x2,3x3)")
    g.set_options(c, s1_form=2)
    _expect_kernel(c, r"conv3x3_wino4_kernel<64,64,\d+,0,false,0,1>")
    _check_exact(c, x, b, want, "F(4x4,3x3)")
    for chain_x in (0, 1, 2):
        for wh in (1, 2):
            g.set_options(c, s1_form=1, chain=1, chain_x=chain_x, chain_wh=wh)
            head = 1 if chain_x and wh == 2 else 0  # the stride-2 head needs the 512-thread workgroup
            _expect_kernel(c, rf"wino_chain_kernel<0,1,{wh},{head}>")
            _check_exact(c, x, b, want, ("chain", chain_x, wh))
    _joined(c, x, want)


@pytest.mark.parametrize("Q", [2, 256])
def test_exact_vectors_joined_launch_2x2_regions(handles, Q):
    """The junction at model_0's 256 x 256 patches: 2 x 2 regions that hand borders to each other."""
    c, b, want = _vector_codec(handles, 0, 256, Q)
    _joined(c, structured_patches(2, 256, seed=310), want)


@pytest.mark.parametrize("Q", g.QUANT_QS)
def test_exact_vectors_stride2(handles, monkeypatch, Q):
    """encode_4 of model_2 (64 -> 64, stride 2): direct in every tiling, and polyphase."""
    c, b, want = _vector_codec(handles, 2, 32, Q)
    x = structured_patches(N, 32, seed=302)
    _direct(c, x, b, want, monkeypatch, 1, 64, 64, s2_form=0)
    g.set_options(c, s2_form=1)
    _expect_kernel(c, r"conv3x3_pwino_kernel<1,64,64,\d+,0,false,0,1>")
    _check_exact(c, x, b, want, "polyphase")


@pytest.mark.parametrize("Q", g.QUANT_QS)
def test_exact_vectors_80_channels(handles, monkeypatch, Q):
    """encode_4 of model_3 (64 -> 80, stride 2): 20 packed stores per pixel, direct form only."""
    c, b, want = _vector_codec(handles, 3, 64, Q)
    _direct(c, structured_patches(N, 64, seed=303), b, want, monkeypatch, 1, 64, 80)


@pytest.mark.parametrize("Q", g.QUANT_QS)
def test_exact_vectors_ch128(handles, monkeypatch, Q):
    """encode_3 of base_model/ch_128 (128 -> 64, stride 1): direct in every tiling, F(2x2,3x3)."""
    c, b, want = _vector_codec(handles, 128, 64, Q)
    x = structured_patches(N, 64, seed=304)
    _direct(c, x, b, want, monkeypatch, 0, 128, 64, s1_form=0)
    g.set_options(c, s1_form=1)
    _expect_kernel(c, r"conv3x3_wino_kernel<128,64,\d+,\d+,\d+,0,false,0,1>")
    _check_exact(c, x, b, want, "F(2x2,3x3)")


def _check_rule(idx, pre, Q, what):
    """idx == rint(sigmoid_f64(pre) * (Q-1)) wherever the f32 arithmetic cannot decide otherwise."""
    assert np.all(np.isfinite(pre)), what
    t, safe = g.quant_rule_excluded(pre, Q)
    assert float(np.mean(~safe)) <= 1e-3, what
    bad = np.argwhere((idx != np.rint(t)) & safe)
    assert bad.size == 0, (what, len(bad), [(float(pre[tuple(i)]), int(idx[tuple(i)])) for i in bad[:8]])
    assert set(idx.ravel().tolist()) == set(range(Q)), what


@pytest.mark.parametrize("model_id,gain", [(0, 4.0), (3, 1.0)])
def test_whole_level_range(handles, model_id, gain):
    """All 256 levels on real convolution output, every stride-1 form unchained, the chain and
    (model_0) the joined launch."""
    P, Q = 64, 256
    c, params = handles(model_id, P, Q, ("gain", gain), lambda: g.gained_params(model_id, gain))
    x = structured_patches(4, P, seed=5)
    paths = [dict(s1_form=0), dict(s1_form=1), dict(s1_form=2), dict(s1_form=1, chain=1, chain_x=2)]
    last = g.layer_index(c, g.last_encoder_layer(model_id))
    for opts in paths:
        g.set_options(c, **opts)
        k = g.launched_kernel(c, last, 2)
        if model_id == 0 and "chain" in opts:
            assert k == "wino_chain_kernel<0,1,2,1>", k
        elif model_id == 0:
            want = ("conv3x3<0,64,64,", "conv3x3_wino_kernel<64,64,", "conv3x3_wino4_kernel<64,64,")[opts["s1_form"]]
            assert k.startswith(want) and k.endswith(",0,1>"), (k, opts)
        else:
            assert k.startswith("conv3x3<1,64,80,") and k.endswith(",0,1>"), (k, opts)
        idx, _ = g.check_codec(c, params, model_id, P, x, Q=Q)
        idx2, pre = c.encode(x, return_preact=True)
        assert np.array_equal(idx, idx2)
        _check_rule(idx, pre, Q, opts)
    if model_id == 0:
        chain_idx, chain_pre = idx, pre
        g.set_options(c, s1_form=1, chain=1, chain_x=2, chain_j=1)
        m = JOINED.fullmatch(g.launched_kernel(c, last, 2, codec_step=True))
        assert m and int(m[1]) & 16, c.codec_kernels(2)
        idx, rgb = g.device_codec(c, x)
        _check_rule(idx, chain_pre, Q, "joined")
        assert np.array_equal(idx, chain_idx)
        g.set_options(c, s1_form=1, chain=0)  # the unfused path just held to check_codec's bars
        assert np.array_equal(rgb, c.decode(idx))

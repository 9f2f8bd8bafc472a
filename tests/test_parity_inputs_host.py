"""The input conditions the GPU tests of the quantiser, the dequantiser and the unclipped
decoder rely on (test_gpu_quantiser.py, test_gpu_dequantiser.py), asserted on the CPU with the
oracle alone: a later change of synthetic_params or structured_patches must not silently empty
those tests; likewise for the geometry sweep (test_gpu_geometry.py), for exactly its patches.
Reference: the quantiser round(sigmoid(x) * (Q-1)) of model_0/model.py:136-138
(tf.round: half to even), the dequantiser :148-155, denormalise + clip :250-259."""
import numpy as np
import pytest

from conftest import structured_patches
import gpu_checks as g
from oracle import tic_oracle as o


@pytest.mark.parametrize("cout", [64, 80])
@pytest.mark.parametrize("Q", g.QUANT_QS)
def test_quantiser_bias_vectors(Q, cout):
    b, tie = g.quant_bias_vector(Q, cout)
    assert b.dtype == np.float32 and b.shape == (cout,)
    t = g.quant_level_f64(b, Q)
    sym = g.quantize_f64(b, Q)
    # every value but the tie itself sits more than 0.2 level from every rounding threshold, so
    # the f32 sigmoid (a few 2^-24 (Q-1) levels of error, < 1e-4 level at Q = 256) cannot move it
    assert np.all(g.half_margin(t[~tie]) > 0.2)
    # the tie: +0 and -0, level (Q-1)/2 exactly, rounded half to even
    assert np.count_nonzero(tie) >= 2 and np.any(np.signbit(b[tie])) and not np.all(np.signbit(b[tie]))
    assert np.all(t[tie] == (Q - 1) / 2)
    want = {2: 0, 3: 1, 4: 2, 6: 2, 16: 8, 255: 127, 256: 128}[Q]
    assert np.all(sym[tie] == want)
    # the clamp and the overflow values, both signs
    for v in g.QUANT_EXTREMES:
        assert np.all(sym[b == np.float32(v)] == Q - 1) and np.any(b == np.float32(v))
        assert np.all(sym[b == np.float32(-v)] == 0) and np.any(b == np.float32(-v))
    # the lowest and the highest threshold from both sides, and every level in between for small Q
    assert {0, 1, Q - 2, Q - 1} <= set(sym.tolist())
    if Q <= 16:
        assert set(sym.tolist()) == set(range(Q))
    # neighbouring channels differ wherever the symbols allow it, and no packed u32 (four
    # consecutive channels) holds one symbol only
    same = np.count_nonzero(sym[1:] == sym[:-1])
    assert same == 0 if Q >= 3 else same <= cout // 8
    groups = [len(set(sym[i:i + 4].tolist())) for i in range(0, cout, 4)]
    assert min(groups) >= 2 and (Q < 16 or min(groups) >= 3)


GAIN_CASES = [(0, 4.0), (3, 1.0)]  # (model, gain of the last encoder layer)


@pytest.mark.parametrize("model_id,gain", GAIN_CASES)
def test_all_256_levels_reached(model_id, gain):
    P, Q = 64, 256
    params = g.gained_params(model_id, gain)
    pre, idx = o.encoder(params, g.codec_mean(), g.codec_std(), structured_patches(4, P, seed=5), P, Q, model_id)
    assert set(idx.ravel().tolist()) == set(range(256))
    assert float(np.abs(pre).max()) > 16  # the saturated ends are reached with room
    _, safe = g.quant_rule_excluded(pre, Q)
    assert float(np.mean(~safe)) <= 1e-3


@pytest.mark.parametrize("model_id,P", g.UNCLIPPED_CASES)
def test_unclipped_params_leave_nothing_clipped(model_id, P):
    params = g.unclipped_params(model_id)
    x = structured_patches(3, P, seed=61 + model_id)
    _, idx = o.encoder(params, g.codec_mean(), g.codec_std(), x, P, 2, model_id)
    ref_f, _ = o.decoder(params, g.codec_mean(), g.codec_std(), idx, 2, model_id)
    share, span = g.clipped_share_and_span(ref_f)
    assert share <= 0.01 and span >= 100, (share, span)


@pytest.mark.parametrize("model_id,P", g.GEOMETRY_CASES)
def test_geometry_sweep_inputs(model_id, P):
    """test_gpu_geometry.py's patches: at most 1e-3 of the symbols inside check_codec's 1e-5
    decision band (the symbol bar says nothing there), and on the unclipped parameters at most 1e-3
    of the oracle's reconstruction exactly 0 or 255 (the float and byte bars see no last layer
    there)."""
    x = g.geometry_patches(model_id, P)
    assert x.shape == (g.GEOMETRY_N, P, P, 3)
    from tf_image_compression_amd.weights import synthetic_params
    pre, idx = o.encoder(synthetic_params(model_id, seed=0), g.codec_mean(), g.codec_std(), x, P, 2, model_id)
    scale = max(1.0, float(np.max(np.abs(pre))))
    band = float(np.mean(o.decision_margin(pre, 2) <= 1e-5 * scale))
    params = g.geometry_unclipped_params(model_id, P)
    ref_f, _ = o.decoder(params, g.codec_mean(), g.codec_std(), idx, 2, model_id)
    share, span = g.clipped_share_and_span(ref_f)
    print(f"\ngeometry model {model_id} P {P}: band share {band:.2e} clipped share {share:.2e} span {span:.1f}")
    assert band <= 1e-3, band
    assert share <= 1e-3, share


# ---------------------------------------------------------------------------
# The rmbe net and the whole-image driver (test_gpu_rmbe.py, test_gpu_product.py): what the float
# bars of those tests cannot see is capped here, on the oracle alone
# (submit/2/rmbe/model.py:113-197, rmbe.py:15-111).
# ---------------------------------------------------------------------------
def test_rmbe_net_windows_inputs():
    """The structured, Gaussian and all-0 windows (the float bar's set): at most 1e-3 of the
    oracle's outputs exactly 0 or 255, E32 > 0.  The all-255 window is an input like the others but
    12.6 % of its outputs clip at 0: the GPU tests hold it to the bar of its own E32 and to bit
    identity, and it stays out of this share."""
    params = g.rmbe_params()
    w = g.rmbe_net_windows()
    assert w.shape == (5, 128, 128, 3) and w.dtype == np.float32
    assert np.all(w[3] == 0) and np.all(w[4] == 255) and w[:3].std(axis=(1, 2, 3)).min() > 10
    ref, e32 = g.rmbe_reference(params, w[g.RMBE_NET_FLOAT])
    share = g.rmbe_clipped_share(ref)
    ref255, e255 = g.rmbe_reference(params, w[g.RMBE_NET_FLAT255])
    print(f"\nrmbe net windows: E32 {e32:.3e} clipped share {share:.2e}; all-255 window: E32 {e255:.3e} "
          f"clipped share {g.rmbe_clipped_share(ref255):.2e}")
    assert share <= 1e-3, share
    assert e32 > 0 and e255 > 0
    assert float(ref.max() - ref.min()) >= 100


def test_rmbe_pass_windows_inputs():
    """The windows test_gpu_product.py compares with the oracle at the 4K image's pass sizes (the
    first two, the second chunk's first and the last two of 464 and of 480): structured and noise, nothing clipped."""
    params = g.rmbe_params()
    w = g.rmbe_pass_windows(480)
    for n in g.RMBE_4K_PASSES:
        sel = g.rmbe_pass_checked(n)
        assert sel[:2] == [0, 1] and sel[-2:] == [n - 2, n - 1] and 256 in sel
        ref, e32 = g.rmbe_reference(params, w[sel])
        share = g.rmbe_clipped_share(ref)
        print(f"\nrmbe pass of {n} windows: E32 {e32:.3e} clipped share {share:.2e}")
        assert share <= 1e-3 and e32 > 0
    # 3840 x 2160: the two pass sizes, and the handle's chunk of 256 cuts both
    assert [a * b for a, b in g.rmbe_window_counts(2160, 3840)] == list(g.RMBE_4K_PASSES) == [464, 480]


@pytest.mark.parametrize("H,W", list(g.RMBE_IMAGES), ids=[f"{H}x{W}" for H, W in g.RMBE_IMAGES])
def test_rmbe_image_inputs(H, W):
    """Every whole-image case has the window counts its comment names; among the pixels inside a
    window at most 1e-3 of the oracle's outputs are exactly 0 or 255; E32 > 0 wherever a window
    exists (191 x 191 has none: that case is bit identity with the input, not a float bar); and
    the oracle leaves every pixel outside the windows as it is."""
    want = g.RMBE_IMAGES[(H, W)]
    got = g.rmbe_window_counts(H, W)
    assert [a * b for a, b in got] == [a * b for a, b in want], (got, want)
    for (a, b), (c, d) in zip(got, want):
        assert a * b == 0 or (a, b) == (c, d)
    img = g.rmbe_image(H, W)
    assert img.shape == (H, W, 3) and img.dtype == np.float32
    ref, e32 = g.rmbe_image_reference(g.rmbe_params(), img)
    cov = g.rmbe_covered(H, W)
    share = g.rmbe_clipped_share(ref, cov)
    print(f"\nrmbe image {H}x{W}: windows {got} E32 {e32:.3e} clipped share {share:.2e}")
    assert np.array_equal(ref[~cov], img[~cov])
    if sum(a * b for a, b in got) == 0:
        assert not cov.any() and np.array_equal(ref, img)
        return
    assert share <= 1e-3, share
    assert e32 > 0
    assert float(np.mean(ref[cov] != img[cov])) > 0.99  # the filter does change what it covers

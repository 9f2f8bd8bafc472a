"""Shared GPU parity checks (imported by the -m gpu test modules; not a test module).

The bars are DESIGN.md §4's: pre-activations within 1e-4 relative of the oracle, symbols
bit-exact outside the 1e-5 decision band, decoder float within 1e-2 on the [0,255]
scale when fed the same symbols, uint8 within 1 and only on .5 rounding edges, dataset
PSNR within 0.02 dB (north_star tolerance)."""
import numpy as np

from oracle import tic_oracle as o


def check_codec(codec, params, model_id, P, patches, Q=2):
    idx, pre = codec.encode(patches, return_preact=True)
    ref_pre, ref_idx = o.encoder(params, codec_mean(), codec_std(), patches, P, Q, model_id)
    scale = max(1.0, float(np.max(np.abs(ref_pre))))
    assert pre.shape == ref_pre.shape and idx.shape == ref_idx.shape
    assert float(np.max(np.abs(pre - ref_pre))) <= 1e-4 * scale
    margin = o.decision_margin(ref_pre, Q)
    safe = margin > 1e-5 * scale
    mism = int(np.count_nonzero((idx != ref_idx) & safe))
    assert mism == 0, f"{mism} symbol mismatches outside the tie band"
    # decoder on the GPU's own symbols, oracle on the same symbols
    rgb, f = codec.decode(idx, return_float=True)
    ref_f, ref_u8 = o.decoder(params, codec_mean(), codec_std(), idx, Q, model_id)
    assert float(np.max(np.abs(f - ref_f))) <= 1e-2
    du = np.abs(rgb.astype(np.int16) - ref_u8.astype(np.int16))
    assert int(du.max()) <= 1
    edge = np.abs((ref_f - np.floor(ref_f)) - 0.5) < 1e-2
    assert int(np.count_nonzero((du > 0) & ~edge)) == 0
    p_gpu = o.dataset_psnr([(patches[i], rgb[i]) for i in range(len(patches))])
    p_ref = o.dataset_psnr([(patches[i], ref_u8[i]) for i in range(len(patches))])
    assert abs(p_gpu - p_ref) <= 0.02, (p_gpu, p_ref)
    return idx, rgb


def check_codec_subset(codec, params, model_id, P, patches, k, Q=2):
    """Encode + decode ALL patches in one call each (the launch sequence of that batch
    size), check the first k against the oracle with check_codec's bars; returns the full
    symbols and bytes."""
    idx, pre = codec.encode(patches, return_preact=True)
    rgb, f = codec.decode(idx, return_float=True)
    sub = patches[:k]
    ref_pre, ref_idx = o.encoder(params, codec_mean(), codec_std(), sub, P, Q, model_id)
    scale = max(1.0, float(np.max(np.abs(ref_pre))))
    assert float(np.max(np.abs(pre[:k] - ref_pre))) <= 1e-4 * scale
    safe = o.decision_margin(ref_pre, Q) > 1e-5 * scale
    mism = int(np.count_nonzero((idx[:k] != ref_idx) & safe))
    assert mism == 0, f"{mism} symbol mismatches outside the tie band"
    ref_f, ref_u8 = o.decoder(params, codec_mean(), codec_std(), idx[:k], Q, model_id)
    assert float(np.max(np.abs(f[:k] - ref_f))) <= 1e-2
    du = np.abs(rgb[:k].astype(np.int16) - ref_u8.astype(np.int16))
    assert int(du.max()) <= 1
    edge = np.abs((ref_f - np.floor(ref_f)) - 0.5) < 1e-2
    assert int(np.count_nonzero((du > 0) & ~edge)) == 0
    p_gpu = o.dataset_psnr([(sub[i], rgb[i]) for i in range(k)])
    p_ref = o.dataset_psnr([(sub[i], ref_u8[i]) for i in range(k)])
    assert abs(p_gpu - p_ref) <= 0.02, (p_gpu, p_ref)
    return idx, rgb


# ---------------------------------------------------------------------------
# Crafted parameters and inputs of the quantiser / dequantiser / unclipped-decoder tests
# (test_gpu_quantiser.py, test_gpu_dequantiser.py; their input conditions are asserted on the
# CPU by test_parity_inputs_host.py).  Nothing below needs a GPU.
# ---------------------------------------------------------------------------

QUANT_QS = (2, 3, 4, 6, 16, 255, 256)
# the clamp and expf's overflow: sigmoid saturates in f32 from |x| ~ 17 on, expf(x) is inf from
# x ~ 88.7 on and expf(-x) flushes to 0 from x ~ 104 on
QUANT_EXTREMES = (20.0, 88.0, 89.0, 104.0, 1e4, 3e38)


def last_encoder_layer(model_id):
    return o.MODELS[model_id][0][-1][0]


def first_decoder_layer(model_id):
    return o.MODELS[model_id][1][0][0]


def last_decoder_layer(model_id):
    return o.MODELS[model_id][1][-1][0]


def quantize_f64(x, Q):
    """oracle.quantize without the overflow warning of exp(1e4)."""
    with np.errstate(over="ignore"):
        return o.quantize(np.asarray(x, np.float64), Q)


def quant_level_f64(x, Q):
    """sigmoid(x) * (Q - 1) in float64: the real number the quantiser rounds."""
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-np.asarray(x, np.float64))) * (Q - 1)


def half_margin(t):
    """Distance of a level t from the nearest half-integer (a rounding threshold)."""
    return np.abs(t - np.floor(t) - 0.5)


def quant_bias_vector(Q, cout):
    """(b, tie): cout float32 pre-activations whose symbol is known, and which of them are the
    exact tie.  +-0 (sigmoid = 0.5 exactly, level (Q-1)/2: a tie for even Q); the clamp / overflow
    values +-QUANT_EXTREMES; and for levels k spread evenly over 0..Q-2 (k = 0 and k = Q-2
    always) the two points a quarter level inside the thresholds of k + 0.5:
    float32(logit((k + 0.5 -+ 0.25) / (Q-1))).  Ordered so that neighbouring channels have
    different symbols wherever the symbols allow it (a lane or byte permutation of the packed
    store then changes the result); a list shorter than cout repeats."""
    q1 = Q - 1
    vals = [0.0, -0.0]
    for v in QUANT_EXTREMES:
        vals += [v, -v]
    nk = max(1, min(q1, (cout - len(vals)) // 2))
    for k in sorted({int(round(k)) for k in np.linspace(0, Q - 2, nk)}):
        for d in (0.25, 0.75):
            p = (k + d) / q1
            vals.append(float(np.float32(np.log(p / (1.0 - p)))))
    vals = np.asarray(vals, np.float32)
    sym = quantize_f64(vals, Q)
    order, rest = [], list(range(len(vals)))
    while rest:
        recent = [sym[i] for i in order[-3:]]
        pick = next((i for i in rest if sym[i] not in recent), None)
        if pick is None:
            pick = next((i for i in rest if not order or sym[i] != sym[order[-1]]), rest[0])
        order.append(pick)
        rest.remove(pick)
    b = np.asarray([vals[order[j % len(order)]] for j in range(cout)], np.float32)
    return b, b == 0


def quantiser_params(model_id, b, seed=0):
    """synthetic params whose last encoder layer has a zero kernel and bias b: every
    pre-activation is b[c] exactly in every form (Winograd transforms of zeros are zeros)."""
    from tf_image_compression_amd.weights import synthetic_params
    params = dict(synthetic_params(model_id, seed=seed))
    name = last_encoder_layer(model_id)
    params[f"{name}/kernel"] = np.zeros_like(params[f"{name}/kernel"])
    params[f"{name}/bias"] = np.asarray(b, np.float32)
    assert params[f"{name}/bias"].shape == (params[f"{name}/kernel"].shape[3],)
    return params


def gained_params(model_id, gain, seed=0):
    """synthetic params with the last encoder layer's kernel and bias multiplied by gain (at
    gain 4, model_0's pre-activations reach every one of 256 levels)."""
    from tf_image_compression_amd.weights import synthetic_params
    params = dict(synthetic_params(model_id, seed=seed))
    name = last_encoder_layer(model_id)
    for v in ("kernel", "bias"):
        params[f"{name}/{v}"] = (params[f"{name}/{v}"] * np.float32(gain)).astype(np.float32)
    return params


# the last decoder layer's kernel gain that keeps the reconstruction inside (0, 255)
UNCLIPPED_GAIN = {0: 1 / 8, 1: 1 / 4, 2: 1 / 8, 3: 1 / 32, 128: 1 / 32}
# (model, P): every model at the smallest patch size the suite runs it at
UNCLIPPED_CASES = [(0, 64), (1, 32), (2, 32), (3, 64), (128, 64)]


def unclipped_params(model_id, seed=0, gain=None):
    """synthetic params with the last decoder layer's kernel scaled by UNCLIPPED_GAIN (bias
    unchanged; `gain`: a case's own value instead): with the plain synthetic weights up to 85 % of
    the oracle's outputs are exactly 0 or 255 and the float and byte bars see nothing of the last
    layers there."""
    from tf_image_compression_amd.weights import synthetic_params
    params = dict(synthetic_params(model_id, seed=seed))
    name = last_decoder_layer(model_id)
    gain = UNCLIPPED_GAIN[model_id] if gain is None else gain
    params[f"{name}/kernel"] = (params[f"{name}/kernel"] * np.float32(gain)).astype(np.float32)
    return params


# ---------------------------------------------------------------------------
# The geometry sweep (test_gpu_geometry.py; input conditions: test_parity_inputs_host.py).
# (model, P): the chain's 8x8 regions at stage sides the other modules never compare with
# anything — model_0/1 stage P/16: 1, 2, 5, 7 (one partial region, odd Winograd half tiles), 8
# (exactly one full region), 9 = 8 + 1 (a 1-wide partial region whose only column is its hand-off
# column), 10 = 8 + 2, 15, 17 = 8 + 8 + 1; model_2 stage P/8 (2, 6, 10, 18) with the stride-2
# quantiser layer behind it; model_3 stages P/4 and P/8 (4/2, 12/6, 20/10, 36/18); ch_128 stage
# P/4 at the odd sides 5, 7, 9 of its 128-wide Winograd, transposed and stride-2 instances.
# ---------------------------------------------------------------------------
GEOMETRY_CASES = ([(0, P) for P in (16, 32, 80, 112, 128, 144, 160, 240, 272)] + [(1, 16), (1, 144)] +
                  [(2, P) for P in (16, 48, 80, 144)] + [(3, P) for P in (16, 48, 80, 144)] +
                  [(128, P) for P in (20, 28, 36)])
GEOMETRY_N = 3  # two lanes get 2 + 1 patches
# model_1 at P = 144 with the module's gain of 1/4: 1.9e-2 of the oracle's outputs are exactly 0 or 255
GEOMETRY_UNCLIPPED_GAIN = {(1, 144): 1 / 8}


def geometry_patches(model_id, P):
    from tf_image_compression_amd.synthetic import structured_patches
    return structured_patches(GEOMETRY_N, P, seed=1000 + model_id + P)


def geometry_unclipped_params(model_id, P):
    return unclipped_params(model_id, gain=GEOMETRY_UNCLIPPED_GAIN.get((model_id, P)))


def clipped_share_and_span(ref_f):
    f = np.asarray(ref_f)
    return float(np.mean((f <= 0) | (f >= 255))), float(f.max() - f.min())


def quant_rule_excluded(pre, Q):
    """(t, safe): the f64 level of each pre-activation and where the f32 quantiser's result is
    determined: farther than 8 * 2^-24 * (Q-1) levels from a threshold (expf within 2 ulp, the
    add, the division and the multiplication within half an ulp each, times two)."""
    t = quant_level_f64(pre, Q)
    return t, half_margin(t) > 8 * 2.0 ** -24 * (Q - 1)


def crafted_symbols(Q, code_shape, seed):
    """Five symbol patches no encoder produced: two uniform random ones, all 0, all Q-1 (the SAME
    padding around them must read 0.0, not lut[0]) and a checkerboard of 0 and Q-1."""
    eh, ew, ec = code_shape
    r = np.random.default_rng(np.random.PCG64(seed))
    s = np.empty((5, eh, ew, ec), np.uint8)
    s[:2] = r.integers(0, Q, (2, eh, ew, ec))
    s[2] = 0
    s[3] = Q - 1
    yy, xx, cc = np.meshgrid(np.arange(eh), np.arange(ew), np.arange(ec), indexing="ij")
    s[4] = np.where((yy + xx + cc) % 2 == 0, 0, Q - 1)
    return s


def decoder_reference(params, model_id, idx, Q):
    """(ref_f, ref_u8, E32): the f64-accumulated oracle on these symbols, and per patch the max
    distance of the same oracle accumulated in f32 from it — the reference's own f32 error."""
    ref_f, ref_u8 = o.decoder(params, codec_mean(), codec_std(), idx, Q, model_id)
    f32, _ = o.decoder(params, codec_mean(), codec_std(), idx, Q, model_id, acc=np.float32)
    e32 = np.max(np.abs(f32.astype(np.float64) - ref_f), axis=(1, 2, 3))
    return ref_f, ref_u8, e32


def decoder_errors(codec, idx, ref, patches=None):
    """check_codec's decoder half without its float bar: decode idx on the GPU, assert the byte
    bar (within 1, and only where the oracle's float sits on a .5 rounding edge) and, given the
    patches, the PSNR bar; returns the per-patch max |float - oracle|, the bytes and the floats."""
    ref_f, ref_u8, _ = ref
    rgb, f = codec.decode(idx, return_float=True)
    assert f.shape == ref_f.shape and rgb.shape == ref_u8.shape
    du = np.abs(rgb.astype(np.int16) - ref_u8.astype(np.int16))
    assert int(du.max()) <= 1
    edge = np.abs((ref_f - np.floor(ref_f)) - 0.5) < 1e-2
    assert int(np.count_nonzero((du > 0) & ~edge)) == 0
    if patches is not None:
        p_gpu = o.dataset_psnr([(patches[i], rgb[i]) for i in range(len(patches))])
        p_ref = o.dataset_psnr([(patches[i], ref_u8[i]) for i in range(len(patches))])
        assert abs(p_gpu - p_ref) <= 0.02, (p_gpu, p_ref)
    return np.max(np.abs(f.astype(np.float64) - ref_f), axis=(1, 2, 3)), rgb, f


def float_bar(e32):
    """The decoder's float bar where nothing is clipped: four times the reference's own f32 error
    (the MFMA and Winograd summation orders differ from numpy's), never above DESIGN.md §4's 1e-2."""
    return min(4.0 * float(e32), 1e-2)


def wino4_float_bar(err_direct):
    """F(4x4,3x3): the rule of test_gpu_wino4.py as it stands there, within twice the direct
    form's error, that error floored at 1e-3 — and never above 1e-2.  The form's transforms
    (constants up to 8) cost it a few times the error of the reference's own op order; on the
    unclipped parameters it measures 1.1 to 4.1 E32 and up to 2.6 times the direct form's error,
    both a few f32 ulp of the output, so the floor decides here."""
    return min(2.0 * max(float(err_direct), 1e-3), 1e-2)


# ---------------------------------------------------------------------------
# The rmbe post-filter: the window network and the whole-image driver (test_gpu_rmbe.py,
# test_gpu_product.py; input conditions: test_parity_inputs_host.py).  Nothing below needs a GPU.
# Reference: submit/2/rmbe/model.py:113-197 (the net), submit/2/rmbe/rmbe.py:15-111 (the passes).
# ---------------------------------------------------------------------------
# the variant tables of the fused head, the fused tail and the VALU last layer (conv_rgb.hip
# enc01_variants(): TH1 2/4 padded, 2/4/8 compact; dec10_variants(): PK x PF x TA x CMP;
# convT_rgb_valu.h: TW 64/32/16 one-shot, then persistent)
ENC01_VARIANTS = range(5)
DEC10_VARIANTS = range(16)
RGB_OUT_TILES = range(6)
RGB_OUT_PERSISTENT_FROM = 3

RMBE_P, RMBE_OFF = 128, 64
# (H, W): ((hn, wn) of pass 1, (hn, wn) of pass 2) — 0 windows where either count is 0
RMBE_IMAGES = {
    (128, 192): ((1, 1), (0, 1)),   # pass 1 is 1 x 1, pass 2 has no window
    (192, 128): ((1, 0), (1, 1)),   # pass 1 has no window, pass 2 is 1 x 1
    (192, 192): ((1, 1), (1, 1)),   # one window each, overlapping
    (191, 191): ((1, 0), (0, 1)),   # no window in either pass
    (200, 330): ((1, 2), (1, 2)),
    (320, 448): ((2, 3), (2, 3)),   # hn != wn; at chunk 4: 4 + 2 windows, 2 + 2 and 1 + 1 per lane
    (448, 320): ((3, 2), (3, 2)),
}


RMBE_NET_FLOAT = slice(0, 4)    # rmbe_net_windows(): the windows whose oracle output clips nowhere
RMBE_NET_FLAT255 = slice(4, 5)  # the all-255 window: 12.6 % of its oracle output is exactly 0
RMBE_4K_PASSES = (464, 480)     # windows per pass of 3840 x 2160: 16 x 29 and 16 x 30


def rmbe_pass_checked(n):
    """The windows of a pass-sized call compared with the oracle: the first two (the first chunk's
    first lane), the first of the second chunk (its first lane) and the last two (its last lane)."""
    return [0, 1, 256, n - 2, n - 1]


def rmbe_params():
    from tf_image_compression_amd.topology import RMBE_ID
    from tf_image_compression_amd.weights import synthetic_params
    return synthetic_params(RMBE_ID, seed=0)


def structured_image(H, W, seed):
    """The smooth-plus-noise uint8 image of the whole-image tests (test_gpu_image.py's _image)."""
    r = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    base = 128 + 60 * np.sin(xx / 17.0)[..., None] * np.cos(yy / 23.0)[..., None] + r.normal(0, 12, (H, W, 3))
    return np.clip(base, 0, 255).astype(np.uint8)


def rmbe_image(H, W):
    """The float32 image of a whole-image case ((200, 330): test_rmbe_whole_image's seed)."""
    return structured_image(H, W, 11 if (H, W) == (200, 330) else 7 * H + W).astype(np.float32)


def rmbe_window_counts(H, W):
    """((hn, wn), (hn, wn)) of the two passes (rmbe.py:70-72 and :92-94)."""
    return ((H // RMBE_P, (W - RMBE_OFF) // RMBE_P), ((H - RMBE_OFF) // RMBE_P, W // RMBE_P))


def rmbe_net_windows():
    """Five windows: two crops of a structured image, one of clipped Gaussian noise
    (test_rmbe_network's), all 0 and all 255 — the flat ones show the SAME padding and the f32
    normalise at the border, where a padded tap must read 0.0 and not (0 - mean) / std."""
    img = structured_image(300, 400, 3).astype(np.float32)
    w = np.empty((5, RMBE_P, RMBE_P, 3), np.float32)
    w[0] = img[:128, :128]
    w[1] = img[150:278, 201:329]
    w[2] = np.clip(np.random.default_rng(3).normal(120, 50, (RMBE_P, RMBE_P, 3)), 0, 255)
    w[3] = 0
    w[4] = 255
    return w


def rmbe_pass_windows(n):
    """n windows as the 4K image's passes bring them: clipped Gaussian noise, with crops of a
    structured image at 0, 255, 256 (the two sides of the handle's chunk boundary) and n - 1."""
    r = np.random.default_rng(464)
    w = np.clip(r.normal(120, 50, (n, RMBE_P, RMBE_P, 3)), 0, 255).astype(np.float32)
    img = structured_image(256, 256, 5).astype(np.float32)
    for k, (y, x) in zip((0, 255, 256, n - 1), ((0, 0), (0, 128), (128, 0), (128, 128))):
        w[k] = img[y:y + RMBE_P, x:x + RMBE_P]
    return w


def rmbe_reference(params, windows):
    """(ref, E32): the f64-accumulated oracle of the window network, and the max distance of the
    same oracle accumulated in f32 from it over this call (decoder_reference's rule)."""
    ref = o.rmbe_model(params, codec_mean(), codec_std(), windows)
    f32 = o.rmbe_model(params, codec_mean(), codec_std(), windows, acc=np.float32)
    return ref, float(np.max(np.abs(f32.astype(np.float64) - ref)))


def rmbe_image_reference(params, img):
    """(ref, E32) of the two-pass whole-image filter, as rmbe_reference (E32 over both passes;
    0.0 for an image without a window, whose reference is the image itself)."""
    ref = o.rmbe(img, params, codec_mean(), codec_std())
    f32 = o.rmbe(img, params, codec_mean(), codec_std(), acc=np.float32)
    return ref, float(np.max(np.abs(f32.astype(np.float64) - ref)))


def rmbe_clipped_share(ref, changed=None):
    """Share of oracle outputs exactly 0 or 255 among the values the filter changes (all of a
    window batch; of an image, the pixels inside a window of either pass)."""
    f = np.asarray(ref)
    if changed is not None:
        f = f[changed]
    return float(np.mean((f <= 0) | (f >= 255))) if f.size else 0.0


def rmbe_covered(H, W):
    """Boolean [H, W]: the pixels inside a window of either pass (every other pixel the oracle
    leaves unchanged)."""
    m = np.zeros((H, W), bool)
    (h1, w1), (h2, w2) = rmbe_window_counts(H, W)
    if h1 > 0 and w1 > 0:
        m[:h1 * RMBE_P, RMBE_OFF:RMBE_OFF + w1 * RMBE_P] = True
    if h2 > 0 and w2 > 0:
        m[RMBE_OFF:RMBE_OFF + h2 * RMBE_P, :w2 * RMBE_P] = True
    return m


def set_options(codec, **kw):
    """Every structural option the parity tests vary, set explicitly (handles are shared)."""
    opts = {"streams": 2, "fuse01": -1, "fuse_tail": -1, "s1_form": -1, "s2_form": -1, "chain": 0, "chain_wh": 2,
            "chain_x": 0, "chain_j": 0}
    assert set(kw) <= set(opts), kw
    opts.update(kw)
    for k, v in opts.items():
        codec.set_option(k, v)


POISON_WORD = 0x7FC5A5A5  # tic.h, option "poison": a NaN as f32; bytes 165, 165, 197, 127


def poisoned(codec):
    """Turn option "poison" on for a handle and return it: from here on every pass starts from
    workspaces, hand-off buffer and output staging that hold POISON_WORD, so a bit-identity check
    on one handle no longer finds the previous run's (equal, hence right) values in what a kernel
    left unwritten.  Not for handles whose test measures time, tunes or replays a graph."""
    codec.set_option("poison", 1)
    return codec


def layer_index(codec, name):
    return [lay[0] for lay in codec.layers()].index(name)


def launched_kernel(codec, layer, n, codec_step=False):
    """The kernel that runs `layer` for lane batch n: its own, or the fused launch it is inside
    (tic_layer_kernel / tic_codec_kernel name layers inside a launch '').  Asks for the layers
    up to `layer` only, so a forced tiling need not exist for the layers behind it."""
    import ctypes as C
    from tf_image_compression_amd._lib import check, lib
    fn = lib().tic_codec_kernel if codec_step else lib().tic_layer_kernel
    names = []
    for i in range(layer + 1):
        buf = C.create_string_buffer(160)
        check(fn(codec._h, i, n, buf, 160), "tic_layer_kernel")
        names.append(buf.value.decode())
    while layer > 0 and names[layer] == "":
        layer -= 1
    return names[layer]


def device_codec(codec, x):
    """tic_codec_device on x (the only entry that runs the joined launch): (symbols, bytes)."""
    eh, ew, ec = codec.code_shape
    n = len(x)
    nsym = n * eh * ew * ec
    d_in, d_idx, d_rgb = codec.alloc(x.nbytes), codec.alloc(nsym), codec.alloc(x.nbytes)
    try:
        d_in.upload(x)
        codec.memset_device(d_idx, 0xA5, nsym)  # nothing carried over from an earlier run
        codec.memset_device(d_rgb, 0x5A, x.nbytes)
        codec.codec_device(d_in, n, d_idx, d_rgb)
        codec.synchronize()
        return d_idx.download((n, eh, ew, ec), np.uint8), d_rgb.download(x.shape, np.uint8)
    finally:
        for b in (d_in, d_idx, d_rgb):
            b.free()


def codec_mean():
    from tf_image_compression_amd.weights import SYNTH_MEAN
    return SYNTH_MEAN


def codec_std():
    from tf_image_compression_amd.weights import SYNTH_STD
    return SYNTH_STD

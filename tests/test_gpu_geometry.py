"""Geometry sweep: every model at the small and odd stage sides the other modules never compare
with anything (gpu_checks.GEOMETRY_CASES: a 1- and a 2-wide partial chain region, 5- to 7-wide
regions with odd Winograd half tiles, exactly one full region, sides 1 and 2, ch_128's 128-wide
instances at odd sides), three patches on two lanes (2 + 1), every handle with option "poison" on
(tic.h), so nothing a kernel leaves unwritten passes for an earlier run's value.

(a) oracle parity in the fully unfused configuration and in each model's default options, at
    the bars of gpu_checks, and the decoder's float error on parameters that
    clip nothing against the reference's own f32 error (float_bar / wino4_float_bar);
(b) bit identity with the unfused run of the same forms for the chain (workgroup sizes,
    chain_x levels, one and two lanes), decode_2 in the polyphase form inside the chain, the
    joined launch of codec_device, and every variant of the fused head, the fused tail and the
    VALU last layer.  Each sub-case first asserts that the launch it means to test is planned;
    where the planner declines a fusion the tables below say so and the decline is asserted.
The input conditions (decision band, nothing clipped) are asserted on the CPU by
test_parity_inputs_host.py::test_geometry_sweep_inputs.  Reference layers: model_0/model.py:34-263,
model_1 .. model_3 likewise, base_model/ch_128/model.py:34-215."""
import re

import numpy as np
import pytest

import gpu_checks as g

pytestmark = pytest.mark.gpu

CASES = g.GEOMETRY_CASES
IDS = [f"m{m}-P{P}" for m, P in CASES]
CHAIN_CASES = [(m, P) for m, P in CASES if m in (0, 1, 2, 3)]
CHAIN_IDS = [f"m{m}-P{P}" for m, P in CHAIN_CASES]
UNFUSED = dict(chain=0, fuse01=0, fuse_tail=0)
CHAIN = re.compile(r"wino_chain_kernel<(\d),(\d),(\d),(\d+)>")
JOINED = re.compile(r"wino_chain_kernel<0,1,2,(\d+)>")
HEAD, TAIL, TAIL2, TAIL2_PW, JOIN = 1, 2, 4, 8, 16  # wino_chain.h HT bits

# The chain launches planned with the fused head and tail at their defaults, as the HT bits of
# each launch in layer order: [model][(chain_wh, chain_x, s2_form of decode_2)].  None of it
# depends on the geometry at these sizes (chain_x_fits: 2 x lanes x regions <= CUs holds up to 5 x 5
# regions).  Declines, all by the planner's rules and asserted as such:
# * chain_wh 1: the 256-thread workgroup runs no head or tail, so chain_x changes nothing;
# * model_2: decode_2 is the fused tail's first layer (dec10_kernel), not a TAIL2; its encoder
#   run ends before the stride-2 quantiser layer, so no launch is joined (test_gpu_chain_junction.py);
# * model_3: the run at P/4 in the encoder follows a 32 -> 64 layer (no 64 -> 64 head), the one
#   in the decoder is followed by decode_2 (64 -> 32: no tail); decode_3 is the P/8 run's tail.
def _expected_hts(model_id, wh, cx, pw):
    x = cx if wh == 2 else 0
    t2 = (TAIL2 | (TAIL2_PW if pw else 0)) if x >= 2 else 0
    if model_id in (0, 1):
        return [HEAD if x else 0, (TAIL | t2) if x else 0]
    if model_id == 2:
        return [HEAD if x else 0, TAIL if x else 0]
    return [0, HEAD if x else 0, TAIL if x else 0, 0]


NO_ENC01 = {128}  # encode_1 .. encode_2 is 64 -> 128: none of enc01_kernel's widths
NO_DEC10 = {128}  # decode_2 is 128 -> 64: none of dec10_kernel's widths
S2_DEFAULT_PW = {0: True, 1: True, 2: False, 3: True}  # tic.h "s2_form": the model's default form


@pytest.fixture(scope="module")
def handles():
    """Poisoned handles per (model, P, unclipped?) with their parameters and the case's patches."""
    from tf_image_compression_amd.codec import Codec
    from tf_image_compression_amd.weights import synthetic_params
    cache = {}

    def get(model_id, P, unclipped=False):
        key = (model_id, P, unclipped)
        if key not in cache:
            params = g.geometry_unclipped_params(model_id, P) if unclipped else synthetic_params(model_id, seed=0)
            c = Codec(model_id, params, g.codec_mean(), g.codec_std(), patch_size=P)
            cache[key] = (g.poisoned(c), params)
        return cache[key] + (g.geometry_patches(model_id, P),)

    yield get
    for c, _ in cache.values():
        c.close()


def _run(c, x):
    idx, pre = c.encode(x, return_preact=True)
    u8, f = c.decode(idx, return_float=True)
    return idx, pre, u8, f


def _same(ref, got, what):
    for name, a, b in zip(("symbols", "pre-activations", "bytes", "floats"), ref, got):
        assert np.array_equal(a, b), (what, name, int(np.count_nonzero(a != b)))


def _lane_batches(streams):
    return (g.GEOMETRY_N,) if streams == 1 else (2, 1)


def _chain_hts(c, n, codec_step=False):
    kern = c.codec_kernels(n) if codec_step else c.layer_kernels(n)
    return [(int(m[3]), int(m[4])) for m in map(CHAIN.fullmatch, kern) if m]


# ---------------------------------------------------------------------------- (a) oracle parity
def _configs(model_id):
    """(tag, options, kernels that must be planned): the fully unfused configuration and the
    model's default options; ch_128 also with its 128-wide layers in the direct stride-1 form and
    in the polyphase stride-2 / transposed form."""
    cfg = [("unfused", dict(UNFUSED, s1_form=1, s2_form=0), [r"conv3x3_wino_kernel<", r"conv3x3<[12],"]),
           ("default", dict(chain=-1, chain_x=-1, chain_j=-1), [])]
    if model_id == 128:
        cfg += [("unfused direct", dict(UNFUSED, s1_form=0, s2_form=0), [r"conv3x3<0,128,128,", r"conv3x3<2,128,64,"]),
                ("unfused polyphase", dict(UNFUSED, s1_form=1, s2_form=1),
                 [r"conv3x3_pwino_kernel<1,64,128,", r"conv3x3_pwino_kernel<2,128,64,", r"conv3x3_wino_kernel<128,128,"])]
    return cfg


@pytest.mark.parametrize("model_id,P", CASES, ids=IDS)
def test_oracle_parity(handles, model_id, P):
    c, params, x = handles(model_id, P)
    cu, params_u, _ = handles(model_id, P, unclipped=True)
    # the direct form's decoder error first: F(4x4,3x3)'s bar is stated against it
    g.set_options(cu, **dict(UNFUSED, s1_form=0, s2_form=0))
    idx = cu.encode(x)
    ref = g.decoder_reference(params_u, model_id, idx, 2)
    e32 = float(ref[2].max())
    share, _ = g.clipped_share_and_span(ref[0])
    assert share <= 1e-3, share  # the symbols are the GPU's: the CPU test's condition, met here too
    err_direct = float(g.decoder_errors(cu, idx, ref, x)[0].max())
    print(f"\ngeometry model {model_id} P {P}: E32 {e32:.3e} direct {err_direct:.3e} ({err_direct / e32:.2f} E32)")
    assert err_direct <= g.float_bar(e32), (err_direct, e32)
    for tag, opts, planned in _configs(model_id):
        g.set_options(c, **opts)
        kern = c.layer_kernels(2)
        if tag != "default":
            assert not any(k == "" or "wino_chain" in k or "enc01" in k or "dec10" in k for k in kern), kern
        for pat in planned:
            assert any(re.match(pat, k) for k in kern), (pat, kern)
        g.check_codec(c, params, model_id, P, x)
        g.set_options(cu, **opts)
        wino4 = any("wino4" in k for k in cu.layer_kernels(2))
        err = float(g.decoder_errors(cu, idx, ref, x)[0].max())
        bar = g.wino4_float_bar(err_direct) if wino4 else g.float_bar(e32)
        print(f"  {tag}: max |gpu - oracle| {err:.3e} ({err / e32:.2f} E32) bar {bar:.3e}" + (" F(4x4,3x3)" if wino4 else ""))
        assert err <= bar, (tag, err, e32, bar)
    if model_id == 3:  # the default stride-1 form of model_3 is F(4x4,3x3) (tic.h "s1_form")
        assert wino4
    g.set_options(c)
    g.set_options(cu)


# ---------------------------------------------------------------------------- (b) bit identity
@pytest.mark.parametrize("model_id,P", CHAIN_CASES, ids=CHAIN_IDS)
def test_chain_equals_unfused(handles, model_id, P):
    """chain 1 at both workgroup sizes, every chain_x level, one and two lanes, in the model's
    stride-2 form, against the unfused F(2x2,3x3) launches (models 0-2 as they are, model_3 with
    s1_form 1: the chain runs no other form)."""
    c, _, x = handles(model_id, P)
    g.set_options(c, **dict(UNFUSED, s1_form=1))
    assert not any(k == "" or "wino_chain" in k for k in c.layer_kernels(2))
    ref = _run(c, x)
    for wh in (1, 2):
        for cx in (0, 1, 2):
            for streams in (1, 2):
                g.set_options(c, chain=1, chain_wh=wh, chain_x=cx, streams=streams, s1_form=1)
                want = _expected_hts(model_id, wh, cx, S2_DEFAULT_PW[model_id])
                for n in _lane_batches(streams):
                    got = _chain_hts(c, n)
                    assert [w for w, _ in got] == [wh] * len(want) and [h for _, h in got] == want, (got, want)
                _same(ref, _run(c, x), (wh, cx, streams))
    g.set_options(c)


@pytest.mark.parametrize("model_id,P", CHAIN_CASES, ids=CHAIN_IDS)
def test_chain_decode2_polyphase_equals_standalone(handles, model_id, P):
    """s2_form 1 with chain_x 2: decode_2 behind the chain's tail in the polyphase form
    (CH_TAIL2_PW) against the standalone conv3x3_pwino_kernel (test_gpu_pwino.py's rule)."""
    c, _, x = handles(model_id, P)
    g.set_options(c, **dict(UNFUSED, s1_form=1, s2_form=1))
    kern = c.layer_kernels(2)
    assert not any(k == "" or "wino_chain" in k for k in kern)
    # models 2 and 3: decode_2 is the fused tail's first layer, which keeps the direct form
    # whatever the flags say (pwino_layer), and is no TAIL2 — declined, and run all the same
    pw = model_id in (0, 1)
    assert kern[g.layer_index(c, "decode_2")].startswith("conv3x3_pwino_kernel<2,64,32,") == pw, kern
    ref = _run(c, x)
    for streams in (1, 2):
        g.set_options(c, chain=1, chain_wh=2, chain_x=2, streams=streams, s1_form=1, s2_form=1)
        want = _expected_hts(model_id, 2, 2, True)
        for n in _lane_batches(streams):
            assert [h for _, h in _chain_hts(c, n)] == want, (c.layer_kernels(n), want)
            inside = c.layer_kernels(n)[g.layer_index(c, "decode_2")] == ""
            assert inside == pw
        _same(ref, _run(c, x), streams)
    g.set_options(c)


@pytest.mark.parametrize("model_id,P", [mp for mp in CASES if mp[0] in (0, 1)],
                         ids=[i for i, mp in zip(IDS, CASES) if mp[0] in (0, 1)])
def test_joined_launch_equals_unfused(handles, model_id, P):
    """chain_j 1 through codec_device: one launch from encode_3 to the decoder's tail, against
    the unfused host run's symbols and bytes.  Only those two: codec_device, the one entry that
    runs the joined launch, returns neither pre-activations nor decoder floats."""
    c, _, x = handles(model_id, P)
    g.set_options(c, **dict(UNFUSED, s1_form=1))
    idx, _, u8, _ = _run(c, x)
    for cx in (1, 2):
        for streams in (1, 2):
            g.set_options(c, chain=1, chain_wh=2, chain_x=cx, chain_j=1, streams=streams, s1_form=1)
            want = HEAD | _expected_hts(model_id, 2, cx, S2_DEFAULT_PW[model_id])[1] | JOIN
            for n in _lane_batches(streams):
                hts = [int(m[1]) for m in map(JOINED.fullmatch, c.codec_kernels(n)) if m]
                assert hts == [want], (c.codec_kernels(n), want)
            for _ in range(2):  # the second launch runs on the first one's flags (next epoch)
                d_idx, d_u8 = g.device_codec(c, x)
                assert np.array_equal(d_idx, idx) and np.array_equal(d_u8, u8), (cx, streams)
    g.set_options(c)


@pytest.mark.parametrize("model_id,P", CASES, ids=IDS)
def test_head_tail_and_last_layer_variants(handles, monkeypatch, model_id, P):
    """Every TIC_ENC01_VARIANT, TIC_DEC10_VARIANT and TIC_RGB_OUT_TILE against the unfused run in
    the model's default forms."""
    c, _, x = handles(model_id, P)
    n_lane = 2
    g.set_options(c, **UNFUSED)
    assert not any(k == "" for k in c.layer_kernels(n_lane))
    ref = _run(c, x)
    L = len(c.layers())
    # the fused head
    g.set_options(c, **dict(UNFUSED, fuse01=1))
    names = set()
    for v in g.ENC01_VARIANTS:
        monkeypatch.setenv("TIC_ENC01_VARIANT", str(v))
        kern = c.layer_kernels(n_lane)
        if model_id in NO_ENC01:
            assert not any("enc01" in k for k in kern) and all(kern), kern
            continue
        assert kern[0].startswith("enc01_kernel<") and kern[1] == "", kern
        names.add(kern[0])
        idx, pre = c.encode(x, return_preact=True)
        assert np.array_equal(pre, ref[1]) and np.array_equal(idx, ref[0]), v
    assert len(names) == (0 if model_id in NO_ENC01 else len(g.ENC01_VARIANTS)), names
    monkeypatch.delenv("TIC_ENC01_VARIANT")
    # the fused tail
    g.set_options(c, **dict(UNFUSED, fuse_tail=1))
    names = set()
    for v in g.DEC10_VARIANTS:
        monkeypatch.setenv("TIC_DEC10_VARIANT", str(v))
        kern = c.layer_kernels(n_lane)
        if model_id in NO_DEC10:
            assert not any("dec10" in k for k in kern) and all(kern), kern
            continue
        assert kern[L - 2].startswith("dec10_kernel<") and kern[L - 1] == "", kern
        names.add(kern[L - 2])
        u8, f = c.decode(ref[0], return_float=True)
        assert np.array_equal(u8, ref[2]) and np.array_equal(f, ref[3]), v
    assert len(names) == (0 if model_id in NO_DEC10 else len(g.DEC10_VARIANTS)), names
    monkeypatch.delenv("TIC_DEC10_VARIANT")
    # the VALU last layer's tilings, the persistent ones also with several tiles per workgroup
    g.set_options(c, **UNFUSED)
    names = set()
    for t in g.RGB_OUT_TILES:
        monkeypatch.setenv("TIC_RGB_OUT_TILE", str(t))
        kern = c.layer_kernels(n_lane)
        assert re.fullmatch(r"convT_rgb_valu(_persist)?_kernel<\d+,\d+>", kern[L - 1]), kern
        assert ("_persist" in kern[L - 1]) == (t >= g.RGB_OUT_PERSISTENT_FROM), kern
        names.add(kern[L - 1])
        for grid in ((0, 7) if t >= g.RGB_OUT_PERSISTENT_FROM else (0,)):
            c.set_option("persist_grid", grid)
            u8, f = c.decode(ref[0], return_float=True)
            c.set_option("persist_grid", 0)
            assert np.array_equal(u8, ref[2]) and np.array_equal(f, ref[3]), (t, grid)
    assert len(names) == len(g.RGB_OUT_TILES), names
    g.set_options(c)

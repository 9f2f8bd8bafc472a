"""CPU tests of the MS-SSIM / rate-estimate feature: the scratch arithmetic and the argument
checks of the two C entries (no device is touched), the host combination of the device sums
(evaluate.msssim_from_sums) against the float64 restatement in tests/msssim_ref.py,
evaluate.estimated_bits against the files the range coder writes, and the CLI's parser."""
import ctypes as C
import os

import numpy as np
import pytest

import msssim_ref as ref

EINVAL = -1


@pytest.fixture(scope="module")
def L():
    from tf_image_compression_amd import _lib
    return _lib.lib()


def _i32(v):
    return np.asarray(v, np.int32)


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t)) if a is not None else None


def _scratch(L, sizes, n=None, hs_null=False, ws_null=False, out_null=False):
    hs, ws = _i32([s[0] for s in sizes]), _i32([s[1] for s in sizes])
    b = C.c_size_t(12345)
    rc = L.tic_msssim_scratch_bytes(None if hs_null else _p(hs, C.c_int32), None if ws_null else _p(ws, C.c_int32),
                                    len(sizes) if n is None else n, None if out_null else C.byref(b))
    return rc, b.value


# ---------------------------------------------------------------------------- scratch bytes
def test_scratch_bytes_grow_with_size_and_list_length(L):
    last = 0
    for side in range(161, 700, 7):  # never shrinks ...
        rc, b = _scratch(L, [(side, side)])
        assert rc == 0 and b >= last
        last = b
    last = 0
    for side in (161, 177, 256, 600, 2048):  # ... and grows with every larger pyramid
        rc, b = _scratch(L, [(side, side)])
        assert rc == 0 and b > last
        last = b
    rc, wide = _scratch(L, [(161, 900)])
    rc2, tall = _scratch(L, [(900, 161)])
    rc3, small = _scratch(L, [(161, 161)])
    assert rc == rc2 == rc3 == 0 and wide > small and tall > small
    last = 0
    for n in range(1, 70, 17):  # also past the 64 images one launch holds
        rc, b = _scratch(L, [(177, 203)] * n)
        assert rc == 0 and b > last
        last = b
    rc, one = _scratch(L, [(177, 203)])
    rc, other = _scratch(L, [(256, 320)])
    rc, both = _scratch(L, [(177, 203), (256, 320)])
    assert both == one + other  # per-image needs add up
    assert _scratch(L, [], n=0) == (0, 0)


def test_scratch_bytes_holds_planes_and_partials(L):
    """At least the pyramid planes of scales 1..4 (two float32 images each) must fit."""
    H, W = 177, 203
    planes, h, w = 0, H, W
    for _ in range(4):
        h, w = (h + 1) // 2, (w + 1) // 2
        planes += 2 * h * w * 3 * 4
    rc, b = _scratch(L, [(H, W)])
    assert rc == 0 and b > planes


def test_scratch_bytes_errors(L):
    for sizes in ([(160, 161)], [(161, 160)], [(300, 300), (160, 400)], [(0, 200)], [(-5, 200)]):
        rc, b = _scratch(L, sizes)
        assert rc == EINVAL and b == 0, sizes
    assert b"161" in L.tic_last_error()
    assert _scratch(L, [(200, 200)], hs_null=True)[0] == EINVAL
    assert _scratch(L, [(200, 200)], ws_null=True)[0] == EINVAL
    assert _scratch(L, [(200, 200)], out_null=True)[0] == EINVAL
    assert _scratch(L, [(200, 200)], n=-1)[0] == EINVAL
    from tf_image_compression_amd.codec import Codec
    assert Codec.msssim_scratch_bytes([(177, 203)]) == _scratch(L, [(177, 203)])[1]
    assert Codec.msssim_scratch_bytes([]) == 0
    with pytest.raises(ValueError, match="161"):
        Codec.msssim_scratch_bytes([(200, 160)])


# ---------------------------------------------------------------------------- argument errors, no device
class _Call:
    """tic_msssim_images_device with a zeroed block as the handle (never dereferenced by a call
    that fails its argument checks, as in test_image_batch_host.py) and a made-up device pointer."""

    def __init__(self, L):
        self.L = L
        self.block = C.create_string_buffer(1 << 16)
        self.h = C.cast(self.block, C.c_void_p)
        self.dev = C.c_void_p(0x1000)

    def __call__(self, sizes, offsets, h="h", a="d", b="d", scr="d", out="d", n=None, scratch_bytes=1 << 40,
                 off_null=False, hs_null=False, ws_null=False):
        hs, ws = _i32([s[0] for s in sizes]), _i32([s[1] for s in sizes])
        off = np.asarray(offsets, np.int64)
        pick = lambda v: self.dev if v == "d" else v  # noqa: E731
        return self.L.tic_msssim_images_device(
            self.h if h == "h" else h, pick(a), pick(b), None if off_null else _p(off, C.c_int64),
            None if hs_null else _p(hs, C.c_int32), None if ws_null else _p(ws, C.c_int32),
            len(sizes) if n is None else n, pick(scr), scratch_bytes, pick(out))


@pytest.fixture(scope="module")
def call(L):
    return _Call(L)


def test_argument_errors_without_device(L, call):
    sizes, offs = [(161, 161), (177, 203)], [0, 161 * 161 * 3]
    assert call(sizes, offs, h=None) == EINVAL
    assert b"null handle" in L.tic_last_error()
    assert call(sizes, offs, h=None, n=0) == EINVAL  # an empty list still needs a handle
    for kw in ({"a": None}, {"b": None}, {"scr": None}, {"out": None}, {"off_null": True}, {"hs_null": True},
               {"ws_null": True}):
        assert call(sizes, offs, **kw) == EINVAL, kw
    assert call(sizes, offs, n=-1) == EINVAL
    assert b"n_images" in L.tic_last_error()
    assert call([(161, 161), (160, 300)], offs) == EINVAL
    assert b"161" in L.tic_last_error()
    assert call([(300, 160)], [0]) == EINVAL
    assert call(sizes, [0, -1]) == EINVAL
    need = _scratch(L, sizes)[1]
    assert call(sizes, offs, scratch_bytes=need - 1) == EINVAL
    assert b"too small" in L.tic_last_error()
    assert call(sizes, offs, scratch_bytes=0) == EINVAL
    # n_images == 0 is a no-op that looks at nothing else
    assert call([], [], a=None, b=None, scr=None, out=None, n=0, scratch_bytes=0, off_null=True, hs_null=True,
                ws_null=True) == 0


def test_python_wrapper_raises_value_error(call):
    from tf_image_compression_amd.codec import Codec

    class Buf:
        ptr = call.dev
        nbytes = 1 << 40

    class Small(Buf):
        nbytes = 16

    c = Codec.__new__(Codec)
    c._h = call.h
    try:
        with pytest.raises(ValueError, match="161"):
            c.msssim_images_device(Buf, Buf, [0], [(160, 200)], Buf, Buf)
        with pytest.raises(ValueError, match="too small"):
            c.msssim_images_device(Buf, Buf, [0], [(200, 200)], Small, Buf)
        with pytest.raises(ValueError, match="offsets for"):
            c.msssim_images_device(Buf, Buf, [0, 5], [(200, 200)], Buf, Buf)
        with pytest.raises(ValueError, match="d_out holds"):
            c.msssim_images_device(Buf, Buf, [0], [(200, 200)], Buf, Small)
    finally:
        c._h = None  # nothing to destroy


# ---------------------------------------------------------------------------- host combination
@pytest.mark.parametrize("H,W", [(161, 161), (177, 203)])
def test_msssim_from_sums_equals_restatement(H, W):
    from tf_image_compression_amd.evaluate import msssim_from_sums, msssim_counts
    a = ref.image("noise", H, W, 3)
    b = ref.distort(a, 20, 4)
    s = ref.sums(a, b)
    want = ref.msssim(a, b)
    assert 0.0 < want < 1.0
    assert abs(msssim_from_sums(s, H, W) - want) <= 1e-12
    assert np.array_equal(msssim_counts(H, W), ref.counts(H, W))
    # sums equal to the counts: every mean is 1
    ones = np.broadcast_to(ref.counts(H, W)[:, None, None], (5, 3, 2)).copy()
    assert msssim_from_sums(ones, H, W) == 1.0
    with pytest.raises(ValueError, match="161"):
        msssim_from_sums(s, 160, W)


def test_msssim_from_sums_clamps_negative_means_to_zero():
    from tf_image_compression_amd.evaluate import msssim_from_sums
    a = ref.image("noise", 161, 161, 5)
    s = ref.sums(a, 255 - a)
    m = ref.means(s, 161, 161)
    assert np.all(m[:4, :, 0] < 0)  # about -0.99, -0.95, -0.83, -0.50
    # scale 3 has 121 positions only, so its mean moves with the seed
    assert np.allclose(m[:4, :, 0].mean(axis=1), [-0.99, -0.95, -0.83, -0.50], atol=[0.01, 0.01, 0.02, 0.1])
    assert msssim_from_sums(s, 161, 161) == 0.0
    assert ref.combine(s, 161, 161) == 0.0


# ---------------------------------------------------------------------------- estimated_bits
def _tables():
    from tf_image_compression_amd.range_coder import symbol_table
    return {"q2_70_30": symbol_table([0.7, 0.3], 4096), "q2_97_03": symbol_table([0.97, 0.03], 4096),
            "q4": symbol_table([0.5, 0.25, 0.15, 0.1], 4096)}


@pytest.mark.parametrize("table", ["q2_70_30", "q2_97_03", "q4"])
@pytest.mark.parametrize("n", [100, 16384, 10 ** 6])
@pytest.mark.parametrize("matched", [True, False])
def test_estimated_bits_against_the_range_coder(tmp_path, table, n, matched):
    """|file bytes - est_bits / 8| <= 2 + 5e-4 * est_bits / 8: the coder alone stays within +-1
    byte of the ideal length on streams drawn from its table and was measured up to 1.9e-4
    (relative) below it on mismatched ones; the bar is about 2.5x that, two-sided."""
    from tf_image_compression_amd.evaluate import estimated_bits
    from tf_image_compression_amd.range_coder import RangeEncoder
    cum = _tables()[table]
    Q = len(cum) - 1
    p = np.diff(np.asarray(cum, np.float64)) / cum[-1] if matched else np.full(Q, 1.0 / Q)
    r = np.random.default_rng(n + Q + 7 * matched)
    data = r.choice(Q, size=n, p=p)
    path = str(tmp_path / "s.bin")
    enc = RangeEncoder(path)
    enc.encode(data, cum)
    enc.close()
    size = os.path.getsize(path)
    est = estimated_bits(np.bincount(data, minlength=Q), cum) / 8.0
    print(f"{table} n={n} matched={matched}: file {size} B, estimate {est:.1f} B")
    assert abs(size - est) <= 2 + 5e-4 * est


def test_estimated_bits_definition_and_errors():
    from tf_image_compression_amd.evaluate import estimated_bits
    assert estimated_bits([3, 1], [0, 2, 4]) == 4.0          # both symbols cost one bit
    assert estimated_bits([8, 0], [0, 1, 4]) == 16.0         # an unused symbol costs nothing
    assert estimated_bits([0, 0], [0, 1, 4]) == 0.0
    with pytest.raises(ValueError):
        estimated_bits([1, 1, 1], [0, 2, 4])
    with pytest.raises(ValueError):
        estimated_bits([1, 1], [0, 4, 4])                    # a counted symbol the table cannot code


# ---------------------------------------------------------------------------- CLI
def test_cli_parsing():
    import evaluate_codec as ec
    a = ec.my_parse_args(["-m", "0", "-g", "3"])
    assert a.data_list == "data_info/tiny_valid_data_list.txt" and a.batch_images == 1
    assert a.dist == "data_info/distribution_info_{}.npy" and a.rmbe == "" and a.json == ""
    assert not a.synthetic_weights and a.params_file == ""
    b = ec.my_parse_args(["-m", "3", "-g", "0", "--synthetic-weights", "--batch-images", "4", "--rmbe", "w.npz",
                          "--json", "out.json", "-v", "list.txt", "-p", "ckpt", "--norm", "n.npz", "--dist", "d.npy"])
    assert (b.batch_images, b.rmbe, b.json, b.data_list, b.params_file) == (4, "w.npz", "out.json", "list.txt", "ckpt")
    for bad in ("0", "-2"):
        with pytest.raises(SystemExit):
            ec.my_parse_args(["-m", "0", "-g", "0", "--batch-images", bad])
    with pytest.raises(SystemExit):
        ec.my_parse_args(["-g", "0"])


def test_cli_summary_arithmetic():
    import math
    import evaluate_codec as ec
    rows = [{"height": 200, "width": 100, "sse": 6000, "msssim": 0.9, "est_bits": 1000.0},
            {"height": 100, "width": 100, "sse": 3000, "msssim": float("nan"), "est_bits": 500.0}]
    d = ec.dataset_summary(rows)
    assert d["pixels"] == 30000 and d["n_msssim"] == 1 and d["msssim"] == 0.9
    assert d["est_bpp"] == 1500.0 / 30000
    assert abs(d["psnr"] - (20 * math.log10(255.0) - 10 * math.log10(9000 / 90000))) < 1e-12
    assert abs(ec.msssim_db(0.99) - 20.0) < 1e-9 and ec.msssim_db(1.0) == float("inf")
    rows[1]["est_bits"] = None
    assert ec.dataset_summary(rows)["est_bpp"] is None

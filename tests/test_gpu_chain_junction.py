"""The codec step's joined chain launch (option chain_j; csrc/wino_chain.h CH_JOIN): in
tic_codec_device the encoder's last chain launch (encode_3 as the head, the res blocks, encode_4
and the quantiser) and the decoder's first (the dequantiser table, decode_4, the res blocks,
decode_3 as the tail, perhaps decode_2 behind it) run as one launch.  At the junction a region
workgroup quantises with OUT_QUANT's arithmetic, writes the same symbols to the same addresses
and hands the dequantised symbols to decode_4 through LDS and one ordinary border hand-off —
the floats the decoder-side launch stages from the symbols through the table.  Nothing else
changes, so the bar is byte identity of symbols and reconstruction with the two launches
(chain_j 0), with tic_encode_device followed by tic_decode_device, and with the unfused path
(chain 0).  Reference layers: model_0/model.py:90-144 (encode_3 .. encode_4, quantiser),
148-222 (dequantiser, decode_4 .. decode_2); model_1/model.py, model_2/model.py."""
import re

import numpy as np
import pytest

from conftest import structured_patches
from gpu_checks import poisoned

pytestmark = pytest.mark.gpu

JOINED = re.compile(r"wino_chain_kernel<0,1,2,(\d+)>")


def _codec(model_id, P, Q=2):
    from tf_image_compression_amd.codec import Codec
    from tf_image_compression_amd.weights import synthetic_params, SYNTH_MEAN, SYNTH_STD
    return poisoned(Codec(model_id, synthetic_params(model_id, seed=0), SYNTH_MEAN, SYNTH_STD, patch_size=P,
                          quan_scale=Q))


class _Bufs:
    def __init__(self, c, x):
        eh, ew, ec = c.code_shape
        self.c, self.x, self.n = c, x, len(x)
        self.code = (self.n, eh, ew, ec)
        self.d_in, self.d_idx, self.d_rgb = c.alloc(x.nbytes), c.alloc(int(np.prod(self.code))), c.alloc(x.nbytes)
        self.d_in.upload(x)

    def _out(self):
        self.c.synchronize()
        return self.d_idx.download(self.code, np.uint8), self.d_rgb.download(self.x.shape, np.uint8)

    def _clear(self):  # no result is carried over from the run before
        self.c.memset_device(self.d_idx, 0xA5, int(np.prod(self.code)))
        self.c.memset_device(self.d_rgb, 0x5A, self.x.nbytes)

    def codec(self):
        self._clear()
        self.c.codec_device(self.d_in, self.n, self.d_idx, self.d_rgb)
        return self._out()

    def enc_dec(self):
        self._clear()
        self.c.encode_device(self.d_in, self.n, self.d_idx)
        self.c.decode_device(self.d_idx, self.n, self.d_rgb)
        return self._out()


def _joined_ht(c, lane_n):
    """HT of the joined launch tic_codec_device plans for lane batch lane_n (None: two launches);
    checks that the launch starts at encode_3 and holds every layer up to its tail."""
    kern = c.codec_kernels(lane_n)
    hts = [int(m[1]) for m in map(JOINED.fullmatch, kern) if m and int(m[1]) & 16]
    if not hts:
        assert kern == c.layer_kernels(lane_n)
        return None
    assert len(hts) == 1, kern
    names = [lay[0] for lay in c.layers()]
    ht = hts[0]
    assert ht & 3 == 3, kern  # head and tail
    first = names.index("encode_3")
    last = names.index("decode_2" if ht & 4 else "decode_3")
    assert JOINED.fullmatch(kern[first]) and all(k == "" for k in kern[first + 1:last + 1]), kern
    plain = c.layer_kernels(lane_n)  # everything outside it, and the separate calls, as before
    assert kern[:first] == plain[:first] and kern[last + 1:] == plain[last + 1:]
    assert not any((m := JOINED.fullmatch(k)) and int(m[1]) & 16 for k in plain), plain
    return ht


def _setup(c, chain_x=2, fuse_tail=None):
    c.set_option("s1_form", 1)
    c.set_option("chain", 1)
    c.set_option("chain_wh", 2)
    c.set_option("chain_x", chain_x)
    if fuse_tail is not None:
        c.set_option("fuse_tail", fuse_tail)


def _check_all_paths(c, b, streams_list=(1, 2), expect_ht=None, joinable=True):
    """codec_device with chain_j 1 against chain_j 0, encode_device + decode_device and chain 0."""
    c.set_option("chain", 0)
    c.set_option("streams", 1)
    ref = b.codec()  # the fully unfused path
    c.set_option("chain", 1)
    for streams in streams_list:
        c.set_option("streams", streams)
        c.set_option("chain_j", 0)
        lane_n = -(-b.n // min(streams, b.n))
        assert _joined_ht(c, lane_n) is None
        two = b.codec()
        c.set_option("chain_j", 1)
        ht = _joined_ht(c, lane_n)
        # the joined launch really is planned (or, where the planner's rule excludes it, is not)
        assert (ht is not None) == joinable, c.codec_kernels(lane_n)
        if expect_ht is not None:
            assert ht == expect_ht, ht
        for _ in range(2):  # twice: the second launch runs on the first one's flags (next epoch)
            one = b.codec()
            sep = b.enc_dec()
            for name, other in (("chain_j 0", two), ("encode + decode", sep), ("chain 0", ref)):
                assert np.array_equal(one[0], other[0]), (name, "symbols", streams)
                assert np.array_equal(one[1], other[1]), (name, "reconstruction", streams)


# (model, P, n, fuse_tail): model_0 at 256 — 2 x 2 regions, the flagship stage; on two lanes one
# launch holds two images and the other one.  P = 288: 3 x 3 regions, partial ones below and
# right, and a region with all eight neighbours.  P = 64: one region, its halo outside the image,
# no hand-off.  P = 48: one partial region.  model_1: 16-channel outer layers.  model_2 with the
# decoder-tail fusion off: decode_2 behind the tail feeds a standalone last layer — but model_2's
# encode_4 and decode_4 are stride-2 / transposed layers (model_2/model.py), so its encoder chain
# ends at encode_res_2, not at the quantiser, and the planner's rule (the encoder's last chain
# span ends at the encoder's last layer) keeps the two launches: the case runs every path all the
# same and asserts that chain_j 1 falls back there.
CASES = [(0, 256, 3, None, True), (0, 288, 2, None, True), (0, 64, 3, None, True), (0, 48, 3, None, True),
         (1, 64, 3, None, True), (2, 128, 3, 0, False)]


@pytest.mark.parametrize("model_id,P,n,fuse_tail,joinable", CASES)
def test_joined_launch_bit_identical(model_id, P, n, fuse_tail, joinable):
    with _codec(model_id, P) as c:
        _setup(c, chain_x=2, fuse_tail=fuse_tail)
        b = _Bufs(c, structured_patches(n, P, seed=900 + model_id + P))
        _check_all_paths(c, b, joinable=joinable)


@pytest.mark.parametrize("chain_x,s2_form,ht", [(1, 1, 19), (2, 0, 23), (2, 1, 31)])
def test_joined_launch_tail_forms(chain_x, s2_form, ht):
    """model_0 at 256: the tail alone (decode_2 standalone), decode_2 behind it in the direct
    form (TAIL2) and in the polyphase form (TAIL2_PW)."""
    with _codec(0, 256) as c:
        _setup(c, chain_x=chain_x)
        c.set_option("s2_form", s2_form)
        b = _Bufs(c, structured_patches(3, 256, seed=931 + chain_x + s2_form))
        _check_all_paths(c, b, expect_ht=ht)


def test_joined_launch_region_orders():
    """The region orders only place the workgroups (n = 9: a full group of eight patches and one
    that keeps the identity order under the XCD-aware order)."""
    with _codec(0, 256) as c:
        _setup(c)
        b = _Bufs(c, structured_patches(9, 256, seed=940))
        c.set_option("chain_j", 0)
        ref = b.codec()
        c.set_option("chain_j", 1)
        for order in (0, 1, 2, -1):
            c.set_option("chain_order", order)
            for streams in (1, 2):
                c.set_option("streams", streams)
                assert _joined_ht(c, -(-9 // streams)) is not None
                got = b.codec()
                assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]), (order, streams)


def test_joined_launch_quan_scale_256():
    """A 256-level quantiser (as tests/test_gpu_parity.py::test_quan_scale_256): the junction's
    symbols are encode_device's, its table look-up decode_device's."""
    with _codec(0, 64, Q=256) as c:
        _setup(c)
        b = _Bufs(c, structured_patches(4, 64, seed=950))
        c.set_option("chain_j", 1)
        assert _joined_ht(c, 2) is not None
        one, sep = b.codec(), b.enc_dec()
        assert len(np.unique(sep[0])) > 2  # more than the two levels of the default quantiser
        assert np.array_equal(one[0], sep[0])
        assert np.array_equal(one[1], sep[1])


def test_joined_launch_oversubscribed():
    """2 x 256 patches at P = 256 through codec_device with chunk 512, three calls in a row: 1024
    region workgroups per lane, more than are resident.  The scheduling assumption is the one of
    test_wino_chain_stride2_neighbours_oversubscribed, and the join adds nothing to it: with a
    grid that is not resident the region order is the atomic ticket (chain_launch_order), a
    workgroup waits only on regions of its own patch, a patch's R regions hold consecutive
    tickets, and R workgroups of a lane fit the GPU with a margin of two (chain_x_fits, a
    condition of the join).  So every patch but the one being handed out holds all its tickets in
    running workgroups and finishes whatever else is resident; the last one gets its remaining
    workgroups as soon as any other finishes.  The argument never counts layers or hand-offs, so
    it holds for the 10-layer joined launch as for the two 5-layer ones."""
    with _codec(0, 256) as c:
        _setup(c)
        x = structured_patches(8, 256, seed=960)
        small = _Bufs(c, x)
        c.set_option("chain_j", 0)
        ref = small.codec()
        c.set_option("chain_j", 1)
        c.set_option("chunk", 512)
        assert _joined_ht(c, 256) is not None
        big = _Bufs(c, np.concatenate([x] * 64))
        for _ in range(3):
            idx, rgb = big.codec()
            assert all(np.array_equal(idx[i * 8:(i + 1) * 8], ref[0]) for i in range(64))
            assert all(np.array_equal(rgb[i * 8:(i + 1) * 8], ref[1]) for i in range(64))


def test_joined_launch_tuning_round_trip():
    """tic_tuning_export carries chain_j; a second handle importing it plans the same launches and
    runs bit-identically; a text without the flag imports with the model's default; other values
    are rejected.  Also ADVICE r06 item 1: a conv entry whose form disagrees with its key's form
    bits (a polyphase kernel under a direct-form key) is rejected."""
    P, n = 64, 8
    x = structured_patches(n, P, seed=970)
    with _codec(0, P) as c, _codec(0, P) as c2:
        _setup(c)
        b = _Bufs(c, x)
        c.autotune(b.d_in, n // 2, reps=1)
        for j in (0, 1):
            c.set_option("chain_j", j)
            got = b.codec()
            text = c.tuning_export()
            assert f"flag chain_j {j}\n" in text
            c2.tuning_import(text)
            assert c2.tuning_export() == text
            assert c2.codec_kernels(n // 2) == c.codec_kernels(n // 2)
            assert (_joined_ht(c2, n // 2) is not None) == bool(j)
            got2 = _Bufs(c2, x).codec()
            assert np.array_equal(got[0], got2[0]) and np.array_equal(got[1], got2[1])
        c2.set_option("chain_j", 0)
        old = "".join(ln + "\n" for ln in text.splitlines() if not ln.startswith("flag chain_j"))
        c2.tuning_import(old)
        assert "flag chain_j 1\n" in c2.tuning_export()  # model_0's default
        for bad in ("flag chain_j 2", "flag chain_j -1"):
            with pytest.raises(ValueError):
                c2.tuning_import("tic-tuning 1\n" + bad + "\n")
        # (encode_2 runs standalone in the polyphase form: its entries carry form 1 in their keys)
        convs = [ln for ln in text.splitlines() if ln.startswith("conv ") and int(ln.split()[2]) >> 24 == 1]
        assert convs
        for ln in convs:
            k = ln.split()
            k[2] = str(int(k[2]) & 0xFFFFFF)  # the same kernel under the direct form's key
            with pytest.raises(ValueError):
                c2.tuning_import("tic-tuning 1\n" + " ".join(k) + "\n")
        assert "flag chain_j 1\n" in c2.tuning_export()  # nothing applied by the rejected imports


def test_joined_launch_graph_replay():
    """Option graph: the captured and replayed codec sequence with the joined launch equals the
    eager run."""
    P, n = 64, 6
    with _codec(0, P) as c:
        _setup(c)
        c.set_option("chain_j", 1)
        assert _joined_ht(c, n // 2) is not None
        b = _Bufs(c, structured_patches(n, P, seed=980))
        ref = b.codec()
        c.set_option("poison", 0)  # graph replay runs unpoisoned: the two options exclude each other
        c.set_option("graph", 1)
        for _ in range(3):  # capture, then replays
            got = b.codec()
            assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
        c.set_option("graph", 0)

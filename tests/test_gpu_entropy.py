"""GPU tests of the device entropy coder (csrc/tic_entropy.cpp): byte parity of
tic_entropy_encode_device with the host container (entropy.pack), symbol parity of
tic_entropy_decode_device with tic_rcseg_decode, the argument contract, and the layers above
(ImageCodec streams, evaluate_images' coded_bytes, encode.py / decode.py --entropy device)."""
import os
import struct

import numpy as np
import pytest

from conftest import structured_patches
from entropy_cases import TABLES, draw

pytestmark = pytest.mark.gpu

U64_MAX = np.iinfo(np.uint64).max
# one lane; a tail of 5; a full segment less one, exactly one, one more; three and a bit
COUNTS_4096 = [1, 5, 4095, 4096, 4097, 3 * 4096 + 5]
# one lane, then 63, 64 and 66 segments: the wave / workgroup edges
COUNTS_4 = [5, 63 * 4, 64 * 4, 65 * 4 + 1]


@pytest.fixture(scope="module")
def codec():
    from tf_image_compression_amd.codec import Codec
    from tf_image_compression_amd.weights import synthetic_params, SYNTH_MEAN, SYNTH_STD
    with Codec(0, synthetic_params(0), SYNTH_MEAN, SYNTH_STD, patch_size=64, quan_scale=2, device=0) as c:
        yield c


def _place(lengths, layout):
    """Offsets of blocks of these lengths in an arena, and the arena's size."""
    n = len(lengths)
    order = list(range(n))[::-1] if layout == "reversed" else list(range(n))
    lead, gap = {"packed": (0, 0), "odd": (1, 3), "reversed": (5, 2)}[layout]
    offs, at = [0] * n, lead
    for i in order:
        offs[i] = at
        at += lengths[i] + gap
    return offs, at + 7


def _arena(blocks, offs, size, fill):
    a = np.full(size, fill, np.uint8)
    used = np.zeros(size, bool)
    for b, o in zip(blocks, offs):
        a[o:o + len(b)] = np.frombuffer(bytes(b), np.uint8) if not isinstance(b, np.ndarray) else b
        used[o:o + len(b)] = True
    return a, used


def device_encode(codec, streams, L, layout="packed", slack=64):
    """(sizes uint64 [n], the whole d_out as bytes); d_out was filled with 0x5A."""
    from tf_image_compression_amd import entropy
    counts = [len(s) for s in streams]
    offs, size = _place(counts, layout)
    arena, _ = _arena(streams, offs, size, 0xA5)
    d_sym = codec.alloc(size)
    d_sym.upload(arena)
    cap = sum(entropy.bound(n, L) for n in counts) + slack
    d_out, d_sizes = codec.alloc(cap), codec.alloc(8 * len(streams))
    d_scr = codec.alloc(codec.entropy_scratch_bytes(counts, L))
    codec.memset_device(d_out, 0x5A, cap)
    codec.memset_device(d_sizes, 0x5A, 8 * len(streams))
    codec.entropy_encode_device(d_sym, offs, counts, L, d_scr, d_out, d_sizes)
    sizes = d_sizes.download((len(streams),), np.uint64)
    out = d_out.download((cap,), np.uint8).tobytes()
    for b in (d_sym, d_out, d_sizes, d_scr):
        b.free()
    return sizes, out


def device_decode(codec, blobs, counts, L, layout="packed"):
    """Decoded streams; the sentinels around the symbols and between them are checked."""
    boffs, bsize = _place([len(b) for b in blobs], layout)
    soffs, ssize = _place(counts, layout)
    barena, _ = _arena(blobs, boffs, bsize, 0xA5)
    d_blob, d_sym = codec.alloc(bsize), codec.alloc(ssize)
    d_blob.upload(barena)
    codec.memset_device(d_sym, 0xA5, ssize)
    d_scr = codec.alloc(codec.entropy_scratch_bytes(counts, L))
    codec.entropy_decode_device(d_blob, boffs, [len(b) for b in blobs], counts, d_sym, soffs, d_scr)
    got = d_sym.download((ssize,), np.uint8)
    for b in (d_blob, d_sym, d_scr):
        b.free()
    used = np.zeros(ssize, bool)
    for o, n in zip(soffs, counts):
        used[o:o + n] = True
    assert np.all(got[~used] == 0xA5), "bytes outside the streams were written"
    return [got[o:o + n] for o, n in zip(soffs, counts)]


@pytest.mark.parametrize("L,counts", [(4096, COUNTS_4096), (4, COUNTS_4)], ids=["L4096", "L4"])
@pytest.mark.parametrize("name", list(TABLES))
def test_encode_matches_host_container(codec, name, L, counts):
    from tf_image_compression_amd import entropy
    cum = TABLES[name]
    codec.entropy_set_table(cum)
    streams = [draw(cum, n, seed=1000 + n) for n in counts]
    want = [entropy.pack(s, cum, segment=L) for s in streams]
    for layout in ("packed", "odd", "reversed"):
        sizes, out = device_encode(codec, streams, L, layout)
        assert sizes.tolist() == [len(w) for w in want], layout
        blob = b"".join(want)
        assert out[:len(blob)] == blob, layout
        assert set(out[len(blob):]) == {0x5A}, "bytes behind the last container were written"


def test_random_stream_with_ff_bytes_and_determinism(codec):
    from tf_image_compression_amd import entropy
    cum = TABLES["p98"]
    codec.entropy_set_table(cum)
    sym = draw(cum, 200000, seed=7)
    want = entropy.pack(sym, cum, segment=4096)
    S = -(-200000 // 4096)
    assert b"\xff" in want[20 + 2 * S:]  # the pending-0xFF / carry path is in play (seed chosen on the CPU)
    sizes, out = device_encode(codec, [sym], 4096)
    assert int(sizes[0]) == len(want) and out[:len(want)] == want
    sizes2, out2 = device_encode(codec, [sym], 4096)
    assert np.array_equal(sizes, sizes2) and out == out2
    # a container depends neither on its neighbours nor on its position
    a, b = draw(cum, 5000, seed=1), draw(cum, 333, seed=2)
    s3, o3 = device_encode(codec, [a, sym, b], 4096, "odd")
    at = int(s3[0])
    assert o3[at:at + int(s3[1])] == want
    s4, o4 = device_encode(codec, [b, a], 4096, "reversed")
    assert o4[int(s4[0]):int(s4[0]) + int(s4[1])] == o3[:at]
    got = device_decode(codec, [want], [200000], 4096)[0]
    assert np.array_equal(got, sym)


@pytest.mark.parametrize("L,counts", [(4096, COUNTS_4096), (4, COUNTS_4)], ids=["L4096", "L4"])
@pytest.mark.parametrize("name", list(TABLES))
def test_decode_matches_host(codec, name, L, counts):
    from tf_image_compression_amd import entropy
    cum = TABLES[name]
    nsym = len(cum) - 1
    codec.entropy_set_table(cum)
    streams = [draw(cum, n, seed=2000 + n) for n in counts]
    blobs = [entropy.pack(s, cum, segment=L) for s in streams]
    for layout in ("packed", "odd", "reversed"):
        got = device_decode(codec, blobs, counts, L, layout)
        for g, s in zip(got, streams):
            assert np.array_equal(g, s), (layout, len(s))
    # device -> device
    sizes, out = device_encode(codec, streams, L, "odd")
    cuts = np.concatenate([[0], np.cumsum(sizes.astype(np.int64))])
    dev_blobs = [out[cuts[i]:cuts[i + 1]] for i in range(len(streams))]
    for g, s in zip(device_decode(codec, dev_blobs, counts, L, "reversed"), streams):
        assert np.array_equal(g, s)
    # payload bytes replaced by a fixed pseudo-random pattern, header and lengths intact: input the
    # decoder is specified for (zero padding past a segment's end, extents clamped); the symbols
    # must be tic_rcseg_decode's on the same bytes
    rng = np.random.default_rng(99)
    noisy = []
    for b, n in zip(blobs, counts):
        head = 20 + 2 * -(-n // L)
        noisy.append(b[:head] + rng.integers(0, 256, len(b) - head, dtype=np.uint8).tobytes())
    want = [entropy.unpack(b, cum, n=n) for b, n in zip(noisy, counts)]
    got = device_decode(codec, noisy, counts, L, "odd")
    for g, w in zip(got, want):
        assert int(g.max()) < nsym
        assert np.array_equal(g, w)


def test_decode_mixed_segment_lengths_and_bad_headers(codec):
    """Containers of different L in one call; a container whose header does not fit the caller's
    count decodes to zeros without touching its neighbours."""
    from tf_image_compression_amd import entropy
    cum = TABLES["p60"]
    codec.entropy_set_table(cum)
    a, b, c = draw(cum, 1000, seed=1), draw(cum, 777, seed=2), draw(cum, 300, seed=3)
    blobs = [entropy.pack(a, cum, segment=64), entropy.pack(b, cum, segment=4096), entropy.pack(c, cum, segment=8)]
    got = device_decode(codec, blobs, [1000, 777, 300], 8, "odd")
    assert all(np.array_equal(g, s) for g, s in zip(got, (a, b, c)))
    wrong = bytearray(blobs[1])
    wrong[12:20] = struct.pack("<Q", 778)
    got = device_decode(codec, [blobs[0], bytes(wrong), blobs[2]], [1000, 777, 300], 8, "odd")
    assert np.array_equal(got[0], a) and np.array_equal(got[2], c) and not got[1].any()


def test_argument_errors_leave_outputs_untouched(codec):
    from tf_image_compression_amd import entropy
    from tf_image_compression_amd.codec import Codec
    from tf_image_compression_amd.weights import synthetic_params, SYNTH_MEAN, SYNTH_STD
    cum = TABLES["p60"]
    codec.entropy_set_table(cum)
    counts, L = [100, 4097], 4096
    streams = [draw(cum, n, seed=n) for n in counts]
    d_sym = codec.alloc(sum(counts))
    d_sym.upload(np.concatenate(streams))
    offs = [0, 100]
    need = codec.entropy_scratch_bytes(counts, L)
    cap = sum(entropy.bound(n, L) for n in counts)
    d_scr, d_out, d_sizes = codec.alloc(need), codec.alloc(cap), codec.alloc(16)

    def untouched():
        return (set(d_out.download((cap,), np.uint8).tolist()) == {0x5A}
                and set(d_sizes.download((16,), np.uint8).tolist()) == {0x5A})

    codec.memset_device(d_out, 0x5A, cap)
    codec.memset_device(d_sizes, 0x5A, 16)
    with pytest.raises(ValueError, match="scratch"):
        codec.entropy_encode_device(d_sym, offs, counts, L, d_scr, d_out, d_sizes, scratch_bytes=need - 1)
    with pytest.raises(ValueError, match="out_cap"):
        codec.entropy_encode_device(d_sym, offs, counts, L, d_scr, d_out, d_sizes, out_cap=cap - 1)
    with pytest.raises(ValueError, match="segment length"):
        codec.entropy_encode_device(d_sym, offs, counts, 6, d_scr, d_out, d_sizes)
    with pytest.raises(ValueError, match="at least one symbol"):
        codec.entropy_encode_device(d_sym, offs, [100, 0], L, d_scr, d_out, d_sizes)
    with pytest.raises(ValueError, match="negative"):
        codec.entropy_encode_device(d_sym, [0, -1], counts, L, d_scr, d_out, d_sizes)
    with pytest.raises(ValueError):
        codec.entropy_scratch_bytes(counts, 6)
    with pytest.raises(ValueError):
        codec.entropy_scratch_bytes([5, 0], 4096)
    for bad in ([0, 10, 10, 4096], list(range(258)), [0, 1, (1 << 24) + 1]):
        with pytest.raises(ValueError):
            codec.entropy_set_table(bad)
    with pytest.raises(OverflowError):
        codec.entropy_set_table([0, 1, 1 << 32])
    with Codec(0, synthetic_params(0), SYNTH_MEAN, SYNTH_STD, patch_size=64, device=0) as fresh:
        with pytest.raises(ValueError, match="no entropy table"):
            fresh.entropy_encode_device(d_sym, offs, counts, L, d_scr, d_out, d_sizes)
        with pytest.raises(ValueError, match="no entropy table"):
            fresh.entropy_decode_device(d_out, [0], [30], [5], d_sym, [0], d_scr)
    codec.entropy_encode_device(d_sym, [], [], L, d_scr, d_out, d_sizes)  # n_streams == 0: nothing
    codec.entropy_decode_device(d_out, [], [], [], d_sym, [], d_scr)
    codec.synchronize()
    assert untouched()
    # the failed calls left the table in place (a rejected table does not replace it)
    codec.entropy_encode_device(d_sym, offs, counts, L, d_scr, d_out, d_sizes)
    sizes = d_sizes.download((2,), np.uint64)
    want = [entropy.pack(s, cum, segment=L) for s in streams]
    assert sizes.tolist() == [len(w) for w in want]
    assert d_out.download((int(sizes.sum()),), np.uint8).tobytes() == b"".join(want)
    for b in (d_sym, d_scr, d_out, d_sizes):
        b.free()


def test_stream_with_symbol_outside_the_table(codec):
    from tf_image_compression_amd import entropy
    cum = TABLES["total5000"]  # three symbols
    codec.entropy_set_table(cum)
    a, b, c = draw(cum, 5000, seed=1), draw(cum, 9000, seed=2), draw(cum, 70, seed=3)
    b[8191] = 3  # the table's symbol count, in the last symbol of the middle segment
    sizes, out = device_encode(codec, [a, b, c], 4096, "odd")
    wa, wc = entropy.pack(a, cum, segment=4096), entropy.pack(c, cum, segment=4096)
    assert sizes.tolist() == [len(wa), int(U64_MAX), len(wc)]
    assert out[:len(wa) + len(wc)] == wa + wc
    assert set(out[len(wa) + len(wc):]) == {0x5A}


def _images():
    out = []
    for k, (h, w) in enumerate([(70, 90), (64, 64), (130, 65)]):
        out.append(np.ascontiguousarray(structured_patches(1, 192, seed=300 + k)[0][:h, :w]))
    return out


def test_image_codec_streams(codec):
    from tf_image_compression_amd import entropy
    from tf_image_compression_amd.image_codec import ImageCodec
    cum = TABLES["p60"]
    ic = ImageCodec(codec)
    images = _images()
    sizes = [im.shape[:2] for im in images]
    symbols = ic.encode_images(images)
    streams = ic.encode_images_to_streams(images, cum, segment=64)
    assert len(streams) == 3
    for s, sym in zip(streams, symbols):
        assert entropy.parse(s) == (64, sym.size)
        assert np.array_equal(entropy.unpack(s, cum), sym.reshape(-1))
    want = ic.decode_images(symbols, sizes, post_filter=False)
    got = ic.decode_streams_to_images(streams, sizes, cum, post_filter=False)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))
    # host-packed containers of another segment length decode alike
    other = [entropy.pack(sym, cum, segment=4096) for sym in symbols]
    got = ic.decode_streams_to_images(other, sizes, cum, post_filter=False)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))
    res = ic.evaluate_images(images, post_filter=False, cum_freq=cum, entropy_segment=64)
    assert [r["coded_bytes"] for r in res] == [len(s) for s in streams]
    assert "coded_bytes" not in ic.evaluate_images(images, post_filter=False, cum_freq=cum)[0]
    with pytest.raises(ValueError, match="symbols"):
        ic.decode_streams_to_images(streams, [(64, 64)] * 3, cum, post_filter=False)
    with pytest.raises(ValueError, match="not a segmented stream"):
        ic.decode_streams_to_images([b"\x00" * 40] * 3, sizes, cum, post_filter=False)
    with pytest.raises(ValueError, match="outside the frequency table"):
        ic.encode_images_to_streams(images, [0, 4096], segment=64)  # one symbol only: symbol 1 is outside
    ic.close()


@pytest.mark.parametrize("model_num", ["0", "3"])
def test_cli_entropy_device(tmp_path, model_num):
    import decode
    import encode
    from tf_image_compression_amd import entropy, utils
    paths = []
    for k, im in enumerate(_images()):
        p = str(tmp_path / f"img{k}.png")
        utils.imsave(p, im)
        paths.append(p)
    lst = tmp_path / "list.txt"
    lst.write_text("\n".join(paths) + "\n")
    np.save(tmp_path / f"dist_{model_num}.npy", np.array([0.6, 0.4]))
    common = ["-m", model_num, "-g", "0", "--synthetic-weights", "--dist", str(tmp_path / "dist_{}.npy"),
              "--norm", "/nonexistent"]
    cfg = encode.load_config(model_num)
    dirs = {m: (str(tmp_path / f"enc_{m}"), str(tmp_path / f"rec_{m}")) for m in ("host", "device")}
    extra = {"host": ["--entropy", "host"], "device": ["--entropy", "device", "--batch-images", "4"]}
    for mode, (enc_dir, rec_dir) in dirs.items():
        seg = ["--segment", "64"] if mode == "device" else []
        eargs = encode.my_parse_args(common + extra[mode] + seg + ["-v", str(lst), "-o", enc_dir])
        encode.compress(encode.load_model(eargs, cfg), eargs)
        dargs = decode.my_parse_args(common + extra[mode] + ["-i", enc_dir, "-o", rec_dir])
        decode.uncompress(decode.load_model(dargs, cfg), dargs)
    files = sorted(os.listdir(dirs["host"][0]))
    assert len(files) == 3 and files == sorted(os.listdir(dirs["device"][0]))
    for f in files:
        data = open(os.path.join(dirs["device"][0], f), "rb").read()
        L, n = entropy.parse(data)
        assert L == 64 and n == decode.get_img_info(f, cfg)[0]
        assert not entropy.is_container(open(os.path.join(dirs["host"][0], f), "rb").read())
    pngs = sorted(os.listdir(dirs["host"][1]))
    assert len(pngs) == 3 and pngs == sorted(os.listdir(dirs["device"][1]))
    for f in pngs:
        assert open(os.path.join(dirs["host"][1], f), "rb").read() == open(os.path.join(dirs["device"][1], f), "rb").read()
    # the two cross-mode decodes
    dargs = decode.my_parse_args(common + ["--entropy", "host", "-i", dirs["device"][0], "-o", str(tmp_path / "x")])
    with pytest.raises(ValueError, match="--entropy device"):
        decode.uncompress(decode.load_model(dargs, cfg), dargs)
    dargs = decode.my_parse_args(common + ["--entropy", "device", "-i", dirs["host"][0], "-o", str(tmp_path / "y")])
    with pytest.raises(ValueError, match="not a segmented stream"):
        decode.uncompress(decode.load_model(dargs, cfg), dargs)
    for mod in (encode, decode):
        with pytest.raises(SystemExit):
            mod.my_parse_args(common + ["--entropy", "device", "--raw"])

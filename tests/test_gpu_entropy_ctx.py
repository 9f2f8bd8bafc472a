"""GPU tests of the context coder (csrc/tic_entropy.cpp, "TICS" version 2): byte parity of
tic_entropy_encode_ctx_device with the host container (entropy.pack under 2-D tables), symbol
parity of tic_entropy_decode_ctx_device with the host decoder, containers the header kernel must
reject, the argument contract, tic_histogram_ctx_device, and the layers above (ImageCodec streams,
evaluate_images, encode.py / decode.py --entropy device with a 2-D --dist)."""
import functools
import os
import struct

import numpy as np
import pytest

from entropy_ctx_cases import MIXED_TOTALS, draw_ctx, make_tables
from test_gpu_entropy import COUNTS_4, COUNTS_4096, _arena, _place

pytestmark = pytest.mark.gpu

# name -> (K, ncum, mixed totals).  K16384 * 3 words = 196 608 B: over the 64 KiB the kernels stage
# in LDS, so it runs the global-table kernels; every other case runs the LDS ones, K5000 (60 000 B)
# above the 48 KiB a kernel gets without asking.
CASES = {
    "K1": (1, 3, False),
    "K3": (3, 3, False),
    "K3_mixed": (3, 3, True),
    "K64": (64, 3, False),
    "K64_mixed": (64, 3, True),
    "K80": (80, 3, False),
    "K5_sym256": (5, 257, False),
    "K5000": (5000, 3, False),
    "K16384": (16384, 3, False),
}


@functools.lru_cache(maxsize=None)
def tables_of(name):
    K, ncum, mixed = CASES[name]
    t = make_tables(K, ncum, seed=sum(name.encode()), totals=MIXED_TOTALS if mixed else (4096,))
    t.setflags(write=False)
    return t


@pytest.fixture(scope="module")
def codec():
    from tf_image_compression_amd.codec import Codec
    from tf_image_compression_amd.weights import synthetic_params, SYNTH_MEAN, SYNTH_STD
    with Codec(0, synthetic_params(0), SYNTH_MEAN, SYNTH_STD, patch_size=64, quan_scale=2, device=0) as c:
        yield c


def device_encode(codec, streams, L, tables, layout="packed", slack=64):
    """(sizes uint64 [n], the whole d_out as bytes); d_out was filled with 0x5A."""
    from tf_image_compression_amd import entropy
    counts = [len(s) for s in streams]
    offs, size = _place(counts, layout)
    arena, _ = _arena(streams, offs, size, 0xA5)
    d_sym = codec.alloc(size)
    d_sym.upload(arena)
    cap = sum(entropy.bound(n, L, tables) for n in counts) + slack
    d_out, d_sizes = codec.alloc(cap), codec.alloc(8 * len(streams))
    d_scr = codec.alloc(codec.entropy_scratch_bytes(counts, L))
    codec.memset_device(d_out, 0x5A, cap)
    codec.memset_device(d_sizes, 0x5A, 8 * len(streams))
    codec.entropy_encode_ctx_device(d_sym, offs, counts, L, d_scr, d_out, d_sizes)
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
    codec.entropy_decode_ctx_device(d_blob, boffs, [len(b) for b in blobs], counts, d_sym, soffs, d_scr)
    got = d_sym.download((ssize,), np.uint8)
    for b in (d_blob, d_sym, d_scr):
        b.free()
    used = np.zeros(ssize, bool)
    for o, n in zip(soffs, counts):
        used[o:o + n] = True
    assert np.all(got[~used] == 0xA5), "bytes outside the streams were written"
    return [got[o:o + n] for o, n in zip(soffs, counts)]


@pytest.mark.parametrize("L,counts", [(4096, COUNTS_4096), (4, COUNTS_4)], ids=["L4096", "L4"])
@pytest.mark.parametrize("name", list(CASES))
def test_encode_matches_host_container(codec, name, L, counts):
    from tf_image_compression_amd import entropy
    tables = tables_of(name)
    codec.entropy_set_tables(tables)
    streams = [draw_ctx(tables, n, seed=1000 + n) for n in counts]
    want = [entropy.pack(s, tables, segment=L) for s in streams]
    blob = b"".join(want)
    first = None
    for layout in ("packed", "odd", "reversed", "packed"):
        sizes, out = device_encode(codec, streams, L, tables, layout)
        assert sizes.tolist() == [len(w) for w in want], layout
        assert out[:len(blob)] == blob, layout
        assert set(out[len(blob):]) == {0x5A}, "bytes behind the last container were written"
        if layout == "packed":  # two identical calls: identical bytes
            assert first is None or first == out
            first = out


@pytest.mark.parametrize("L,counts", [(4096, COUNTS_4096), (4, COUNTS_4)], ids=["L4096", "L4"])
@pytest.mark.parametrize("name", list(CASES))
def test_decode_matches_host(codec, name, L, counts):
    from tf_image_compression_amd import entropy
    tables = tables_of(name)
    K, ncum, _ = CASES[name]
    codec.entropy_set_tables(tables)
    streams = [draw_ctx(tables, n, seed=2000 + n) for n in counts]
    blobs = [entropy.pack(s, tables, segment=L) for s in streams]
    for layout in ("packed", "odd", "reversed"):
        got = device_decode(codec, blobs, counts, L, layout)
        for g, s in zip(got, streams):
            assert np.array_equal(g, s), (layout, len(s))
    # device -> device
    sizes, out = device_encode(codec, streams, L, tables, "odd")
    cuts = np.concatenate([[0], np.cumsum(sizes.astype(np.int64))])
    dev_blobs = [out[cuts[i]:cuts[i + 1]] for i in range(len(streams))]
    for g, s in zip(device_decode(codec, dev_blobs, counts, L, "reversed"), streams):
        assert np.array_equal(g, s)
    # containers the header kernel rejects: exactly counts[i] zeros each, the neighbour untouched
    n, blob = counts[-1], blobs[-1]
    S = -(-n // L)
    wrong_k = blob[:20] + struct.pack("<I", K + 1) + blob[24:]
    wrong_crc = blob[:24] + bytes([blob[24] ^ 0x40]) + blob[25:]
    version_1 = entropy.pack(streams[-1], tables[0], segment=L)
    cut_lens = blob[:28 + 2 * S - 1]
    bad = [wrong_k, wrong_crc, version_1, cut_lens]
    got = device_decode(codec, bad + [blobs[0]], [n] * 4 + [counts[0]], L, "odd")
    for g in got[:4]:
        assert g.size == n and not g.any()
    assert np.array_equal(got[4], streams[0])
    # payload bits flipped, header and lengths intact: input the decoder is specified for (zero
    # padding past a segment's end, extents clamped); the symbols are in range and the host's
    rng = np.random.default_rng(99)
    noisy = []
    for b, cnt in zip(blobs, counts):
        a = np.frombuffer(b, np.uint8).copy()
        head = 28 + 2 * -(-cnt // L)
        if a.size > head:
            at = rng.integers(head, a.size, size=max(1, (a.size - head) // 16))
            a[at] ^= (1 << rng.integers(0, 8, size=at.size)).astype(np.uint8)
        noisy.append(a.tobytes())
    want = [entropy.unpack(b, tables, n=cnt) for b, cnt in zip(noisy, counts)]
    got = device_decode(codec, noisy, counts, L, "odd")
    for g, w in zip(got, want):
        assert int(g.max()) < ncum - 1
        assert np.array_equal(g, w)


def test_stream_with_symbol_outside_the_tables(codec):
    """A symbol >= ncum - 1 marks its stream with UINT64_MAX and leaves its neighbours' containers
    as they are, under tables in LDS and in global memory."""
    from tf_image_compression_amd import entropy
    for name in ("K80", "K16384"):
        tables = tables_of(name)
        codec.entropy_set_tables(tables)
        a, b, c = draw_ctx(tables, 5000, seed=1), draw_ctx(tables, 9000, seed=2), draw_ctx(tables, 70, seed=3)
        b[8191] = 2  # the tables' symbol count, in the last symbol of the middle segment
        sizes, out = device_encode(codec, [a, b, c], 4096, tables, "odd")
        wa, wc = entropy.pack(a, tables, segment=4096), entropy.pack(c, tables, segment=4096)
        assert sizes.tolist() == [len(wa), int(np.iinfo(np.uint64).max), len(wc)], name
        assert out[:len(wa) + len(wc)] == wa + wc
        assert set(out[len(wa) + len(wc):]) == {0x5A}
        with pytest.raises(ValueError, match="outside the table"):
            entropy.pack(b, tables, segment=4096)


def test_argument_contract(codec):
    import ctypes as C
    from tf_image_compression_amd import entropy
    from tf_image_compression_amd._lib import lib
    from tf_image_compression_amd.codec import Codec
    from tf_image_compression_amd.weights import synthetic_params, SYNTH_MEAN, SYNTH_STD
    tables = tables_of("K80")
    table_v1 = [0, 2457, 4096]
    counts, L = [100, 4097], 4096
    streams = [draw_ctx(tables, n, seed=n) for n in counts]
    d_sym = codec.alloc(sum(counts))
    d_sym.upload(np.concatenate(streams))
    offs = [0, 100]
    need = codec.entropy_scratch_bytes(counts, L)
    cap = sum(entropy.bound(n, L, tables) for n in counts)
    d_scr, d_out, d_sizes = codec.alloc(need), codec.alloc(cap), codec.alloc(16)

    def untouched():
        return (set(d_out.download((cap,), np.uint8).tolist()) == {0x5A}
                and set(d_sizes.download((16,), np.uint8).tolist()) == {0x5A})

    codec.memset_device(d_out, 0x5A, cap)
    codec.memset_device(d_sizes, 0x5A, 16)
    with Codec(0, synthetic_params(0), SYNTH_MEAN, SYNTH_STD, patch_size=64, device=0) as fresh:
        fresh.entropy_set_table(table_v1)  # the version-1 table is not the context tables
        with pytest.raises(ValueError, match="no context tables"):
            fresh.entropy_encode_ctx_device(d_sym, offs, counts, L, d_scr, d_out, d_sizes)
        with pytest.raises(ValueError, match="no context tables"):
            fresh.entropy_decode_ctx_device(d_out, [0], [40], [5], d_sym, [0], d_scr)
    codec.entropy_set_table(table_v1)
    codec.entropy_set_tables(tables)
    with pytest.raises(ValueError, match="scratch"):
        codec.entropy_encode_ctx_device(d_sym, offs, counts, L, d_scr, d_out, d_sizes, scratch_bytes=need - 1)
    with pytest.raises(ValueError, match="out_cap"):
        codec.entropy_encode_ctx_device(d_sym, offs, counts, L, d_scr, d_out, d_sizes, out_cap=cap - 1)
    with pytest.raises(ValueError, match="scratch"):
        codec.entropy_decode_ctx_device(d_out, [0, 50], [50, 50], counts, d_sym, offs, d_scr, scratch_bytes=16)
    with pytest.raises(ValueError, match="segment length"):
        codec.entropy_encode_ctx_device(d_sym, offs, counts, 6, d_scr, d_out, d_sizes)
    i64 = C.POINTER(C.c_int64)
    o = np.asarray(offs, np.int64).ctypes.data_as(i64)
    c = np.asarray(counts, np.int64).ctypes.data_as(i64)
    for nulls in ((None, d_scr.ptr, d_out.ptr, d_sizes.ptr), (d_sym.ptr, None, d_out.ptr, d_sizes.ptr),
                  (d_sym.ptr, d_scr.ptr, None, d_sizes.ptr), (d_sym.ptr, d_scr.ptr, d_out.ptr, None)):
        s, scr, out, sz = nulls
        assert lib().tic_entropy_encode_ctx_device(codec._h, s, o, c, 2, L, scr, need, out, cap, sz) == -1
    assert lib().tic_entropy_encode_ctx_device(codec._h, d_sym.ptr, None, c, 2, L, d_scr.ptr, need, d_out.ptr, cap,
                                               d_sizes.ptr) == -1
    assert lib().tic_entropy_decode_ctx_device(codec._h, None, o, c, c, 2, d_sym.ptr, o, d_scr.ptr, need) == -1
    assert lib().tic_entropy_decode_ctx_device(codec._h, d_out.ptr, o, c, c, 2, None, o, d_scr.ptr, need) == -1
    assert lib().tic_entropy_decode_ctx_device(codec._h, d_out.ptr, o, c, c, 2, d_sym.ptr, o, None, need) == -1
    assert lib().tic_histogram_ctx_device(codec._h, None, 8, 2, 4, d_out.ptr) == -1
    assert lib().tic_histogram_ctx_device(codec._h, d_sym.ptr, 8, 2, 0, d_out.ptr) == -1
    assert lib().tic_histogram_ctx_device(codec._h, d_sym.ptr, 8, 2, 65537, d_out.ptr) == -1
    for bad in ([[0, 10, 10]], [[0, 5, 9], [0, 5, 1 << 25]], [[1, 2, 3]], np.zeros((0, 3), np.int64)):
        with pytest.raises(ValueError):
            codec.entropy_set_tables(bad)
    with pytest.raises(OverflowError):
        codec.entropy_set_tables([[0, 1, 1 << 32]])
    codec.entropy_encode_ctx_device(d_sym, [], [], L, d_scr, d_out, d_sizes)  # n_streams == 0: nothing
    codec.entropy_decode_ctx_device(d_out, [], [], [], d_sym, [], d_scr)
    codec.synchronize()
    assert untouched()
    # the failed calls left the tables in place, and the version-1 entries still use set_table's table
    codec.entropy_encode_ctx_device(d_sym, offs, counts, L, d_scr, d_out, d_sizes)
    sizes = d_sizes.download((2,), np.uint64)
    want = [entropy.pack(s, tables, segment=L) for s in streams]
    assert sizes.tolist() == [len(w) for w in want]
    assert d_out.download((int(sizes.sum()),), np.uint8).tobytes() == b"".join(want)
    codec.entropy_encode_device(d_sym, offs, counts, L, d_scr, d_out, d_sizes)
    sizes = d_sizes.download((2,), np.uint64)
    want = [entropy.pack(s, table_v1, segment=L) for s in streams]
    assert sizes.tolist() == [len(w) for w in want]
    assert d_out.download((int(sizes.sum()),), np.uint8).tobytes() == b"".join(want)
    # smaller tables after larger ones reuse the buffer; larger ones replace it
    for name in ("K3", "K16384", "K64"):
        t = tables_of(name)
        codec.entropy_set_tables(t)
        codec.entropy_encode_ctx_device(d_sym, offs, counts, L, d_scr, d_out, d_sizes)
        sizes = d_sizes.download((2,), np.uint64)
        want = [entropy.pack(s, t, segment=L) for s in streams]
        assert d_out.download((int(sizes.sum()),), np.uint8).tobytes() == b"".join(want), name
    for b in (d_sym, d_scr, d_out, d_sizes):
        b.free()


@pytest.mark.parametrize("K", [64, 80, 1024])
def test_histogram_ctx(codec, K):
    n, Q = 2 * 4 * 4 * K, 2
    rng = np.random.default_rng(K)
    bias = rng.random(K)
    sym = (rng.random(n) < bias[np.arange(n) % K]).astype(np.uint8)
    want = np.stack([np.bincount(sym[k::K], minlength=Q) for k in range(K)]).astype(np.uint64)
    d_sym, d_cnt = codec.alloc(n + 3), codec.alloc(8 * K * Q + 8)
    codec.memset_device(d_cnt, 0, 8 * K * Q)
    codec.memset_device(d_cnt.view(8 * K * Q), 0x5A, 8)
    d_sym.upload(np.concatenate([[7], sym, [7, 7]]).astype(np.uint8))  # d_sym of any alignment
    codec.histogram_ctx_device(d_sym.view(1), n, Q, K, d_cnt)
    assert np.array_equal(d_cnt.download((K, Q), np.uint64), want)
    codec.histogram_ctx_device(d_sym.view(1), n, Q, K, d_cnt)  # accumulates
    assert np.array_equal(d_cnt.download((K, Q), np.uint64), 2 * want)
    # a count that ends inside the period, and np.histogram's closed last bin (v == Q counts in Q - 1)
    m = n - K // 2 - 1
    codec.memset_device(d_cnt, 0, 8 * K * Q)
    edge = sym[:m].copy()
    edge[5], edge[6] = Q, Q + 1
    d_sym.upload(edge)
    codec.histogram_ctx_device(d_sym, m, Q, K, d_cnt)
    ref = edge.copy()
    ref[5] = Q - 1
    keep = np.arange(m) != 6
    want = np.stack([np.bincount(ref[k::K][keep[k::K]], minlength=Q) for k in range(K)]).astype(np.uint64)
    assert np.array_equal(d_cnt.download((K, Q), np.uint64), want)
    assert set(d_cnt.download((8 * K * Q + 8,), np.uint8)[-8:].tolist()) == {0x5A}
    d_sym.free()
    d_cnt.free()


def _images():
    from conftest import structured_patches
    out = []
    for k, (h, w) in enumerate([(64, 64), (96, 64), (70, 50)]):
        out.append(np.ascontiguousarray(structured_patches(1, 128, seed=400 + k)[0][:h, :w]))
    return out


def _tables_from(symbols, C_):
    """(global table, per-channel tables) from the symbols' own histograms."""
    from tf_image_compression_amd.range_coder import symbol_table, symbol_tables
    allsym = np.concatenate([s.reshape(-1, C_) for s in symbols])
    per = np.stack([np.bincount(allsym[:, c], minlength=2) for c in range(C_)]).astype(np.float64)
    glob = per.sum(axis=0)
    return (symbol_table(glob / glob.sum(), resolution=4096),
            symbol_tables(per / per.sum(axis=1, keepdims=True), resolution=4096), glob, per)


def test_image_codec_context_streams(codec):
    from tf_image_compression_amd import entropy
    from tf_image_compression_amd.evaluate import estimated_bits_ctx
    from tf_image_compression_amd.image_codec import ImageCodec
    ic = ImageCodec(codec)
    images = _images()
    sizes = [im.shape[:2] for im in images]
    symbols = ic.encode_images(images)
    C_ = codec.code_shape[2]
    table, tables, _, _ = _tables_from(symbols, C_)
    flat = ic.encode_images_to_streams(images, table, segment=2048)
    ctx = ic.encode_images_to_streams(images, tables, segment=2048)
    for s, sym in zip(ctx, symbols):
        assert entropy.parse_ctx(s) == (2048, sym.size, C_, entropy.tables_crc(tables))
        assert s == entropy.pack(sym, tables, segment=2048)
    print(f"single table {sum(map(len, flat))} B, per-channel tables {sum(map(len, ctx))} B")
    assert sum(map(len, ctx)) < sum(map(len, flat))
    want = ic.decode_streams_to_images(flat, sizes, table, post_filter=False)
    got = ic.decode_streams_to_images(ctx, sizes, tables, post_filter=False)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))
    res = ic.evaluate_images(images, post_filter=False, cum_freq=tables, entropy_segment=2048)
    assert [r["coded_bytes"] for r in res] == [len(s) for s in ctx]
    for r, sym in zip(res, symbols):
        per = np.stack([np.bincount(sym.reshape(-1, C_)[:, c], minlength=2) for c in range(C_)])
        est = estimated_bits_ctx(per, tables)
        assert abs(r["est_bits"] - est) <= 1e-9 * est
        assert np.array_equal(r["counts"], per.sum(axis=0))
    assert "coded_bytes" not in ic.evaluate_images(images, post_filter=False, cum_freq=tables)[0]
    other = tables.copy()
    other[3, 1] += 1
    with pytest.raises(ValueError, match="other context tables"):
        ic.decode_streams_to_images(ctx, sizes, other, post_filter=False)
    with pytest.raises(ValueError, match="version 1"):
        ic.decode_streams_to_images(flat, sizes, tables, post_filter=False)
    with pytest.raises(ValueError, match="version 2"):
        ic.decode_streams_to_images(ctx, sizes, table, post_filter=False)
    ic.close()


def test_get_encoded_distribution_contexts(codec, tmp_path):
    """get_encoded_distribution.py --context on 66 PNG patches (two batches of <= 64): the per-context
    counts equal numpy's on the encoder's symbols, for one table per channel and one per position."""
    import get_encoded_distribution as ged
    from PIL import Image
    from conftest import structured_patches
    pats = structured_patches(66, 64, seed=21)
    paths = []
    for i, p in enumerate(pats):
        f = str(tmp_path / f"p{i}.png")
        Image.fromarray(p).save(f)
        paths.append(f)
    sym = codec.encode(pats)
    for mode in ("channel", "position"):
        K = ged.context_count(mode, codec.code_shape)
        freq, ctx_freq = ged.encoded_context_frequencies(codec, ged.patch_batches(paths, 64), 2, K)
        folded = sym.reshape(-1, K)
        want = np.stack([(folded == q).sum(axis=0) for q in range(2)], axis=1)
        assert np.array_equal(ctx_freq, want.astype(np.float64)), mode
        assert np.array_equal(freq, want.sum(axis=0).astype(np.float64))


def test_cli_context_distribution(tmp_path):
    import decode
    import encode
    from tf_image_compression_amd import entropy, utils
    from test_gpu_entropy import _images as cli_images
    paths = []
    for k, im in enumerate(cli_images()):
        p = str(tmp_path / f"img{k}.png")
        utils.imsave(p, im)
        paths.append(p)
    lst = tmp_path / "list.txt"
    lst.write_text("\n".join(paths) + "\n")
    rng = np.random.default_rng(5)
    p1 = rng.random(64) ** 3
    np.save(tmp_path / "flat_0.npy", np.array([0.6, 0.4]))
    np.save(tmp_path / "ctx_0.npy", np.stack([1 - p1, p1], axis=1))
    cfg = encode.load_config("0")
    dirs = {}
    for mode in ("flat", "ctx"):
        common = ["-m", "0", "-g", "0", "--synthetic-weights", "--dist", str(tmp_path / (mode + "_{}.npy")),
                  "--norm", "/nonexistent", "--entropy", "device", "--batch-images", "4"]
        enc_dir, rec_dir = str(tmp_path / f"enc_{mode}"), str(tmp_path / f"rec_{mode}")
        eargs = encode.my_parse_args(common + ["--segment", "64", "-v", str(lst), "-o", enc_dir])
        encode.compress(encode.load_model(eargs, cfg), eargs)
        dargs = decode.my_parse_args(common + ["-i", enc_dir, "-o", rec_dir])
        decode.uncompress(decode.load_model(dargs, cfg), dargs)
        dirs[mode] = (enc_dir, rec_dir, common)
    files = sorted(os.listdir(dirs["flat"][0]))
    assert len(files) == 3 and files == sorted(os.listdir(dirs["ctx"][0]))
    for f in files:
        data = open(os.path.join(dirs["ctx"][0], f), "rb").read()
        L, n, K, _ = entropy.parse_ctx(data)
        assert (L, n, K) == (64, decode.get_img_info(f, cfg)[0], 64)
        assert entropy.container_version(open(os.path.join(dirs["flat"][0], f), "rb").read()) == 1
    pngs = sorted(os.listdir(dirs["flat"][1]))
    assert len(pngs) == 3 and pngs == sorted(os.listdir(dirs["ctx"][1]))
    for f in pngs:
        assert open(os.path.join(dirs["flat"][1], f), "rb").read() == open(os.path.join(dirs["ctx"][1], f), "rb").read()
    # a file's version byte against the table given
    dargs = decode.my_parse_args(dirs["flat"][2] + ["-i", dirs["ctx"][0], "-o", str(tmp_path / "x")])
    with pytest.raises(ValueError, match="version-2"):
        decode.uncompress(decode.load_model(dargs, cfg), dargs)
    dargs = decode.my_parse_args(dirs["ctx"][2] + ["-i", dirs["flat"][0], "-o", str(tmp_path / "y")])
    with pytest.raises(ValueError, match="version-1"):
        decode.uncompress(decode.load_model(dargs, cfg), dargs)

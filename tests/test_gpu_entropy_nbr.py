"""GPU tests of the neighbour coder (csrc/tic_entropy.cpp, "TICS" version 3): byte parity of
tic_entropy_encode_nbr_device with the host container (entropy.pack under 3-D tables), symbol
parity of tic_entropy_decode_nbr_device with the host decoder, containers the header kernel must
reject, the argument contract, tic_histogram_nbr_device, and the layers above (ImageCodec streams,
evaluate_images, encode.py / decode.py --entropy device with a 3-D --dist)."""
import functools
import os
import struct

import numpy as np
import pytest

from entropy_ctx_cases import MIXED_TOTALS
from entropy_nbr_cases import draw, make_nbr_tables, nb_rows_np
from test_gpu_entropy import _arena, _place

pytestmark = pytest.mark.gpu

# name -> (eh, ew, C, K0, neighbours, ncum, mixed totals, [L]).  Table bytes are K0 * M * ncum * 4:
# pos_global (590 KB) runs the global-table kernels, every other case the LDS ones; lds_56k and
# lds_54k_n2 lie between the 48 KiB a kernel gets without asking and the 64 KiB staged at most.
CASES = {
    "g2x3x4_n1": (2, 3, 4, 4, 1, 3, False, (4, 8, 16)),
    "g2x3x4_n2": (2, 3, 4, 4, 2, 3, True, (4, 8, 16)),
    "g2x2x3_n2": (2, 2, 3, 3, 2, 3, False, (4, 8, 16)),        # C not a multiple of 4
    "g2x2x3_k1": (2, 2, 3, 1, 1, 3, True, (4, 16)),
    "g4x4x64_n2": (4, 4, 64, 64, 2, 3, False, (16, 2048)),      # a segment spans two patches
    "g8x8x80_n1": (8, 8, 80, 80, 1, 3, False, (2048,)),         # segments straddle patches
    "g8x8x80_n2": (8, 8, 80, 80, 2, 3, True, (2048,)),
    "g16x16x64_n1": (16, 16, 64, 64, 1, 3, False, (2048, 4096)),
    "g16x16x64_n2": (16, 16, 64, 64, 2, 3, True, (2048, 4096)),
    "sym256_n2": (4, 4, 64, 4, 2, 257, False, (2048,)),         # class(s) is not the symbol
    "lds_56k": (16, 16, 64, 1600, 1, 3, False, (2048,)),        # 1600 * 3 * 3 * 4 = 57 600 B, K0 not a divisor of anything
    "lds_54k_n2": (16, 16, 64, 500, 2, 3, True, (2048,)),       # 500 * 9 * 3 * 4 = 54 000 B beside 8 KiB of rings
    "pos_global": (16, 16, 64, 16384, 1, 3, False, (2048,)),    # 589 824 B of tables: global-memory kernels
    "far_row": (2, 300, 64, 64, 2, 3, False, (4096, 16384)),    # ew * C = 19 200 > any L: N never inside a segment
    "long_row": (2, 250, 64, 64, 2, 3, False, (16384,)),        # ew * C = 16 000 bits of ring: 125 KiB, over the LDS budget
}


@functools.lru_cache(maxsize=None)
def tables_of(name):
    eh, ew, C_, K0, nbrs, ncum, mixed, _ = CASES[name]
    t = make_nbr_tables(K0, nbrs, ncum, seed=sum(name.encode()), totals=MIXED_TOTALS if mixed else (4096,))
    t.setflags(write=False)
    return t


def counts_for(name, L):
    eh, ew, C_ = CASES[name][:3]
    patch = eh * ew * C_
    big = 2 * max(L, min(patch, 20000)) + 7
    return [1, L - 1, L, L + 1, big, 3 * L + 2]


def cases_with_L():
    return [(name, L) for name in CASES for L in CASES[name][7]]


@pytest.fixture(scope="module")
def codec():
    from tf_image_compression_amd.codec import Codec
    from tf_image_compression_amd.weights import synthetic_params, SYNTH_MEAN, SYNTH_STD
    with Codec(0, synthetic_params(0), SYNTH_MEAN, SYNTH_STD, patch_size=64, quan_scale=2, device=0) as c:
        yield c


def device_encode(codec, streams, L, tables, layout="packed", slack=64):
    """(sizes uint64 [n], the whole d_out as bytes); d_out and the scratch were filled with a poison byte."""
    from tf_image_compression_amd import entropy
    counts = [len(s) for s in streams]
    offs, size = _place(counts, layout)
    arena, _ = _arena(streams, offs, size, 0xA5)
    d_sym = codec.alloc(size)
    d_sym.upload(arena)
    cap = sum(entropy.bound(n, L, tables) for n in counts) + slack
    d_out, d_sizes = codec.alloc(cap), codec.alloc(8 * len(streams))
    need = codec.entropy_scratch_bytes(counts, L)
    d_scr = codec.alloc(need)
    codec.memset_device(d_out, 0x5A, cap)
    codec.memset_device(d_sizes, 0x5A, 8 * len(streams))
    codec.memset_device(d_scr, 0xC3, need)
    codec.entropy_encode_nbr_device(d_sym, offs, counts, L, d_scr, d_out, d_sizes)
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
    need = codec.entropy_scratch_bytes(counts, L)
    d_scr = codec.alloc(need)
    codec.memset_device(d_scr, 0xC3, need)
    codec.entropy_decode_nbr_device(d_blob, boffs, [len(b) for b in blobs], counts, d_sym, soffs, d_scr)
    got = d_sym.download((ssize,), np.uint8)
    for b in (d_blob, d_sym, d_scr):
        b.free()
    used = np.zeros(ssize, bool)
    for o, n in zip(soffs, counts):
        used[o:o + n] = True
    assert np.all(got[~used] == 0xA5), "bytes outside the streams were written"
    return [got[o:o + n] for o, n in zip(soffs, counts)]


@functools.lru_cache(maxsize=None)
def host_side(name, L):
    """(streams, host containers) of a case, computed once for the encode and the decode test."""
    from tf_image_compression_amd import entropy
    eh, ew, C_, K0, nbrs, ncum, _, _ = CASES[name]
    tables = tables_of(name)
    streams = [draw(n, ncum - 1, seed=1000 + n) for n in counts_for(name, L)]
    blobs = [entropy.pack(s, tables, segment=L, geometry=(eh, ew, C_)) for s in streams]
    return streams, blobs


@pytest.mark.parametrize("name,L", cases_with_L())
def test_encode_matches_host_container(codec, name, L):
    geo, tables = CASES[name][:3], tables_of(name)
    codec.entropy_set_tables_nbr(tables, geo)
    streams, want = host_side(name, L)
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


@pytest.mark.parametrize("name,L", cases_with_L())
def test_decode_matches_host(codec, name, L):
    from tf_image_compression_amd import entropy
    eh, ew, C_, K0, nbrs, ncum, _, _ = CASES[name]
    geo, tables = (eh, ew, C_), tables_of(name)
    codec.entropy_set_tables_nbr(tables, geo)
    streams, blobs = host_side(name, L)
    counts = [len(s) for s in streams]
    first = None
    for layout in ("packed", "odd", "reversed", "packed"):
        got = device_decode(codec, blobs, counts, L, layout)
        for g, s in zip(got, streams):
            assert np.array_equal(g, s), (layout, len(s))
        if layout == "packed":
            assert first is None or all(np.array_equal(a, b) for a, b in zip(first, got))
            first = got
    # containers the header kernel rejects: exactly counts[i] zeros each, the neighbour untouched
    n, blob = counts[-1], blobs[-1]
    S = -(-n // L)

    def patched(at, data):
        return blob[:at] + data + blob[at + len(data):]

    bad = [patched(4, b"\x02"), patched(20, struct.pack("<I", K0 + 1)), patched(24, bytes([blob[24] ^ 0x40])),
           patched(28, struct.pack("<H", eh + 1)), patched(30, struct.pack("<H", ew + 1)),
           patched(32, struct.pack("<H", C_ + 1)), patched(34, bytes([3 - nbrs])), patched(35, b"\x01"),
           patched(12, struct.pack("<Q", n + 1)), blob[:36 + 2 * S - 1]]
    got = device_decode(codec, bad + [blobs[3]], [n] * len(bad) + [counts[3]], L, "odd")
    for g in got[:-1]:
        assert g.size == n and not g.any()
    assert np.array_equal(got[-1], streams[3])
    # payloads replaced by pseudo-random bytes, header and lengths intact: garbage in still gives a
    # defined result (zero padding past a segment's end, extents clamped), and it is the host's
    rng = np.random.default_rng(99)
    noisy = []
    for b, cnt in zip(blobs, counts):
        a = np.frombuffer(b, np.uint8).copy()
        head = 36 + 2 * -(-cnt // L)
        a[head:] = rng.integers(0, 256, size=a.size - head, dtype=np.uint8)
        noisy.append(a.tobytes())
    want = [entropy.unpack(b, tables, n=cnt, geometry=geo) for b, cnt in zip(noisy, counts)]
    got = device_decode(codec, noisy, counts, L, "odd")
    for g, w in zip(got, want):
        assert int(g.max()) < ncum - 1
        assert np.array_equal(g, w)


def test_stream_with_symbol_outside_the_tables(codec):
    from tf_image_compression_amd import entropy
    for name in ("g8x8x80_n2", "pos_global"):
        geo, tables = CASES[name][:3], tables_of(name)
        codec.entropy_set_tables_nbr(tables, geo)
        a, b, c = draw(5000, 2, seed=1), draw(9000, 2, seed=2), draw(70, 2, seed=3)
        b[4095] = 2  # the tables' symbol count, in the last symbol of a segment
        sizes, out = device_encode(codec, [a, b, c], 2048, tables, "odd")
        wa, wc = (entropy.pack(s, tables, segment=2048, geometry=geo) for s in (a, c))
        assert sizes.tolist() == [len(wa), int(np.iinfo(np.uint64).max), len(wc)], name
        assert out[:len(wa) + len(wc)] == wa + wc
        assert set(out[len(wa) + len(wc):]) == {0x5A}


def test_argument_contract(codec):
    import ctypes as C
    from tf_image_compression_amd import entropy
    from tf_image_compression_amd._lib import lib
    from tf_image_compression_amd.codec import Codec
    from tf_image_compression_amd.weights import synthetic_params, SYNTH_MEAN, SYNTH_STD
    name = "g8x8x80_n2"
    geo, tables = CASES[name][:3], tables_of(name)
    counts, L = [100, 4097], 2048
    streams = [draw(n, 2, seed=n) for n in counts]
    d_sym = codec.alloc(sum(counts))
    d_sym.upload(np.concatenate(streams))
    offs = [0, 100]
    need = codec.entropy_scratch_bytes(counts, L)
    cap = sum(entropy.bound(n, L, tables) for n in counts)
    d_scr, d_out, d_sizes = codec.alloc(need), codec.alloc(cap), codec.alloc(16)
    d_cnt = codec.alloc(8 * 80 * 9 * 2)
    codec.memset_device(d_out, 0x5A, cap)
    codec.memset_device(d_sizes, 0x5A, 16)
    with Codec(0, synthetic_params(0), SYNTH_MEAN, SYNTH_STD, patch_size=64, device=0) as fresh:
        fresh.entropy_set_table([0, 2457, 4096])
        fresh.entropy_set_tables(tables[:, 0])  # version-2 tables are not neighbour tables
        with pytest.raises(ValueError, match="no neighbour tables"):
            fresh.entropy_encode_nbr_device(d_sym, offs, counts, L, d_scr, d_out, d_sizes)
        with pytest.raises(ValueError, match="no neighbour tables"):
            fresh.entropy_decode_nbr_device(d_out, [0], [40], [5], d_sym, [0], d_scr)
        with pytest.raises(ValueError, match="no neighbour tables"):
            fresh.histogram_nbr_device(d_sym, offs, counts, 2, L, d_cnt)
        fresh.entropy_set_tables_nbr(tables)  # the codec's own code shape
        with pytest.raises(ValueError, match="no context tables"):  # and the other way round
            fresh.entropy_encode_ctx_device(d_sym, offs, counts, L, d_scr, d_out, d_sizes)
    codec.entropy_set_tables_nbr(tables, geo)
    with pytest.raises(ValueError, match="scratch"):
        codec.entropy_encode_nbr_device(d_sym, offs, counts, L, d_scr, d_out, d_sizes, scratch_bytes=need - 1)
    with pytest.raises(ValueError, match="out_cap"):
        codec.entropy_encode_nbr_device(d_sym, offs, counts, L, d_scr, d_out, d_sizes, out_cap=cap - 1)
    with pytest.raises(ValueError, match="scratch"):
        codec.entropy_decode_nbr_device(d_out, [0, 50], [50, 50], counts, d_sym, offs, d_scr, scratch_bytes=16)
    for bad_L in (6, 0, 16388):
        with pytest.raises(ValueError, match="segment length"):
            codec.entropy_encode_nbr_device(d_sym, offs, counts, bad_L, d_scr, d_out, d_sizes)
        with pytest.raises(ValueError, match="segment length"):
            codec.histogram_nbr_device(d_sym, offs, counts, 2, bad_L, d_cnt)
    i64 = C.POINTER(C.c_int64)
    o = np.asarray(offs, np.int64).ctypes.data_as(i64)
    c = np.asarray(counts, np.int64).ctypes.data_as(i64)
    for nulls in ((None, d_scr.ptr, d_out.ptr, d_sizes.ptr), (d_sym.ptr, None, d_out.ptr, d_sizes.ptr),
                  (d_sym.ptr, d_scr.ptr, None, d_sizes.ptr), (d_sym.ptr, d_scr.ptr, d_out.ptr, None)):
        s, scr, out, sz = nulls
        assert lib().tic_entropy_encode_nbr_device(codec._h, s, o, c, 2, L, scr, need, out, cap, sz) == -1
    assert lib().tic_entropy_encode_nbr_device(codec._h, d_sym.ptr, None, c, 2, L, d_scr.ptr, need, d_out.ptr, cap,
                                               d_sizes.ptr) == -1
    assert lib().tic_entropy_encode_nbr_device(None, d_sym.ptr, o, c, 2, L, d_scr.ptr, need, d_out.ptr, cap,
                                               d_sizes.ptr) == -1
    assert lib().tic_entropy_decode_nbr_device(codec._h, None, o, c, c, 2, d_sym.ptr, o, d_scr.ptr, need) == -1
    assert lib().tic_entropy_decode_nbr_device(codec._h, d_out.ptr, o, c, c, 2, None, o, d_scr.ptr, need) == -1
    assert lib().tic_entropy_decode_nbr_device(codec._h, d_out.ptr, o, c, c, 2, d_sym.ptr, o, None, need) == -1
    assert lib().tic_histogram_nbr_device(codec._h, None, o, c, 2, 2, L, d_cnt.ptr) == -1
    assert lib().tic_histogram_nbr_device(codec._h, d_sym.ptr, o, c, 2, 2, L, None) == -1
    assert lib().tic_histogram_nbr_device(codec._h, d_sym.ptr, None, c, 2, 2, L, d_cnt.ptr) == -1
    assert lib().tic_histogram_nbr_device(codec._h, d_sym.ptr, o, c, 2, 0, L, d_cnt.ptr) == -1
    assert lib().tic_entropy_set_tables_nbr(None, None, 1, 1, 3, 1, 1, 1) == -1
    for bad in ([[[0, 10, 10]] * 3], [[[0, 5, 9]] * 2 + [[0, 5, 1 << 25]]], [[[1, 2, 3]] * 3]):
        with pytest.raises(ValueError):
            codec.entropy_set_tables_nbr(bad, geo)
    with pytest.raises(ValueError, match="geometry"):
        codec.entropy_set_tables_nbr(tables, (8, 0, 80))
    with pytest.raises(OverflowError):
        codec.entropy_set_tables_nbr([[[0, 1, 1 << 32]] * 3], geo)
    codec.entropy_encode_nbr_device(d_sym, [], [], L, d_scr, d_out, d_sizes)  # n_streams == 0: nothing
    codec.entropy_decode_nbr_device(d_out, [], [], [], d_sym, [], d_scr)
    codec.synchronize()
    assert set(d_out.download((cap,), np.uint8).tolist()) == {0x5A}
    assert set(d_sizes.download((16,), np.uint8).tolist()) == {0x5A}
    # the failed calls left the tables in place; tables of other sizes replace them
    for other in (name, "g2x3x4_n1", "pos_global", "g16x16x64_n2"):
        t, g = tables_of(other), CASES[other][:3]
        codec.entropy_set_tables_nbr(t, g)
        codec.entropy_encode_nbr_device(d_sym, offs, counts, L, d_scr, d_out, d_sizes)
        sizes = d_sizes.download((2,), np.uint64)
        want = [entropy.pack(s, t, segment=L, geometry=g) for s in streams]
        assert sizes.tolist() == [len(w) for w in want], other
        assert d_out.download((int(sizes.sum()),), np.uint8).tobytes() == b"".join(want), other
    for b in (d_sym, d_scr, d_out, d_sizes, d_cnt):
        b.free()


@pytest.mark.parametrize("name,L", [("g2x3x4_n2", 8), ("g2x2x3_n2", 4), ("g8x8x80_n2", 2048), ("g16x16x64_n1", 4096),
                                    ("far_row", 4096)])
def test_histogram_nbr(codec, name, L):
    eh, ew, C_, K0, nbrs, _, _, _ = CASES[name]
    M, Q = 3 ** nbrs, 2
    codec.entropy_set_tables_nbr(tables_of(name), (eh, ew, C_))
    counts = [1, L + 1, 2 * eh * ew * C_ + 5, 3 * L]
    streams = [draw(n, Q, seed=70 + n) for n in counts]
    streams[2][5], streams[2][6] = Q, Q + 1  # np.histogram's closed last bin; a value in no bin
    want = np.zeros((K0 * M, Q), np.uint64)
    for s in streams:
        ref = np.minimum(s, Q - 1)  # a neighbour's class is that of its bin
        rows = nb_rows_np(ref, eh, ew, C_, L, K0, nbrs, Q)
        keep = s <= Q
        np.add.at(want, (rows[keep], ref[keep]), 1)
    offs, size = _place(counts, "odd")
    arena, _ = _arena(streams, offs, size, 0xA5)
    d_sym, d_cnt = codec.alloc(size), codec.alloc(8 * K0 * M * Q + 8)
    d_sym.upload(arena)
    codec.memset_device(d_cnt, 0, 8 * K0 * M * Q)
    codec.memset_device(d_cnt.view(8 * K0 * M * Q), 0x5A, 8)
    codec.histogram_nbr_device(d_sym, offs, counts, Q, L, d_cnt)
    assert np.array_equal(d_cnt.download((K0 * M, Q), np.uint64), want)
    codec.histogram_nbr_device(d_sym, offs, counts, Q, L, d_cnt)  # accumulates
    assert np.array_equal(d_cnt.download((K0 * M, Q), np.uint64), 2 * want)
    assert set(d_cnt.download((8 * K0 * M * Q + 8,), np.uint8)[-8:].tolist()) == {0x5A}
    d_sym.free()
    d_cnt.free()


def _nbr_tables_from(symbols, code_shape, neighbours, L):
    from tf_image_compression_amd.range_coder import nbr_probabilities, symbol_tables_nbr
    eh, ew, C_ = code_shape
    M = 3 ** neighbours
    counts = np.zeros(C_ * M * 2, np.int64)
    for s in symbols:
        flat = s.reshape(-1)
        rows = nb_rows_np(flat, eh, ew, C_, L, C_, neighbours, 2)
        counts += np.bincount(rows * 2 + flat, minlength=counts.size)
    return symbol_tables_nbr(nbr_probabilities(counts.reshape(C_, M, 2)), resolution=4096)


@pytest.mark.parametrize("neighbours", [1, 2])
def test_image_codec_neighbour_streams(codec, neighbours):
    from test_gpu_entropy_ctx import _images, _tables_from
    from tf_image_compression_amd import entropy
    from tf_image_compression_amd.evaluate import estimated_bits_ctx
    from tf_image_compression_amd.image_codec import ImageCodec
    ic = ImageCodec(codec)
    images = _images()
    sizes = [im.shape[:2] for im in images]
    symbols = ic.encode_images(images)
    geo = tuple(int(v) for v in codec.code_shape)
    C_, L = geo[2], 2048
    _, tables_v2, _, _ = _tables_from(symbols, C_)
    tables = _nbr_tables_from(symbols, geo, neighbours, L)
    v2 = ic.encode_images_to_streams(images, tables_v2, segment=L)
    v3 = ic.encode_images_to_streams(images, tables, segment=L)
    for s, sym in zip(v3, symbols):
        assert entropy.parse_nbr(s) == (L, sym.size, C_, entropy.tables_crc(tables), geo, neighbours)
        assert s == entropy.pack(sym, tables, segment=L, geometry=geo)
    print(f"per-channel tables {sum(map(len, v2))} B, channel x {3 ** neighbours} neighbour classes {sum(map(len, v3))} B")
    want = ic.decode_streams_to_images(v2, sizes, tables_v2, post_filter=False)
    got = ic.decode_streams_to_images(v3, sizes, tables, post_filter=False)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))
    res = ic.evaluate_images(images, post_filter=False, cum_freq=tables, entropy_segment=L)
    assert [r["coded_bytes"] for r in res] == [len(s) for s in v3]
    flat_tables = tables.reshape(-1, 3)
    for r, sym in zip(res, symbols):
        flat = sym.reshape(-1)
        rows = nb_rows_np(flat, *geo, L, C_, neighbours, 2)
        per = np.bincount(rows * 2 + flat, minlength=flat_tables.shape[0] * 2).reshape(-1, 2)
        est = estimated_bits_ctx(per, flat_tables)
        assert abs(r["est_bits"] - est) <= 1e-9 * est
        assert np.array_equal(r["counts"], per.sum(axis=0))
    other = tables.copy()
    other[3, 1, 1] += 1
    with pytest.raises(ValueError, match="other neighbour tables"):
        ic.decode_streams_to_images(v3, sizes, other, post_filter=False)
    with pytest.raises(ValueError, match="version 2"):
        ic.decode_streams_to_images(v2, sizes, tables, post_filter=False)
    with pytest.raises(ValueError, match="version 3"):
        ic.decode_streams_to_images(v3, sizes, tables_v2, post_filter=False)
    ic.close()


def test_get_encoded_distribution_neighbours(codec, tmp_path):
    """get_encoded_distribution.py --neighbours on 66 PNG patches (two batches, each one stream): the
    counts equal numpy's on the encoder's symbols."""
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
    eh, ew, C_ = (int(v) for v in codec.code_shape)
    for nbrs in (1, 2):
        freq, nbr_freq = ged.encoded_neighbour_frequencies(codec, ged.patch_batches(paths, 64), 2, C_, nbrs, 2048)
        want = np.zeros(C_ * 3 ** nbrs * 2, np.int64)
        for batch in (sym[:64].reshape(-1), sym[64:].reshape(-1)):
            rows = nb_rows_np(batch, eh, ew, C_, 2048, C_, nbrs, 2)
            want += np.bincount(rows * 2 + batch, minlength=want.size)
        assert np.array_equal(nbr_freq, want.reshape(C_, 3 ** nbrs, 2).astype(np.float64)), nbrs
        assert np.array_equal(freq, np.bincount(sym.reshape(-1), minlength=2).astype(np.float64))


def test_cli_neighbour_distribution(tmp_path):
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
    p1 = rng.random((64, 9)) ** 3 * 0.98 + 0.01
    np.save(tmp_path / "flat_0.npy", np.array([0.6, 0.4]))
    np.save(tmp_path / "nbr_0.npy", np.stack([1 - p1, p1], axis=2))
    cfg = encode.load_config("0")
    dirs = {}
    for mode in ("flat", "nbr"):
        common = ["-m", "0", "-g", "0", "--synthetic-weights", "--dist", str(tmp_path / (mode + "_{}.npy")),
                  "--norm", "/nonexistent", "--entropy", "device", "--batch-images", "4"]
        enc_dir, rec_dir = str(tmp_path / f"enc_{mode}"), str(tmp_path / f"rec_{mode}")
        eargs = encode.my_parse_args(common + ["--segment", "64", "-v", str(lst), "-o", enc_dir])
        encode.compress(encode.load_model(eargs, cfg), eargs)
        dargs = decode.my_parse_args(common + ["-i", enc_dir, "-o", rec_dir])
        decode.uncompress(decode.load_model(dargs, cfg), dargs)
        dirs[mode] = (enc_dir, rec_dir, common)
    files = sorted(os.listdir(dirs["flat"][0]))
    assert len(files) == 3 and files == sorted(os.listdir(dirs["nbr"][0]))
    for f in files:
        data = open(os.path.join(dirs["nbr"][0], f), "rb").read()
        L, n, K0, _, geo, nbrs = entropy.parse_nbr(data)
        assert (L, n, K0, nbrs) == (64, decode.get_img_info(f, cfg)[0], 64, 2) and geo[2] == 64
    pngs = sorted(os.listdir(dirs["flat"][1]))
    assert len(pngs) == 3 and pngs == sorted(os.listdir(dirs["nbr"][1]))
    for f in pngs:
        assert open(os.path.join(dirs["flat"][1], f), "rb").read() == open(os.path.join(dirs["nbr"][1], f), "rb").read()
    # a file's version byte against the table given, and its geometry against the model's
    dargs = decode.my_parse_args(dirs["flat"][2] + ["-i", dirs["nbr"][0], "-o", str(tmp_path / "x")])
    with pytest.raises(ValueError, match="version-3"):
        decode.uncompress(decode.load_model(dargs, cfg), dargs)
    dargs = decode.my_parse_args(dirs["nbr"][2] + ["-i", dirs["flat"][0], "-o", str(tmp_path / "y")])
    with pytest.raises(ValueError, match="version-1"):
        decode.uncompress(decode.load_model(dargs, cfg), dargs)
    other = tmp_path / "enc_other"
    other.mkdir()
    for f in files:
        data = bytearray(open(os.path.join(dirs["nbr"][0], f), "rb").read())
        data[28:30] = struct.pack("<H", struct.unpack_from("<H", data, 28)[0] + 1)
        (other / f).write_bytes(bytes(data))
    dargs = decode.my_parse_args(dirs["nbr"][2] + ["-i", str(other), "-o", str(tmp_path / "z")])
    with pytest.raises(ValueError, match="code geometry"):
        decode.uncompress(decode.load_model(dargs, cfg), dargs)

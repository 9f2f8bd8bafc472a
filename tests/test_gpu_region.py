"""GPU tests of region decode: the device range decoder (tic_entropy_decode_ranges*_device) against
entropy.unpack_range, the clause that lets a container be uploaded sparsely, the region
post-filter (tic_rmbe_regions_device) against tic_rmbe_image_device, ImageCodec.decode_regions
against the crop of decode_streams_to_images, and decode.py --region."""
import functools
import struct

import numpy as np
import pytest

from entropy_ctx_cases import MIXED_TOTALS, make_tables
from entropy_nbr_cases import draw, make_nbr_tables
from test_gpu_entropy import _arena, _place

pytestmark = pytest.mark.gpu

HEADER = {1: 20, 2: 28, 3: 36}

# name -> (version, (eh, ew, C), K or K0, neighbours, mixed totals, [L]).  The two geometries at
# L = 16 have many segments per patch; at L = 2048 a segment of g4x4x64 (patches of 1024) spans two
# patches, so a patch's range drops leading and trailing symbols.  v2_global: 16384 * 3 * 4 bytes of
# tables, the global-memory kernel.  v3_long_row: ew * C = 16000 bits of ring a lane, over the LDS
# budget of 64 lanes, so the range kernel runs 32 lanes a workgroup.
CASES = {
    "v1_g4x4x64": (1, (4, 4, 64), 1, 0, False, (16, 2048)),
    "v1_g16x16x64": (1, (16, 16, 64), 1, 0, False, (16, 2048)),
    "v2_g4x4x64": (2, (4, 4, 64), 64, 0, True, (16, 2048)),
    "v2_g16x16x64": (2, (16, 16, 64), 64, 0, False, (16, 2048)),
    "v2_global": (2, (16, 16, 64), 16384, 0, False, (16, 2048)),
    "v3_g4x4x64_n2": (3, (4, 4, 64), 64, 2, False, (16, 2048)),
    "v3_g16x16x64_n2": (3, (16, 16, 64), 64, 2, True, (16, 2048)),
    "v3_long_row": (3, (2, 250, 64), 64, 2, False, (16384,)),
}


def cases_with_L():
    return [(name, L) for name in CASES for L in CASES[name][5]]


@functools.lru_cache(maxsize=None)
def tables_of(name):
    version, _, K, nbrs, mixed, _ = CASES[name]
    totals = MIXED_TOTALS if mixed else (4096,)
    seed = sum(name.encode())
    if version == 1:
        t = make_tables(1, 3, seed, totals)[0]
    elif version == 2:
        t = make_tables(K, 3, seed, totals)
    else:
        t = make_nbr_tables(K, nbrs, 3, seed, totals)
    t.setflags(write=False)
    return t


def set_tables(codec, name):
    version, geo = CASES[name][:2]
    if version == 1:
        codec.entropy_set_table(tables_of(name))
    elif version == 2:
        codec.entropy_set_tables(tables_of(name))
    else:
        codec.entropy_set_tables_nbr(tables_of(name), geo)


def ranges_for(n, L, patch):
    """One symbol at each end, inside a segment, up to a segment border, across three segments, a
    whole patch (the ranges region decode asks for), everything."""
    out = [(0, 1), (n - 1, 1), (1, min(n, L) - 2), (0, n)]
    if n >= 2 * L:
        out.append((L // 2, 2 * L - L // 2))
    if n >= 2 * L + 1:
        out.append((L - 1, L + 2))
    if n >= 2 * patch:
        out.append((patch, patch))
    return [(f, c) for f, c in out if c > 0]


@functools.lru_cache(maxsize=None)
def host_side(name, L):
    """(streams, containers, ranges as (container, first, count), their symbols by
    entropy.unpack_range): two containers, several ranges each, interleaved.  Computed once."""
    from tf_image_compression_amd import entropy
    version, geo = CASES[name][:2]
    g = geo if version == 3 else None
    patch = geo[0] * geo[1] * geo[2]
    tables = tables_of(name)
    counts = [2 * max(L, patch) + 7, 3 * L + 2 + patch]
    streams = [draw(n, 2, seed=1000 + n) for n in counts]
    blobs = [entropy.pack(s, tables, segment=L, geometry=g) for s in streams]
    per = [ranges_for(n, L, patch) for n in counts]
    recs = [(ci, f, c) for k in range(max(map(len, per))) for ci in (0, 1) if k < len(per[ci]) for f, c in [per[ci][k]]]
    want = [entropy.unpack_range(blobs[ci], tables, f, c, geometry=g) for ci, f, c in recs]
    for (ci, f, c), w in zip(recs, want):
        assert np.array_equal(w, streams[ci][f:f + c])
    return streams, blobs, recs, want


def device_decode_ranges(codec, version, blobs, stream_counts, recs, L, layout="packed", blob_sizes=None):
    """The ranges' symbols; d_sym and the scratch are poisoned first and every byte of d_sym outside
    the ranges must still be poison afterwards.  blobs: what lies on the device (bytes or uint8
    arrays, possibly sparse copies)."""
    boffs, bsize = _place([len(b) for b in blobs], "odd")
    barena, _ = _arena(blobs, boffs, bsize, 0xA5)
    counts = [c for _, _, c in recs]
    soffs, ssize = _place(counts, layout)
    d_blob, d_sym = codec.alloc(bsize), codec.alloc(ssize)
    d_blob.upload(barena)
    codec.memset_device(d_sym, 0xA5, ssize)
    need = codec.entropy_ranges_scratch_bytes([f for _, f, _ in recs], counts, L)
    d_scr = codec.alloc(need)
    codec.memset_device(d_scr, 0xC3, need)
    sizes = [len(b) for b in blobs] if blob_sizes is None else blob_sizes
    codec.entropy_decode_ranges_device(d_blob, [boffs[ci] for ci, _, _ in recs], [sizes[ci] for ci, _, _ in recs],
                                       [stream_counts[ci] for ci, _, _ in recs], [f for _, f, _ in recs], counts,
                                       d_sym, soffs, d_scr, version=version)
    got = d_sym.download((ssize,), np.uint8)
    for b in (d_blob, d_sym, d_scr):
        b.free()
    used = np.zeros(ssize, bool)
    for o, n in zip(soffs, counts):
        used[o:o + n] = True
    assert np.all(got[~used] == 0xA5), "bytes outside the ranges were written"
    return [got[o:o + n] for o, n in zip(soffs, counts)]


@pytest.fixture(scope="module")
def codec():
    from tf_image_compression_amd.codec import Codec
    from tf_image_compression_amd.weights import synthetic_params, SYNTH_MEAN, SYNTH_STD
    with Codec(0, synthetic_params(0), SYNTH_MEAN, SYNTH_STD, patch_size=64, quan_scale=2, device=0) as c:
        yield c


@pytest.mark.parametrize("name,L", cases_with_L())
def test_ranges_match_host(codec, name, L):
    version = CASES[name][0]
    set_tables(codec, name)
    streams, blobs, recs, want = host_side(name, L)
    counts = [len(s) for s in streams]
    first = None
    for layout in ("packed", "odd", "reversed", "packed"):
        got = device_decode_ranges(codec, version, blobs, counts, recs, L, layout)
        for g, w, rec in zip(got, want, recs):
            assert np.array_equal(g, w), (layout, rec)
        if layout == "packed":  # two identical calls: identical bytes
            assert first is None or all(np.array_equal(a, b) for a, b in zip(first, got))
            first = got


@pytest.mark.parametrize("name,L", [(n, L) for n, L in cases_with_L() if n != "v2_global"])
def test_only_the_extents_are_read(codec, name, L):
    """The device copy of each container holds 0xA5 everywhere but the header, the length table and
    the ranges' extents."""
    from tf_image_compression_amd import entropy
    version, geo = CASES[name][:2]
    g = geo if version == 3 else None
    set_tables(codec, name)
    tables = tables_of(name)
    n = 16 * max(L, 1024) + 7
    streams = [draw(n, 2, seed=7 + L), draw(n, 2, seed=8 + L)]
    blobs = [entropy.pack(s, tables, segment=L, geometry=g) for s in streams]
    recs = [(0, 0, 1), (1, n - 1, 1), (0, 3 * L - 1, L + 2), (1, 5 * L, L), (0, n // 2 + 3, n // 16)]
    sparse, poisoned, payload = [], 0, 0
    for ci, blob in enumerate(blobs):
        a = np.frombuffer(blob, np.uint8)
        keep = np.zeros(a.size, bool)
        head = HEADER[version] + 2 * -(-n // L)
        keep[:head] = True
        covered = 0
        for cj, f, c in recs:
            if cj == ci:
                _, _, off, length = entropy.range_extent(blob[:head], f, c)
                keep[off:off + length] = True
                covered += c
        assert covered <= n // 4
        sparse.append(np.where(keep, a, 0xA5).astype(np.uint8))
        poisoned += int((~keep).sum())
        payload += a.size - head
    assert 2 * poisoned >= payload, (poisoned, payload)
    got = device_decode_ranges(codec, version, sparse, [n, n], recs, L, "odd")
    for gsym, (ci, f, c) in zip(got, recs):
        assert np.array_equal(gsym, streams[ci][f:f + c]), (ci, f, c)


@pytest.mark.parametrize("name", ["v1_g4x4x64", "v2_g4x4x64", "v3_g4x4x64_n2"])
def test_rejected_containers_give_zeros_in_their_ranges_only(codec, name):
    version, geo, K = CASES[name][:3]
    set_tables(codec, name)
    L = 16
    streams, blobs, _, _ = host_side(name, L)
    n, blob = len(streams[0]), blobs[0]
    hdr, S = HEADER[version], -(-len(streams[0]) // L)

    def patched(at, data):
        return blob[:at] + data + blob[at + len(data):]

    bad = [patched(4, bytes([1 + version % 3])),          # the wrong version for the entry
           patched(12, struct.pack("<Q", n + 1)),          # the header's n is not stream_counts
           patched(8, struct.pack("<I", 6))]               # a bad L
    if version >= 2:
        bad += [patched(20, struct.pack("<I", K + 1)), patched(24, bytes([blob[24] ^ 0x40]))]  # K / K0, CRC
    if version == 3:
        bad += [patched(28, struct.pack("<H", geo[0] + 1)), patched(32, struct.pack("<H", geo[2] + 1)),
                patched(34, b"\x01")]                      # geometry, neighbours
    recs = []
    for ci in range(len(bad)):
        recs += [(ci, 5, 40), (ci, n - 9, 9)]
    good = len(bad)
    recs += [(good, 3, 50)]
    got = device_decode_ranges(codec, version, bad + [blobs[0]], [n] * (len(bad) + 1), recs, L, "odd")
    for g_, (ci, f, c) in zip(got, recs):
        if ci == good:
            assert np.array_equal(g_, streams[0][f:f + c])
        else:
            assert g_.size == c and not g_.any(), (ci, f, c)
    # wrong stream_counts; an extent cut off by blob_sizes (the last segment's payload ends outside)
    got = device_decode_ranges(codec, version, [blob, blob], [n - 1, n], [(0, 5, 40), (1, 3, 50)], L, "odd")
    assert not got[0].any() and np.array_equal(got[1], streams[0][3:53])
    recs = [(0, n - 9, 9), (1, 3, 50), (0, 0, 4)]  # the first range needs the last byte, the third does not
    got = device_decode_ranges(codec, version, [blob, blob], [n, n], recs, L, "odd",
                               blob_sizes=[len(blob) - 1, len(blob)])
    assert not got[0].any()
    assert np.array_equal(got[1], streams[0][3:53]) and np.array_equal(got[2], streams[0][0:4])
    # the length table itself cut off
    got = device_decode_ranges(codec, version, [blob, blob], [n, n], [(0, 0, 4), (1, 3, 50)], L, "odd",
                               blob_sizes=[hdr + 2 * S - 1, len(blob)])
    assert not got[0].any() and np.array_equal(got[1], streams[0][3:53])


def test_range_argument_errors_leave_d_sym_untouched(codec):
    import ctypes as C
    from tf_image_compression_amd._lib import lib
    from tf_image_compression_amd.codec import Codec
    from tf_image_compression_amd.weights import synthetic_params, SYNTH_MEAN, SYNTH_STD
    name, L = "v1_g4x4x64", 16
    set_tables(codec, name)
    streams, blobs, _, _ = host_side(name, L)
    n, blob = len(streams[0]), blobs[0]
    d_blob, d_sym = codec.alloc(len(blob)), codec.alloc(256)
    d_blob.upload(np.frombuffer(blob, np.uint8))
    codec.memset_device(d_sym, 0xA5, 256)
    need = codec.entropy_ranges_scratch_bytes([5], [40], L)
    assert need == codec.entropy_ranges_scratch_bytes([0], [40], L)  # wherever the range starts
    d_scr = codec.alloc(need)

    def call(first=5, count=40, scnt=n, boff=0, bsize=len(blob), soff=0, scratch=None, version=1, c=codec):
        c.entropy_decode_ranges_device(d_blob, [boff], [bsize], [scnt], [first], [count], d_sym, [soff], d_scr,
                                       scratch_bytes=scratch, version=version)

    for kw in (dict(count=0), dict(count=-1), dict(first=-1), dict(first=n), dict(first=n - 1, count=2),
               dict(scnt=0), dict(boff=-1), dict(bsize=-1), dict(soff=-1)):
        with pytest.raises(ValueError):
            call(**kw)
    with pytest.raises(ValueError, match="scratch"):  # not even one segment per range
        call(scratch=16)
    with pytest.raises(ValueError, match="version"):
        call(version=4)
    with Codec(0, synthetic_params(0), SYNTH_MEAN, SYNTH_STD, patch_size=64, device=0) as fresh:
        for version, what in ((1, "no entropy table"), (2, "no context tables"), (3, "no neighbour tables")):
            with pytest.raises(ValueError, match=what):
                call(version=version, c=fresh)
    for bad_L in (0, 6, 16388):
        with pytest.raises(ValueError, match="segment length"):
            codec.entropy_ranges_scratch_bytes([0], [4], bad_L)
    with pytest.raises(ValueError):
        codec.entropy_ranges_scratch_bytes([0], [0], L)
    i64 = C.POINTER(C.c_int64)
    one = lambda v: np.asarray([v], np.int64).ctypes.data_as(i64)
    args = [one(0), one(len(blob)), one(n), one(5), one(40)]
    fn = lib().tic_entropy_decode_ranges_device
    assert fn(None, d_blob.ptr, *args, 1, d_sym.ptr, one(0), d_scr.ptr, need) == -1
    assert fn(codec._h, None, *args, 1, d_sym.ptr, one(0), d_scr.ptr, need) == -1
    assert fn(codec._h, d_blob.ptr, *args, 1, None, one(0), d_scr.ptr, need) == -1
    assert fn(codec._h, d_blob.ptr, *args, 1, d_sym.ptr, one(0), None, need) == -1
    assert fn(codec._h, d_blob.ptr, *args[:3], None, args[4], 1, d_sym.ptr, one(0), d_scr.ptr, need) == -1
    assert fn(codec._h, d_blob.ptr, *args, -1, d_sym.ptr, one(0), d_scr.ptr, need) == -1
    assert fn(codec._h, d_blob.ptr, *args, 0, d_sym.ptr, one(0), d_scr.ptr, need) == 0  # nothing to do
    codec.synchronize()
    assert np.all(d_sym.download((256,), np.uint8) == 0xA5)
    call()  # and the call they were variations of works
    codec.synchronize()
    assert np.array_equal(d_sym.download((256,), np.uint8)[:40], streams[0][5:45])
    for b in (d_blob, d_sym, d_scr):
        b.free()


# ---------------------------------------------------------------------------------------------
# the region post-filter, ImageCodec.decode_regions and decode.py --region

@pytest.fixture(scope="module")
def codecs():
    from tf_image_compression_amd.codec import Codec
    from tf_image_compression_amd.weights import synthetic_params, SYNTH_MEAN, SYNTH_STD
    from tf_image_compression_amd.topology import RMBE_ID
    c0 = Codec(0, synthetic_params(0, seed=0), SYNTH_MEAN, SYNTH_STD, patch_size=64, quan_scale=2)
    cr = Codec(RMBE_ID, synthetic_params(RMBE_ID, seed=0), SYNTH_MEAN, SYNTH_STD, patch_size=128)
    yield c0, cr
    c0.close()
    cr.close()


def _image(H, W, seed):
    r = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    base = 128 + 60 * np.sin(xx / 17.0)[..., None] * np.cos(yy / 23.0)[..., None] + r.normal(0, 12, (H, W, 3))
    return np.clip(base, 0, 255).astype(np.uint8)


def test_rmbe_regions_against_the_whole_image(codecs):
    """Region 0 is the whole 330 x 460 image and must be tic_rmbe_image_device's result bit for
    bit; two more regions, the boxes region_plan gives for two crops, are filtered in the same
    call and compared with it on the crops they were planned for."""
    from tf_image_compression_amd.codec import Codec
    _, cr = codecs
    H, W = 330, 460
    img = np.random.default_rng(3).uniform(0, 255, (H, W, 3)).astype(np.float32)
    d_full = cr.alloc(img.nbytes)
    d_full.upload(img)
    cr.rmbe_image_device(d_full, H, W)
    cr.synchronize()
    want = d_full.download((H, W, 3), np.float32)
    d_full.free()
    assert not np.array_equal(want, img)

    crops = [(200, 210, 20, 30),   # the box starts at column 64: a multiple of 64, not of 128
             (300, 440, 30, 20)]   # reaches the bottom-right corner; the box starts at column 320 = 5 * 64
    blocks, sizes, origins = [img], [(H, W)], [(0, 0)]
    for y, x, h, w in crops:
        py0, py1, px0, px1 = Codec.region_plan(H, W, 64, y, x, h, w, 128)
        y0, y1, x0, x1 = py0 * 64, min(py1 * 64, H), px0 * 64, min(px1 * 64, W)
        blocks.append(np.ascontiguousarray(img[y0:y1, x0:x1]))
        sizes.append((y1 - y0, x1 - x0))
        origins.append((y0, x0))
    assert origins[1] == (128, 64) and origins[2] == (128, 320) and sizes[2] == (H - 128, W - 320)
    gap = 5  # floats between the blocks: any alignment
    offs, at = [], 3
    for b in blocks:
        offs.append(at)
        at += b.size + gap
    arena = np.full(at, np.float32(-7.0))
    for b, o in zip(blocks, offs):
        arena[o:o + b.size] = b.reshape(-1)
    d = cr.alloc(arena.nbytes)
    d.upload(arena)
    cr.rmbe_regions_device(d, offs, sizes, origins, [(H, W)] * 3)
    cr.synchronize()
    got = d.download((at,), np.float32)
    used = np.zeros(at, bool)
    for b, o in zip(blocks, offs):
        used[o:o + b.size] = True
    assert np.all(got[~used] == np.float32(-7.0)), "floats outside the regions were written"
    full = got[offs[0]:offs[0] + img.size].reshape(H, W, 3)
    assert np.array_equal(full, want)
    for (y, x, h, w), (bh, bw), (y0, x0), o in zip(crops, sizes[1:], origins[1:], offs[1:]):
        box = got[o:o + bh * bw * 3].reshape(bh, bw, 3)
        assert np.array_equal(box[y - y0:y - y0 + h, x - x0:x - x0 + w], want[y:y + h, x:x + w]), (y, x, h, w)
    # argument errors: a region outside its image, overlapping regions, a codec handle
    with pytest.raises(ValueError, match="not inside"):
        cr.rmbe_regions_device(d, offs[:1], [(H, W)], [(1, 0)], [(H, W)])
    with pytest.raises(ValueError, match="overlap"):
        cr.rmbe_regions_device(d, [offs[0], offs[0] + 9], sizes[:2], origins[:2], [(H, W)] * 2)
    with pytest.raises(ValueError, match="rmbe"):
        codecs[0].rmbe_regions_device(d, offs, sizes, origins, [(H, W)] * 3)
    d.free()


REGION_SIZES = [(330, 460), (200, 150)]
# (y, x, h, w) per image, paired by position: two images with different regions in one call
REGIONS = [
    [(150, 200, 1, 1), (199, 149, 1, 1)],          # 1 x 1: in the interior; the last pixel
    [(70, 70, 20, 20), (130, 10, 40, 50)],         # inside one patch
    [(185, 120, 15, 20), (60, 120, 10, 16)],       # across a second-pass window border (row 192, column 128)
    [(300, 430, 30, 30), (150, 100, 50, 50)],      # the last row and column, inside the reflect-padded edge patches
    [(322, 450, 8, 10), (195, 140, 5, 10)],        # an edge strip no window covers
    [(0, 0, 330, 460), (0, 0, 200, 150)],          # the whole image
]


@functools.lru_cache(maxsize=None)
def region_tables(version):
    if version == 1:
        return (0, 2457, 4096)
    t = make_nbr_tables(64, 2, 3, seed=11, totals=MIXED_TOTALS)
    t.setflags(write=False)
    return t


@pytest.fixture(scope="module")
def full_decodes(codecs):
    """(version, L, post) -> (streams, images by decode_streams_to_images), computed once."""
    from tf_image_compression_amd.image_codec import ImageCodec
    c0, cr = codecs
    ic = ImageCodec(c0, cr)
    images = [_image(H, W, 11 * H + W) for H, W in REGION_SIZES]
    cache = {}

    def get(version, L, post):
        key = (version, L, post)
        if key not in cache:
            tables = region_tables(version)
            skey = (version, L)
            if skey not in cache:
                cache[skey] = ic.encode_images_to_streams(images, tables, segment=L)
            cache[key] = (cache[skey], ic.decode_streams_to_images(cache[skey], REGION_SIZES, tables, post_filter=post))
        return cache[key]

    yield ic, get
    ic.close()


@pytest.mark.parametrize("post", [False, True], ids=["plain", "rmbe"])
@pytest.mark.parametrize("L", [2048, 16])
@pytest.mark.parametrize("version", [1, 3])
def test_decode_regions_is_the_crop_of_the_full_decode(full_decodes, version, L, post):
    from tf_image_compression_amd import entropy
    ic, get = full_decodes
    streams, full = get(version, L, post)
    assert entropy.container_version(streams[0]) == version
    tables = region_tables(version)
    for pair in REGIONS:
        # the upload is sparse and leaves the rest of the device buffer as it was: poison it, so
        # that a piece the decoder needs and the upload left out is not still there from the full decode
        d_blob = ic._buf("entropy_blob", sum(len(s) for s in streams))
        ic.codec.memset_device(d_blob, 0xA5, d_blob.nbytes)
        got = ic.decode_regions(streams, REGION_SIZES, pair, tables, post_filter=post)
        for g, im, (y, x, h, w) in zip(got, full, pair):
            assert g.dtype == np.uint8 and g.shape == (h, w, 3)
            assert np.array_equal(g, im[y:y + h, x:x + w]), (version, L, post, (y, x, h, w))
        stats = ic.last_region_stats
        for st, size, region in zip(stats, REGION_SIZES, pair):
            py0, py1, px0, px1 = ic.region_plan(size, region, post)
            assert st["patches"] == (py1 - py0) * (px1 - px0) <= st["patches_image"]
            assert st["bytes_uploaded"] <= st["bytes_container"]
    # an interior region without the post-filter: the plan's patches, not the image's
    ic.decode_regions(streams[:1], REGION_SIZES[:1], [(70, 70, 20, 20)], tables, post_filter=False)
    assert ic.last_region_stats[0]["patches"] == 1 and ic.last_region_stats[0]["patches_image"] == 6 * 8
    # one image alone, the other order, and the same region twice give the same bytes
    y, x, h, w = REGIONS[2][1]
    one = ic.decode_regions(streams[1:], REGION_SIZES[1:], [REGIONS[2][1]], tables, post_filter=post)[0]
    assert np.array_equal(one, full[1][y:y + h, x:x + w])
    two = ic.decode_regions(streams[::-1], REGION_SIZES[::-1], [REGIONS[2][1], REGIONS[2][0]], tables, post_filter=post)
    assert np.array_equal(two[0], one)


def test_decode_regions_validation(full_decodes):
    ic, get = full_decodes
    streams, _ = get(1, 2048, False)
    tables = region_tables(1)
    for bad in [(0, 0, 0, 5), (0, 0, 331, 5), (329, 0, 2, 5), (0, 459, 1, 2), (-1, 0, 2, 2)]:
        with pytest.raises(ValueError):
            ic.decode_regions(streams[:1], REGION_SIZES[:1], [bad], tables)
    with pytest.raises(ValueError, match="regions for"):
        ic.decode_regions(streams, REGION_SIZES, [(0, 0, 1, 1)], tables)
    with pytest.raises(ValueError, match="symbols"):  # the container of the other image
        ic.decode_regions(streams[::-1], REGION_SIZES, [(0, 0, 1, 1)] * 2, tables)
    with pytest.raises(ValueError):  # version-1 containers under 3-D tables
        ic.decode_regions(streams, REGION_SIZES, [(0, 0, 1, 1)] * 2, region_tables(3))
    assert ic.decode_regions([], [], [], tables) == []


@pytest.mark.parametrize("model_num,rmbe", [("0", False), ("3", True)])
def test_cli_region(tmp_path, model_num, rmbe):
    import os
    import decode
    import encode
    from tf_image_compression_amd import utils
    from tf_image_compression_amd.topology import RMBE_ID
    from tf_image_compression_amd.weights import save_params, synthetic_params
    sizes = [(300, 200), (130, 257), (256, 300)]
    paths = []
    for k, (h, w) in enumerate(sizes):
        p = str(tmp_path / f"img{k}.png")
        utils.imsave(p, _image(h, w, 60 + k))
        paths.append(p)
    lst = tmp_path / "list.txt"
    lst.write_text("\n".join(paths) + "\n")
    np.save(tmp_path / f"dist_{model_num}.npy", np.array([0.6, 0.4]))
    common = ["-m", model_num, "-g", "0", "--synthetic-weights", "--dist", str(tmp_path / "dist_{}.npy"),
              "--norm", "/nonexistent"]
    dev = ["--entropy", "device"]
    post = []
    if rmbe:
        wfile = str(tmp_path / "rmbe.npz")
        save_params(wfile, synthetic_params(RMBE_ID))
        post = ["--rmbe", wfile, "--rmbe-norm", "/nonexistent"]
    cfg = encode.load_config(model_num)
    enc_dir = str(tmp_path / "enc")
    eargs = encode.my_parse_args(common + dev + ["--segment", "64", "-v", str(lst), "-o", enc_dir])
    encode.compress(encode.load_model(eargs, cfg), eargs)
    dargs = decode.my_parse_args(common + dev + post + ["-i", enc_dir, "-o", str(tmp_path / "full")])
    model = decode.load_model(dargs, cfg)
    decode.uncompress(model, dargs)
    X, Y, Wd, Ht = 40, 30, 150, 90
    for nb in ("1", "3"):
        out = str(tmp_path / f"reg{nb}")
        dargs = decode.my_parse_args(common + dev + post + ["-i", enc_dir, "-o", out, "--batch-images", nb,
                                                            "--region", f"{X},{Y},{Wd},{Ht}"])
        decode.uncompress(model, dargs)
        assert sorted(os.listdir(out)) == [f"img{k}_x{X}_y{Y}_{Wd}x{Ht}.png" for k in range(3)]
        for k in range(3):
            whole = utils.imread(str(tmp_path / "full" / f"img{k}.png"))
            part = utils.imread(os.path.join(out, f"img{k}_x{X}_y{Y}_{Wd}x{Ht}.png"))
            assert part.shape == (Ht, Wd, 3) and np.array_equal(part, whole[Y:Y + Ht, X:X + Wd]), (nb, k)
    # without the flag nothing changes
    assert sorted(os.listdir(tmp_path / "full")) == [f"img{k}.png" for k in range(3)]
    # the error cases
    for extra, what in ((["--raw"], "--raw"), (["--entropy", "host"], "--entropy device"), ([], "--entropy device")):
        with pytest.raises(SystemExit):
            decode.my_parse_args(common + extra + ["-i", enc_dir, "-o", out, "--region", "0,0,8,8"])
    for bad in ("1,2,3", "a,b,c,d", "0,0,0,8", "-1,0,8,8"):
        with pytest.raises(SystemExit):
            decode.my_parse_args(common + dev + ["-i", enc_dir, "-o", out, f"--region={bad}"])
    dargs = decode.my_parse_args(common + dev + ["-i", enc_dir, "-o", str(tmp_path / "none"), "--region", "20,50,160,90"])
    with pytest.raises(ValueError, match=r"img1.*does not contain the region 160 x 90 at \(20, 50\)"):
        decode.uncompress(model, dargs)
    assert not os.path.exists(tmp_path / "none") or not os.listdir(tmp_path / "none")  # nothing was written

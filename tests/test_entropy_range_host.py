"""CPU tests of the symbol-range entries of the segmented container (include/tic.h:
tic_rcseg_range_extent, tic_rcseg_decode_range / _ctx / _nbr; entropy.range_extent,
entropy.unpack_range).  The reference of a range is the slice of the full decode; the reference of
an extent is numpy arithmetic on the parsed length table."""
import struct

import numpy as np
import pytest

from entropy_ctx_cases import MIXED_TOTALS, make_tables
from entropy_nbr_cases import draw, make_nbr_tables
from tf_image_compression_amd import entropy

GEOS = [(2, 3, 4), (4, 4, 64)]
SEGMENTS = [4, 16, 2048]
HEADER = {1: 20, 2: 28, 3: 36}


def tables_for(version, geo, ncum=3, seed=5):
    """A table of the rank that selects ``version``: K = K0 = C."""
    if version == 1:
        return make_tables(1, ncum, seed, (4096,))[0]
    if version == 2:
        return make_tables(geo[2], ncum, seed, MIXED_TOTALS)
    return make_nbr_tables(geo[2], 2, ncum, seed, MIXED_TOTALS)


def lengths_for(geo, L):
    patch = geo[0] * geo[1] * geo[2]
    return [1, L - 1, L, L + 1, 3 * L + 2, 2 * patch + 7]


def ranges_for(n, L):
    """One symbol at 0 and at n - 1, a range inside one segment, one ending exactly on a segment
    border, one spanning three segments, the whole stream: those that fit n."""
    out = [(0, 1), (n - 1, 1), (0, n)]
    if n >= 3:
        out.append((1, min(n, L) - 2))  # inside segment 0
    if n >= 2 * L:
        out.append((L // 2, 2 * L - L // 2))  # ends where segment 2 starts
    if n >= 2 * L + 1:
        out.append((L - 1, L + 2))  # the last of segment 0, all of 1, the first of 2
    return [(f, c) for f, c in out if c > 0]


def extent_numpy(buf, version, first, count):
    """(j0, nj, byte_off, byte_len) from the header and the length table."""
    hdr = HEADER[version]
    L, n = struct.unpack_from("<IQ", buf, 8)
    S = -(-n // L)
    lens = np.frombuffer(buf, "<u2", S, hdr).astype(np.int64)
    starts = hdr + 2 * S + np.concatenate([[0], np.cumsum(lens)])
    j0, j1 = first // L, (first + count - 1) // L
    return j0, j1 - j0 + 1, int(starts[j0]), int(starts[j1 + 1] - starts[j0])


@pytest.mark.parametrize("L", SEGMENTS)
@pytest.mark.parametrize("geo", GEOS, ids=["g2x3x4", "g4x4x64"])
@pytest.mark.parametrize("version", [1, 2, 3])
def test_unpack_range_is_the_slice_of_unpack(version, geo, L):
    tables = tables_for(version, geo)
    for n in lengths_for(geo, L):
        sym = draw(n, 2, seed=n + L)
        buf = entropy.pack(sym, tables, segment=L, geometry=geo if version == 3 else None)
        full = entropy.unpack(buf, tables, geometry=geo if version == 3 else None)
        assert np.array_equal(full, sym)
        for first, count in ranges_for(n, L):
            got = entropy.unpack_range(buf, tables, first, count, geometry=geo if version == 3 else None)
            assert got.dtype == np.uint8 and got.shape == (count,)
            assert np.array_equal(got, full[first:first + count]), (version, geo, L, n, first, count)


@pytest.mark.parametrize("version", [1, 2, 3])
def test_unpack_range_with_256_symbols(version):
    geo, L = (2, 3, 4), 16
    tables = tables_for(version, geo, ncum=257)
    sym = draw(3 * L + 2, 256, seed=9)
    g = geo if version == 3 else None
    buf = entropy.pack(sym, tables, segment=L, geometry=g)
    for first, count in ranges_for(sym.size, L):
        assert np.array_equal(entropy.unpack_range(buf, tables, first, count, geometry=g), sym[first:first + count])


@pytest.mark.parametrize("L", SEGMENTS)
@pytest.mark.parametrize("version", [1, 2, 3])
def test_range_extent_is_the_length_tables(version, L):
    geo = (4, 4, 64)
    tables = tables_for(version, geo)
    g = geo if version == 3 else None
    for n in lengths_for(geo, L):
        buf = entropy.pack(draw(n, 2, seed=n), tables, segment=L, geometry=g)
        S = -(-n // L)
        head = buf[:HEADER[version] + 2 * S]
        for first, count in ranges_for(n, L):
            want = extent_numpy(buf, version, first, count)
            assert entropy.range_extent(buf, first, count) == want
            assert entropy.range_extent(head, first, count) == want  # payloads absent
            assert want[2] + want[3] <= len(buf)


@pytest.mark.parametrize("L", [16, 2048])
@pytest.mark.parametrize("version", [1, 2, 3])
def test_payload_outside_the_extent_is_never_read(version, L):
    """Every payload byte outside the extent is overwritten with 0xA5; the ranges cover at most a
    quarter of the stream, so more than half of the payload is poison."""
    geo = (4, 4, 64)
    tables = tables_for(version, geo)
    g = geo if version == 3 else None
    n = 16 * max(L, 1024) + 7
    sym = draw(n, 2, seed=L + version)
    buf = entropy.pack(sym, tables, segment=L, geometry=g)
    hdr = HEADER[version]
    S = -(-n // L)
    payload0 = hdr + 2 * S
    rng = np.random.default_rng(version * 100 + L)
    ranges = [(0, 1), (n - 1, 1), (3 * L - 1, L + 2), (5 * L, L)]
    ranges += [(int(rng.integers(0, n - n // 8)), int(rng.integers(1, n // 8))) for _ in range(4)]
    for first, count in ranges:
        assert count <= n // 4
        _, _, off, length = entropy.range_extent(buf, first, count)
        a = np.frombuffer(buf, np.uint8).copy()
        keep = np.zeros(a.size, bool)
        keep[:payload0] = True
        keep[off:off + length] = True
        a[~keep] = 0xA5
        poisoned = int((~keep).sum())
        assert 2 * poisoned > a.size - payload0, (first, count, poisoned, a.size - payload0)
        got = entropy.unpack_range(a.tobytes(), tables, first, count, geometry=g)
        assert np.array_equal(got, sym[first:first + count]), (version, L, first, count)


@pytest.mark.parametrize("version", [1, 2, 3])
def test_error_paths(version):
    geo, L, n = (2, 3, 4), 8, 50
    tables = tables_for(version, geo)
    g = geo if version == 3 else None
    sym = draw(n, 2, seed=3)
    buf = entropy.pack(sym, tables, segment=L, geometry=g)
    S = -(-n // L)
    assert np.array_equal(entropy.unpack_range(buf, tables, 7, 20, geometry=g), sym[7:27])
    # a range past n, an empty one
    for first, count in [(n, 1), (n - 1, 2), (0, n + 1), (0, 0), (5, 0), (-1, 2), (2, -1)]:
        with pytest.raises(ValueError):
            entropy.unpack_range(buf, tables, first, count, geometry=g)
        with pytest.raises(ValueError):
            entropy.range_extent(buf, first, count)
    # the length table not wholly present; a header cut short; no container at all
    for cut in (HEADER[version] + 2 * S - 1, HEADER[version] - 1, 3, 0):
        with pytest.raises(ValueError):
            entropy.range_extent(buf[:cut], 0, 1)
    with pytest.raises(ValueError, match="version"):
        entropy.range_extent(buf[:4] + b"\x04" + buf[5:], 0, 1)
    with pytest.raises(ValueError):
        entropy.unpack_range(buf[:-1], tables, 0, 1, geometry=g)  # the full validation of unpack
    # the wrong version for the entry
    for other in {1, 2, 3} - {version}:
        with pytest.raises(ValueError):
            entropy.unpack_range(buf, tables_for(other, geo), 0, 1, geometry=geo if other == 3 else None)


def test_wrong_tables_crc_k_and_geometry():
    geo, L = (2, 3, 4), 8
    sym = draw(60, 2, seed=4)
    t2, t3 = tables_for(2, geo), tables_for(3, geo)
    b2 = entropy.pack(sym, t2, segment=L)
    b3 = entropy.pack(sym, t3, segment=L, geometry=geo)
    crc2 = t2.copy()
    crc2[1, -1] += 1  # still a valid table, not the one the stream was coded under
    with pytest.raises(ValueError, match="CRC"):
        entropy.unpack_range(b2, crc2, 3, 9)
    with pytest.raises(ValueError):
        entropy.unpack_range(b2, t2[:3], 3, 9)  # K
    crc3 = t3.copy()
    crc3[0, 0, -1] += 1
    with pytest.raises(ValueError, match="CRC"):
        entropy.unpack_range(b3, crc3, 3, 9, geometry=geo)
    with pytest.raises(ValueError):
        entropy.unpack_range(b3, t3[:2], 3, 9, geometry=geo)  # K0
    with pytest.raises(ValueError, match="geometry"):
        entropy.unpack_range(b3, t3, 3, 9, geometry=(3, 2, 4))
    with pytest.raises(ValueError, match="neighbours"):
        entropy.unpack_range(b3, t3[:, :3], 3, 9, geometry=geo)
    with pytest.raises(ValueError):
        entropy.unpack_range(b3, t3, 3, 9)  # no geometry

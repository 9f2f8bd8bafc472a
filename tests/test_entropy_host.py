"""CPU tests of the segmented range-coder stream (include/tic.h, "TICS" version 1): the host
reference tic_rcseg_* behind tf_image_compression_amd.entropy.  A segment's payload is defined as
the bytes the file coder writes for it, so parity is against RangeEncoder / RangeDecoder files."""
import ctypes as C
import struct

import numpy as np
import pytest

from entropy_cases import TABLES, decode_file, draw, reference_container
from tf_image_compression_amd import entropy
from tf_image_compression_amd._lib import lib, u8p

NS = [1, 3, 4, 5, 4095, 4096, 4097, 3 * 4096 + 5]
LS = [4, 64, 4096]


@pytest.mark.parametrize("name", list(TABLES))
def test_pack_is_the_file_coder_per_segment(name, tmp_path):
    cum = TABLES[name]
    for n in NS:
        sym = draw(cum, n, seed=n)
        for L in LS + ([8192] if n < 8192 else []):  # 8192: L > n for every n but the last
            ref, _ = reference_container(sym, cum, L, tmp_path)
            got = entropy.pack(sym, cum, segment=L)
            assert got == ref, (name, n, L)
            assert len(got) <= entropy.bound(n, L)
            assert entropy.parse(got) == (L, n)


@pytest.mark.parametrize("name", list(TABLES))
def test_unpack_round_trip_and_file_decoder_per_segment(name, tmp_path):
    cum = TABLES[name]
    for n, L in [(1, 4), (5, 4), (4097, 64), (3 * 4096 + 5, 4096), (4095, 8192)]:
        sym = draw(cum, n, seed=100 + n)
        blob = entropy.pack(sym, cum, segment=L)
        assert np.array_equal(entropy.unpack(blob, cum), sym)
        assert np.array_equal(entropy.unpack(blob, cum, n=n), sym)
        # every segment's payload decodes as a file of its own
        S = -(-n // L)
        lens = struct.unpack_from(f"<{S}H", blob, 20)
        at = 20 + 2 * S
        for j in range(min(S, 40)):
            cnt = min(L, n - j * L)
            assert np.array_equal(decode_file(blob[at:at + lens[j]], cnt, cum, tmp_path), sym[j * L:j * L + cnt])
            at += lens[j]


def test_random_stream_with_ff_bytes():
    """The carry path: the 200 000-symbol stream the GPU test codes holds 0xFF payload bytes."""
    cum = TABLES["p98"]
    sym = draw(cum, 200000, seed=7)
    blob = entropy.pack(sym, cum, segment=4096)
    S = -(-200000 // 4096)
    assert b"\xff" in blob[20 + 2 * S:]
    assert np.array_equal(entropy.unpack(blob, cum), sym)


def test_bound_and_capacity():
    L = lib()
    cum = np.array(TABLES["total2p24"], np.int64)
    # the rarest symbol only: three bytes per symbol, the worst case the bound allows for
    sym = np.zeros(4099, np.uint8)
    for seg in (4, 64, 4096):
        cap = entropy.bound(sym.size, seg)
        S = -(-sym.size // seg)
        assert cap == 20 + 2 * S + 3 * sym.size + 4 * S
        out = np.empty(cap, np.uint8)
        w = C.c_size_t()
        args = (sym.ctypes.data_as(u8p), sym.size, seg, cum.ctypes.data_as(C.POINTER(C.c_int64)), cum.size,
                out.ctypes.data_as(u8p))
        assert L.tic_rcseg_encode(*args, cap, C.byref(w)) == 0
        assert 0 < w.value <= cap
        assert L.tic_rcseg_encode(*args, cap - 1, C.byref(w)) == -1
        assert b"tic_rcseg_bound" in L.tic_rc_last_error()
    for bad_L in (0, 6, 16388):
        with pytest.raises(ValueError):
            entropy.bound(10, bad_L)
    with pytest.raises(ValueError):
        entropy.bound(0, 4096)


def _valid():
    cum = TABLES["p60"]
    sym = draw(cum, 200, seed=3)
    return bytearray(entropy.pack(sym, cum, segment=64)), cum, sym  # 4 segments


def _mutations():
    blob, _, _ = _valid()
    S = 4
    lens = list(struct.unpack_from("<4H", blob, 20))

    def with_(off, data):
        b = bytearray(blob)
        b[off:off + len(data)] = data
        return bytes(b)

    def with_len(j, v, tail=b""):
        return with_(20 + 2 * j, struct.pack("<H", v)) + tail

    return {
        "magic": with_(0, b"TICX"),
        "version": with_(4, b"\x02"),
        "reserved": with_(6, b"\x01"),
        "L=0": with_(8, struct.pack("<I", 0)),
        "L=6": with_(8, struct.pack("<I", 6)),
        "L=16388": with_(8, struct.pack("<I", 16388)),
        "n=0": with_(12, struct.pack("<Q", 0)),
        "short header": bytes(blob[:19]),
        "truncated length table": bytes(blob[:20 + 2 * S - 1]),
        "n needs a longer table": with_(12, struct.pack("<Q", 64 * 4000)),
        # 8 symbols in the last segment: at most 28 bytes; the sum is kept right by padding
        "length above 3*len+4": with_len(3, 29, bytes(29 - lens[3])),
        "lengths sum to more": with_len(0, lens[0] + 1),
        "lengths sum to less": with_len(0, lens[0] - 1),
        "trailing byte": bytes(blob) + b"\x00",
        "missing last byte": bytes(blob[:-1]),
    }


@pytest.mark.parametrize("case", list(_mutations()))
def test_invalid_containers(case):
    blob, cum, sym = _valid()
    assert entropy.parse(blob) == (64, 200)
    bad = _mutations()[case]
    with pytest.raises(ValueError, match="segmented stream|not a segmented stream"):
        entropy.parse(bad)
    with pytest.raises(ValueError):
        entropy.unpack(bad, cum, n=200)


def test_count_must_match_the_header():
    blob, cum, sym = _valid()
    with pytest.raises(ValueError, match="200 symbols, 199 expected"):
        entropy.unpack(blob, cum, n=199)
    with pytest.raises(ValueError):
        entropy.unpack(blob, cum, n=201)
    assert np.array_equal(entropy.unpack(blob, cum, n=200), sym)


def test_plain_stream_is_not_a_container(tmp_path):
    from tf_image_compression_amd.range_coder import RangeEncoder
    p = str(tmp_path / "plain.encoded")
    e = RangeEncoder(p)
    e.encode([0, 1, 0, 0, 1] * 20, TABLES["p60"])
    e.close()
    data = open(p, "rb").read()
    assert not entropy.is_container(data)
    with pytest.raises(ValueError, match="not a segmented stream"):
        entropy.parse(data)


def test_table_contract():
    sym = np.array([0, 1, 2, 1], np.uint8)
    with pytest.raises(ValueError, match="outside the table"):
        entropy.pack(sym, [0, 2457, 4096])
    with pytest.raises(ValueError, match="frequency > 0"):
        entropy.pack(sym, [0, 10, 10, 4096])
    with pytest.raises(ValueError, match="at most 257"):
        entropy.pack(sym, list(range(258)))
    assert entropy.unpack(entropy.pack(sym, list(range(257))), list(range(257))).tolist() == [0, 1, 2, 1]
    with pytest.raises(OverflowError):
        entropy.pack(sym, [0, 1, 2, 2 ** 32])
    with pytest.raises(ValueError, match="2\\^24"):
        entropy.pack(sym, [0, 1, 2, 2 ** 24 + 1])
    blob = entropy.pack(sym, [0, 5, 9, 12])
    with pytest.raises(ValueError):
        entropy.unpack(blob, [0, 10, 10, 4096])
    with pytest.raises(ValueError):
        entropy.pack(np.array([300]), [0, 1, 2])
    with pytest.raises(ValueError):
        entropy.pack(np.zeros(0, np.uint8), [0, 1, 2])

"""CPU tests of the context stream (include/tic.h, "TICS" version 2): K cumulative tables, symbol
k of a stream under table k mod K.  A segment's payload is defined as the bytes RangeEncoder
writes when every symbol is passed in an encode() call of its own under its context's table, so
parity is against such files; the header and the length table are checked field by field."""
import ctypes as C
import math
import os
import struct

import numpy as np
import pytest

import encode
import get_encoded_distribution as ged
from conftest import ROOT
from entropy_ctx_cases import CASES, MIXED_TOTALS, case_tables, draw_ctx, make_tables, reference_container_ctx
from test_gpu_entropy import COUNTS_4, COUNTS_4096
from tf_image_compression_amd import entropy
from tf_image_compression_amd._lib import lib, u8p
from tf_image_compression_amd.evaluate import estimated_bits, estimated_bits_ctx
from tf_image_compression_amd.range_coder import symbol_table, symbol_tables


def counts_for(L):
    return COUNTS_4 if L == 4 else COUNTS_4096


def crc32c(data: bytes) -> int:
    """Bitwise CRC-32C (Castagnoli, reflected 0x82F63B78), independent of the library's."""
    crc = 0xFFFFFFFF
    for b in data:
        crc ^= b
        for _ in range(8):
            crc = (crc >> 1) ^ (0x82F63B78 if crc & 1 else 0)
    return crc ^ 0xFFFFFFFF


@pytest.mark.parametrize("name", list(CASES))
def test_pack_is_the_file_coder_per_symbol(name, tmp_path):
    K, ncum, L = CASES[name]
    tables = case_tables(name)
    assert tables.shape == (K, ncum)
    if name.endswith("mixed"):
        assert sorted(set(tables[:, -1].tolist())) == sorted(MIXED_TOTALS)
    for n in counts_for(L):
        sym = draw_ctx(tables, n, seed=n)
        ref, segs = reference_container_ctx(sym, tables, L, tmp_path)
        got = entropy.pack(sym, tables, segment=L)
        S = -(-n // L)
        # the header, field by field
        assert got[:4] == b"TICS" and got[4:8] == bytes([2, 0, 0, 0])
        assert struct.unpack_from("<IQII", got, 8) == (L, n, K, entropy.tables_crc(tables))
        assert list(struct.unpack_from(f"<{S}H", got, 28)) == [len(s) for s in segs]
        assert got[28 + 2 * S:] == b"".join(segs), (name, n)
        assert got == ref
        assert len(got) <= entropy.bound(n, L, tables) == entropy.bound(n, L) + 8
        assert entropy.parse_ctx(got) == (L, n, K, entropy.tables_crc(tables))
        assert np.array_equal(entropy.unpack(got, tables), sym)
        assert np.array_equal(entropy.unpack(got, tables, n=n), sym)


def test_tables_crc_is_crc32c_of_the_int64_entries():
    tables = case_tables("K3_mixed")
    assert entropy.tables_crc(tables) == crc32c(tables.astype("<i8").tobytes())
    assert entropy.tables_crc(tables.tolist()) == entropy.tables_crc(tables)


def test_one_context_is_version_1_behind_another_header():
    for L, counts in ((4, COUNTS_4), (4096, COUNTS_4096)):
        table = [0, 2457, 4096]
        for n in counts:
            sym = draw_ctx([table], n, seed=50 + n)
            v1, v2 = entropy.pack(sym, table, segment=L), entropy.pack(sym, [table], segment=L)
            assert v2[28:] == v1[20:]  # the length table and the payloads
            assert v2[:4] == v1[:4] and v2[8:20] == v1[8:20] and v2[4] == 2 and v1[4] == 1


def test_versions_do_not_cross():
    tables = case_tables("K3")
    sym = draw_ctx(tables, 300, seed=1)
    v2 = entropy.pack(sym, tables, segment=64)
    v1 = entropy.pack(sym, tables[0], segment=64)
    with pytest.raises(ValueError, match="version 2 is not supported"):
        entropy.parse(v2)
    a = np.frombuffer(v2, np.uint8)
    assert lib().tic_rcseg_parse(a.ctypes.data_as(u8p), a.size, None, None) == -1
    with pytest.raises(ValueError, match="version 1"):
        entropy.parse_ctx(v1)
    with pytest.raises(ValueError):
        entropy.unpack(v1, tables)
    with pytest.raises(ValueError):
        entropy.unpack(v2, tables[0])
    assert entropy.container_version(v1) == 1 and entropy.container_version(v2) == 2
    assert entropy.is_ctx_table(tables) and not entropy.is_ctx_table(tables[0]) and entropy.is_ctx_table([[0, 1, 2]])


def test_decode_rejects_other_tables_and_damaged_framing():
    tables = case_tables("K80")
    n, L = 3 * 4096 + 5, 4096
    sym = draw_ctx(tables, n, seed=2)
    blob = entropy.pack(sym, tables, segment=L)
    with pytest.raises(ValueError, match="80 tables, 79 given"):
        entropy.unpack(blob, tables[:79])
    other = tables.copy()
    other[41, 1] += 1  # one entry changed
    with pytest.raises(ValueError, match="CRC"):
        entropy.unpack(blob, other)
    wrong_k = bytearray(blob)
    wrong_k[20:24] = struct.pack("<I", 81)
    with pytest.raises(ValueError, match="81 tables"):
        entropy.unpack(bytes(wrong_k), tables)
    wrong_crc = bytearray(blob)
    wrong_crc[24] ^= 1
    with pytest.raises(ValueError, match="CRC"):
        entropy.unpack(bytes(wrong_crc), tables)
    for k in (0, 0x10000 + 1):
        bad = bytearray(blob)
        bad[20:24] = struct.pack("<I", k)
        with pytest.raises(ValueError, match="context count"):
            entropy.parse_ctx(bytes(bad))
    for cut in (0, 3, 19, 20, 27, 28, 30, 35, len(blob) - 1):
        with pytest.raises(ValueError):
            entropy.parse_ctx(blob[:cut])
        with pytest.raises(ValueError):
            entropy.unpack(blob[:cut], tables, n=n)
    with pytest.raises(ValueError):
        entropy.parse_ctx(blob + b"\0")
    # a length past 3 * len + 4 (the last segment holds 5 symbols: at most 19 bytes)
    S = -(-n // L)
    lens = list(struct.unpack_from(f"<{S}H", blob, 28))
    move = 20 - lens[-1]
    lens[-1] += move
    lens[0] -= move
    long_seg = blob[:28] + struct.pack(f"<{S}H", *lens) + blob[28 + 2 * S:]
    with pytest.raises(ValueError, match="claims 20 bytes for 5 symbols"):
        entropy.parse_ctx(long_seg)
    with pytest.raises(ValueError, match="symbols"):
        entropy.unpack(blob, tables, n=n + 1)


def test_tables_are_validated():
    sym = np.zeros(8, np.uint8)
    good = make_tables(4, 3, seed=0)
    assert entropy.unpack(entropy.pack(sym, good, segment=4), good).tolist() == [0] * 8
    L = lib()
    out = np.empty(256, np.uint8)
    w = C.c_size_t()
    i64 = C.POINTER(C.c_int64)

    def enc(tables, K, ncum):
        t = np.ascontiguousarray(tables, np.int64)
        return L.tic_rcseg_encode_ctx(sym.ctypes.data_as(u8p), 8, 4, t.ctypes.data_as(i64), K, ncum,
                                      out.ctypes.data_as(u8p), out.size, C.byref(w))

    assert enc(good, 4, 3) == 0
    assert enc(good, 0, 3) == -1 and b"context count" in L.tic_rc_last_error()
    assert enc(good, 65537, 3) == -1
    assert enc(good, 4, 1) == -1 and enc(good, 4, 258) == -1
    big = make_tables(1024, 257, seed=1)  # 263 168 entries: over the limit of 262 144
    assert enc(big, 1024, 257) == -1 and b"262144" in L.tic_rc_last_error()
    assert enc(big, 1020, 257) == 0  # 262 140 entries
    for row, bad_row, code in ((2, [0, 7, 7], -1), (3, [0, 0, 9], -1), (1, [1, 2, 3], -1), (0, [0, 5, 4], -1),
                               (2, [0, 1, (1 << 24) + 1], -1), (1, [0, 1, 1 << 32], -7)):
        bad = good.copy()
        bad[row] = bad_row
        assert enc(bad, 4, 3) == code, bad_row
        assert f"context {row}:".encode() in L.tic_rc_last_error()
        blob = entropy.pack(sym, good, segment=4)
        a = np.frombuffer(blob, np.uint8)
        back = np.empty(8, np.uint8)
        assert L.tic_rcseg_decode_ctx(a.ctypes.data_as(u8p), a.size, bad.ctypes.data_as(i64), 4, 3,
                                      back.ctypes.data_as(u8p), 8) == code
    with pytest.raises(ValueError, match="zero|frequency > 0"):
        entropy.pack(sym, [[0, 5, 9], [0, 5, 5]], segment=4)
    with pytest.raises(ValueError, match="common length"):
        entropy.pack(sym, [[0, 5, 9], [0, 5, 7, 9]], segment=4)
    with pytest.raises(ValueError, match="outside the table"):
        entropy.pack(np.array([0, 1, 2], np.uint8), good, segment=4)
    small = np.empty(entropy.bound(8, 4, good) - 1, np.uint8)
    assert L.tic_rcseg_encode_ctx(sym.ctypes.data_as(u8p), 8, 4, good.ctypes.data_as(i64), 4, 3,
                                  small.ctypes.data_as(u8p), small.size, C.byref(w)) == -1
    assert b"below tic_rcseg_bound_ctx" in L.tic_rc_last_error()


def test_symbol_tables_and_estimated_bits_ctx():
    prob = np.array([[0.9, 0.1], [0.2, 0.8], [0.5, 0.5]])
    tables = symbol_tables(prob, resolution=4096)
    assert tables.shape == (3, 3) and tables.dtype == np.int64
    assert [row.tolist() for row in tables] == [symbol_table(p, resolution=4096) for p in prob]
    with pytest.raises(ValueError):
        symbol_tables(prob[0])
    counts = np.array([[10, 0], [3, 7], [0, 0]])
    want = sum(estimated_bits(c, t) for c, t in zip(counts, tables))
    assert abs(estimated_bits_ctx(counts, tables) - want) <= 1e-12 * want
    with pytest.raises(ValueError):
        estimated_bits_ctx(counts[:2], tables)


def test_per_channel_tables_halve_the_golden_code():
    """tests/golden/model0_p256.npz idx (16 * 16 * 64 bits): under tables from its own per-channel
    histogram the version-2 container is below 0.60 of the version-1 container under the global
    table (ideal code lengths: 930 B against 1926 B, a ratio of 0.48; the cap leaves room for the
    28-byte header and 2 + 5 bytes of length entry and flush for each of the 8 segments and cannot
    be met without context coding), and within 28 + 8 * S bytes of its ideal code length."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "model0_p256.npz"), allow_pickle=False)
    idx = z["idx"]
    C_, L = idx.shape[-1], 2048
    sym = idx.reshape(-1)
    S = -(-sym.size // L)
    glob = np.bincount(sym, minlength=2).astype(np.float64)
    per = np.stack([np.bincount(idx[..., c].reshape(-1), minlength=2) for c in range(C_)]).astype(np.float64)
    table = symbol_table(glob / glob.sum(), resolution=4096)
    tables = symbol_tables(per / per.sum(axis=1, keepdims=True), resolution=4096)
    v1 = entropy.pack(sym, table, segment=L)
    v2 = entropy.pack(sym, tables, segment=L)
    assert np.array_equal(entropy.unpack(v2, tables), sym)
    est = estimated_bits_ctx(per, tables)
    print(f"v1 {len(v1)} B, v2 {len(v2)} B, ratio {len(v2) / len(v1):.4f}, ideal {est / 8:.1f} B, "
          f"framing and flush {len(v2) - math.ceil(est / 8)} B of {28 + 8 * S} allowed")
    assert len(v2) < 0.60 * len(v1)
    assert len(v2) <= math.ceil(est / 8) + 28 + 8 * S


def test_cli_context_arguments(tmp_path):
    a = ged.my_parse_args(["-m", "0", "-g", "0"])
    assert a.context == "none" and a.output_file == "data_info/distribution_info_{}.npy"
    assert a.context_output == "data_info/distribution_ctx_{}.npy"
    for mode in ("channel", "position"):
        assert ged.my_parse_args(["-m", "3", "-g", "0", "--context", mode]).context == mode
    with pytest.raises(SystemExit):
        ged.my_parse_args(["-m", "0", "-g", "0", "--context", "pixel"])
    assert ged.context_count("none", (16, 16, 64)) == 1
    assert ged.context_count("channel", (16, 16, 64)) == 64
    assert ged.context_count("channel", (8, 8, 80)) == 80
    assert ged.context_count("position", (16, 16, 64)) == 16384
    assert ged.context_count("position", (8, 8, 80)) == 5120


def test_host_coder_refuses_context_distribution(tmp_path, capsys):
    import decode
    import evaluate_codec
    np.save(tmp_path / "ctx_0.npy", np.full((64, 2), 0.5))
    np.save(tmp_path / "flat_0.npy", np.array([0.6, 0.4]))
    for mod in (encode, decode, evaluate_codec):
        with pytest.raises(SystemExit):
            mod.my_parse_args(["-m", "0", "-g", "0", "--entropy", "host", "--dist", str(tmp_path / "ctx_{}.npy")])
        assert "--entropy device" in capsys.readouterr().err
        with pytest.raises(SystemExit):  # host is the default
            mod.my_parse_args(["-m", "0", "-g", "0", "--dist", str(tmp_path / "ctx_{}.npy")])
        capsys.readouterr()
        mod.my_parse_args(["-m", "0", "-g", "0", "--entropy", "device", "--dist", str(tmp_path / "ctx_{}.npy")])
        mod.my_parse_args(["-m", "0", "-g", "0", "--entropy", "host", "--dist", str(tmp_path / "flat_{}.npy")])
        mod.my_parse_args(["-m", "0", "-g", "0", "--dist", str(tmp_path / "missing_{}.npy")])

"""Shared by the segmented-stream tests: the tables, symbol sources and the container built
from what ``RangeEncoder`` writes per segment to files (the format's definition)."""
import os
import struct

import numpy as np

from tf_image_compression_amd.range_coder import RangeDecoder, RangeEncoder, symbol_table


def table_256():
    p = np.exp(-0.04 * np.arange(256))
    return symbol_table(p / p.sum(), resolution=4096)


TABLES = {
    "p60": [0, 2457, 4096],
    "p98": [0, 4013, 4096],
    "p4095": [0, 4095, 4096],
    "sym256": table_256(),
    "total5000": [0, 3000, 4999, 5000],
    "total2p24": [0, 1, 9000000, 1 << 24],
    # beyond the issue's list: the largest total the device decodes through its LDS byte table
    "total65536": [0, 60000, 65535, 65536],
}


def draw(cum, n, seed):
    """n symbols distributed as the table says."""
    rng = np.random.default_rng(seed)
    p = np.diff(np.asarray(cum, np.float64))
    return rng.choice(len(p), size=n, p=p / p.sum()).astype(np.uint8)


def segment_files(sym, cum, L, tmpdir):
    """One RangeEncoder file per segment; their bytes."""
    out = []
    path = os.path.join(str(tmpdir), "seg.bin")
    for b in range(0, len(sym), L):
        e = RangeEncoder(path)
        e.encode(sym[b:b + L].astype(np.int64), cum)
        e.close()
        with open(path, "rb") as f:
            out.append(f.read())
    return out


def reference_container(sym, cum, L, tmpdir):
    segs = segment_files(sym, cum, L, tmpdir)
    head = b"TICS" + bytes([1, 0, 0, 0]) + struct.pack("<IQ", L, len(sym))
    return head + b"".join(struct.pack("<H", len(s)) for s in segs) + b"".join(segs), segs


def decode_file(payload, n, cum, tmpdir):
    path = os.path.join(str(tmpdir), "dec.bin")
    with open(path, "wb") as f:
        f.write(payload)
    d = RangeDecoder(path)
    out = d.decode_array(n, cum)
    d.close()
    return out.astype(np.uint8)

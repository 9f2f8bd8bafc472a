"""Shared by the context-stream tests ("TICS" version 2): the table sets, symbol sources and the
container built from what ``RangeEncoder`` writes per segment when every symbol goes through an
``encode()`` call of its own under its context's table (the format's definition)."""
import os
import struct

import numpy as np

from tf_image_compression_amd import entropy
from tf_image_compression_amd.range_coder import RangeEncoder

MIXED_TOTALS = (4096, 5000, 1 << 24)


def make_tables(K, ncum, seed, totals=(4096,)):
    """[K, ncum] int64 tables with every frequency > 0; row k's total is totals[k % len(totals)].
    Rows are biased one way or the other, as the channels of a code are."""
    rng = np.random.default_rng(seed)
    nsym = ncum - 1
    out = np.zeros((K, ncum), np.int64)
    for k in range(K):
        total = int(totals[k % len(totals)])
        p = rng.random(nsym) ** 4 + 1e-3
        p[rng.integers(nsym)] += nsym  # one dominant symbol
        freq = 1 + np.floor(p / p.sum() * (total - nsym)).astype(np.int64)
        freq[0] += total - int(freq.sum())
        assert freq.min() >= 1 and int(freq.sum()) == total
        out[k, 1:] = np.cumsum(freq)
    return out


# name -> (K, ncum, L); "mixed" rows have the totals 4096, 5000 and 2^24 in turn
CASES = {
    "K1": (1, 3, 4),
    "K3": (3, 3, 4),
    "K3_mixed": (3, 3, 4),
    "K64": (64, 3, 4096),
    "K80": (80, 3, 4096),  # 4096 mod 80 != 0: segments start inside the period
    "K5_sym256": (5, 257, 2048),
}


def case_tables(name):
    K, ncum, _ = CASES[name]
    return make_tables(K, ncum, seed=sum(name.encode()), totals=MIXED_TOTALS if name.endswith("mixed") else (4096,))


def draw_ctx(tables, n, seed):
    """n symbols, symbol i distributed as row i mod K says (a stream starts at context 0)."""
    t = np.asarray(tables, np.int64)
    rng = np.random.default_rng(seed)
    rows = t[np.arange(n) % t.shape[0]]
    val = np.floor(rng.random(n) * rows[:, -1]).astype(np.int64)
    return (val[:, None] >= rows[:, 1:-1]).sum(axis=1).astype(np.uint8)


def segment_files_ctx(sym, tables, L, tmpdir):
    """One RangeEncoder file per segment, one encode() call per symbol; their bytes."""
    rows = [[int(v) for v in row] for row in np.asarray(tables)]
    K = len(rows)
    out = []
    path = os.path.join(str(tmpdir), "seg_ctx.bin")
    for b in range(0, len(sym), L):
        e = RangeEncoder(path)
        for i in range(b, min(len(sym), b + L)):
            e.encode([int(sym[i])], rows[i % K])
        e.close()
        with open(path, "rb") as f:
            out.append(f.read())
    return out


def reference_container_ctx(sym, tables, L, tmpdir):
    segs = segment_files_ctx(sym, tables, L, tmpdir)
    t = np.asarray(tables, np.int64)
    head = (b"TICS" + bytes([2, 0, 0, 0]) + struct.pack("<IQ", L, len(sym))
            + struct.pack("<II", t.shape[0], entropy.tables_crc(t)))
    return head + b"".join(struct.pack("<H", len(s)) for s in segs) + b"".join(segs), segs

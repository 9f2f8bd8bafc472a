"""Segmented range-coder streams ("TICS" versions 1 to 3, include/tic.h), host side.

A container cuts a symbol sequence into segments of ``L`` symbols, each an independent stream of
the range coder in csrc/range_coder.cpp (byte for byte what ``RangeEncoder`` writes for the
segment), behind a header and a table of u16 segment lengths.  Independent segments are what the
device coder (csrc/tic_entropy.cpp, ``Codec.entropy_encode_device``) runs one per lane; the
functions here are its reference and read or write a container without a GPU.

Symbols are bytes; the table is a ``range_coder`` cumulative table with at most 256 symbols and
no zero frequency.  Errors are mapped as ``range_coder._raise`` maps them.

A 2-D table ``[K, ncum]`` selects the periodic context model of version 2: symbol ``k`` of the
stream is coded under row ``k mod K`` (``K`` = the code's channel count: one table per channel;
``K`` = the symbols of a patch: one per code position).  ``pack``, ``unpack`` and ``bound`` take
either kind of table; ``parse`` reads version 1 only and ``parse_ctx`` version 2 only.

``range_extent`` and ``unpack_range`` read a symbol range out of a container of any version: the
segments that hold it and nothing else.

A 3-D table ``[K0, M, ncum]`` selects the causal-neighbour model of version 3 and needs
``geometry=(eh, ew, C)``, the shape of the code the symbols are a patch-major sequence of:
``M`` = 3 conditions every symbol on the class of its W neighbour (one position to the left, same
channel), ``M`` = 9 on W and N (one row up); symbol ``k`` is coded under row ``k mod K0`` of the
tables, entry ``nb`` (include/tic.h has the definition).  ``parse_nbr`` reads version 3 only.

An ``Adaptive`` in place of a table selects a "TICA" container: the same context rows, under
tables fitted to the stream's own counts by an integer rule and written into the container, so
``unpack`` and ``unpack_range`` take ``None`` for the table.  ``parse_emb`` and ``range_extent_emb``
read these containers only; the "TICS" functions reject them.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import math

import numpy as np

from ._lib import lib, u8p
from .range_coder import _raise, _table

MAGIC = b"TICS"
HEADER_BYTES = 20
HEADER_BYTES_CTX = 28
HEADER_BYTES_NBR = 36
DEFAULT_SEGMENT = 2048  # faster than 4096 end to end, under 1 % bytes over the single stream


def _u8(a):
    return a.ctypes.data_as(u8p)


def _i64(a):
    return a.ctypes.data_as(C.POINTER(C.c_int64))


def _symbols(symbols) -> np.ndarray:
    a = np.asarray(symbols)
    if a.dtype != np.uint8:
        if a.size and (a.min() < 0 or a.max() > 255):
            raise ValueError("segmented streams code byte symbols (0..255)")
        a = a.astype(np.uint8)
    return np.ascontiguousarray(a.reshape(-1))


def is_container(buf) -> bool:
    """True when ``buf`` starts with the container's magic (no validation)."""
    return bytes(buf[:4]) == MAGIC


def container_version(buf) -> int:
    """The version byte of a container (no validation); ValueError without the magic."""
    if not is_container(buf) or len(buf) < 5:
        raise ValueError("not a segmented stream: magic is not \"TICS\"")
    return int(bytes(buf[4:5])[0])


def is_ctx_table(cum_freq) -> bool:
    """True for a 2-D ``[K, ncum]`` table (version 2), False for a 1-D one (version 1) and for a
    3-D one (version 3, ``is_nbr_table``)."""
    try:
        return len(cum_freq) > 0 and np.ndim(cum_freq[0]) > 0 and not is_nbr_table(cum_freq)
    except TypeError:
        return False


def is_nbr_table(cum_freq) -> bool:
    """True for a 3-D ``[K0, M, ncum]`` table (version 3)."""
    try:
        return len(cum_freq) > 0 and np.ndim(cum_freq[0]) > 1
    except TypeError:
        return False


def nbr_tables(tables) -> np.ndarray:
    """``[K0, M, ncum]`` cumulative tables as a C-contiguous int64 array; ``M`` is 3 (W) or 9
    (W and N)."""
    rows = [ctx_tables(block) for block in tables]
    if not rows or len({r.shape for r in rows}) != 1:
        raise ValueError("neighbour tables need at least one context and one common shape")
    t = np.ascontiguousarray(np.stack(rows))
    if t.shape[1] not in (3, 9):
        raise ValueError(f"neighbour tables are [K0, 3 or 9, ncum], got shape {t.shape}")
    return t


def neighbours_of(tables) -> int:
    """1 for ``[K0, 3, ncum]`` tables, 2 for ``[K0, 9, ncum]``."""
    return {3: 1, 9: 2}[nbr_tables(tables).shape[1]]


def _geometry(geometry):
    if geometry is None:
        raise ValueError("3-D (neighbour) tables need geometry=(eh, ew, C)")
    eh, ew, c = (int(v) for v in geometry)
    if not all(1 <= v <= 65535 for v in (eh, ew, c)):
        raise ValueError(f"code geometry {eh} x {ew} x {c} must be in [1, 65535] each")
    return eh, ew, c


def ctx_tables(tables) -> np.ndarray:
    """``[K, ncum]`` cumulative tables as a C-contiguous int64 array (``range_coder`` contract
    per entry: integers below 2^32)."""
    rows = [_table(row) for row in tables]
    if not rows or len({r.size for r in rows}) != 1:
        raise ValueError("context tables need at least one row and one common length")
    return np.ascontiguousarray(np.stack(rows))


def tables_crc(tables) -> int:
    """The CRC-32C a version-2 or version-3 header carries: of the ``K * ncum`` entries (2-D or
    3-D tables) as little-endian int64, row-major."""
    t = nbr_tables(tables) if is_nbr_table(tables) else ctx_tables(tables)
    data = t.astype("<i8").tobytes()
    return int(lib().tic_crc32c(data, len(data), 0))


def bound(n: int, segment: int = DEFAULT_SEGMENT, cum_freq=None, geometry=None) -> int:
    """Worst-case container size for ``n`` symbols (version 2 when ``cum_freq`` is 2-D, version 3
    when it is 3-D; a "TICA" container when it is an ``Adaptive``, which needs ``geometry``)."""
    out = C.c_size_t()
    if isinstance(cum_freq, Adaptive):
        model = cum_freq.widest()
        rc = lib().tic_rcseg_bound_emb(int(n), int(segment), model.K0(_geometry(geometry)[2]), model.neighbours,
                                       model.nsym, C.byref(out))
        if rc:
            _raise(rc, "entropy.bound")
        return int(out.value)
    fn = lib().tic_rcseg_bound
    if cum_freq is not None and is_nbr_table(cum_freq):
        fn = lib().tic_rcseg_bound_nbr
    elif cum_freq is not None and is_ctx_table(cum_freq):
        fn = lib().tic_rcseg_bound_ctx
    rc = fn(int(n), int(segment), C.byref(out))
    if rc:
        _raise(rc, "entropy.bound")
    return int(out.value)


def pack(symbols, cum_freq, segment: int = DEFAULT_SEGMENT, geometry=None) -> bytes:
    """The container of ``symbols`` (flattened in C order); version 2 under a 2-D table, version 3
    under a 3-D one (with ``geometry``); a "TICA" container under an ``Adaptive`` (with
    ``geometry``)."""
    if isinstance(cum_freq, Adaptive):
        return _pack_emb(symbols, cum_freq, segment, geometry)
    ctx, nbr = is_ctx_table(cum_freq), is_nbr_table(cum_freq)
    table = nbr_tables(cum_freq) if nbr else ctx_tables(cum_freq) if ctx else _table(cum_freq)
    sym = _symbols(symbols)
    cap = bound(sym.size, segment, cum_freq)
    out = np.empty(cap, np.uint8)
    written = C.c_size_t()
    if nbr:
        eh, ew, c = _geometry(geometry)
        rc = lib().tic_rcseg_encode_nbr(_u8(sym), sym.size, int(segment), _i64(table), table.shape[0],
                                        neighbours_of(table), table.shape[2], eh, ew, c, _u8(out), cap,
                                        C.byref(written))
    elif ctx:
        rc = lib().tic_rcseg_encode_ctx(_u8(sym), sym.size, int(segment), _i64(table), table.shape[0],
                                        table.shape[1], _u8(out), cap, C.byref(written))
    else:
        rc = lib().tic_rcseg_encode(_u8(sym), sym.size, int(segment), _i64(table), table.size, _u8(out), cap,
                                    C.byref(written))
    if rc:
        _raise(rc, "entropy.pack")
    return out[:written.value].tobytes()


def parse(buf) -> tuple[int, int]:
    """Validate a container; ``(L, n)``."""
    a = np.frombuffer(bytes(buf), np.uint8)
    L, n = C.c_uint32(), C.c_uint64()
    rc = lib().tic_rcseg_parse(_u8(a) if a.size else None, a.size, C.byref(L), C.byref(n))
    if rc:
        _raise(rc, "entropy.parse")
    return int(L.value), int(n.value)


def parse_ctx(buf) -> tuple[int, int, int, int]:
    """Validate a version-2 container; ``(L, n, K, crc)``."""
    a = np.frombuffer(bytes(buf), np.uint8)
    L, n, K, crc = C.c_uint32(), C.c_uint64(), C.c_uint32(), C.c_uint32()
    rc = lib().tic_rcseg_parse_ctx(_u8(a) if a.size else None, a.size, C.byref(L), C.byref(n), C.byref(K),
                                   C.byref(crc))
    if rc:
        _raise(rc, "entropy.parse_ctx")
    return int(L.value), int(n.value), int(K.value), int(crc.value)


def parse_nbr(buf) -> tuple[int, int, int, int, tuple[int, int, int], int]:
    """Validate a version-3 container; ``(L, n, K0, crc, (eh, ew, C), neighbours)``."""
    a = np.frombuffer(bytes(buf), np.uint8)
    L, n = C.c_uint32(), C.c_uint64()
    f = [C.c_uint32() for _ in range(6)]
    rc = lib().tic_rcseg_parse_nbr(_u8(a) if a.size else None, a.size, C.byref(L), C.byref(n),
                                   *[C.byref(v) for v in f])
    if rc:
        _raise(rc, "entropy.parse_nbr")
    K0, crc, eh, ew, c, nb = (int(v.value) for v in f)
    return int(L.value), int(n.value), K0, crc, (eh, ew, c), nb


def unpack(buf, cum_freq, n: int | None = None, geometry=None) -> np.ndarray:
    """The symbols of a container (uint8); ``n``, when given, must be the header's count.  A 2-D
    table reads version 2 and must be the one the container was packed under (its K and CRC); a
    3-D table reads version 3 and must match its K0, ``neighbours``, CRC and ``geometry``.
    ``None`` or an ``Adaptive`` reads a "TICA" container, which carries its own tables."""
    if cum_freq is None or isinstance(cum_freq, Adaptive):
        a = np.frombuffer(bytes(buf), np.uint8)
        if n is None:
            n = parse_emb(a)["n"]
        out = np.empty(int(n), np.uint8)
        rc = lib().tic_rcseg_decode_emb(_u8(a) if a.size else None, a.size, _u8(out), int(n))
        if rc:
            _raise(rc, "entropy.unpack")
        return out
    ctx, nbr = is_ctx_table(cum_freq), is_nbr_table(cum_freq)
    table = nbr_tables(cum_freq) if nbr else ctx_tables(cum_freq) if ctx else _table(cum_freq)
    a = np.frombuffer(bytes(buf), np.uint8)
    if n is None:
        n = parse_nbr(a)[1] if nbr else parse_ctx(a)[1] if ctx else parse(a)[1]
    out = np.empty(int(n), np.uint8)
    if nbr:
        eh, ew, c = _geometry(geometry)
        rc = lib().tic_rcseg_decode_nbr(_u8(a) if a.size else None, a.size, _i64(table), table.shape[0],
                                        neighbours_of(table), table.shape[2], eh, ew, c, _u8(out), int(n))
    elif ctx:
        rc = lib().tic_rcseg_decode_ctx(_u8(a) if a.size else None, a.size, _i64(table), table.shape[0],
                                        table.shape[1], _u8(out), int(n))
    else:
        rc = lib().tic_rcseg_decode(_u8(a) if a.size else None, a.size, _i64(table), table.size, _u8(out), int(n))
    if rc:
        _raise(rc, "entropy.unpack")
    return out


def range_extent(buf, first: int, count: int) -> tuple[int, int, int, int]:
    """``(j0, nj, byte_off, byte_len)``: the segments ``j0 .. j0 + nj - 1`` that hold symbols
    ``[first, first + count)`` of a container of any version, and the byte extent of their
    payloads from the container's start.  ``buf`` needs to hold the header and the length table
    only."""
    if int(first) < 0 or int(count) < 0:
        raise ValueError(f"symbol range [{first}, {first} + {count}) is negative")
    a = np.frombuffer(bytes(buf), np.uint8)
    out = [C.c_size_t() for _ in range(4)]
    rc = lib().tic_rcseg_range_extent(_u8(a) if a.size else None, a.size, int(first), int(count),
                                      *[C.byref(v) for v in out])
    if rc:
        _raise(rc, "entropy.range_extent")
    return tuple(int(v.value) for v in out)


def unpack_range(buf, cum_freq, first: int, count: int, geometry=None) -> np.ndarray:
    """``unpack(buf, cum_freq, geometry=geometry)[first:first + count]`` decoding only the
    segments that hold the range (no payload byte outside ``range_extent``'s extent is read).
    The version follows the table's rank as in ``unpack``, with the same checks."""
    if int(first) < 0 or int(count) < 0:
        raise ValueError(f"symbol range [{first}, {first} + {count}) is negative")
    if cum_freq is None or isinstance(cum_freq, Adaptive):
        a = np.frombuffer(bytes(buf), np.uint8)
        n = parse_emb(a)["n"]
        out = np.empty(max(int(count), 1), np.uint8)
        rc = lib().tic_rcseg_decode_range_emb(_u8(a) if a.size else None, a.size, _u8(out), n, int(first),
                                              int(count))
        if rc:
            _raise(rc, "entropy.unpack_range")
        return out[:int(count)]
    ctx, nbr = is_ctx_table(cum_freq), is_nbr_table(cum_freq)
    table = nbr_tables(cum_freq) if nbr else ctx_tables(cum_freq) if ctx else _table(cum_freq)
    a = np.frombuffer(bytes(buf), np.uint8)
    n = parse_nbr(a)[1] if nbr else parse_ctx(a)[1] if ctx else parse(a)[1]
    out = np.empty(max(int(count), 1), np.uint8)
    pa = _u8(a) if a.size else None
    if nbr:
        eh, ew, c = _geometry(geometry)
        rc = lib().tic_rcseg_decode_range_nbr(pa, a.size, _i64(table), table.shape[0], neighbours_of(table),
                                              table.shape[2], eh, ew, c, _u8(out), n, int(first), int(count))
    elif ctx:
        rc = lib().tic_rcseg_decode_range_ctx(pa, a.size, _i64(table), table.shape[0], table.shape[1], _u8(out), n,
                                              int(first), int(count))
    else:
        rc = lib().tic_rcseg_decode_range(pa, a.size, _i64(table), table.size, _u8(out), n, int(first), int(count))
    if rc:
        _raise(rc, "entropy.unpack_range")
    return out[:int(count)]


# --- "TICA": containers that carry tables fitted to their own symbols (include/tic.h) ---

MAGIC_EMB = b"TICA"
HEADER_BYTES_EMB = 40
EMB_TOTAL = 4096


@dataclasses.dataclass(frozen=True)
class Adaptive:
    """The model of a "TICA" container, in place of a table: the tables are fitted to the stream
    and written into it.  ``context`` "none" is one periodic context (K0 = 1), "channel" one per
    channel of the code (K0 = C); ``neighbours`` 0, 1 (W) or 2 (W and N) as version 3.
    ``Adaptive.auto()`` lets ``choose_model`` pick per stream."""
    context: str = "channel"
    neighbours: int = 0
    nsym: int = 2
    automatic: bool = False

    def __post_init__(self):
        if self.context not in ("none", "channel"):
            raise ValueError(f"context {self.context!r} must be 'none' or 'channel'")
        if self.neighbours not in (0, 1, 2):
            raise ValueError(f"neighbours {self.neighbours!r} must be 0, 1 or 2")
        if not 2 <= int(self.nsym) <= 256:
            raise ValueError(f"nsym {self.nsym!r} must be in [2, 256]")

    @classmethod
    def auto(cls, nsym: int = 2) -> "Adaptive":
        return cls("channel", 2, nsym, True)

    def K0(self, channels: int) -> int:
        return int(channels) if self.context == "channel" else 1

    @property
    def M(self) -> int:
        return 3 ** self.neighbours

    def widest(self) -> "Adaptive":
        """The candidate with the largest table block (what ``bound`` must allow for)."""
        return Adaptive("channel", 2, self.nsym) if self.automatic else self

    def candidates(self) -> list["Adaptive"]:
        """What ``choose_model`` chooses among, in tie-break order."""
        return [Adaptive("none", 0, self.nsym), Adaptive("channel", 0, self.nsym),
                Adaptive("channel", 1, self.nsym), Adaptive("channel", 2, self.nsym)]


def is_adaptive(buf) -> bool:
    """True when ``buf`` starts with the "TICA" magic (no validation)."""
    return bytes(buf[:4]) == MAGIC_EMB


def count_rows(symbols, model: Adaptive, geometry, segment: int = DEFAULT_SEGMENT) -> np.ndarray:
    """uint64 counts ``[K0*M, nsym]`` of the symbols under ``model``'s rows at segment length
    ``segment`` (``Adaptive.auto()``: the (channel, 2) rows ``choose_model`` takes)."""
    model = model.widest()
    eh, ew, c = _geometry(geometry)
    sym = _symbols(symbols)
    out = np.zeros((model.K0(c) * model.M, model.nsym), np.uint64)
    rc = lib().tic_rcseg_count_nbr(_u8(sym) if sym.size else None, sym.size, int(segment), model.K0(c),
                                   model.neighbours, model.nsym, eh, ew, c,
                                   out.ctypes.data_as(C.POINTER(C.c_uint64)))
    if rc:
        _raise(rc, "entropy.count_rows")
    return out


def fit_tables(counts) -> np.ndarray:
    """The fit rule of include/tic.h: counts ``[K, nsym]`` to int64 cumulative tables
    ``[K, nsym + 1]`` with totals 4096 and no zero frequency."""
    c = np.ascontiguousarray(np.asarray(counts, dtype=np.uint64))
    if c.ndim != 2:
        raise ValueError(f"counts are [K, nsym], got shape {c.shape}")
    out = np.empty((c.shape[0], c.shape[1] + 1), np.int64)
    rc = lib().tic_rcseg_fit_tables(c.ctypes.data_as(C.POINTER(C.c_uint64)), c.shape[0], c.shape[1], _i64(out))
    if rc:
        _raise(rc, "entropy.fit_tables")
    return out


def marginal_counts(counts_c_wn, model: Adaptive, channels: int) -> np.ndarray:
    """The counts of ``model``'s rows from the ``[C*9, nsym]`` counts of (channel, 2): row
    c*9 + tW + 3*tN is summed over what ``model`` does not condition on."""
    full = np.asarray(counts_c_wn, dtype=np.uint64).reshape(int(channels), 3, 3, -1)  # [c, tN, tW, s]
    if model.neighbours == 2:
        m = full.reshape(int(channels), 9, -1)
    elif model.neighbours == 1:
        m = full.sum(axis=1, dtype=np.uint64)
    else:
        m = full.sum(axis=(1, 2), dtype=np.uint64)[:, None, :]
    if model.context == "none":
        if model.neighbours:
            raise ValueError("neighbour rows of one context are not a marginal of per-channel rows at K0 = C")
        m = m.sum(axis=0, dtype=np.uint64)[None]
    return np.ascontiguousarray(m.reshape(-1, full.shape[-1]))


def estimate_bytes(counts) -> int:
    """``T + ceil(sum(-c * log2(f / 4096)) / 8)`` in float64 under the tables fitted to ``counts``:
    the table block plus the ideal code length, what ``choose_model`` compares."""
    c = np.asarray(counts, dtype=np.uint64)
    f = np.diff(fit_tables(c), axis=1).astype(np.float64)
    bits = float(np.sum(-c.astype(np.float64) * np.log2(f / EMB_TOTAL)))
    return int(c.shape[0] * (c.shape[1] - 1) * 2 + math.ceil(bits / 8))


def choose_model(counts_c_wn, n: int, channels: int) -> Adaptive:
    """The candidate (``Adaptive.candidates``) with the smallest ``estimate_bytes``, the earlier one
    on ties, from a stream's ``[C*9, nsym]`` counts under (channel, 2).  ``n``: the stream's symbol
    count, which the counts must sum to."""
    c = np.asarray(counts_c_wn, dtype=np.uint64)
    if c.ndim != 2 or c.shape[0] != 9 * int(channels):
        raise ValueError(f"counts are [C*9, nsym] = [{9 * int(channels)}, nsym], got shape {c.shape}")
    if int(c.sum(dtype=np.uint64)) != int(n):
        raise ValueError(f"counts sum to {int(c.sum(dtype=np.uint64))}, the stream has {n} symbols")
    cands = Adaptive(nsym=c.shape[1]).candidates()
    cost = [estimate_bytes(marginal_counts(c, m, channels)) for m in cands]
    return cands[int(np.argmin(cost))]  # argmin returns the first of equal minima


def _pack_emb(symbols, model: Adaptive, segment, geometry) -> bytes:
    eh, ew, c = _geometry(geometry)
    sym = _symbols(symbols)
    if model.automatic:
        model = choose_model(count_rows(sym, model, geometry, segment), sym.size, c)
    cap = bound(sym.size, segment, model, geometry)
    out = np.empty(cap, np.uint8)
    written = C.c_size_t()
    rc = lib().tic_rcseg_encode_emb(_u8(sym), sym.size, int(segment), model.K0(c), model.neighbours, model.nsym,
                                    eh, ew, c, _u8(out), cap, C.byref(written))
    if rc:
        _raise(rc, "entropy.pack")
    return out[:written.value].tobytes()


def parse_emb(buf) -> dict:
    """Validate a "TICA" container; its header as a dict: ``L``, ``n``, ``K0``, ``geometry``
    (eh, ew, C), ``neighbours``, ``nsym``, ``tables`` (int64 ``[K0*M, nsym + 1]``, cumulative) and
    ``model`` (the ``Adaptive`` it was packed under; context "channel" when K0 = C > 1)."""
    a = np.frombuffer(bytes(buf), np.uint8)
    L, n = C.c_uint32(), C.c_uint64()
    f = [C.c_uint32() for _ in range(6)]
    pa = _u8(a) if a.size else None
    rc = lib().tic_rcseg_parse_emb(pa, a.size, C.byref(L), C.byref(n), *[C.byref(v) for v in f], None)
    if rc:
        _raise(rc, "entropy.parse_emb")
    K0, eh, ew, c, nb, nsym = (int(v.value) for v in f)
    tables = np.empty((K0 * 3 ** nb, nsym + 1), np.int64)
    rc = lib().tic_rcseg_parse_emb(pa, a.size, None, None, None, None, None, None, None, None, _i64(tables))
    if rc:
        _raise(rc, "entropy.parse_emb")
    return {"L": int(L.value), "n": int(n.value), "K0": K0, "geometry": (eh, ew, c), "neighbours": nb, "nsym": nsym,
            "tables": tables, "model": Adaptive("none" if K0 == 1 else "channel", nb, nsym)}


def range_extent_emb(buf, first: int, count: int) -> tuple[int, int, int, int]:
    """``range_extent`` for a "TICA" container; ``buf`` needs to hold the header, the table block
    and the length table only."""
    if int(first) < 0 or int(count) < 0:
        raise ValueError(f"symbol range [{first}, {first} + {count}) is negative")
    a = np.frombuffer(bytes(buf), np.uint8)
    out = [C.c_size_t() for _ in range(4)]
    rc = lib().tic_rcseg_range_extent_emb(_u8(a) if a.size else None, a.size, int(first), int(count),
                                          *[C.byref(v) for v in out])
    if rc:
        _raise(rc, "entropy.range_extent_emb")
    return tuple(int(v.value) for v in out)

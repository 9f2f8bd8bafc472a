"""Segmented range-coder streams ("TICS" version 1, include/tic.h), host side.

A container cuts a symbol sequence into segments of ``L`` symbols, each an independent stream of
the range coder in csrc/range_coder.cpp (byte for byte what ``RangeEncoder`` writes for the
segment), behind a header and a table of u16 segment lengths.  Independent segments are what the
device coder (csrc/tic_entropy.cpp, ``Codec.entropy_encode_device``) runs one per lane; the
functions here are its reference and read or write a container without a GPU.

Symbols are bytes; the table is a ``range_coder`` cumulative table with at most 256 symbols and
no zero frequency.  Errors are mapped as ``range_coder._raise`` maps them.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import lib, u8p
from .range_coder import _raise, _table

MAGIC = b"TICS"
HEADER_BYTES = 20
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


def bound(n: int, segment: int = DEFAULT_SEGMENT) -> int:
    """Worst-case container size for ``n`` symbols."""
    out = C.c_size_t()
    rc = lib().tic_rcseg_bound(int(n), int(segment), C.byref(out))
    if rc:
        _raise(rc, "entropy.bound")
    return int(out.value)


def pack(symbols, cum_freq, segment: int = DEFAULT_SEGMENT) -> bytes:
    """The container of ``symbols`` (flattened in C order)."""
    table = _table(cum_freq)
    sym = _symbols(symbols)
    cap = bound(sym.size, segment)
    out = np.empty(cap, np.uint8)
    written = C.c_size_t()
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


def unpack(buf, cum_freq, n: int | None = None) -> np.ndarray:
    """The symbols of a container (uint8); ``n``, when given, must be the header's count."""
    table = _table(cum_freq)
    a = np.frombuffer(bytes(buf), np.uint8)
    if n is None:
        _, n = parse(a)
    out = np.empty(int(n), np.uint8)
    rc = lib().tic_rcseg_decode(_u8(a) if a.size else None, a.size, _i64(table), table.size, _u8(out), int(n))
    if rc:
        _raise(rc, "entropy.unpack")
    return out

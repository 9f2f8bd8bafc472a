"""CPU tests of the image-list entries (tic_images_to_patches_device,
tic_patches_to_images_device, tic_rmbe_images_device): exported and bound, argument
validation answers TIC_EINVAL before any HIP call, and ImageCodec.plan_batches groups as
documented.  No device is touched."""
import ctypes as C

import numpy as np
import pytest

EINVAL = -1
NAMES = ["tic_images_to_patches_device", "tic_patches_to_images_device", "tic_rmbe_images_device"]


@pytest.fixture(scope="module")
def L():
    from tf_image_compression_amd import _lib
    return _lib.lib()


def test_symbols_exported_and_bound(L):
    from tf_image_compression_amd import _lib
    bound = {n: (res, args) for n, res, args in _lib.SIGNATURES}
    for n in NAMES:
        assert n in bound
        assert hasattr(L, n)
        assert getattr(L, n).restype is C.c_int
    assert len(bound["tic_images_to_patches_device"][1]) == 9
    assert len(bound["tic_patches_to_images_device"][1]) == 8
    assert len(bound["tic_rmbe_images_device"][1]) == 6


def _table(offsets, sizes):
    off = np.asarray(offsets, np.int64)
    hs = np.asarray([s[0] for s in sizes], np.int32)
    ws = np.asarray([s[1] for s in sizes], np.int32)
    return off, hs, ws


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


class _Calls:
    """The three entries over one per-image table.  ``h`` and ``dev`` are never dereferenced by
    a call that fails its argument checks: a handle cannot exist without a device, so the checks
    are reached with the address of a zeroed block (read as model 0, not finalized, if it were)."""

    def __init__(self, L):
        self.L = L
        self.block = C.create_string_buffer(1 << 16)
        self.h = C.cast(self.block, C.c_void_p)
        self.dev = C.c_void_p(0x1000)  # stands for a device pointer; only compared with NULL
        self.n = C.c_int(-7)

    def tile(self, h, src, off, hs, ws, n, P, dst, nout=True):
        return self.L.tic_images_to_patches_device(
            h, src, _p(off, C.c_int64) if off is not None else None, _p(hs, C.c_int32) if hs is not None else None,
            _p(ws, C.c_int32) if ws is not None else None, n, P, dst, C.byref(self.n) if nout else None)

    def stitch(self, h, src, off, hs, ws, n, P, dst):
        return self.L.tic_patches_to_images_device(
            h, src, _p(off, C.c_int64) if off is not None else None, _p(hs, C.c_int32) if hs is not None else None,
            _p(ws, C.c_int32) if ws is not None else None, n, P, dst)

    def rmbe(self, h, img, off, hs, ws, n):
        return self.L.tic_rmbe_images_device(
            h, img, _p(off, C.c_int64) if off is not None else None, _p(hs, C.c_int32) if hs is not None else None,
            _p(ws, C.c_int32) if ws is not None else None, n)


@pytest.fixture(scope="module")
def calls(L):
    return _Calls(L)


def test_null_handle(calls):
    off, hs, ws = _table([0, 300], [(10, 10), (4, 5)])
    assert calls.tile(None, calls.dev, off, hs, ws, 2, 64, calls.dev) == EINVAL
    assert b"null handle" in calls.L.tic_last_error()
    assert calls.stitch(None, calls.dev, off, hs, ws, 2, 64, calls.dev) == EINVAL
    assert calls.rmbe(None, calls.dev, off, hs, ws, 2) == EINVAL
    # also for an empty list: nothing is done, but a handle is still required
    assert calls.tile(None, calls.dev, off, hs, ws, 0, 64, calls.dev) == EINVAL


def test_null_pointers(calls):
    off, hs, ws = _table([0, 300], [(10, 10), (4, 5)])
    h, d = calls.h, calls.dev
    assert calls.tile(h, None, off, hs, ws, 2, 64, d) == EINVAL
    assert calls.tile(h, d, off, hs, ws, 2, 64, None) == EINVAL
    assert calls.tile(h, d, off, hs, ws, 2, 64, d, nout=False) == EINVAL
    assert calls.tile(h, d, None, hs, ws, 2, 64, d) == EINVAL
    assert calls.tile(h, d, off, None, ws, 2, 64, d) == EINVAL
    assert calls.tile(h, d, off, hs, None, 2, 64, d) == EINVAL
    assert calls.stitch(h, None, off, hs, ws, 2, 64, d) == EINVAL
    assert calls.stitch(h, d, off, hs, ws, 2, 64, None) == EINVAL
    assert calls.stitch(h, d, None, hs, ws, 2, 64, d) == EINVAL
    assert calls.stitch(h, d, off, None, ws, 2, 64, d) == EINVAL
    assert calls.stitch(h, d, off, hs, None, 2, 64, d) == EINVAL
    assert calls.rmbe(h, None, off, hs, ws, 2) == EINVAL
    assert calls.rmbe(h, d, None, hs, ws, 2) == EINVAL
    assert calls.rmbe(h, d, off, None, ws, 2) == EINVAL
    assert calls.rmbe(h, d, off, hs, None, 2) == EINVAL


def test_negative_count(calls):
    off, hs, ws = _table([0], [(10, 10)])
    h, d = calls.h, calls.dev
    assert calls.tile(h, d, off, hs, ws, -1, 64, d) == EINVAL
    assert b"n_images" in calls.L.tic_last_error()
    assert calls.stitch(h, d, off, hs, ws, -1, 64, d) == EINVAL
    assert calls.rmbe(h, d, off, hs, ws, -1) == EINVAL


@pytest.mark.parametrize("sizes", [[(10, 10), (0, 5)], [(10, 10), (5, 0)], [(-3, 10), (4, 5)], [(10, -1), (4, 5)]])
def test_non_positive_sizes(calls, sizes):
    off, hs, ws = _table([0, 300], sizes)
    h, d = calls.h, calls.dev
    assert calls.tile(h, d, off, hs, ws, 2, 64, d) == EINVAL
    assert b"must be positive" in calls.L.tic_last_error()
    assert calls.stitch(h, d, off, hs, ws, 2, 64, d) == EINVAL
    assert calls.rmbe(h, d, off, hs, ws, 2) == EINVAL


def test_negative_offset_and_bad_patch_size(calls):
    h, d = calls.h, calls.dev
    off, hs, ws = _table([0, -1], [(10, 10), (4, 5)])
    assert calls.tile(h, d, off, hs, ws, 2, 64, d) == EINVAL
    assert b"negative offset" in calls.L.tic_last_error()
    assert calls.stitch(h, d, off, hs, ws, 2, 64, d) == EINVAL
    assert calls.rmbe(h, d, off, hs, ws, 2) == EINVAL
    off, hs, ws = _table([0, 300], [(10, 10), (4, 5)])
    for P in (0, -4, 2, 6, 63):  # tic_image_to_patches_device's rule: a positive multiple of 4
        assert calls.tile(h, d, off, hs, ws, 2, P, d) == EINVAL, P
    for P in (0, -64):           # tic_patches_to_image_device's rule: positive
        assert calls.stitch(h, d, off, hs, ws, 2, P, d) == EINVAL, P
    assert calls.tile(h, d, off, hs, ws, 2, 64, C.c_void_p(0x1002)) == EINVAL
    assert b"aligned" in calls.L.tic_last_error()


def test_overlapping_output_ranges(calls):
    h, d = calls.h, calls.dev
    # 10x10x3 = 300 elements at 0 and 4x5x3 = 60 at 299: one element shared; also in reversed order
    for offsets, sizes in ([0, 299], [(10, 10), (4, 5)]), ([299, 0], [(4, 5), (10, 10)]), ([5, 5], [(1, 1), (1, 1)]):
        off, hs, ws = _table(offsets, sizes)
        assert calls.stitch(h, d, off, hs, ws, 2, 64, d) == EINVAL
        assert b"overlap" in calls.L.tic_last_error()
        assert calls.rmbe(h, d, off, hs, ws, 2) == EINVAL
        assert b"overlap" in calls.L.tic_last_error()


def test_empty_list_is_a_no_op(calls):
    h, d = calls.h, calls.dev
    calls.n.value = -7
    assert calls.tile(h, None, None, None, None, 0, 64, None) == 0
    assert calls.n.value == 0
    assert calls.stitch(h, None, None, None, None, 0, 64, None) == 0
    assert calls.rmbe(h, None, None, None, None, 0) == 0


def test_python_wrappers_raise_value_error(calls):
    """Codec's wrappers turn TIC_EINVAL into ValueError (no device: the handle is the zeroed block)."""
    from tf_image_compression_amd.codec import Codec

    class Buf:
        ptr = calls.dev

    c = Codec.__new__(Codec)
    c._h = calls.h
    try:
        with pytest.raises(ValueError, match="must be positive"):
            c.images_to_patches_device(Buf, [0], [(0, 4)], 64, Buf)
        with pytest.raises(ValueError, match="overlap"):
            c.patches_to_images_device(Buf, [0, 10], [(2, 2), (2, 2)], 64, Buf)
        with pytest.raises(ValueError, match="offsets for"):
            c.rmbe_images_device(Buf, [0, 10], [(2, 2)])
    finally:
        c._h = None  # nothing to destroy


# ---------------------------------------------------------------------------- plan_batches
def _plan(*a, **k):
    from tf_image_compression_amd.image_codec import ImageCodec
    return ImageCodec.plan_batches(*a, **k)


def test_plan_empty():
    assert _plan([], 256, 4) == []


def test_plan_image_cap_keeps_order():
    sizes = [(10, 10)] * 7  # one patch each
    assert _plan(sizes, 256, 3) == [[0, 1, 2], [3, 4, 5], [6]]
    assert _plan(sizes, 256, 1) == [[i] for i in range(7)]
    assert _plan(sizes, 256, 100) == [list(range(7))]


def test_plan_patch_cap():
    # P = 64: (64,64) 1 patch, (100,130) 2x3 = 6, (65,64) 2, (128,128) 4
    sizes = [(64, 64), (100, 130), (65, 64), (128, 128), (64, 64)]
    assert _plan(sizes, 64, 10, max_patches=9) == [[0, 1, 2], [3, 4]]     # 1+6+2 = 9 fits exactly; +4 does not
    assert _plan(sizes, 64, 10, max_patches=8) == [[0, 1], [2, 3, 4]]     # 1+6 = 7, +2 = 9 > 8; 2+4+1 = 7
    assert _plan(sizes, 64, 2, max_patches=9) == [[0, 1], [2, 3], [4]]    # the image cap closes first


def test_plan_oversize_image_alone():
    sizes = [(64, 64), (640, 640), (64, 64), (64, 64)]  # 1, 100, 1, 1 patches at P = 64
    assert _plan(sizes, 64, 10, max_patches=50) == [[0], [1], [2, 3]]
    assert _plan([(640, 640)], 64, 10, max_patches=50) == [[0]]
    assert _plan([(640, 640), (640, 640)], 64, 10, max_patches=50) == [[0], [1]]


def test_plan_default_patch_cap_is_512():
    sizes = [(2048, 2048)] * 9  # 64 patches each at P = 256: eight fill 512
    assert _plan(sizes, 256, 100) == [list(range(8)), [8]]


def test_plan_rejects_bad_caps():
    with pytest.raises(ValueError):
        _plan([(1, 1)], 64, 0)
    with pytest.raises(ValueError):
        _plan([(1, 1)], 64, 1, max_patches=0)

"""Host-side codec object over libtic.so.

``Codec`` is one libtic handle: a model's weights resident on one MI355X plus the
stream its kernels run on.  It is the object behind the reference-shaped modules
``tf_image_compression_amd.model_N.model`` (``encoder`` / ``decoder``, mirroring
model_N/model.py:34 and :147) and behind ``encode.py`` / ``decode.py``.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, ptr, lib
from .topology import CH128_ID, RMBE_ID, param_shapes

F32 = np.float32


class DeviceBuffer:
    """Device allocation owned by a Codec handle (freed with the handle)."""

    def __init__(self, codec: "Codec", nbytes: int):
        self.codec = codec
        self.nbytes = int(nbytes)
        p = C.c_void_p()
        check(lib().tic_device_alloc(codec._h, self.nbytes, C.byref(p)), "tic_device_alloc")
        self.ptr = p

    def upload(self, arr: np.ndarray) -> None:
        arr = np.ascontiguousarray(arr)
        if arr.nbytes > self.nbytes:
            raise ValueError("array larger than device buffer")
        check(lib().tic_memcpy_h2d(self.codec._h, self.ptr, arr.ctypes.data, arr.nbytes), "tic_memcpy_h2d")

    def download(self, shape, dtype) -> np.ndarray:
        out = np.empty(shape, dtype)
        if out.nbytes > self.nbytes:
            raise ValueError("requested more bytes than the device buffer holds")
        check(lib().tic_memcpy_d2h(self.codec._h, out.ctypes.data, self.ptr, out.nbytes), "tic_memcpy_d2h")
        return out

    def view(self, offset: int) -> "DeviceView":
        """The same allocation from byte ``offset`` on (a pointer into it, as a C caller
        would pass one; not owned)."""
        if not 0 <= offset <= self.nbytes:
            raise ValueError(f"offset {offset} outside the {self.nbytes}-byte buffer")
        return DeviceView(self, int(offset))

    def free(self) -> None:
        if self.ptr is not None and self.codec._h is not None:
            check(lib().tic_device_free(self.codec._h, self.ptr), "tic_device_free")
        self.ptr = None


class DeviceView:
    """A byte offset into a DeviceBuffer, accepted wherever a DeviceBuffer is (``.ptr``)."""

    def __init__(self, buf: DeviceBuffer, offset: int):
        self.codec = buf.codec
        self.base = buf
        self.offset = offset
        self.nbytes = buf.nbytes - offset
        self.ptr = C.c_void_p(buf.ptr.value + offset)

    def upload(self, arr: np.ndarray) -> None:
        """``arr`` to the bytes from this view's offset on; the rest of the buffer stays as it was."""
        arr = np.ascontiguousarray(arr)
        if arr.nbytes > self.nbytes:
            raise ValueError("array larger than the rest of the device buffer")
        check(lib().tic_memcpy_h2d(self.codec._h, self.ptr, arr.ctypes.data, arr.nbytes), "tic_memcpy_h2d")

    def download(self, shape, dtype) -> np.ndarray:
        """The bytes from this view's offset on, as ``DeviceBuffer.download``."""
        out = np.empty(shape, dtype)
        if out.nbytes > self.nbytes:
            raise ValueError("requested more bytes than the rest of the device buffer holds")
        check(lib().tic_memcpy_d2h(self.codec._h, out.ctypes.data, self.ptr, out.nbytes), "tic_memcpy_d2h")
        return out


class Codec:
    """A model_N codec on one GPU.  ``params``: TF-named float32 arrays (weights.py)."""

    def __init__(self, model_id: int, params: dict, mean, std, patch_size: int | None = None,
                 quan_scale: int = 2, device: int = 0, tuning: str = "auto"):
        """``tuning``: "auto" applies the shipped tuning database (tuning.py: the fusions,
        tilings and variants bench.py measured best for this model / patch / lanes);
        "none" keeps the runtime's built-in per-model defaults."""
        self.model_id = int(model_id)
        if patch_size is None:
            patch_size = 128 if model_id in (2, 3, CH128_ID, RMBE_ID) else 256
        self.patch_size = int(patch_size)
        self.quan_scale = int(quan_scale)
        self.device = int(device)
        h = C.c_void_p()
        check(lib().tic_create(self.model_id, self.patch_size, self.quan_scale, self.device, C.byref(h)),
              "tic_create")
        self._h = h
        try:
            mean = np.ascontiguousarray(mean, F32).reshape(3)
            std = np.ascontiguousarray(std, F32).reshape(3)
            check(lib().tic_set_normalization(h, ptr(mean, C.c_float), ptr(std, C.c_float)),
                  "tic_set_normalization")
            for name in param_shapes(self.model_id):
                if name not in params:
                    raise ValueError(f"missing variable {name!r}")
            for name, arr in params.items():
                a = np.ascontiguousarray(arr, F32)
                shape = (C.c_int64 * a.ndim)(*a.shape)
                check(lib().tic_set_param(h, name.encode(), ptr(a, C.c_float), shape, a.ndim),
                      f"tic_set_param({name})")
            check(lib().tic_finalize(h), "tic_finalize")
            self.tuning_source = "runtime defaults"
            self._auto_tuning = tuning == "auto"
            if tuning == "auto":
                from . import tuning as _tuning
                self.tuning_source = _tuning.apply(self)
            elif tuning != "none":
                raise ValueError(f"tuning must be 'auto' or 'none', got {tuning!r}")
        except Exception:
            self.close()
            raise

    # ------------------------------------------------------------------ info
    @property
    def code_shape(self) -> tuple[int, int, int]:
        eh, ew, ec = C.c_int(), C.c_int(), C.c_int()
        check(lib().tic_code_shape(self._h, C.byref(eh), C.byref(ew), C.byref(ec)), "tic_code_shape")
        return eh.value, ew.value, ec.value

    def device_info(self) -> str:
        buf = C.create_string_buffer(256)
        check(lib().tic_device_info(self._h, buf, 256), "tic_device_info")
        return buf.value.decode()

    def layers(self):
        out = []
        n = check(lib().tic_num_layers(self._h), "tic_num_layers")
        for i in range(n):
            name = C.create_string_buffer(128)
            v = [C.c_int() for _ in range(6)]
            check(lib().tic_layer_info(self._h, i, name, 128, *[C.byref(x) for x in v]), "tic_layer_info")
            out.append((name.value.decode(), *[x.value for x in v]))
        return out

    # ------------------------------------------------------------------ host entry points
    def encode(self, patches: np.ndarray, return_preact: bool = False):
        """uint8 [N,P,P,3] -> uint8 symbols [N,h,w,C] (model_N.encoder + sess.run)."""
        x = np.ascontiguousarray(patches)
        if x.dtype != np.uint8:
            raise ValueError(f"patches must be uint8, got {x.dtype}")
        P = self.patch_size
        x = x.reshape(-1, P, P, 3)  # model_0/model.py:39 reshape [-1,P,P,3]
        n = x.shape[0]
        eh, ew, ec = self.code_shape
        idx = np.empty((n, eh, ew, ec), np.uint8)
        pre = np.empty((n, eh, ew, ec), F32) if return_preact else None
        check(lib().tic_encode(self._h, ptr(x, C.c_uint8), n, ptr(idx, C.c_uint8), ptr(pre, C.c_float)),
              "tic_encode")
        return (idx, pre) if return_preact else idx

    def decode(self, symbols: np.ndarray, return_float: bool = False):
        """uint8/int symbols [N,h,w,C] -> uint8 RGB [N,P,P,3] (np.around of the clipped float)."""
        eh, ew, ec = self.code_shape
        s = np.asarray(symbols)
        if s.dtype != np.uint8:
            if np.any(s < 0) or np.any(s >= self.quan_scale):
                raise ValueError("symbols out of range [0, quan_scale)")
            s = s.astype(np.uint8)
        elif s.size and int(s.max()) >= self.quan_scale:
            raise ValueError("symbols out of range [0, quan_scale)")
        s = np.ascontiguousarray(s).reshape(-1, eh, ew, ec)
        n = s.shape[0]
        P = self.patch_size
        rgb = np.empty((n, P, P, 3), np.uint8)
        f = np.empty((n, P, P, 3), F32) if return_float else None
        check(lib().tic_decode(self._h, ptr(s, C.c_uint8), n, ptr(rgb, C.c_uint8), ptr(f, C.c_float)),
              "tic_decode")
        return (rgb, f) if return_float else rgb

    def rmbe_windows(self, windows: np.ndarray) -> np.ndarray:
        """float32 [N,128,128,3] -> float32 (submit/2/rmbe/model.py:113-197)."""
        if self.model_id != RMBE_ID:
            raise ValueError("not an rmbe codec")
        x = np.ascontiguousarray(windows, F32).reshape(-1, self.patch_size, self.patch_size, 3)
        out = np.empty_like(x)
        check(lib().tic_rmbe(self._h, ptr(x, C.c_float), x.shape[0], ptr(out, C.c_float)), "tic_rmbe")
        return out

    # ------------------------------------------------------------------ device entry points
    def alloc(self, nbytes: int) -> DeviceBuffer:
        return DeviceBuffer(self, nbytes)

    def encode_device(self, d_in: DeviceBuffer, n: int, d_idx: DeviceBuffer, d_pre: DeviceBuffer | None = None):
        check(lib().tic_encode_device(self._h, d_in.ptr, n, d_idx.ptr, d_pre.ptr if d_pre else None),
              "tic_encode_device")

    def decode_device(self, d_idx: DeviceBuffer, n: int, d_rgb: DeviceBuffer | None, d_f32: DeviceBuffer | None = None):
        check(lib().tic_decode_device(self._h, d_idx.ptr, n, d_rgb.ptr if d_rgb else None,
                                      d_f32.ptr if d_f32 else None), "tic_decode_device")

    def codec_device(self, d_in: DeviceBuffer, n: int, d_idx: DeviceBuffer, d_rgb: DeviceBuffer):
        check(lib().tic_codec_device(self._h, d_in.ptr, n, d_idx.ptr, d_rgb.ptr), "tic_codec_device")

    def rmbe_device(self, d_in: DeviceBuffer, n: int, d_out: DeviceBuffer):
        check(lib().tic_rmbe_device(self._h, d_in.ptr, n, d_out.ptr), "tic_rmbe_device")

    def set_option(self, key: str, value: int) -> None:
        check(lib().tic_set_option(self._h, key.encode(), int(value)), f"tic_set_option({key})")
        if key == "streams" and getattr(self, "_auto_tuning", False):
            # the shipped entries are keyed by per-launch batch, which the lane count changes
            from . import tuning as _tuning
            self.tuning_source = _tuning.reapply_entries(self, int(value))

    def stream_ptr(self) -> C.c_void_p:
        s = C.c_void_p()
        check(lib().tic_get_stream(self._h, C.byref(s)), "tic_get_stream")
        return s

    def stream_external(self, on: bool) -> None:
        """Whether work of the caller's own may be pending on stream_ptr() (tic_stream_external)."""
        check(lib().tic_stream_external(self._h, int(bool(on))), "tic_stream_external")

    def synchronize(self) -> None:
        check(lib().tic_synchronize(self._h), "tic_synchronize")

    def profile_layers(self, d_in: DeviceBuffer, n: int, iters: int) -> np.ndarray:
        nl = check(lib().tic_num_layers(self._h), "tic_num_layers")
        ms = np.zeros(nl, F32)
        check(lib().tic_profile_layers(self._h, d_in.ptr, n, iters, ptr(ms, C.c_float)), "tic_profile_layers")
        return ms

    def mark_durations(self, cap: int = 8192) -> np.ndarray:
        """ms of every launch recorded under option "mark_layer" since the last call (all
        lanes, in-step: tic_mark_durations)."""
        ms = np.zeros(cap, F32)
        k = check(lib().tic_mark_durations(self._h, ptr(ms, C.c_float), cap), "tic_mark_durations")
        return ms[:k]

    def autotune(self, d_in: DeviceBuffer, n: int, reps: int = 5) -> None:
        check(lib().tic_autotune(self._h, d_in.ptr, n, reps), "tic_autotune")

    def autotune_step(self, d_in: DeviceBuffer, n: int, rounds: int = 1, reps: int = 5) -> None:
        """Per-layer variants chosen by the whole dual-lane step time (tic_autotune_step)."""
        check(lib().tic_autotune_step(self._h, d_in.ptr, n, rounds, reps), "tic_autotune_step")

    def layer_variants(self, n: int):
        out = []
        for i in range(len(self.layers())):
            th, ns = C.c_int(), C.c_int()
            check(lib().tic_layer_variant(self._h, i, n, C.byref(th), C.byref(ns)), "tic_layer_variant")
            out.append((th.value, ns.value))
        return out

    def layer_kernels(self, n: int):
        """Kernel instance each layer launches for batch n ('' if fused into the previous)."""
        out = []
        for i in range(len(self.layers())):
            buf = C.create_string_buffer(160)
            check(lib().tic_layer_kernel(self._h, i, n, buf, 160), "tic_layer_kernel")
            out.append(buf.value.decode())
        return out

    def codec_kernels(self, n: int):
        """Kernel instance each layer launches in codec_device for batch n: layer_kernels' except
        where option "chain_j" joins the two chain launches at the quantiser (tic_codec_kernel)."""
        out = []
        for i in range(len(self.layers())):
            buf = C.create_string_buffer(160)
            check(lib().tic_codec_kernel(self._h, i, n, buf, 160), "tic_codec_kernel")
            out.append(buf.value.decode())
        return out

    def tuning_export(self) -> str:
        """Tuned tilings / variants / fusion flags as text (tic_tuning_export)."""
        n = check(lib().tic_tuning_export(self._h, None, 0), "tic_tuning_export")
        buf = C.create_string_buffer(n + 1)
        check(lib().tic_tuning_export(self._h, buf, n + 1), "tic_tuning_export")
        return buf.value.decode()

    def tuning_import(self, text: str) -> None:
        check(lib().tic_tuning_import(self._h, text.encode()), "tic_tuning_import")

    def conv3x3_device(self, kind: int, act: int, d_in: DeviceBuffer, n: int, H: int, W: int, cin: int,
                       cout: int, kernel: np.ndarray, bias: np.ndarray, d_res: DeviceBuffer | None,
                       d_out: DeviceBuffer) -> None:
        k = np.ascontiguousarray(kernel, F32)
        b = np.ascontiguousarray(bias, F32)
        check(lib().tic_conv3x3_device(self._h, kind, act, d_in.ptr, n, H, W, cin, cout, ptr(k, C.c_float),
                                       ptr(b, C.c_float), d_res.ptr if d_res else None, d_out.ptr),
              "tic_conv3x3_device")

    # ------------------------------------------------------------------ whole images (image_ops.hip)
    def image_to_patches_device(self, d_img: DeviceBuffer, H: int, W: int, P: int, d_patches: DeviceBuffer):
        check(lib().tic_image_to_patches_device(self._h, d_img.ptr, H, W, P, d_patches.ptr),
              "tic_image_to_patches_device")

    def patches_to_image_device(self, d_patches: DeviceBuffer, H: int, W: int, P: int, d_img: DeviceBuffer):
        check(lib().tic_patches_to_image_device(self._h, d_patches.ptr, H, W, P, d_img.ptr),
              "tic_patches_to_image_device")

    def rmbe_image_device(self, d_img: DeviceBuffer, H: int, W: int):
        check(lib().tic_rmbe_image_device(self._h, d_img.ptr, H, W), "tic_rmbe_image_device")

    # lists of different-sized images in one arena (tic_image_batch.cpp): ``offsets`` in elements
    # of the arena's type, ``sizes`` a list of (H, W)
    @staticmethod
    def _image_table(offsets, sizes):
        off = np.ascontiguousarray(offsets, np.int64).reshape(-1)
        hw = np.asarray(sizes, np.int32).reshape(-1, 2)
        if off.size != hw.shape[0]:
            raise ValueError(f"{off.size} offsets for {hw.shape[0]} image sizes")
        return off, np.ascontiguousarray(hw[:, 0]), np.ascontiguousarray(hw[:, 1])

    def images_to_patches_device(self, d_images: DeviceBuffer, offsets, sizes, P: int,
                                 d_patches: DeviceBuffer) -> int:
        """uint8 images of an arena -> one patch batch (tic_images_to_patches_device).  Returns
        the number of patches."""
        off, hs, ws = self._image_table(offsets, sizes)
        n = C.c_int()
        check(lib().tic_images_to_patches_device(self._h, d_images.ptr, ptr(off, C.c_int64), ptr(hs, C.c_int32),
                                                 ptr(ws, C.c_int32), off.size, P, d_patches.ptr, C.byref(n)),
              "tic_images_to_patches_device")
        return n.value

    def patches_to_images_device(self, d_patches: DeviceBuffer, offsets, sizes, P: int, d_images: DeviceBuffer):
        off, hs, ws = self._image_table(offsets, sizes)
        check(lib().tic_patches_to_images_device(self._h, d_patches.ptr, ptr(off, C.c_int64), ptr(hs, C.c_int32),
                                                 ptr(ws, C.c_int32), off.size, P, d_images.ptr),
              "tic_patches_to_images_device")

    def rmbe_images_device(self, d_images: DeviceBuffer, offsets, sizes):
        off, hs, ws = self._image_table(offsets, sizes)
        check(lib().tic_rmbe_images_device(self._h, d_images.ptr, ptr(off, C.c_int64), ptr(hs, C.c_int32),
                                           ptr(ws, C.c_int32), off.size), "tic_rmbe_images_device")

    # a region of an image (tic_region.cpp)
    @staticmethod
    def region_plan(H: int, W: int, P: int, y: int, x: int, h: int, w: int, S: int = 0) -> tuple[int, int, int, int]:
        """``(py0, py1, px0, px1)``: the patches ``py0 <= py < py1``, ``px0 <= px < px1`` the region
        ``[y, y + h) x [x, x + w)`` of an ``H x W`` image needs; ``S``: the post-filter's window side
        (128), 0 without it (tic_region_plan; host arithmetic)."""
        vals = [int(v) for v in (H, W, P, y, x, h, w, S)]
        if any(abs(v) >= 2 ** 31 for v in vals):
            raise ValueError("region_plan: arguments must fit 32 bits")
        out = [C.c_int() for _ in range(4)]
        check(lib().tic_region_plan(*vals, *[C.byref(v) for v in out]), "tic_region_plan")
        return tuple(v.value for v in out)

    def rmbe_regions_device(self, d_arena: DeviceBuffer, offsets, sizes, origins, full_sizes):
        """The post-filter on parts of images: region i, ``sizes[i]`` at float ``offsets[i]`` of the
        arena, holds the pixels from ``origins[i] = (y0, x0)`` on of an image of ``full_sizes[i]``;
        the windows of the full image's grid that lie wholly inside it are filtered in place
        (tic_rmbe_regions_device)."""
        off, hs, ws = self._image_table(offsets, sizes)
        _, ys, xs = self._image_table(offsets, origins)
        _, fh, fw = self._image_table(offsets, full_sizes)
        i32 = C.c_int32
        check(lib().tic_rmbe_regions_device(self._h, d_arena.ptr, ptr(off, C.c_int64), ptr(hs, i32), ptr(ws, i32),
                                            ptr(ys, i32), ptr(xs, i32), ptr(fh, i32), ptr(fw, i32), off.size),
              "tic_rmbe_regions_device")

    def crop_regions_device(self, d_boxes: DeviceBuffer, offsets, sizes, origins, crop_sizes, out_offsets,
                            d_out: DeviceBuffer):
        """Crop i: ``crop_sizes[i]`` pixels from ``origins[i]`` on of the uint8 HWC box ``sizes[i]``
        at byte ``offsets[i]`` -> a dense block at byte ``out_offsets[i]`` of ``d_out``
        (tic_crop_regions_device)."""
        off, hs, ws = self._image_table(offsets, sizes)
        _, ys, xs = self._image_table(offsets, origins)
        ooff, ch, cw = self._image_table(out_offsets, crop_sizes)
        if ooff.size != off.size:
            raise ValueError(f"{ooff.size} output offsets for {off.size} boxes")
        i32 = C.c_int32
        check(lib().tic_crop_regions_device(self._h, d_boxes.ptr, ptr(off, C.c_int64), ptr(hs, i32), ptr(ws, i32),
                                            ptr(ys, i32), ptr(xs, i32), ptr(ch, i32), ptr(cw, i32),
                                            ptr(ooff, C.c_int64), off.size, d_out.ptr), "tic_crop_regions_device")

    # MS-SSIM of lists of uint8 image pairs (tic_msssim.cpp)
    @staticmethod
    def msssim_scratch_bytes(sizes) -> int:
        """Bytes of device scratch ``msssim_images_device`` needs for images of these (H, W)
        (tic_msssim_scratch_bytes: host arithmetic, no device)."""
        hw = np.asarray(sizes, np.int32).reshape(-1, 2)
        hs, ws = np.ascontiguousarray(hw[:, 0]), np.ascontiguousarray(hw[:, 1])
        if hw.shape[0] == 0:  # an empty array has no address to pass
            hs = ws = np.zeros(1, np.int32)
        n = C.c_size_t()
        check(lib().tic_msssim_scratch_bytes(ptr(hs, C.c_int32), ptr(ws, C.c_int32), hw.shape[0], C.byref(n)),
              "tic_msssim_scratch_bytes")
        return n.value

    def msssim_images_device(self, d_a: DeviceBuffer, d_b: DeviceBuffer, offsets, sizes, d_scratch: DeviceBuffer,
                             d_out: DeviceBuffer) -> None:
        """Sums of cs and l*cs per scale and channel of every image pair of two uint8 arenas
        (image i of both at byte ``offsets[i]``) into ``d_out``: float64 [n, 5, 3, 2]
        (tic_msssim_images_device; evaluate.msssim_from_sums combines them)."""
        off, hs, ws = self._image_table(offsets, sizes)
        if d_out.nbytes < off.size * 30 * 8:
            raise ValueError(f"d_out holds {d_out.nbytes} bytes, {off.size} images need {off.size * 30 * 8}")
        check(lib().tic_msssim_images_device(self._h, d_a.ptr, d_b.ptr, ptr(off, C.c_int64), ptr(hs, C.c_int32),
                                             ptr(ws, C.c_int32), off.size, d_scratch.ptr, d_scratch.nbytes,
                                             d_out.ptr), "tic_msssim_images_device")

    # segmented range-coder streams on the device (tic_entropy.cpp; entropy.py is the host side)
    @staticmethod
    def _stream_table(*cols):
        arrs = [np.ascontiguousarray(c, np.int64).reshape(-1) for c in cols]
        if len({a.size for a in arrs}) != 1:
            raise ValueError("per-stream arrays differ in length")
        if arrs[0].size == 0:  # an empty array has no address to pass
            arrs = [np.zeros(1, np.int64) for _ in arrs]
            return 0, arrs
        return arrs[0].size, arrs

    def entropy_set_table(self, cum_freq) -> None:
        """The cumulative table (``range_coder`` contract, at most 256 symbols, no zero frequency)
        of the following entropy calls on this codec (tic_entropy_set_table)."""
        from .range_coder import _table
        t = _table(cum_freq)
        check(lib().tic_entropy_set_table(self._h, ptr(t, C.c_int64), t.size), "tic_entropy_set_table")

    @staticmethod
    def entropy_scratch_bytes(counts, segment: int) -> int:
        """Bytes of device scratch either entropy entry needs for streams of these symbol counts
        (tic_entropy_scratch_bytes; for decoding, ``segment`` is the smallest L of the containers)."""
        n, (cnt,) = Codec._stream_table(counts)
        out = C.c_size_t()
        check(lib().tic_entropy_scratch_bytes(ptr(cnt, C.c_int64), n, int(segment), C.byref(out)),
              "tic_entropy_scratch_bytes")
        return out.value

    def entropy_encode_device(self, d_sym: DeviceBuffer, sym_offsets, counts, segment: int, d_scratch: DeviceBuffer,
                              d_out: DeviceBuffer, d_sizes: DeviceBuffer, scratch_bytes: int | None = None,
                              out_cap: int | None = None) -> None:
        """Stream i (``counts[i]`` uint8 symbols at byte ``sym_offsets[i]`` of ``d_sym``) -> its
        container; the containers back to back in ``d_out``, their sizes (uint64, UINT64_MAX for a
        stream with a symbol outside the table) in ``d_sizes`` (tic_entropy_encode_device)."""
        n, (off, cnt) = self._stream_table(sym_offsets, counts)
        if d_sizes.nbytes < 8 * n:
            raise ValueError(f"d_sizes holds {d_sizes.nbytes} bytes, {n} streams need {8 * n}")
        check(lib().tic_entropy_encode_device(
            self._h, d_sym.ptr, ptr(off, C.c_int64), ptr(cnt, C.c_int64), n, int(segment), d_scratch.ptr,
            d_scratch.nbytes if scratch_bytes is None else int(scratch_bytes), d_out.ptr,
            d_out.nbytes if out_cap is None else int(out_cap), d_sizes.ptr), "tic_entropy_encode_device")

    def entropy_decode_device(self, d_blob: DeviceBuffer, blob_offsets, blob_sizes, counts, d_sym: DeviceBuffer,
                              sym_offsets, d_scratch: DeviceBuffer, scratch_bytes: int | None = None) -> None:
        """Container i (``blob_sizes[i]`` bytes at ``blob_offsets[i]`` of ``d_blob``, validated by
        ``entropy.parse`` before the upload) -> its ``counts[i]`` symbols at ``sym_offsets[i]`` of
        ``d_sym`` (tic_entropy_decode_device)."""
        n, (boff, bsz, cnt, soff) = self._stream_table(blob_offsets, blob_sizes, counts, sym_offsets)
        check(lib().tic_entropy_decode_device(
            self._h, d_blob.ptr, ptr(boff, C.c_int64), ptr(bsz, C.c_int64), ptr(cnt, C.c_int64), n, d_sym.ptr,
            ptr(soff, C.c_int64), d_scratch.ptr, d_scratch.nbytes if scratch_bytes is None else int(scratch_bytes)),
            "tic_entropy_decode_device")

    # version-2 (context) streams: K tables, symbol k of a stream under table k mod K
    def entropy_set_tables(self, tables) -> None:
        """The ``[K, ncum]`` cumulative tables of the following ``*_ctx_device`` calls on this codec,
        uploaded to the device (tic_entropy_set_tables); ``entropy_set_table``'s table is untouched."""
        from .entropy import ctx_tables
        t = ctx_tables(tables)
        check(lib().tic_entropy_set_tables(self._h, ptr(t, C.c_int64), t.shape[0], t.shape[1]),
              "tic_entropy_set_tables")

    def entropy_encode_ctx_device(self, d_sym: DeviceBuffer, sym_offsets, counts, segment: int,
                                  d_scratch: DeviceBuffer, d_out: DeviceBuffer, d_sizes: DeviceBuffer,
                                  scratch_bytes: int | None = None, out_cap: int | None = None) -> None:
        """``entropy_encode_device`` writing version-2 containers under the tables set
        (tic_entropy_encode_ctx_device); every stream starts at context 0."""
        n, (off, cnt) = self._stream_table(sym_offsets, counts)
        if d_sizes.nbytes < 8 * n:
            raise ValueError(f"d_sizes holds {d_sizes.nbytes} bytes, {n} streams need {8 * n}")
        check(lib().tic_entropy_encode_ctx_device(
            self._h, d_sym.ptr, ptr(off, C.c_int64), ptr(cnt, C.c_int64), n, int(segment), d_scratch.ptr,
            d_scratch.nbytes if scratch_bytes is None else int(scratch_bytes), d_out.ptr,
            d_out.nbytes if out_cap is None else int(out_cap), d_sizes.ptr), "tic_entropy_encode_ctx_device")

    def entropy_decode_ctx_device(self, d_blob: DeviceBuffer, blob_offsets, blob_sizes, counts, d_sym: DeviceBuffer,
                                  sym_offsets, d_scratch: DeviceBuffer, scratch_bytes: int | None = None) -> None:
        """``entropy_decode_device`` for version-2 containers (validated by ``entropy.parse_ctx``
        before the upload) under the tables set (tic_entropy_decode_ctx_device)."""
        n, (boff, bsz, cnt, soff) = self._stream_table(blob_offsets, blob_sizes, counts, sym_offsets)
        check(lib().tic_entropy_decode_ctx_device(
            self._h, d_blob.ptr, ptr(boff, C.c_int64), ptr(bsz, C.c_int64), ptr(cnt, C.c_int64), n, d_sym.ptr,
            ptr(soff, C.c_int64), d_scratch.ptr, d_scratch.nbytes if scratch_bytes is None else int(scratch_bytes)),
            "tic_entropy_decode_ctx_device")

    def histogram_ctx_device(self, d_sym: DeviceBuffer, n: int, Q: int, K: int, d_counts: DeviceBuffer):
        """Accumulate the histogram of symbol ``i`` of ``d_sym[0..n)`` into row ``i mod K`` of the
        uint64 counts ``d_counts[K, Q]`` (tic_histogram_ctx_device)."""
        if d_counts.nbytes < 8 * int(K) * int(Q):
            raise ValueError(f"d_counts holds {d_counts.nbytes} bytes, [{K}, {Q}] counts need {8 * int(K) * int(Q)}")
        check(lib().tic_histogram_ctx_device(self._h, d_sym.ptr, n, Q, K, d_counts.ptr), "tic_histogram_ctx_device")

    # version-3 (causal-neighbour) streams: K0 * M tables, symbol k under row (k mod K0) * M + nb
    def entropy_set_tables_nbr(self, tables, geometry=None) -> None:
        """The ``[K0, M, ncum]`` cumulative tables (``M`` = 3: W neighbour; 9: W and N) and the code
        geometry ``(eh, ew, C)`` (default: this codec's ``code_shape``) of the following
        ``*_nbr_device`` calls (tic_entropy_set_tables_nbr).  They share the device buffer of
        ``entropy_set_tables`` and replace its tables."""
        from .entropy import nbr_tables, neighbours_of
        t = nbr_tables(tables)
        eh, ew, c = (int(v) for v in (self.code_shape if geometry is None else geometry))
        if not all(0 <= v < 2 ** 32 for v in (eh, ew, c)):
            raise ValueError(f"code geometry {eh} x {ew} x {c} must be in [1, 65535] each")
        check(lib().tic_entropy_set_tables_nbr(self._h, ptr(t, C.c_int64), t.shape[0], neighbours_of(t), t.shape[2],
                                               eh, ew, c), "tic_entropy_set_tables_nbr")
        self._nbr_rows = t.shape[0] * t.shape[1]

    def entropy_encode_nbr_device(self, d_sym: DeviceBuffer, sym_offsets, counts, segment: int,
                                  d_scratch: DeviceBuffer, d_out: DeviceBuffer, d_sizes: DeviceBuffer,
                                  scratch_bytes: int | None = None, out_cap: int | None = None) -> None:
        """``entropy_encode_device`` writing version-3 containers under the tables and geometry set
        (tic_entropy_encode_nbr_device); every stream starts at position 0 of a patch."""
        n, (off, cnt) = self._stream_table(sym_offsets, counts)
        if d_sizes.nbytes < 8 * n:
            raise ValueError(f"d_sizes holds {d_sizes.nbytes} bytes, {n} streams need {8 * n}")
        check(lib().tic_entropy_encode_nbr_device(
            self._h, d_sym.ptr, ptr(off, C.c_int64), ptr(cnt, C.c_int64), n, int(segment), d_scratch.ptr,
            d_scratch.nbytes if scratch_bytes is None else int(scratch_bytes), d_out.ptr,
            d_out.nbytes if out_cap is None else int(out_cap), d_sizes.ptr), "tic_entropy_encode_nbr_device")

    def entropy_decode_nbr_device(self, d_blob: DeviceBuffer, blob_offsets, blob_sizes, counts, d_sym: DeviceBuffer,
                                  sym_offsets, d_scratch: DeviceBuffer, scratch_bytes: int | None = None) -> None:
        """``entropy_decode_device`` for version-3 containers (validated by ``entropy.parse_nbr``
        before the upload) under the tables and geometry set (tic_entropy_decode_nbr_device)."""
        n, (boff, bsz, cnt, soff) = self._stream_table(blob_offsets, blob_sizes, counts, sym_offsets)
        check(lib().tic_entropy_decode_nbr_device(
            self._h, d_blob.ptr, ptr(boff, C.c_int64), ptr(bsz, C.c_int64), ptr(cnt, C.c_int64), n, d_sym.ptr,
            ptr(soff, C.c_int64), d_scratch.ptr, d_scratch.nbytes if scratch_bytes is None else int(scratch_bytes)),
            "tic_entropy_decode_nbr_device")

    def histogram_nbr_device(self, d_sym: DeviceBuffer, sym_offsets, counts, Q: int, segment: int,
                             d_counts: DeviceBuffer):
        """Accumulate symbol ``k`` of every stream into row ``(k mod K0) * M + nb`` of the uint64
        counts ``d_counts[K0 * M, Q]``, ``nb`` as the coder derives it at this ``segment`` from the
        geometry, ``K0`` and ``M`` last set by ``entropy_set_tables_nbr`` (tic_histogram_nbr_device)."""
        n, (off, cnt) = self._stream_table(sym_offsets, counts)
        rows = getattr(self, "_nbr_rows", 0)
        if rows and d_counts.nbytes < 8 * rows * int(Q):
            raise ValueError(f"d_counts holds {d_counts.nbytes} bytes, [{rows}, {Q}] counts need {8 * rows * int(Q)}")
        check(lib().tic_histogram_nbr_device(self._h, d_sym.ptr, ptr(off, C.c_int64), ptr(cnt, C.c_int64), n, int(Q),
                                             int(segment), d_counts.ptr), "tic_histogram_nbr_device")

    # symbol ranges of containers of any version (entropy.unpack_range is the host side)
    @staticmethod
    def entropy_ranges_scratch_bytes(firsts, counts, segment: int) -> int:
        """Bytes of device scratch ``entropy_decode_ranges_device`` needs for these symbol ranges
        (tic_entropy_ranges_scratch_bytes; ``segment`` is the smallest L of the containers)."""
        n, (fst, cnt) = Codec._stream_table(firsts, counts)
        out = C.c_size_t()
        check(lib().tic_entropy_ranges_scratch_bytes(ptr(fst, C.c_int64), ptr(cnt, C.c_int64), n, int(segment),
                                                     C.byref(out)), "tic_entropy_ranges_scratch_bytes")
        return out.value

    def entropy_decode_ranges_device(self, d_blob: DeviceBuffer, blob_offsets, blob_sizes, stream_counts, firsts,
                                     counts, d_sym: DeviceBuffer, sym_offsets, d_scratch: DeviceBuffer,
                                     scratch_bytes: int | None = None, version: int = 1) -> None:
        """Range r: symbols ``[firsts[r], firsts[r] + counts[r])`` of the container at
        ``blob_offsets[r]`` (``blob_sizes[r]`` bytes, ``stream_counts[r]`` symbols; several ranges
        may name one container) -> ``counts[r]`` symbols at ``sym_offsets[r]`` of ``d_sym``.  Only
        the header, the length table and the payloads of the range's segments are read, so the rest
        of the container need not be on the device.  ``version`` 1, 2 or 3 selects
        tic_entropy_decode_ranges_device, ``_ctx_device`` or ``_nbr_device`` (under the table or
        tables set on this codec)."""
        name = {1: "tic_entropy_decode_ranges_device", 2: "tic_entropy_decode_ranges_ctx_device",
                3: "tic_entropy_decode_ranges_nbr_device"}.get(int(version))
        if name is None:
            raise ValueError(f"container version {version} is not 1, 2 or 3")
        n, (boff, bsz, scnt, fst, cnt, soff) = self._stream_table(blob_offsets, blob_sizes, stream_counts, firsts,
                                                                  counts, sym_offsets)
        check(getattr(lib(), name)(
            self._h, d_blob.ptr, ptr(boff, C.c_int64), ptr(bsz, C.c_int64), ptr(scnt, C.c_int64), ptr(fst, C.c_int64),
            ptr(cnt, C.c_int64), n, d_sym.ptr, ptr(soff, C.c_int64), d_scratch.ptr,
            d_scratch.nbytes if scratch_bytes is None else int(scratch_bytes)), name)

    # "TICA" streams: tables fitted to each stream and carried in its container (tic_entropy_emb.cpp).
    # ``model`` is an ``entropy.Adaptive`` (not ``auto``); ``geometry`` defaults to ``code_shape``.
    def _emb_model(self, model, geometry=None):
        if getattr(model, "automatic", False):
            raise ValueError("the device entries take one model per call: resolve Adaptive.auto() with choose_model")
        eh, ew, c = (int(v) for v in (self.code_shape if geometry is None else geometry))
        if not all(1 <= v <= 65535 for v in (eh, ew, c)):
            raise ValueError(f"code geometry {eh} x {ew} x {c} must be in [1, 65535] each")
        return model.K0(c), int(model.neighbours), int(model.nsym), eh, ew, c

    def histogram_streams_nbr_device(self, d_sym: DeviceBuffer, sym_offsets, counts, model, segment: int,
                                     d_counts: DeviceBuffer, geometry=None):
        """Accumulate symbol ``k`` of stream ``i`` into row ``(k mod K0) * M + nb`` of the uint64
        counts ``d_counts[n_streams, K0 * M, nsym]`` under ``model``'s rows at this ``segment``
        (tic_histogram_streams_nbr_device)."""
        n, (off, cnt) = self._stream_table(sym_offsets, counts)
        K0, nb, nsym, eh, ew, c = self._emb_model(model, geometry)
        need = 8 * n * K0 * 3 ** nb * nsym
        if d_counts.nbytes < need:
            raise ValueError(f"d_counts holds {d_counts.nbytes} bytes, the counts of {n} streams need {need}")
        check(lib().tic_histogram_streams_nbr_device(self._h, d_sym.ptr, ptr(off, C.c_int64), ptr(cnt, C.c_int64), n,
                                                     nsym, int(segment), K0, nb, eh, ew, c, d_counts.ptr),
              "tic_histogram_streams_nbr_device")

    @staticmethod
    def entropy_emb_scratch_bytes(counts, segment: int, model, channels: int) -> int:
        """Bytes of device scratch ``entropy_encode_emb_device`` / ``entropy_decode_emb_device`` need
        (tic_entropy_emb_scratch_bytes); ``channels``: the code's C, which gives ``model`` its K0."""
        n, (cnt,) = Codec._stream_table(counts)
        out = C.c_size_t()
        check(lib().tic_entropy_emb_scratch_bytes(ptr(cnt, C.c_int64), n, int(segment), model.widest().K0(channels),
                                                  int(model.widest().neighbours), int(model.nsym), C.byref(out)),
              "tic_entropy_emb_scratch_bytes")
        return out.value

    def entropy_encode_emb_device(self, d_sym: DeviceBuffer, sym_offsets, counts, segment: int, model,
                                  d_scratch: DeviceBuffer, d_out: DeviceBuffer, d_sizes: DeviceBuffer,
                                  scratch_bytes: int | None = None, out_cap: int | None = None,
                                  geometry=None) -> None:
        """``entropy_encode_device`` writing "TICA" containers under ``model``: the tables are
        fitted to every stream on the device and written into its container
        (tic_entropy_encode_emb_device; ``entropy.pack`` with an ``Adaptive`` is the host side)."""
        n, (off, cnt) = self._stream_table(sym_offsets, counts)
        if d_sizes.nbytes < 8 * n:
            raise ValueError(f"d_sizes holds {d_sizes.nbytes} bytes, {n} streams need {8 * n}")
        check(lib().tic_entropy_encode_emb_device(
            self._h, d_sym.ptr, ptr(off, C.c_int64), ptr(cnt, C.c_int64), n, int(segment),
            *self._emb_model(model, geometry), d_scratch.ptr,
            d_scratch.nbytes if scratch_bytes is None else int(scratch_bytes), d_out.ptr,
            d_out.nbytes if out_cap is None else int(out_cap), d_sizes.ptr), "tic_entropy_encode_emb_device")

    def entropy_decode_emb_device(self, d_blob: DeviceBuffer, blob_offsets, blob_sizes, counts, model,
                                  d_sym: DeviceBuffer, sym_offsets, d_scratch: DeviceBuffer,
                                  scratch_bytes: int | None = None, geometry=None) -> None:
        """``entropy_decode_device`` for "TICA" containers of one ``model`` (what their headers say:
        ``entropy.parse_emb``); no table is needed (tic_entropy_decode_emb_device)."""
        n, (boff, bsz, cnt, soff) = self._stream_table(blob_offsets, blob_sizes, counts, sym_offsets)
        check(lib().tic_entropy_decode_emb_device(
            self._h, d_blob.ptr, ptr(boff, C.c_int64), ptr(bsz, C.c_int64), ptr(cnt, C.c_int64), n,
            *self._emb_model(model, geometry), d_sym.ptr, ptr(soff, C.c_int64), d_scratch.ptr,
            d_scratch.nbytes if scratch_bytes is None else int(scratch_bytes)), "tic_entropy_decode_emb_device")

    @staticmethod
    def entropy_ranges_emb_scratch_bytes(firsts, counts, segment: int, model, channels: int) -> int:
        """Bytes of device scratch ``entropy_decode_ranges_emb_device`` needs
        (tic_entropy_ranges_emb_scratch_bytes)."""
        n, (fst, cnt) = Codec._stream_table(firsts, counts)
        out = C.c_size_t()
        check(lib().tic_entropy_ranges_emb_scratch_bytes(ptr(fst, C.c_int64), ptr(cnt, C.c_int64), n, int(segment),
                                                         model.K0(channels), int(model.neighbours), int(model.nsym),
                                                         C.byref(out)), "tic_entropy_ranges_emb_scratch_bytes")
        return out.value

    def entropy_decode_ranges_emb_device(self, d_blob: DeviceBuffer, blob_offsets, blob_sizes, stream_counts, firsts,
                                         counts, model, d_sym: DeviceBuffer, sym_offsets, d_scratch: DeviceBuffer,
                                         scratch_bytes: int | None = None, geometry=None) -> None:
        """``entropy_decode_ranges_device`` for "TICA" containers of one ``model``: only the header,
        the table block, the length table and the payloads of a range's segments are read
        (tic_entropy_decode_ranges_emb_device)."""
        n, (boff, bsz, scnt, fst, cnt, soff) = self._stream_table(blob_offsets, blob_sizes, stream_counts, firsts,
                                                                  counts, sym_offsets)
        check(lib().tic_entropy_decode_ranges_emb_device(
            self._h, d_blob.ptr, ptr(boff, C.c_int64), ptr(bsz, C.c_int64), ptr(scnt, C.c_int64), ptr(fst, C.c_int64),
            ptr(cnt, C.c_int64), n, *self._emb_model(model, geometry), d_sym.ptr, ptr(soff, C.c_int64), d_scratch.ptr,
            d_scratch.nbytes if scratch_bytes is None else int(scratch_bytes)),
            "tic_entropy_decode_ranges_emb_device")

    def round_u8_device(self, d_in: DeviceBuffer, n: int, d_out: DeviceBuffer):
        check(lib().tic_round_u8_device(self._h, d_in.ptr, n, d_out.ptr), "tic_round_u8_device")

    def histogram_device(self, d_sym: DeviceBuffer, n: int, Q: int, d_counts: DeviceBuffer):
        check(lib().tic_histogram_device(self._h, d_sym.ptr, n, Q, d_counts.ptr), "tic_histogram_device")

    def sse_u8_device(self, d_a: DeviceBuffer, d_b: DeviceBuffer, n: int, d_acc: DeviceBuffer):
        check(lib().tic_sse_u8_device(self._h, d_a.ptr, d_b.ptr, n, d_acc.ptr), "tic_sse_u8_device")

    def memset_device(self, d: DeviceBuffer, value: int, nbytes: int):
        check(lib().tic_memset_device(self._h, d.ptr, value, nbytes), "tic_memset_device")

    def wait_for(self, other: "Codec") -> None:
        """Order this handle's stream after everything enqueued so far on ``other``'s."""
        check(lib().tic_stream_wait(self._h, other._h), "tic_stream_wait")

    def record(self, slot: int) -> None:
        """Mark the work enqueued so far on this handle's stream as event ``slot`` (0..7)."""
        check(lib().tic_event_record(self._h, slot), "tic_event_record")

    def wait_event(self, other: "Codec", slot: int) -> None:
        """Order this handle's stream after ``other``'s last mark of ``slot`` (if any)."""
        check(lib().tic_stream_wait_event(self._h, other._h, slot), "tic_stream_wait_event")

    # ------------------------------------------------------------------ lifetime
    def close(self) -> None:
        if getattr(self, "_h", None) is not None:
            lib().tic_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def version() -> str:
    return lib().tic_version().decode()


__all__ = ["Codec", "DeviceBuffer", "DeviceView", "version", "_lib"]

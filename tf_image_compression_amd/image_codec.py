"""Whole-image encode / decode on one GPU (BASELINE config 5), device-resident end to end.

The reference does the image plumbing on the host between ``sess.run`` calls:
``utils.crop_image_input_patches`` (utils/utils.py:96-133) before the encoder,
``utils.concat_patches`` (:136-167) after the decoder, then for CLIC submission 2 the
block-effect post-filter ``rmbe.rmbe`` (submit/2/rmbe/rmbe.py:15-111) and
``np.around(...).astype(np.uint8)`` (submit/2/decoder.py:176; decode.py:249).  Here every
one of those steps is a kernel on the codec's stream (image_ops.hip), the rmbe network
runs on its own handle, and the two streams are chained with events instead of a host
synchronisation.  Host memory is touched only to upload the uint8 image / symbols and
download the result.

Pipelining (BASELINE configs[4]): the stitched float image that the post-filter works on
in place alternates between two buffers, and the codec stream waits only for the rmbe
pass that last used the buffer it is about to overwrite (image i-2, a named event), not
for everything the rmbe stream has queued.  So the codec of image i+1 runs while the rmbe
passes of image i do — two streams, two networks, one GPU.  Callers that reuse their own
output buffer for consecutive images are ordered by the same rule (see decode_image_device).

Lists of images (opt-in; ``encode.py`` / ``decode.py --batch-images N``): the reference takes
images strictly one after another (encode.py:152, "To be paralleled").  ``encode_images`` /
``decode_images`` and their ``*_device`` forms put the patches of a whole group of
different-sized images into ONE patch batch — one tiling launch, one encoder / decoder call,
one stitch launch, one window batch per rmbe pass (tic_image_batch.cpp) — with the same two
stitch buffers and the same events as above between groups.  ``plan_batches`` forms the groups.
"""
from __future__ import annotations

import numpy as np

from .codec import Codec, DeviceBuffer


class ImageCodec:
    """``codec``: a model_N Codec; ``post``: optional rmbe Codec (TIC_MODEL_RMBE)."""

    NSLOT = 2  # stitch buffers in flight (codec of image i+1 beside rmbe of image i)

    def __init__(self, codec: Codec, post: Codec | None = None):
        self.codec = codec
        self.post = post
        self._bufs: dict[str, DeviceBuffer] = {}
        self._slot = 0
        self.last_slot = 0  # event slot of the last post-filtered image (decode_image_device)

    # ------------------------------------------------------------------ geometry
    def grid(self, H: int, W: int) -> tuple[int, int]:
        """Patches per column / row (utils/utils.py:100-113: pad up to a multiple of P)."""
        P = self.codec.patch_size
        return -(-H // P), -(-W // P)

    def num_patches(self, H: int, W: int) -> int:
        hn, wn = self.grid(H, W)
        return hn * wn

    def _buf(self, key: str, nbytes: int, owner: Codec | None = None) -> DeviceBuffer:
        b = self._bufs.get(key)
        if b is None or b.nbytes < nbytes:
            if b is not None:
                b.free()
            b = (owner or self.codec).alloc(max(int(nbytes), 16))
            self._bufs[key] = b
        return b

    # ------------------------------------------------------------------ device pipeline
    def encode_image_device(self, d_img: DeviceBuffer, H: int, W: int, d_sym: DeviceBuffer) -> int:
        """uint8 HWC image (device) -> symbols [n, eh, ew, ec] (device).  Returns n."""
        P = self.codec.patch_size
        n = self.num_patches(H, W)
        d_pat = self._buf("patches_u8", n * P * P * 3)
        self.codec.image_to_patches_device(d_img, H, W, P, d_pat)
        self.codec.encode_device(d_pat, n, d_sym)
        return n

    def decode_image_device(self, d_sym: DeviceBuffer, H: int, W: int, d_out: DeviceBuffer,
                            post_filter: bool = True) -> None:
        """symbols (device) -> uint8 HWC image [H, W, 3] (device).

        Readiness of ``d_out``: with the post-filter it is written on the rmbe handle's
        stream (so the next image's codec work is not held behind this image's filter);
        it is complete after ``synchronize()``, or for stream-ordered consumers after
        ``consumer.wait_event(self.post, slot)`` with the slot this call recorded
        (``last_slot``).  Without the post-filter it is written on the codec's stream."""
        P = self.codec.patch_size
        n = self.num_patches(H, W)
        d_f = self._buf("patches_f32", n * P * P * 3 * 4)
        if post_filter and self.post is not None:
            k = self._slot
            self._slot = (k + 1) % self.NSLOT
            self.last_slot = k
            d_img = self._buf(f"image_f32_{k}", H * W * 3 * 4)
            self.codec.decode_device(d_sym, n, None, d_f)
            # the rmbe pass that last filtered this stitch buffer (and wrote the previous
            # output from it) must be done before the codec overwrites it
            self.codec.wait_event(self.post, k)
            self.codec.patches_to_image_device(d_f, H, W, P, d_img)
            self.codec.record(k)
            self.post.wait_event(self.codec, k)
            self.post.rmbe_image_device(d_img, H, W)
            self.post.round_u8_device(d_img, H * W * 3, d_out)
            self.post.record(k)
        else:
            # no post-filter: everything on the codec stream, ordered after any pending
            # post-filter work that still reads a stitch buffer
            d_img = self._buf("image_f32_0", H * W * 3 * 4)
            if self.post is not None:
                self.codec.wait_event(self.post, 0)
            self.codec.decode_device(d_sym, n, None, d_f)
            self.codec.patches_to_image_device(d_f, H, W, P, d_img)
            self.codec.round_u8_device(d_img, H * W * 3, d_out)
            if self.post is not None:
                self.codec.record(0)
                self.post.wait_event(self.codec, 0)  # a later filtered image reuses slot 0

    def roundtrip_device(self, d_img: DeviceBuffer, H: int, W: int, d_sym: DeviceBuffer, d_out: DeviceBuffer,
                         post_filter: bool = True) -> None:
        self.encode_image_device(d_img, H, W, d_sym)
        self.decode_image_device(d_sym, H, W, d_out, post_filter)

    def synchronize(self) -> None:
        self.codec.synchronize()
        if self.post is not None:
            self.post.synchronize()

    # ------------------------------------------------------------------ host entry points
    def encode_image(self, image: np.ndarray) -> np.ndarray:
        """uint8 [H, W, 3] -> uint8 symbols [n, eh, ew, ec] (encode.py:154-182)."""
        img = np.ascontiguousarray(image)
        if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
            raise ValueError(f"image must be uint8 [H, W, 3], got {img.dtype} {img.shape}")
        H, W, _ = img.shape
        eh, ew, ec = self.codec.code_shape
        n = self.num_patches(H, W)
        d_img = self._buf("image_u8", img.nbytes)
        d_img.upload(img)
        d_sym = self._buf("symbols", n * eh * ew * ec)
        self.encode_image_device(d_img, H, W, d_sym)
        return d_sym.download((n, eh, ew, ec), np.uint8)

    def decode_image(self, symbols: np.ndarray, H: int, W: int, post_filter: bool = True) -> np.ndarray:
        """uint8 symbols [n, eh, ew, ec] -> uint8 [H, W, 3] (decode.py:204-249,
        submit/2/decoder.py:150-176 with the post-filter)."""
        eh, ew, ec = self.codec.code_shape
        n = self.num_patches(H, W)
        s = np.ascontiguousarray(symbols, np.uint8).reshape(-1, eh, ew, ec)
        if s.shape[0] != n:
            raise ValueError(f"{s.shape[0]} patches of symbols for a {H}x{W} image (expected {n})")
        if s.size and int(s.max()) >= self.codec.quan_scale:
            raise ValueError("symbols out of range [0, quan_scale)")
        d_sym = self._buf("symbols", s.nbytes)
        d_sym.upload(s)
        d_out = self._buf("image_out", H * W * 3)
        self.decode_image_device(d_sym, H, W, d_out, post_filter)
        self.synchronize()
        return d_out.download((H, W, 3), np.uint8)

    # ------------------------------------------------------------------ lists of images
    # Several images of different sizes as ONE patch batch (tic_image_batch.cpp): an image of
    # 384-2048 px is 4-64 patches at P = 256, so one image per launch sequence runs the conv
    # kernels far below the batch they are tuned at.  The images of a group lie in one device
    # arena, image i at ``offsets[i]`` — bytes of the uint8 arenas, floats of the float32
    # stitch arena, the same list for both.
    @staticmethod
    def plan_batches(sizes, P: int, max_images: int, max_patches: int = 512) -> list[list[int]]:
        """Consecutive groups of image indices, in list order: a group closes when the next
        image would take it past ``max_images`` images or ``max_patches`` patches; an image
        that alone exceeds ``max_patches`` forms its own group.  (512 patches of 256x256x3
        float32 are a 403 MB patch buffer.)  Pure host arithmetic, no device."""
        if max_images < 1 or max_patches < 1:
            raise ValueError("max_images and max_patches must be positive")
        groups: list[list[int]] = []
        cur: list[int] = []
        used = 0
        for i, (H, W) in enumerate(sizes):
            n = -(-int(H) // P) * -(-int(W) // P)
            if cur and (len(cur) >= max_images or used + n > max_patches):
                groups.append(cur)
                cur, used = [], 0
            cur.append(i)
            used += n
        if cur:
            groups.append(cur)
        return groups

    @staticmethod
    def packed_offsets(sizes) -> tuple[list[int], int]:
        """Offsets of images laid back to back, and the arena's length (elements)."""
        offs, end = [], 0
        for H, W in sizes:
            offs.append(end)
            end += int(H) * int(W) * 3
        return offs, end

    def _num_patches_list(self, sizes) -> int:
        return sum(self.num_patches(int(H), int(W)) for H, W in sizes)

    @staticmethod
    def _runs(offsets, sizes):
        """The images' element ranges merged into maximal contiguous runs [(start, length)]."""
        spans = sorted((int(o), int(o) + int(H) * int(W) * 3) for o, (H, W) in zip(offsets, sizes))
        runs: list[list[int]] = []
        for lo, hi in spans:
            if runs and lo == runs[-1][1]:
                runs[-1][1] = hi
            else:
                runs.append([lo, hi])
        return [(lo, hi - lo) for lo, hi in runs]

    def encode_images_device(self, d_images: DeviceBuffer, offsets, sizes, d_sym: DeviceBuffer) -> int:
        """uint8 HWC images of one arena (device) -> symbols [n, eh, ew, ec] (device), the
        patches of image i behind those of image i-1.  Returns n."""
        P = self.codec.patch_size
        n = self._num_patches_list(sizes)
        if n == 0:
            return 0
        d_pat = self._buf("patches_u8", n * P * P * 3)
        got = self.codec.images_to_patches_device(d_images, offsets, sizes, P, d_pat)
        assert got == n, (got, n)
        self.codec.encode_device(d_pat, n, d_sym)
        return n

    def decode_images_device(self, d_sym: DeviceBuffer, offsets, sizes, d_out: DeviceBuffer,
                             post_filter: bool = True) -> None:
        """symbols of a group (device) -> uint8 HWC images in the arena ``d_out`` (device),
        image i at byte ``offsets[i]``; bytes of ``d_out`` that belong to no image are not
        written.  One decoder call, one stitch launch and (with the post-filter) one gather /
        network run / write-back per rmbe pass for the whole group.  Readiness of ``d_out``
        and the hand-off between the codec's and the post-filter's stream are those of
        ``decode_image_device``: the stitch arena alternates between the same two buffers, the
        codec overwrites one only after the rmbe pass that last read it, and nothing here
        synchronises with the host, so groups can be enqueued back to back."""
        P = self.codec.patch_size
        n = self._num_patches_list(sizes)
        if n == 0:
            return
        extent = max(int(o) + int(H) * int(W) * 3 for o, (H, W) in zip(offsets, sizes))
        runs = self._runs(offsets, sizes)
        d_f = self._buf("patches_f32", n * P * P * 3 * 4)
        if post_filter and self.post is not None:
            k = self._slot
            self._slot = (k + 1) % self.NSLOT
            self.last_slot = k
            d_img = self._buf(f"image_f32_{k}", extent * 4)
            self.codec.decode_device(d_sym, n, None, d_f)
            self.codec.wait_event(self.post, k)
            self.codec.patches_to_images_device(d_f, offsets, sizes, P, d_img)
            self.codec.record(k)
            self.post.wait_event(self.codec, k)
            self.post.rmbe_images_device(d_img, offsets, sizes)
            for lo, ln in runs:
                self.post.round_u8_device(d_img.view(lo * 4), ln, d_out.view(lo))
            self.post.record(k)
        else:
            d_img = self._buf("image_f32_0", extent * 4)
            if self.post is not None:
                self.codec.wait_event(self.post, 0)
            self.codec.decode_device(d_sym, n, None, d_f)
            self.codec.patches_to_images_device(d_f, offsets, sizes, P, d_img)
            for lo, ln in runs:
                self.codec.round_u8_device(d_img.view(lo * 4), ln, d_out.view(lo))
            if self.post is not None:
                self.codec.record(0)
                self.post.wait_event(self.codec, 0)

    def encode_images(self, images) -> list[np.ndarray]:
        """[uint8 [H_i, W_i, 3]] -> [uint8 symbols [n_i, eh, ew, ec]]: ``encode_image`` of every
        image, as one upload, one patch batch and one download."""
        imgs = [np.ascontiguousarray(im) for im in images]
        for im in imgs:
            if im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] != 3 or im.size == 0:
                raise ValueError(f"image must be uint8 [H, W, 3], got {im.dtype} {im.shape}")
        if not imgs:
            return []
        sizes = [im.shape[:2] for im in imgs]
        offsets, total = self.packed_offsets(sizes)
        eh, ew, ec = self.codec.code_shape
        counts = [self.num_patches(H, W) for H, W in sizes]
        n = sum(counts)
        d_img = self._buf("image_u8", total)
        d_img.upload(np.concatenate([im.reshape(-1) for im in imgs]))
        d_sym = self._buf("symbols", n * eh * ew * ec)
        self.encode_images_device(d_img, offsets, sizes, d_sym)
        sym = d_sym.download((n, eh, ew, ec), np.uint8)
        cuts = np.cumsum(counts)[:-1]
        return [np.ascontiguousarray(s) for s in np.split(sym, cuts)]

    def decode_images(self, symbols_list, sizes, post_filter: bool = True) -> list[np.ndarray]:
        """[uint8 symbols [n_i, eh, ew, ec]], [(H_i, W_i)] -> [uint8 [H_i, W_i, 3]]:
        ``decode_image`` of every image, as one upload, one patch batch and one download."""
        eh, ew, ec = self.codec.code_shape
        sizes = [(int(H), int(W)) for H, W in sizes]
        if len(symbols_list) != len(sizes):
            raise ValueError(f"{len(symbols_list)} symbol arrays for {len(sizes)} image sizes")
        if not sizes:
            return []
        parts = []
        for s, (H, W) in zip(symbols_list, sizes):
            if H <= 0 or W <= 0:
                raise ValueError(f"image size {H}x{W} must be positive")
            s = np.ascontiguousarray(s, np.uint8).reshape(-1, eh, ew, ec)
            if s.shape[0] != self.num_patches(H, W):
                raise ValueError(f"{s.shape[0]} patches of symbols for a {H}x{W} image "
                                 f"(expected {self.num_patches(H, W)})")
            if s.size and int(s.max()) >= self.codec.quan_scale:
                raise ValueError("symbols out of range [0, quan_scale)")
            parts.append(s)
        sym = np.concatenate(parts)
        offsets, total = self.packed_offsets(sizes)
        d_sym = self._buf("symbols", sym.nbytes)
        d_sym.upload(sym)
        d_out = self._buf("image_out", total)
        self.decode_images_device(d_sym, offsets, sizes, d_out, post_filter)
        self.synchronize()
        flat = d_out.download((total,), np.uint8)
        return [flat[o:o + H * W * 3].reshape(H, W, 3).copy() for o, (H, W) in zip(offsets, sizes)]

    # ------------------------------------------------------------------ segmented streams
    # The entropy coder on the device (tic_entropy.cpp): the symbols of a group never visit the
    # host, every image becomes one "TICS" container (entropy.py), all of them in one coder call.
    def _entropy_encode(self, d_sym: DeviceBuffer, counts, cum_freq, segment: int):
        """Symbols of consecutive streams in ``d_sym`` -> (d_blob, d_sizes), nothing downloaded.
        A 2-D ``cum_freq`` ([K, ncum], entropy.py) takes the context coder: version-2 containers; a
        3-D one ([K0, M, ncum]) the neighbour coder under the codec's code shape: version 3."""
        from . import entropy
        c = self.codec
        ctx, nbr = entropy.is_ctx_table(cum_freq), entropy.is_nbr_table(cum_freq)
        if nbr:
            c.entropy_set_tables_nbr(cum_freq)
        elif ctx:
            c.entropy_set_tables(cum_freq)
        else:
            c.entropy_set_table(cum_freq)
        offs = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)
        d_scr = self._buf("entropy_scratch", c.entropy_scratch_bytes(counts, segment))
        d_blob = self._buf("entropy_blob", sum(entropy.bound(n, segment, cum_freq) for n in counts))
        d_sizes = self._buf("entropy_sizes", 8 * len(counts))
        encode = c.entropy_encode_nbr_device if nbr else c.entropy_encode_ctx_device if ctx else c.entropy_encode_device
        encode(d_sym, offs, counts, segment, d_scr, d_blob, d_sizes)
        return d_blob, d_sizes

    def _emb_models(self, d_sym: DeviceBuffer, offs, counts, model, segment: int):
        """The ``entropy.Adaptive`` of every stream, with the codec's symbol count: ``model`` itself
        or, under ``Adaptive.auto()``, ``entropy.choose_model`` on the stream's counts under
        (channel, 2): one per-stream histogram on the device and one download of 9 * C * nsym
        uint64 per stream."""
        import dataclasses
        from . import entropy
        c = self.codec
        model = dataclasses.replace(model, nsym=int(c.quan_scale))
        if not model.automatic:
            return [model] * len(counts)
        ch = int(c.code_shape[2])
        shape = (len(counts), 9 * ch, model.nsym)
        nbytes = 8 * int(np.prod(shape))
        d_cnt = self._buf("entropy_emb_counts", nbytes)
        c.memset_device(d_cnt, 0, nbytes)
        c.histogram_streams_nbr_device(d_sym, offs, counts, model.widest(), segment, d_cnt)
        full = d_cnt.download(shape, np.uint64)
        return [entropy.choose_model(full[i], counts[i], ch) for i in range(len(counts))]

    def _entropy_encode_emb(self, d_sym: DeviceBuffer, counts, model, segment: int):
        """``_entropy_encode`` under an ``entropy.Adaptive``: "TICA" containers, the streams grouped
        by their model, one coder call per group.  ``(d_blob, d_sizes, order, bases)``: the sizes
        and the containers lie in the order ``order`` of stream indices, group after group, the
        containers of a group back to back from byte ``bases[g]`` of ``d_blob``; ``bases`` is
        ``[(first position in order, byte offset)]``."""
        from . import entropy
        c = self.codec
        geo = tuple(int(v) for v in c.code_shape)
        offs = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)
        models = self._emb_models(d_sym, offs, counts, model, segment)
        groups: dict = {}
        for i, m in enumerate(models):
            groups.setdefault(m, []).append(i)
        caps = {m: sum(entropy.bound(counts[i], segment, m, geo) for i in idx) for m, idx in groups.items()}
        need = max(c.entropy_emb_scratch_bytes([counts[i] for i in idx], segment, m, geo[2]) for m, idx in groups.items())
        d_scr = self._buf("entropy_scratch", need)
        d_blob = self._buf("entropy_blob", sum(-(-v // 16) * 16 for v in caps.values()))
        d_sizes = self._buf("entropy_sizes", 8 * len(counts))
        order, bases, at = [], [], 0
        for m, idx in groups.items():
            c.entropy_encode_emb_device(d_sym, offs[idx], [counts[i] for i in idx], segment, m, d_scr, d_blob.view(at),
                                        d_sizes.view(8 * len(order)), out_cap=caps[m])
            bases.append((len(order), at))
            order += idx
            at += -(-caps[m] // 16) * 16
        self.last_models = models
        return d_blob, d_sizes, order, bases

    def encode_images_to_streams(self, images, cum_freq, segment: int = 2048) -> list[bytes]:
        """[uint8 [H_i, W_i, 3]] -> one segmented-stream container per image (entropy.unpack gives
        ``encode_images``' symbols back): one upload, ``encode_images_device``, one coder call over
        all images, one download of the sizes and one of the containers.  A 2-D ``cum_freq``
        ([K, ncum]) codes symbol k of an image under row k mod K and writes version-2 containers; a
        3-D one ([K0, M, ncum]) also conditions on the causal neighbours' classes (version 3, the
        geometry being this codec's code shape).  An ``entropy.Adaptive`` in place of the table
        writes "TICA" containers: the tables are fitted to every image's own symbols on the device
        and travel inside its container (``Adaptive.auto()`` chooses the model per image;
        ``last_models`` holds the choices)."""
        from . import entropy
        imgs = [np.ascontiguousarray(im) for im in images]
        for im in imgs:
            if im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] != 3 or im.size == 0:
                raise ValueError(f"image must be uint8 [H, W, 3], got {im.dtype} {im.shape}")
        if not imgs:
            return []
        sizes = [im.shape[:2] for im in imgs]
        offsets, total = self.packed_offsets(sizes)
        code = int(np.prod(self.codec.code_shape))
        counts = [self.num_patches(H, W) * code for H, W in sizes]
        d_img = self._buf("image_u8", total)
        d_img.upload(np.concatenate([im.reshape(-1) for im in imgs]))
        d_sym = self._buf("symbols", sum(counts))
        self.encode_images_device(d_img, offsets, sizes, d_sym)
        if isinstance(cum_freq, entropy.Adaptive):
            d_blob, d_sizes, order, bases = self._entropy_encode_emb(d_sym, counts, cum_freq, segment)
            nbytes = d_sizes.download((len(imgs),), np.uint64)
            bad = np.flatnonzero(nbytes == np.iinfo(np.uint64).max)
            if bad.size:
                raise ValueError(f"image {order[int(bad[0])]}: a symbol outside the model's symbol count")
            out: list = [None] * len(imgs)
            ends = [b[0] for b in bases[1:]] + [len(order)]
            for (k0, at), k1 in zip(bases, ends):
                sz = nbytes[k0:k1].astype(np.int64)
                part = d_blob.view(at).download((int(sz.sum()),), np.uint8)
                for i, piece in zip(order[k0:k1], np.split(part, np.cumsum(sz)[:-1])):
                    out[i] = piece.tobytes()
            return out
        d_blob, d_sizes = self._entropy_encode(d_sym, counts, cum_freq, segment)
        nbytes = d_sizes.download((len(imgs),), np.uint64)
        bad = np.flatnonzero(nbytes == np.iinfo(np.uint64).max)
        if bad.size:
            raise ValueError(f"image {int(bad[0])}: a symbol outside the frequency table")
        blob = d_blob.download((int(nbytes.sum()),), np.uint8)
        cuts = np.cumsum(nbytes.astype(np.int64))[:-1]
        return [part.tobytes() for part in np.split(blob, cuts)]

    def _check_streams(self, streams, sizes, cum_freq):
        """The host validation of ``decode_streams_to_images`` and ``decode_regions``: every
        container parsed as the version the table's rank selects, its K / K0, geometry, neighbours
        and CRC against the tables, its symbol count against the image size and the code shape.
        ``(version, tables, sizes, counts, min_L)``; tables is None for version 1."""
        from . import entropy
        ctx, nbr = entropy.is_ctx_table(cum_freq), entropy.is_nbr_table(cum_freq)
        if nbr:
            tables = entropy.nbr_tables(cum_freq)
            crc = entropy.tables_crc(tables)
            mine = (tables.shape[0], tuple(int(v) for v in self.codec.code_shape), entropy.neighbours_of(tables))
        elif ctx:
            tables = entropy.ctx_tables(cum_freq)
            crc = entropy.tables_crc(tables)
        sizes = [(int(H), int(W)) for H, W in sizes]
        if len(streams) != len(sizes):
            raise ValueError(f"{len(streams)} streams for {len(sizes)} image sizes")
        code = int(np.prod(self.codec.code_shape))
        counts, min_L = [], 16384
        for i, (buf, (H, W)) in enumerate(zip(streams, sizes)):
            if H <= 0 or W <= 0:
                raise ValueError(f"image size {H}x{W} must be positive")
            if nbr:
                L, n, K0, hcrc, geometry, neighbours = entropy.parse_nbr(buf)
                if (K0, geometry, neighbours) != mine or hcrc != crc:
                    raise ValueError(f"stream {i} was coded under other neighbour tables (K0 {K0}, geometry "
                                     f"{geometry}, neighbours {neighbours}, CRC {hcrc:#010x}; given K0 {mine[0]}, "
                                     f"geometry {mine[1]}, neighbours {mine[2]}, CRC {crc:#010x})")
            elif ctx:
                L, n, K, hcrc = entropy.parse_ctx(buf)
                if K != tables.shape[0] or hcrc != crc:
                    raise ValueError(f"stream {i} was coded under other context tables (K {K}, CRC {hcrc:#010x}; "
                                     f"given K {tables.shape[0]}, CRC {crc:#010x})")
            else:
                L, n = entropy.parse(buf)
            want = self.num_patches(H, W) * code
            if n != want:
                raise ValueError(f"stream {i} holds {n} symbols, a {H}x{W} image has {want}")
            counts.append(n)
            min_L = min(min_L, L)
        return (3 if nbr else 2 if ctx else 1), (tables if ctx or nbr else None), sizes, counts, min_L

    def _check_streams_emb(self, streams, sizes, cum_freq):
        """``_check_streams`` for "TICA" containers, which carry their tables: every container
        parsed (entropy.parse_emb), its geometry against the codec's code shape, its symbol count
        against the image size.  ``(models, sizes, counts, Ls)``, or None when no stream is a
        "TICA" container and a table was given (the "TICS" path).  A list that mixes the two
        kinds is a ValueError, as is a "TICS" stream without a table."""
        from . import entropy
        emb = [entropy.is_adaptive(b) for b in streams]
        if not any(emb) and not (cum_freq is None or isinstance(cum_freq, entropy.Adaptive)):
            return None
        if not all(emb):
            if any(emb):
                raise ValueError("the list mixes \"TICA\" and \"TICS\" streams: decode them in separate calls")
            if len(streams):
                raise ValueError("\"TICS\" streams need the table they were coded under (cum_freq is None)")
        sizes = [(int(H), int(W)) for H, W in sizes]
        if len(streams) != len(sizes):
            raise ValueError(f"{len(streams)} streams for {len(sizes)} image sizes")
        geo = tuple(int(v) for v in self.codec.code_shape)
        code = int(np.prod(geo))
        models, counts, Ls = [], [], []
        for i, (buf, (H, W)) in enumerate(zip(streams, sizes)):
            if H <= 0 or W <= 0:
                raise ValueError(f"image size {H}x{W} must be positive")
            p = entropy.parse_emb(buf)
            if p["geometry"] != geo or p["nsym"] != int(self.codec.quan_scale) or p["K0"] not in (1, geo[2]):
                raise ValueError(f"stream {i} was coded for the code geometry {p['geometry']}, {p['nsym']} symbols and "
                                 f"K0 {p['K0']}; this codec has {geo}, {int(self.codec.quan_scale)} symbols and K0 1 or "
                                 f"{geo[2]}")
            want = self.num_patches(H, W) * code
            if p["n"] != want:
                raise ValueError(f"stream {i} holds {p['n']} symbols, a {H}x{W} image has {want}")
            # K0 = 1 = C (a one-channel code) is the same rows under either name
            models.append(entropy.Adaptive("channel" if p["K0"] == geo[2] else "none", p["neighbours"], p["nsym"]))
            counts.append(p["n"])
            Ls.append(p["L"])
        return models, sizes, counts, Ls

    @staticmethod
    def _groups(models):
        groups: dict = {}
        for i, m in enumerate(models):
            groups.setdefault(m, []).append(i)
        return groups

    def decode_streams_to_images(self, streams, sizes, cum_freq, post_filter: bool = True) -> list[np.ndarray]:
        """[container], [(H_i, W_i)] -> [uint8 [H_i, W_i, 3]]: every container is validated on the
        host (entropy.parse) and its symbol count checked against the image size and the code
        shape; then one upload, one decoder call for all of them and ``decode_images_device``.  A 2-D
        ``cum_freq`` reads version-2 containers, which must have been coded under these tables; a
        3-D one version-3 containers coded under these tables for this codec's code shape.  "TICA"
        containers carry their tables: ``cum_freq`` is None (or ignored), and the streams are
        decoded grouped by the model in their headers, one decoder call per group."""
        emb = self._check_streams_emb(streams, sizes, cum_freq)
        if emb is not None:
            models, sizes, counts, Ls = emb
            if not sizes:
                return []
            c = self.codec
            blob = np.frombuffer(b"".join(bytes(b) for b in streams), np.uint8)
            bsizes = np.array([len(b) for b in streams], np.int64)
            boffs = np.concatenate([[0], np.cumsum(bsizes)[:-1]]).astype(np.int64)
            soffs = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)
            cnts = np.array(counts, np.int64)
            groups = self._groups(models)
            d_blob = self._buf("entropy_blob", blob.size)
            d_blob.upload(blob)
            d_scr = self._buf("entropy_scratch", max(
                c.entropy_emb_scratch_bytes(cnts[idx], min(Ls[i] for i in idx), m, c.code_shape[2])
                for m, idx in groups.items()))
            d_sym = self._buf("symbols", sum(counts))
            for m, idx in groups.items():
                c.entropy_decode_emb_device(d_blob, boffs[idx], bsizes[idx], cnts[idx], m, d_sym, soffs[idx], d_scr)
            offsets, total = self.packed_offsets(sizes)
            d_out = self._buf("image_out", total)
            self.decode_images_device(d_sym, offsets, sizes, d_out, post_filter)
            self.synchronize()
            flat = d_out.download((total,), np.uint8)
            return [flat[o:o + H * W * 3].reshape(H, W, 3).copy() for o, (H, W) in zip(offsets, sizes)]
        ver, tables, sizes, counts, min_L = self._check_streams(streams, sizes, cum_freq)
        if not sizes:
            return []
        ctx, nbr = ver >= 2, ver == 3
        c = self.codec
        blob = np.frombuffer(b"".join(bytes(b) for b in streams), np.uint8)
        bsizes = [len(b) for b in streams]
        boffs = np.concatenate([[0], np.cumsum(bsizes)[:-1]]).astype(np.int64)
        soffs = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)
        if nbr:
            c.entropy_set_tables_nbr(tables)
        elif ctx:
            c.entropy_set_tables(tables)
        else:
            c.entropy_set_table(cum_freq)
        d_blob = self._buf("entropy_blob", blob.size)
        d_blob.upload(blob)
        d_scr = self._buf("entropy_scratch", c.entropy_scratch_bytes(counts, min_L))
        d_sym = self._buf("symbols", sum(counts))
        decode = c.entropy_decode_nbr_device if nbr else c.entropy_decode_ctx_device if ctx else c.entropy_decode_device
        decode(d_blob, boffs, bsizes, counts, d_sym, soffs, d_scr)
        offsets, total = self.packed_offsets(sizes)
        d_out = self._buf("image_out", total)
        self.decode_images_device(d_sym, offsets, sizes, d_out, post_filter)
        self.synchronize()
        flat = d_out.download((total,), np.uint8)
        return [flat[o:o + H * W * 3].reshape(H, W, 3).copy() for o, (H, W) in zip(offsets, sizes)]

    # ------------------------------------------------------------------ regions
    # A rectangle of an image from a small part of its container: patches are independent and so
    # are the segments of a container, so the crop needs the patches it touches (and, with the
    # post-filter, those its windows reach: tic_region_plan) and those patches' symbols need the
    # segments that hold them and nothing else (tic_entropy_decode_ranges*_device).
    RMBE_WINDOW = 128  # the post-filter's window side (submit/2/rmbe/rmbe.py:12)

    def region_plan(self, size, region, post_filter: bool = True) -> tuple[int, int, int, int]:
        """``(py0, py1, px0, px1)``: the box of patches the region ``(y, x, h, w)`` of an image of
        ``size = (H, W)`` is decoded from; with the post-filter (and a ``post`` codec) widened over
        the windows the region's pixels depend on.  ValueError for a region that is empty or not
        inside the image."""
        H, W = (int(v) for v in size)
        y, x, h, w = (int(v) for v in region)
        S = self.RMBE_WINDOW if post_filter and self.post is not None else 0
        return Codec.region_plan(H, W, self.codec.patch_size, y, x, h, w, S)

    @staticmethod
    def _merge_extents(extents):
        """Byte extents [(offset, length)] merged where they overlap or touch, sorted."""
        out: list[list[int]] = []
        for lo, ln in sorted((int(o), int(n)) for o, n in extents if n > 0):
            if out and lo <= out[-1][1]:
                out[-1][1] = max(out[-1][1], lo + ln)
            else:
                out.append([lo, lo + ln])
        return [(lo, hi - lo) for lo, hi in out]

    def decode_regions(self, streams, sizes, regions, cum_freq, post_filter: bool = True) -> list[np.ndarray]:
        """[container], [(H_i, W_i)], [(y_i, x_i, h_i, w_i)] -> [uint8 [h_i, w_i, 3]]: the bytes of
        ``decode_streams_to_images(...)[i][y:y + h, x:x + w]`` from the patches of ``region_plan``'s
        box only.  Validation as ``decode_streams_to_images`` does it.  For every grid row of a box
        its patches are one contiguous symbol range, and the ranges' outputs laid back to back are
        the patch batch of the boxes.  Only the header, the length table and the byte extents of
        those ranges (entropy.range_extent, overlapping ones merged) are copied to the device, at
        their container offsets; the rest of the device buffer is left as it was.  Then one range
        decoder call, one decoder call, one stitch, the region post-filter on the post-filter's
        stream, one rounding, the crops and one download.  ``last_region_stats`` holds, per
        stream, the patches decoded and the bytes uploaded.  "TICA" containers (``cum_freq`` None)
        work the same way: their head also holds the table block, and the ranges are decoded
        grouped by their container's model."""
        from . import entropy
        emb = self._check_streams_emb(streams, sizes, cum_freq)
        if emb is not None:  # "TICA": the tables travel in the head of every container
            models, sizes, counts, Ls = emb
            ver, tables, min_L = 0, None, min(Ls, default=16384)
        else:
            ver, tables, sizes, counts, min_L = self._check_streams(streams, sizes, cum_freq)
        if len(regions) != len(sizes):
            raise ValueError(f"{len(regions)} regions for {len(sizes)} images")
        if not sizes:
            return []
        c = self.codec
        P = c.patch_size
        code = int(np.prod(c.code_shape))
        use_post = post_filter and self.post is not None
        hdr = {0: 0, 1: entropy.HEADER_BYTES, 2: entropy.HEADER_BYTES_CTX, 3: entropy.HEADER_BYTES_NBR}[ver]
        extent = entropy.range_extent_emb if ver == 0 else entropy.range_extent
        regions = [tuple(int(v) for v in r) for r in regions]
        bsizes = [len(b) for b in streams]
        boffs = np.concatenate([[0], np.cumsum(bsizes)[:-1]]).astype(np.int64)
        # per range (one per grid row of a box): its container, first symbol and symbol count
        r_stream, r_first, r_count = [], [], []
        boxes, origins, crops, pieces, stats = [], [], [], [], []
        for i, ((H, W), (y, x, h, w), buf) in enumerate(zip(sizes, regions, streams)):
            py0, py1, px0, px1 = self.region_plan((H, W), (y, x, h, w), post_filter)
            wn = self.grid(H, W)[1]
            L = int.from_bytes(bytes(buf[8:12]), "little")  # validated above
            if ver == 0:  # header, table block, length table
                hdr = entropy.HEADER_BYTES_EMB + int.from_bytes(bytes(buf[32:36]), "little")
            head = bytes(buf[:hdr + 2 * -(-counts[i] // L)])
            extents = []
            for py in range(py0, py1):
                first, count = (py * wn + px0) * code, (px1 - px0) * code
                r_stream.append(i), r_first.append(first), r_count.append(count)
                extents.append(extent(head, first, count)[2:])
            merged = self._merge_extents(extents)
            pieces += [(int(boffs[i]), head)] + [(int(boffs[i]) + o, bytes(buf[o:o + ln])) for o, ln in merged]
            boxes.append((min(py1 * P, H) - py0 * P, min(px1 * P, W) - px0 * P))
            origins.append((py0 * P, px0 * P))
            crops.append((y - py0 * P, x - px0 * P))
            stats.append({"patches": (py1 - py0) * (px1 - px0), "patches_image": self.num_patches(H, W),
                          "bytes_uploaded": len(head) + sum(ln for _, ln in merged), "bytes_container": len(buf)})
        self.last_region_stats = stats
        n_box = sum(s["patches"] for s in stats)
        if ver == 3:
            c.entropy_set_tables_nbr(tables)
        elif ver == 2:
            c.entropy_set_tables(tables)
        elif ver == 1:
            c.entropy_set_table(cum_freq)
        d_blob = self._buf("entropy_blob", int(sum(bsizes)))
        for at, data in pieces:  # the sparse upload: everything else in d_blob stays as it was
            d_blob.view(at).upload(np.frombuffer(data, np.uint8))
        d_sym = self._buf("symbols", n_box * code)
        soffs = np.concatenate([[0], np.cumsum(r_count)[:-1]]).astype(np.int64)
        if ver == 0:  # the ranges grouped by their container's model, one range-decoder call per group
            groups = self._groups([models[i] for i in r_stream])
            pick = lambda vals, idx: [vals[k] for k in idx]
            d_scr = self._buf("entropy_scratch", max(
                c.entropy_ranges_emb_scratch_bytes(pick(r_first, idx), pick(r_count, idx), min_L, m, c.code_shape[2])
                for m, idx in groups.items()))
            for m, idx in groups.items():
                rs = pick(r_stream, idx)
                c.entropy_decode_ranges_emb_device(d_blob, [boffs[i] for i in rs], [bsizes[i] for i in rs],
                                                   [counts[i] for i in rs], pick(r_first, idx), pick(r_count, idx), m,
                                                   d_sym, soffs[idx], d_scr)
        else:
            d_scr = self._buf("entropy_scratch", c.entropy_ranges_scratch_bytes(r_first, r_count, min_L))
            c.entropy_decode_ranges_device(d_blob, [boffs[i] for i in r_stream], [bsizes[i] for i in r_stream],
                                           [counts[i] for i in r_stream], r_first, r_count, d_sym, soffs, d_scr,
                                           version=ver)
        # the boxes are the images of a group: decode_images_device's steps with the region filter
        offsets, total = self.packed_offsets(boxes)
        runs = self._runs(offsets, boxes)
        d_f = self._buf("patches_f32", n_box * P * P * 3 * 4)
        d_u8 = self._buf("image_out", total)
        out_sizes = [(h, w) for _, _, h, w in regions]
        out_offs, out_total = self.packed_offsets(out_sizes)
        d_crop = self._buf("region_out", out_total)
        if use_post:
            k = self._slot
            self._slot = (k + 1) % self.NSLOT
            self.last_slot = k
            d_img = self._buf(f"image_f32_{k}", total * 4)
            c.decode_device(d_sym, n_box, None, d_f)
            c.wait_event(self.post, k)
            c.patches_to_images_device(d_f, offsets, boxes, P, d_img)
            c.record(k)
            self.post.wait_event(c, k)
            self.post.rmbe_regions_device(d_img, offsets, boxes, origins, sizes)
            last = self.post
        else:
            d_img = self._buf("image_f32_0", total * 4)
            if self.post is not None:
                c.wait_event(self.post, 0)
            c.decode_device(d_sym, n_box, None, d_f)
            c.patches_to_images_device(d_f, offsets, boxes, P, d_img)
            last = c
        for lo, ln in runs:
            last.round_u8_device(d_img.view(lo * 4), ln, d_u8.view(lo))
        last.crop_regions_device(d_u8, offsets, boxes, crops, out_sizes, out_offs, d_crop)
        if use_post:
            self.post.record(k)
        elif self.post is not None:
            c.record(0)
            self.post.wait_event(c, 0)
        self.synchronize()
        flat = d_crop.download((out_total,), np.uint8)
        return [flat[o:o + h * w * 3].reshape(h, w, 3).copy() for o, (h, w) in zip(out_offs, out_sizes)]

    # ------------------------------------------------------------------ rate / distortion
    def evaluate_images(self, images, post_filter: bool = True, cum_freq=None,
                        entropy_segment: int | None = None) -> list[dict]:
        """Round trip of a list of uint8 [H_i, W_i, 3] images with its quality and rate measures,
        without leaving the device: one upload, ``encode_images_device`` / ``decode_images_device``
        on one arena, per image the exact squared error (tic_sse_u8_device) and the symbol
        histogram (tic_histogram_device) through views, one tic_msssim_images_device call over
        the images with both sides >= 161 (smaller ones get ``msssim = nan``), one download of
        the small results.  Per image: ``sse`` (int), ``psnr`` (evaluate.mse2psnr of sse / dims),
        ``msssim``, ``counts`` (uint64 [Q]), ``n_symbols`` and ``est_bits``
        (evaluate.estimated_bits under ``cum_freq``, a range_coder.symbol_table table; None
        without one).  With ``entropy_segment`` and ``cum_freq`` every result also has
        ``coded_bytes``: the size of the image's segmented-stream container at that segment length,
        from one entropy_encode_device call over the symbols on the device (the real rate beside
        the estimate).  Under a 2-D ``cum_freq`` ([K, Q + 1] context tables, entropy.py)
        ``est_bits`` is evaluate.estimated_bits_ctx of the image's per-context histogram
        (tic_histogram_ctx_device) and ``coded_bytes`` the size of its version-2 container; under a
        3-D one ([K0, M, Q + 1]) ``est_bits`` uses the rows the neighbour coder uses at
        ``entropy_segment`` (tic_histogram_nbr_device; entropy.DEFAULT_SEGMENT without one) and
        ``coded_bytes`` is the size of the version-3 container.  Under an ``entropy.Adaptive``
        ``coded_bytes`` is the size of the image's "TICA" container, tables included (at
        ``entropy_segment``, entropy.DEFAULT_SEGMENT without one), and ``est_bits`` is None: the
        tables are the image's own.  Images
        start at 4-byte boundaries of the arena (the alignment tic_sse_u8_device asks for)."""
        from . import entropy
        from . import evaluate as ev
        adaptive = isinstance(cum_freq, entropy.Adaptive)  # real coded_bytes, no estimate: the tables are the image's own
        if adaptive and entropy_segment is None:
            entropy_segment = entropy.DEFAULT_SEGMENT
        tables = entropy.ctx_tables(cum_freq) if cum_freq is not None and not adaptive and entropy.is_ctx_table(cum_freq) \
            else None
        nbr = cum_freq is not None and not adaptive and entropy.is_nbr_table(cum_freq)
        if nbr:  # the estimate sees the K0 * M rows as a version-2 estimate sees its K rows
            t3 = entropy.nbr_tables(cum_freq)
            tables = t3.reshape(-1, t3.shape[2])
        imgs = [np.ascontiguousarray(im) for im in images]
        for im in imgs:
            if im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] != 3 or im.size == 0:
                raise ValueError(f"image must be uint8 [H, W, 3], got {im.dtype} {im.shape}")
        if not imgs:
            return []
        c = self.codec
        Q = c.quan_scale
        sizes = [tuple(int(v) for v in im.shape[:2]) for im in imgs]
        offsets, total = [], 0
        for H, W in sizes:
            offsets.append(total)
            total += -(-(H * W * 3) // 4) * 4
        code = int(np.prod(c.code_shape))
        if code % 4:
            raise ValueError(f"code of {code} symbols per patch: the per-image histogram needs a multiple of 4")
        counts = [self.num_patches(H, W) for H, W in sizes]
        pbase = np.concatenate([[0], np.cumsum(counts)])
        arena = np.zeros(total, np.uint8)
        for im, off in zip(imgs, offsets):
            arena[off:off + im.size] = im.reshape(-1)
        d_img = self._buf("image_u8", total)
        d_img.upload(arena)
        d_sym = self._buf("symbols", int(pbase[-1]) * code)
        d_out = self._buf("image_out", total)
        self.encode_images_device(d_img, offsets, sizes, d_sym)
        d_sizes = None
        emb_order = None
        if adaptive:
            _, d_sizes, emb_order, _ = self._entropy_encode_emb(d_sym, [k * code for k in counts], cum_freq,
                                                                int(entropy_segment))
        elif entropy_segment is not None and cum_freq is not None:
            _, d_sizes = self._entropy_encode(d_sym, [k * code for k in counts], cum_freq, int(entropy_segment))
        self.decode_images_device(d_sym, offsets, sizes, d_out, post_filter)
        if post_filter and self.post is not None:
            c.wait_event(self.post, self.last_slot)  # d_out was written on the post-filter's stream
        big = [i for i, (H, W) in enumerate(sizes) if min(H, W) >= ev.MSSSIM_MIN_SIDE]
        n, rec = len(imgs), (1 + Q) * 8  # per image: sse, counts[Q] (uint64); then 30 doubles per MS-SSIM image
        d_res = self._buf("eval_results", n * rec + len(big) * 240)
        c.memset_device(d_res, 0, n * rec)
        for i, (H, W) in enumerate(sizes):
            c.sse_u8_device(d_img.view(offsets[i]), d_out.view(offsets[i]), H * W * 3, d_res.view(i * rec))
            c.histogram_device(d_sym.view(int(pbase[i]) * code), counts[i] * code, Q, d_res.view(i * rec + 8))
        if big:
            bsizes = [sizes[i] for i in big]
            d_scr = self._buf("msssim_scratch", c.msssim_scratch_bytes(bsizes))
            c.msssim_images_device(d_img, d_out, [offsets[i] for i in big], bsizes, d_scr, d_res.view(n * rec))
        ctx_counts = None
        if tables is not None:
            K = tables.shape[0]
            if tables.shape[1] != Q + 1:
                raise ValueError(f"context tables of {tables.shape[1] - 1} symbols for a quantiser of {Q}")
            d_ctx = self._buf("eval_ctx_counts", n * K * Q * 8)
            c.memset_device(d_ctx, 0, n * K * Q * 8)
            if nbr:
                c.entropy_set_tables_nbr(t3)
                seg = entropy.DEFAULT_SEGMENT if entropy_segment is None else int(entropy_segment)
            for i in range(n):
                if nbr:
                    c.histogram_nbr_device(d_sym, [int(pbase[i]) * code], [counts[i] * code], Q, seg,
                                           d_ctx.view(i * K * Q * 8))
                else:
                    c.histogram_ctx_device(d_sym.view(int(pbase[i]) * code), counts[i] * code, Q, K,
                                           d_ctx.view(i * K * Q * 8))
            ctx_counts = d_ctx.download((n, K, Q), np.uint64)
        raw = d_res.download((n * rec + len(big) * 240,), np.uint8)
        ints = raw[:n * rec].view(np.uint64).reshape(n, 1 + Q)
        sums = raw[n * rec:].view(np.float64).reshape(len(big), 5, 3, 2)
        ms = {i: ev.msssim_from_sums(sums[k], *sizes[i]) for k, i in enumerate(big)}
        coded = None if d_sizes is None else d_sizes.download((n,), np.uint64)
        if emb_order is not None:  # the sizes lie group after group
            coded = coded[np.argsort(emb_order)]
        if coded is not None and np.any(coded == np.iinfo(np.uint64).max):
            raise ValueError("a symbol outside the frequency table")
        out = []
        for i, (H, W) in enumerate(sizes):
            sse = int(ints[i, 0])
            cnt = ints[i, 1:].copy()
            with np.errstate(divide="ignore"):
                psnr = float(ev.mse2psnr(np.float64(sse) / (H * W * 3)))
            if cum_freq is None or adaptive:
                est = None
            elif tables is not None:
                est = ev.estimated_bits_ctx(ctx_counts[i], tables)
            else:
                est = ev.estimated_bits(cnt, cum_freq)
            out.append({"sse": sse, "psnr": psnr, "msssim": ms.get(i, float("nan")), "counts": cnt,
                        "n_symbols": counts[i] * code, "est_bits": est})
            if coded is not None:
                out[-1]["coded_bytes"] = int(coded[i])
        return out

    def close(self) -> None:
        for b in self._bufs.values():
            b.free()
        self._bufs.clear()


def symbol_histogram(codec: Codec, d_sym: DeviceBuffer, n_symbols: int, Q: int,
                     d_counts: DeviceBuffer | None = None, reset: bool = True) -> np.ndarray:
    """np.histogram(symbols, range(Q + 1))[0] on the GPU (get_encoded_distribution.py:113-126)."""
    own = d_counts is None
    if own:
        d_counts = codec.alloc(8 * Q)
    if reset:
        codec.memset_device(d_counts, 0, 8 * Q)
    codec.histogram_device(d_sym, n_symbols, Q, d_counts)
    counts = d_counts.download((Q,), np.uint64)
    if own:
        d_counts.free()
    return counts

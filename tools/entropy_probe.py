#!/usr/bin/env python3
"""What does range-coding on the GPU (segmented streams, csrc/tic_entropy.cpp) cost beside the
host coder the CLI uses by default?

Runs on the GPU, in one process; every timed window ends in a synchronise and is timed with the
host clock; the arms of a comparison alternate, and the order of the segment lengths is reversed
from one window to the next.

  (a) coder alone: 64 model_0 patches' worth of symbols (64 x 16384 = 1 Mi binary symbols drawn
      from each of three tables), resident on the device.  Per segment length L: the time of one
      entropy_encode_device call and of one entropy_decode_device call.  Beside them the host
      path of today's CLI on the same symbols: download, widen to int64, RangeEncoder to a file;
      RangeDecoder from that file.
  (b) end to end: the 24-image mix of tools/image_batch_probe.py on model_0 at P = 256, groups of
      plan_batches.  Encode: encode_images + one RangeEncoder file per image against
      encode_images_to_streams (+ writing the files).  Decode: RangeDecoder per file +
      decode_images against decode_streams_to_images (+ reading the files).  Per L.
  (c) byte overhead: total container bytes over total single-stream bytes on the real symbols of
      (b), per L.

The result goes to profiles/entropy_<tag>.json (or --out).
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.image_batch_probe import SEED, SIZES, seeded_images, stats  # noqa: E402

SEGMENTS = [1024, 2048, 4096, 8192, 16384]
TABLES = {"p60": [0, 2457, 4096], "p90": [0, 3685, 4096], "p98": [0, 4013, 4096]}


def window(fn, sync, passes):
    sync()
    t = time.perf_counter()
    for _ in range(passes):
        fn()
    sync()
    return (time.perf_counter() - t) * 1e3 / passes


def coder_alone(codec, args, tmp):
    from tf_image_compression_amd import entropy
    from tf_image_compression_amd.range_coder import RangeDecoder, RangeEncoder
    n = 64 * 16384
    out = {}
    for name, cum in TABLES.items():
        rng = np.random.default_rng(SEED)
        p = np.diff(np.asarray(cum, np.float64)) / cum[-1]
        sym = rng.choice(len(p), size=n, p=p).astype(np.uint8)
        d_sym, d_back = codec.alloc(n), codec.alloc(n)
        d_sym.upload(sym)
        codec.entropy_set_table(cum)
        d_scr = codec.alloc(max(codec.entropy_scratch_bytes([n], L) for L in SEGMENTS))
        d_blob = codec.alloc(max(entropy.bound(n, L) for L in SEGMENTS))
        d_size = codec.alloc(8)
        path = os.path.join(tmp, "single.encoded")

        def host_encode():
            seq = d_sym.download((n,), np.uint8)
            enc = RangeEncoder(path)
            enc.encode(seq, cum)  # widens to int64, as encode.py's store() does
            enc.close()

        def host_decode():
            dec = RangeDecoder(path)
            seq = dec.decode_array(n, cum).astype(np.uint8)
            dec.close()
            d_back.upload(seq)

        arms = {}
        sizes = {}
        for L in SEGMENTS:
            def enc(L=L):
                codec.entropy_encode_device(d_sym, [0], [n], L, d_scr, d_blob, d_size)
            enc()
            size = int(d_size.download((1,), np.uint64)[0])
            blob = d_blob.download((size,), np.uint8).tobytes()
            if blob != entropy.pack(sym, cum, segment=L):
                raise SystemExit(f"{name} L={L}: the device container differs from the host's")
            # decode from a copy of its own, so that encode windows do not rewrite what it reads
            d_in = codec.alloc(size)
            d_in.upload(np.frombuffer(blob, np.uint8))

            def dec(L=L, d_in=d_in, size=size):
                codec.entropy_decode_device(d_in, [0], [size], [n], d_back, [0], d_scr)
            dec()
            if not np.array_equal(d_back.download((n,), np.uint8), sym):
                raise SystemExit(f"{name} L={L}: the device decoder's symbols differ")
            arms[f"device_encode_L{L}"] = (enc, args.passes)
            arms[f"device_decode_L{L}"] = (dec, args.passes)
            sizes[L] = size
        host_encode()
        single = os.path.getsize(path)
        host_decode()
        if not np.array_equal(d_back.download((n,), np.uint8), sym):
            raise SystemExit(f"{name}: the host decoder's symbols differ")
        arms["host_encode"] = (host_encode, 1)
        arms["host_decode"] = (host_decode, 1)
        for fn, _ in arms.values():
            fn()
        ms = {k: [] for k in arms}
        for w in range(args.windows):
            order = list(arms) if w % 2 == 0 else list(arms)[::-1]
            for k in order:
                fn, passes = arms[k]
                ms[k].append(window(fn, codec.synchronize, passes))
        res = {k: stats(v) for k, v in ms.items()}
        for k, r in res.items():
            r["msym_per_s"] = round(n / r["median_ms"] / 1e3, 1)
        out[name] = {"cum_freq": cum, "symbols": n, "single_stream_bytes": single,
                     "container_bytes": {str(L): sizes[L] for L in SEGMENTS},
                     "overhead": {str(L): round(sizes[L] / single - 1, 5) for L in SEGMENTS}, "times": res}
        print(json.dumps({name: {k: (r["median_ms"], r["spread"]) for k, r in res.items()}}), flush=True)
    return out


def end_to_end(codec, args, tmp):
    from tf_image_compression_amd import entropy
    from tf_image_compression_amd.image_codec import ImageCodec
    from tf_image_compression_amd.range_coder import RangeDecoder, RangeEncoder, symbol_table
    ic = ImageCodec(codec)
    P = codec.patch_size
    sizes = SIZES[:args.images] if args.images else SIZES
    images = seeded_images(sizes, SEED)
    groups = ic.plan_batches(sizes, P, args.max_images)
    code_shape = codec.code_shape
    # the table the CLI would use: the measured distribution of these symbols
    symbols = []
    for g in groups:
        symbols += ic.encode_images([images[i] for i in g])
    hist = np.bincount(np.concatenate([s.reshape(-1) for s in symbols]), minlength=codec.quan_scale)
    cum = symbol_table(hist / hist.sum(), resolution=4096)
    files = [os.path.join(tmp, f"img{i}.encoded") for i in range(len(images))]

    def host_encode():
        for g in groups:
            for i, sym in zip(g, ic.encode_images([images[i] for i in g])):
                enc = RangeEncoder(files[i])
                enc.encode(sym.reshape(-1), cum)
                enc.close()

    def host_decode():
        for g in groups:
            syms = []
            for i in g:
                dec = RangeDecoder(files[i])
                syms.append(dec.decode_array(symbols[i].size, cum).astype(np.uint8).reshape((-1,) + tuple(code_shape)))
                dec.close()
            ic.decode_images(syms, [sizes[i] for i in g], post_filter=False)

    def device_encode(L, keep=None):
        for g in groups:
            for i, s in zip(g, ic.encode_images_to_streams([images[i] for i in g], cum, segment=L)):
                with open(files[i] + f".L{L}", "wb") as f:
                    f.write(s)
                if keep is not None:
                    keep[i] = s

    def device_decode(L, keep=None):
        for g in groups:
            streams = [open(files[i] + f".L{L}", "rb").read() for i in g]
            out = ic.decode_streams_to_images(streams, [sizes[i] for i in g], cum, post_filter=False)
            if keep is not None:
                for i, im in zip(g, out):
                    keep[i] = im

    # equal results first
    host_encode()
    single = [os.path.getsize(f) for f in files]
    ref = {}
    for g in groups:
        for i, im in zip(g, ic.decode_images([symbols[i] for i in g], [sizes[i] for i in g], post_filter=False)):
            ref[i] = im
    container = {}
    for L in SEGMENTS:
        streams, recon = {}, {}
        device_encode(L, streams)
        for i, s in streams.items():
            if not np.array_equal(entropy.unpack(s, cum), symbols[i].reshape(-1)):
                raise SystemExit(f"L={L} image {i}: the container's symbols differ from encode_images'")
        device_decode(L, recon)
        for i in recon:
            if not np.array_equal(recon[i], ref[i]):
                raise SystemExit(f"L={L} image {i}: the decoded image differs")
        container[L] = [len(streams[i]) for i in range(len(images))]

    arms = {"host_encode": host_encode, "host_decode": host_decode}
    for L in SEGMENTS:
        arms[f"device_encode_L{L}"] = lambda L=L: device_encode(L)
        arms[f"device_decode_L{L}"] = lambda L=L: device_decode(L)
    ms = {k: [] for k in arms}
    for w in range(args.windows):
        order = list(arms) if w % 2 == 0 else list(arms)[::-1]
        for k in order:
            ms[k].append(window(arms[k], ic.synchronize, 1))
    res = {k: stats(v) for k, v in ms.items()}
    print(json.dumps({"end_to_end": {k: (r["median_ms"], r["spread"]) for k, r in res.items()}}), flush=True)
    n_sym = int(sum(s.size for s in symbols))
    out = {"model": 0, "patch": P, "images": len(images), "pixels": int(sum(H * W for H, W in sizes)),
           "groups": groups, "symbols": n_sym, "cum_freq": [int(v) for v in cum], "outputs_equal": True,
           "times": res,
           "overhead": {"single_stream_bytes": int(sum(single)),
                        "container_bytes": {str(L): int(sum(container[L])) for L in SEGMENTS},
                        "overhead": {str(L): round(sum(container[L]) / sum(single) - 1, 5) for L in SEGMENTS}}}
    ic.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--tag", default="probe")
    ap.add_argument("--out", default=None, help="default: profiles/entropy_<tag>.json")
    ap.add_argument("--windows", type=int, default=7, help="timed windows per arm")
    ap.add_argument("--passes", type=int, default=50, help="device coder calls per window in (a)")
    ap.add_argument("--max-images", type=int, default=16)
    ap.add_argument("--images", type=int, default=0, help="only the first N images of the list (0: all)")
    ap.add_argument("--skip", choices=["a", "b"], action="append", default=[])
    args = ap.parse_args()
    from tf_image_compression_amd.codec import Codec
    from tf_image_compression_amd.weights import synthetic_params, SYNTH_MEAN, SYNTH_STD
    out_path = args.out or os.path.join(ROOT, "profiles", f"entropy_{args.tag}.json")
    codec = Codec(0, synthetic_params(0), SYNTH_MEAN, SYNTH_STD, patch_size=256)
    doc = {"tool": "tools/entropy_probe.py", "tag": args.tag, "seed": SEED, "device": codec.device_info(),
           "windows": args.windows, "passes_per_window_a": args.passes, "segments": SEGMENTS}
    with tempfile.TemporaryDirectory() as tmp:
        if "a" not in args.skip:
            doc["coder_alone"] = coder_alone(codec, args, tmp)
        if "b" not in args.skip:
            doc["end_to_end"] = end_to_end(codec, args, tmp)
    codec.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(f"wrote {out_path}")


if __name__ == "__main__":
    main()

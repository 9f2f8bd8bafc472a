#!/usr/bin/env python3
"""What do per-channel and per-position tables (the context coder, "TICS" version 2,
csrc/tic_entropy.cpp) save in bytes, and what do they cost in time beside the single-table device
coder?

Runs on the GPU, in one process, on the symbols model_0 (P = 256, synthetic weights) produces for
the 24-image mix of tools/image_batch_probe.py.

  bytes   The tables are ESTIMATED ON ONE HALF of the images (the even-numbered ones; per-context
          histograms through tic_histogram_ctx_device, checked against numpy) and APPLIED TO THE
          OTHER HALF: one container per odd-numbered image at segment length L, under the single
          table (version 1), one table per channel (K = 64) and one per code position
          (K = 16 * 16 * 64 = 16384).  Beside the container bytes the ideal code lengths
          (evaluate.estimated_bits / estimated_bits_ctx).  Also the same three with the tables
          estimated on the coded half itself (what a table fitted to its data would give).
  time    The first 64 patches of the mix's symbols (1 Mi) as one stream, resident on the device:
          one encode call and one decode call at L for the single table, K = 64 (tables staged in
          LDS) and K = 16384 (tables read from global memory).  Every timed window ends in a
          synchronise and is timed with the host clock; a round times the six arms one after
          another, each in a window of its own, and every other round runs them in reverse
          order.  Every arm's output is checked against the host coder first.

The result goes to profiles/entropy_ctx_<tag>.json (or --out).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.image_batch_probe import SEED, SIZES, seeded_images, stats  # noqa: E402


def window(fn, sync, passes):
    sync()
    t = time.perf_counter()
    for _ in range(passes):
        fn()
    sync()
    return (time.perf_counter() - t) * 1e3 / passes


def context_counts(codec, sym, K, Q):
    """[K, Q] histogram of a stream of whole patches on the device, checked against numpy."""
    d_sym, d_cnt = codec.alloc(sym.size), codec.alloc(8 * K * Q)
    d_sym.upload(sym)
    codec.memset_device(d_cnt, 0, 8 * K * Q)
    codec.histogram_ctx_device(d_sym, sym.size, Q, K, d_cnt)
    got = d_cnt.download((K, Q), np.uint64)
    d_sym.free()
    d_cnt.free()
    folded = sym.reshape(-1, K)
    want = np.stack([(folded == q).sum(axis=0) for q in range(Q)], axis=1).astype(np.uint64)
    if not np.array_equal(got, want):
        raise SystemExit(f"K={K}: tic_histogram_ctx_device differs from numpy")
    return got.astype(np.float64)


def tables_for(counts, resolution=4096):
    from tf_image_compression_amd.range_coder import symbol_table, symbol_tables
    if counts.shape[0] == 1:
        return symbol_table(counts[0] / counts[0].sum(), resolution=resolution)
    return symbol_tables(counts / counts.sum(axis=1, keepdims=True), resolution=resolution)


def coded_bytes(codec, streams, table, L):
    """Container sizes of the streams under `table` from one device coder call, checked against
    the host coder on the first stream."""
    from tf_image_compression_amd import entropy
    ctx = entropy.is_ctx_table(table)
    counts = [s.size for s in streams]
    offs = np.concatenate([[0], np.cumsum(counts)[:-1]])
    d_sym = codec.alloc(sum(counts))
    d_sym.upload(np.concatenate(streams))
    d_scr = codec.alloc(codec.entropy_scratch_bytes(counts, L))
    d_blob = codec.alloc(sum(entropy.bound(n, L, table) for n in counts))
    d_sizes = codec.alloc(8 * len(counts))
    if ctx:
        codec.entropy_set_tables(table)
        codec.entropy_encode_ctx_device(d_sym, offs, counts, L, d_scr, d_blob, d_sizes)
    else:
        codec.entropy_set_table(table)
        codec.entropy_encode_device(d_sym, offs, counts, L, d_scr, d_blob, d_sizes)
    sizes = d_sizes.download((len(counts),), np.uint64).astype(np.int64)
    first = d_blob.download((int(sizes[0]),), np.uint8).tobytes()
    if first != entropy.pack(streams[0], table, segment=L):
        raise SystemExit("the device container differs from the host's")
    for b in (d_sym, d_scr, d_blob, d_sizes):
        b.free()
    return [int(v) for v in sizes]


def rate(codec, symbols, Q, code, C_, L):
    from tf_image_compression_amd.evaluate import estimated_bits, estimated_bits_ctx
    train = np.concatenate([s.reshape(-1) for s in symbols[0::2]])
    test = [s.reshape(-1) for s in symbols[1::2]]
    test_all = np.concatenate(test)
    out = {"segment": L, "train_images": len(symbols[0::2]), "test_images": len(test),
           "train_symbols": int(train.size), "test_symbols": int(test_all.size),
           "raw_bytes": int(test_all.size // 8) if Q == 2 else int(test_all.size)}
    for fit, src in (("held_out", train), ("fitted_to_the_coded_half", test_all)):
        rows = {}
        for name, K in (("single_table", 1), ("per_channel", C_), ("per_position", code)):
            counts = context_counts(codec, src, K, Q)
            table = tables_for(counts)
            on_test = context_counts(codec, test_all, K, Q)
            ideal = estimated_bits(on_test[0], table) if K == 1 else estimated_bits_ctx(on_test, table)
            sizes = coded_bytes(codec, test, table, L)
            rows[name] = {"K": K, "container_bytes": int(sum(sizes)), "ideal_bytes": round(ideal / 8, 1)}
        base = rows["single_table"]["container_bytes"]
        for r in rows.values():
            r["of_single_table"] = round(r["container_bytes"] / base, 4)
        out[fit] = rows
    return out, train


def timing(codec, args, stream, train, Q, code, C_, L):
    from tf_image_compression_amd import entropy
    n = stream.size
    tables = {"single_table": tables_for(context_counts(codec, train, 1, Q)),
              "per_channel_K64": tables_for(context_counts(codec, train, C_, Q)),
              "per_position_K16384": tables_for(context_counts(codec, train, code, Q))}
    d_sym, d_back = codec.alloc(n), codec.alloc(n)
    d_sym.upload(stream)
    d_scr = codec.alloc(codec.entropy_scratch_bytes([n], L))
    d_blob = codec.alloc(entropy.bound(n, L) + 8)
    d_size = codec.alloc(8)
    # the version-1 table and the context tables are independent per handle; the two context
    # table sets need a handle each, so that no arm uploads tables inside its window
    from tf_image_compression_amd.codec import Codec
    from tf_image_compression_amd.weights import synthetic_params, SYNTH_MEAN, SYNTH_STD
    other = Codec(0, synthetic_params(0), SYNTH_MEAN, SYNTH_STD, patch_size=codec.patch_size)
    codec.entropy_set_table(tables["single_table"])
    codec.entropy_set_tables(tables["per_channel_K64"])
    other.entropy_set_tables(tables["per_position_K16384"])
    arms, sizes, copies = {}, {}, []
    for name, table in tables.items():
        h = other if name == "per_position_K16384" else codec
        enc_fn = h.entropy_encode_device if name == "single_table" else h.entropy_encode_ctx_device
        dec_fn = h.entropy_decode_device if name == "single_table" else h.entropy_decode_ctx_device

        def enc(enc_fn=enc_fn):
            enc_fn(d_sym, [0], [n], L, d_scr, d_blob, d_size)
        enc()
        h.synchronize()
        size = int(d_size.download((1,), np.uint64)[0])
        blob = d_blob.download((size,), np.uint8).tobytes()
        if blob != entropy.pack(stream, table, segment=L):
            raise SystemExit(f"{name}: the device container differs from the host's")
        d_in = codec.alloc(size)  # a copy of its own, so that encode windows do not rewrite what decode reads
        d_in.upload(np.frombuffer(blob, np.uint8))
        copies.append(d_in)

        def dec(dec_fn=dec_fn, d_in=d_in, size=size):
            dec_fn(d_in, [0], [size], [n], d_back, [0], d_scr)
        dec()
        h.synchronize()
        if not np.array_equal(d_back.download((n,), np.uint8), stream):
            raise SystemExit(f"{name}: the device decoder's symbols differ")
        arms[f"{name}_encode"] = (enc, h)
        arms[f"{name}_decode"] = (dec, h)
        sizes[name] = size
    for fn, h in arms.values():  # warm-up
        for _ in range(5):
            fn()
        h.synchronize()
    ms = {k: [] for k in arms}
    for w in range(args.windows):
        order = list(arms) if w % 2 == 0 else list(arms)[::-1]
        for k in order:
            fn, h = arms[k]
            ms[k].append(window(fn, h.synchronize, args.passes))
    res = {k: stats(v) for k, v in ms.items()}
    for k, r in res.items():
        base = res["single_table_" + k.rsplit("_", 1)[1]]["median_ms"]
        r["msym_per_s"] = round(n / r["median_ms"] / 1e3, 1)
        r["of_single_table"] = round(r["median_ms"] / base, 3)
    print(json.dumps({k: (r["median_ms"], r["spread"], r["of_single_table"]) for k, r in res.items()}), flush=True)
    other.close()
    for b in [d_sym, d_back, d_scr, d_blob, d_size] + copies:
        b.free()
    return {"symbols": int(n), "segment": L, "container_bytes": sizes, "times": res}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--tag", default="pr")
    ap.add_argument("--out", default=None, help="default: profiles/entropy_ctx_<tag>.json")
    ap.add_argument("--segment", type=int, default=2048)
    ap.add_argument("--windows", type=int, default=9, help="timed windows per arm (rounds over the arms)")
    ap.add_argument("--passes", type=int, default=50, help="coder calls per window")
    ap.add_argument("--max-images", type=int, default=16,
                    help="images per encode_images group when producing the symbols (plan_batches)")
    args = ap.parse_args()
    from tf_image_compression_amd.codec import Codec
    from tf_image_compression_amd.image_codec import ImageCodec
    from tf_image_compression_amd.weights import synthetic_params, SYNTH_MEAN, SYNTH_STD
    out_path = args.out or os.path.join(ROOT, "profiles", f"entropy_ctx_{args.tag}.json")
    codec = Codec(0, synthetic_params(0), SYNTH_MEAN, SYNTH_STD, patch_size=256)
    ic = ImageCodec(codec)
    Q = codec.quan_scale
    code, C_ = int(np.prod(codec.code_shape)), int(codec.code_shape[2])
    images = seeded_images(SIZES, SEED)
    symbols = []
    for g in ic.plan_batches(SIZES, codec.patch_size, args.max_images):
        symbols += ic.encode_images([images[i] for i in g])
    doc = {"tool": "tools/entropy_ctx_probe.py", "tag": args.tag, "seed": SEED, "device": codec.device_info(),
           "model": 0, "patch": codec.patch_size, "weights": "synthetic (He-normal): no trained checkpoint exists",
           "images": len(images), "windows": args.windows, "passes_per_window": args.passes}
    doc["rate"], train = rate(codec, symbols, Q, code, C_, args.segment)
    print(json.dumps({"rate": doc["rate"]}), flush=True)
    stream = np.concatenate([s.reshape(-1) for s in symbols])[:64 * code]
    if stream.size != 64 * code:
        raise SystemExit("the image mix holds fewer than 64 patches")
    doc["time"] = timing(codec, args, np.ascontiguousarray(stream), train, Q, code, C_, args.segment)
    ic.close()
    codec.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(f"wrote {out_path}")


if __name__ == "__main__":
    main()

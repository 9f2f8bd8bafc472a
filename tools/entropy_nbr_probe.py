#!/usr/bin/env python3
"""What do causal-neighbour context tables (the neighbour coder, "TICS" version 3,
csrc/tic_entropy.cpp) save in bytes over per-channel tables, and what do they cost in time beside
the version-2 coder?

Runs on the GPU, in one process, on the symbols model_0 (P = 256, synthetic weights) produces for
the 24-image mix of tools/image_batch_probe.py, with tools/entropy_ctx_probe.py's method.

  bytes   At L = 2048 and L = 4096 the tables are ESTIMATED ON ONE HALF of the images (the
          even-numbered ones) and APPLIED TO THE OTHER HALF, one container per odd-numbered image:
          one table (version 1), one per channel (K = 64) and one per code position (K = 16384)
          (version 2), and K0 = 64 with the W neighbour (192 tables) and with W and N (576 tables)
          (version 3; counted by tic_histogram_nbr_device at the same L, every image one stream,
          and checked against numpy).  Beside the container bytes the ideal code lengths, each
          also as a fraction of the single-table container.
  time    The first 64 patches of the mix's symbols (1 Mi) as one stream at L = 2048, resident on
          the device: one encode call and one decode call for version 2 at K = 64 (the baseline:
          its code is the parent commit's) and version 3 at K0 = 64 with neighbours 1 and 2, every
          arm on a handle of its own so that no window uploads tables.  Every timed window ends in
          a synchronise and is timed with the host clock; a round times the arms one after
          another, and every other round runs them in reverse order.  Every arm's output is
          checked against the host coder first.

The result goes to profiles/entropy_nbr_<tag>.json (or --out).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.entropy_ctx_probe import coded_bytes, context_counts, tables_for, window  # noqa: E402
from tools.image_batch_probe import SEED, SIZES, seeded_images, stats  # noqa: E402


def rows_np(sym, geo, L, K0, neighbours, nsym):
    """The table row of every symbol of one stream (include/tic.h), with numpy index arithmetic."""
    eh, ew, C_ = geo
    sym = np.asarray(sym).astype(np.int64)
    k = np.arange(sym.size, dtype=np.int64)
    p = k % (eh * ew * C_)
    h, w, seg0 = p // (ew * C_), (p // C_) % ew, L * (k // L)
    cls = (2 * sym >= nsym).astype(np.int64)

    def t(j, ok):
        ok = ok & (j >= seg0)
        return np.where(ok, 1 + cls[np.where(ok, j, 0)], 0)

    nb = t(k - C_, w >= 1)
    if neighbours == 2:
        nb = nb + 3 * t(k - ew * C_, h >= 1)
    return (k % K0) * 3 ** neighbours + nb


def neighbour_counts(codec, streams, geo, K0, neighbours, Q, L):
    """[K0, M, Q] histogram of the streams on the device at segment length L, checked against numpy."""
    M = 3 ** neighbours
    codec.entropy_set_tables_nbr(np.tile(np.arange(Q + 1, dtype=np.int64), (K0, M, 1)), geo)
    counts = [s.size for s in streams]
    offs = np.concatenate([[0], np.cumsum(counts)[:-1]])
    d_sym, d_cnt = codec.alloc(sum(counts)), codec.alloc(8 * K0 * M * Q)
    d_sym.upload(np.concatenate(streams))
    codec.memset_device(d_cnt, 0, 8 * K0 * M * Q)
    codec.histogram_nbr_device(d_sym, offs, counts, Q, L, d_cnt)
    got = d_cnt.download((K0, M, Q), np.uint64)
    d_sym.free()
    d_cnt.free()
    want = np.zeros(K0 * M * Q, np.int64)
    for s in streams:
        want += np.bincount(rows_np(s, geo, L, K0, neighbours, Q) * Q + s, minlength=want.size)
    if not np.array_equal(got.reshape(-1), want.astype(np.uint64)):
        raise SystemExit(f"neighbours={neighbours}: tic_histogram_nbr_device differs from numpy")
    return got.astype(np.float64)


def nbr_tables_for(counts, resolution=4096):
    from tf_image_compression_amd.range_coder import nbr_probabilities, symbol_tables_nbr
    return symbol_tables_nbr(nbr_probabilities(counts), resolution=resolution)


def coded_bytes_nbr(codec, streams, tables, geo, L):
    """Container sizes of the streams under 3-D `tables` from one device coder call, checked
    against the host coder on the first stream."""
    from tf_image_compression_amd import entropy
    counts = [s.size for s in streams]
    offs = np.concatenate([[0], np.cumsum(counts)[:-1]])
    d_sym = codec.alloc(sum(counts))
    d_sym.upload(np.concatenate(streams))
    d_scr = codec.alloc(codec.entropy_scratch_bytes(counts, L))
    d_blob = codec.alloc(sum(entropy.bound(n, L, tables) for n in counts))
    d_sizes = codec.alloc(8 * len(counts))
    codec.entropy_set_tables_nbr(tables, geo)
    codec.entropy_encode_nbr_device(d_sym, offs, counts, L, d_scr, d_blob, d_sizes)
    sizes = d_sizes.download((len(counts),), np.uint64).astype(np.int64)
    first = d_blob.download((int(sizes[0]),), np.uint8).tobytes()
    if first != entropy.pack(streams[0], tables, segment=L, geometry=geo):
        raise SystemExit("the device container differs from the host's")
    for b in (d_sym, d_scr, d_blob, d_sizes):
        b.free()
    return [int(v) for v in sizes]


def rate(codec, symbols, Q, geo, L):
    from tf_image_compression_amd.evaluate import estimated_bits, estimated_bits_ctx
    code, C_ = int(np.prod(geo)), geo[2]
    train_streams = [s.reshape(-1) for s in symbols[0::2]]
    test = [s.reshape(-1) for s in symbols[1::2]]
    train, test_all = np.concatenate(train_streams), np.concatenate(test)
    out = {"segment": L, "train_images": len(train_streams), "test_images": len(test),
           "train_symbols": int(train.size), "test_symbols": int(test_all.size),
           "raw_bytes": int(test_all.size // 8) if Q == 2 else int(test_all.size)}
    rows = {}
    for name, K in (("single_table", 1), ("per_channel_K64", C_), ("per_position_K16384", code)):
        table = tables_for(context_counts(codec, train, K, Q))
        on_test = context_counts(codec, test_all, K, Q)
        ideal = estimated_bits(on_test[0], table) if K == 1 else estimated_bits_ctx(on_test, table)
        rows[name] = {"tables": K, "container_bytes": int(sum(coded_bytes(codec, test, table, L))),
                      "ideal_bytes": round(ideal / 8, 1)}
    for nbrs in (1, 2):
        tables = nbr_tables_for(neighbour_counts(codec, train_streams, geo, C_, nbrs, Q, L))
        on_test = neighbour_counts(codec, test, geo, C_, nbrs, Q, L)
        ideal = estimated_bits_ctx(on_test.reshape(-1, Q), tables.reshape(-1, Q + 1))
        rows[f"channel_x_neighbours_{nbrs}"] = {
            "tables": C_ * 3 ** nbrs, "container_bytes": int(sum(coded_bytes_nbr(codec, test, tables, geo, L))),
            "ideal_bytes": round(ideal / 8, 1)}
    base, per_channel = rows["single_table"]["container_bytes"], rows["per_channel_K64"]
    for r in rows.values():
        r["of_single_table"] = round(r["container_bytes"] / base, 4)
        r["ideal_of_single_table"] = round(r["ideal_bytes"] / base, 4)
        r["of_per_channel"] = round(r["container_bytes"] / per_channel["container_bytes"], 4)
        r["ideal_of_per_channel_ideal"] = round(r["ideal_bytes"] / per_channel["ideal_bytes"], 4)
    out["held_out"] = rows
    return out


def timing(args, stream, symbols, Q, geo, L):
    from tf_image_compression_amd import entropy
    from tf_image_compression_amd.codec import Codec
    from tf_image_compression_amd.weights import synthetic_params, SYNTH_MEAN, SYNTH_STD
    n, C_ = stream.size, geo[2]
    train_streams = [s.reshape(-1) for s in symbols[0::2]]
    handles = {name: Codec(0, synthetic_params(0), SYNTH_MEAN, SYNTH_STD, patch_size=256)
               for name in ("version2_K64", "version3_K0_64_neighbours_1", "version3_K0_64_neighbours_2")}
    first = handles["version2_K64"]
    tables = {"version2_K64": tables_for(context_counts(first, np.concatenate(train_streams), C_, Q))}
    for nbrs in (1, 2):
        tables[f"version3_K0_64_neighbours_{nbrs}"] = nbr_tables_for(
            neighbour_counts(first, train_streams, geo, C_, nbrs, Q, L))
    d_sym, d_back = first.alloc(n), first.alloc(n)
    d_sym.upload(stream)
    d_scr = first.alloc(first.entropy_scratch_bytes([n], L))
    d_blob = first.alloc(entropy.bound(n, L) + 16)
    d_size = first.alloc(8)
    arms, sizes, copies = {}, {}, []
    for name, table in tables.items():
        h = handles[name]
        v3 = name.startswith("version3")
        if v3:
            h.entropy_set_tables_nbr(table, geo)
        else:
            h.entropy_set_tables(table)
        enc_fn = h.entropy_encode_nbr_device if v3 else h.entropy_encode_ctx_device
        dec_fn = h.entropy_decode_nbr_device if v3 else h.entropy_decode_ctx_device

        def enc(enc_fn=enc_fn):
            enc_fn(d_sym, [0], [n], L, d_scr, d_blob, d_size)
        enc()
        h.synchronize()
        size = int(d_size.download((1,), np.uint64)[0])
        blob = d_blob.download((size,), np.uint8).tobytes()
        want = entropy.pack(stream, table, segment=L, geometry=geo) if v3 else entropy.pack(stream, table, segment=L)
        if blob != want:
            raise SystemExit(f"{name}: the device container differs from the host's")
        d_in = first.alloc(size)  # a copy of its own, so that encode windows do not rewrite what decode reads
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
        base = res["version2_K64_" + k.rsplit("_", 1)[1]]["median_ms"]
        r["msym_per_s"] = round(n / r["median_ms"] / 1e3, 1)
        r["of_version2_K64"] = round(r["median_ms"] / base, 3)
    print(json.dumps({k: (r["median_ms"], r["spread"], r["of_version2_K64"]) for k, r in res.items()}), flush=True)
    for b in [d_sym, d_back, d_scr, d_blob, d_size] + copies:
        b.free()
    for h in handles.values():
        h.close()
    return {"symbols": int(n), "segment": L, "container_bytes": sizes, "times": res}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--tag", default="pr")
    ap.add_argument("--out", default=None, help="default: profiles/entropy_nbr_<tag>.json")
    ap.add_argument("--windows", type=int, default=9, help="timed windows per arm (rounds over the arms)")
    ap.add_argument("--passes", type=int, default=50, help="coder calls per window")
    ap.add_argument("--max-images", type=int, default=16,
                    help="images per encode_images group when producing the symbols (plan_batches)")
    args = ap.parse_args()
    from tf_image_compression_amd import _lib
    from tf_image_compression_amd.codec import Codec
    from tf_image_compression_amd.image_codec import ImageCodec
    from tf_image_compression_amd.weights import synthetic_params, SYNTH_MEAN, SYNTH_STD
    out_path = args.out or os.path.join(ROOT, "profiles", f"entropy_nbr_{args.tag}.json")
    codec = Codec(0, synthetic_params(0), SYNTH_MEAN, SYNTH_STD, patch_size=256)
    ic = ImageCodec(codec)
    Q = codec.quan_scale
    geo = tuple(int(v) for v in codec.code_shape)
    images = seeded_images(SIZES, SEED)
    symbols = []
    for g in ic.plan_batches(SIZES, codec.patch_size, args.max_images):
        symbols += ic.encode_images([images[i] for i in g])
    doc = {"tool": "tools/entropy_nbr_probe.py", "tag": args.tag, "seed": SEED, "device": codec.device_info(),
           "model": 0, "patch": codec.patch_size, "weights": "synthetic (He-normal): no trained checkpoint exists",
           "images": len(images), "windows": args.windows, "passes_per_window": args.passes,
           "source_digest": _lib.source_digest()}
    doc["rate"] = {}
    for L in (2048, 4096):
        doc["rate"][f"L{L}"] = rate(codec, symbols, Q, geo, L)
        print(json.dumps({f"rate_L{L}": doc["rate"][f"L{L}"]["held_out"]}), flush=True)
    stream = np.concatenate([s.reshape(-1) for s in symbols])[:64 * int(np.prod(geo))]
    if stream.size != 64 * int(np.prod(geo)):
        raise SystemExit("the image mix holds fewer than 64 patches")
    ic.close()
    codec.close()
    doc["time"] = timing(args, np.ascontiguousarray(stream), symbols, Q, geo, 2048)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(f"wrote {out_path}")


if __name__ == "__main__":
    main()

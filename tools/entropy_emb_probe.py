#!/usr/bin/env python3
"""What do tables fitted to every image and carried in its container ("TICA" version 1,
csrc/tic_entropy_emb.cpp) cost and save beside tables from a side file ("TICS" versions 1 to 3)?

Runs on the GPU on the symbols model_0 (P = 256, synthetic weights) produces for the 24-image mix
of tools/image_batch_probe.py, with tools/entropy_nbr_probe.py's method.  Weights and images are
synthetic.

  bytes      At L = 2048 and L = 4096, one container per odd-numbered image (12 images): "TICA"
             under channel, channel + W, channel + W + N and auto (with the share of the table
             blocks and auto's choice per image), against "TICS" under one table, 64 per-channel
             tables, 64 x 3 and 64 x 9 neighbour tables, the tables fitted ON THE OTHER HALF of the
             images (the README's protocol) and ON THE SAME images (pooled).  Every first container
             is checked against the host coder.
  time       The first 64 patches of the mix (1 Mi symbols) as one stream at L = 2048, resident on
             the device, in one process: tic_entropy_encode_emb_device / decode_emb_device at
             channel + W against the version-3 entries at K0 = 64, neighbours 1, and
             tic_histogram_streams_nbr_device alone (the counting pass; the fit and the CRC are two
             launches over 192 rows that only the encode arm contains).  Windows end in a
             synchronise and are timed with the host clock; the arms alternate, every other round
             in reverse order.
  existing   (--parent-lib PATH) tic_entropy_encode / decode {,_ctx,_nbr}_device on the same
             stream, in fresh child processes that alternate between the parent commit's library
             (TIC_LIB) and this tree's; both medians and spreads are recorded.
  end to end ImageCodec.encode_images_to_streams / decode_streams_to_images on the 12 odd-numbered
             images under Adaptive.auto() against version 3 (64 x 3 tables from the other half).

The result goes to profiles/entropy_emb_<tag>.json (or --out).
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.entropy_ctx_probe import coded_bytes, context_counts, tables_for, window  # noqa: E402
from tools.entropy_nbr_probe import coded_bytes_nbr, nbr_tables_for, neighbour_counts  # noqa: E402
from tools.image_batch_probe import SEED, SIZES, seeded_images, stats  # noqa: E402
from tools.region_probe import narrow_binding  # noqa: E402


def new_codec():
    from tf_image_compression_amd.codec import Codec
    from tf_image_compression_amd.weights import synthetic_params, SYNTH_MEAN, SYNTH_STD
    return Codec(0, synthetic_params(0), SYNTH_MEAN, SYNTH_STD, patch_size=256)


def coded_bytes_emb(ic, streams, model, geo, L):
    """(container sizes, table-block bytes, models) of the streams under an Adaptive from the device
    coder (one call per model), the first container checked against the host coder."""
    from tf_image_compression_amd import entropy
    counts = [s.size for s in streams]
    d_sym = ic._buf("symbols", sum(counts))
    d_sym.upload(np.concatenate(streams))
    d_blob, d_sizes, order, bases = ic._entropy_encode_emb(d_sym, counts, model, L)
    sizes = d_sizes.download((len(counts),), np.uint64).astype(np.int64)[np.argsort(order)]
    models = list(ic.last_models)
    at = bases[0][1]
    first = d_blob.view(at).download((int(sizes[order[0]]),), np.uint8).tobytes()
    if first != entropy.pack(streams[order[0]], models[order[0]], segment=L, geometry=geo):
        raise SystemExit("the device container differs from the host's")
    tbytes = [m.K0(geo[2]) * m.M * (m.nsym - 1) * 2 for m in models]
    return [int(v) for v in sizes], tbytes, models


def tics_tables(codec, streams, geo, Q, L):
    """{name: tables} for one table, 64 per-channel tables and the two neighbour models, fitted on `streams`."""
    C_ = geo[2]
    pooled = np.concatenate(streams)
    out = {"v1_single_table": tables_for(context_counts(codec, pooled, 1, Q)),
           "v2_per_channel": tables_for(context_counts(codec, pooled, C_, Q))}
    for nbrs in (1, 2):
        out[f"v3_channel_x_neighbours_{nbrs}"] = nbr_tables_for(neighbour_counts(codec, streams, geo, C_, nbrs, Q, L))
    return out


def rate(codec, ic, symbols, Q, geo, L):
    from tf_image_compression_amd.entropy import Adaptive, is_nbr_table
    train = [s.reshape(-1) for s in symbols[0::2]]
    test = [s.reshape(-1) for s in symbols[1::2]]
    n_test = sum(s.size for s in test)
    out = {"segment": L, "test_images": len(test), "test_symbols": int(n_test),
           "raw_bytes": int(n_test // 8) if Q == 2 else int(n_test)}
    rows = {}
    for where, fit_on in (("other_half", train), ("same_images", test)):
        for name, t in tics_tables(codec, fit_on, geo, Q, L).items():
            sizes = coded_bytes_nbr(codec, test, t, geo, L) if is_nbr_table(t) else coded_bytes(codec, test, t, L)
            rows[f"tics_{name}_tables_from_{where}"] = {"container_bytes": int(sum(sizes))}
    for name, model in (("channel", Adaptive("channel", 0, Q)), ("channel_w", Adaptive("channel", 1, Q)),
                        ("channel_w_n", Adaptive("channel", 2, Q)), ("auto", Adaptive.auto(Q))):
        sizes, tbytes, models = coded_bytes_emb(ic, test, model, geo, L)
        rows[f"tica_{name}"] = {"container_bytes": int(sum(sizes)), "table_block_bytes": int(sum(tbytes)),
                                "table_block_share": round(sum(tbytes) / sum(sizes), 4)}
        if name == "auto":
            rows["tica_auto"]["choice_per_image"] = [f"{m.context}+{m.neighbours}" for m in models]
            rows["tica_auto"]["image_bytes"] = sizes
    base = rows["tics_v1_single_table_tables_from_other_half"]["container_bytes"]
    for r in rows.values():
        r["of_v1_other_half"] = round(r["container_bytes"] / base, 4)
    out["containers"] = rows
    return out


def timing(args, stream, symbols, Q, geo, L):
    from tf_image_compression_amd import entropy
    n, C_ = stream.size, geo[2]
    model = entropy.Adaptive("channel", 1, Q)
    h3, he = new_codec(), new_codec()
    t3 = nbr_tables_for(neighbour_counts(h3, [s.reshape(-1) for s in symbols[0::2]], geo, C_, 1, Q, L))
    h3.entropy_set_tables_nbr(t3, geo)
    d_sym, d_back = h3.alloc(n), h3.alloc(n)
    d_sym.upload(stream)
    d_scr = h3.alloc(he.entropy_emb_scratch_bytes([n], L, model, C_))
    d_blob = h3.alloc(entropy.bound(n, L, model, geo) + 16)
    d_size, d_cnt = h3.alloc(8), h3.alloc(8 * C_ * 3 * Q)
    h3.synchronize()
    arms, sizes, copies = {}, {}, []
    for name, h in (("version3_K0_64_neighbours_1", h3), ("tica_channel_w", he)):
        emb = name.startswith("tica")

        def enc(h=h, emb=emb):
            if emb:
                h.entropy_encode_emb_device(d_sym, [0], [n], L, model, d_scr, d_blob, d_size, geometry=geo)
            else:
                h.entropy_encode_nbr_device(d_sym, [0], [n], L, d_scr, d_blob, d_size)
        enc()
        h.synchronize()
        size = int(d_size.download((1,), np.uint64)[0])
        blob = d_blob.download((size,), np.uint8).tobytes()
        want = entropy.pack(stream, model if emb else t3, segment=L, geometry=geo)
        if blob != want:
            raise SystemExit(f"{name}: the device container differs from the host's")
        d_in = h3.alloc(size)
        d_in.upload(np.frombuffer(blob, np.uint8))
        h3.synchronize()
        copies.append(d_in)

        def dec(h=h, emb=emb, d_in=d_in, size=size):
            if emb:
                h.entropy_decode_emb_device(d_in, [0], [size], [n], model, d_back, [0], d_scr, geometry=geo)
            else:
                h.entropy_decode_nbr_device(d_in, [0], [size], [n], d_back, [0], d_scr)
        dec()
        h.synchronize()
        if not np.array_equal(d_back.download((n,), np.uint8), stream):
            raise SystemExit(f"{name}: the device decoder's symbols differ")
        arms[f"{name}_encode"] = (enc, h)
        arms[f"{name}_decode"] = (dec, h)
        sizes[name] = size

    def hist():
        he.histogram_streams_nbr_device(d_sym, [0], [n], model, L, d_cnt, geometry=geo)
    arms["tica_channel_w_histogram_only"] = (hist, he)
    for fn, h in arms.values():  # warm-up
        for _ in range(5):
            fn()
        h.synchronize()
    ms = {k: [] for k in arms}
    for w in range(args.windows):
        for k in (list(arms) if w % 2 == 0 else list(arms)[::-1]):
            fn, h = arms[k]
            ms[k].append(window(fn, h.synchronize, args.passes))
    res = {k: stats(v) for k, v in ms.items()}
    for k in ("encode", "decode"):
        res[f"tica_channel_w_{k}"]["of_version3"] = round(
            res[f"tica_channel_w_{k}"]["median_ms"] / res[f"version3_K0_64_neighbours_1_{k}"]["median_ms"], 3)
    res["tica_channel_w_histogram_only"]["of_tica_encode"] = round(
        res["tica_channel_w_histogram_only"]["median_ms"] / res["tica_channel_w_encode"]["median_ms"], 3)
    print(json.dumps({k: (r["median_ms"], r["spread"]) for k, r in res.items()}), flush=True)
    for b in [d_sym, d_back, d_scr, d_blob, d_size, d_cnt] + copies:
        b.free()
    h3.close()
    he.close()
    return {"symbols": int(n), "segment": L, "container_bytes": sizes, "times": res}


def existing_arms(args, stream, symbols, Q, geo, L):
    """The entries that were there before, one handle each: a child of --parent-lib runs only this."""
    from tf_image_compression_amd import entropy
    n, C_ = stream.size, geo[2]
    train = [s.reshape(-1) for s in symbols[0::2]]
    first = new_codec()
    tabs = tics_tables(first, train, geo, Q, L)
    del tabs["v3_channel_x_neighbours_2"]
    d_sym, d_back = first.alloc(n), first.alloc(n)
    d_sym.upload(stream)
    d_scr = first.alloc(first.entropy_scratch_bytes([n], L))
    d_blob, d_size = first.alloc(entropy.bound(n, L) + 16), first.alloc(8)
    first.synchronize()
    arms, keep = {}, [first]
    for name, t in tabs.items():
        h = new_codec()
        keep.append(h)
        kind = "nbr" if name.startswith("v3") else "ctx" if name.startswith("v2") else ""
        if kind == "nbr":
            h.entropy_set_tables_nbr(t, geo)
        elif kind == "ctx":
            h.entropy_set_tables(t)
        else:
            h.entropy_set_table(t)
        enc_fn = getattr(h, "entropy_encode_" + (kind + "_" if kind else "") + "device")
        dec_fn = getattr(h, "entropy_decode_" + (kind + "_" if kind else "") + "device")

        def enc(enc_fn=enc_fn):
            enc_fn(d_sym, [0], [n], L, d_scr, d_blob, d_size)
        enc()
        h.synchronize()
        size = int(d_size.download((1,), np.uint64)[0])
        d_in = first.alloc(size)
        d_in.upload(d_blob.download((size,), np.uint8))
        first.synchronize()
        keep.append(d_in)

        def dec(dec_fn=dec_fn, d_in=d_in, size=size):
            dec_fn(d_in, [0], [size], [n], d_back, [0], d_scr)
        dec()
        h.synchronize()
        if not np.array_equal(d_back.download((n,), np.uint8), stream):
            raise SystemExit(f"{name}: the device decoder's symbols differ")
        arms[f"{name}_encode"] = (enc, h)
        arms[f"{name}_decode"] = (dec, h)
    for fn, h in arms.values():
        for _ in range(5):
            fn()
        h.synchronize()
    ms = {k: [] for k in arms}
    for w in range(args.windows):
        for k in (list(arms) if w % 2 == 0 else list(arms)[::-1]):
            fn, h = arms[k]
            ms[k].append(window(fn, h.synchronize, args.passes))
    return {k: stats(v) for k, v in ms.items()}


def run_ab(args):
    """Child processes alternating between the parent's library and this tree's; per arm the
    windows of all children of a side pooled."""
    pooled = {"parent": {}, "this": {}}
    for r in range(args.ab_rounds):
        for side in (("parent", "this") if r % 2 == 0 else ("this", "parent")):
            env = dict(os.environ)
            if side == "parent":
                env["TIC_LIB"] = os.path.abspath(args.parent_lib)
            else:
                env.pop("TIC_LIB", None)
            tmp = os.path.abspath(args.out + f".{side}{r}.tmp")
            subprocess.run([sys.executable, os.path.abspath(__file__), "--existing-only", "--out", tmp, "--windows",
                            str(args.windows), "--passes", str(args.passes)], check=True, env=env, timeout=400)
            with open(tmp) as f:
                for k, v in json.load(f).items():
                    pooled[side].setdefault(k, []).extend(v["windows_ms_per_pass"])
            os.remove(tmp)
    out = {}
    for k in pooled["this"]:
        p, t = stats(pooled["parent"][k]), stats(pooled["this"][k])
        out[k] = {"parent": p, "this": t, "this_of_parent": round(t["median_ms"] / p["median_ms"], 4)}
    return out


def end_to_end(args, ic, images, symbols, Q, geo, L):
    from tf_image_compression_amd.entropy import Adaptive
    test_images, sizes = images[1::2], [im.shape[:2] for im in images[1::2]]
    train = [s.reshape(-1) for s in symbols[0::2]]
    t3 = nbr_tables_for(neighbour_counts(ic.codec, train, geo, geo[2], 1, Q, L))
    res, total = {}, {}
    for name, model in (("version3_64x3_tables_from_other_half", t3), ("tica_auto", Adaptive.auto(Q))):
        streams = ic.encode_images_to_streams(test_images, model, segment=L)
        total[name] = int(sum(map(len, streams)))
        cf = None if name == "tica_auto" else model
        ic.decode_streams_to_images(streams, sizes, cf, post_filter=False)
        enc, dec = [], []
        for _ in range(args.windows):
            enc.append(window(lambda: ic.encode_images_to_streams(test_images, model, segment=L), ic.synchronize, 1))
            dec.append(window(lambda: ic.decode_streams_to_images(streams, sizes, cf, post_filter=False),
                              ic.synchronize, 1))
        res[f"{name}_encode_images_to_streams"] = stats(enc)
        res[f"{name}_decode_streams_to_images"] = stats(dec)
    for k in ("encode_images_to_streams", "decode_streams_to_images"):
        res[f"tica_auto_{k}"]["of_version3"] = round(
            res[f"tica_auto_{k}"]["median_ms"] / res[f"version3_64x3_tables_from_other_half_{k}"]["median_ms"], 3)
    return {"images": len(test_images), "segment": L, "container_bytes": total, "times": res}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--tag", default="pr")
    ap.add_argument("--out", default=None, help="default: profiles/entropy_emb_<tag>.json")
    ap.add_argument("--windows", type=int, default=9, help="timed windows per arm (rounds over the arms)")
    ap.add_argument("--passes", type=int, default=50, help="coder calls per window")
    ap.add_argument("--max-images", type=int, default=16)
    ap.add_argument("--parent-lib", default="", help="libtic.so of the parent commit: alternate the existing entries with it")
    ap.add_argument("--ab-rounds", type=int, default=2, help="child processes per side")
    ap.add_argument("--existing-only", action="store_true", help="only the existing entries' arms (a child of --parent-lib)")
    args = ap.parse_args()
    args.out = args.out or os.path.join(ROOT, "profiles", f"entropy_emb_{args.tag}.json")
    if os.environ.get("TIC_LIB"):
        narrow_binding()
    # the children run before this process opens the GPU
    ab = run_ab(args) if args.parent_lib and not args.existing_only else None
    from tf_image_compression_amd import _lib
    from tf_image_compression_amd.image_codec import ImageCodec
    codec = new_codec()
    ic = ImageCodec(codec)
    Q = codec.quan_scale
    geo = tuple(int(v) for v in codec.code_shape)
    images = seeded_images(SIZES, SEED)
    symbols = []
    for g in ic.plan_batches(SIZES, codec.patch_size, args.max_images):
        symbols += ic.encode_images([images[i] for i in g])
    stream = np.ascontiguousarray(np.concatenate([s.reshape(-1) for s in symbols])[:64 * int(np.prod(geo))])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    if args.existing_only:
        ic.close()
        codec.close()
        with open(args.out, "w") as f:
            json.dump(existing_arms(args, stream, symbols, Q, geo, 2048), f)
        return
    doc = {"tool": "tools/entropy_emb_probe.py", "tag": args.tag, "seed": SEED, "device": codec.device_info(),
           "model": 0, "patch": codec.patch_size, "weights": "synthetic (He-normal): no trained checkpoint exists",
           "images": "synthetic (tools/image_batch_probe.py)", "windows": args.windows, "passes_per_window": args.passes,
           "source_digest": _lib.source_digest(), "rate": {}}
    for L in (2048, 4096):
        doc["rate"][f"L{L}"] = rate(codec, ic, symbols, Q, geo, L)
        print(json.dumps({f"rate_L{L}": {k: v["container_bytes"] for k, v in doc["rate"][f"L{L}"]["containers"].items()}}),
              flush=True)
    doc["end_to_end"] = end_to_end(args, ic, images, symbols, Q, geo, 2048)
    ic.close()
    codec.close()
    doc["time"] = timing(args, stream, symbols, Q, geo, 2048)
    if ab is not None:
        doc["existing_entries_vs_parent"] = ab
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()

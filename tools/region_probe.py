#!/usr/bin/env python3
"""What does decoding a region of a 4K image cost beside decoding the image and cropping, and did
turning the decode kernels into templates slow the existing decoders down?

Runs on one GPU, in one process, with synthetic weights, on a seeded 3840 x 2160 image.

  regions    Two configurations, both at segment length 2048 under one table (version 1):
             model_0 at P = 256 without the post-filter and model_3 at P = 128 with it.  Centred
             regions of 256^2, 512^2 and 1024^2 pixels and the whole image as a region.  Each
             ``ImageCodec.decode_regions`` arm alternates with ``decode_streams_to_images`` plus a
             host crop of the same region: a round times the arms one after another, each in a
             window of its own that ends in a synchronise (both calls do) and is timed with the
             host clock, and every other round runs them in reverse order.  Every region's bytes
             are checked against the crop first.  Beside the times: bytes uploaded and patches
             decoded per arm.
  decoders   (--decoders-only, or as part of --parent-lib) the decode arms of
             tools/entropy_probe.py, entropy_ctx_probe.py and entropy_nbr_probe.py: 1 Mi symbols
             (64 patches of model_0's code) as one stream resident on the device, one decode call
             at L = 2048 under the single table, 64 per-channel tables and 64 x 9 neighbour tables,
             windows as above.  With --parent-lib PATH the same arms run in fresh child processes
             that alternate between that library (TIC_LIB) and this tree's, and both medians are
             recorded: an arm passes when its median is within the parent's median times (1 + the
             larger of the two spreads).

The result goes to profiles/region_<tag>.json (or --out).
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.image_batch_probe import SEED, seeded_images, stats  # noqa: E402

SIZE = (2160, 3840)
CONFIGS = [{"name": "model_0_P256", "model": 0, "patch": 256, "rmbe": False},
           {"name": "model_3_P128_rmbe", "model": 3, "patch": 128, "rmbe": True}]


def narrow_binding():
    """A library of the parent commit lacks the entries this tool's commit added: bind what it
    exports (the decoders measured here are all there)."""
    import ctypes as C
    from tf_image_compression_amd import _lib
    probe = C.CDLL(_lib.LIB_PATH)
    _lib.SIGNATURES = [s for s in _lib.SIGNATURES if hasattr(probe, s[0])]


def window(fn, passes):
    t = time.perf_counter()
    for _ in range(passes):
        fn()
    return (time.perf_counter() - t) * 1e3 / passes


def alternate(arms, windows, passes):
    """{name: stats}: rounds over the arms, every other round in reverse order."""
    for fn in arms.values():  # warm-up
        for _ in range(2):
            fn()
    ms = {k: [] for k in arms}
    for w in range(windows):
        for k in (list(arms) if w % 2 == 0 else list(arms)[::-1]):
            ms[k].append(window(arms[k], passes))
    return {k: stats(v) for k, v in ms.items()}


def table_of(symbols, Q):
    from tf_image_compression_amd.range_coder import symbol_table
    counts = np.bincount(symbols.reshape(-1), minlength=Q).astype(np.float64) + 1
    return symbol_table(counts / counts.sum(), resolution=4096)


def run_regions(cfg, args):
    from tf_image_compression_amd.codec import Codec
    from tf_image_compression_amd.image_codec import ImageCodec
    from tf_image_compression_amd.topology import RMBE_ID
    from tf_image_compression_amd.weights import synthetic_params, SYNTH_MEAN, SYNTH_STD
    H, W = SIZE
    codec = Codec(cfg["model"], synthetic_params(cfg["model"]), SYNTH_MEAN, SYNTH_STD, patch_size=cfg["patch"])
    post = Codec(RMBE_ID, synthetic_params(RMBE_ID), SYNTH_MEAN, SYNTH_STD, patch_size=128) if cfg["rmbe"] else None
    ic = ImageCodec(codec, post)
    image = seeded_images([SIZE], SEED)[0]
    table = table_of(ic.encode_image(image), codec.quan_scale)
    stream = ic.encode_images_to_streams([image], table, segment=args.segment)[0]
    full = ic.decode_streams_to_images([stream], [SIZE], table, post_filter=cfg["rmbe"])[0]
    regions = {f"{s}x{s}": ((H - s) // 2, (W - s) // 2, s, s) for s in (256, 512, 1024)}
    regions["whole"] = (0, 0, H, W)
    out = {"model": cfg["model"], "patch": cfg["patch"], "post_filter": cfg["rmbe"], "segment": args.segment,
           "container_bytes": len(stream), "patches_image": ic.num_patches(H, W), "regions": {}}
    for name, (y, x, h, w) in regions.items():
        got = ic.decode_regions([stream], [SIZE], [(y, x, h, w)], table, post_filter=cfg["rmbe"])[0]
        if not np.array_equal(got, full[y:y + h, x:x + w]):
            raise SystemExit(f"{cfg['name']} {name}: decode_regions differs from the crop of the full decode")
        st = ic.last_region_stats[0]

        def region_arm(r=(y, x, h, w)):
            ic.decode_regions([stream], [SIZE], [r], table, post_filter=cfg["rmbe"])

        def full_arm(r=(y, x, h, w)):
            im = ic.decode_streams_to_images([stream], [SIZE], table, post_filter=cfg["rmbe"])[0]
            np.ascontiguousarray(im[r[0]:r[0] + r[2], r[1]:r[1] + r[3]])

        res = alternate({"decode_regions": region_arm, "full_decode_and_crop": full_arm}, args.windows, args.passes)
        res["decode_regions"].update(bytes_uploaded=st["bytes_uploaded"], patches_decoded=st["patches"])
        res["full_decode_and_crop"].update(bytes_uploaded=len(stream), patches_decoded=st["patches_image"])
        res["region_of_full"] = round(res["decode_regions"]["median_ms"] / res["full_decode_and_crop"]["median_ms"], 4)
        out["regions"][name] = res
        print(json.dumps({cfg["name"]: {name: (res["decode_regions"]["median_ms"], res["decode_regions"]["spread"],
                                                res["full_decode_and_crop"]["median_ms"],
                                                res["full_decode_and_crop"]["spread"], st["patches"],
                                                st["bytes_uploaded"])}}), flush=True)
    ic.close()
    codec.close()
    if post is not None:
        post.close()
    return out


def run_decoders(args):
    """The three existing decode entries on 1 Mi symbols; {arm: stats}."""
    from tf_image_compression_amd import entropy
    from tf_image_compression_amd.codec import Codec
    from tf_image_compression_amd.range_coder import symbol_tables, symbol_tables_nbr
    from tf_image_compression_amd.weights import synthetic_params, SYNTH_MEAN, SYNTH_STD
    codec = Codec(0, synthetic_params(0), SYNTH_MEAN, SYNTH_STD, patch_size=256)
    Q, geo = codec.quan_scale, tuple(int(v) for v in codec.code_shape)
    code, C_ = int(np.prod(geo)), geo[2]
    n, L = 64 * code, args.segment
    rng = np.random.default_rng(SEED)
    bias = rng.random(C_) ** 2 * 0.9 + 0.05  # channels biased one way or the other, as a code's are
    stream = (rng.random((n // C_, C_)) < bias).astype(np.uint8).reshape(-1)
    p1 = np.stack([1 - bias, bias], axis=1)
    tables = {"single_table": table_of(stream, Q), "per_channel_K64": symbol_tables(p1),
              "neighbours_K64x9": symbol_tables_nbr(np.repeat(p1[:, None, :], 9, axis=1))}
    other = Codec(0, synthetic_params(0), SYNTH_MEAN, SYNTH_STD, patch_size=256)  # a handle per context-table set
    codec.entropy_set_table(tables["single_table"])
    codec.entropy_set_tables(tables["per_channel_K64"])
    other.entropy_set_tables_nbr(tables["neighbours_K64x9"], geo)
    d_back = codec.alloc(n)
    d_scr = codec.alloc(codec.entropy_scratch_bytes([n], L))
    arms, keep = {}, []
    for name, table in tables.items():
        h = other if name.startswith("neighbours") else codec
        fn = {"single_table": h.entropy_decode_device, "per_channel_K64": h.entropy_decode_ctx_device,
              "neighbours_K64x9": h.entropy_decode_nbr_device}[name]
        blob = entropy.pack(stream, table, segment=L, geometry=geo if name.startswith("neighbours") else None)
        d_in = codec.alloc(len(blob))
        d_in.upload(np.frombuffer(blob, np.uint8))
        keep.append(d_in)

        def dec(fn=fn, d_in=d_in, size=len(blob), h=h):
            fn(d_in, [0], [size], [n], d_back, [0], d_scr)
            h.synchronize()
        dec()
        if not np.array_equal(d_back.download((n,), np.uint8), stream):
            raise SystemExit(f"{name}: the device decoder's symbols differ")
        arms[name + "_decode"] = dec
    res = alternate(arms, args.windows, args.decoder_passes)
    other.close()
    codec.close()
    return {"symbols": n, "segment": L, "times": res}


def run_ab(args):
    """Fresh child processes, alternating between the parent's library and this tree's."""
    rounds = {"parent": [], "this": []}
    for r in range(args.ab_rounds):
        for side in (("parent", "this") if r % 2 == 0 else ("this", "parent")):
            env = dict(os.environ)
            if side == "parent":
                env["TIC_LIB"] = os.path.abspath(args.parent_lib)
            else:
                env.pop("TIC_LIB", None)
            tmp = os.path.abspath(args.out + f".{side}{r}.tmp")
            subprocess.run([sys.executable, os.path.abspath(__file__), "--decoders-only", "--out", tmp, "--segment",
                            str(args.segment), "--windows", str(args.windows), "--decoder-passes",
                            str(args.decoder_passes)], check=True, env=env, timeout=300)
            with open(tmp) as f:
                rounds[side].append(json.load(f)["decoders"]["times"])
            os.remove(tmp)
    out = {"rounds_per_side": args.ab_rounds, "arms": {}}
    for arm in rounds["this"][0]:
        side = {}
        for s in ("parent", "this"):
            ms = [v for t in rounds[s] for v in t[arm]["windows_ms_per_pass"]]
            side[s] = stats(ms)
        bound = side["parent"]["median_ms"] * (1 + max(side["parent"]["spread"], side["this"]["spread"]))
        out["arms"][arm] = {"parent": side["parent"], "this": side["this"], "bound_ms": round(bound, 4),
                            "passes": bool(side["this"]["median_ms"] <= bound)}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--tag", default="pr")
    ap.add_argument("--out", default=None, help="default: profiles/region_<tag>.json")
    ap.add_argument("--segment", type=int, default=2048)
    ap.add_argument("--windows", type=int, default=9, help="timed windows per arm (rounds over the arms)")
    ap.add_argument("--passes", type=int, default=3, help="calls per window of a region arm")
    ap.add_argument("--decoder-passes", type=int, default=50, help="calls per window of a decoder arm")
    ap.add_argument("--decoders-only", action="store_true", help="only the existing decoders' arms (a child of --parent-lib)")
    ap.add_argument("--parent-lib", default="", help="libtic.so of the parent commit: alternate the decoder arms with it")
    ap.add_argument("--ab-rounds", type=int, default=2, help="child processes per side")
    args = ap.parse_args()
    args.out = args.out or os.path.join(ROOT, "profiles", f"region_{args.tag}.json")
    if os.environ.get("TIC_LIB"):
        narrow_binding()
    from tf_image_compression_amd.codec import Codec
    from tf_image_compression_amd.weights import synthetic_params, SYNTH_MEAN, SYNTH_STD
    with Codec(0, synthetic_params(0), SYNTH_MEAN, SYNTH_STD, patch_size=64) as c:
        device = c.device_info()
    doc = {"tool": "tools/region_probe.py", "tag": args.tag, "seed": SEED, "device": device,
           "weights": "synthetic (He-normal): no trained checkpoint exists", "image": list(SIZE),
           "windows": args.windows}
    if args.decoders_only:
        doc["decoders"] = run_decoders(args)
    else:
        doc["passes_per_window"] = args.passes
        doc["configs"] = {cfg["name"]: run_regions(cfg, args) for cfg in CONFIGS}
        if args.parent_lib:
            doc["existing_decoders_vs_parent"] = run_ab(args)
            print(json.dumps({k: (v["parent"]["median_ms"], v["this"]["median_ms"], v["bound_ms"], v["passes"])
                              for k, v in doc["existing_decoders_vs_parent"]["arms"].items()}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()

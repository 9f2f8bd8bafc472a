#!/usr/bin/env python3
"""Does one patch batch per GROUP of images beat one launch sequence per image?

Runs on the GPU.  A seeded list of mixed-size images (SIZES below: 24 images of 384-2048 px
a side, the sizes the reference is meant for — SURVEY §6) is encoded, decoded, stitched,
(post-filtered) and rounded entirely on the device by two arms:

  per_image   ImageCodec.roundtrip_device once per image (the path encode.py / decode.py take
              with --batch-images 1)
  batched     ImageCodec.encode_images_device + decode_images_device once per group of
              ImageCodec.plan_batches(sizes, P, --max-images, --max-patches)

for model_0 at P = 256 without the post-filter and for model_3 at P = 128 with the rmbe
post-filter.  Both arms read the same resident input arena and nothing synchronises with the
host inside a window.  First both arms run once and their symbols and output bytes are compared
(any difference is an error).  Then, after --warmup untimed passes of each, --windows timed
windows per arm ALTERNATE within this one process (per_image, batched, per_image, ...); a
window is --passes passes over the whole list, ends in a synchronise of both streams and is
timed with the host clock around it.  The result — every window of both arms, median, min,
max and the spread (max - min) / median per arm, and the ratio of the medians — goes to
profiles/image_batch_<tag>.json (or --out).  A difference between the arms smaller than the
spread is not a difference.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (H, W): photo and screen formats from 384 to 2048 px, portrait and landscape, a few sizes that
# are no multiple of any patch size; 36.3 MPix in all.  At P = 256 an image is 4-64 patches (634 in
# all, groups of 396 and 238 under the default caps), at P = 128 it is 12-256 (2352 in all, five
# groups of 426-510)
SIZES = [(512, 768), (1024, 1536), (2048, 1365), (768, 512), (1200, 1800), (384, 512), (1080, 1920), (720, 1280),
         (2048, 2048), (600, 900), (1365, 2048), (480, 640), (1536, 1024), (900, 600), (1600, 1200), (683, 1024),
         (1920, 1080), (512, 512), (1000, 1500), (2000, 1333), (640, 480), (1333, 2000), (800, 1200), (1440, 1920)]
CONFIGS = [{"name": "model0_p256", "model": 0, "patch": 256, "rmbe": False},
           {"name": "model3_p128_rmbe", "model": 3, "patch": 128, "rmbe": True}]
SEED = 20240229


def seeded_images(sizes, seed):
    """Smooth structure plus noise, so neither the symbols nor the rounding are degenerate."""
    out = []
    for k, (H, W) in enumerate(sizes):
        r = np.random.default_rng(seed + k)
        yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
        base = 128 + 70 * np.sin(xx / (31.0 + k))[..., None] * np.cos(yy / (47.0 - k))[..., None]
        noise = r.integers(-24, 25, (H, W, 3), dtype=np.int16)
        out.append(np.clip(base + noise, 0, 255).astype(np.uint8))
    return out


def stats(ms):
    med = float(np.median(ms))
    return {"windows_ms_per_pass": [round(float(v), 4) for v in ms], "median_ms": round(med, 4),
            "min_ms": round(float(min(ms)), 4), "max_ms": round(float(max(ms)), 4),
            "spread": round(float(max(ms) - min(ms)) / med, 4)}


def run_config(cfg, args):
    from tf_image_compression_amd.codec import Codec
    from tf_image_compression_amd.image_codec import ImageCodec
    from tf_image_compression_amd.topology import RMBE_ID
    from tf_image_compression_amd.weights import synthetic_params, SYNTH_MEAN, SYNTH_STD
    M, P = cfg["model"], cfg["patch"]
    codec = Codec(M, synthetic_params(M), SYNTH_MEAN, SYNTH_STD, patch_size=P)
    post = Codec(RMBE_ID, synthetic_params(RMBE_ID), SYNTH_MEAN, SYNTH_STD, patch_size=128) if cfg["rmbe"] else None
    ic = ImageCodec(codec, post)
    sizes = SIZES[:args.images] if args.images else SIZES
    images = seeded_images(sizes, SEED)
    offs, total = ic.packed_offsets(sizes)
    counts = [ic.num_patches(H, W) for H, W in sizes]
    code = int(np.prod(codec.code_shape))
    sym_off = [int(v) * code for v in np.concatenate([[0], np.cumsum(counts)[:-1]])]
    groups = ic.plan_batches(sizes, P, args.max_images, args.max_patches)

    d_in = codec.alloc(total)
    d_in.upload(np.concatenate([im.reshape(-1) for im in images]))
    d_sym = {arm: codec.alloc(sum(counts) * code) for arm in ("per_image", "batched")}
    d_out = {arm: codec.alloc(total) for arm in ("per_image", "batched")}

    def per_image():
        for i, (H, W) in enumerate(sizes):
            ic.roundtrip_device(d_in.view(offs[i]), H, W, d_sym["per_image"].view(sym_off[i]),
                                d_out["per_image"].view(offs[i]), post_filter=cfg["rmbe"])

    def batched():
        for g in groups:
            gs, go = [sizes[i] for i in g], [offs[i] for i in g]
            sv = d_sym["batched"].view(sym_off[g[0]])
            ic.encode_images_device(d_in, go, gs, sv)
            ic.decode_images_device(sv, go, gs, d_out["batched"], post_filter=cfg["rmbe"])

    arms = {"per_image": per_image, "batched": batched}

    # 1. equal bytes first
    got = {}
    for arm, fn in arms.items():
        fn()
        ic.synchronize()
        got[arm] = (d_sym[arm].download((sum(counts) * code,), np.uint8), d_out[arm].download((total,), np.uint8))
    if not np.array_equal(got["per_image"][0], got["batched"][0]):
        raise SystemExit(f"{cfg['name']}: the arms' symbols differ")
    if not np.array_equal(got["per_image"][1], got["batched"][1]):
        raise SystemExit(f"{cfg['name']}: the arms' output bytes differ")

    # 2. warm-up, then alternating timed windows
    for fn in arms.values():
        for _ in range(args.warmup):
            fn()
        ic.synchronize()
    ms = {arm: [] for arm in arms}
    for _ in range(args.windows):
        for arm, fn in arms.items():
            ic.synchronize()
            t = time.perf_counter()
            for _ in range(args.passes):
                fn()
            ic.synchronize()
            ms[arm].append((time.perf_counter() - t) * 1e3 / args.passes)
    res = {arm: stats(v) for arm, v in ms.items()}
    a, b = res["per_image"], res["batched"]
    ratio = a["median_ms"] / b["median_ms"]
    gain = abs(a["median_ms"] - b["median_ms"]) / a["median_ms"]
    out = {"config": cfg, "device": codec.device_info(), "tuning": codec.tuning_source,
           "post_tuning": post.tuning_source if post else None,
           "images": len(sizes), "sizes": sizes, "pixels": int(sum(H * W for H, W in sizes)),
           "patches": int(sum(counts)), "patches_per_image": counts,
           "groups": groups, "patches_per_group": [int(sum(counts[i] for i in g)) for g in groups],
           "max_images": args.max_images, "max_patches": args.max_patches,
           "outputs_equal": True, "warmup_passes": args.warmup, "passes_per_window": args.passes,
           "per_image": a, "batched": b, "per_image_over_batched": round(ratio, 4),
           "difference_exceeds_spread": bool(gain > max(a["spread"], b["spread"])),
           "mpix_per_s": {arm: round(sum(H * W for H, W in sizes) / res[arm]["median_ms"] / 1e3, 1) for arm in res}}
    ic.close()
    codec.close()
    if post:
        post.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--tag", default="probe")
    ap.add_argument("--out", default=None, help="default: profiles/image_batch_<tag>.json")
    ap.add_argument("--windows", type=int, default=7, help="timed windows per arm")
    ap.add_argument("--passes", type=int, default=20, help="passes over the image list per window")
    ap.add_argument("--warmup", type=int, default=2, help="untimed passes per arm")
    ap.add_argument("--max-images", type=int, default=16)
    ap.add_argument("--max-patches", type=int, default=512)
    ap.add_argument("--images", type=int, default=0, help="only the first N images of the list (0: all)")
    ap.add_argument("--config", choices=[c["name"] for c in CONFIGS], action="append",
                    help="default: every configuration")
    args = ap.parse_args()
    out_path = args.out or os.path.join(ROOT, "profiles", f"image_batch_{args.tag}.json")
    doc = {"tool": "tools/image_batch_probe.py", "tag": args.tag, "seed": SEED, "results": []}
    for cfg in CONFIGS:
        if args.config and cfg["name"] not in args.config:
            continue
        r = run_config(cfg, args)
        doc["results"].append(r)
        print(json.dumps({k: r[k] for k in ("config", "patches", "patches_per_group", "per_image_over_batched",
                                            "difference_exceeds_spread", "mpix_per_s")}), flush=True)
        print(json.dumps({"per_image": r["per_image"], "batched": r["batched"]}), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    print(f"wrote {out_path}")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Rate / distortion of a model over an image list without writing a file: every image goes
image -> gfx950 encoder -> symbols -> decoder (-> rmbe post-filter) -> uint8 image on the
device (image_codec.ImageCodec.evaluate_images), where its PSNR (processing_utils/
evaluate.py:10-32), its MS-SSIM (the CLIC challenge's second measure) and its symbol
histogram are computed; the histogram and the range coder's table (encode.py:77-86) give the
code length the ``.encoded`` file would have to within a few bytes.

Flags as encode.py (``-m -g -p -v``, ``--norm``, ``--dist``, ``--synthetic-weights``,
``--batch-images N``) plus ``--rmbe PARAMS`` / ``--rmbe-norm`` as decode.py and ``--json OUT``.
One line per image (PSNR, MS-SSIM, MS-SSIM in dB = -10 log10(1 - ms), estimated bpp), then the
dataset line: evaluate()'s PSNR formula over all images (sum of SSE over sum of dims), the mean
MS-SSIM (images with a side below 161 have none and are left out) and total estimated bits over
total pixels.  Without a distribution file the rate columns are omitted.  ``--entropy device``
(with ``--segment L``) also range-codes every image's symbols on the GPU into a segmented
stream (tf_image_compression_amd/entropy.py) and prints its real size, ``coded_bytes``, and the
bpp from it.  With ``--entropy device`` a 2-D ``--dist`` array ([K, Q] per-context probabilities,
get_encoded_distribution.py --context) gives both under the context coder: the estimate from
the per-context histogram, ``coded_bytes`` from version-2 containers.  A 3-D array ([K0, M, Q],
get_encoded_distribution.py --context --neighbours) does the same under the causal-neighbour coder
(version-3 containers; the estimate uses the rows the coder uses at ``--segment``).
"""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from tf_image_compression_amd import utils  # noqa: E402
from tf_image_compression_amd.config import load_config  # noqa: E402


def my_parse_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("-m", "--model_num", type=str, choices=["0", "1", "2", "3"], required=True,
                   help="Determine which model to use")
    p.add_argument("-g", "--gpu_num", type=str, choices=[str(i) for i in range(8)], required=True,
                   help="Determine which gpu to use")
    p.add_argument("-p", "--params_file", type=str, default="", help="File for model parameters (.npz)")
    p.add_argument("-v", "--data_list", type=str, default="data_info/tiny_valid_data_list.txt",
                   help="File for data_list")
    p.add_argument("--norm", type=str, default="data_info/channel_normalization_params.npz")
    p.add_argument("--dist", type=str, default="data_info/distribution_info_{}.npy")
    p.add_argument("--synthetic-weights", action="store_true")
    p.add_argument("--rmbe", type=str, default="", help="rmbe post-filter weights .npz (submit/2)")
    p.add_argument("--rmbe-norm", type=str, default="rmbe/channel_normalization_params.npz")
    p.add_argument("--batch-images", type=int, default=1, metavar="N",
                   help="evaluate up to N images (at most 512 patches) as one patch batch; same values as 1")
    p.add_argument("--json", type=str, default="", metavar="OUT", help="also write the results as JSON")
    p.add_argument("--entropy", choices=["host", "device"], default="host",
                   help="device: also range-code every image's symbols on the GPU (segmented streams) and "
                        "print the real coded_bytes and the bpp from them beside the estimate")
    p.add_argument("--segment", type=int, default=2048, metavar="L",
                   help="symbols per segment of --entropy device (multiple of 4, 4..16384)")
    p.add_argument("--tables", choices=["dist", "adaptive", "auto"], default="dist",
                   help="with --entropy device: dist (the default) codes under the --dist array; adaptive fits the "
                        "tables of --context / --neighbours to every image and counts them in coded_bytes (no --dist "
                        "is read, no estimate is printed); auto also chooses the model per image")
    p.add_argument("--context", choices=["none", "channel"], default="channel")
    p.add_argument("--neighbours", type=int, choices=[0, 1, 2], default=0)
    args = p.parse_args(argv)
    if args.batch_images < 1:
        p.error("--batch-images must be at least 1")
    if args.tables != "dist" and args.entropy != "device":
        p.error("--tables adaptive / auto needs --entropy device")
    if args.entropy == "host":
        from tf_image_compression_amd.range_coder import dist_is_ctx
        if dist_is_ctx(args.dist.format(args.model_num)):
            p.error(f"{args.dist.format(args.model_num)} holds per-context probabilities (2-D or 3-D): use --entropy device")
    return args


def load_model(args, config):
    import encode
    return encode.load_model(args, config)


def msssim_db(ms: float) -> float:
    """-10 log10(1 - ms); inf for identical images, nan where there is no MS-SSIM."""
    if math.isnan(ms):
        return float("nan")
    return float("inf") if ms >= 1.0 else -10.0 * math.log10(1.0 - ms)


def dataset_summary(rows) -> dict:
    """evaluate()'s dataset PSNR (sum of SSE over sum of dims), the mean MS-SSIM over the images
    that have one, and total estimated bits over total pixels (None without a table)."""
    from tf_image_compression_amd.evaluate import mse2psnr
    sse = sum(r["sse"] for r in rows)
    dims = sum(r["height"] * r["width"] * 3 for r in rows)
    pixels = sum(r["height"] * r["width"] for r in rows)
    ms = [r["msssim"] for r in rows if not math.isnan(r["msssim"])]
    with np.errstate(divide="ignore"):
        psnr = float(mse2psnr(np.float64(sse) / dims)) if dims else float("nan")
    mean_ms = float(np.mean(ms)) if ms else float("nan")
    bits = None if any(r["est_bits"] is None for r in rows) else float(sum(r["est_bits"] for r in rows))
    out = {"n_images": len(rows), "n_msssim": len(ms), "pixels": pixels, "sse": sse, "psnr": psnr,
           "msssim": mean_ms, "msssim_db": msssim_db(mean_ms), "est_bits": bits,
           "est_bpp": None if bits is None or not pixels else bits / pixels}
    if rows and all("coded_bytes" in r for r in rows):  # --entropy device
        out["coded_bytes"] = sum(r["coded_bytes"] for r in rows)
        out["coded_bpp"] = 8.0 * out["coded_bytes"] / pixels if pixels else None
    return out


def _line(name, r) -> str:
    rate = "" if r["est_bpp"] is None else f"  est_bpp {r['est_bpp']:.4f}"
    if r.get("coded_bytes") is not None:
        rate += f"  coded_bytes {r['coded_bytes']}  coded_bpp {r['coded_bpp']:.4f}"
    return f"{name}: psnr {r['psnr']:.4f}  msssim {r['msssim']:.6f}  msssim_db {r['msssim_db']:.3f}{rate}"


def run(model, args) -> dict:
    config = load_config(args.model_num)
    P, Q = config["patch_size"], config["quan_scale"]
    codec = model.codec(P, Q)
    cum_freq = None
    dist = args.dist.format(args.model_num)
    if getattr(args, "tables", "dist") != "dist":
        from tf_image_compression_amd.entropy import Adaptive
        cum_freq = Adaptive.auto(Q) if args.tables == "auto" else Adaptive(args.context, args.neighbours, Q)
    elif os.path.exists(dist):
        from tf_image_compression_amd.range_coder import dist_table
        cum_freq = dist_table(np.load(dist, allow_pickle=False), resolution=config["resolution"])
        if np.ndim(cum_freq) >= 2 and getattr(args, "entropy", "host") != "device":
            raise ValueError(f"{dist} holds per-context probabilities (2-D or 3-D): use --entropy device")
    else:
        print(f"no symbol distribution at {dist}: the estimated rate is omitted")
    post = None
    if args.rmbe:
        from tf_image_compression_amd.rmbe import RmbeFilter
        post = RmbeFilter.from_files(args.rmbe, args.rmbe_norm, device=codec.device)
    from tf_image_compression_amd.image_codec import ImageCodec
    ic = ImageCodec(codec, post.codec if post is not None else None)
    image_paths = utils.read_image_list(args.data_list)
    sizes = [utils.image_size(p) for p in image_paths]
    rows = []
    segment = None
    if getattr(args, "entropy", "host") == "device":
        if cum_freq is None:
            raise ValueError(f"--entropy device needs the symbol distribution ({dist})")
        segment = args.segment
    for group in ic.plan_batches(sizes, P, args.batch_images):
        images = [utils.imread(image_paths[i]) for i in group]
        for i, image, r in zip(group, images, ic.evaluate_images(images, post_filter=post is not None,
                                                                 cum_freq=cum_freq, entropy_segment=segment)):
            H, W = image.shape[:2]
            row = {"path": image_paths[i], "height": H, "width": W, "sse": r["sse"], "psnr": r["psnr"],
                   "msssim": r["msssim"], "msssim_db": msssim_db(r["msssim"]), "n_symbols": r["n_symbols"],
                   "counts": [int(v) for v in r["counts"]], "est_bits": r["est_bits"],
                   "est_bpp": None if r["est_bits"] is None else r["est_bits"] / (H * W)}
            if "coded_bytes" in r:
                row["coded_bytes"] = r["coded_bytes"]
                row["coded_bpp"] = 8.0 * r["coded_bytes"] / (H * W)
            rows.append(row)
            print(_line(image_paths[i], row))
    ic.close()
    result = {"model": int(args.model_num), "patch_size": P, "quan_scale": Q, "post_filter": post is not None,
              "images": rows, "dataset": dataset_summary(rows)}
    print(_line("dataset", result["dataset"]))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)
    return result


if __name__ == "__main__":
    args = my_parse_args()
    cfg = load_config(args.model_num)
    run(load_model(args, cfg), args)

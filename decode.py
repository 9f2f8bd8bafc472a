#!/usr/bin/env python3
"""Drop-in for the reference's decode.py (same flags, paths and file naming):
``.encoded`` dir -> range decoder -> symbols [-1, eh, ew, ec] -> gfx950 decoder ->
stitched, cropped uint8 PNG ``<stem>.png`` (decode.py:143-264), with the optional
submit/2 block-effect post-filter (``--rmbe``, submit/2/decoder.py:184).

Reference: /root/reference/decode.py:20-76 (flags), :79-140 (range decoding, file-name
parsing), :143-264 (uncompress).  ``-g`` accepts -1..7 (-1 is accepted for
compatibility; there is no CPU path, so it maps to device 0 with a warning).
``--entropy device`` reads the segmented-stream containers ``encode.py --entropy device``
writes and decodes them on the GPU, a group of files per call.
``--region X,Y,W,H`` (with ``--entropy device``) writes only that rectangle of every image,
``<stem>_x{X}_y{Y}_{W}x{H}.png``, decoded from the patches and the container segments it needs.
"""
import argparse
import os
import sys
import time
from pathlib import Path

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from tf_image_compression_amd import utils  # noqa: E402
from tf_image_compression_amd.config import load_config  # noqa: E402


def my_parse_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("-m", "--model_num", type=str, choices=["0", "1", "2", "3"], required=True)
    p.add_argument("-g", "--gpu_num", type=str, choices=[str(i) for i in range(-1, 8)], required=True)
    p.add_argument("-d", "--debug_mode", type=str, choices=["on", "off"], default="off")
    p.add_argument("-p", "--params_file", type=str, default="")
    p.add_argument("-i", "--input_dir", type=str, default="model_{}/encoded_data")
    p.add_argument("-o", "--output_dir", type=str, default="model_{}/recons_data")
    p.add_argument("--norm", type=str, default="data_info/channel_normalization_params.npz")
    p.add_argument("--dist", type=str, default="data_info/distribution_info_{}.npy")
    p.add_argument("--synthetic-weights", action="store_true")
    p.add_argument("--raw", action="store_true", help="symbols stored bit-packed (encode.py --raw)")
    p.add_argument("--rmbe", type=str, default="", help="rmbe post-filter weights .npz (submit/2)")
    p.add_argument("--rmbe-norm", type=str, default="rmbe/channel_normalization_params.npz")
    p.add_argument("--batch-images", type=int, default=1, metavar="N",
                   help="decode up to N files (at most 512 patches) as one patch batch; same files and "
                        "output as 1, the default (one image per launch sequence)")
    p.add_argument("--entropy", choices=["host", "device"], default="host",
                   help="host: single-stream files (the default); device: segmented-stream containers "
                        "(encode.py --entropy device), range-decoded on the GPU")
    p.add_argument("--region", type=str, default="", metavar="X,Y,W,H",
                   help="decode only the W x H rectangle at column X, row Y of every image (needs --entropy "
                        "device): the bytes of that crop of the full decode, written as "
                        "<stem>_x{X}_y{Y}_{W}x{H}.png")
    args = p.parse_args(argv)
    if args.region:
        if args.raw:
            p.error("--region reads segmented streams: it cannot be combined with --raw")
        if args.entropy != "device":
            p.error("--region needs --entropy device: the single-stream host coder cannot start inside a stream")
        try:
            x, y, w, h = (int(v) for v in args.region.split(","))
        except ValueError:
            p.error(f"--region {args.region!r} is not X,Y,W,H (four integers)")
        if x < 0 or y < 0 or w <= 0 or h <= 0:
            p.error(f"--region {args.region!r}: X and Y must not be negative, W and H must be positive")
        args.region = (x, y, w, h)
    else:
        args.region = None
    if args.entropy == "device" and args.raw:
        p.error("--raw files hold no entropy-coded stream: it cannot be combined with --entropy device")
    if args.entropy == "host" and not args.raw:
        from tf_image_compression_amd.range_coder import dist_is_ctx
        if dist_is_ctx(args.dist.format(args.model_num)):
            p.error(f"{args.dist.format(args.model_num)} holds per-context probabilities (2-D or 3-D): the single-stream "
                    "host coder has one table; use --entropy device")
    return args


def get_img_info(filename, config):
    """decode.py:104-115: '<stem>@_@h_w_c@_@len_H_W.encoded' -> (len, H, W)."""
    info = filename.replace(".encoded", "").split(config["name_sep"])[-1]
    seq_len, height, width = (int(v) for v in info.split("_"))
    return seq_len, height, width


def get_recons_image_path(filename, args, config):
    stem = filename.replace(".encoded", "").split(config["name_sep"])[0]
    if getattr(args, "region", None):
        x, y, w, h = args.region
        stem += f"_x{x}_y{y}_{w}x{h}"
    return str(Path(args.output_dir.format(args.model_num)) / (stem + ".png"))


def get_encoded_shape(input_dir, config):
    """decode.py:130-140: the shape comes from the FIRST file name in the directory."""
    sample = sorted(f for f in os.listdir(input_dir) if f.endswith(".encoded"))[0]
    eh, ew, ec = (int(v) for v in sample.split(config["name_sep"])[1].split("_"))
    return eh, ew, ec


def apply_range_decoder(seq_len, path, cum_freq):
    from tf_image_compression_amd.range_coder import RangeDecoder
    dec = RangeDecoder(path)
    out = dec.decode_array(seq_len, cum_freq)
    dec.close()
    return out


def is_adaptive_file(path):
    """True when the file starts with the magic of a container that carries its own tables."""
    from tf_image_compression_amd import entropy
    with open(path, "rb") as f:
        return entropy.is_adaptive(f.read(4))


def check_container_version(path, stream, cum_freq, args, code_shape=None):
    """The coder follows the file's version byte: version 1 was coded under one table (a 1-D
    --dist array), version 2 under per-context tables (a 2-D one), version 3 under context x
    neighbour tables (a 3-D one) for a code geometry that must be the model's (``code_shape``)."""
    from tf_image_compression_amd import entropy
    if not entropy.is_container(stream):
        return  # entropy.parse names what it is not
    version, ctx = entropy.container_version(stream), entropy.is_ctx_table(cum_freq)
    nbr = entropy.is_nbr_table(cum_freq)
    dist = args.dist.format(args.model_num)
    if version == 3 and not nbr:
        raise ValueError(f"{path} is a version-3 (neighbour) stream, but {dist} does not hold 3-D tables: pass "
                         "the 3-D distribution it was encoded with")
    if version != 3 and nbr:
        raise ValueError(f"{path} is a version-{version} stream, but {dist} holds 3-D context x neighbour "
                         "tables: pass the distribution it was encoded with")
    if version == 3:
        geometry = entropy.parse_nbr(stream)[4]
        if code_shape is not None and tuple(geometry) != tuple(int(v) for v in code_shape):
            raise ValueError(f"{path} was coded for the code geometry {geometry}, the model's at this patch size "
                             f"is {tuple(int(v) for v in code_shape)}")
        return
    if version == 2 and not ctx:
        raise ValueError(f"{path} is a version-2 (context) stream, but {dist} holds one 1-D table: pass the "
                         "2-D per-context distribution it was encoded with")
    if version == 1 and ctx:
        raise ValueError(f"{path} is a version-1 (single-table) stream, but {dist} holds 2-D per-context "
                         "tables: pass the 1-D distribution it was encoded with")


def load_model(args, config):
    from tf_image_compression_amd.weights import load_normalization, synthetic_params
    import importlib
    model = importlib.import_module(f"tf_image_compression_amd.model_{args.model_num}.model")
    params = synthetic_params(int(args.model_num)) if args.synthetic_weights else utils.restore_params(args)
    mean, std = load_normalization(args.norm if os.path.exists(args.norm) else None)
    dev = int(args.gpu_num)
    if dev < 0:
        print("warning: -g -1 (TF-CPU) has no equivalent here; using HIP device 0", file=sys.stderr)
        dev = 0
    model.restore(params, mean, std, device=dev)
    return model


def uncompress(model, args):
    print(args)
    config = load_config(args.model_num)
    print(config)
    P, Q = config["patch_size"], config["quan_scale"]
    input_dir = args.input_dir.format(args.model_num)
    eh, ew, ec = get_encoded_shape(input_dir, config)
    codec = model.codec(P, Q)
    if tuple(codec.code_shape) != (eh, ew, ec):
        raise ValueError(f"encoded shape {(eh, ew, ec)} does not match model_{args.model_num} "
                         f"at patch {P}: {codec.code_shape}")
    cum_freq = None
    names = [f for f in sorted(os.listdir(input_dir)) if f.endswith(".encoded")]
    # files that carry their own tables ("TICA", encode.py --tables adaptive / auto) need no --dist
    adaptive = {f: args.entropy == "device" and is_adaptive_file(str(Path(input_dir) / f)) for f in names}
    if not args.raw and not (names and all(adaptive.values())):
        from tf_image_compression_amd.range_coder import dist_table
        cum_freq = dist_table(np.load(args.dist.format(args.model_num), allow_pickle=False),
                              resolution=config["resolution"])
    post = None
    if args.rmbe:
        from tf_image_compression_amd.rmbe import RmbeFilter
        post = RmbeFilter.from_files(args.rmbe, args.rmbe_norm, device=codec.device)
    from tf_image_compression_amd.image_codec import ImageCodec
    ic = ImageCodec(codec, post.codec if post is not None else None)
    out_dir = args.output_dir.format(args.model_num)
    os.makedirs(out_dir, exist_ok=True)
    t0 = time.time()

    def read_symbols(filename):
        path = str(Path(input_dir) / filename)
        seq_len, height, width = get_img_info(filename, config)
        if args.raw:
            raw = np.fromfile(path, np.uint8)
            seq = np.unpackbits(raw)[:seq_len] if Q == 2 else raw[:seq_len]
        else:
            from tf_image_compression_amd import entropy
            with open(path, "rb") as f:
                if entropy.is_container(f.read(4)):
                    raise ValueError(f"{path} is a segmented stream (encode.py --entropy device): "
                                     "decode it with --entropy device")
            seq = apply_range_decoder(seq_len, path, cum_freq)
        return seq.astype(np.uint8).reshape(-1, eh, ew, ec), height, width   # decode.py:204-208

    def store(filename, recons):
        out_path = get_recons_image_path(filename, args, config)
        print(f"recons_image_path: {out_path}")
        utils.imsave(out_path, recons)

    filenames = [f for f in sorted(os.listdir(input_dir)) if f.endswith(".encoded")]
    if args.batch_images < 1:
        raise ValueError("--batch-images must be at least 1")
    if args.entropy == "device":
        # groups as for --batch-images; every container is validated on the host (tic_rcseg_parse),
        # then the group's containers are decoded on the GPU in one call
        sizes = [get_img_info(f, config)[1:] for f in filenames]
        region = None
        if args.region:
            x, y, w, h = args.region
            region = (y, x, h, w)
            for f, (height, width) in zip(filenames, sizes):
                if y + h > height or x + w > width:
                    raise ValueError(f"{Path(input_dir) / f}: the image is {width} x {height}, it does not contain "
                                     f"the region {w} x {h} at ({x}, {y})")
        # a group's files that carry their tables and those coded under --dist are decoded apart
        groups = []
        for group in ic.plan_batches(sizes, P, args.batch_images):
            groups += [part for part in ([i for i in group if adaptive[filenames[i]]],
                                         [i for i in group if not adaptive[filenames[i]]]) if part]
        for group in groups:
            streams = [(Path(input_dir) / filenames[i]).read_bytes() for i in group]
            for i, stream in zip(group, streams):
                if not adaptive[filenames[i]]:
                    check_container_version(str(Path(input_dir) / filenames[i]), stream, cum_freq, args,
                                            ic.codec.code_shape)
            if region:
                images = ic.decode_regions(streams, [sizes[i] for i in group], [region] * len(group), cum_freq,
                                           post_filter=post is not None)
            else:
                images = ic.decode_streams_to_images(streams, [sizes[i] for i in group], cum_freq,
                                                     post_filter=post is not None)
            for i, recons in zip(group, images):
                store(filenames[i], recons)
    elif args.batch_images == 1:
        for filename in filenames:
            symbols, height, width = read_symbols(filename)
            # decode -> concat_patches -> (rmbe) -> np.around, all on the GPU
            store(filename, ic.decode_image(symbols, height, width, post_filter=post is not None))
    else:
        # groups of consecutive files as one patch batch each (ImageCodec.plan_batches)
        sizes = [get_img_info(f, config)[1:] for f in filenames]
        for group in ic.plan_batches(sizes, P, args.batch_images):
            symbols = [read_symbols(filenames[i])[0] for i in group]
            images = ic.decode_images(symbols, [sizes[i] for i in group], post_filter=post is not None)
            for i, recons in zip(group, images):
                store(filenames[i], recons)
    if args.debug_mode == "on":
        print(f"decode time {time.time() - t0:.3f}s")


if __name__ == "__main__":
    args = my_parse_args()
    cfg = load_config(args.model_num)
    uncompress(load_model(args, cfg), args)

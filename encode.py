#!/usr/bin/env python3
"""Drop-in for the reference's encode.py (same flags, paths, file naming and symbol
order): image list -> reflect-padded 256^2 (or 128^2) patches -> gfx950 encoder ->
uint8 symbols (patch-major, then h, w, C) -> range coder -> ``.encoded`` files named
``<stem>@_@{eh}_{ew}_{ec}@_@{len}_{H}_{W}.encoded`` (encode.py:102-122).

Reference: /root/reference/encode.py:17-73 (flags), :76-97 (range coding), :125-212
(compress).  Differences: ``-g`` picks a HIP device (0..7) instead of setting
CUDA_VISIBLE_DEVICES; ``-p`` names the TF checkpoint prefix (read by tf_checkpoint.py) or an
.npz of the same variables; the image is uploaded once and reflect-tiled on the GPU
(image_codec.py), and all its patches go through the encoder in one call instead of
``sess.run`` batches of 64.  Extra optional flags: ``--norm`` (channel statistics
npz), ``--dist`` (symbol distribution npy), ``--synthetic-weights`` (seeded weights when
no checkpoint exists), ``--raw`` (store bit-packed symbols, no entropy coding),
``--batch-images N`` (N > 1: consecutive images share one patch batch, image_codec.py),
``--entropy device`` (the symbols stay on the GPU and are range-coded there, one segment of
``--segment L`` symbols per lane; each file then holds one segmented-stream container,
tf_image_compression_amd/entropy.py, which ``decode.py --entropy device`` reads;
``--tables adaptive`` or ``auto`` fits the tables to every image and stores them in its file, so
no ``--dist`` is read here or by the decoder).  With
``--entropy device`` a 2-D ``--dist`` array ([K, Q] per-context probabilities,
get_encoded_distribution.py --context) codes symbol k of an image under table k mod K and writes
version-2 containers.  A 3-D array ([K0, M, Q], get_encoded_distribution.py --context --neighbours)
also conditions every symbol on its causal neighbours' classes and writes version-3 containers; the
geometry they carry is the model's code shape at the patch size.
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
    p.add_argument("-m", "--model_num", type=str, choices=["0", "1", "2", "3"], required=True,
                   help="Determine which model to use")
    p.add_argument("-g", "--gpu_num", type=str, choices=[str(i) for i in range(8)], required=True,
                   help="Determine which gpu to use")
    p.add_argument("-d", "--debug_mode", type=str, choices=["on", "off"], default="off")
    p.add_argument("-p", "--params_file", type=str, default="", help="File for model parameters (.npz)")
    p.add_argument("-v", "--data_list", type=str, default="data_info/tiny_valid_data_list.txt",
                   help="File for data_list")
    p.add_argument("-o", "--output_dir", type=str, default="model_{}/encoded_data",
                   help="Directory for output compressed data")
    p.add_argument("--norm", type=str, default="data_info/channel_normalization_params.npz")
    p.add_argument("--dist", type=str, default="data_info/distribution_info_{}.npy")
    p.add_argument("--synthetic-weights", action="store_true")
    p.add_argument("--raw", action="store_true", help="bit-pack symbols instead of range coding")
    p.add_argument("--batch-images", type=int, default=1, metavar="N",
                   help="encode up to N images (at most 512 patches) as one patch batch; same files and "
                        "output as 1, the default (one image per launch sequence)")
    p.add_argument("--entropy", choices=["host", "device"], default="host",
                   help="host: the single-stream range coder (the default, the reference's format); device: "
                        "range-code on the GPU into one segmented-stream container per file")
    p.add_argument("--segment", type=int, default=2048, metavar="L",
                   help="symbols per segment of --entropy device (multiple of 4, 4..16384)")
    p.add_argument("--tables", choices=["dist", "adaptive", "auto"], default="dist",
                   help="with --entropy device: dist (the default) codes under the --dist array; adaptive fits the "
                        "tables of --context / --neighbours to every image and writes them into its file, which "
                        "then decodes without any --dist; auto also chooses the model per image")
    p.add_argument("--context", choices=["none", "channel"], default="channel",
                   help="--tables adaptive: one table (none) or one per channel of the code (channel)")
    p.add_argument("--neighbours", type=int, choices=[0, 1, 2], default=0,
                   help="--tables adaptive: also condition on the class of the W neighbour (1) or of W and N (2)")
    args = p.parse_args(argv)
    if args.entropy == "device" and args.raw:
        p.error("--raw stores symbols without entropy coding: it cannot be combined with --entropy device")
    if args.tables != "dist" and args.entropy != "device":
        p.error("--tables adaptive / auto writes segmented-stream containers: it needs --entropy device")
    if args.entropy == "host" and not args.raw:
        from tf_image_compression_amd.range_coder import dist_is_ctx
        if dist_is_ctx(args.dist.format(args.model_num)):
            p.error(f"{args.dist.format(args.model_num)} holds per-context probabilities (2-D or 3-D): the single-stream "
                    "host coder has one table; use --entropy device")
    return args


def symbol_table(args, config):
    """encode.py:77-86: prob -> prob*resolution+1 -> renormalise -> prob_to_cum_freq."""
    from tf_image_compression_amd.range_coder import dist_table as table
    path = args.dist.format(args.model_num)
    prob = np.load(path, allow_pickle=False)
    return table(prob, resolution=config["resolution"])


def apply_range_encoder(seq_data, encodepath, args, config, cum_freq):
    from tf_image_compression_amd.range_coder import RangeEncoder
    enc = RangeEncoder(encodepath)
    enc.encode(seq_data, cum_freq)
    enc.close()


def get_encodepath(image_path, image, seq_len, args, config, encoded_patches_shape):
    encoded_save_dir = args.output_dir.format(args.model_num)
    stem = image_path.split("/")[-1].replace(".png", "")
    height, width, _ = image.shape
    eh, ew, ec = encoded_patches_shape
    sep = config["name_sep"]
    info = sep + f"{eh}_{ew}_{ec}" + sep + f"{seq_len}_{height}_{width}"
    return str(Path(encoded_save_dir) / stem) + info + ".encoded"


def load_model(args, config):
    from tf_image_compression_amd.weights import load_normalization, synthetic_params
    import importlib
    model = importlib.import_module(f"tf_image_compression_amd.model_{args.model_num}.model")
    if args.synthetic_weights:
        params = synthetic_params(int(args.model_num))
    else:
        params = utils.restore_params(args)
    mean, std = load_normalization(args.norm if os.path.exists(args.norm) else None)
    model.restore(params, mean, std, device=int(args.gpu_num))
    return model


def compress(model, args):
    print(args)
    config = load_config(args.model_num)
    print(config)
    P, Q = config["patch_size"], config["quan_scale"]
    codec = model.codec(P, Q)
    from tf_image_compression_amd.image_codec import ImageCodec
    ic = ImageCodec(codec)
    if args.tables != "dist":  # no --dist file is read: the tables come from every image itself
        from tf_image_compression_amd.entropy import Adaptive
        cum_freq = Adaptive.auto(Q) if args.tables == "auto" else Adaptive(args.context, args.neighbours, Q)
    else:
        cum_freq = None if args.raw else symbol_table(args, config)
    out_dir = args.output_dir.format(args.model_num)
    os.makedirs(out_dir, exist_ok=True)
    t0 = time.time()

    def store(image_path, image, symbols):
        shape = symbols.shape[1:]
        seq = symbols.reshape(-1)                            # encode.py:175-182 order
        encodepath = get_encodepath(image_path, image, seq.size, args, config, shape)
        if args.raw:
            np.packbits(seq.astype(np.uint8) & 1).tofile(encodepath) if Q == 2 else seq.tofile(encodepath)
        else:
            apply_range_encoder(seq, encodepath, args, config, cum_freq)
        print(f"encodepath: {encodepath}")

    image_paths = utils.read_image_list(args.data_list)
    if args.batch_images < 1:
        raise ValueError("--batch-images must be at least 1")
    if args.entropy == "device":
        # groups as for --batch-images; the symbols of a group are coded on the GPU in one call
        sizes = [utils.image_size(p) for p in image_paths]
        shape = tuple(codec.code_shape)
        for group in ic.plan_batches(sizes, P, args.batch_images):
            images = [utils.imread(image_paths[i]) for i in group]
            streams = ic.encode_images_to_streams(images, cum_freq, segment=args.segment)
            for i, image, stream in zip(group, images, streams):
                seq_len = ic.num_patches(*image.shape[:2]) * int(np.prod(shape))
                encodepath = get_encodepath(image_paths[i], image, seq_len, args, config, shape)
                with open(encodepath, "wb") as f:
                    f.write(stream)
                print(f"encodepath: {encodepath}")
    elif args.batch_images == 1:
        for image_path in image_paths:
            image = utils.imread(image_path)
            store(image_path, image, ic.encode_image(image))     # [n, eh, ew, ec] uint8
    else:
        # groups of consecutive images as one patch batch each (ImageCodec.plan_batches)
        sizes = [utils.image_size(p) for p in image_paths]
        for group in ic.plan_batches(sizes, P, args.batch_images):
            images = [utils.imread(image_paths[i]) for i in group]
            for i, image, symbols in zip(group, images, ic.encode_images(images)):
                store(image_paths[i], image, symbols)
    if args.debug_mode == "on":
        print(f"encode time {time.time() - t0:.3f}s")


if __name__ == "__main__":
    args = my_parse_args()
    cfg = load_config(args.model_num)
    compress(load_model(args, cfg), args)

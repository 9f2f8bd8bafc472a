#!/usr/bin/env python3
"""Drop-in for the reference's get_encoded_distribution.py: the symbol distribution of the
encoder over a list of training patches, saved as ``distribution_info_{N}.npy`` (the
probability table encode.py / decode.py turn into the range coder's cum_freq).

Reference: /root/reference/get_encoded_distribution.py:17-83 (flags), :86-134
(get_distribution: batches of 64 patches -> encoder -> np.histogram(out, range(Q+1))
summed -> prob = freq / sum(freq) -> np.save).  Here each batch is uploaded once,
encoded on the GPU and histogrammed on the GPU (tic_histogram_device accumulates into one
device counter array); the counts come back once at the end.  ``-f/--model_file`` is
accepted for flag compatibility (the model is chosen by ``-m``).  Extra optional flags as
encode.py: ``--norm``, ``--synthetic-weights``.

``--context channel`` / ``--context position`` also estimate a periodic context model (the
reference computes the per-position probabilities, cal_encoded_distribution.py:113-160
``seq_prob``, but its coder could not use them): one histogram per channel (K = C) or per code
position (K = eh * ew * C) through tic_histogram_ctx_device, saved as a ``[K, Q]`` probability
array to ``--context-output`` (``data_info/distribution_ctx_{}.npy``), which ``encode.py`` /
``decode.py --entropy device --dist`` take.  The 1-D file is written as without the flag.

``--neighbours 1|2`` (with ``--context``) estimates the causal-neighbour model instead ("TICS"
version 3, include/tic.h): every context is split by the class of the symbol's W neighbour (1) or
of its W and N neighbours (2), counted by tic_histogram_nbr_device at segment length ``--segment``
(a neighbour outside the symbol's segment does not count, so the counts depend on it; every batch
is one stream).  The ``[K0, M, Q]`` probabilities go to ``--context-output``; a context never seen
backs off to its row's distribution summed over the neighbour classes, so no entry is zero.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from tf_image_compression_amd import utils  # noqa: E402
from tf_image_compression_amd.config import load_config  # noqa: E402

BATCH = 64  # get_encoded_distribution.py:98


def my_parse_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("-m", "--model_num", type=str, choices=["0", "1", "2", "3"], required=True,
                   help="Determine which model to use")
    p.add_argument("-g", "--gpu_num", type=str, choices=[str(i) for i in range(8)], required=True,
                   help="Determine which gpu to use")
    p.add_argument("-d", "--debug_mode", type=str, choices=["on", "off"], default="off")
    p.add_argument("-p", "--params_file", type=str, default="", help="File for model parameters")
    p.add_argument("-v", "--data_list", type=str, default="data_info/train_data_patch_list_{}.txt",
                   help="File for data_list ({} = patch size)")
    p.add_argument("-f", "--model_file", type=str, default="model_{}/params_for_test/model.py",
                   help="accepted for compatibility; the model is selected by -m")
    p.add_argument("-o", "--output_file", type=str, default="data_info/distribution_info_{}.npy",
                   help="File to keep encoded distribution info")
    p.add_argument("--norm", type=str, default="data_info/channel_normalization_params.npz")
    p.add_argument("--synthetic-weights", action="store_true")
    p.add_argument("--context", choices=["none", "channel", "position"], default="none",
                   help="also save per-context probabilities [K, Q]: one table per channel (K = C) or per "
                        "code position (K = eh * ew * C)")
    p.add_argument("--context-output", type=str, default="data_info/distribution_ctx_{}.npy",
                   help="File for the per-context probabilities of --context")
    p.add_argument("--neighbours", type=int, choices=[1, 2], default=0,
                   help="with --context: condition every context on the W (1) or the W and N (2) neighbour's "
                        "class and save [K0, M, Q] probabilities instead")
    p.add_argument("--segment", type=int, default=2048,
                   help="segment length the neighbour contexts are counted at (--neighbours)")
    a = p.parse_args(argv)
    if a.neighbours and a.context == "none":
        p.error("--neighbours needs --context channel or --context position")
    return a


def context_count(context, code_shape) -> int:
    """K of --context for a code of shape (eh, ew, C): symbols are ordered patch, h, w, C."""
    eh, ew, ec = (int(v) for v in code_shape)
    return {"none": 1, "channel": ec, "position": eh * ew * ec}[context]


def load_model(args):
    import importlib
    from tf_image_compression_amd.weights import load_normalization, synthetic_params
    model = importlib.import_module(f"tf_image_compression_amd.model_{args.model_num}.model")
    params = synthetic_params(int(args.model_num)) if args.synthetic_weights else utils.restore_params(args)
    mean, std = load_normalization(args.norm if os.path.exists(args.norm) else None)
    model.restore(params, mean, std, device=int(args.gpu_num))
    return model


def encoded_frequencies(codec, patch_iter, Q):
    """Sum over batches of np.histogram(encoder(batch), range(Q+1))[0], on the GPU."""
    return encoded_context_frequencies(codec, patch_iter, Q, None)[0]


def encoded_context_frequencies(codec, patch_iter, Q, K):
    """(freq [Q], ctx_freq [K, Q]): ``encoded_frequencies`` and, in the same pass, the counts of
    symbol i of a batch in row i mod K (a batch holds whole patches, so it starts at context 0
    for K = C and K = eh * ew * C).  ``K = None``: ctx_freq is None."""
    P = codec.patch_size
    eh, ew, ec = codec.code_shape
    d_in = codec.alloc(BATCH * P * P * 3)
    d_sym = codec.alloc(BATCH * eh * ew * ec)
    d_cnt = codec.alloc(8 * Q)
    codec.memset_device(d_cnt, 0, 8 * Q)
    d_ctx = None
    if K is not None:
        d_ctx = codec.alloc(8 * K * Q)
        codec.memset_device(d_ctx, 0, 8 * K * Q)
    for batch in patch_iter:
        x = np.ascontiguousarray(batch, np.uint8).reshape(-1, P, P, 3)
        d_in.upload(x)
        codec.encode_device(d_in, x.shape[0], d_sym)
        codec.histogram_device(d_sym, x.shape[0] * eh * ew * ec, Q, d_cnt)
        if d_ctx is not None:
            codec.histogram_ctx_device(d_sym, x.shape[0] * eh * ew * ec, Q, K, d_ctx)
    freq = d_cnt.download((Q,), np.uint64).astype(np.float64)
    ctx_freq = None if d_ctx is None else d_ctx.download((K, Q), np.uint64).astype(np.float64)
    for b in (d_in, d_sym, d_cnt) + (() if d_ctx is None else (d_ctx,)):
        b.free()
    return freq, ctx_freq


def encoded_neighbour_frequencies(codec, patch_iter, Q, K0, neighbours, segment):
    """(freq [Q], nbr_freq [K0, M, Q]): ``encoded_frequencies`` and, in the same pass, the counts of
    every symbol in row (k mod K0) * M + nb, each batch one stream coded at ``segment``."""
    P = codec.patch_size
    eh, ew, ec = codec.code_shape
    M = 3 ** neighbours
    # the histogram entry takes K0, M and the geometry from the tables set: any valid ones do
    flat = np.tile(np.arange(Q + 1, dtype=np.int64), (K0, M, 1))
    codec.entropy_set_tables_nbr(flat)
    d_in = codec.alloc(BATCH * P * P * 3)
    d_sym = codec.alloc(BATCH * eh * ew * ec)
    d_cnt = codec.alloc(8 * Q)
    d_nbr = codec.alloc(8 * K0 * M * Q)
    codec.memset_device(d_cnt, 0, 8 * Q)
    codec.memset_device(d_nbr, 0, 8 * K0 * M * Q)
    for batch in patch_iter:
        x = np.ascontiguousarray(batch, np.uint8).reshape(-1, P, P, 3)
        d_in.upload(x)
        codec.encode_device(d_in, x.shape[0], d_sym)
        n = x.shape[0] * eh * ew * ec
        codec.histogram_device(d_sym, n, Q, d_cnt)
        codec.histogram_nbr_device(d_sym, [0], [n], Q, segment, d_nbr)
    freq = d_cnt.download((Q,), np.uint64).astype(np.float64)
    nbr_freq = d_nbr.download((K0, M, Q), np.uint64).astype(np.float64)
    for b in (d_in, d_sym, d_cnt, d_nbr):
        b.free()
    return freq, nbr_freq


def save_neighbour_distribution(path, counts):
    """The ``[K0, M, Q]`` probabilities of a neighbour histogram (range_coder.nbr_probabilities:
    unseen contexts back off, no entry is zero) to ``path``."""
    from tf_image_compression_amd.range_coder import nbr_probabilities
    prob = nbr_probabilities(counts)
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    np.save(path, prob)
    return prob


def patch_batches(paths, P):
    for s in range(0, len(paths), BATCH):
        batch = [utils.imread(p) for p in paths[s:s + BATCH]]
        for p, b in zip(paths[s:s + BATCH], batch):
            if b.shape != (P, P, 3):
                raise ValueError(f"{p}: expected a {P}x{P} RGB patch, got {b.shape}")
        yield np.stack(batch)


def get_distribution(model, args):
    print(args)
    config = load_config(args.model_num)
    print(config)
    P, Q = config["patch_size"], config["quan_scale"]
    codec = model.codec(P, Q)
    paths = utils.read_image_list(args.data_list.format(P))
    context = getattr(args, "context", "none")
    neighbours = getattr(args, "neighbours", 0)
    if neighbours:
        K = context_count(context, codec.code_shape)
        freq, nbr_freq = encoded_neighbour_frequencies(codec, patch_batches(paths, P), Q, K, neighbours, args.segment)
    elif context == "none":
        freq = encoded_frequencies(codec, patch_batches(paths, P), Q)
    else:
        K = context_count(context, codec.code_shape)
        freq, ctx_freq = encoded_context_frequencies(codec, patch_batches(paths, P), Q, K)
    prob = freq / sum(freq)  # get_encoded_distribution.py:129
    print(prob)
    out = args.output_file.format(args.model_num)
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    np.save(out, prob)
    if neighbours:
        ctx_out = args.context_output.format(args.model_num)
        save_neighbour_distribution(ctx_out, nbr_freq)
        print(f"{context} contexts x {3 ** neighbours} neighbour classes at segment {args.segment}: "
              f"[{K}, {3 ** neighbours}, {Q}] probabilities -> {ctx_out}")
    elif context != "none":
        # a context no patch reached keeps the global distribution (symbol_table adds 1 to every
        # frequency anyway, so no table entry is zero)
        rows = ctx_freq.sum(axis=1, keepdims=True)
        ctx_prob = np.where(rows > 0, ctx_freq / np.maximum(rows, 1), prob[None, :])
        ctx_out = args.context_output.format(args.model_num)
        os.makedirs(os.path.dirname(ctx_out) or ".", exist_ok=True)
        np.save(ctx_out, ctx_prob)
        print(f"{context} contexts: [{K}, {Q}] probabilities -> {ctx_out}")
    return prob


if __name__ == "__main__":
    a = my_parse_args()
    get_distribution(load_model(a), a)

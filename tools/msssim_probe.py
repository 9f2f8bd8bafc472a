#!/usr/bin/env python3
"""What does MS-SSIM on the device cost beside the round trip it measures?

Runs on the GPU.  Two workloads, both resident in HBM before anything is timed:

  mix24   the 24 seeded images of 384-2048 px of tools/image_batch_probe.py (36.3 MPix)
  uhd     one 3840x2160 pair

and two arms on each, in this one process, on the codec's stream:

  roundtrip   model_0 at P = 256: ImageCodec.encode_images_device + decode_images_device per
              group of ImageCodec.plan_batches (the batched round trip the evaluation measures)
  msssim      ONE tic_msssim_images_device call over the originals and the round trip's output

First the round trip runs once, so that the second arena holds real reconstructions, and the
MS-SSIM call runs twice: its 30 doubles per image must be bit-identical.  Then, after --warmup
untimed passes of each arm, --windows timed windows per arm ALTERNATE; a window is --passes
passes between two device events on the stream and ends in a synchronise; its time is the
events' elapsed time over the passes.  Every window, median, min, max and spread
(max - min) / median per arm go to profiles/msssim_<tag>.json (or --out), with the bytes and
floating-point operations the MS-SSIM kernels need by their shapes (counted below) over the
median time.  A difference smaller than the spread is not a difference.
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.image_batch_probe import SIZES, SEED, seeded_images, stats  # noqa: E402

WORKLOADS = {"mix24": SIZES, "uhd": [(2160, 3840)]}


def hip_runtime():
    """The HIP runtime libtic.so is bound to (already mapped once libtic is loaded)."""
    with open("/proc/self/maps") as f:
        paths = {ln.split()[-1] for ln in f if "libamdhip64" in ln}
    if len(paths) != 1:
        raise SystemExit(f"expected one mapped libamdhip64, found {sorted(paths)}")
    hip = C.CDLL(paths.pop())
    hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    hip.hipEventDestroy.argtypes = [C.c_void_p]
    return hip


def hip_ok(rc, what):
    if rc != 0:
        raise SystemExit(f"{what} failed with HIP error {rc}")


def shape_counts(sizes):
    """Bytes and floating-point operations of one MS-SSIM call by its shapes.

    Bytes (compulsory traffic, halo re-reads not counted): the moment kernel of scale 0 and the
    pool kernel of scale 0 each read both uint8 images once; every float plane of scales 1-4
    is written once, read once by its moment kernel and (scales 1-3) once by the next pool.
    Operations per valid position and channel, separable form: the horizontal pass forms 5
    moments from 11 taps (3 products + 5 fused multiply-adds = 13 per tap), the vertical pass 5
    fused multiply-adds per tap, the per-position formulas about 20; a fused multiply-add
    counts 2.  The horizontal pass is counted once per position (its halo rows are overhead)."""
    nbytes = flops = 0
    for H, W in sizes:
        h, w = H, W
        for j in range(5):
            if j == 0:
                nbytes += 2 * (2 * h * w * 3)
            else:
                nbytes += 2 * h * w * 3 * 4 * (3 if j < 4 else 2)
            flops += 3 * (h - 10) * (w - 10) * (11 * 13 + 11 * 10 + 20)
            h, w = (h + 1) // 2, (w + 1) // 2
    return nbytes, flops


def run_workload(name, sizes, codec, ic, hip, stream, args):
    from tf_image_compression_amd.evaluate import msssim_from_sums
    P = codec.patch_size
    images = seeded_images(sizes, SEED)
    offs, total = ic.packed_offsets(sizes)
    counts = [ic.num_patches(H, W) for H, W in sizes]
    code = int(np.prod(codec.code_shape))
    sym_off = [int(v) * code for v in np.concatenate([[0], np.cumsum(counts)[:-1]])]
    groups = ic.plan_batches(sizes, P, args.max_images, args.max_patches)
    d_in, d_out, d_sym = codec.alloc(total), codec.alloc(total), codec.alloc(sum(counts) * code)
    d_in.upload(np.concatenate([im.reshape(-1) for im in images]))
    scratch = codec.msssim_scratch_bytes(sizes)
    d_scr, d_ms = codec.alloc(scratch), codec.alloc(len(sizes) * 240)

    def roundtrip():
        for g in groups:
            gs, go = [sizes[i] for i in g], [offs[i] for i in g]
            sv = d_sym.view(sym_off[g[0]])
            ic.encode_images_device(d_in, go, gs, sv)
            ic.decode_images_device(sv, go, gs, d_out, post_filter=False)

    def msssim():
        codec.msssim_images_device(d_in, d_out, offs, sizes, d_scr, d_ms)

    arms = {"roundtrip": roundtrip, "msssim": msssim}
    roundtrip()
    msssim()
    first = d_ms.download((len(sizes), 5, 3, 2), np.float64)
    msssim()
    if not np.array_equal(first, d_ms.download((len(sizes), 5, 3, 2), np.float64)):
        raise SystemExit(f"{name}: two MS-SSIM calls differ")
    values = [msssim_from_sums(s, H, W) for s, (H, W) in zip(first, sizes)]

    for fn in arms.values():
        for _ in range(args.warmup):
            fn()
        codec.synchronize()
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        hip_ok(hip.hipEventCreate(C.byref(e)), "hipEventCreate")
    ms = {arm: [] for arm in arms}
    for _ in range(args.windows):
        for arm, fn in arms.items():
            codec.synchronize()
            hip_ok(hip.hipEventRecord(ev[0], stream), "hipEventRecord")
            for _ in range(args.passes):
                fn()
            hip_ok(hip.hipEventRecord(ev[1], stream), "hipEventRecord")
            hip_ok(hip.hipEventSynchronize(ev[1]), "hipEventSynchronize")
            codec.synchronize()
            t = C.c_float()
            hip_ok(hip.hipEventElapsedTime(C.byref(t), ev[0], ev[1]), "hipEventElapsedTime")
            ms[arm].append(t.value / args.passes)
    for e in ev:
        hip.hipEventDestroy(e)
    res = {arm: stats(v) for arm, v in ms.items()}
    nbytes, flops = shape_counts(sizes)
    t = res["msssim"]["median_ms"] * 1e-3
    pixels = int(sum(H * W for H, W in sizes))
    out = {"workload": name, "images": len(sizes), "sizes": sizes, "pixels": pixels, "patches": int(sum(counts)),
           "groups": len(groups), "scratch_bytes": scratch, "msssim_min": round(min(values), 6),
           "msssim_max": round(max(values), 6), "repeat_bit_identical": True,
           "warmup_passes": args.warmup, "passes_per_window": args.passes,
           "roundtrip": res["roundtrip"], "msssim": res["msssim"],
           "msssim_over_roundtrip": round(res["msssim"]["median_ms"] / res["roundtrip"]["median_ms"], 4),
           "msssim_shape_bytes": nbytes, "msssim_shape_flops": flops,
           "msssim_gbytes_per_s": round(nbytes / t / 1e9, 1), "msssim_gflops_per_s": round(flops / t / 1e9, 1),
           "msssim_mpix_per_s": round(pixels / t / 1e6, 1)}
    for d in (d_in, d_out, d_sym, d_scr, d_ms):
        d.free()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--tag", default="probe")
    ap.add_argument("--out", default=None, help="default: profiles/msssim_<tag>.json")
    ap.add_argument("--windows", type=int, default=7, help="timed windows per arm")
    ap.add_argument("--passes", type=int, default=20, help="passes per window")
    ap.add_argument("--warmup", type=int, default=3, help="untimed passes per arm")
    ap.add_argument("--max-images", type=int, default=16)
    ap.add_argument("--max-patches", type=int, default=512)
    ap.add_argument("--workload", choices=sorted(WORKLOADS), action="append", help="default: both")
    args = ap.parse_args()
    from tf_image_compression_amd.codec import Codec
    from tf_image_compression_amd.image_codec import ImageCodec
    from tf_image_compression_amd.weights import synthetic_params, SYNTH_MEAN, SYNTH_STD
    codec = Codec(0, synthetic_params(0), SYNTH_MEAN, SYNTH_STD, patch_size=256)
    hip = hip_runtime()
    stream = codec.stream_ptr()
    codec.stream_external(False)  # only the events below go to the stream, and they order nothing
    ic = ImageCodec(codec)
    out_path = args.out or os.path.join(ROOT, "profiles", f"msssim_{args.tag}.json")
    doc = {"tool": "tools/msssim_probe.py", "tag": args.tag, "seed": SEED, "device": codec.device_info(),
           "tuning": codec.tuning_source, "config": {"model": 0, "patch": 256, "rmbe": False}, "results": []}
    for name in args.workload or sorted(WORKLOADS):
        r = run_workload(name, WORKLOADS[name], codec, ic, hip, stream, args)
        doc["results"].append(r)
        print(json.dumps({k: r[k] for k in ("workload", "pixels", "msssim_over_roundtrip", "msssim_gbytes_per_s",
                                            "msssim_gflops_per_s", "msssim_mpix_per_s")}), flush=True)
        print(json.dumps({"roundtrip": r["roundtrip"], "msssim": r["msssim"]}), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    ic.close()
    codec.close()
    print(f"wrote {out_path}")


if __name__ == "__main__":
    main()

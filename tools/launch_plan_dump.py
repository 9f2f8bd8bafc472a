"""Records which kernels a handle launches, and what a codec step computes, for the grid of
option sets below: the fixture of tests/test_gpu_launch_plan.py (tests/golden/launch_plan.json.gz).

    python tools/launch_plan_dump.py OUT.json.gz

Uses the public Codec API only (set_option, tuning_import, layer_kernels, codec_kernels,
layer_variants, codec_device / encode / decode), so the same file runs on any checkout that
has that API: record the fixture on the commit whose behaviour is to be kept, replay it (the
test) on the commit under test.  Needs a GPU (a handle needs a device); the plan part launches
no kernel.

Fixture (gzip-compressed JSON; `python -m gzip -dc FILE` prints it): {"lists": [every distinct per-layer list once], "plans": [distinct (layer_kernels,
codec_kernels, layer_variants) as three indices into lists], "grid": [{model, patch, ns, idx}],
"extra": [...], "tunings": [...], "digests": [...]} where every idx list holds one plan index
per (option set, n) in the order option_sets() x ns gives.
"""
import glob
import gzip
import hashlib
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

RMBE, CH128 = 100, 128
NS = (1, 3, 64)
PATCHES = (32, 64, 128, 256)
MODELS = (0, 1, 2, 3, RMBE, CH128)
GRID = [(m, P, NS) for m in MODELS for P in PATCHES]
DEFAULTS = {"chain_wh": 2, "chain_x": -1, "chain_j": -1, "streams": 2, "chunk": 256}


def option_sets():
    """Every option set of one (model, patch), in a fixed order; each sets every option."""
    for s1, s2, f01, ft, ch in itertools.product((0, 1, 2), (0, 1), (0, 1), (0, 1), (0, 1)):
        base = dict(DEFAULTS, s1_form=s1, s2_form=s2, fuse01=f01, fuse_tail=ft, chain=ch)
        yield base
        if ch == 1 and s1 == 1:
            for wh, x, j, st in itertools.product((1, 2), (0, 1, 2), (0, 1), (1, 2, 4)):
                yield dict(base, chain_wh=wh, chain_x=x, chain_j=j, streams=st)


# model 0 at P = 256: a chunk past chain_end's 32-bit hand-off bound (chunk * 2 * 2 * 16 KB
# > 2^31), and the environment overrides the plan and the names read
EXTRA = [
    {"options": {"chunk": 40000}, "env": {}},
    {"options": {}, "env": {"TIC_ENC01_VARIANT": "1"}},
    {"options": {}, "env": {"TIC_DEC10_VARIANT": "5"}},
    {"options": {}, "env": {"TIC_TEST_CHAIN_CUT": "3"}},
]
EXTRA_BASE = dict(DEFAULTS, s1_form=1, s2_form=1, fuse01=1, fuse_tail=1, chain=1, chain_x=2, chain_j=1)

# bit digests: model 0, 3 patches on 2 lanes (launches of 2 and 1), P = 256 (a 16x16 trunk: four
# 8x8 regions, the smallest chain that hands borders over); one option set per launch kind
_D = dict(DEFAULTS, fuse01=0, fuse_tail=0, s1_form=0, s2_form=0, chain=0, chain_x=0, chain_j=0)
DIGEST_CASES = [
    ("per_layer", 0, dict(_D)),
    ("fused_pairs", 0, dict(_D, fuse01=1, fuse_tail=1)),
    ("chain", 0, dict(_D, fuse01=1, fuse_tail=1, s1_form=1, chain=1)),
    ("chain_x2_pwino", 0, dict(_D, fuse01=1, fuse_tail=1, s1_form=1, chain=1, chain_x=2, s2_form=1)),
    ("chain_j", 0, dict(_D, fuse01=1, fuse_tail=1, s1_form=1, chain=1, chain_x=1, chain_j=1)),
    ("wino4", 0, dict(_D, fuse01=1, fuse_tail=1, s1_form=2)),
    ("model3_chain", 3, dict(_D, fuse01=1, fuse_tail=1, s1_form=1, chain=1, chain_x=1)),
]
DIGEST_P, DIGEST_N = 256, 3


def make_codec(model, P):
    from tf_image_compression_amd.codec import Codec
    from tf_image_compression_amd.weights import SYNTH_MEAN, SYNTH_STD, synthetic_params
    return Codec(model, synthetic_params(model, 0), SYNTH_MEAN, SYNTH_STD, patch_size=P, quan_scale=2, device=0,
                 tuning="none")


def apply_options(codec, opts):
    for k, v in opts.items():
        codec.set_option(k, v)


def plan(codec, n):
    """What the handle would launch for lane batch n; an entry that fails reports its error."""
    out = []
    for fn in (codec.layer_kernels, codec.codec_kernels, codec.layer_variants):
        try:
            out.append([list(v) if isinstance(v, tuple) else v for v in fn(n)])
        except Exception as e:  # noqa: BLE001 (recorded, and must stay the same error)
            out.append("error: " + str(e))
    return out


class PlanTable:
    """Distinct plans, each three indices into the distinct per-layer lists."""

    def __init__(self):
        self.lists, self.plans, self.index = [], [], {}

    def _add(self, table, item):
        key = (id(table), json.dumps(item))
        if key not in self.index:
            self.index[key] = len(table)
            table.append(item)
        return self.index[key]

    def add(self, p):
        return self._add(self.plans, [self._add(self.lists, part) for part in p])


def grid_plans(model, P, ns):
    """One plan per (option set, n) in option_sets() x ns order, or the error of tic_create."""
    try:
        codec = make_codec(model, P)
    except Exception as e:  # noqa: BLE001
        return "error: " + str(e)
    with codec:
        out = []
        for opts in option_sets():
            apply_options(codec, opts)
            out.extend(plan(codec, n) for n in ns)
        return out


def extra_plans():
    out = []
    with make_codec(0, 256) as codec:
        for case in EXTRA:
            apply_options(codec, dict(EXTRA_BASE, **case["options"]))
            os.environ.update(case["env"])
            try:
                out.append([plan(codec, n) for n in NS])
            finally:
                for k in case["env"]:
                    del os.environ[k]
    return out


def tuning_plans(doc):
    """The plans after importing one shipped tuning text, for NS and the text's own lane batch."""
    m = doc["_meta"]
    lanes = m["streams"]
    ns = sorted(set(NS) | {(m["batch"] + lanes - 1) // lanes, m["batch"] // lanes})
    with make_codec(m["model"], m["patch"]) as codec:
        codec.set_option("streams", lanes)
        codec.tuning_import(doc["tuning"])
        return ns, [plan(codec, n) for n in ns]


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def digests(codec, opts, x):
    """SHA-256 of a codec_device step's symbols and bytes, and of encode / decode on their own."""
    apply_options(codec, opts)
    eh, ew, ec = codec.code_shape
    n = len(x)
    d_in, d_idx, d_rgb = codec.alloc(x.nbytes), codec.alloc(n * eh * ew * ec), codec.alloc(x.nbytes)
    try:
        d_in.upload(x)
        codec.memset_device(d_idx, 0xA5, n * eh * ew * ec)
        codec.memset_device(d_rgb, 0x5A, x.nbytes)
        codec.codec_device(d_in, n, d_idx, d_rgb)
        codec.synchronize()
        sym = d_idx.download((n, eh, ew, ec), np.uint8)
        rgb = d_rgb.download(x.shape, np.uint8)
    finally:
        for b in (d_in, d_idx, d_rgb):
            b.free()
    enc = codec.encode(x)
    dec = codec.decode(enc)
    return {"codec_symbols": sha(sym), "codec_rgb": sha(rgb), "encode_symbols": sha(enc), "decode_rgb": sha(dec)}


def digest_cases():
    x = np.random.default_rng(1234).integers(0, 256, (DIGEST_N, DIGEST_P, DIGEST_P, 3), dtype=np.uint8)
    codecs = {}
    try:
        for name, model, opts in DIGEST_CASES:
            if model not in codecs:
                codecs[model] = make_codec(model, DIGEST_P)
            yield name, digests(codecs[model], opts, x), plan(codecs[model], 2)
    finally:
        for c in codecs.values():
            c.close()


def save_fixture(doc, path):
    """The fixture as gzip-compressed JSON (the plan tables repeat themselves: 0.5 MB -> 18 KB)."""
    with open(path, "wb") as f, gzip.GzipFile(fileobj=f, mode="wb", filename="", mtime=0) as z:
        z.write((json.dumps(doc, separators=(",", ":")) + "\n").encode())


def load_fixture(path):
    with gzip.open(path, "rt") as f:
        return json.load(f)


def record(out_path):
    table = PlanTable()
    doc = {"lists": table.lists, "plans": table.plans, "grid": [], "extra": [], "tunings": [], "digests": []}
    for model, P, ns in GRID:
        got = grid_plans(model, P, ns)
        doc["grid"].append({"model": model, "patch": P, "ns": list(ns),
                            "idx": got if isinstance(got, str) else [table.add(p) for p in got]})
    for case, got in zip(EXTRA, extra_plans()):
        doc["extra"].append(dict(case, idx=[table.add(p) for p in got]))
    for path in sorted(glob.glob(os.path.join(ROOT, "tf_image_compression_amd", "tune", "*.json"))):
        with open(path) as f:
            tdoc = json.load(f)
        ns, got = tuning_plans(tdoc)
        doc["tunings"].append({"file": os.path.basename(path), "_meta": tdoc["_meta"], "tuning": tdoc["tuning"],
                               "ns": ns, "idx": [table.add(p) for p in got]})
    first, second = list(digest_cases()), list(digest_cases())
    for (name, a, p), (_, b, _) in zip(first, second):
        if a != b:
            raise SystemExit(f"digest case {name}: two runs differ ({a} vs {b}): not recorded")
        doc["digests"].append({"case": name, "sha256": a, "plan": table.add(p)})
    save_fixture(doc, out_path)
    nconf = sum(len(g["idx"]) for g in doc["grid"] if not isinstance(g["idx"], str))
    print(f"recorded {nconf} grid plans, {len(doc['extra'])} extra, {len(doc['tunings'])} tunings, "
          f"{len(doc['digests'])} digest cases; {len(table.plans)} distinct plans -> {out_path}")


if __name__ == "__main__":
    record(sys.argv[1])

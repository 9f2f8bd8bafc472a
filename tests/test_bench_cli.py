"""bench.py's command line: a plain run prints the headline result line only, ``--full`` adds
the per-kernel / roofline / parity figures, ``--dump-outputs DIR`` writes what the last timed
step computed — the same files from two runs with the same arguments."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup")
FULL_ONLY = ("roofline", "roofline_groups", "roofline_step_frac", "reheat", "ranks", "stats_allgather", "parity",
             "cpu_baseline")


def _bench_module():
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def test_dump_outputs_whole_when_they_fit(tmp_path):
    bench = _bench_module()
    a = np.arange(2 * 3 * 4, dtype=np.uint8).reshape(2, 3, 4)
    bench.dump_outputs(str(tmp_path / "d"), {"a": a, "b": a[:1]})
    got = np.load(tmp_path / "d" / "a.npy")
    assert got.dtype == np.float32 and got.shape == a.shape and np.array_equal(got, a)
    assert np.array_equal(np.load(tmp_path / "d" / "b.npy"), a[:1])


def test_dump_outputs_samples_rows_within_the_budget(tmp_path, monkeypatch):
    """Over the budget every array keeps a seeded choice of its rows: within the budget in
    all, the rows unchanged and in order, and the same rows on a second call."""
    bench = _bench_module()
    monkeypatch.setattr(bench, "DUMP_BYTES", 4 * 1000)
    r = np.random.default_rng(3)
    arrays = {"big": r.integers(0, 256, (100, 5, 8), dtype=np.uint8), "small": r.integers(0, 256, (50, 10), dtype=np.uint8)}
    bench.dump_outputs(str(tmp_path / "d1"), arrays)
    bench.dump_outputs(str(tmp_path / "d2"), arrays)
    total = 0
    for name, a in arrays.items():
        got = np.load(tmp_path / "d1" / f"{name}.npy")
        assert np.array_equal(got, np.load(tmp_path / "d2" / f"{name}.npy"))
        assert got.dtype == np.float32 and 0 < got.shape[0] < a.shape[0]
        rows = a.reshape(a.shape[0], -1)
        at = [int(np.flatnonzero((rows == g).all(axis=1))[0]) for g in got]
        assert at == sorted(set(at))
        total += got.nbytes
    assert 0.8 * 4000 <= total <= 4000


def test_full_and_dump_options_parse(monkeypatch):
    bench = _bench_module()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    args = bench.parse()
    assert args.full is False and args.dump_outputs is None and args.steps == 7
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "out"])
    args = bench.parse()
    assert args.full is True and args.dump_outputs == "out"


def _run_bench(*extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--batch", "4", "--patch", "64", "--no-autotune", "--preheat-s", "0", *extra]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_repeatably(tmp_path):
    """Two plain runs with the same arguments: the headline keys and none of the --full ones,
    and the dumped symbols and reconstruction equal element for element (the inputs are
    seeded, every kernel form is bit-reproducible)."""
    outs = []
    for d in ("a", "b"):
        out = _run_bench("--dump-outputs", str(tmp_path / d))
        assert all(k in out for k in HEADLINE) and not any(k in out for k in FULL_ONLY)
        assert out["steps"] == 3 and out["ms_per_step"] > 0 and out["unit"] == "MPix/s"
        assert abs(out["value"] - 4 * 64 * 64 / out["ms_per_step"] / 1e3) <= 0.01 * out["value"]
        outs.append({n: np.load(tmp_path / d / n) for n in sorted(os.listdir(tmp_path / d))})
    assert list(outs[0]) == ["reconstruction.npy", "symbols.npy"]
    assert outs[0]["reconstruction.npy"].shape == (4, 64, 64, 3) and outs[0]["reconstruction.npy"].dtype == np.float32
    assert outs[0]["symbols.npy"].shape[0] == 4 and set(np.unique(outs[0]["symbols.npy"])) <= {0.0, 1.0}
    assert outs[0]["reconstruction.npy"].std() > 0
    for n in outs[0]:
        assert np.array_equal(outs[0][n], outs[1][n])


@pytest.mark.gpu
def test_full_run_keeps_its_figures(tmp_path):
    """--full reports what the benchmark measured beside the headline before the option
    existed (CPU baseline left off here: it alone takes >= 12 s)."""
    out = _run_bench("--full", "--reheat-s", "0", "--no-cpu-baseline", "--layers-out", str(tmp_path / "layers.json"))
    assert all(k in out for k in HEADLINE)
    assert all(k in out for k in FULL_ONLY if k != "cpu_baseline")
    assert out["parity"]["symbol_mismatch_outside_band"] == 0
    assert out["stats_allgather"]["images"] == 4 * 3
    assert json.load(open(tmp_path / "layers.json"))["layers"]

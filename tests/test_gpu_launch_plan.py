"""The launch plan (csrc/tic_runtime.cpp plan_launches: which launches run a pass's layers, and
with which kernel instance) and what a codec step computes are pinned to a recording:
tests/golden/launch_plan.json.gz, written by tools/launch_plan_dump.py on the commit whose
behaviour is kept.  Replayed here through the same tool: every kernel name tic_layer_kernel /
tic_codec_kernel report and every (th, nsplit) of tic_layer_variant must be equal for every
recorded option set (the fusions, the forms, the chain with its shapes, neighbours, join and
lane counts, per model, patch size and batch; a chunk past the chain's 32-bit hand-off bound;
the variant and chain-cut environment overrides; the shipped tuning texts, which the fixture
embeds), and the SHA-256 of tic_codec_device's symbols and bytes, and of encode / decode, must
be equal for one option set per launch kind.  The plan part launches no kernel."""
import importlib.util
import os

import pytest

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("launch_plan_dump", os.path.join(ROOT, "tools", "launch_plan_dump.py"))
dump = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(dump)

FIX = dump.load_fixture(os.path.join(GOLDEN, "launch_plan.json.gz"))


def recorded(idx):
    """The recorded plan idx: [layer_kernels, codec_kernels, layer_variants]."""
    return [FIX["lists"][k] for k in FIX["plans"][idx]]


def differences(label, sets, ns, got, want_idx):
    """Plans that differ from the recording, as readable lines (the first few)."""
    assert len(got) == len(want_idx), f"{label}: {len(got)} configurations ran, the fixture holds {len(want_idx)}"
    bad = []
    for k, (g, w) in enumerate(zip(got, want_idx)):
        if g != recorded(w):
            what = ["layer_kernels", "codec_kernels", "layer_variants"]
            parts = {what[j]: {"now": g[j], "recorded": recorded(w)[j]} for j in range(3) if g[j] != recorded(w)[j]}
            bad.append(f"{label} {sets[k // len(ns)]} n={ns[k % len(ns)]}: {parts}")
    return bad


def test_the_fixture_holds_the_whole_grid():
    sets = list(dump.option_sets())
    assert [(g["model"], g["patch"], tuple(g["ns"])) for g in FIX["grid"]] == list(dump.GRID)
    assert all(len(g["idx"]) == len(sets) * len(g["ns"]) for g in FIX["grid"] if not isinstance(g["idx"], str))
    assert len(FIX["extra"]) == len(dump.EXTRA) and len(FIX["tunings"]) == 5
    assert [d["case"] for d in FIX["digests"]] == [c[0] for c in dump.DIGEST_CASES]


@pytest.mark.parametrize("model", dump.MODELS)
def test_grid_plans_are_the_recorded_ones(model):
    sets = list(dump.option_sets())
    groups = [g for g in FIX["grid"] if g["model"] == model]
    assert len(groups) == len(dump.PATCHES)
    ran, bad = 0, []
    for g in groups:
        got = dump.grid_plans(model, g["patch"], g["ns"])
        if isinstance(g["idx"], str) or isinstance(got, str):  # tic_create declined the patch size
            assert got == g["idx"]
            continue
        bad += differences(f"model {model} P {g['patch']}", sets, g["ns"], got, g["idx"])
        ran += len(got)
    assert not bad, f"{len(bad)} of {ran} plans differ:\n" + "\n".join(bad[:5])
    assert ran == sum(len(g["idx"]) for g in groups if not isinstance(g["idx"], str))


def test_chunk_bound_and_environment_overrides():
    assert [dict(options=e["options"], env=e["env"]) for e in FIX["extra"]] == dump.EXTRA
    got = dump.extra_plans()
    assert len(got) == len(FIX["extra"])
    bad = []
    for e, g in zip(FIX["extra"], got):
        bad += differences(f"{e['options']} {e['env']}", [""], dump.NS, g, e["idx"])
    assert not bad, "\n".join(bad[:5])
    for k in ("TIC_ENC01_VARIANT", "TIC_DEC10_VARIANT", "TIC_TEST_CHAIN_CUT"):
        assert k not in os.environ


@pytest.mark.parametrize("k", range(5))
def test_shipped_tuning_texts_plan_as_recorded(k):
    t = FIX["tunings"][k]
    ns, got = dump.tuning_plans(t)
    assert ns == t["ns"]
    bad = differences(t["file"], [""], ns, got, t["idx"])
    assert not bad, "\n".join(bad[:5])


def test_codec_bits_are_the_recorded_ones():
    got = list(dump.digest_cases())
    assert len(got) == len(FIX["digests"])
    for (name, sha, plan), want in zip(got, FIX["digests"]):
        assert name == want["case"]
        assert plan == recorded(want["plan"]), name  # the case still runs the launch kind it names
        assert sha == want["sha256"], name

"""The embedded-table ("TICA") container host code under AddressSanitizer + UBSan: `make
asan-rcseg-emb` builds tests/native/rcseg_emb_fuzz.cpp (its own main) against range_coder.cpp and
host_util.cpp with -fsanitize=address,undefined; the program runs round trips and ranges in
exact-size blocks, overwrites payload bytes outside a range's extent, and feeds truncated,
bit-flipped and random containers and every error path of tic_rcseg_count_nbr,
tic_rcseg_fit_tables and tic_rcseg_*_emb.  CPU only; nothing here is loaded into Python.  Any
sanitizer report or failed check fails the test."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_rcseg_emb_host_code_under_asan():
    build = subprocess.run(["make", "-C", ROOT, "build/rcseg_emb_fuzz_asan"], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([os.path.join(ROOT, "build", "rcseg_emb_fuzz_asan")], capture_output=True, text=True,
                         timeout=300)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    assert "rcseg_emb_fuzz ok" in run.stdout

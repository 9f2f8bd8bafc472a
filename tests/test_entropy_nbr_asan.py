"""The version-3 (causal-neighbour) container host code under AddressSanitizer + UBSan: `make
asan-rcseg-nbr` builds tests/native/rcseg_nbr_fuzz.cpp (its own main) against range_coder.cpp and
host_util.cpp with -fsanitize=address,undefined; the program runs round trips against the
definition's rows, random, truncated, bit-flipped and length-inconsistent containers and every
tic_rcseg_*_nbr error path.  CPU only; nothing here is loaded into Python.  Any sanitizer report
or failed check fails the test."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_rcseg_nbr_host_code_under_asan(tmp_path):
    build = subprocess.run(["make", "-C", ROOT, "build/rcseg_nbr_fuzz_asan"], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([os.path.join(ROOT, "build", "rcseg_nbr_fuzz_asan"), str(tmp_path)], capture_output=True,
                         text=True, timeout=300)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    assert "rcseg_nbr_fuzz ok" in run.stdout

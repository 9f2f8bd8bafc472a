"""The symbol-range entries of the container host code under AddressSanitizer + UBSan: `make
asan-rcseg-range` builds tests/native/rcseg_range_fuzz.cpp (its own main) against range_coder.cpp
and host_util.cpp with -fsanitize=address,undefined; the program decodes ranges of containers of
all three versions into blocks of exactly `count` bytes, takes the extent from the header and the
length table alone, overwrites the payload bytes outside the extent, and runs truncated and
bit-flipped containers and every error path.  CPU only; nothing here is loaded into Python.  Any
sanitizer report or failed check fails the test."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_rcseg_range_host_code_under_asan():
    build = subprocess.run(["make", "-C", ROOT, "build/rcseg_range_fuzz_asan"], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([os.path.join(ROOT, "build", "rcseg_range_fuzz_asan")], capture_output=True, text=True,
                         timeout=300)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    assert "rcseg_range_fuzz ok" in run.stdout

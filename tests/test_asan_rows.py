"""Rows back to texts' host code (llmtokenizer_amd/src/bpe_rows.c: bpe_rows_check and bpe_unpack_rows_host) under
AddressSanitizer + UBSan: a stand-alone program over exactly sized buffers (tests/asan_rows/asan_rows.c): B == 0 and
L == 0, both cell widths, row_stride > L in a grid that ends with its last cell, ids_cap == n exactly, and every
refusal.  CPU only; nothing here is loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("gcc") is None and shutil.which("cc") is None, reason="no C compiler")
def test_rows_host_code_under_asan_ubsan():
    subprocess.run(["make", "-s", "asan-rows"], cwd=ROOT, check=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(ROOT, "tests", "asan_rows", "asan_rows")], capture_output=True, text=True,
                       timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "asan_rows: ok" in r.stdout
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]

"""BPE_SPLIT_CL100K's host code (llmtokenizer_amd/src/bpe_split_preset.c: the rule through
bpe_split_offsets_host; src/bpe_special.c: the preset through bpe_split_offsets_host_special) under
AddressSanitizer + UBSan: a stand-alone program (tests/asan_split_cl100k/asan_split_cl100k.c) with
texts and offsets in buffers of exactly their size.  CPU only."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("gcc") is None and shutil.which("cc") is None, reason="no C compiler")
def test_split_cl100k_host_code_under_asan_ubsan():
    subprocess.run(["make", "-s", "asan-split-cl100k"], cwd=ROOT, check=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(ROOT, "tests", "asan_split_cl100k", "asan_split_cl100k")], capture_output=True,
                       text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "asan_split_cl100k: ok" in r.stdout
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]

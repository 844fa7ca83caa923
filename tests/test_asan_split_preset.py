"""The preset rules' host code (llmtokenizer_amd/src/bpe_split_preset.c: the rules in
plain C, bpe_encode_split_preset, bpe_train_split_preset) and the bodies and context
cache it goes through under AddressSanitizer + UBSan: a stand-alone program with a host
model of the engine calls (tests/asan_split_preset/asan_split_preset.c).  CPU only."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("gcc") is None and shutil.which("cc") is None, reason="no C compiler")
def test_split_preset_host_code_under_asan_ubsan():
    subprocess.run(["make", "-s", "asan-split-preset"], cwd=ROOT, check=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(ROOT, "tests", "asan_split_preset", "asan_split_preset")], capture_output=True,
                       text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "asan_split_preset: ok" in r.stdout
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]

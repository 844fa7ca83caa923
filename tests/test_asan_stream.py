"""The packed streams' host code (llmtokenizer_amd/src/bpe_stream.c: bpe_stream_check and bpe_pack_stream_host)
under AddressSanitizer + UBSan: a stand-alone program over exactly sized buffers (tests/asan_stream/asan_stream.c): no
text, all texts empty, one text, a thousand texts, every BOS / EOS / drop_last combination with rows_cap == R
exactly, and every refusal.  CPU only; nothing here is loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("gcc") is None and shutil.which("cc") is None, reason="no C compiler")
def test_stream_host_code_under_asan_ubsan():
    subprocess.run(["make", "-s", "asan-stream"], cwd=ROOT, check=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(ROOT, "tests", "asan_stream", "asan_stream")], capture_output=True, text=True,
                       timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "asan_stream: ok" in r.stdout
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]

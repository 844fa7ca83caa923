"""The token spans' host code (llmtokenizer_amd/src/bpe_spans.c: bpe_span_lens and bpe_token_spans_host)
under AddressSanitizer + UBSan: a stand-alone program over exactly sized buffers
(tests/asan_spans/asan_spans.c): the table with and without a vocabulary with holes, both units over texts
that cut a character, no text, empty texts, and every refusal.  CPU only; nothing here is loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("gcc") is None and shutil.which("cc") is None, reason="no C compiler")
def test_spans_host_code_under_asan_ubsan():
    subprocess.run(["make", "-s", "asan-spans"], cwd=ROOT, check=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(ROOT, "tests", "asan_spans", "asan_spans")], capture_output=True, text=True,
                       timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "asan_spans: ok" in r.stdout
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]

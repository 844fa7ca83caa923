"""The host definition of NFC (llmtokenizer_amd/src/bpe_normalize.c, api.nfc_host; the contract: include/bpe_gpu.h,
"Normalization") against unicodedata.normalize on the text decoded with errors="surrogateescape".  No GPU."""
import itertools
import unicodedata

import pytest

from llmtokenizer_amd import api

S, L, V, T = 0xAC00, 0x1100, 0x1161, 0x11A7  # Hangul: the first syllable, leading consonant, vowel and (T + 1) trailing


def ref(data):
    return unicodedata.normalize("NFC", data.decode("utf-8", "surrogateescape")).encode("utf-8", "surrogateescape")


def code_points():
    return [c for c in range(0x110000) if not 0xD800 <= c < 0xE000]


def decomposable():
    """(code point, its raw canonical decomposition) of every code point that has one"""
    for c in code_points():
        d = unicodedata.decomposition(chr(c))
        if d and not d.startswith("<"):
            yield c, "".join(chr(int(x, 16)) for x in d.split())


def test_tables_are_this_pythons():
    want = f"unicodedata {unicodedata.unidata_version}"
    assert api.nfc_info()["source"] == want, f"regenerate csrc/unicode_nfc.h (tools/gen_unicode_nfc.py) under {want}"


def test_every_code_point():
    data = "".join("a" + chr(c) for c in code_points()).encode()
    assert api.nfc_host(data) == ref(data)


def test_pairs_and_exclusions():
    """every decomposition of two or one code points behind its composite: the listed pairs compose, the exclusions
    and singletons do not"""
    data = "".join(chr(c) + " " + d + " " for c, d in decomposable()).encode()
    assert api.nfc_host(data) == ref(data)


@pytest.mark.parametrize("text", [
    "".join(chr(l) + chr(v) + " " + chr(l) + chr(v) + chr(t) + " " + chr(S + ((l - L) * 21 + (v - V)) * 28) + chr(t) + " " +
            chr(S + ((l - L) * 21 + (v - V)) * 28 + 1) + chr(t) + " "
            for l in (L, L + 18) for v in (V, V + 20) for t in (T, T + 1, T + 27, T + 28)),  # (T and T + 28: no trailing)
    "".join("a" + "".join(p) + " " for p in itertools.permutations("\u0301\u0323\u0327")),  # ccc 230, 220, 202
    "".join("a" + "".join(p) + " " for p in itertools.permutations("\u0301\u0300\u0302")),  # all 230: stable
    "a\u0327\u0327\u0301 a\u0323\u0323\u0307 \u1100\u0301\u1161 e\u0301\u0301",  # blocked
    "\u0301\u0323 marks first",
], ids=["hangul", "distinct", "equal", "blocked", "nobase"])
def test_cases(text):
    data = text.encode()
    assert api.nfc_host(data) == ref(data)


@pytest.mark.parametrize("data", [b"a\x80\xcc\x81", b"e\xcc", b"a\xc0\xaf\xcc\x81", b"\xed\xa0\x80\xcc\x81",
                                  b"\xf4\x90\x80\x80", b"a\x00\xcc\x81"])
def test_ill_formed(data):
    assert api.nfc_host(data) == ref(data)

"""The class table of BPE_SPLIT_GPT2_UNICODE (llmtokenizer_amd/csrc/unicode_classes.h through
bpe_ex.h bpe_unicode_class / bpe_unicode_info): every class against the `regex` module when the
installed version is the one the table came from, the digest the header states, and values that
hold in any Unicode version.  No GPU."""
import pytest

from llmtokenizer_amd import api

NCP = 0x110000
WHITE_SPACE = [0x85, 0xA0, 0x1680, 0x2028, 0x2029, 0x202F, 0x205F, 0x3000] + list(range(0x09, 0x0E)) + list(range(0x2000, 0x200B))


@pytest.fixture(scope="module")
def classes():
    return [api.unicode_class(cp) for cp in range(NCP)]


def test_every_class_equals_regex(classes):
    regex = pytest.importorskip("regex")
    info = api.unicode_info()
    if info["source"] != f"regex {regex.__version__}":
        pytest.skip(f"the table came from {info['source']}, installed is regex {regex.__version__}")
    text = "".join(chr(c) for c in range(NCP))
    want = ["P"] * NCP
    for pat, k in ((r"\p{N}", "N"), (r"\p{L}", "L"), (r"\s", "W")):  # (later ones win: the order of the definition)
        for m in regex.finditer(pat, text):
            want[ord(m.group())] = k
    want[0x20] = "S"
    assert classes == want


def test_the_digest(classes):
    h = 0xCBF29CE484222325  # FNV-1a 64 over the classes as bytes 0 P, 1 L, 2 N, 3 S, 4 W
    for k in bytes(api.UNICODE_CLASSES.index(c) for c in classes):
        h = ((h ^ k) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    info = api.unicode_info()
    assert h == info["digest"]
    assert info["source"].startswith("regex ")


def test_values_of_every_unicode_version(classes):
    for ch in "AéЖ中\U00010400":
        assert classes[ord(ch)] == "L", hex(ord(ch))
    for ch in "7٣²½\U0001d7d8":
        assert classes[ord(ch)] == "N", hex(ord(ch))
    assert [cp for cp in range(NCP) if classes[cp] == "S"] == [0x20]
    assert [cp for cp in range(NCP) if classes[cp] == "W"] == sorted(WHITE_SPACE) and len(WHITE_SPACE) == 24
    for cp in (0x1C, 0x1D, 0x1E, 0x1F, 0x0301, 0x2014, 0x1F600, 0xD800, 0x10FFFF, 0x00, 0x27):
        assert classes[cp] == "P", hex(cp)
    for cp in (0x110000, 0xFFFFFFFF):
        assert api.unicode_class(cp) == "P"

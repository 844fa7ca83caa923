"""BPE_SPLIT_GPT2_UNICODE in plain C (bpe_ex.h bpe_split_offsets_host, api.split_host(data,
"gpt2_unicode")) against Python's re: GPT-2's pattern with \\p{L}, \\p{N} and \\s written out as
character classes from api.unicode_class over all code points, over the text decoded with
errors="surrogateescape", its match offsets mapped back to bytes by the same codec.  This tests
the rule (UTF-8 decoding, ill-formed bytes, the look-ahead at end(i), the contractions), not the
class table: tests/test_unicode_classes.py holds that.  No GPU."""
import itertools
import re

import numpy as np
import pytest

from llmtokenizer_amd import api

RULE = "gpt2_unicode"
EOT = b"<|endoftext|>"

# the alphabet of the rule's checks: ASCII, letters, numbers, white space, other, ill-formed fragments
ASCII = [b"'", b"s", b"t", b"r", b"e", b"l", b"v", b"a", b"Z", b"1", b"!", b"\n", b" ", b"\x00", b"\x1c"]
LETTERS = [s.encode() for s in ("é", "ß", "Ж", "中", "\U00010400")]
NUMBERS = [s.encode() for s in ("٣", "²", "½", "\U0001d7d8")]
SPACES = [s.encode() for s in ("\u00a0", "\u2003", "\u3000", "\u2028", "\u0085")]
OTHER = [s.encode() for s in ("—", "€", "\U0001f600", "\u0301")]
ILL = [b"\x80", b"\xc3", b"\xe2", b"\xe2\x82", b"\xf0\x9f", b"\xf0\x9f\x98", b"\xc0\x80", b"\xed\xa0\x80",
       b"\xf4\x90\x80\x80", b"\xff", b"\xe0\x80\x80"]
FULL = ASCII + LETTERS + NUMBERS + SPACES + OTHER + ILL
TEN = [b"'", b"s", b"l", b" ", b"\n", "é".encode(), "٣".encode(), "\u3000".encode(), b"\xe2\x82", "—".encode()]


def _ranges(cps):
    """a sorted list of code points as the inside of a character class"""
    out, i = [], 0
    while i < len(cps):
        j = i
        while j + 1 < len(cps) and cps[j + 1] == cps[j] + 1:
            j += 1
        out.append("\\U%08x" % cps[i] if i == j else "\\U%08x-\\U%08x" % (cps[i], cps[j]))
        i = j + 1
    return "".join(out)


@pytest.fixture(scope="module")
def pattern():
    by = {k: [] for k in api.UNICODE_CLASSES}
    for cp in range(0x110000):
        by[api.unicode_class(cp)].append(cp)
    assert by["S"] == [0x20] and len(by["W"]) == 24
    L, N, ws = _ranges(by["L"]), _ranges(by["N"]), _ranges(sorted(by["S"] + by["W"]))
    return re.compile(f"'s|'t|'re|'ve|'m|'ll|'d| ?[{L}]+| ?[{N}]+| ?[^{ws}{L}{N}]+|[{ws}]+(?![^{ws}])|[{ws}]+")


def pattern_offsets(pat, data):
    """the byte offsets of the pattern's successive matches over data decoded with surrogateescape"""
    text = data.decode("utf-8", "surrogateescape")
    at = np.zeros(len(text) + 1, dtype=np.int64)  # byte offset of every character
    at[1:] = np.cumsum([len(ch.encode("utf-8", "surrogateescape")) for ch in text])
    out, pos = [], 0
    for m in pat.finditer(text):
        assert m.start() == pos and m.end() > pos
        out.append(int(at[pos]))
        pos = m.end()
    assert pos == len(text)
    return out + [len(data)]


def check(pat, data):
    got = api.split_host(data, RULE)
    assert got.dtype == np.uint64
    assert got.tolist() == pattern_offsets(pat, data), data


def random_strings(seed, count, items, alphabet):
    rng = np.random.default_rng(seed)
    for n in rng.integers(0, items + 1, count).tolist():
        yield b"".join(alphabet[k] for k in rng.integers(0, len(alphabet), n).tolist())


def test_every_short_string_over_ten_items(pattern):
    assert len(TEN) == 10
    for n in range(5):
        for t in itertools.product(TEN, repeat=n):
            check(pattern, b"".join(t))


def test_random_strings_over_the_full_alphabet(pattern):
    for data in random_strings(21, 100000, 12, FULL):
        check(pattern, data)


def test_uniformly_random_bytes(pattern):
    rng = np.random.default_rng(22)
    for _ in range(5000):
        check(pattern, rng.integers(0, 256, int(rng.integers(0, 25)), dtype=np.uint8).tobytes())


def test_empty_and_one_byte(pattern):
    assert api.split_host(b"", RULE).tolist() == [0]
    for b in range(256):
        assert api.split_host(bytes([b]), RULE).tolist() == [0, 1]
        check(pattern, bytes([b]))


@pytest.mark.parametrize("ch", ["é", "\u3000", "中", "\U00010400", "\U0001d7d8"])
def test_a_text_that_ends_inside_a_sequence(pattern, ch):
    """a sequence the end of the text cuts is ill-formed: each of its bytes is a character of class P"""
    full = ch.encode()
    for head in (b"", b"a", b"a ", b" ", "é".encode(), b"a\n\n", b"1"):
        for k in range(1, len(full) + 1):
            check(pattern, head + full[:k])
            check(pattern, head + full[:k] + b"a")
    assert api.split_host(b"a" + "中".encode()[:2], RULE).tolist() == [0, 1, 3]
    assert api.split_host(b"a" + "中".encode(), RULE).tolist() == [0, 4]


def test_the_issue_s_examples():
    def pieces(text):
        data = text.encode()
        off = api.split_host(data, RULE).tolist()
        return [data[a:b].decode() for a, b in zip(off, off[1:])]
    assert pieces("a—b €5") == ["a", "—", "b", " €", "5"]
    assert pieces("x٣½y") == ["x", "٣½", "y"]
    assert pieces("e\u0301's") == ["e", "\u0301'", "s"]  # a decomposed e-acute splits at its combining mark (class P)
    assert pieces("a\u3000\u3000b\u2028") == ["a", "\u3000", "\u3000", "b", "\u2028"]  # only U+0020 joins what follows
    assert pieces("a\u00a0 b") == ["a", "\u00a0", " b"]
    assert pieces("a\x1c b") == ["a", "\x1c", " b"]  # U+001C is no white space here


def test_the_real_pattern_when_regex_is_installed():
    """the same strings against the regex module's own classes: those of this alphabet hold in every Unicode version"""
    regex = pytest.importorskip("regex")
    pat = regex.compile(r"'s|'t|'re|'ve|'m|'ll|'d| ?\p{L}+| ?\p{N}+| ?[^\s\p{L}\p{N}]+|\s+(?!\S)|\s+")
    for data in itertools.chain(random_strings(23, 30000, 12, FULL), random_strings(24, 10000, 6, TEN)):
        assert api.split_host(data, RULE).tolist() == pattern_offsets(pat, data), data


def test_ascii_text_splits_as_gpt2():
    rng = np.random.default_rng(25)
    alphabet = np.frombuffer(b"'''stredvml  \n\t\r\x0b\x0caZ09!,.\x00\x7f\x1c", np.uint8)
    for n in rng.integers(0, 40, 10000).tolist():
        data = rng.choice(alphabet, n).tobytes()
        assert api.split_host(data, RULE).tolist() == api.split_host(data, "gpt2").tolist(), data


def restate_special(data, specials):
    """the definition with specials: the matches found from the left, every stretch between them a text of its own"""
    out, seg, i = [], 0, 0
    while i < len(data):
        hit = next((s for s in specials if data.startswith(s, i)), None)
        if hit is None:
            i += 1
            continue
        out += [seg + int(o) for o in api.split_host(data[seg:i], RULE)[:-1]] + [i]
        i += len(hit)
        seg = i
    return out + [seg + int(o) for o in api.split_host(data[seg:], RULE)[:-1]] + [len(data)]


def test_specials_cut_the_text_into_segments():
    sp = [EOT, b"\xac|x|"]
    euro = "€".encode()
    assert euro[2:] + b"|x|" == sp[1]
    # the special begins with what would be the euro sign's last byte: the match cuts the sequence, E2 and 82 are ill-formed
    data = b"a " + euro + b"|x| b"
    assert api.split_host(data, RULE, specials=sp).tolist() == [0, 1, 4, 8, 10]  # a | space E2 82 | the special | space b
    assert api.split_host(data, RULE, specials=[EOT]).tolist() == [0, 1, 6, 7, 8, 10]  # a | space euro bar | x | bar | space b
    rng = np.random.default_rng(26)
    items = FULL + [EOT, EOT, sp[1], b"\xe2\x82" + sp[1]]
    for _ in range(20000):
        data = b"".join(items[k] for k in rng.integers(0, len(items), int(rng.integers(0, 10))).tolist())
        got, piece, index = api.split_host_special(data, RULE, sp)
        assert got.tolist() == restate_special(data, sp), data
        assert [data[int(got[p]):int(got[p + 1])] for p in piece.tolist()] == [sp[j] for j in index.tolist()]


def test_the_preset_has_no_tables():
    assert api.SPLIT_PRESETS[RULE] == 4
    with pytest.raises(api.BpeError, match="no tables"):
        api.split_rule(RULE)

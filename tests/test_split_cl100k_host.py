"""BPE_SPLIT_CL100K in plain C (bpe_ex.h bpe_split_offsets_host, api.split_host(data, "cl100k")) against
its restatement character by character (tests/cl100k_ref.py) and, where the regex module is installed,
against the pattern itself over the text decoded with errors="surrogateescape", its match offsets
mapped back to bytes by the same codec.  Every byte string decodes under that codec, one character per
byte in no well-formed sequence, so the random bytes need no filter.  No GPU."""
import itertools

import numpy as np
import pytest

import cl100k_ref as C
import special_ref as SR
from llmtokenizer_amd import api

RULE = "cl100k"
EOT = b"<|endoftext|>"

TWELVE = [b"'", b"s", b"S", b"r", b"e", b"l", b"L", b"a", b"1", b"!", b" ", b"\n"]
MORE = [s.encode() for s in ("\t", "\r", "ſ", "é", "٣", "½", "　", "—")]
ILL = [b"\x80", b"\xc3", b"\xe2\x82", b"\xf0\x9f\x98", b"\xc0\x80", b"\xed\xa0\x80", b"\xff"]
FULL = TWELVE + MORE + ILL


def check(data):
    got = api.split_host(data, RULE)
    assert got.dtype == np.uint64
    assert got.tolist() == C.offsets(data), data


def random_strings(seed, count, items, alphabet):
    rng = np.random.default_rng(seed)
    for n in rng.integers(0, items + 1, count).tolist():
        yield b"".join(alphabet[k] for k in rng.integers(0, len(alphabet), n).tolist())


def random_bytes(seed, count):
    rng = np.random.default_rng(seed)
    for _ in range(count):
        yield rng.integers(0, 256, int(rng.integers(0, 25)), dtype=np.uint8).tobytes()


def test_every_short_string_over_twelve_items():
    assert len(TWELVE) == 12
    for n in range(6):
        for t in itertools.product(TWELVE, repeat=n):
            check(b"".join(t))


def test_random_strings_over_the_full_alphabet():
    for data in random_strings(31, 100000, 16, FULL):
        check(data)


def test_uniformly_random_bytes():
    for data in random_bytes(32, 3000):
        check(data)


def test_empty_and_one_byte():
    assert api.split_host(b"", RULE).tolist() == [0]
    for b in range(256):
        assert api.split_host(bytes([b]), RULE).tolist() == [0, 1]


@pytest.mark.parametrize("ch", ["é", "ſ", "　", "٣", "\U0001d7d8"])
def test_a_text_that_ends_inside_a_sequence(ch):
    full = ch.encode()
    for head in (b"", b"a", b"a ", b" ", b"a'", b"1", b"12", b"123", b"!\n", b"\n "):
        for k in range(1, len(full) + 1):
            check(head + full[:k])
            check(head + full[:k] + b"a")


def test_a_text_that_ends_inside_a_contraction():
    for head in (b"", b"a", b"1", b"\n", b" ", b"!"):
        for tail in (b"'", b"'r", b"'R", b"'l", b"'v", b"'\xc5", b"'re", b"'s", "'ſ".encode(), b"'ll", b"'lx"):
            check(head + tail)
    assert api.split_host(b"a'r", RULE).tolist() == [0, 1, 3]  # a | 'r: the apostrophe is the letter's prefix
    assert api.split_host(b"a're", RULE).tolist() == [0, 1, 4]


def pieces(text, specials=None):
    data = text.encode()
    off = api.split_host(data, RULE, specials=specials).tolist()
    return [data[a:b].decode() for a, b in zip(off, off[1:])]


def test_the_named_examples():
    assert pieces("don't") == ["don", "'t"]
    assert pieces("DON'T") == ["DON", "'T"]
    assert pieces("'there") == ["'t", "here"]
    assert pieces("'hello") == ["'hello"]
    assert pieces(" 's") == [" '", "s"]
    assert pieces("12345") == ["123", "45"]
    assert pieces(" 123") == [" ", "123"]
    assert pieces("!\n\n  x") == ["!\n\n", " ", " x"]
    assert pieces("x \n \ny") == ["x", " \n \n", "y"]
    assert pieces("a  b") == ["a", " ", " b"]
    assert pieces('"hi"') == ['"hi', '"']
    assert pieces("'ſ") == ["'ſ"]
    assert pieces("a'ſb") == ["a", "'ſ", "b"]  # a contraction of three bytes
    assert pieces("٣٣٣٣½") == ["٣٣٣", "٣½"]    # the index in a run counts characters


def test_the_real_pattern_when_regex_is_installed():
    regex = pytest.importorskip("regex")
    pat = regex.compile(C.PATTERN)

    def pattern_offsets(data):
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

    short = (b"".join(t) for n in range(5) for t in itertools.product(TWELVE, repeat=n))
    for data in itertools.chain(short, random_strings(33, 40000, 16, FULL), random_bytes(32, 3000)):
        assert api.split_host(data, RULE).tolist() == pattern_offsets(data), data


def test_specials_cut_the_text_into_segments():
    sp = [EOT, b"\xac|x|"]
    rng = np.random.default_rng(34)
    items = FULL + [EOT, EOT, sp[1], b"\xe2\x82" + sp[1], b"12", b"\n\n", b"  "]
    for _ in range(20000):
        data = b"".join(items[k] for k in rng.integers(0, len(items), int(rng.integers(0, 12))).tolist())
        want, wp, wi = SR.restate(data, sp, C.offsets)
        got, piece, index = api.split_host_special(data, RULE, sp)
        assert got.tolist() == want.tolist(), data
        assert piece.tolist() == wp.tolist() and index.tolist() == wi.tolist()
        assert api.split_host(data, RULE, specials=sp).tolist() == want.tolist()


def test_a_match_breaks_every_chain():
    sp = [EOT]
    e = EOT.decode()
    assert pieces("1234" + e + "5678", sp) == ["123", "4", e, "567", "8"]  # the run after the match counts from it
    assert pieces("1234" + "5678") == ["123", "456", "78"]
    assert pieces("!\n" + e + "\n  x", sp) == ["!\n", e, "\n", " ", " x"]
    assert pieces("!\n" + e + "\n  \nx", sp) == ["!\n", e, "\n  \n", "x"]  # no P before the run after the match
    assert pieces("!\n\n  \nx") == ["!\n\n", "  \n", "x"]
    assert pieces("x\n  " + e + " \ny", sp) == ["x", "\n", "  ", e, " \n", "y"]  # no newline after the spaces in their segment
    assert pieces("x\n   \ny") == ["x", "\n   \n", "y"]


def test_the_preset_has_no_tables_and_the_gaps_are_no_presets():
    assert api.SPLIT_PRESETS[RULE] == 6
    with pytest.raises(api.BpeError, match="no tables"):
        api.split_rule(RULE)
    import ctypes
    from llmtokenizer_amd import _lib
    L = _lib.load()
    buf = np.frombuffer(b"a b", np.uint8)
    cnt = ctypes.c_size_t(0)
    for preset in (3, 5, 7, -1, 1000):
        rc = L.bpe_split_offsets_host(preset, buf.ctypes.data_as(ctypes.c_void_p), buf.size, None, 0, ctypes.byref(cnt))
        assert L.bpe_gpu_strerror(rc) == b"invalid argument", preset
    rc = L.bpe_split_offsets_host(6, buf.ctypes.data_as(ctypes.c_void_p), buf.size, None, 0, ctypes.byref(cnt))
    assert rc == 0 and cnt.value == 3

"""The preset split rules in plain C (bpe_ex.h bpe_split_offsets_host,
api.split_host): "gpt2" against Python's re and the bytes pattern bpe_gpu.h
gives for it, "lines" and "words" against the numpy restatement of their
tables.  No GPU: the call is a pure host function, and tests/test_gpu_split_gpt2.py
holds the device kernel to it."""
import itertools
import re

import numpy as np
import pytest

from llmtokenizer_amd import api

# GPT-2's alternation with \p{L}, \p{N} and \s replaced by the byte classes of bpe_gpu.h
PATTERN = re.compile(rb"'s|'t|'re|'ve|'m|'ll|'d| ?[A-Za-z\x80-\xff]+| ?[0-9]+| ?[^\sA-Za-z0-9\x80-\xff]+|\s+(?!\S)|\s+")
assert re.fullmatch(rb"\s+", b" \t\n\v\f\r") and not re.search(rb"\s", bytes(set(range(256)) - set(b" \t\n\v\f\r")))

EXAMPLE = b"Hello, world  42x\n\nfoo's it'll've 'tis don't  'd"
EXAMPLE_PIECES = [b"Hello", b",", b" world", b" ", b" 42", b"x", b"\n", b"\n", b"foo", b"'s", b" it", b"'ll", b"'ve",
                  b" '", b"tis", b" don", b"'t", b" ", b" '", b"d"]


def re_offsets(data):
    """the starts of the pattern's successive matches, which tile data, followed by len(data)"""
    out, pos = [], 0
    for m in PATTERN.finditer(data):
        assert m.start() == pos and m.end() > pos
        out.append(pos)
        pos = m.end()
    assert pos == len(data)
    return out + [len(data)]


def restate(data, cls, brk):
    b = np.frombuffer(data, np.uint8)
    c = np.asarray(cls)[b]
    st = np.ones(b.size, bool)
    st[1:] = (np.asarray(brk)[c[:-1]] >> c[1:]) & 1
    return np.append(np.flatnonzero(st), b.size).astype(np.uint64)


def check(data):
    got = api.split_host(data, "gpt2")
    assert got.dtype == np.uint64
    assert got.tolist() == re_offsets(data), data


def test_the_example_string():
    off = api.split_host(EXAMPLE, "gpt2").tolist()
    assert [EXAMPLE[a:b] for a, b in zip(off, off[1:])] == EXAMPLE_PIECES
    check(EXAMPLE)


def test_every_short_string_over_ten_bytes():
    alphabet = b"'srela1! \n"
    assert len(alphabet) == 10
    for n in range(6):
        for t in itertools.product(alphabet, repeat=n):
            check(bytes(t))


def test_random_strings_over_a_wider_alphabet():
    rng = np.random.default_rng(11)
    alphabet = np.frombuffer(b"'''stredvml  \n\t\r\x0b\x0caZ09!,.\x00\x7f\x80\xc3\xa9\xff", np.uint8)
    lens = rng.integers(0, 15, 100000)
    flat = rng.choice(alphabet, int(lens.sum())).tobytes()
    o = 0
    for n in lens.tolist():
        check(flat[o:o + n])
        o += n


def test_uniformly_random_bytes():
    rng = np.random.default_rng(12)
    for _ in range(3000):
        check(rng.integers(0, 256, int(rng.integers(0, 301)), dtype=np.uint8).tobytes())


@pytest.mark.parametrize("tail", [b"  ", b" ", b"\n\n", b"'l", b"'r", b"'ll", b"'"])
def test_the_end_of_the_text(tail):
    """white space that reaches the end stays whole; a contraction cut by the end is none"""
    for head in (b"", b"a", b"ab ", b"it", b"x\n", b"7", b"a "):
        check(head + tail)
    # ... and the same bytes followed by text are cut as text: the end is part of the rule
    check(b"a" + tail + b"l")
    check(b"a" + tail + b"e")


def test_empty_and_one_byte():
    assert api.split_host(b"", "gpt2").tolist() == [0]
    for b in range(256):
        assert api.split_host(bytes([b]), "gpt2").tolist() == [0, 1]


@pytest.mark.parametrize("rule", ["lines", "words"])
def test_table_presets_equal_the_numpy_restatement(rule):
    cls, brk = api.split_rule(rule)
    rng = np.random.default_rng(13)
    texts = [b"", b"x", b"\n", EXAMPLE, "naïve  café \n".encode()]
    texts += [rng.integers(0, 256, int(rng.integers(0, 400)), dtype=np.uint8).tobytes() for _ in range(300)]
    texts += [rng.choice(np.frombuffer(b"ab 1\n\t,", np.uint8), int(rng.integers(0, 400))).tobytes() for _ in range(300)]
    for t in texts:
        assert api.split_host(t, rule).tolist() == restate(t, cls, brk).tolist(), (rule, t)


def test_split_host_rejects_what_is_no_preset():
    with pytest.raises(api.BpeError):
        api.split_host(b"abc", "gpt3")
    with pytest.raises(api.BpeError):
        api.split_host(b"abc", api.split_rule("words"))
    with pytest.raises(api.BpeError, match="no tables"):
        api.split_rule("gpt2")

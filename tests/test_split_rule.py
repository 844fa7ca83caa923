"""Split rules (bpe_gpu.h bpe_gpu_split_rule): the two presets against tables
built here from their definitions, and the rule's restatement in numpy on the
header's example.  No GPU: the preset call is a pure host function."""
import numpy as np
import pytest

from llmtokenizer_amd import api


def restate(data, cls, brk):
    """the piece starts followed by len(data): what bpe_gpu_split must produce"""
    b = np.frombuffer(data, np.uint8)
    c = np.asarray(cls)[b]
    st = np.ones(b.size, bool)
    st[1:] = (np.asarray(brk)[c[:-1]] >> c[1:]) & 1
    return np.append(np.flatnonzero(st), b.size).astype(np.uint64)


def pieces(data, cls, brk):
    off = restate(data, cls, brk)
    return [data[int(a):int(b)] for a, b in zip(off, off[1:])]


def test_lines_preset():
    cls, brk = api.split_rule("lines")
    want_cls = np.zeros(256, np.uint8)
    want_cls[ord("\n")] = 1
    want_brk = np.zeros(16, np.uint16)
    want_brk[1] = 0x3
    assert cls.dtype == np.uint8 and brk.dtype == np.uint16
    assert cls.tolist() == want_cls.tolist() and brk.tolist() == want_brk.tolist()


def test_words_preset():
    cls, brk = api.split_rule("words")
    want_cls = np.zeros(256, np.uint8)
    for b in range(256):
        ch = bytes([b])
        if b >= 0x80 or ch.isalpha():
            want_cls[b] = 1
        elif ch.isdigit():
            want_cls[b] = 2
        elif b == 0x20:
            want_cls[b] = 3
        elif ch in b"\t\n\v\f\r":
            want_cls[b] = 4
    want_brk = np.zeros(16, np.uint16)
    for p in (0, 1, 2, 4):
        want_brk[p] = 0x1F & ~(1 << p)
    want_brk[3] = 1 << 4
    assert cls.tolist() == want_cls.tolist() and brk.tolist() == want_brk.tolist()
    assert int(cls.max()) <= 15


def test_unknown_preset():
    with pytest.raises(api.BpeError):
        api.split_rule("gpt2")


def test_example_string():
    cls, brk = api.split_rule("words")
    text = b"Hello, world  42x\n\nfoo's"
    assert pieces(text, cls, brk) == [b"Hello", b",", b" world", b"  42", b"x", b"\n\n", b"foo", b"'", b"s"]
    assert restate(b"", cls, brk).tolist() == [0]
    # a UTF-8 sequence never splits, and spaces attach to what follows them unless white space does
    assert pieces("naïve  café \n".encode(), cls, brk) == ["naïve".encode(), "  café".encode(), b" ", b"\n"]


def test_lines_on_text():
    cls, brk = api.split_rule("lines")
    text = b"one\ntwo\n\nthree"
    assert pieces(text, cls, brk) == text.splitlines(keepends=True) == [b"one\n", b"two\n", b"\n", b"three"]


def test_split_geometry_is_exported():
    info = api.split_info()
    assert info["tile"] > 0 and info["tile"] % 16 == 0 and info["grid_bytes"] % info["tile"] == 0

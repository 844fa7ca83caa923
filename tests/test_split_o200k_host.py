"""BPE_SPLIT_O200K on the host (src/bpe_split_preset.c over src/bpe_o200k_rule.h; no GPU): api.split_host(data,
"o200k") equals the `regex` module's own run of the pattern, over exhaustive small strings, random ones, random
bytes and the named examples; with specials it is the rule applied between the matches; the case class table
agrees with `regex` on every code point.  The maps the device composes are not probed here (the host rule walks
the automaton, it composes nothing): tests/test_gpu_split_o200k.py covers them by runs longer than a grid step."""
import itertools
import random

import pytest

from llmtokenizer_amd import api
from llmtokenizer_amd.vocab import O200K_PATTERN

regex = pytest.importorskip("regex")
PAT = regex.compile(O200K_PATTERN)
TWELVE = ["A", "a", "ʰ", "ǅ", "́", "'", "s", "!", "/", " ", "\n", "1"]


def want(data):
    """the pattern over the text decoded as the rule decodes it: a byte in no well-formed sequence is a character
    of its own that is no letter, number or white space (here a private-use one)"""
    chars, pos, i = [], [], 0
    while i < len(data):
        ch = None
        for ln in (1, 2, 3, 4):
            try:
                ch = data[i:i + ln].decode("utf-8")
                break
            except UnicodeDecodeError:
                ch = None
        if ch is None or len(ch) != 1:
            ch, ln = chr(0xE000 + data[i]), 1
        chars.append(ch)
        pos.append(i)
        i += ln
    pos.append(len(data))
    out = [pos[m.start()] for m in PAT.finditer("".join(chars))]
    return out + [len(data)]


def same(data):
    assert api.split_host(data, "o200k").tolist() == want(data), data


@pytest.mark.parametrize("items,longest", [(["A", "a", "中"], 8), (["a", "'", "s", "S"], 8), (TWELVE, 5)])
def test_every_small_string(items, longest):
    enc = [x.encode() for x in items]
    for n in range(1, longest + 1):
        for t in itertools.product(enc, repeat=n):
            same(b"".join(t))


def test_random_strings_and_random_bytes():
    rnd = random.Random(1)
    items = [x.encode() for x in TWELVE + ["ll", "RE", "ſ", "٣", "\r", " "]] + [b"\x80"]
    for _ in range(20000):
        same(b"".join(rnd.choice(items) for _ in range(rnd.randint(1, 64))))
    for _ in range(1000):
        same(bytes(rnd.randrange(256) for _ in range(rnd.randint(1, 64))))


@pytest.mark.parametrize("text,pieces", [
    ("A中Aa", ["A中Aa"]), ("A中A", ["A中", "A"]), ("A中AA中A", ["A中AA中", "A"]),
    ("it'sa", ["it's", "a"]), ("HE'LL", ["HE'LL"]), ("a's's's'sb", ["a's", "'s's", "'sb"]),
    ("A'S'S'Sb", ["A'S", "'S'S", "b"]), ("a'll's", ["a'll", "'s"]), ("ab'Sc'd", ["ab'S", "c'd"]), ("a'ſ", ["a'ſ"]),
    ("!́x", ["!́x"]), ("!!́x", ["!!́", "x"]), ("a!́́x", ["a", "!́́x"]),
    ("!!́́x", ["!!́́", "x"]), ("a//\n/x", ["a", "//\n/", "x"]), ("1234567", ["123", "456", "7"]),
])
def test_the_named_examples(text, pieces):
    data = text.encode()
    off = api.split_host(data, "o200k").tolist()
    assert [data[a:b].decode() for a, b in zip(off, off[1:])] == pieces
    same(data)


def test_specials_cut_the_text_into_segments():
    eot, rnd = b"<|endoftext|>", random.Random(2)
    items = [x.encode() for x in TWELVE] + [eot]
    for _ in range(2000):
        parts = [rnd.choice(items) for _ in range(rnd.randint(1, 40))]
        data, exp, at = b"".join(parts), [], 0
        for seg in data.split(eot):  # every segment's own starts, then the match behind it
            exp += [at + o for o in want(seg)[:-1]] + [at + len(seg)]
            at += len(seg) + len(eot)
        assert api.split_host_special(data, "o200k", [eot])[0].tolist() == exp, data


def test_the_preset_has_no_tables_and_the_case_classes_are_regex_s():
    assert api.SPLIT_PRESETS["o200k"] == 8
    with pytest.raises(api.BpeError, match="no tables"):
        api.split_rule("o200k")
    text = "".join(chr(c) for c in range(0x110000))
    exp = ["O"] * 0x110000
    for pat, k in ((r"[\p{Lu}\p{Lt}]", "U"), (r"\p{Ll}", "l"), (r"[\p{Lm}\p{Lo}]", "B"), (r"\p{M}", "M")):
        for m in regex.finditer(pat, text):
            exp[ord(m.group())] = k
    assert [api.unicode_case_class(c) for c in range(0x110000)] == exp
    assert api.unicode_case_class(0x110000) == "O"

"""Special tokens on the host (bpe_ex.h bpe_specials_check and bpe_split_offsets_host_special;
api.check_specials, api.split_host(..., specials)): the set's limits and its overlap-free
condition, and the split against the Python restatement of tests/special_ref.py, whose segments
go through the existing api.split_host(segment, rule) and, for "gpt2", also through the re pattern
of tests/test_split_gpt2_host.py.  No GPU."""
import functools
import itertools

import numpy as np
import pytest

import special_ref as R
from test_split_gpt2_host import re_offsets

from llmtokenizer_amd import api

EOT = b"<|endoftext|>"
RULES = ["lines", "words", "gpt2"]


@functools.lru_cache(maxsize=None)
def seg_host(seg, rule):
    """the existing split of a segment alone (the same few segments come back all the time)"""
    return tuple(api.split_host(seg, rule).tolist())


@functools.lru_cache(maxsize=None)
def seg_re(seg):
    return tuple(re_offsets(seg))


def check(data, specials, rules=RULES):
    for rule in rules:
        want, piece, index = R.restate(data, specials, lambda seg: seg_host(seg, rule))
        got, gp, gi = api.split_host_special(data, rule, specials)
        assert got.dtype == np.uint64
        assert got.tolist() == want.tolist(), (rule, data)
        assert gp.tolist() == piece.tolist() and gi.tolist() == index.tolist(), (rule, data)
        if rule == "gpt2":
            assert got.tolist() == R.restate(data, specials, seg_re)[0].tolist(), data


# ---------------------------------------------------------------- the set

@pytest.mark.parametrize("good", [R.GPT2_SET, R.CHATML_SET, R.RESERVED_SET, [], [b"\x01"], [b"x" + b"y" * 63]])
def test_accepted_sets(good):
    api.check_specials(good)


def test_the_limits():
    with pytest.raises(api.BpeError, match="at most 256"):
        api.check_specials([b"<%d>" % i for i in range(257)])
    api.check_specials([b"<%d>" % i for i in range(256)])
    with pytest.raises(api.BpeError, match="special 1 is 0 bytes"):
        api.check_specials([b"<a>", b""])
    with pytest.raises(api.BpeError, match="special 0 is 65 bytes"):
        api.check_specials([b"<" + b"y" * 63 + b">"])
    with pytest.raises(api.BpeError, match="NUL"):
        api.check_specials([b"<a>", b"<\0>"])


def test_the_overlap_free_condition_names_the_pair():
    with pytest.raises(api.BpeError, match=r"twice.*special 0 \"<a>\" and special 2 \"<a>\""):
        api.check_specials([b"<a>", b"<b>", b"<a>"])
    with pytest.raises(api.BpeError, match=r"substring.*special 1 \"b\|\" and special 0 \"<\|b\|>\""):
        api.check_specials([b"<|b|>", b"b|"])
    with pytest.raises(api.BpeError, match=r"suffix.*special 0 \"aa\" and special 0 \"aa\""):
        api.check_specials([b"aa"])
    with pytest.raises(api.BpeError, match=r"suffix.*special 0 \"<a>\" and special 1 \"><\""):
        api.check_specials([b"<a>", b"><"])
    with pytest.raises(api.BpeError, match="suffix"):
        api.check_specials([b"abab"])
    with pytest.raises(api.BpeError, match="suffix"):
        api.check_specials([b"<|x|>", b"|>y"])
    # every call that takes specials refuses such a set, on the host
    with pytest.raises(api.BpeError, match="suffix"):
        api.split_host(b"aaa", "words", [b"aa"])


# ---------------------------------------------------------------- the split

def test_the_three_examples():
    def pieces(data):
        off = api.split_host(data, "gpt2", [EOT]).tolist()
        return [data[a:b] for a, b in zip(off, off[1:])]
    assert pieces(b"a  " + EOT) == [b"a", b"  ", EOT]
    assert pieces(EOT + b"'s") == [EOT, b"'s"]
    assert pieces(b"x" + EOT + b" y") == [b"x", EOT, b" y"]
    for t in (b"a  " + EOT, EOT + b"'s", b"x" + EOT + b" y"):
        check(t, [EOT])
        for rule in RULES:  # (split_host with specials is split_host_special's offsets)
            assert api.split_host(t, rule, [EOT]).tolist() == api.split_host_special(t, rule, [EOT])[0].tolist()
    # without the special the same bytes are cut inside it
    off = api.split_host(b"x" + EOT, "gpt2").tolist()
    assert [(b"x" + EOT)[a:b] for a, b in zip(off, off[1:])] == [b"x", b"<|", b"endoftext", b"|>"]


def test_every_short_string_over_seven_symbols():
    symbols = [b"<|e|>", b"'", b"s", b" ", b"\n", b"a", b"1"]
    for n in range(7):
        for t in itertools.product(symbols, repeat=n):
            check(b"".join(t), [b"<|e|>"])


def test_random_strings_with_specials_spliced_in():
    rng = np.random.default_rng(21)
    alphabet = np.frombuffer(b"'''stredvml  \n\t\raZ09!,.<|>\x7f\x80\xc3\xa9\xff", np.uint8)
    sets = [R.GPT2_SET, R.CHATML_SET, [b"<|e|>", b"\x01"], [b"!."]]
    for k in range(50000):
        specials = sets[k % len(sets)]
        parts = []
        room = 40
        while room > 0:
            if rng.integers(0, 3) == 0:
                s = specials[int(rng.integers(0, len(specials)))]
                if len(s) > room:
                    break
                parts.append(s)
                room -= len(s)
            else:
                m = int(rng.integers(0, min(room, 8) + 1))
                parts.append(rng.choice(alphabet, m).tobytes())
                room -= max(m, 1)
        check(b"".join(parts), specials, rules=[RULES[k % 3]])


def test_matches_at_the_ends_adjacent_and_short_segments():
    sp = [EOT, b"<|im_end|>"]
    check(EOT, sp)
    check(EOT + b"abc", sp)
    check(b"abc" + EOT, sp)
    check(EOT + EOT + sp[1] + EOT, sp)
    check(b"a" + EOT + sp[1] + b"b", sp)
    for fill in (b"a's  \n x", b"  \n\n 's", b"'ll 1 "):
        for n in range(1, 6):
            seg = (fill * 2)[:n]
            check(EOT + seg + sp[1] + seg + EOT + seg, sp)
            check(seg + EOT + seg + EOT, sp)


def test_a_text_ending_in_every_proper_prefix_of_a_special():
    for k in range(1, len(EOT)):
        for head in (b"", b"a ", EOT, b"x" + EOT + b" "):
            data = head + EOT[:k]
            check(data, [EOT])
            assert R.matches(data, [EOT]) == R.matches(head, [EOT])


def test_one_byte_and_64_byte_specials():
    one, long = b"\x01", b"<" + b"0123456789" * 6 + b"ab>"
    assert len(long) == 64
    sp = [one, long]
    check(one, sp)
    check(long, sp)
    check(one * 5, sp)
    check(b"a" + one + b" b" + long + one + b"'s" + long[:63] + one + long, sp)
    check(long + long[:63], sp)


def test_table_rules_and_the_empty_set():
    rng = np.random.default_rng(22)
    for seed in (1, 2):
        cls, brk = R.random_rule(seed)
        for _ in range(200):
            t = rng.choice(np.frombuffer(b"ab <|e>\n", np.uint8), int(rng.integers(0, 60))).tobytes()
            t = t.replace(b"<<", b"<|e|>")
            want = R.restate(t, [b"<|e|>"], R.table_split(cls, brk))[0]
            assert api.split_host(t, (cls, brk), [b"<|e|>"]).tolist() == want.tolist()
            assert api.split_host(t, (cls, brk), []).tolist() == R.table_split(cls, brk)(t).tolist()
    for rule in RULES:  # no specials: today's offsets
        for t in (b"", b"x", b"a  <|endoftext|>'s"):
            assert api.split_host(t, rule, []).tolist() == api.split_host(t, rule).tolist()
    with pytest.raises(api.BpeError):
        api.split_host(b"abc", "gpt3", [EOT])

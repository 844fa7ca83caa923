"""Text batches on the host (llmtokenizer_amd/src/bpe_texts.c through api.check_texts and api.texts_gap):
every refusal of the offsets' check with the offending index in its message, the gapped bytes against numpy,
and the Python restatement of the batch's split (tests/texts_ref.py) against the single-text split it is made
of.  The last two tests hold tests/texts_ref.py, the yardstick of tests/test_gpu_texts.py, to api.split_host and
call nothing new: they check the reference, not the feature.  CPU only."""
import numpy as np
import pytest

import texts_ref as R
from llmtokenizer_amd import api
from llmtokenizer_amd.api import BpeError

LIMIT = 0xFFFFFFFE


def test_offsets_accepted():
    for off, n in ([0], 0), ([0, 0, 0], 0), ([0, 5], 5), ([0, 0, 3, 3, 7], 7), ([0, LIMIT - 1], LIMIT - 1):
        assert api.check_texts(off, n).tolist() == off


@pytest.mark.parametrize("off, n, words", [
    ([1, 5], 5, ["offset 0 ", "is 1"]),
    ([0, 4, 3, 9], 9, ["offset 2 (3)", "offset 1 (4)"]),
    ([0, 4, 4, 2], 2, ["offset 3 (2)", "offset 2 (4)"]),
    ([0, 4, 8], 9, ["offset 2", "is 8", "bytes 9"]),
    ([0, 4, 10], 9, ["offset 2", "is 10", "bytes 9"]),
    ([0], 3, ["offset 0", "bytes 3"]),
    ([0, LIMIT], LIMIT, ["4294967294 bytes and 1 gap"]),
    ([0, 0, LIMIT - 1], LIMIT - 1, ["4294967293 bytes and 2 gap"]),
])
def test_offsets_refused_with_the_index(off, n, words):
    with pytest.raises(BpeError) as e:
        api.check_texts(off, n)
    assert str(e.value).startswith("texts: ")
    for w in words:
        assert w in str(e.value), str(e.value)


def test_no_offsets_at_all():
    with pytest.raises(BpeError):
        api.check_texts([], 0)


@pytest.mark.parametrize("texts", [
    [], [b""], [b"", b"", b""], [b"abc"], [b"a", b"", b"bc", b"", b"", b"d\0e", b""],
    [bytes([k % 256]) * (k % 5) for k in range(300)],
])
def test_gapped_bytes_equal_numpy(texts):
    off = R.byte_offsets(texts)
    data = b"".join(texts)
    got = api.texts_gap(data, off)
    want = np.insert(np.frombuffer(data, dtype=np.uint8), off[1:].astype(np.int64), 0).tobytes()
    assert got == want == R.gapped(texts)


def test_gapped_stretches_equal_slices():
    texts = [b"a", b"", b"bcd", b"", b"", b"e\0f", b"", b"ghijklmnop"]
    off, data, whole = R.byte_offsets(texts), b"".join(texts), R.gapped(texts)
    for lo in range(len(whole) + 1):
        for hi in range(lo, len(whole) + 1):
            assert api.texts_gap(data, off, lo, hi) == whole[lo:hi], (lo, hi)
    for lo, hi in ((3, 2), (0, len(whole) + 1)):
        with pytest.raises(BpeError):
            api.texts_gap(data, off, lo, hi)


def test_gapped_bytes_refuse_bad_offsets():
    with pytest.raises(BpeError):
        api.texts_gap(b"abc", [0, 2, 1, 3])


@pytest.mark.parametrize("rule", ["words", "gpt2", "gpt2_unicode", "cl100k"])
def test_reference_is_the_single_text_split_per_text(rule):
    texts = [b"it", b"'s 1234", b"", b"567 a  ", b"b\n\n", "éx".encode()[:1], "éx".encode()[1:]]
    off, per_text, special = R.split_texts(texts, rule)
    assert special == [] and per_text[2] == 0 and int(off[-1]) == sum(len(t) for t in texts)
    at, base = 0, 0
    for t, k in zip(texts, per_text):
        if t:
            assert (off[at:at + k + 1] - np.uint64(base) == api.split_host(t, rule)).all()
        at, base = at + int(k), base + len(t)
    # joined, the texts split otherwise: "it" + "'s" is one piece under gpt2, and the digit runs join
    if rule != "words":
        assert off.tolist() != api.split_host(b"".join(texts), rule).tolist()


def test_reference_with_specials():
    sp = [b"<|endoftext|>"]
    texts = [b"a<|endof", b"text|>b", b"x<|endoftext|>", b"<|endoftext|>y"]
    off, per_text, special = R.split_texts(texts, "gpt2", sp)
    assert [j for _, j in special] == [0, 0] and len(special) == 2
    pieces = [b"".join(texts)[int(a):int(b)] for a, b in zip(off[:-1], off[1:])]
    assert [pieces[p] for p, _ in special] == sp * 2
    assert api.split_host(b"".join(texts), "gpt2", sp).size != off.size  # (joined, the cut special matches)

"""BPE_TEXT_REPLACE / BPE_TEXT_HOLD on the host (src/bpe_utf8.c over src/bpe_utf8_rule.h; the contract: include/bpe_gpu.h,
"Decoded text"): api.utf8_repair_host against CPython's two definitions, bytes.decode("utf-8", "replace") and the
incremental decoder with final=False, on a fixed list of edge cases, on random strings over the bytes where Table 3-7
turns, and on the same strings as one text batch.  No GPU."""
import codecs
import itertools

import numpy as np
import pytest

from llmtokenizer_amd import api

LEADS = [b"\xC2", b"\xDF", b"\xE0", b"\xE1", b"\xED", b"\xEF", b"\xF0", b"\xF1", b"\xF4"]
# every boundary of Table 3-7, the classic ill-formed forms, stray continuation bytes in runs of 1 .. 5 ...
FIXED = [bytes.fromhex(h) for h in (
    "", "41", "C1", "C180", "C2", "C280", "DFBF", "E09F80", "E0A080", "ED9FBF", "EDA080", "EFBFBF", "F08F8080",
    "F0908080", "F48FBFBF", "F4908080", "F5", "F580", "FF", "F080", "E08080", "EDA080", "C0AF", "F88080")]
FIXED += [b"A" + b"\x80" * k + b"B" for k in range(1, 6)] + [b"\xBF" * k for k in range(1, 6)]
# ... and each lead followed by 0, 1, ... valid continuation bytes, then a bad byte, then the text's end
for lead in LEADS:
    second = {b"\xE0": b"\xA0", b"\xED": b"\x9F", b"\xF0": b"\x90", b"\xF4": b"\x8F"}.get(lead, b"\x80")
    for k in range(4):
        seq = lead + (second + b"\x80" * 3)[:k]
        FIXED += [seq, seq + b"A", seq + b"\xFF", b"z" + seq + lead]
ALPHABET = bytes.fromhex("41809FA0BFC2E0EDF0F4FF")


def cpython(b, errors):
    """(text, held) by CPython"""
    if errors == "replace":
        return b.decode("utf-8", "replace").encode("utf-8"), 0
    d = codecs.getincrementaldecoder("utf-8")("replace")
    return d.decode(b, final=False).encode("utf-8"), len(d.getstate()[0])


def random_strings():
    rng = np.random.default_rng(20240607)
    return [bytes(rng.choice(np.frombuffer(ALPHABET, np.uint8), rng.integers(0, 13))) for _ in range(4000)]


def check_batch(texts, errors, repair):
    """repair(joined bytes, offsets, errors) against CPython text by text: bytes, offsets and held"""
    off = np.concatenate([[0], np.cumsum([len(t) for t in texts])]).astype(np.uint64)
    want = [cpython(t, errors) for t in texts]
    out, bo, held = repair(b"".join(texts), off, errors)
    assert bo.dtype == np.uint64 and held.dtype == np.uint32 and held.shape == (len(texts),)
    assert np.array_equal(bo, np.concatenate([[0], np.cumsum([len(w) for w, _ in want])]))
    assert out == b"".join(w for w, _ in want)
    assert held.tolist() == [h for _, h in want]


@pytest.mark.parametrize("errors", ["replace", "hold"])
@pytest.mark.parametrize("strings", [FIXED, random_strings()], ids=["fixed", "random"])
def test_one_text_equals_cpython(strings, errors):
    for s in strings:
        out, bo, held = api.utf8_repair_host(s, None, errors)
        assert (out, int(held[0])) == cpython(s, errors) and bo is None and held.shape == (1,), s.hex()


@pytest.mark.parametrize("errors", ["replace", "hold"])
def test_texts_do_not_join(errors):
    """every string as a text of one batch, and a 4-byte character cut at every position with empty texts between:
    a lead at a text's end and the continuation bytes behind it are never one character, and held is per text"""
    cut = "\U0001F600".encode()
    pieces = list(itertools.chain.from_iterable((cut[:k], b"", cut[k:], b"") for k in range(5)))
    check_batch(pieces + FIXED + random_strings() + pieces, errors, api.utf8_repair_host)
    check_batch([], errors, api.utf8_repair_host)


def test_raw_and_refusals():
    s = b"".join(FIXED)
    off = np.array([0, 3, 3, len(s)], dtype=np.uint64)
    out, bo, held = api.utf8_repair_host(s, off, None)
    assert out == s and np.array_equal(bo, off) and not held.any()
    for bad in ([1, len(s)], [0, 5, 4, len(s)], [0, len(s) - 1]):
        with pytest.raises(api.BpeError, match="invalid argument"):
            api.utf8_repair_host(s, bad, "replace")
    with pytest.raises(api.BpeError, match="errors must be"):
        api.utf8_repair_host(s, None, "strict")

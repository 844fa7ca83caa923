"""Token spans on the host (llmtokenizer_amd/src/bpe_spans.c through api.span_lens and api.token_spans_host; no
GPU): the length table against Vocab.token_bytes() with and without a vocabulary with holes, the spans against
the pure-Python reference (tests/spans_ref.py) in both units and against the character offsets `tokenizers`
recorded (tests/golden/vocab/spans_*.json), the refusals by code and message, texts that are no UTF-8, no text
and empty texts."""
import json
import os

import numpy as np
import pytest

import golden_lib as G
import spans_ref as SR
from llmtokenizer_amd import api
from llmtokenizer_amd.api import BpeError
from llmtokenizer_amd.vocab import Vocab

FIXTURES = ["spans_gpt2u", "spans_cl100k"]


def load_fixture(name, tmp_path):
    """(the recorded fixture, its Vocab)"""
    with open(os.path.join(G.GOLD, "vocab", name + ".json"), encoding="utf-8") as f:
        fx = json.load(f)
    with open(os.path.join(G.GOLD, "vocab", fx["vocab"] + ".json"), encoding="utf-8") as f:
        tj = json.load(f)["tokenizer_json"]
    p = tmp_path / "tokenizer.json"
    p.write_text(json.dumps(tj, ensure_ascii=False), encoding="utf-8")
    return fx, Vocab.from_tokenizer_json(p)


def join(texts):
    """(the texts' bytes joined, their byte offsets)"""
    raw = [t.encode("utf-8") if isinstance(t, str) else bytes(t) for t in texts]
    return b"".join(raw), np.concatenate([[0], np.cumsum([len(t) for t in raw])]).astype(np.uint64), raw


# a small list of its own: 256 = "ab", 257 = "abc", 258 = E2 82, 259 = the euro sign, 260 = NUL NUL
MERGES = np.array([[0x61, 0x62], [256, 0x63], [0xE2, 0x82], [258, 0xAC], [0, 0]], dtype=np.uint32)
SPECIALS = [b"<s>", b"<|e|>"]


def test_span_lens_internal_ids():
    lens = api.span_lens(MERGES, SPECIALS)
    want = [len(t) for t in SR.internal_token_bytes(MERGES, SPECIALS)]
    assert lens.dtype == np.uint32 and lens.tolist() == want
    assert lens[0] == 1 and lens[260] == 2  # NUL counts: a byte of the text like any other
    assert api.span_lens(MERGES).tolist() == want[:-2]
    assert api.span_lens(np.zeros((0, 2), dtype=np.uint32)).tolist() == [1] * 256


@pytest.mark.parametrize("name", FIXTURES)
def test_span_lens_vocabulary_with_holes(name, tmp_path):
    _, v = load_fixture(name, tmp_path)
    lens = api.span_lens(v.merges, v.specials, vocab=v)
    token_of = SR.token_bytes_by_id(v)
    assert lens.size == v.size and lens.size > len(token_of)  # (holes)
    want = np.zeros(v.size, dtype=np.uint32)
    for i, t in token_of.items():
        want[i] = len(t)
    assert (lens == want).all() and (lens == 0).sum() == v.size - len(token_of)
    internal = api.span_lens(v.merges, v.specials)
    assert internal.tolist() == [len(t) for t in v.token_bytes()] + [len(s) for s in v.specials]


@pytest.mark.parametrize("name", FIXTURES)
def test_recorded_offsets_and_reference(name, tmp_path):
    """every fixture text alone and all of them as one batch: the char unit is what `tokenizers` recorded, both
    units are what the Python reference says"""
    fx, v = load_fixture(name, tmp_path)
    assert len(fx["texts"]) >= 42
    lens = api.span_lens(v.merges, v.specials, vocab=v)
    token_of = SR.token_bytes_by_id(v)
    for text, ids, off in zip(fx["texts"], fx["ids"], fx["offsets"]):
        raw = text.encode("utf-8")
        got = api.token_spans_host(ids, [0, len(ids)], raw, [0, len(raw)], lens, "char")
        assert got.dtype == np.uint32 and got.shape == (len(ids), 2) and got.tolist() == off, repr(text)
        got = api.token_spans_host(ids, [0, len(ids)], raw, [0, len(raw)], lens, "byte")
        assert got.tolist() == [list(s) for s in SR.spans_of_text([token_of[i] for i in ids], raw, "byte")]
    data, boff, raw = join(fx["texts"])
    ids = np.array([i for x in fx["ids"] for i in x], dtype=np.uint32)
    toff = np.concatenate([[0], np.cumsum([len(x) for x in fx["ids"]])])
    got = api.token_spans_host(ids, toff, data, boff, lens, "char")
    assert got.tolist() == [o for x in fx["offsets"] for o in x]
    for unit in ("byte", "char"):
        assert (api.token_spans_host(ids, toff, data, boff, lens, unit) == SR.batch_spans(token_of, ids, toff, raw, unit)).all()


def test_not_utf8_the_clamp_holds():
    lens = api.span_lens(MERGES, SPECIALS)
    for text, ids in ((b"\x80\x80a", [0x80, 0x80, 0x61]), (b"\xe2\x82", [258]), (b"\xe2\x82", [0xE2, 0x82]),
                      (b"\xac\xe2\x82\xac\x80", [0xAC, 259, 0x80]), (b"\x00\x00\x00", [260, 0])):
        toks = [SR.internal_token_bytes(MERGES, SPECIALS)[i] for i in ids]
        for unit in ("byte", "char"):
            got = api.token_spans_host(ids, [0, len(ids)], text, [0, len(text)], lens, unit)
            assert got.tolist() == [list(s) for s in SR.spans_of_text(toks, text, unit)], (text, unit)
            assert got.max() <= len(text)  # nothing wrapped
    assert api.token_spans_host([0x80, 0x80, 0x61], [0, 3], b"\x80\x80a", [0, 3], lens, "char").tolist() == [[0, 0], [0, 0], [0, 1]]
    assert api.token_spans_host([258], [0, 1], b"\xe2\x82", [0, 2], lens, "char").tolist() == [[0, 1]]


def test_no_text_and_empty_texts():
    lens = api.span_lens(MERGES)
    for unit in ("byte", "char"):
        assert api.token_spans_host([], [0], b"", [0], lens, unit).shape == (0, 2)
        assert api.token_spans_host([], [0, 0, 0, 0], b"", [0, 0, 0, 0], lens, unit).shape == (0, 2)
        got = api.token_spans_host([257, 0x61], [0, 0, 1, 1, 2, 2], b"abca", [0, 0, 3, 3, 4, 4], lens, unit)
        assert got.tolist() == [[0, 3], [0, 1]]


def test_refusals_by_code_and_message():
    bad = MERGES.copy()
    bad[1, 0] = 300  # merge 1 names an id that does not exist yet
    with pytest.raises(BpeError, match=r"invalid argument.*merge 1 names the id 300"):
        api.span_lens(bad)
    bad[1, 0] = 257  # ... its own
    with pytest.raises(BpeError, match=r"merge 1 names the id 257"):
        api.span_lens(bad)
    dbl = np.array([[0x61, 0x61]] + [[255 + r, 255 + r] for r in range(1, 33)], dtype=np.uint32)
    assert api.span_lens(dbl[:31])[-1] == 1 << 31
    with pytest.raises(BpeError, match=r"out of range.*merge 31 makes a token of 4294967296 bytes"):
        api.span_lens(dbl)
    lens = api.span_lens(MERGES, SPECIALS)
    with pytest.raises(BpeError, match=r"corrupt merge list \(spans: unknown token id 263 at index 1 \(text 0\)"):
        api.token_spans_host([257, 263], [0, 2], b"abcd", [0, 4], lens)
    with pytest.raises(BpeError, match=r"corrupt merge list \(spans: the ids of text 1 have lengths that sum to 3, the text holds 2 bytes"):
        api.token_spans_host([257, 257], [0, 1, 2], b"abcab", [0, 3, 5], lens, "char")
    with pytest.raises(BpeError, match=r"the ids of text 0 have lengths that sum to 3, the text holds 4 bytes"):
        api.token_spans_host([257, 0x61], [0, 1, 2], b"abcab", [0, 4, 5], lens)  # (the total is right, the texts are not)
    with pytest.raises(BpeError, match="id offsets"):
        api.token_spans_host([257], [0, 2], b"abc", [0, 3], lens)
    with pytest.raises(BpeError, match="byte offsets"):
        api.token_spans_host([257], [0, 1], b"abc", [0, 2], lens)
    with pytest.raises(BpeError, match="unit"):
        api.token_spans_host([257], [0, 1], b"abc", [0, 3], lens, "word")
    assert api.span_info()["per_thread"] >= 1

"""Text batches on the device (texts.hip, bpe_gpu_load_texts / _fetch_text_offsets / _pack_texts,
Engine.load_texts, Tokenizer.encode_batch / decode_batch): the pieces of a batch against the per-text host
split (tests/texts_ref.py), its ids and text_off against a loop of Tokenizer.encode over the 300-merge
vocabularies of tests/golden/vocab, breaks placed around every step of the split kernels, empty texts, the
state rules, and the packed rows against numpy."""
import json
import os

import numpy as np
import pytest

import golden_lib as G
import texts_ref as R
from llmtokenizer_amd import api
from llmtokenizer_amd.api import BpeError
from llmtokenizer_amd.synth import english_like
from llmtokenizer_amd.vocab import Tokenizer, Vocab

pytestmark = pytest.mark.gpu

ESTATE, EINVAL = "call out of order", "invalid argument"
RULES = ["words", "gpt2", "gpt2_unicode", "cl100k"]
STEP, WAVE, TILE, GB = 16, 1024, 4096, 4096 * 2048  # a thread's bytes, a wave's (the count tile), the marking tile, a grid step
EOT = b"<|endoftext|>"
# text that every rule has something to say about, the specials of the vocabularies included
SRC = (english_like(3000) + b" 12345678 it's IT'S  \n\n \t\xc3\xa9\xe2\x82\xac\xf0\x9f\x98\x80 " + EOT + b"<|im_start|>x\0y ") * 3000


@pytest.fixture(scope="module")
def vocabs(tmp_path_factory):
    """{(rule, with specials)}: the golden vocabularies; "words" and "gpt2" number vocab_gpt2u's merges"""
    out = {}
    for name in ("vocab_gpt2u", "vocab_cl100k"):
        with open(os.path.join(G.GOLD, "vocab", name + ".json"), encoding="utf-8") as f:
            fx = json.load(f)
        p = tmp_path_factory.mktemp("vocab") / (name + ".json")
        p.write_text(json.dumps(fx["tokenizer_json"], ensure_ascii=False), encoding="utf-8")
        v = Vocab.from_tokenizer_json(p)
        assert v.merges.shape[0] == 300 and v.specials == [EOT, b"<|im_start|>"]
        for rule in ([v.rule] if v.rule == "cl100k" else ["words", "gpt2", "gpt2_unicode"]):
            out[rule, True] = Vocab(v.merges, v.byte_ids, v.merge_ids, v.special_ids, v.specials, rule)
            out[rule, False] = Vocab(v.merges, v.byte_ids, v.merge_ids, [], [], rule)
    return out


@pytest.fixture(scope="module")
def toks(vocabs):
    """per vocabulary the tokenizer under test and another one, with an engine of its own, for the per-text loop"""
    t = {k: (Tokenizer(v), Tokenizer(v)) for k, v in vocabs.items()}
    yield t
    for a, b in t.values():
        a.close()
        b.close()


@pytest.fixture(scope="module")
def eng():
    e = api.Engine(0)
    yield e
    e.close()


_single = {}  # (rule, specials?, text) -> (ids, id offsets of its pieces): Tokenizer.encode of one text, computed once


def single(toks, rule, sp, text):
    key = (rule, sp, text)
    if key not in _single:
        ids, doc_off, _ = toks[rule, sp][1].encode(text, return_offsets=True)
        _single[key] = (ids.copy(), doc_off.copy())
    return _single[key]


def check_batch(toks, rule, sp, texts):
    """the whole contract for one batch; returns (ids, text_off)"""
    tok = toks[rule, sp][0]
    texts = R.as_bytes(texts)
    ids, toff = tok.encode_batch(texts)
    assert ids.dtype == np.uint32 and toff.dtype == np.uint64 and toff.size == len(texts) + 1
    want_ids, want_doc, at = [], [0], 0
    for t in texts:
        if t:  # (an empty text has no id)
            i, d = single(toks, rule, sp, t)
            want_ids.append(i)
            want_doc += (d[1:] + np.uint64(at)).tolist()
            at += i.size
    lens = [single(toks, rule, sp, t)[0].size if t else 0 for t in texts]
    assert toff.tolist() == np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64).tolist()
    assert np.array_equal(ids, np.concatenate(want_ids) if want_ids else np.zeros(0, dtype=np.uint32))
    e = tok._eng()
    off, per_text, special = R.split_texts(texts, rule, tok.vocab.specials if sp else None)
    assert np.array_equal(e.split_offsets(), off)
    assert np.array_equal(e.doc_offsets(), np.array(want_doc, dtype=np.uint64))
    piece, index = e.special_pieces()
    assert list(zip(piece.tolist(), index.tolist())) == special
    assert e.split_special_info()["matches"] == len(special)
    return ids, toff


# ---------------------------------------------------------------- what a break must keep apart

def _cut_characters():
    out = []
    for ch in ("é", "€", "😀"):
        b = ch.encode("utf-8")
        out += [[b"a" + b[:i], b[i:] + b"z"] for i in range(1, len(b))]
    return out


AROUND = [
    ["1234", "567"], ["it", "'s"], ["IT", "'S"], ["a  ", "b"], ["!\n", "\n\n"], [" ", "x"],
    ["<|endof", "text|>"], [b"x" + EOT, "y"], ["x", EOT + b"y"], [EOT, EOT, b" " + EOT + b" "],
    [b"a\0b", b"\0", b"c\0", b"\0\0d"], ["don", "'t  ", " 12", "3\n", "\n x"],
] + _cut_characters()


@pytest.mark.parametrize("sp", [False, True], ids=["plain", "specials"])
@pytest.mark.parametrize("rule", RULES)
def test_texts_around_a_break(toks, rule, sp):
    for texts in AROUND:
        check_batch(toks, rule, sp, texts)
    check_batch(toks, rule, sp, [t for texts in AROUND for t in R.as_bytes(texts)])


def test_a_break_changes_what_the_join_would_give(toks):
    """the cases are cases: joined, the same bytes encode otherwise"""
    t0 = toks["cl100k", True][1]
    for texts in (["1234", "567"], ["<|endof", "text|>"], ["a  ", "b"]):
        joined = t0.encode("".join(texts)).tolist()
        ids, _ = toks["cl100k", True][0].encode_batch(texts)
        assert ids.tolist() != joined


# ---------------------------------------------------------------- where a break may fall

def texts_with_gaps_at(positions, end):
    """texts of SRC whose gap bytes land on the resident positions given (ascending), the last gap at end"""
    texts, prev, at = [], -1, 0
    for g in list(positions) + [end]:
        n = g - prev - 1
        assert n >= 0
        texts.append(SRC[at:at + n])
        at, prev = at + n, g
    return texts


@pytest.mark.parametrize("d", range(-8, 9))
@pytest.mark.parametrize("rule", RULES)
def test_breaks_around_the_kernels_steps(toks, rule, d):
    pos = sorted({5 * STEP + d, WAVE + d, TILE + d, 2 * TILE + WAVE + d, 3 * TILE + d})
    texts = texts_with_gaps_at(pos, 3 * TILE + 700)
    assert R.gapped(texts)[pos[2]] == 0 and len(R.gapped(texts)) == 3 * TILE + 701
    check_batch(toks, rule, True, texts)


@pytest.mark.parametrize("rule", RULES)
def test_breaks_around_a_grid_step(toks, rule):
    assert api.split_info() == {"tile": TILE, "grid_bytes": GB}
    texts = texts_with_gaps_at([GB - 8, GB - 1, GB, GB + 1, GB + 8], GB + 5000)
    check_batch(toks, rule, True, texts)


def test_no_text_and_one_text(toks):
    for rule in RULES:
        ids, toff = check_batch(toks, rule, True, [])
        assert ids.size == 0 and toff.tolist() == [0]
        one = SRC[:5000]
        ids, toff = check_batch(toks, rule, True, [one])
        assert ids.tolist() == toks[rule, True][1].encode(one).tolist() and toff.tolist() == [0, ids.size]


@pytest.mark.parametrize("rule", RULES)
def test_empty_texts(toks, rule):
    a, b = SRC[:300], SRC[300:700]
    for texts in ([b"", a, b], [a, b, b""], [a, b"", b], [a, b"", b"", b"", b], [b"", b"", a, b"", b"", b"", b, b""],
                  [b""], [b"", b"", b"", b""]):
        for sp in (False, True):
            ids, toff = check_batch(toks, rule, sp, texts)
            assert [int(toff[k + 1] - toff[k]) == 0 for k in range(len(texts))] == [not t for t in texts]


@pytest.mark.parametrize("rule, sp", [("gpt2_unicode", True), ("cl100k", False), ("words", True)])
def test_many_one_byte_texts(toks, rule, sp):
    """70,000 breaks: more than the match list's first room (n / 256 + 1024 entries)"""
    raw = np.random.default_rng(5).integers(0, 256, 70000, dtype=np.uint8)
    texts = [bytes([b]) for b in raw.tolist()]
    tok = toks[rule, sp][0]
    ids, toff = tok.encode_batch(texts)
    one = np.array([single(toks, rule, sp, bytes([b]))[0] for b in range(256)], dtype=np.uint32)
    assert one.shape == (256, 1)
    assert (toff == np.arange(70001, dtype=np.uint64)).all() and (ids == one[raw, 0]).all()
    e = tok._eng()
    assert (e.split_offsets() == np.arange(70001, dtype=np.uint64)).all()
    assert (e.doc_offsets() == np.arange(70001, dtype=np.uint64)).all()
    assert e.special_pieces()[0].size == 0


def test_more_texts_than_a_grid_of_the_per_text_kernels(toks):
    """600,000 one-byte texts: the per-break kernels (2,048 workgroups of 256 threads) walk them in grid strides,
    and so does the pack over rows at a row length whose workgroups hold few rows (65,535 workgroups of 4 rows)"""
    import torch
    rule, sp, T = "cl100k", True, 600000
    raw = np.random.default_rng(6).integers(0, 256, T, dtype=np.uint8)
    tok = toks[rule, sp][0]
    ids, toff = tok.encode_batch([bytes([b]) for b in raw.tolist()])
    one = np.array([single(toks, rule, sp, bytes([b]))[0] for b in range(256)], dtype=np.uint32)
    assert (toff == np.arange(T + 1, dtype=np.uint64)).all() and (ids == one[raw, 0]).all()
    e = tok._eng()
    assert (e.split_offsets() == np.arange(T + 1, dtype=np.uint64)).all()
    assert (e.doc_offsets() == np.arange(T + 1, dtype=np.uint64)).all()
    rows, lens = e.pack_texts(1, 7)
    assert rows.shape == (T, 1) and (rows[:, 0] == ids).all() and (lens == 1).all()
    out = torch.zeros((T, 256), dtype=torch.int32, device=torch.device("cuda", 0))
    rows, lens = e.pack_texts(256, 0x7FFFFFF0, "left", out=out)
    want = torch.from_numpy(ids.astype(np.int32)).to(out.device)
    assert bool((rows[:, 0] == want).all()) and bool((rows[:, 1:] == 0x7FFFFFF0).all()) and bool((lens == 1).all())


# ---------------------------------------------------------------- state

def test_refusals_and_lifetime(eng, vocabs):
    v = vocabs["cl100k", True]
    data = SRC[:20000]
    with pytest.raises(BpeError, match=ESTATE):  # (no text batch yet)
        eng.load(data)
        eng.text_offsets()
    texts = [data[:7000], b"", data[7000:]]
    assert eng.load_texts(texts) == 3
    for call, word in ((lambda: eng.encode(v.merges), "encode: the context holds a text batch"),
                       (lambda: eng.train(10), "train: the context holds a text batch"),
                       (lambda: eng.encode_docs([0, len(data) + 3], v.merges), "encode_docs: the context holds a text batch"),
                       (lambda: eng.text_offsets(), "encode_split first"),
                       (lambda: eng.pack_texts(8, 0), "encode_split first")):
        with pytest.raises(BpeError, match=ESTATE) as e:
            call()
        assert word in str(e.value)
    pieces = eng.split("cl100k", v.specials)
    with pytest.raises(BpeError, match=ESTATE) as e:
        eng.train_split(10)
    assert "train_split: the context holds a text batch" in str(e.value)
    with pytest.raises(BpeError, match=EINVAL) as e:  # 256 specials: index 255 is the break's
        eng.split("cl100k", [b"<%03d>" % k for k in range(256)])
    assert "at most 255 specials" in str(e.value) and "BPE_GPU_TEXT_BREAK" in str(e.value)
    assert eng.split("cl100k", [b"<%03d>" % k for k in range(255)]) > 0
    # split_offsets: the plain join's coordinates, the pieces of the per-text split
    assert eng.split("cl100k", v.specials) == pieces
    off, _, special = R.split_texts(texts, "cl100k", v.specials)
    assert eng.split_offsets().tolist() == off.tolist() and pieces == off.size - 1 and int(off[-1]) == len(data)
    eng.encode_split(v.merges)
    first = eng.ids().copy()
    assert eng.text_offsets()[-1] == first.size and eng.doc_offsets().size == pieces + 1
    with pytest.raises(BpeError, match=EINVAL) as e:
        eng.pack_texts(0, 0)
    assert "row_len is 0" in str(e.value)
    # a second split by another rule over the same batch
    p2 = eng.split("gpt2", v.specials)
    off2, _, _ = R.split_texts(texts, "gpt2", v.specials)
    assert p2 == off2.size - 1 and eng.split_offsets().tolist() == off2.tolist()
    eng.encode_split(v.merges)
    assert eng.text_offsets().size == 4
    # the breaks die on load: the same context encodes what the one-call path encodes, and is no text batch
    eng.load(data)
    eng.split("cl100k", v.specials)
    eng.encode_split(v.merges)
    want, want_ido, want_bo = api.encode_split(data, v.merges, "cl100k", specials=v.specials)
    assert eng.ids_checksum() == G.ids_checksum(want) and eng.split_offsets().tolist() == want_bo.tolist()
    assert eng.doc_offsets().tolist() == want_ido.tolist()
    for call in (eng.text_offsets, lambda: eng.pack_texts(8, 0)):
        with pytest.raises(BpeError, match=ESTATE) as e:
            call()
        assert "no text batch" in str(e.value)
    eng.encode(v.merges)  # (and the calls a text batch refuses work again)


def test_offsets_refused_by_the_load(eng):
    L, vp = eng.L, __import__("ctypes").c_void_p
    buf = np.frombuffer(b"abcdef", dtype=np.uint8)
    off = np.array([0, 4, 3, 6], dtype=np.uint64)
    rc = L.bpe_gpu_load_texts(eng.ctx, buf.ctypes.data_as(vp), buf.size, off.ctypes.data_as(vp), 3)
    assert L.bpe_gpu_strerror(rc).decode() == EINVAL
    assert "offset 2 (3) is below offset 1 (4)" in L.bpe_gpu_last_error().decode()


# ---------------------------------------------------------------- rows

PAD_BYTES = np.arange(0xF5, 0x100, dtype=np.uint8)  # bytes no UTF-8 text holds, so no merge names them: one id each


def texts_of_lengths(lens, seed=3):
    """texts whose id counts are exactly lens: letters under "words" (one piece), every byte one id"""
    rng = np.random.default_rng(seed)
    return [rng.choice(PAD_BYTES, n).tobytes() for n in lens]


def load_lengths(eng, v, lens):
    eng.load_texts(texts_of_lengths(lens))
    eng.split("words")
    eng.encode_split(v.merges)
    toff = eng.text_offsets()
    assert np.diff(toff.astype(np.int64)).tolist() == list(lens)
    return eng.ids().copy(), toff


@pytest.mark.parametrize("row_len", [1, 3, 4, 5, 64, 257])
def test_pack_equals_numpy(eng, vocabs, row_len):
    v = vocabs["words", False]
    cycle = [0, 1, row_len - 1, row_len, row_len + 1, 3 * row_len]
    lens = [cycle[k % 6] for k in range(257)]
    ids, toff = load_lengths(eng, v, lens)
    for side in ("right", "left"):
        for pad in (0, 0xFFFFFFFF):
            rows, got = eng.pack_texts(row_len, pad, side)
            want_rows, want = R.pack_rows(ids, toff, row_len, pad, side)
            assert rows.dtype == np.uint32 and rows.shape == (257, row_len) and got.dtype == np.uint32
            assert (got == want).all() and (got == np.minimum(lens, row_len)).all()
            assert (rows == want_rows).all()
    with pytest.raises(BpeError):
        eng.pack_texts(row_len, 0, "middle")


@pytest.mark.parametrize("T", [1, 255, 256, 257])
def test_pack_text_counts(eng, vocabs, T):
    v = vocabs["words", False]
    lens = [(7 * k + 3) % 23 for k in range(T)]
    ids, toff = load_lengths(eng, v, lens)
    for row_len in (5, 8):
        for side in ("right", "left"):
            rows, got = eng.pack_texts(row_len, 9, side)
            want_rows, want = R.pack_rows(ids, toff, row_len, 9, side)
            assert (rows == want_rows).all() and (got == want).all()


def test_pack_into_tensors(eng, vocabs):
    import torch
    v = vocabs["words", False]
    row_len = 64
    cycle = [0, 1, row_len - 1, row_len, row_len + 1, 3 * row_len]
    lens = [cycle[k % 6] for k in range(300)]
    ids, toff = load_lengths(eng, v, lens)
    dev = torch.device("cuda", 0)
    for side in ("right", "left"):
        want_rows, want = R.pack_rows(ids, toff, row_len, 0xFFFFFFFF, side)
        out = torch.zeros((300, row_len), dtype=torch.int32, device=dev)
        rows, got = eng.pack_texts(row_len, 0xFFFFFFFF, side, out=out)
        assert rows is out and got.dtype == torch.int32 and got.device == out.device
        assert (rows.cpu().numpy().view(np.uint32) == want_rows).all() and (got.cpu().numpy().view(np.uint32) == want).all()
        # an output that is only 4-byte aligned: the kernel's scalar path at a row length the vector path takes
        flat = torch.zeros(300 * row_len + 1, dtype=torch.int32, device=dev)
        odd = flat[1:].view(300, row_len)
        assert odd.data_ptr() % 16 == 4 and odd.is_contiguous()
        rows, got = eng.pack_texts(row_len, 0xFFFFFFFF, side, out=odd)
        assert int(flat[0]) == 0 and (rows.cpu().numpy().view(np.uint32) == want_rows).all()
    for bad in (torch.zeros((300, row_len), dtype=torch.int32), torch.zeros((300, row_len + 1), dtype=torch.int32, device=dev),
                torch.zeros((300, row_len), dtype=torch.float32, device=dev)):
        with pytest.raises(BpeError):
            eng.pack_texts(row_len, 0, out=bad)


def test_encode_batch_rows(toks):
    import torch
    tok = toks["cl100k", True][0]
    texts = [SRC[:40], b"", SRC[40:41], SRC[41:900], EOT, SRC[900:1100]]
    ids, toff = tok.encode_batch(texts)
    assert (ids < 256 + 300).sum() < ids.size  # (vocabulary ids: the specials' lie far above the merges')
    for side in ("right", "left"):
        want_rows, want = R.pack_rows(ids, toff, 16, 128001, side)
        rows, lens = tok.encode_batch(texts, max_length=16, pad_id=128001, truncation_side=side)
        assert rows.dtype == np.uint32 and (rows == want_rows).all() and (lens == want).all()
        pt_rows, pt_lens = tok.encode_batch(texts, max_length=16, pad_id=128001, truncation_side=side, return_tensors="pt")
        assert pt_rows.dtype == torch.int32 and pt_lens.dtype == torch.int32
        assert pt_rows.device == torch.device("cuda", tok.device) == pt_lens.device
        assert (pt_rows.cpu().numpy().view(np.uint32) == rows).all() and (pt_lens.cpu().numpy().view(np.uint32) == lens).all()
    for kw in ({"max_length": 4}, {"pad_id": 0}, {"return_tensors": "pt"}, {"max_length": 4, "pad_id": 0, "return_tensors": "np"}):
        with pytest.raises(BpeError):
            tok.encode_batch(texts, **kw)
    rows, lens = tok.encode_batch([], max_length=4, pad_id=0, return_tensors="pt")
    assert tuple(rows.shape) == (0, 4) and tuple(lens.shape) == (0,)


@pytest.mark.parametrize("rule", ["gpt2_unicode", "cl100k"])
def test_decode_batch_returns_the_texts(toks, rule):
    tok = toks[rule, True][0]
    texts = [SRC[:700], b"", "é€😀 it's".encode(), EOT + b"a" + EOT, b"a\0b\0", b"\0", SRC[700:2000]]
    ids, toff = tok.encode_batch(texts)
    assert tok.decode_batch(ids, toff) == [t.replace(b"\0", b"") for t in texts]  # (the decoders drop NULs)
    assert tok.decode_batch(*tok.encode_batch([])) == []

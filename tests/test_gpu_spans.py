"""Token spans on the device (spans.hip, bpe_gpu_token_spans / _fetch_token_spans / _pack_spans,
Engine.token_spans / pack_spans, Tokenizer.encode / encode_batch with return_spans).  The yardsticks are the host C
definition (api.token_spans_host, itself held to tests/spans_ref.py and to `tokenizers` by tests/test_spans_host.py)
and tests/spans_ref.py: the recorded character offsets of tests/golden/vocab/spans_*.json, both units at every id
count where the kernels' loops take another shape, token boundaries and multi-byte characters around a 64-byte mask
word and the character pass's grid step, text batches of every kind, spans before and after map_ids, the tiling
invariants, the packed rows against numpy, the refusals, and the ids of the calls that ask for no span."""
import ctypes
import json
import os

import numpy as np
import pytest

import golden_lib as G
import spans_ref as SR
from llmtokenizer_amd import api
from llmtokenizer_amd.api import BpeError
from llmtokenizer_amd.synth import english_like
from llmtokenizer_amd.vocab import Tokenizer, Vocab

pytestmark = pytest.mark.gpu

ESTATE, EINVAL, EDATA = "call out of order", "invalid argument", "unknown token id or corrupt merge list"
UNITS = ["byte", "char"]
# ids per thread, workgroup and grid step of k_spans and bytes per grid step of k_span_lead: api.span_info(), held to
# these by test_span_info (the library is not loaded while pytest collects)
TH, WG, GR, LG = 1, 256, 256 * 2048, 16 * 256 * 1024
SIZES = sorted({0, 1, 2, 63, 64, 65, WG - 1, WG, WG + 1, GR - 1, GR, GR + 1})
# bytes english_like never holds, so no merge names them and each stays one id: continuation bytes and bytes that
# read as the first of a character, so that both kinds of byte lie everywhere
PAD = np.concatenate([np.arange(0x80, 0x90), np.arange(0xF0, 0x100)]).astype(np.uint8)
TEXT = english_like(1 << 16)
MULTI = "é€😀".encode("utf-8")  # a 2-, a 3- and a 4-byte character
FIXTURES = ["spans_gpt2u", "spans_cl100k"]


@pytest.fixture(scope="module")
def eng():
    e = api.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def merges():
    m, _ = api.train_bytes(TEXT[:20000], 300)
    assert m.shape == (300, 2) and not np.isin(m, PAD).any()
    return m


@pytest.fixture(scope="module")
def voc(merges):
    """shuffled ids with holes, no specials"""
    ids = np.random.default_rng(21).permutation(256 + 300 + 100)[: 256 + 300]
    return Vocab(merges, ids[:256], ids[256:], [], [], "cl100k")


def fixed_checksum(eng, voc):
    """the ids of a fixed text through calls that ask for no span: load, split, encode_split, map_ids"""
    eng.load(TEXT[:30000] + MULTI)
    eng.split("cl100k")
    eng.encode_split(voc.merges)
    eng.map_ids(voc)
    c = eng.ids_checksum()
    assert c == G.ids_checksum(eng.ids())
    return c


@pytest.fixture(scope="module")
def checksum_before(eng, voc):
    """taken by the first test of this module, before any span call of the process"""
    return fixed_checksum(eng, voc)


def test_span_info_and_first_checksum(checksum_before):
    assert api.span_info() == {"per_thread": TH, "per_block": WG, "per_grid": GR, "lead_bytes_per_grid": LG}
    assert checksum_before != 0


def load_fixture(name, tmp_path):
    with open(os.path.join(G.GOLD, "vocab", name + ".json"), encoding="utf-8") as f:
        fx = json.load(f)
    with open(os.path.join(G.GOLD, "vocab", fx["vocab"] + ".json"), encoding="utf-8") as f:
        tj = json.load(f)["tokenizer_json"]
    p = tmp_path / "tokenizer.json"
    p.write_text(json.dumps(tj, ensure_ascii=False), encoding="utf-8")
    return fx, Vocab.from_tokenizer_json(p)


def join(texts):
    raw = [t.encode("utf-8") if isinstance(t, str) else bytes(t) for t in texts]
    return b"".join(raw), np.concatenate([[0], np.cumsum([len(t) for t in raw])]).astype(np.uint64), raw


def check_resident(eng, merges, data, boff, specials=None, vocab=None, batch=False):
    """both units of the resident ids against the host definition; returns {unit: spans}.  batch: the context holds
    a text batch with the byte offsets boff, else the one text data"""
    ids = eng.ids()
    toff = eng.text_offsets() if batch else np.array([0, ids.size], dtype=np.uint64)
    lens = api.span_lens(merges, specials, vocab)
    out = {}
    for unit in UNITS:
        got = eng.token_spans(merges, specials, vocab, unit)
        want = api.token_spans_host(ids, toff, data, boff, lens, unit)
        assert got.dtype == np.uint32 and got.shape == (ids.size, 2)
        assert np.array_equal(got, want), (unit, np.flatnonzero((got != want).any(axis=1))[:5])
        out[unit] = got
    return out


def run_texts(eng, merges, texts, rule="cl100k", specials=None):
    """load the texts as a batch, split, encode, check both units; returns (ids, text_off, {unit: spans})"""
    data, boff, raw = join(texts)
    eng.load_texts(data, offsets=boff)
    eng.split(rule, specials)
    eng.encode_split(merges)
    spans = check_resident(eng, merges, data, boff, specials, batch=True)
    return eng.ids(), eng.text_offsets(), spans


# ---------------------------------------------------------------- fixtures recorded from `tokenizers`

@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_texts_one_by_one(name, tmp_path):
    fx, v = load_fixture(name, tmp_path)
    tok = Tokenizer(v)
    try:
        for text, want_ids, want in zip(fx["texts"], fx["ids"], fx["offsets"]):
            ids, spans = tok.encode(text, return_spans="char")
            assert ids.tolist() == want_ids and spans.dtype == np.uint32 and spans.shape == (len(want_ids), 2)
            assert spans.tolist() == want, repr(text)
        text = fx["texts"][-1]
        ids, doc_off, byte_off, spans = tok.encode(text, return_offsets=True, return_spans="byte")
        raw = text.encode("utf-8")
        token_of = SR.token_bytes_by_id(v)
        assert spans.tolist() == [list(s) for s in SR.spans_of_text([token_of[i] for i in ids.tolist()], raw, "byte")]
        assert doc_off[-1] == ids.size and byte_off[-1] == len(raw)
        assert isinstance(tok.encode(text), np.ndarray)
        with pytest.raises(BpeError, match="return_spans"):
            tok.encode(text, return_spans="word")
    finally:
        tok.close()


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_texts_as_one_batch(name, tmp_path):
    import torch
    fx, v = load_fixture(name, tmp_path)
    tok = Tokenizer(v)
    try:
        texts = fx["texts"]
        ids, toff, spans = tok.encode_batch(texts, return_spans="char")
        assert ids.tolist() == [i for x in fx["ids"] for i in x]
        assert toff.tolist() == np.concatenate([[0], np.cumsum([len(x) for x in fx["ids"]])]).tolist()
        assert spans.tolist() == [o for x in fx["offsets"] for o in x]
        _, _, raw = join(texts)
        _, _, bspans = tok.encode_batch(texts, return_spans="byte")
        assert np.array_equal(bspans, SR.batch_spans(SR.token_bytes_by_id(v), ids, toff, raw, "byte"))
        # rows: numpy and torch, both sides
        for side in ("right", "left"):
            rows, lens, srows = tok.encode_batch(texts, max_length=8, pad_id=7, truncation_side=side, return_spans="char")
            want = pack_ref(spans, toff, 8, side)
            assert srows.dtype == np.uint32 and np.array_equal(srows, want)
            pr, pl, ps = tok.encode_batch(texts, max_length=8, pad_id=7, truncation_side=side, return_tensors="pt",
                                          return_spans="char")
            assert ps.dtype == torch.int32 and ps.device == pr.device and tuple(ps.shape) == (len(texts), 8, 2)
            assert np.array_equal(ps.cpu().numpy().view(np.uint32), want)
            assert np.array_equal(pr.cpu().numpy().view(np.uint32), rows) and np.array_equal(pl.cpu().numpy().view(np.uint32), lens)
        assert len(tok.encode_batch(texts, max_length=8, pad_id=7)) == 2  # (no span asked for: the result of before)
        with pytest.raises(BpeError, match="return_spans"):
            tok.encode_batch(texts, return_spans=True)
    finally:
        tok.close()


# ---------------------------------------------------------------- geometry of the span kernel

_head_ids = {}


def text_of_ids(eng, merges, n, seed=1):
    """bytes whose encode under merges has exactly n ids (as tests/test_gpu_vocab.py builds them): a head of text
    the merges shorten, then random PAD bytes, each of which stays one id"""
    h = min(n // 2, 3000)
    if h not in _head_ids:
        eng.load(TEXT[:h])
        eng.encode(merges)
        _head_ids[h] = eng.ids().size
    pad = np.random.default_rng(seed).choice(PAD, n - _head_ids[h]).tobytes()
    return TEXT[:h] + pad


@pytest.mark.parametrize("n", SIZES)
def test_id_counts_around_the_kernels_steps(eng, merges, n):
    data = text_of_ids(eng, merges, n)
    if n == 0:  # (no byte: a batch of one empty text)
        ids, toff, spans = run_texts(eng, merges, [b""])
        assert ids.size == 0 and all(s.shape == (0, 2) for s in spans.values())
        return
    eng.load(data)
    eng.encode_docs([0, len(data)], merges)
    assert eng.ids().size == n
    spans = check_resident(eng, merges, data, [0, len(data)])
    assert spans["byte"][0, 0] == 0 and spans["byte"][-1, 1] == len(data)
    # the same ids as a batch of two texts, the break in the kernel's last step
    cut = len(data) - min(len(data), 3)
    ids, toff, _ = run_texts(eng, merges, [data[:cut], data[cut:]], rule="words")
    assert toff[-1] == ids.size


# ---------------------------------------------------------------- the character pass: mask words and its grid step

_BASE = {}


def with_cluster(base, at):
    """base with MULTI written over the bytes from `at`"""
    return base[:at] + MULTI + base[at + len(MULTI):]


@pytest.mark.parametrize("d", [-1, 0, 1])
def test_characters_around_a_mask_word_and_the_lead_grid_step(eng, merges, d):
    """a token boundary and a 2-, 3- and 4-byte character at -1, 0, +1 of 64-byte words and of k_span_lead's
    grid step, every inner byte of each character on the edge once"""
    if "base" not in _BASE:
        _BASE["base"] = english_like(LG + 4096)
    base = data = _BASE["base"]
    for edge in (64, 4096, LG):
        # word edges 128 bytes apart from `edge` on, on each (at d = 0) another inner byte of a character: the byte
        # after 1 of é, after 1 / 2 of the euro, after 1 / 2 / 3 of the emoji; at the grid step the emoji's middle
        backs = (7, 1, 3, 4, 6, 8) if edge == LG else (1, 3, 4, 6, 7, 8)
        for k, back in enumerate(backs):
            data = with_cluster(data, edge + 128 * k - back + d)
    assert len(data) == len(base)
    eng.load(data)
    eng.split("cl100k")
    eng.encode_split(merges)
    spans = check_resident(eng, merges, data, [0, len(data)])
    assert spans["char"][-1, 1] == int(((np.frombuffer(data, dtype=np.uint8) & 0xC0) != 0x80).sum())
    # the same bytes as texts whose breaks fall on the edges, inside the characters
    cuts = [0, 64 + d, 192 + d, 4096 + d, LG + d, LG + 128 + d, len(data)]
    run_texts(eng, merges, [data[a:b] for a, b in zip(cuts, cuts[1:])])


def test_a_break_at_each_inner_byte_of_a_character(eng, merges):
    texts = []
    for ch in ("é", "€", "😀"):
        b = ch.encode("utf-8")
        for i in range(1, len(b)):
            texts += [b"ab " + b[:i], b[i:] + b" yz", b[i:], b[:i]]
    ids, toff, spans = run_texts(eng, merges, texts)
    _, _, raw = join(texts)
    token_of = dict(enumerate(SR.internal_token_bytes(merges)))
    for unit in UNITS:
        assert np.array_equal(spans[unit], SR.batch_spans(token_of, ids, toff, raw, unit))
    # the same cuts with the first text filling 61 .. 63 bytes of a mask word
    for fill in (57, 58, 59, 60):
        run_texts(eng, merges, [b"x" * fill + "😀".encode()[:i] for i in (1, 2, 3)] + ["😀".encode()[i:] for i in (1, 2, 3)])


# ---------------------------------------------------------------- text batches

SRC = (english_like(3000) + b" 12345 it's \n\n \t" + MULTI + b" <|endoftext|>x\0y ") * 40


@pytest.mark.parametrize("T", [1, 255, 256, 257])
def test_text_counts(eng, merges, T):
    cuts = np.linspace(0, len(SRC), T + 1).astype(np.int64)
    run_texts(eng, merges, [SRC[a:b] for a, b in zip(cuts, cuts[1:])], specials=[b"<|endoftext|>"])


@pytest.mark.parametrize("where", ["first", "last", "middle", "three", "all", "none"])
def test_empty_texts(eng, merges, where):
    a, b, c = SRC[:700], SRC[700:701], SRC[701:2000]
    texts = {"first": [b"", a, b, c], "last": [a, b, c, b""], "middle": [a, b"", b, c], "three": [a, b"", b"", b"", b, c],
             "all": [b"", b"", b"", b"", b""], "none": []}[where]
    ids, toff, spans = run_texts(eng, merges, texts)
    assert toff.size == len(texts) + 1
    if where in ("all", "none"):
        assert ids.size == 0 and eng.pack_spans(4).shape == (len(texts), 4, 2) and not eng.pack_spans(4).any()


def test_one_byte_texts_every_wave_searches(eng, merges):
    """70,000 texts of one byte: a wave's 64 ids lie in 64 texts, past what a lane walks"""
    T = 70000
    raw = np.random.default_rng(5).integers(0, 256, T, dtype=np.uint8)
    ids, toff, spans = run_texts(eng, merges, [bytes([b]) for b in raw.tolist()])
    assert ids.size == T and (spans["byte"] == [0, 1]).all()
    assert (spans["char"][:, 0] == 0).all() and (spans["char"][:, 1] == ((raw & 0xC0) != 0x80)).all()


def test_one_long_text_among_short_ones(eng, merges):
    texts = [SRC[k:k + 3] for k in range(0, 300, 3)] + [SRC[300:90000]] + [SRC[90000 + k:90002 + k] for k in range(0, 400, 2)]
    run_texts(eng, merges, texts)
    # texts of 0 .. 9 ids in turn: the walk's limit is crossed inside many waves
    rng = np.random.default_rng(9)
    run_texts(eng, merges, [rng.choice(PAD, k % 10).tobytes() for k in range(3000)], rule="words")


def test_spans_before_and_after_map_ids(eng, merges, voc):
    cuts = np.linspace(0, 60000, 41).astype(np.int64)
    texts = [SRC[a:b] for a, b in zip(cuts, cuts[1:])]
    data, boff, _ = join(texts)
    eng.load_texts(data, offsets=boff)
    eng.split("cl100k")
    eng.encode_split(merges)
    before = {u: eng.token_spans(merges, unit=u) for u in UNITS}
    with pytest.raises(BpeError, match=ESTATE):  # unmapped ids with a vocabulary
        eng.token_spans(merges, vocab=voc)
    eng.token_spans(merges, unit="char")
    eng.map_ids(voc)
    srows = eng.pack_spans(16)  # the spans outlive the map: numbering is not position
    assert np.array_equal(srows, pack_ref(before["char"], eng.text_offsets(), 16, "right"))
    with pytest.raises(BpeError, match=ESTATE):  # mapped ids without one
        eng.token_spans(merges)
    after = check_resident(eng, merges, data, boff, vocab=voc, batch=True)
    for u in UNITS:
        assert np.array_equal(before[u], after[u])


def test_invariants_on_a_mebibyte(eng, merges):
    data = english_like(1 << 20)
    cuts = np.linspace(0, len(data), 301).astype(np.int64)
    texts = [data[a:b] for a, b in zip(cuts, cuts[1:])]
    ids, toff, spans = run_texts(eng, merges, texts)
    s, e = spans["byte"][:, 0].astype(np.int64), spans["byte"][:, 1].astype(np.int64)
    first, last = toff[:-1].astype(np.int64), toff[1:].astype(np.int64) - 1
    assert (s[first] == 0).all() and (e[last] == np.diff(cuts)).all()  # (no text here is empty)
    inner = np.ones(ids.size, dtype=bool)
    inner[last] = False
    assert (e[inner] == s[1:][inner[:-1]]).all() and (e > s).all()
    token_of = SR.internal_token_bytes(merges)
    text_of_id = np.repeat(np.arange(300), np.diff(toff.astype(np.int64)))
    base = cuts[text_of_id]
    for i in range(ids.size):
        assert data[base[i] + s[i]:base[i] + e[i]] == token_of[ids[i]], i


# ---------------------------------------------------------------- rows

def pack_ref(spans, toff, row_len, side):
    T = len(toff) - 1
    out = np.zeros((T, row_len, 2), dtype=np.uint32)
    for k in range(T):
        a, b = int(toff[k]), int(toff[k + 1])
        keep = min(b - a, row_len)
        src = b - row_len if side == "left" and b - a > row_len else a
        out[k, :keep] = spans[src:src + keep]
    return out


def load_lengths(eng, merges, lens, seed=3):
    """texts whose id counts are exactly lens: PAD bytes under "words", every byte one id; the spans in bytes"""
    rng = np.random.default_rng(seed)
    eng.load_texts([rng.choice(PAD, n).tobytes() for n in lens])
    eng.split("words")
    eng.encode_split(merges)
    toff = eng.text_offsets()
    assert np.diff(toff.astype(np.int64)).tolist() == list(lens)
    return eng.token_spans(merges), toff


@pytest.mark.parametrize("row_len", [1, 2, 3, 4, 5, 64, 257])
def test_pack_spans_equals_numpy(eng, merges, row_len):
    import torch
    cycle = [0, 1, row_len - 1, row_len, row_len + 1, 3 * row_len]
    lens = [cycle[k % 6] for k in range(257)]
    spans, toff = load_lengths(eng, merges, lens)
    dev = torch.device("cuda", 0)
    for side in ("right", "left"):
        want = pack_ref(spans, toff, row_len, side)
        rows = eng.pack_spans(row_len, side)
        assert rows.dtype == np.uint32 and rows.shape == (257, row_len, 2) and np.array_equal(rows, want)
        for k, n in enumerate(lens):  # the cells behind the ids are (0, 0); with "left" the spans are the text's own
            assert not rows[k, min(n, row_len):].any()
            if n > row_len and side == "left":
                assert rows[k, 0, 0] == n - row_len and rows[k, -1, 1] == n
        out = torch.full((257, row_len, 2), -1, dtype=torch.int32, device=dev)
        got = eng.pack_spans(row_len, side, out=out)
        assert got is out and np.array_equal(out.cpu().numpy().view(np.uint32), want)
        # an output that is only 8-byte aligned: the one-cell path at a row length the two-cell path takes
        flat = torch.full((257 * row_len * 2 + 2,), -1, dtype=torch.int32, device=dev)
        odd = flat[2:].view(257, row_len, 2)
        assert odd.data_ptr() % 16 == 8 and odd.is_contiguous()
        eng.pack_spans(row_len, side, out=odd)
        assert int(flat[0]) == -1 and int(flat[1]) == -1 and np.array_equal(odd.cpu().numpy().view(np.uint32), want)
    with pytest.raises(BpeError):
        eng.pack_spans(row_len, "middle")
    for bad in (torch.zeros((257, row_len, 2), dtype=torch.int32), torch.zeros((257, row_len + 1, 2), dtype=torch.int32, device=dev),
                torch.zeros((257, row_len, 2), dtype=torch.float32, device=dev), torch.zeros((257, row_len), dtype=torch.int32, device=dev)):
        with pytest.raises(BpeError):
            eng.pack_spans(row_len, out=bad)


# ---------------------------------------------------------------- refusals and lifetime

def test_refusals_and_lifetime(eng, merges, voc):
    fresh = api.Engine(0)
    try:
        with pytest.raises(BpeError, match=ESTATE):  # before an encode
            fresh.token_spans(merges)
    finally:
        fresh.close()
    data = SRC[:20000]
    eng.load(data)
    with pytest.raises(BpeError, match=ESTATE):  # after a load
        eng.token_spans(merges)
    eng.encode(merges)
    with pytest.raises(BpeError, match=ESTATE) as e:  # the ids of a plain encode
        eng.token_spans(merges)
    assert "encode_split" in str(e.value)
    eng.split("cl100k")
    eng.encode_split(merges)
    assert ctypes_count(eng) is None  # no spans yet: the fetch is out of order
    with pytest.raises(BpeError, match=EINVAL) as e:  # a merge count that is not the encode's
        eng.token_spans(merges[:299])
    assert "299 merges" in str(e.value) and "300" in str(e.value)
    with pytest.raises(BpeError, match="unit"):
        eng.token_spans(merges, unit="word")
    rc = eng.L.bpe_gpu_token_spans(eng.ctx, merges.ctypes.data_as(ctypes.c_void_p), 300, None, None, 2)
    assert eng.L.bpe_gpu_strerror(rc).decode() == EINVAL
    good = check_resident(eng, merges, data, [0, len(data)])
    assert ctypes_count(eng) == good["byte"].shape[0]
    # the right count, other lengths: refused by the sum, and the spans of before are not kept
    other = merges.copy()
    other[10:] = np.stack([np.arange(256, 256 + 290), np.full(290, 0x61)], axis=1)  # merge r: merge r - 10 and a letter
    assert not np.array_equal(api.span_lens(other), api.span_lens(merges))
    with pytest.raises(BpeError, match=EDATA) as e:
        eng.token_spans(other)
    assert "not the merge list of this encode" in str(e.value) and f"the text holds {len(data)} bytes" in str(e.value)
    assert ctypes_count(eng) is None
    again = check_resident(eng, merges, data, [0, len(data)])  # ... and the engine goes on
    assert ctypes_count(eng) == again["byte"].shape[0] and np.array_equal(again["char"], good["char"])
    with pytest.raises(BpeError, match=ESTATE) as e:  # rows need a text batch
        eng.pack_spans(8)
    assert "no text batch" in str(e.value)
    # specials that the split knew and the call does not: their ids lie past the table
    sp = [b"<|endoftext|>"]
    eng.split("cl100k", sp)
    eng.encode_split(merges)
    with pytest.raises(BpeError, match=EDATA) as e:
        eng.token_spans(merges)
    assert "spans: unknown token id" in str(e.value)
    check_resident(eng, merges, data, [0, len(data)], specials=sp)
    # a batch: the same total, other texts
    texts = [data[:7000], b"", data[7000:]]
    eng.load_texts(texts)
    eng.split("cl100k", sp)
    eng.encode_split(merges)
    with pytest.raises(BpeError, match=ESTATE) as e:
        eng.pack_spans(8)
    assert "no spans" in str(e.value)
    eng.token_spans(merges, sp)
    for call, code, word in ((lambda: eng.pack_spans(0), EINVAL, "row_len is 0"),
                             (lambda: eng.pack_spans((1 << 24) + 1), "out of range", "row_len above 2^24")):
        with pytest.raises(BpeError, match=code) as e:
            call()
        assert word in str(e.value)
    assert eng.pack_spans(4).shape == (3, 4, 2)
    eng.encode_split(merges)  # new ids: the spans went with the old ones
    with pytest.raises(BpeError, match=ESTATE):
        eng.pack_spans(4)
    assert ctypes_count(eng) is None


def ctypes_count(eng):
    """the span count of bpe_gpu_fetch_token_spans, or None when it is out of order"""
    n = ctypes.c_size_t(0)
    rc = eng.L.bpe_gpu_fetch_token_spans(eng.ctx, None, 0, ctypes.byref(n))
    if rc:
        assert eng.L.bpe_gpu_strerror(rc).decode() == ESTATE
        return None
    return n.value


# ---------------------------------------------------------------- the calls that ask for no span

def test_untouched_paths_keep_their_ids(eng, voc, checksum_before):
    """(runs last: span calls of every kind have been made in this process by now)"""
    assert fixed_checksum(eng, voc) == checksum_before
    eng.token_spans(voc.merges, vocab=voc, unit="char")
    assert eng.ids_checksum() == checksum_before
    assert fixed_checksum(eng, voc) == checksum_before

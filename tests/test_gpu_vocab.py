"""Vocabulary ids on the device (vocab.hip, bpe_gpu_map_ids, bpe_gpu_decode_docs_vocab, vocab.Tokenizer):
the ids `tokenizers` recorded for the fixture texts, the map against fwd[ids] from numpy at every size
where the kernel's loop takes another shape, the way back through decode_docs(vocab=), unknown ids as
error returns, the mapped mark's life, the identity numbering and specials numbered low and high."""
import json
import os

import numpy as np
import pytest

import golden_lib as G
from llmtokenizer_amd import api
from llmtokenizer_amd.api import BpeError
from llmtokenizer_amd.synth import english_like
from llmtokenizer_amd.vocab import Tokenizer, Vocab, vocab_tables

pytestmark = pytest.mark.gpu

ESTATE = "call out of order"
EDATA = "unknown token id"
# ids one thread of the map kernels moves per step, per workgroup step and per grid step: api.map_info(), held to
# these by test_map_info (the library is not loaded while pytest collects)
TH, WG, GR = 4, 4 * 256, 4 * 256 * 2048
SIZES = [0, 1, TH - 1, TH, TH + 1, WG - 1, WG, WG + 1, GR - 1, GR, GR + 1, 3 * GR + 7]
PAD = np.arange(0xF0, 0x100, dtype=np.uint8)  # bytes english_like never holds: no merge names them
TEXT = english_like(1 << 16)  # every text below is a slice of it


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


_head_ids = {}


def text_of_ids(eng, merges, n, seed=1):
    """bytes whose plain encode under merges has exactly n ids: a head of text the merges shorten (its id count
    measured once per length) followed by random PAD bytes, each of which stays one id"""
    h = min(n // 2, 3000)
    if h not in _head_ids:
        eng.load(TEXT[:h])
        eng.encode(merges)
        _head_ids[h] = eng.ids().size
    pad = np.random.default_rng(seed).choice(PAD, n - _head_ids[h]).tobytes()
    return TEXT[:h] + pad


# ---------------------------------------------------------------- fixtures recorded from `tokenizers`

@pytest.mark.parametrize("name", ["vocab_gpt2u", "vocab_cl100k"])
def test_fixture_ids_and_texts(name, tmp_path):
    with open(os.path.join(G.GOLD, "vocab", name + ".json"), encoding="utf-8") as f:
        fx = json.load(f)
    p = tmp_path / "tokenizer.json"
    p.write_text(json.dumps(fx["tokenizer_json"], ensure_ascii=False), encoding="utf-8")
    v = Vocab.from_tokenizer_json(p)
    assert v.rule == fx["rule"] and len(v.specials) == 2 and len(fx["texts"]) >= 30
    tok = Tokenizer(v)
    try:
        for text, want in zip(fx["texts"], fx["ids"]):
            got = tok.encode(text)
            assert got.dtype == np.uint32 and got.tolist() == want, repr(text)
            assert tok.decode(want) == text.encode("utf-8"), repr(text)
    finally:
        tok.close()


# ---------------------------------------------------------------- geometry of the map and its inverse

def test_map_info():
    assert api.map_info() == {"thread": TH, "workgroup": WG, "grid": GR}


@pytest.mark.parametrize("n", SIZES)
def test_map_equals_numpy_and_decodes_back(eng, merges, voc, n):
    fwd, _ = vocab_tables(voc)
    data = text_of_ids(eng, merges, n)
    eng.load(data)
    eng.encode(merges)
    internal = eng.ids().copy()
    assert internal.size == n
    eng.map_ids(voc)
    got = eng.ids()
    assert got.dtype == np.uint32 and got.size == n and (got == fwd[internal]).all()
    assert eng.ids_checksum() == G.ids_checksum(fwd[internal])
    assert eng.ids_checksum(5) == G.ids_checksum(fwd[internal], base=5)
    back, off = eng.decode_docs(got, [0, n], merges, vocab=voc)
    assert back == data and off.tolist() == [0, len(data)]


# ---------------------------------------------------------------- unknown ids are error returns

def _bad_ids(voc):
    _, inv = vocab_tables(voc)
    return {"hole": int(np.flatnonzero(inv == 0xFFFFFFFF)[0]), "past": inv.size, "all_ones": 0xFFFFFFFF}


@pytest.mark.parametrize("where", ["first", "last", "tail"])
@pytest.mark.parametrize("kind", ["hole", "past", "all_ones"])
def test_unknown_id_raises_and_the_engine_goes_on(eng, merges, voc, kind, where):
    """the kernel compares every id with the table's length before it indexes: an error return, no fault"""
    n = WG + 3  # (the last three ids are the scalar tail of the vector loop)
    good = voc.byte_ids[np.random.default_rng(3).integers(0x61, 0x7B, n)]
    ids = good.copy()
    ids[{"first": 0, "last": n - 1, "tail": n - 2}[where]] = _bad_ids(voc)[kind]
    with pytest.raises(BpeError, match=EDATA):
        eng.decode_docs(ids, [0, n], merges, vocab=voc)
    back, _ = eng.decode_docs(good, [0, n], merges, vocab=voc)
    _, inv = vocab_tables(voc)
    assert back == inv[good].astype(np.uint8).tobytes()


# ---------------------------------------------------------------- the mapped mark

def test_state(merges, voc):
    e = api.Engine(0)
    try:
        with pytest.raises(BpeError, match=ESTATE):
            e.map_ids(voc)  # nothing loaded
        data = TEXT[:3000]
        e.load(data)
        with pytest.raises(BpeError, match=ESTATE):
            e.map_ids(voc)  # loaded, not encoded
        e.split("cl100k")
        e.encode_split(merges)
        internal, off = e.ids().copy(), e.doc_offsets().copy()
        e.map_ids(voc)
        fwd, _ = vocab_tables(voc)
        assert (e.ids() == fwd[internal]).all()
        assert (e.doc_offsets() == off).all()
        with pytest.raises(BpeError, match=ESTATE):
            e.map_ids(voc)  # twice
        assert (e.ids() == fwd[internal]).all()  # (the refused call changed nothing)
        e.encode_split(merges)  # a new encode clears the mark
        assert (e.ids() == internal).all()
        e.map_ids(voc)
        assert (e.ids() == fwd[internal]).all()
        e.load(data)  # so does a load: the ids go with it
        with pytest.raises(BpeError, match=ESTATE):
            e.map_ids(voc)
        e.encode(merges)
        e.map_ids(voc)
        short = Vocab(merges[:299], voc.byte_ids, voc.merge_ids[:299], [], [], "cl100k")
        e.encode(merges)
        with pytest.raises(BpeError, match="299 merges"):
            e.map_ids(short)  # not this encode's vocabulary
    finally:
        e.close()


# ---------------------------------------------------------------- Tokenizer

def test_identity_numbering_equals_encode_split(merges):
    data = TEXT[:50000] + b" It's 12345 o'clock\n\n" * 3
    v = Vocab.from_merges(merges, "cl100k")
    tok = Tokenizer(v)
    try:
        ids, id_off, byte_off = tok.encode(data, return_offsets=True)
        want = api.encode_split(data, merges, "cl100k")
        assert (ids == want[0]).all() and (id_off == want[1]).all() and (byte_off == want[2]).all()
        assert tok.decode(ids) == data
    finally:
        tok.close()


@pytest.mark.parametrize("special_ids", [[5, 300], [70000, (1 << 24) - 1]], ids=["low", "high"])
def test_specials_numbered_low_and_high_round_trip(merges, special_ids):
    """specials whose ids lie below 256 + merges (among the bytes' and merges' ids) and far above them"""
    specials = [b"<|endoftext|>", b"<|im_start|>"]
    free = np.setdiff1d(np.arange(256 + 300 + 50), special_ids)
    ids = np.random.default_rng(4).permutation(free)[: 256 + 300]
    v = Vocab(merges, ids[:256], ids[256:], special_ids, specials, "gpt2_unicode")
    data = b"<|im_start|>" + TEXT[:4000] + b"<|endoftext|>" + TEXT[5000:5100] + b"<|endoftext|><|im_start|>x"
    tok = Tokenizer(v)
    try:
        got = tok.encode(data)
        assert int((got == special_ids[0]).sum()) == 2 and int((got == special_ids[1]).sum()) == 2
        assert got[0] == special_ids[1] and got[-2] == special_ids[1]
        want, _, _ = api.encode_split(data, merges, "gpt2_unicode", specials=specials)
        fwd, _ = vocab_tables(v)
        assert (got == fwd[want]).all()
        assert tok.decode(got) == data
    finally:
        tok.close()


# ---------------------------------------------------------------- the C layer's convenience calls

def test_c_layer_encode_split_vocab_and_decode_docs_vocab(merges):
    """bpe_ex.h bpe_encode_split_vocab / bpe_decode_docs_vocab: load, one thing, malloc'd results"""
    import ctypes
    from llmtokenizer_amd import _lib
    L = _lib.load()
    specials = [b"<|endoftext|>"]
    ids = np.random.default_rng(8).permutation(256 + 300 + 30)[: 256 + 300]
    v = Vocab(merges, ids[:256], ids[256:], [4000], specials, "cl100k")
    data = TEXT[:7000] + b"<|endoftext|>" + TEXT[7000:7777]
    tok = Tokenizer(v)
    try:
        want, want_ido, want_bo = tok.encode(data, return_offsets=True)
    finally:
        tok.close()
    buf = np.frombuffer(data, np.uint8)
    sp = api._Specials(specials)
    arr = api._merges_to_arr(merges)
    vp, u64p = ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)
    n, nd, total = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_size_t(0)
    ido, bo, byo = u64p(), u64p(), u64p()
    free = ctypes.CDLL(None).free
    free.argtypes = [vp]
    try:
        p = L.bpe_encode_split_vocab(buf.ctypes.data_as(vp), buf.size, api.SPLIT_PRESETS["cl100k"], None, None, sp.ref, arr,
                                     v.c_vocab().ref, 0, ctypes.byref(n), ctypes.byref(ido), ctypes.byref(bo),
                                     ctypes.byref(nd))
        assert p
        got = np.ctypeslib.as_array(p, shape=(n.value,)).copy()
        got_ido = np.ctypeslib.as_array(ido, shape=(nd.value + 1,)).copy()
        got_bo = np.ctypeslib.as_array(bo, shape=(nd.value + 1,)).copy()
        for q in (p, ido, bo):
            free(ctypes.cast(q, vp))
        assert (got == want).all() and (got_ido == want_ido).all() and (got_bo == want_bo).all()
        assert int((got == 4000).sum()) == 1
        off = np.array([0, got.size], dtype=np.uint64)
        s = L.bpe_decode_docs_vocab(got.ctypes.data_as(vp), got.size, off.ctypes.data_as(vp), 1, arr, sp.ref,
                                    v.c_vocab().ref, 0, ctypes.byref(total), ctypes.byref(byo))
        assert s
        assert ctypes.string_at(s, total.value) == data and [int(byo[0]), int(byo[1])] == [0, len(data)]
        free(vp(s))
        free(ctypes.cast(byo, vp))
        bad = got.copy()
        bad[5] = 4001  # one past the inverse table: the call reports and returns NULL
        assert not L.bpe_decode_docs_vocab(bad.ctypes.data_as(vp), bad.size, off.ctypes.data_as(vp), 1, arr, sp.ref,
                                           v.c_vocab().ref, 0, ctypes.byref(total), ctypes.byref(byo))
    finally:
        L.dyn_arr_free(arr)

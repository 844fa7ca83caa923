"""The piece-local replay (encode_piece.hip; encoder="piece" / "auto"): merge lists beyond the window
encoders' limits, rank order inside a piece, the tile geometry, agreement with the window encoder, and the
tokenizer on a vocabulary of more than 65,279 merges.  Every expectation is the oracle's, piece by piece
(O.encode through test_encode_limits._oracle_docs), or vocab.replay's.  Sizes come from api.piece_info(), asked inside the tests: the library is not
loaded while pytest collects."""
import functools
import random
from types import SimpleNamespace

import numpy as np
import pytest

import encode_limits_lib as EL
from llmtokenizer_amd import api, synth, vocab
from test_encode_limits import _doc_cuts, _oracle_docs, chain_case, count_case

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _sizes():
    """(core, longest piece) of a tile"""
    pi = api.piece_info()
    assert pi["tile"] == pi["core"] + pi["piece_max"] and pi["max_ids"] >= 1 << 20
    return pi["core"], pi["piece_max"]


def _run(docs, merges, encoder="piece"):
    """(ids, id offsets, docs_info, stats) of the resident encode_docs"""
    e = api.Engine(0)
    try:
        e.load(b"".join(docs))
        e.encode_docs(np.cumsum([0] + [len(d) for d in docs]).astype(np.uint64), merges, encoder=encoder)
        return e.ids(), e.doc_offsets(), e.docs_info(), e.stats()
    finally:
        e.close()


def _check(docs, merges, encoder="piece"):
    """the oracle's ids and offsets, through the piece path, with exactly the longer documents on the fallback"""
    oids, ooff = _oracle_docs(docs, merges)
    ids, off, info, st = _run(docs, merges, encoder)
    assert off.tolist() == ooff.tolist()
    assert ids.size == oids.size and (ids == oids).all()
    assert st["enc_path"] == 4 and st["n_out"] == oids.size
    assert info["docs_fallback"] == sum(len(d) > _sizes()[1] for d in docs)
    return ids, info


# ---- 1. lists beyond each limit of the window encoders

def _limit_case(name):
    if name == "chain-257":  # 257 layers; its text has no starts: cut it every 64 bytes or anywhere
        c = chain_case(257, False)
        return SimpleNamespace(m=c.m, merges=c.merges, text=c.text, starts=list(range(0, len(c.text), 64)))
    kind, m = name.split("-")
    return count_case(kind, int(m))


@pytest.mark.parametrize("encoder", ["piece", "auto"])
@pytest.mark.parametrize("name", ["random-65280", "two_layer-70000", "chain-257"])
def test_lists_beyond_each_limit(name, encoder):
    """An id above 65,535 is asserted where the list has one (70,000 merges): 65,280 merges end at id 65,535
    and the chain at 512."""
    c = _limit_case(name)
    docs = _doc_cuts(c, 2)  # (seed 2: an empty and a 1-byte document, none longer than a tile takes)
    C, P = _sizes()
    assert max(len(d) for d in docs) <= P
    ids, info = _check(docs, c.merges, encoder)
    assert info["docs_fallback"] == 0 and info["windows"] == 0 and info["tiles"] == -(-len(c.text) // C)
    if name != "chain-257":
        assert ids.max() >= 65000
    if 255 + c.m > 65535:
        assert (ids > 65535).any()


# ---- 2. rank order, not position order

AB_AA = np.array([[97, 98], [256, 256]], dtype=np.uint32)
AA_AA = np.array([[97, 97], [256, 256]], dtype=np.uint32)
# a repeated pair (rank 1 never matches), a forward reference (rank 2), a == a merges of merged ids (ranks 3, 4)
ODD = np.array([[97, 98], [97, 98], [300, 99], [256, 256], [259, 259], [99, 259]], dtype=np.uint32)
RUNS = np.array([[97, 97], [256, 256], [257, 257], [98, 256]], dtype=np.uint32)
ORDER = [
    ("abc", [b"abc"], np.array([[98, 99], [97, 98]], dtype=np.uint32)),
    ("abab", [b"abab", b"aaaaa"], AB_AA),
    ("aaaaa", [b"abab", b"aaaaa", b"aaaa", b"a"], AA_AA),
    ("odd_records", [b"ab" * 9 + b"c", b"cab" * 8, b"abababab" + b"c" * 3 + b"ab" * 4], ODD),
    # runs of even and odd length that cross the lanes' ranges (16 positions each in a full half tile), side by side
    ("runs", [b"a" * 33, b"b" + b"a" * 64, b"a" * 1000, b"", b"a" * 333 + b"b" + b"a" * 334], RUNS),
    ("run_fills_a_tile", lambda P: [b"a" * P, b"a" * (P - 1), b"ba"], RUNS),
]


@pytest.mark.parametrize("name,docs,merges", ORDER, ids=[o[0] for o in ORDER])
def test_rank_order_inside_a_piece(name, docs, merges):
    ids, info = _check(docs(_sizes()[1]) if callable(docs) else docs, merges)
    assert info["docs_fallback"] == 0
    if name == "abc":
        assert ids.tolist() == [97, 256]  # (98, 99) first although (97, 98) comes first in the text


# ---- 3. tile geometry

CHAIN = EL.chain_list(20)
DEEP = EL.expand(CHAIN, 256 + 19)  # 21 bytes, 20 merges one after the other
GEOMETRY = {  # the documents' lengths, from a tile's core C and its longest piece P
    "starts_around_the_core_edge": lambda C, P: [C - 1, 1, 1, 7],
    "longest_piece_at_the_last_owned_position": lambda C, P: [C - 1, P, 5],
    "lengths_around_the_longest": lambda C, P: [P - 1, P, P + 1, 3],
    "tiles_without_a_piece_start": lambda C, P: [C - 1, P + 1 + C, 4],
    "one_byte_pieces": lambda C, P: [1] * C + [3],
    "empty_pieces": lambda C, P: [0, 5, 0, 0, C, 0, 2, 0, 0, 0],
}


@pytest.mark.parametrize("name", list(GEOMETRY))
def test_tile_geometry(name):
    rng = random.Random(len(name))
    merges = EL._random_merges(random.Random(5), b"abcd", 300, eq=0.2)
    lens = GEOMETRY[name](*_sizes())
    docs = [bytes(rng.choice(b"abcd") for _ in range(n)) for n in lens]
    ids, info = _check(docs, merges)
    assert (ids.max() > 255 or max(lens) < 4) and info["tiles"] == -(-sum(lens) // _sizes()[0])


def test_one_round_beside_twenty():
    docs = [b"ab", DEEP, b"abz", DEEP * 3, b"", b"ba"]
    ids, info = _check(docs, CHAIN)
    assert info["rounds"] == 20 and info["tiles"] == 1 and (ids == 256 + 19).sum() == 4


# ---- 4. both encoders agree where both apply

@pytest.mark.parametrize("rule", ["words", "cl100k"])
def test_piece_equals_window(rule):
    text = synth.english_like(65536)
    merges = api.train_split(text, rule=rule, max_merges=200)
    assert len(merges) == 200
    off = api.split_host(text, rule)
    assert int(np.diff(off.astype(np.int64)).max()) <= _sizes()[1]
    want = api.encode_split(text, merges, rule=rule, encoder="window")
    got = api.encode_split(text, merges, rule=rule, encoder="piece")
    assert api.last_stats()["enc_path"] == 4
    for g, w in zip(got, want):
        assert g.tolist() == w.tolist()
    e = api.Engine(0)
    try:
        e.load_texts([text[:30000], b"", text[30000:]])
        res = []
        for enc in ("window", "piece"):
            e.split(rule)
            e.encode_split(merges, encoder=enc)
            res.append((e.ids().tolist(), e.doc_offsets().tolist(), e.text_offsets().tolist(), e.stats()["enc_path"]))
        assert res[0][:3] == res[1][:3] and (res[0][3], res[1][3]) == (1, 4)
        assert e.docs_info()["docs_fallback"] == 0
    finally:
        e.close()


# ---- 5. through the tokenizer

def test_tokenizer_beyond_65279_merges():
    trained = api.train_split(synth.english_like(65536), rule="cl100k", max_merges=300)
    k = 65300 - len(trained)  # padding that never matches: byte 1, which no text holds, before the id of the record before
    pad = np.stack([np.ones(k, np.uint32), 255 + len(trained) + np.arange(k, dtype=np.uint32)], axis=1)
    pad[0] = (1, 2)
    specials = [b"<|endoftext|>", b"<|pad|>"]
    v = vocab.Vocab.from_merges(np.vstack([trained, pad]), "cl100k", specials)
    texts = ["the quick brown fox", "", "one<|endoftext|>two  three\n", "café naïve 中文 ok", "tail  "]
    rank = {tuple(p): r for r, p in reversed(list(enumerate(trained.tolist())))}
    want = []
    for raw in (t.encode() for t in texts):
        off, at, which = api.split_host_special(raw, "cl100k", specials)
        sp = dict(zip(at.tolist(), which.tolist()))
        want.append([x for d, (a, b) in enumerate(zip(off.tolist(), off.tolist()[1:]))
                     for x in ([256 + 65300 + sp[d]] if d in sp else vocab.replay(list(raw[a:b]), rank))])
    tk = vocab.Tokenizer(v)
    try:
        ids, toff = tk.encode_batch(texts)
        st, info = tk._eng().stats(), tk._eng().docs_info()
        assert [ids[a:b].tolist() for a, b in zip(toff.tolist(), toff.tolist()[1:])] == want
        assert st["enc_path"] == 4 and info["docs_fallback"] == 0 and info["tiles"] >= 1
        assert tk.decode_batch(ids, toff) == [t.encode() for t in texts]
    finally:
        tk.close()

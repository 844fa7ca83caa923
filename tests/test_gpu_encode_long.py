"""The long-piece kernel behind the piece-local replay (encode_long.hip; encoder="piece_long", and "auto" where
it picks the piece path): documents longer than a tile takes, up to api.long_piece_info()["piece_max"] bytes,
are replayed by one workgroup each; only longer ones reach the per-document fallback.  Every expectation is the
oracle's, document by document, or vocab.replay's.  P = a tile's longest piece, M = the long kernel's, C = a
tile's core, asked inside the tests."""
import random

import numpy as np
import pytest

import encode_limits_lib as EL
from llmtokenizer_amd import api, synth, vocab
from test_encode_limits import _oracle_docs, count_case

pytestmark = pytest.mark.gpu


def _sizes():
    pi, M = api.piece_info(), api.long_piece_info()["piece_max"]
    assert M >= 16384 and M > pi["piece_max"]
    return pi["core"], pi["piece_max"], M


def _check(docs, merges):
    """the oracle's ids and offsets under "piece_long"; the documents of (P, M] bytes are the long kernel's, those
    beyond M the fallback's; returns (ids, id offsets, long_info)"""
    C, P, M = _sizes()
    oids, ooff = _oracle_docs(docs, merges)
    e = api.Engine(0)
    try:
        e.load(b"".join(docs))
        e.encode_docs(np.cumsum([0] + [len(d) for d in docs]).astype(np.uint64), merges, encoder="piece_long")
        ids, off, info, li, st = e.ids(), e.doc_offsets(), e.docs_info(), e.long_info(), e.stats()
    finally:
        e.close()
    assert off.tolist() == ooff.tolist()
    assert ids.size == oids.size and (ids == oids).all()
    assert st["enc_path"] == 4 and st["n_out"] == oids.size
    over = sum(len(d) > M for d in docs)
    assert info["docs_fallback"] == over and info["tiles"] == -(-sum(map(len, docs)) // C)
    assert (li["long_pieces"], li["long_fallback"]) == (sum(P < len(d) <= M for d in docs), over)
    assert (li["workgroups"] >= 1) == (len(b"".join(docs)) > 0)
    return ids, off, li


# ---- 1. lengths around both limits, 3. the long pieces among the tiles (the extra gather entries, stage[])

GEOMETRY = {
    "lengths_around_both_limits": lambda C, P, M: [P, P + 1, M - 1, M, M + 1],
    "starts_at_the_last_byte_of_a_core": lambda C, P, M: [C - 1, P + 5, 3],
    "back_to_back": lambda C, P, M: [7, P + 1, P + 300, 2],
    "between_one_byte_and_empty_pieces": lambda C, P, M: [1, 0, P + 9, 0, 1, 1],
    "last_document": lambda C, P, M: [5, C, P + 77],
    "cores_wholly_inside": lambda C, P, M: [3, P + 1 + 3 * C, 4, P + 2 * C],
}


@pytest.mark.parametrize("name", list(GEOMETRY))
def test_long_pieces_among_the_tiles(name):
    rng = random.Random(len(name))
    merges = EL._random_merges(random.Random(5), b"abcd", 300, eq=0.2)
    docs = [bytes(rng.choice(b"abcd") for _ in range(n)) for n in GEOMETRY[name](*_sizes())]
    ids, _, li = _check(docs, merges)
    assert ids.max() > 255 and li["long_rounds"] >= 1


# ---- 2. a == a runs: which token of a run pairs comes from the run's head and the token's ordinal

RUNS = np.array([[97, 97], [256, 256], [257, 257], [98, 256]], dtype=np.uint32)
RUN_DOCS = {
    "even_beside_odd": lambda M: [b"a" * M, b"a" * (M - 1)],
    "b_first": lambda M: [b"b" + b"a" * (M - 1)],
    # 16 positions a thread in the first round: the b sits at an odd offset, last of a thread's range
    "cut_at_a_range_edge": lambda M: [b"a" * (16 * 37 - 1) + b"b" + b"a" * (M - 16 * 37)],
    "cut_after_a_range_edge": lambda M: [b"a" * (16 * 37 + 1) + b"b" + b"a" * (M - 16 * 37 - 2)],
}


@pytest.mark.parametrize("name", list(RUN_DOCS))
def test_runs(name):
    docs = RUN_DOCS[name](_sizes()[2])
    ids, off, li = _check(docs, RUNS)
    assert li["long_rounds"] in (3, 4)
    if name == "even_beside_odd":
        assert ids[off[1] - 1] == 258 and ids[off[2] - 1] == 97


# ---- 4. depth: the rounds of a long piece are its merges one after the other

def test_depth():
    chain = EL.chain_list(20)
    deep = EL.expand(chain, 256 + 19)  # 21 bytes, 20 merges one after the other
    P = _sizes()[1]
    ids, _, li = _check([b"ab", deep * (P // len(deep) + 1), deep], chain)
    assert li["long_rounds"] == 20 and (ids == 256 + 19).sum() == P // len(deep) + 2


# ---- 5. ids above 65,535 inside a long piece

def test_ids_above_16_bits():
    c = count_case("two_layer", 70000)
    step = _sizes()[1] + 300
    ids, _, li = _check([c.text[i:i + step] for i in range(0, len(c.text), step)], c.merges)
    assert li["long_pieces"] >= 2 and (ids > 65535).any()


# ---- 6. through the tokenizer, encoder left at "auto"

def test_tokenizer_long_pieces():
    trained = api.train_split(synth.english_like(65536), rule="cl100k", max_merges=300)
    k = 65300 - len(trained)  # padding that never matches, as in test_tokenizer_beyond_65279_merges
    pad = np.stack([np.ones(k, np.uint32), 255 + len(trained) + np.arange(k, dtype=np.uint32)], axis=1)
    pad[0] = (1, 2)
    specials = [b"<|endoftext|>", b"<|pad|>"]
    v = vocab.Vocab.from_merges(np.vstack([trained, pad]), "cl100k", specials)
    word = "".join(random.Random(3).choice("etaoinshr") for _ in range(3000))
    texts = ["see " + word + " end", "a" + " " * 2000 + "b", "", word + "<|endoftext|>" + "-" * 1500 + "\n", "tail"]
    rank = {tuple(p): r for r, p in reversed(list(enumerate(trained.tolist())))}
    want, nlong = [], 0
    for raw in (t.encode() for t in texts):
        off, at, which = api.split_host_special(raw, "cl100k", specials)
        sp = dict(zip(at.tolist(), which.tolist()))
        nlong += int((np.diff(off.astype(np.int64)) > _sizes()[1]).sum())
        want.append([x for d, (a, b) in enumerate(zip(off.tolist(), off.tolist()[1:]))
                     for x in ([256 + 65300 + sp[d]] if d in sp else vocab.replay(list(raw[a:b]), rank))])
    tk = vocab.Tokenizer(v)
    try:
        ids, toff = tk.encode_batch(texts)
        st, info, li = tk._eng().stats(), tk._eng().docs_info(), tk._eng().long_info()
        assert [ids[a:b].tolist() for a, b in zip(toff.tolist(), toff.tolist()[1:])] == want
        assert st["enc_path"] == 4 and info["docs_fallback"] == 0
        assert nlong == 4 and (li["long_pieces"], li["long_fallback"]) == (nlong, 0)
        assert tk.decode_batch(ids, toff) == [t.encode() for t in texts]
    finally:
        tk.close()

"""Training on the pieces of a split (train_split.hip, bpe_gpu_train_split & co.):
merges, stop reason and counters equal the plain-Python restatement
(tests/train_split_ref.py) exactly; the piece table is the multiset of pieces."""
import ctypes
import random
from collections import Counter

import numpy as np
import pytest

import train_split_ref as R
from llmtokenizer_amd import _lib, api
from llmtokenizer_amd.synth import english_like, synth_bytes

pytestmark = pytest.mark.gpu

ESTATE = "call out of order"
ONE_PIECE = (np.zeros(256, np.uint8), np.zeros(16, np.uint16))


def _random_rule(rng, k):
    """the rules of tests/test_gpu_split.py: k even 16 classes (short pieces), k odd 3 (long ones)"""
    hi = 16 if k % 2 == 0 else 3
    cls = rng.integers(0, hi, 256).astype(np.uint8)
    brk = rng.integers(0, 1 << 16, 16).astype(np.uint16)
    if k % 4 == 1:
        brk &= rng.integers(0, 1 << 16, 16).astype(np.uint16)
    return cls, brk


def _start_at(ch):
    """a piece starts at every byte `ch`"""
    cls = np.zeros(256, np.uint8)
    cls[ch] = 1
    brk = np.zeros(16, np.uint16)
    brk[0] = brk[1] = 0x2
    return cls, brk


def _tables(rule):
    return api.split_rule(rule) if isinstance(rule, str) else rule


@pytest.fixture(scope="module")
def eng():
    e = api.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def dedup_max(eng):
    eng.load(b"ab ab")
    eng.split("words")
    eng.train_split()
    return eng.train_split_info()["dedup_max"]


def _check(eng, data, rule, max_merges=-1, what=None):
    """load, split, train_split against the restatement; returns (merges, info, pieces)"""
    pieces = R.pieces_of(data, *_tables(rule))
    want, stop, _ = R.train(pieces, max_merges)
    eng.load(data)
    assert eng.split(rule) == len(pieces), what
    k = eng.train_split(max_merges)
    got = eng.split_merges()
    assert got.dtype == np.uint32 and got.shape == (k, 2), what
    assert [tuple(m) for m in got.tolist()] == want, what
    info = eng.train_split_info()
    assert info["stop_reason"] == stop and info["merges"] == len(want) == k and info["pieces"] == len(pieces), what
    return got, info, pieces


def _check_table(eng, data, pieces, info):
    """the piece table: counts sum to the pieces, its expansion is the multiset of pieces, entries of at
    most dedup_max bytes are pairwise distinct and start where their bytes first occur"""
    st, ln, ct = eng.piece_table()
    assert st.size == ln.size == ct.size == info["entries"]
    assert (np.diff(st.astype(np.int64)) > 0).all()
    assert int(ct.sum()) == len(pieces) == info["pieces"]
    assert int(ln.sum()) == info["entry_bytes"]
    rows = [(data[int(s):int(s) + int(n)], int(c), int(s)) for s, n, c in zip(st, ln, ct)]
    expansion = Counter()
    for b, c, _ in rows:
        expansion[b] += c
    assert expansion == Counter(pieces)
    short = [(b, s) for b, _, s in rows if len(b) <= info["dedup_max"]]
    assert len({b for b, _ in short}) == len(short)
    first, o = {}, 0
    for p in pieces:
        first.setdefault(p, o)
        o += len(p)
    assert all(first[b] == s for b, s in short)
    assert all(c == 1 for b, c, _ in rows if len(b) > info["dedup_max"])
    assert info["long_pieces"] == sum(1 for p in pieces if len(p) > info["dedup_max"])


# ---------------------------------------------------------------- 1. the examples

def test_the_line_example():
    data = b"ab\n" * 8
    assert api.train_split(data, "lines").tolist() == [[97, 98], [256, 10]]
    assert api.train_bytes(data)[0].shape[0] > 2  # the stream trainer goes on across the line ends
    assert api.train_split(b"a a a a a a", "words").tolist() == [[32, 97]]


# ---------------------------------------------------------------- 2. against the restatement

CORPORA = {"english": lambda n: english_like(n), "seed3": lambda n: synth_bytes(3, n)}
RULES = {"words": "words", "lines": "lines", "random0": _random_rule(np.random.default_rng(77), 0),
         "random1": _random_rule(np.random.default_rng(78), 1)}


@pytest.mark.parametrize("rule", sorted(RULES))
@pytest.mark.parametrize("corpus", sorted(CORPORA))
def test_200_merges_equal_the_restatement(eng, corpus, rule):
    data = CORPORA[corpus](65536)
    _, info, pieces = _check(eng, data, RULES[rule], 200, what=(corpus, rule))
    _check_table(eng, data, pieces, info)


def test_the_random_corpus_ties_early():
    pieces = R.pieces_of(synth_bytes(3, 65536), *api.split_rule("words"))
    assert R.train(pieces, 3)[2] == 1  # (the tie rule decides from the second merge on in the cases above)


@pytest.mark.parametrize("rule", ["words", "lines", "random1"])
@pytest.mark.parametrize("corpus", sorted(CORPORA))
def test_until_the_stop_rule(eng, corpus, rule):
    _, info, _ = _check(eng, CORPORA[corpus](4096), RULES[rule], -1, what=(corpus, rule))
    assert info["stop_reason"] == 1


# ---------------------------------------------------------------- 3. one piece is the stream

def test_one_piece_equals_stream_training(eng):
    data = english_like(65536)
    eng.load(data)
    assert eng.split(ONE_PIECE) == 1
    assert eng.train_split(32) == 32
    assert eng.split_merges().tolist() == api.train_bytes(data, 32)[0].tolist()
    assert eng.train_split_info()["stop_reason"] == 2


# ---------------------------------------------------------------- 4. the longest piece that is deduplicated

def test_pieces_around_dedup_max(eng, dedup_max):
    rng = random.Random(9)
    longs = [bytes(rng.choice(b"abc") for _ in range(dedup_max + d)) for d in (-2, -1, 0, 1) for _ in range(2)]
    words = []
    for _ in range(400):
        words.append(rng.choice([b"ab", b"abc", b"b", b"cab", b"abcabc"]))
        if rng.random() < 0.06:
            words.append(rng.choice(longs))
    for p in longs * 3:
        words.insert(rng.randrange(len(words)), p)
    data = b" ".join(words)
    _, info, pieces = _check(eng, data, "words", 60)
    # (a piece is a word with its leading space: lengths dedup_max - 1 .. dedup_max + 2)
    assert {dedup_max - 1, dedup_max, dedup_max + 1, dedup_max + 2} <= {len(p) for p in pieces}
    assert info["long_pieces"] >= 12
    _check_table(eng, data, pieces, info)


# ---------------------------------------------------------------- 5. weights and table pressure

def test_a_count_above_16_bits(eng):
    data = b"hello " * 70000
    _, info, pieces = _check(eng, data, "words", 20)
    assert info["entries"] == 3 and max(Counter(pieces).values()) == 69999
    _check_table(eng, data, pieces, info)


def test_every_piece_distinct_grows_the_table(eng, monkeypatch):
    monkeypatch.setenv("BPE_TS_SLOTS", "1024")
    alpha = bytes(range(0x80, 0x80 + 40))  # (class 1 of the words rule: 40^3 = 64,000 words)
    words = [bytes((alpha[i % 40], alpha[i // 40 % 40], alpha[i // 1600])) for i in range(50000)]
    random.Random(4).shuffle(words)
    data = b" ".join(words)
    _, info, pieces = _check(eng, data, "words", 8)
    assert info["entries"] == info["pieces"] == 50000
    assert info["table_slots"] >= 4 * 1024  # grown at least once from the 1,024 slots it began with
    _check_table(eng, data, pieces, info)


def test_all_pieces_identical(eng):
    data = b"abcab\n" * 3000
    _, info, pieces = _check(eng, data, "lines")
    assert info["entries"] == 1 and info["entry_bytes"] == 6
    _check_table(eng, data, pieces, info)


@pytest.mark.parametrize("data", [b"", b"a", b"aa", b"ab", b"a\n"])
def test_tiny_inputs(eng, data):
    for rule in ("words", "lines"):
        got, info, pieces = _check(eng, data, rule)
        assert got.shape == (0, 2) and info["stop_reason"] == 1
        assert eng.piece_table()[0].size == info["entries"] == len(set(pieces))


def test_piece_starts_around_tile_and_wave_steps(eng):
    tile = api.split_info()["tile"]
    rng = random.Random(6)
    n = 2 * tile + 100
    for d in (-1, 0, 1):
        buf = bytearray(rng.choice(b"axy") for _ in range(n))
        starts = sorted({1024 + d, tile + d, tile + 1024 + d, 2 * tile + d, 64 + d, 256 + d})
        for p in starts:
            buf[p] = ord("c")
        data = bytes(buf)
        _, info, pieces = _check(eng, data, _start_at(ord("c")), 40, what=d)
        assert info["pieces"] == len(starts) + 1
        _check_table(eng, data, pieces, info)


# ---------------------------------------------------------------- 6. runs

RUNS = {
    "short runs": (b"aaaa aaa aaaaa a\n" * 300, "words"),
    "short runs, lines": (b"aaaa aaa aaaaa a\n" * 300, "lines"),
    "one line of 70,001": (b"a" * 70001, "lines"),
    "the run cut at an odd offset": (b"a" * 33333 + b"\n" + b"a" * 36668, "lines"),
    "a run of a merged id": (b"ab" * 5000 + b"\n" + b"ab" * 777 + b"a\n" + b"b" + b"ab" * 30, "lines"),
}


@pytest.mark.parametrize("name", sorted(RUNS))
def test_runs(eng, name):
    data, rule = RUNS[name]
    got, info, _ = _check(eng, data, rule, what=name)
    assert info["stop_reason"] == 1 and any(a == b for a, b in got.tolist())


# ---------------------------------------------------------------- 7. state and lifetime

def test_state_and_lifetime():
    data = english_like(30000)
    cls, brk = api.split_rule("words")
    pieces = R.pieces_of(data, cls, brk)
    e = api.Engine(0)
    try:
        with pytest.raises(api.BpeError, match=ESTATE):
            e.train_split()  # nothing loaded
        e.load(data)
        with pytest.raises(api.BpeError, match=ESTATE):
            e.train_split()  # no split
        for call in (e.split_merges, e.train_split_info, e.piece_table):
            with pytest.raises(api.BpeError, match=ESTATE):
                call()
        assert e.split("words") == len(pieces)
        with pytest.raises(api.BpeError, match=ESTATE):
            e.split_merges()  # a split, not trained on yet
        off = e.split_offsets()
        assert e.train_split(150) == 150
        merges = e.split_merges()
        # the offsets and the bytes are untouched: encode over them with no reload and no new split
        assert (e.split_offsets() == off).all()
        e.encode_split(merges)
        ids, id_off = api.encode_batch(pieces, merges)
        assert (e.ids() == ids).all() and e.doc_offsets().tolist() == id_off.tolist()
        # every merge is usable: each id of the list occurs in the encoding or inside a later merge
        used = set(np.unique(ids).tolist()) | set(merges.reshape(-1).tolist())
        assert set(range(256, 256 + 150)) <= used
        # the encode keeps the results; a second run gives the same list
        assert e.split_merges().tolist() == merges.tolist()
        assert e.train_split(150) == 150 and e.split_merges().tolist() == merges.tolist()
        # a new split drops them, and so does a load
        e.split("lines")
        with pytest.raises(api.BpeError, match=ESTATE):
            e.split_merges()
        e.train_split(5)
        e.load(data)
        for call in (e.split_merges, e.train_split_info, e.piece_table, e.train_split):
            with pytest.raises(api.BpeError, match=ESTATE):
                call()
        # stream training drops the split and what was trained on it
        e.split("words")
        e.train_split(5)
        e.train(5)
        with pytest.raises(api.BpeError, match=ESTATE):
            e.split_merges()
        # trim, then a fresh load, split and train
        e.trim()
        with pytest.raises(api.BpeError, match=ESTATE):
            e.train_split()
        e.load(data)
        e.split("words")
        assert e.train_split(150) == 150 and e.split_merges().tolist() == merges.tolist()
    finally:
        e.close()


# ---------------------------------------------------------------- 8. the C layer

def test_c_layer(eng):
    rng = random.Random(51)
    text = bytes(rng.choice(b"ab ab\n7") for _ in range(3000))
    cls, brk = api.split_rule("words")
    want = R.train(R.pieces_of(text, cls, brk), 40)[0]
    assert [tuple(m) for m in api.train_split(text, "words", 40).tolist()] == want
    assert [tuple(m) for m in api.train_split(text, (cls, brk), 40).tolist()] == want
    L = _lib.load()
    buf = np.frombuffer(text, dtype=np.uint8)
    vp = ctypes.c_void_p
    arr = L.bpe_train_split(buf.ctypes.data_as(vp), buf.size, cls.ctypes.data_as(vp), brk.ctypes.data_as(vp), 40, 0)
    assert arr and arr.contents.last_index == 255 + len(want)
    assert [tuple(m) for m in api._arr_to_merges(arr).tolist()] == want
    L.dyn_arr_free(arr)
    # bad arguments and a class above 15 fail cleanly; the next call works
    assert not L.bpe_train_split(buf.ctypes.data_as(vp), buf.size, None, brk.ctypes.data_as(vp), 40, 0)
    assert not L.bpe_train_split(buf.ctypes.data_as(vp), buf.size, cls.ctypes.data_as(vp), None, 40, 0)
    assert not L.bpe_train_split(None, buf.size, cls.ctypes.data_as(vp), brk.ctypes.data_as(vp), 40, 0)
    bad = cls.copy()
    bad[200] = 16
    assert not L.bpe_train_split(buf.ctypes.data_as(vp), buf.size, bad.ctypes.data_as(vp), brk.ctypes.data_as(vp), 40, 0)
    with pytest.raises(api.BpeError):
        api.train_split(text, (bad, brk))
    assert [tuple(m) for m in api.train_split(text, "words", 40).tolist()] == want
    # the engine calls: NULL arguments
    assert L.bpe_gpu_train_split(eng.ctx, -1, None) != 0
    assert L.bpe_gpu_fetch_split_merges(eng.ctx, None, 0, None) != 0
    assert L.bpe_gpu_train_split_info(eng.ctx, None) != 0
    assert L.bpe_gpu_fetch_piece_table(eng.ctx, None, None, None, 0, None) != 0

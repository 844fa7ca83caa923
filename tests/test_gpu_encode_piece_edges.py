"""The piece-local encoders (k_enc_piece, k_enc_long, k_enc_piece_drop, k_enc_long_drop) where their own test
files do not reach:
  1. the dropout kernels against the C oracle at a threshold of 0 (a probability above 0 that drops nothing),
  2. more long pieces than workgroups: the stride loop takes a second and third piece, one beyond the limit among them,
  3. the id limit api.piece_info()["max_ids"] from both sides, ids with all 21 bits set beside offsets with all 14,
  4. a != b merges and table lookups at every value of a long piece's high offset bits under dropout,
  5. encode_split and the Tokenizer under dropout, id for id: the draws are keyed by the resident byte offset,
  6. a probe chain that runs across the end of the rank table.
Every expectation is the oracle's (oracle_lib.encode, document by document) or dropout_ref._replay's, which
test_dropout_ref.py holds to the oracle.  Sizes are asked of the library inside the tests: C = a tile's core, P = a
tile's longest piece, M = the long kernel's."""
import functools
import random
from types import SimpleNamespace

import numpy as np
import pytest

import encode_limits_lib as EL
import oracle_lib as O
import test_gpu_encode_long as TL
import test_gpu_encode_piece as TP
from dropout_ref import _mix64, _rank, _replay
from llmtokenizer_amd import api, synth, vocab
from llmtokenizer_amd.api import BpeError
from test_dropout_ref import (TINY, letters, long_geometry_docs, merges300, order_docs, piece_geometry_docs, replay_docs,
                              sizes)
from test_encode_limits import _oracle_docs, count_case

pytestmark = pytest.mark.gpu

SEEDS = (0, 2**64 - 1)


def _enc(docs, merges, encoder="piece_long", **kw):
    """the resident encode_docs of the joined documents: ids, id offsets and the three sets of counters"""
    e = api.Engine(0)
    try:
        e.load(b"".join(docs))
        e.encode_docs(np.cumsum([0] + [len(d) for d in docs]).astype(np.uint64), merges, encoder=encoder, **kw)
        return SimpleNamespace(ids=e.ids().tolist(), off=e.doc_offsets().tolist(), info=e.docs_info(), li=e.long_info(),
                               st=e.stats())
    finally:
        e.close()


def _flat(parts):
    return [x for p in parts for x in p], np.cumsum([0] + [len(p) for p in parts]).tolist()


def _same(got, want_ids, want_off, docs):
    """ids and id offsets, the piece path, and the counters of the documents' lengths"""
    C, P, M, _ = sizes()
    assert got.off == list(want_off)
    assert got.ids == list(want_ids)
    assert got.st["enc_path"] == 4 and got.st["n_out"] == len(want_ids)
    over = sum(len(d) > M for d in docs)
    assert got.info["docs_fallback"] == over
    assert (got.li["long_pieces"], got.li["long_fallback"]) == (sum(P < len(d) <= M for d in docs), over)


# ---- 1. the dropout kernels against the oracle: a probability above 0 whose threshold is 0

def _chain_docs():
    return [b"ab", TP.DEEP, b"abz", TP.DEEP * 3, b"", b"ba"], TP.CHAIN


def _depth_docs():
    chain = EL.chain_list(20)
    deep = EL.expand(chain, 256 + 19)
    return [b"ab", deep * (sizes()[1] // len(deep) + 1), deep], chain


def _above_16_bits_docs():
    c = count_case("two_layer", 70000)
    step = sizes()[1] + 300
    return [c.text[i:i + step] for i in range(0, len(c.text), step)], c.merges


THR0 = {f"order-{o[0]}": functools.partial(order_docs, o[0]) for o in TP.ORDER}
THR0.update({f"tiles-{n}": (lambda n=n: (piece_geometry_docs(n), merges300())) for n in TP.GEOMETRY})
THR0["one_round_beside_twenty"] = _chain_docs
THR0.update({f"long-{n}": (lambda n=n: (long_geometry_docs(n), merges300())) for n in TL.GEOMETRY})
THR0.update({f"runs-{n}": (lambda n=n: (TL.RUN_DOCS[n](sizes()[2]), TL.RUNS)) for n in TL.RUN_DOCS})
THR0["depth"] = _depth_docs
THR0["ids_above_16_bits"] = _above_16_bits_docs


@pytest.mark.parametrize("name", list(THR0))
def test_dropout_kernels_equal_the_oracle_at_threshold_0(name):
    """dropout=1e-12 is above 0, so encode_drop.hip's two kernels run, and floor(1e-12 * 2^32) = 0, so they drop
    nothing: by the contract's p = 0 sentence the ids are the oracle's, whatever the seed."""
    assert int(TINY * 2**32) == 0 and TINY > 0
    docs, merges = THR0[name]()
    oids, ooff = _oracle_docs(docs, merges)
    runs = [_enc(docs, merges, dropout=TINY, seed=s) for s in SEEDS]
    for got in runs:
        _same(got, oids.tolist(), ooff.tolist(), docs)
    assert (runs[0].ids, runs[0].off) == (runs[1].ids, runs[1].off)


# ---- 2. more long pieces than workgroups

@functools.lru_cache(maxsize=None)
def _stride_batch():
    """605 documents: 599 of (P, M] bytes (lengths P + 1 .. P + 400 in turn; a few of M, M - 1 and 5,000 bytes among
    the first 256, so that a workgroup's second piece is much shorter than its first), one of M + 1 late in the
    batch, three short and two empty ones"""
    C, P, M, _ = sizes()
    lens = [P + 1 + i % 400 for i in range(600)]
    for i, n in {3: M, 17: M - 1, 64: 5000, 100: M, 130: 5003, 200: M - 1, 250: M}.items():
        lens[i] = n
    lens[470] = M + 1
    for at, n in ((590, 0), (400, 3), (300, 1), (129, 0), (5, 700)):
        lens.insert(at, n)
    rng = random.Random(2)
    docs = [letters(rng, n) for n in lens]
    assert len(docs) == 605 and 700_000 < sum(lens) < 900_000
    assert sum(P < n <= M for n in lens) == 599 and sum(n > M for n in lens) == 1
    oids, ooff = _oracle_docs(docs, merges300())
    return docs, oids.tolist(), ooff.tolist()


def _stride_counters(got):
    assert got.li["workgroups"] == 256 and got.li["long_pieces"] == 599 and got.li["long_fallback"] == 1


def test_more_long_pieces_than_workgroups():
    """600 listed pieces on 256 workgroups: every workgroup takes a second piece, most a third, with tok[], rk[] and
    the sixteen-word arrays left by the one before; the piece beyond M is skipped in the middle of a stride (the
    list's order is any, so only the counts are asserted)."""
    docs, oids, ooff = _stride_batch()
    got = _enc(docs, merges300())
    _same(got, oids, ooff, docs)
    _stride_counters(got)


def test_more_long_pieces_than_workgroups_threshold_0():
    docs, oids, ooff = _stride_batch()
    got = _enc(docs, merges300(), dropout=TINY, seed=77)
    _same(got, oids, ooff, docs)
    _stride_counters(got)


def test_more_long_pieces_than_workgroups_dropout():
    """p = 0.3 against the replay; the document beyond M is the fallback's and keeps its deterministic ids"""
    docs, oids, ooff = _stride_batch()
    M = sizes()[2]
    want = replay_docs(docs, merges300(), 0.3, 9, batch=True)
    big = [len(d) for d in docs].index(M + 1)
    want[big] = oids[ooff[big]:ooff[big + 1]]
    wids, woff = _flat(want)
    got = _enc(docs, merges300(), dropout=0.3, seed=9)
    _same(got, wids, woff, docs)
    _stride_counters(got)
    assert len(wids) > len(oids)  # (dropped merges leave more ids)


# ---- 3. the id limit

LETTERS = EL._random_merges(random.Random(5), b"abcd", 60, eq=0.2)


@functools.lru_cache(maxsize=None)
def _limit_list():
    """(merges, K, rank of the real records): max_ids - 256 records, the first K = max_ids - 256 - 60 of them padding
    that never matches (byte 1, which no text holds, before the id of the record before), the last 60 LETTERS with
    every id above 255 moved up by K: their ids are max_ids - 60 .. max_ids - 1"""
    max_ids = sizes()[3]
    K = max_ids - 256 - 60
    pad = np.stack([np.ones(K, np.uint32), 255 + np.arange(K, dtype=np.uint32)], axis=1)
    pad[0] = (1, 2)
    real = LETTERS.astype(np.int64)
    real[real >= 256] += K
    merges = np.vstack([pad, real.astype(np.uint32)])
    assert merges.shape == (max_ids - 256, 2)
    merges.setflags(write=False)
    return merges, K, {tuple(m): K + j for j, m in reversed(list(enumerate(real.tolist())))}


@functools.lru_cache(maxsize=None)
def _limit_docs():
    """short documents (the bytes of the list's last ids), one of P, of P + 1 and of M bytes, and their replay at a
    threshold of 0"""
    C, P, M, max_ids = sizes()
    rng = random.Random(11)
    docs = [EL.expand(LETTERS, 256 + 59 - j) for j in range(8)] + [b"d", b""]
    docs += [letters(rng, n) for n in (40, P, P + 1, 7, M)]
    rank = _limit_list()[2]
    return docs, rank, replay_docs(docs, None, TINY, 0, rank)


def test_the_replay_reaches_the_last_ids():
    """on the reference alone: the expectation holds the list's last id, 2^21 - 1, and ids within 8 of it inside the
    M-byte piece's upper half, where the packed offset's high bits are set too"""
    C, P, M, max_ids = sizes()
    docs, rank, want = _limit_docs()
    assert max(x for w in want for x in w) == max_ids - 1 == (1 << 21) - 1
    assert min(x for w in want for x in w if x > 255) >= max_ids - 60
    long_ids, at = want[-1], 0
    assert len(docs[-1]) == M
    high = set()
    ln = EL.expansion_lengths(LETTERS)
    for x in long_ids:
        if x >= 256:
            high.add((at >> 11, x))
        at += ln[x - _limit_list()[1]] if x >= 256 else 1
    assert at == M
    assert {e for e, x in high} == set(range(8)) and any(e == 7 and x >= max_ids - 8 for e, x in high)


def test_ids_at_the_limit():
    """Three encodes of one list of exactly max_ids - 256 merges (each builds the 64 MiB table anew): deterministic,
    dropout at a threshold of 0, dropout 0.25.  The first two equal each other and the replay at threshold 0."""
    merges, K, rank = _limit_list()
    docs, _, want = _limit_docs()
    wids, woff = _flat(want)
    det = _enc(docs, merges)
    _same(det, wids, woff, docs)
    thr0 = _enc(docs, merges, dropout=TINY, seed=5)
    _same(thr0, wids, woff, docs)
    assert max(det.ids) == sizes()[3] - 1
    dids, doff = _flat(replay_docs(docs, None, 0.25, 5, rank))
    drop = _enc(docs, merges, dropout=0.25, seed=5)
    _same(drop, dids, doff, docs)
    assert max(drop.ids) >= sizes()[3] - 8 and drop.ids != det.ids


def test_one_merge_beyond_the_id_limit():
    """("auto" without dropout is left out: it would send every document alone through a two-million-merge list)"""
    merges = np.vstack([_limit_list()[0], np.array([[1, 3]], dtype=np.uint32)])
    assert 256 + len(merges) == sizes()[3] + 1
    e = api.Engine(0)
    try:
        e.load(b"abcdabcd")
        for kw in ({"encoder": "piece"}, {"encoder": "piece_long"}, {"encoder": "auto", "dropout": 0.1}):
            with pytest.raises(BpeError, match="out of range"):
                e.encode_docs([0, 3, 8], merges, **kw)
    finally:
        e.close()


# ---- 4. high offsets under dropout with a != b merges

@functools.lru_cache(maxsize=None)
def _high_docs():
    """a one-byte document first: the long pieces start at odd resident offsets"""
    M = sizes()[2]
    rng = random.Random(4)
    return [b"c", letters(rng, M), letters(rng, M - 1), b"ab"]


@pytest.mark.parametrize("seed", [1, 0xDEADBEEFCAFEF00D])
@pytest.mark.parametrize("p", [0.1, 0.5, 0.9])
def test_long_pieces_of_mixed_letters_under_dropout(p, seed):
    docs = _high_docs()
    merges = merges300()
    want = replay_docs(docs, merges, p, seed, batch=True)
    ln = EL.expansion_lengths(merges)
    for d, w in zip(docs[1:3], want[1:3]):  # from the reference: merged tokens start in every eighth of the piece
        starts = np.cumsum([0] + [ln[x] for x in w])[:-1]
        assert int(starts[-1]) + ln[w[-1]] == len(d)
        assert {int(s) >> 11 for s, x in zip(starts, w) if x > 255} == set(range(8))
        assert any(merges[x - 256][0] != merges[x - 256][1] for x in w if x > 255)
    wids, woff = _flat(want)
    _same(_enc(docs, merges, dropout=p, seed=seed), wids, woff, docs)


def test_the_largest_threshold():
    """p = 1 - 2^-33: floor(p * 2^32) = 2^32 - 1, the other end of the threshold's range (a pair is kept only when its
    draw is 0xFFFFFFFF)"""
    p = 1 - 2.0**-33
    assert p < 1 and int(p * 4294967296.0) == 2**32 - 1
    P = sizes()[1]
    rng = random.Random(8)
    docs = [letters(rng, n) for n in (300, 1, 0, P, P + 1, 2500, 2)]
    wids, woff = _flat(replay_docs(docs, merges300(), p, 3))
    _same(_enc(docs, merges300(), dropout=p, seed=3), wids, woff, docs)


# ---- 5. encode_split and the Tokenizer under dropout, exactly

SPECIALS = [b"<|endoftext|>", b"<|pad|>"]
P_SPLIT = 0.3


@functools.lru_cache(maxsize=None)
def _trained():
    m = api.train_split(synth.english_like(65536), rule="cl100k", max_merges=300)
    assert len(m) == 300
    m.setflags(write=False)
    return m


def _word(seed, n):
    return "".join(random.Random(seed).choice("etaoinshr") for _ in range(n))


def _text():
    """specials at the start, in the middle and at the end, runs of spaces, a word longer than P, non-ASCII"""
    return ("<|endoftext|>the quick brown fox   jumps over    the lazy dog\n\n" + _word(3, sizes()[1] + 500) +
            " then<|pad|><|endoftext|> café naïve 中文 the other thing, the same thing" + " " * 40 +
            "the end of the text<|endoftext|>").encode()


def _expect_pieces(raw, off, base, merges, seed, shift=None):
    """the ids of every piece [off[d], off[d + 1]) of raw, a special piece its one id, every other the replay keyed
    at base + off[d] (shift: at that constant, whatever the piece's place)"""
    hoff, at, which = api.split_host_special(raw, "cl100k", SPECIALS)
    assert hoff.tolist() == list(off)
    sp = dict(zip(at.tolist(), which.tolist()))
    rank = _rank(merges)
    return [[256 + len(merges) + sp[d]] if d in sp else
            _replay(raw[a:b], base + a if shift is None else shift, rank, P_SPLIT, seed)
            for d, (a, b) in enumerate(zip(off, off[1:]))]


@pytest.mark.parametrize("seed", [6, 2**64 - 1])
def test_encode_split_under_dropout(seed):
    """Pieces from the device splitter, each drawn at its resident byte offset.  The control: replaying every piece as
    if it lay at offset 0 gives other ids for this text, so a kernel that keyed its draws by the offset in the piece
    would fail here."""
    merges, text = _trained(), _text()
    e = api.Engine(0)
    try:
        e.load(text)
        e.split("cl100k", specials=SPECIALS)
        e.encode_split(merges, encoder="auto", dropout=P_SPLIT, seed=seed)
        raw, off = e.bytes(), e.split_offsets().tolist()
        ids, ioff, st, li = e.ids().tolist(), e.doc_offsets().tolist(), e.stats(), e.long_info()
    finally:
        e.close()
    assert raw == text
    want = _expect_pieces(raw, off, 0, merges, seed)
    assert sum(len(w) == 1 and w[0] >= 256 + len(merges) for w in want) == 4
    wids, woff = _flat(want)
    assert ioff == woff and ids == wids
    assert st["enc_path"] == 4 and li["long_pieces"] == 1
    assert _flat(_expect_pieces(raw, off, 0, merges, seed, shift=0))[0] != wids


def test_encode_split_of_a_text_batch_under_dropout():
    """A text batch keeps a gap byte behind every text, so text k's pieces lie k bytes further into the resident
    buffer than in the plain join that split_offsets() describes: the draws follow the resident offset.  A gap piece
    has no id, as in the deterministic run of the same engine."""
    merges = _trained()
    texts = [b"the quick brown fox", b"", b"<|endoftext|>", _text(), "naïve  the lazy dog ".encode(), b"the end"]
    e = api.Engine(0)
    try:
        e.load_texts(texts)
        e.split("cl100k", specials=SPECIALS)
        e.encode_split(merges, encoder="auto")
        det = (e.ids().tolist(), e.doc_offsets().tolist(), e.text_offsets().tolist())
        e.split("cl100k", specials=SPECIALS)
        e.encode_split(merges, encoder="auto", dropout=P_SPLIT, seed=21)
        raw, off = e.bytes(), e.split_offsets().tolist()
        got = (e.ids().tolist(), e.doc_offsets().tolist(), e.text_offsets().tolist())
        st = e.stats()
    finally:
        e.close()
    assert raw == b"".join(t + b"\0" for t in texts)
    tb = np.cumsum([0] + [len(t) for t in texts]).tolist()  # the texts in the plain join
    assert off[-1] == tb[-1]
    want_det, want, plain, toff, toff_det, cut = [], [], [], [0], [0], 0
    for k, t in enumerate(texts):
        n = sum(tb[k] <= a < tb[k + 1] for a in off[:-1])  # this text's pieces
        po = [a - tb[k] for a in off[cut:cut + n]] + [len(t)]
        cut += n
        if t:
            assert raw[tb[k] + k:tb[k + 1] + k] == t
            want += _expect_pieces(t, po, tb[k] + k, merges, 21)
            plain += _expect_pieces(t, po, tb[k], merges, 21)  # (the control: keyed as if there were no gap bytes)
            hoff, at, which = api.split_host_special(t, "cl100k", SPECIALS)
            sp = dict(zip(at.tolist(), which.tolist()))
            want_det += [[256 + len(merges) + sp[d]] if d in sp else O.encode(t[a:b], merges).tolist()
                         for d, (a, b) in enumerate(zip(po, po[1:]))]
        toff.append(sum(map(len, want)))
        toff_det.append(sum(map(len, want_det)))
    assert cut == len(off) - 1
    assert det == _flat(want_det) + (toff_det,)
    assert got == _flat(want) + (toff,) and st["enc_path"] == 4
    assert len(got[0]) > len(det[0]) and plain != want


def _resident_want(tk, merges, seed):
    e = tk._eng()
    return _flat(_expect_pieces(e.bytes(), e.split_offsets().tolist(), 0, merges, seed))[0]


def test_tokenizer_seed_sequence():
    """Tokenizer(v, dropout=0.3, seed=11): the first three encodes, of whatever kind, use the seeds 11, 12 and 13.
    What vocab.py does with an explicit seed=: the call uses that seed and still counts as a dropout encode made, so
    the implicit call after it uses the tokenizer's seed plus the number of ALL dropout encodes before it."""
    merges = _trained()
    v = vocab.Vocab.from_merges(merges, "cl100k", SPECIALS)
    text = _text().decode()
    texts = ["the quick brown fox", "", "one<|endoftext|>two  three\n", "café naïve 中文 ok", "tail  "]
    tk, ref, tk3 = (vocab.Tokenizer(v, dropout=P_SPLIT, seed=s) for s in (11, 500, 11))
    try:
        first = tk.encode(text).tolist()
        assert first == _resident_want(tk, merges, 11)
        assert first == ref.encode(text, seed=11).tolist()
        ids, toff = tk.encode_batch(texts)
        rids, rtoff = ref.encode_batch(texts, seed=12)
        assert (ids.tolist(), toff.tolist()) == (rids.tolist(), rtoff.tolist())
        assert ids.tolist() != ref.encode_batch(texts, seed=11)[0].tolist()
        rows, n = tk.encode_packed(texts, 16, 0)
        rrows, rn = ref.encode_packed(texts, 16, 0, seed=13)
        assert n == rn and rows.tolist() == rrows.tolist()
        assert tk.encode(text).tolist() == ref.encode(text, seed=14).tolist()
        # an explicit seed in between
        assert tk3.encode(text, seed=99).tolist() == ref.encode(text, seed=99).tolist()
        assert tk3.encode(text).tolist() == ref.encode(text, seed=12).tolist() != first
    finally:
        tk.close(), ref.close(), tk3.close()


def test_tokenizer_seed_wraps_at_2_64():
    merges = _trained()
    v = vocab.Vocab.from_merges(merges, "cl100k", SPECIALS)
    text = _text().decode()
    tk, ref = vocab.Tokenizer(v, dropout=P_SPLIT, seed=2**64 - 1), vocab.Tokenizer(v, dropout=P_SPLIT, seed=0)
    try:
        assert tk.encode(text).tolist() == _resident_want(tk, merges, 2**64 - 1)
        second = tk.encode(text).tolist()  # seed 2^64: api takes it mod 2^64
        assert second == ref.encode(text).tolist() == _resident_want(ref, merges, 0)
    finally:
        tk.close(), ref.close()


# ---- 6. a probe chain across the table's end

EP_H = 64        # engine.hip ep_table: the slots of a list with at most 16 records that name an id above 255
EP_ID_BITS = 21  # encode_piece.hip


def _home(u, v):
    return _mix64((u << EP_ID_BITS) | v) & 0xFFFFFFFF & (EP_H - 1)


def _slots(merges):
    """ep_table's open addressing, record by record: {(u, v): (home slot, slot)}"""
    used, out = set(), {}
    for r, (u, v) in enumerate(merges):
        if (u | v) < 256 or u >= 256 + r or v >= 256 + r or (u, v) in out:
            continue
        s = _home(u, v)
        while s in used:
            s = (s + 1) & (EP_H - 1)
        used.add(s)
        out[u, v] = (_home(u, v), s)
    return out


@functools.lru_cache(maxsize=None)
def _wrap_case():
    """40 byte-pair merges over a..h, then 12 records that name an id above 255 and whose home slot is 62 or 63,
    each kept only if the oracle's ids of expand(u) + expand(v) hold its id; then pairs that are no record and hash
    into the chain"""
    rng = random.Random(6)
    pairs = [(a, b) for a in b"abcdefgh" for b in b"abcdefgh"]
    rng.shuffle(pairs)
    merges = pairs[:40]
    docs = []
    cands = list(b"abcdefgh") + list(range(256, 296))
    tries = [(u, v) for u in cands for v in cands if (u | v) >= 256 and _home(u, v) >= EP_H - 2]
    rng.shuffle(tries)
    for u, v in tries:
        if len(merges) == 52:
            break
        m = np.array(merges + [(u, v)], dtype=np.uint32)
        new = docs + [EL.expand(m, u) + EL.expand(m, v)]
        if all(256 + 40 + r in O.encode(d, m).tolist() for r, d in enumerate(new)):  # (the earlier ones' ids stay)
            merges.append((u, v))
            docs = new
    assert len(merges) == 52
    m = np.array(merges, dtype=np.uint32)
    m.setflags(write=False)
    slots = _slots(merges)
    chain = {s for _, s in slots.values()}
    absent, miss = [], []
    for u, v in ((u, v) for u in cands for v in cands):
        if (u | v) < 256 or (u, v) in slots or _home(u, v) not in chain or len(absent) == 10:
            continue
        d = EL.expand(m, u) + EL.expand(m, v)
        ids = O.encode(d, m).tolist()
        if (u, v) in zip(ids, ids[1:]):  # the two meet in the replay, are looked up, and stay apart
            absent.append((u, v))
            miss.append(d)
    return m, slots, docs, absent, miss


def test_the_wrap_case_wraps():
    """On the reference alone.  _home and _slots mirror ep_table's rule for H (64 slots while at most 16 records name
    an id above 255), its hash (mix64 of u << 21 | v, the low bits) and its linear probe; if any of them changes in
    engine.hip, this search and the test below lose their point WITHOUT failing."""
    m, slots, docs, absent, miss = _wrap_case()
    assert sum((u | v) >= 256 for u, v in m.tolist()) == 12 <= EP_H // 4
    at_end = [(h, s) for h, s in slots.values() if h >= EP_H - 2]
    assert len(at_end) >= 8 and sum(s < h for h, s in at_end) >= 6
    assert sorted(s for _, s in slots.values()) == list(range(10)) + [62, 63]  # one chain: 62, 63, 0, 1, ... 9
    assert len(absent) >= 6 and any(h >= EP_H - 2 for h in (_home(u, v) for u, v in absent))
    for r, d in enumerate(docs):
        assert 256 + 40 + r in O.encode(d, m).tolist()
    for (u, v), d in zip(absent, miss):
        ids = O.encode(d, m).tolist()
        assert (u, v) in zip(ids, ids[1:]) and (u, v) not in set(map(tuple, m.tolist()))


@pytest.mark.parametrize("how", ["piece", "piece_long", "threshold_0"])
def test_probe_chain_across_the_tables_end(how):
    """twelve records whose probe chain runs 62, 63, 0, 1, ... 9 (test_the_wrap_case_wraps), every one found, and
    pairs that are no record and probe through the same slots to the chain's end"""
    m, slots, docs, absent, miss = _wrap_case()
    P = sizes()[1]
    batch = docs + miss
    if how != "piece":
        both = b"".join(d + b"z" for d in docs + miss)  # (z is in no record: the documents stay apart)
        batch = batch + [both * (P // len(both) + 1)]
        assert len(batch[-1]) > P and set(range(296, 308)) <= set(O.encode(batch[-1], m).tolist())
    oids, ooff = _oracle_docs(batch, m)
    kw = {"dropout": TINY, "seed": 3} if how == "threshold_0" else {}
    got = _enc(batch, m, encoder="piece" if how == "piece" else "piece_long", **kw)
    _same(got, oids.tolist(), ooff.tolist(), batch)
    assert set(range(296, 308)) <= set(got.ids)

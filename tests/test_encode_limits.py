"""The window encoders at the limits their 16-bit LDS layout rests on
(encode_win.hip): EW_MAX_MERGES = 65279 merges (ids up to 0xFFFE, ranks up to
0xFEFE, just below the rk marks), EW_MAX_BATCHES = 256 layers (mask word 7,
bit 31) and EW_PENDCAP = 512 entries of the per-batch lookup list -- through
k_enc_win, its document twin (encode_docs.hip, encode_split), the shard-group
path, k_ew_gather's u16 unmap[] in dynamic LDS, the global replay beyond the
limits, and the decoder.  Everything is bit-exact against the oracle's
sequential replace passes.

The unmarked tests hold the inputs (encode_limits_lib.py) to what the GPU
tests depend on: the layer counts, and that the ids at the limit really occur
in the expected output."""
import functools
import random
from types import SimpleNamespace

import numpy as np
import pytest

import encode_limits_lib as EL
import oracle_lib as O
from llmtokenizer_amd import api

gpu = pytest.mark.gpu

M = 65279        # encode_win.hip EW_MAX_MERGES: the longest list the window encoders take
LAYERS = 256     # EW_MAX_BATCHES: the deepest plan
SHORT = 1900     # bytes of a text that is one window at the default halo (core = 2048 - 2 * 48 = 1952)
LONG = 4400      # three windows at halo 48 (core 1952) and at halo 256 (core 1536)
COUNTS = [("two_layer", M - 1), ("two_layer", M), ("two_layer", M + 1), ("two_layer", 70000),
          ("random", M - 1), ("random", M), ("random", M + 1)]
AT_LIMIT = [c for c in COUNTS if c[1] == M]


def _id(c):
    return f"{c[0]}-{c[1]}"


# ------------------------------------------------------------------ inputs, built once

@functools.lru_cache(maxsize=None)
def count_case(kind, m):
    """a list of m merges whose last id occurs in the output, a three-window
    text of its highest ids' expansions, that text's first window, and the
    oracle's ids of both"""
    rng = random.Random(m)
    if kind == "two_layer":
        base = EL.two_layer_list(m)
        ids = list(range(256 + m - 3000, 256 + m))
        rng.shuffle(ids)
        layer = 1  # (the pinned record must not open a third layer, nor land in the first)
    else:
        base = EL.random_list(random.Random(7), m)
        ln = EL.expansion_lengths(base)
        ids = [x for x in range(256 + m - 3000, 256 + m) if ln[x] <= 48]
        more = [x for x in range(256 + m - 12000, 256 + m - 3000) if ln[x] <= 48]
        rng.shuffle(ids)
        rng.shuffle(more)
        ids += more
        layer = None
    starts = []
    text = EL.text_for(base, rng, ids, LONG, starts=starts)
    short = text[:SHORT]
    merges = EL.pin_last(base, short, layer=layer)
    c = SimpleNamespace(kind=kind, m=m, merges=merges, text=text, short=short, starts=starts,
                        want=O.encode(text, merges), want_short=O.encode(short, merges), nb=EL.layers(merges)[0])
    for a in (c.merges, c.want, c.want_short):
        a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def chain_case(k, tail):
    """a k-layer chain (tail: followed by records the plan moves in front) and a
    single-window text: the deepest id's bytes three times, zz, a mid-depth id's"""
    rng = random.Random(1000 + k)
    merges = EL.chain_with_tail(k, rng) if tail else EL.chain_list(k)
    deep, mid = EL.expand(merges, 256 + k - 1), EL.expand(merges, 256 + k // 2)
    text = deep * 3 + b"zz" + mid
    if tail:
        text += bytes(rng.choice(EL.TAIL_ALPHABET) for _ in range(300))
    assert len(text) <= SHORT
    c = SimpleNamespace(kind="chain_tail" if tail else "chain", m=len(merges), merges=merges, text=text, short=text,
                        want=O.encode(text, merges), nb=EL.layers(merges)[0])
    c.want_short = c.want
    return c


@functools.lru_cache(maxsize=None)
def chain_long_case():
    """chain_with_tail(256) on three windows: the chain's ids and the tail's letters, mixed"""
    k = LAYERS
    rng = random.Random(77)
    merges = chain_case(k, True).merges
    pieces = [EL.expand(merges, 256 + k - 1), EL.expand(merges, 256 + k // 2), EL.expand(merges, 256 + 7)]
    text, starts = bytearray(), []
    while len(text) < LONG - 300:
        starts.append(len(text))
        text += rng.choice(pieces) + bytes(rng.choice(EL.TAIL_ALPHABET) for _ in range(rng.randint(0, 150)))
    text = bytes(text)
    return SimpleNamespace(kind="chain_tail", m=len(merges), merges=merges, text=text, starts=starts,
                           want=O.encode(text, merges), nb=LAYERS)


CHAINS = [(k, tail) for k in (LAYERS - 1, LAYERS, LAYERS + 1) for tail in (False, True)]


def all_cases():
    return [count_case(*c) for c in COUNTS] + [chain_case(*c) for c in CHAINS]


# ------------------------------------------------------------------ the inputs are what the GPU tests need

def test_layers_of_the_builders():
    for m in (EL.N_LAYER0 + 1, 20000, M, 70000):
        t = EL.two_layer_list(m)
        assert len(t) == m and len(set(map(tuple, t.tolist()))) == m
        assert EL.layers(t)[0] == 2 and not EL.relabeled(t)
    for k in (LAYERS - 1, LAYERS, LAYERS + 1):
        assert EL.layers(EL.chain_list(k))[0] == k and not EL.relabeled(EL.chain_list(k))
        t = EL.chain_with_tail(k, random.Random(k))
        assert len(t) > k + 2000 and EL.layers(t)[0] == k and EL.relabeled(t)
    # records that can never match (a forward reference) go into layer 0 and open no layer
    assert EL.layers(np.array([[97, 98], [300, 99], [256, 99]]))[1] == [0, 0, 1]
    # the same pair again, and an a == a merge on an id in use, come a layer later
    assert EL.layers(np.array([[97, 98], [97, 98], [98, 98], [99, 100]]))[1] == [0, 1, 2, 0]
    assert EL.relabeled(np.array([[97, 98], [97, 98], [98, 98], [99, 100]]))


@pytest.mark.parametrize("case", COUNTS, ids=_id)
def test_lists_as_the_gpu_tests_need_them(case):
    c = count_case(*case)
    assert len(c.merges) == c.m and len(c.short) <= SHORT and 3 * 1952 > len(c.text) > 2 * 1952
    bad = (c.merges >= 256 + np.arange(c.m)[:, None]).any()
    assert not bad  # every record valid: the one past the limit too
    if c.kind == "two_layer":
        assert c.nb == 2 and not EL.relabeled(c.merges)
    else:
        assert 2 <= c.nb <= LAYERS and EL.relabeled(c.merges)
    last = 256 + c.m - 1
    for want in (c.want, c.want_short):
        assert (want == last).any()
    hi = np.unique(c.want[c.want >= last - 2999])
    print(f"\n{_id(case)}: {c.nb} layers, {len(c.text)} bytes -> {c.want.size} ids, max {c.want.max()}, "
          f"{hi.size} distinct among the last 3000 ({np.unique(c.want_short[c.want_short >= last - 2999]).size} "
          f"in the first {len(c.short)} bytes), pinned {c.merges[-1].tolist()}")
    assert hi.size >= 50
    assert c.want.max() >= 65000 and c.want_short.max() >= 65000
    if c.m == 70000:
        assert (c.want >= 65536).sum() >= 50 and (c.want_short >= 65536).any()
    if c.m == M:
        assert last == 0xFFFE
    for text, want in ((c.text, c.want), (c.short, c.want_short)):
        got = O.encode_heap(text, c.merges)
        assert got.size == want.size and (got == want).all()
        assert O.decode(want, c.merges) == text


@pytest.mark.parametrize("case", CHAINS, ids=str)
def test_chains_as_the_gpu_tests_need_them(case):
    c = chain_case(*case)
    k, tail = case
    assert c.nb == k and EL.relabeled(c.merges) == tail
    assert (c.want == 256 + k - 1).sum() == 3 and (c.want == 256 + k // 2).sum() == 1
    got = O.encode_heap(c.text, c.merges)
    assert got.size == c.want.size and (got == c.want).all()
    if tail:
        assert (c.want >= 256 + k).sum() > 20  # the tail's records at work
    if tail and k == LAYERS:
        d = chain_long_case()  # the documents' three-window text
        assert 3 * 1952 > len(d.text) > 2 * 1952
        assert (d.want == 256 + k - 1).sum() >= 3 and (d.want >= 256 + k).sum() > 100


# ------------------------------------------------------------------ GPU

def _encode(text, merges):
    e = api.Engine(0)
    try:
        e.load(text)
        e.encode(merges)
        return e.ids(), e.stats()
    finally:
        e.close()


def _same(got, want):
    return got.size == want.size and bool((got == want).all())


@gpu
@pytest.mark.parametrize("case", COUNTS, ids=_id)
def test_merge_count_boundary_one_window(case):
    """up to EW_MAX_MERGES the window path with the plan's layers, one more merge and the global replay"""
    c = count_case(*case)
    ids, st = _encode(c.short, c.merges)
    print(f"\n{_id(case)} one window: enc_path {st['enc_path']}, iterations {st['iterations']}, layers {c.nb}")
    assert _same(ids, c.want_short)
    if c.m <= M:
        assert st["enc_path"] == 1
        assert st["iterations"] == c.nb
    else:
        assert st["enc_path"] == 2


@gpu
@pytest.mark.parametrize("halo", [48, 256])
@pytest.mark.parametrize("case", COUNTS, ids=_id)
def test_merge_count_boundary_three_windows(case, halo, monkeypatch):
    monkeypatch.setenv("BPE_EW_HALO", str(halo))
    c = count_case(*case)
    ids, st = _encode(c.text, c.merges)
    print(f"\n{_id(case)} halo {halo}: enc_path {st['enc_path']}, windows {st['enc_windows']}, iterations {st['iterations']}")
    assert _same(ids, c.want)
    assert st["n_out"] + st["occurrences"] == len(c.text)
    if st["enc_path"] == 1:
        assert st["enc_windows"] >= 3


@gpu
def test_half_full_hash_table(monkeypatch):
    """BPE_EW_HSCALE=2: 65279 keys in 131072 slots, long probe chains"""
    monkeypatch.setenv("BPE_EW_HSCALE", "2")
    c = count_case("random", M)
    for text, want in ((c.short, c.want_short), (c.text, c.want)):
        ids, st = _encode(text, c.merges)
        assert _same(ids, want)
    ids, st = _encode(c.short, c.merges)
    assert st["enc_path"] == 1 and st["iterations"] == c.nb


@gpu
@pytest.mark.parametrize("case", CHAINS, ids=str)
def test_layer_boundary(case):
    """256 layers use mask word 7, bit 31 and b << 16 at b = 255; 257 do not fit"""
    c = chain_case(*case)
    ids, st = _encode(c.text, c.merges)
    print(f"\nchain {case}: enc_path {st['enc_path']}, iterations {st['iterations']}, layers {c.nb}")
    assert _same(ids, c.want)
    if case[0] <= LAYERS:
        assert st["enc_path"] == 1
        assert st["iterations"] == case[0]
    else:
        assert st["enc_path"] == 2


@gpu
@pytest.mark.parametrize("halo", [16, 48, 256])
def test_256_layers_across_window_edges(halo, monkeypatch):
    """the chain's 257-byte tokens cut by window edges: whatever path, the oracle's ids"""
    monkeypatch.setenv("BPE_EW_HALO", str(halo))
    c = chain_long_case()
    ids, st = _encode(c.text, c.merges)
    print(f"\nchain_tail-256, three windows, halo {halo}: enc_path {st['enc_path']}")
    assert _same(ids, c.want)
    assert st["n_out"] + st["occurrences"] == len(c.text)


@gpu
def test_layer_255_role_bit_at_a_window_edge(monkeypatch):
    """The one input here whose exactness hangs on mask word 7, bit 31: a
    255-layer chain and a last record (its id, `z`) in layer 255, where `z`
    is a right id in no other layer.  At halo 16 (core 2016) the `z` is the
    second window's first core byte.  The 16 chain bytes in that window's left
    halo are right ids of early layers, so the certain range starts at the `z`
    from batch 17 on -- and must move past it in batch 255, where its unknown
    left neighbour (the chain's id, complete in the first window) takes it:
    the window fails and the stream goes again.  Without that bit the second
    window emits a `z` that the first has already merged."""
    k = LAYERS - 1
    merges = np.vstack([EL.chain_list(k), np.array([[256 + k - 1, 122]], dtype=np.uint32)])
    assert EL.layers(merges) == (LAYERS, list(range(LAYERS)))
    whole = EL.expand(merges, 256 + k)
    assert len(whole) == 257 and whole.endswith(b"z") and whole.count(b"z") == 1
    core = 2048 - 2 * 16
    text = b"." * (core - 256) + whole + b"." * 200
    assert text[core] == 122
    want = O.encode(text, merges)
    assert want.tolist() == [46] * (core - 256) + [256 + k] + [46] * 200
    monkeypatch.setenv("BPE_EW_HALO", "16")
    ids, st = _encode(text, merges)
    assert _same(ids, want)
    assert st["enc_path"] == 3  # the first pass failed, the wide halo holds the whole token
    ids, off = api.encode_batch([text], merges)
    assert _same(ids, want) and off.tolist() == [0, want.size]


# ---- documents

def _cut(text, cuts):
    return [text[a:b] for a, b in zip(cuts, cuts[1:])]


def _doc_cuts(c, seed):
    """seeded cuts inside and between expansions, an empty document and a 1-byte document"""
    rng = random.Random(seed)
    n = len(c.text)
    inner = [s for s in c.starts if 0 < s < n]
    cuts = set(rng.sample(inner, 5)) | set(rng.sample(range(1, n), 5))
    p = rng.choice([x for x in range(1, n - 1) if x not in cuts and x + 1 not in cuts])
    cuts = sorted(cuts | {0, n, p, p + 1})  # the 1-byte document
    q = rng.randrange(1, len(cuts) - 1)
    cuts.insert(q, cuts[q])                 # the empty one
    docs = _cut(c.text, cuts)
    assert b"" in docs and any(len(d) == 1 for d in docs) and b"".join(docs) == c.text
    return docs


def _oracle_docs(docs, merges):
    parts = [O.encode(d, merges) for d in docs]
    return np.concatenate(parts).astype(np.uint32), np.cumsum([0] + [p.size for p in parts]).astype(np.uint64)


def _byte_offsets(docs):
    return np.cumsum([0] + [len(d) for d in docs]).astype(np.uint64)


def _check_docs(docs, merges):
    """encode_batch and the resident encode_docs against the oracle, document
    by document, and the way back through decode_docs; returns docs_info()"""
    oids, ooff = _oracle_docs(docs, merges)
    ids, off = api.encode_batch(docs, merges)
    assert off.tolist() == ooff.tolist()
    assert _same(ids, oids)
    e = api.Engine(0)
    try:
        e.load(b"".join(docs))
        e.encode_docs(_byte_offsets(docs), merges)
        assert e.doc_offsets().tolist() == ooff.tolist()
        assert _same(e.ids(), oids)
        info, st = e.docs_info(), e.stats()
        assert info["ndocs"] == len(docs) and st["n_out"] == oids.size
        raw, boff = e.decode_docs(oids, ooff, merges)
        assert raw == b"".join(docs) and boff.tolist() == _byte_offsets(docs).tolist()
    finally:
        e.close()
    return info


DOC_CASES = [_id(c) for c in AT_LIMIT] + ["chain_tail-256"]


def _doc_case(name):
    return chain_long_case() if name == "chain_tail-256" else count_case(*AT_LIMIT[DOC_CASES.index(name)])


@gpu
@pytest.mark.parametrize("name", DOC_CASES)
def test_documents_at_the_limits(name):
    c = _doc_case(name)
    for seed in (1, 2):
        docs = _doc_cuts(c, seed)
        info = _check_docs(docs, c.merges)
        print(f"\n{name} documents (seed {seed}): {info}")
        assert info["windows"] >= 3


@gpu
@pytest.mark.parametrize("name", DOC_CASES)
def test_split_after_filler_bytes(name):
    """encode_split under a custom rule: a piece starts after every filler byte"""
    c = _doc_case(name)
    filler = bytes(EL.TAIL_ALPHABET[:2]) if name == "chain_tail-256" else EL.FILLER
    cls, brk = np.zeros(256, np.uint8), np.zeros(16, np.uint16)
    cls[list(filler)] = 1
    brk[1] = 0xFFFF
    ids, id_off, byte_off = api.encode_split(c.text, c.merges, rule=(cls, brk))
    cuts = [0] + [i for i in range(1, len(c.text)) if c.text[i - 1] in filler] + [len(c.text)]
    assert byte_off.tolist() == cuts and len(cuts) > 100
    oids, ooff = _oracle_docs(_cut(c.text, cuts), c.merges)
    assert id_off.tolist() == ooff.tolist()
    assert _same(ids, oids)
    if c.m == M:
        assert oids.max() >= 65000
    else:
        assert (oids == 256 + LAYERS - 1).any()  # (the chain's bytes hold no filler)


@gpu
@pytest.mark.parametrize("name", ["two_layer-65280", "random-65280", "chain-257"])
def test_documents_beyond_the_limits_fall_back(name):
    """no plan: no window runs and every non-empty document goes through the fallback, exactly"""
    c = chain_case(LAYERS + 1, False) if name == "chain-257" else count_case(name.split("-")[0], M + 1)
    rng = random.Random(5)
    n = len(c.short)
    cuts = sorted(rng.sample(range(1, n), 5))
    cuts = [0] + cuts[:3] + cuts[2:] + [n]  # 7 documents, one of them empty
    docs = _cut(c.short, cuts)
    assert len(docs) <= 8 and b"" in docs
    info = _check_docs(docs, c.merges)
    print(f"\n{name} documents: {info}")
    assert info["windows"] == 0
    assert info["docs_fallback"] == sum(1 for d in docs if d)


# ---- shard group

@gpu
@pytest.mark.parametrize("k", [2, 5])
def test_shard_group_at_the_merge_limit(k, monkeypatch):
    """halo bytes from neighbouring shards, one shard shorter than the halo"""
    monkeypatch.setenv("BPE_EW_HALO", "64")
    c = count_case("random", M)
    rng = random.Random(40 + k)
    n = len(c.text)
    if k == 2:
        cuts = [0, rng.randint(1, 63), n]  # the short shard first
    else:
        first = rng.randrange(700, n - 700)
        cuts = {first, first + rng.randint(1, 63)}  # the short shard inside
        while len(cuts) < k - 1:
            cuts.add(rng.randrange(1, n))
        cuts = [0] + sorted(cuts) + [n]
    assert len(cuts) == k + 1 and min(b - a for a, b in zip(cuts, cuts[1:])) < 64
    g = api.ShardGroup(0, local_shards=k)
    try:
        g.load_split(c.text, cuts)
        g.encode(c.merges)
        ids = g.all_ids()
    finally:
        g.close()
    assert _same(ids, c.want), cuts


# ---- decode

@gpu
def test_decode_with_ids_at_and_beyond_16_bits():
    """the random lists are deeper than k_dec_elen's device passes (the host
    takes over), the two-layer lists finish on the device"""
    e = api.Engine(0)
    try:
        for c in all_cases():
            for text, want in ((c.text, c.want), (c.short, c.want_short)):
                got = e.decode(want, c.merges)
                assert got == text, (c.kind, c.m)
                assert got == O.decode(want, c.merges)
    finally:
        e.close()


# ---- the per-batch lookup list

# encode_win.hip EW_PENDCAP = 512: up to 512 entries the list is walked, beyond it every thread scans its rk
# words for the mark (k_enc_win and k_enc_docs each have their own copy of this).  In b"c" + b"abcc" * k every
# occurrence has a left neighbour and costs two entries, and each batch needs the ranks looked up after the
# one before.  EW_W = 2048 and the default halo 48: the two-window variants put a second copy at byte 2000,
# past the first window's right halo, so that each window sees one copy.
PEND_CHAIN = np.array([[97, 98], [256, 99], [257, 99]], dtype=np.uint32)
PEND_PAIRS = np.array([[97, 98], [256, 256], [257, 257]], dtype=np.uint32)
PEND = [(f"{2 * k}_entries", b"c" + b"abcc" * k, PEND_CHAIN) for k in (255, 256, 257, 300)]
PEND.append(("every_position", b"ab" * 900, PEND_PAIRS))
PEND += [(name + "_two_windows", t + b"." * (2000 - len(t)) + t, m) for name, t, m in list(PEND)]


@gpu
@pytest.mark.parametrize("name,text,merges", PEND, ids=[p[0] for p in PEND])
def test_pending_list_cap(name, text, merges):
    want = O.encode(text, merges)
    assert want.size < len(text) // 2 + 300  # (the merges do apply)
    ids, st = _encode(text, merges)
    assert _same(ids, want)
    assert st["enc_path"] == 1 and st["enc_windows"] == (2 if "two_windows" in name else 1)
    ids, off = api.encode_batch([text], merges)
    assert _same(ids, want) and off.tolist() == [0, want.size]
    rng = random.Random(len(text))
    for _ in range(3):
        docs = _cut(text, [0] + sorted(rng.sample(range(1, len(text)), 2)) + [len(text)])
        info = _check_docs(docs, merges)
        assert info["docs_fallback"] == 0

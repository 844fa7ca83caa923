"""Splitting the resident bytes on the device (split.hip, bpe_gpu_split & co.):
the offsets equal the rule's numpy restatement exactly, and encode_split over
them equals encode_docs / encode_batch / the oracle over the same pieces."""
import ctypes
import os
import random

import numpy as np
import pytest

import golden_lib as G
import oracle_lib as O
from llmtokenizer_amd import _lib, api
from llmtokenizer_amd.synth import english_like

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
# bpe_gpu.h BPE_GPU_SPLIT_TILE and BPE_GPU_SPLIT_TILE * BPE_GPU_SPLIT_GRID: bytes one workgroup handles per
# step and bytes one grid step covers (named here, not asked of the library while the tests are collected;
# test_geometry_matches_the_library holds them to it)
T, GB = 4096, 4096 * 2048
ESTATE = "call out of order"


def restate(data, cls, brk):
    b = np.frombuffer(data, np.uint8)
    c = np.asarray(cls)[b]
    st = np.ones(b.size, bool)
    st[1:] = (np.asarray(brk)[c[:-1]] >> c[1:]) & 1
    return np.append(np.flatnonzero(st), b.size).astype(np.uint64)


def cut(data, off):
    return [data[int(a):int(b)] for a, b in zip(off, off[1:])]


@pytest.fixture(scope="module")
def eng():
    e = api.Engine(0)
    yield e
    e.close()


def _random_rule(rng, k):
    hi = 16 if k % 2 == 0 else 3  # 0..2: long pieces
    cls = rng.integers(0, hi, 256).astype(np.uint8)
    brk = rng.integers(0, 1 << 16, 16).astype(np.uint16)
    if k % 4 == 1:
        brk &= rng.integers(0, 1 << 16, 16).astype(np.uint16)  # sparser
    return cls, brk


def test_geometry_matches_the_library():
    assert api.split_info() == {"tile": T, "grid_bytes": GB}


SIZES = [0, 1, 2, 15, 16, 17, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1, GB + T + 5]


@pytest.mark.parametrize("n", SIZES)
def test_offsets_equal_the_restatement(eng, n):
    rng = np.random.default_rng(1000 + n % 9973)
    data = rng.choice(np.frombuffer(b"ab c", np.uint8), n).tobytes()
    eng.load(data)
    for k in range(20):
        cls, brk = _random_rule(rng, k)
        want = restate(data, cls, brk)
        assert eng.split((cls, brk)) == want.size - 1
        got = eng.split_offsets()
        assert got.dtype == np.uint64 and got.size == want.size and (got == want).all(), (n, k)


def test_every_byte_a_piece_and_one_piece(eng):
    n = (1 << 20) + 3
    data = np.random.default_rng(5).choice(np.frombuffer(b"abcd", np.uint8), n).tobytes()
    eng.load(data)
    cls = np.arange(256, dtype=np.uint8) % 16
    assert eng.split((cls, np.full(16, 0xFFFF, np.uint16))) == n
    assert (eng.split_offsets() == np.arange(n + 1, dtype=np.uint64)).all()
    assert eng.split((cls, np.zeros(16, np.uint16))) == 1
    assert eng.split_offsets().tolist() == [0, n]


def test_predecessor_across_every_edge(eng):
    """all `a` but one `b` at p; class 1 is `b`, brk[0] = 0x2 only: the one interior start is p"""
    cls = np.zeros(256, np.uint8)
    cls[ord("b")] = 1
    brk = np.zeros(16, np.uint16)
    brk[0] = 0x2
    n = T + 64
    ps = sorted(set(range(T - 20, T + 21)) | {k * 16 + d for k in range(1, 9) for d in (-1, 0, 1)}
                | {k * 64 + d for k in range(1, 5) for d in (-1, 0, 1)} | {1, n - 1})
    for p in ps:
        buf = bytearray(b"a" * n)
        buf[p] = ord("b")
        eng.load(bytes(buf))
        assert eng.split((cls, brk)) == 2, p
        assert eng.split_offsets().tolist() == [0, p, n], p


def test_bad_class_is_rejected(eng):
    eng.load(b"abc")
    cls, brk = api.split_rule("words")
    cls[200] = 16
    with pytest.raises(api.BpeError, match="invalid argument"):
        eng.split((cls, brk))
    with pytest.raises(api.BpeError):
        eng.split((np.zeros(255, np.uint8), brk))


def test_lines_preset_on_the_golden_text(eng):
    with open(os.path.join(HERE, "golden", "random_text.txt"), "rb") as f:
        data = f.read()
    assert b"\r" not in data  # (bytes.splitlines would cut there too)
    lines = data.splitlines(keepends=True)
    eng.load(data)
    want = np.cumsum([0] + [len(x) for x in lines]).astype(np.uint64)
    assert eng.split("lines") == len(lines)
    assert (eng.split_offsets() == want).all()
    # and a text that does have newlines
    text = english_like(1 << 16)
    assert text.count(b"\n") > 100
    lines = text.splitlines(keepends=True)
    eng.load(text)
    assert eng.split("lines") == len(lines)
    assert eng.split_offsets().tolist() == np.cumsum([0] + [len(x) for x in lines]).tolist()


def test_words_preset_on_english_like(eng):
    data = english_like(1 << 16)
    cls, brk = api.split_rule("words")
    want = restate(data, cls, brk)
    eng.load(data)
    assert eng.split("words") == want.size - 1
    assert (eng.split_offsets() == want).all()
    assert 3.0 < len(data) / (want.size - 1) < 6.0  # about 4.3 bytes per piece


# ---------------------------------------------------------------- encode over the resident offsets

def _random_merges(rng, alphabet, k, eq=0.3):
    """as tests/test_gpu_encode_docs.py builds them (a == a records included)"""
    ids = list(alphabet)
    out = []
    for r in range(k):
        u, v = rng.choice(ids), rng.choice(ids)
        if rng.random() < eq:
            v = u
        out.append((u, v))
        ids.append(256 + r)
    return np.array(out, dtype=np.uint32).reshape(-1, 2)


def _oracle(docs, merges):
    parts = [O.encode(d, merges) for d in docs]
    ids = np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint32)
    return ids.astype(np.uint32), np.cumsum([0] + [p.size for p in parts]).astype(np.uint64)


def _plain(st):
    return {k: v for k, v in st.items() if not k.startswith("ms_")}


def _check_split_encode(data, rule, merges, oracle=False, what=None):
    """split + encode_split on one context against encode_batch of the restatement's pieces,
    encode_docs with the fetched offsets on another, and (small texts) the oracle per piece"""
    cls, brk = api.split_rule(rule) if isinstance(rule, str) else rule
    want_off = restate(data, cls, brk)
    docs = cut(data, want_off)
    e, d = api.Engine(0), api.Engine(0)
    try:
        e.load(data)
        assert e.split(rule) == len(docs), what
        e.encode_split(merges)
        off = e.split_offsets()
        assert (off == want_off).all(), what
        ids, id_off = e.ids(), e.doc_offsets()
        bids, boff = api.encode_batch(docs, merges)
        assert id_off.tolist() == boff.tolist(), what
        assert ids.size == bids.size and (ids == bids).all(), what
        if oracle:
            oids, ooff = _oracle(docs, merges)
            assert id_off.tolist() == ooff.tolist() and (ids == oids).all(), what
        d.load(data)
        d.encode_docs(off, merges)
        assert e.ids_checksum() == d.ids_checksum() == G.ids_checksum(ids), what
        assert e.ids_checksum(base=7) == d.ids_checksum(base=7), what
        info = e.docs_info()
        assert info == d.docs_info(), what
        assert _plain(e.stats()) == _plain(d.stats()), what
        return info
    finally:
        e.close()
        d.close()


@pytest.fixture(scope="module")
def english():
    data = english_like(200000)
    merges, _ = api.train_bytes(data[: 1 << 16], 300)
    return data, merges


@pytest.mark.parametrize("halo", [16, 48, 256])
@pytest.mark.parametrize("rule", ["lines", "words"])
def test_encode_split_english(english, rule, halo, monkeypatch):
    monkeypatch.setenv("BPE_EW_HALO", str(halo))
    data, merges = english
    info = _check_split_encode(data, rule, merges, what=(rule, halo))
    assert info["halo"] == halo and info["core"] == 2048 - 2 * halo


@pytest.mark.parametrize("halo", [16, 48, 256])
@pytest.mark.parametrize("rule", ["lines", "words"])
def test_encode_split_random_texts(rule, halo, monkeypatch):
    monkeypatch.setenv("BPE_EW_HALO", str(halo))
    rng = random.Random(700 + halo + len(rule))
    for alpha in (b"ab", b"abc"):
        # the presets see something to split at: spaces, digits and newlines among the letters
        body = alpha * 6 + b"  \n1"
        text = bytes(rng.choice(body) for _ in range(rng.randint(6000, 9000)))
        merges = _random_merges(rng, sorted(set(body)), rng.randint(50, 400), eq=rng.choice([0.0, 0.3]))
        _check_split_encode(text, rule, merges, oracle=True, what=(rule, halo, alpha))


def test_piece_starts_at_window_and_halo_edges(monkeypatch):
    """piece starts at -2..+2 of the first three core edges and of their halo edges (halo 48: core 1,952)"""
    halo, core = 48, 1952
    monkeypatch.setenv("BPE_EW_HALO", str(halo))
    rng = random.Random(12)
    n = 4 * core + 100
    cls = np.zeros(256, np.uint8)
    cls[ord("c")] = 1
    brk = np.zeros(16, np.uint16)
    brk[0] = brk[1] = 0x2  # a piece starts at every `c`
    for centre in (0, -halo, halo):
        buf = bytearray(rng.choice(b"ab") for _ in range(n))
        starts = sorted({k * core + centre + d for k in (1, 2, 3) for d in (-2, -1, 0, 1, 2)})
        for p in starts:
            buf[p] = ord("c")
        data = bytes(buf)
        assert restate(data, cls, brk).tolist() == [0] + starts + [n]
        merges = _random_merges(rng, sorted(set(b"abc")), 300, eq=0.3)
        info = _check_split_encode(data, (cls, brk), merges, oracle=True, what=centre)
        assert info["core"] == core and info["windows"] == (n + core - 1) // core


def test_two_merge_lists_over_one_split_and_state():
    rng = random.Random(44)
    text = bytes(rng.choice(b"ab ab\n") for _ in range(5000))
    m1 = _random_merges(rng, sorted(set(b"ab \n")), 120, eq=0.3)
    m2 = _random_merges(rng, sorted(set(b"ab \n")), 77, eq=0.0)
    cls, brk = api.split_rule("words")
    docs = cut(text, restate(text, cls, brk))
    e = api.Engine(0)
    try:
        with pytest.raises(api.BpeError, match=ESTATE):
            e.split("words")  # nothing loaded
        e.load(text)
        with pytest.raises(api.BpeError, match=ESTATE):
            e.encode_split(m1)
        with pytest.raises(api.BpeError, match=ESTATE):
            e.split_offsets()
        assert e.split("words") == len(docs)
        for m in (m1, m2, m1):
            e.encode_split(m)
            oids, ooff = _oracle(docs, m)
            assert (e.ids() == oids).all() and e.doc_offsets().tolist() == ooff.tolist()
        # the single-stream and the document encoder keep the split; a new load drops it
        e.encode(m2)
        e.encode_docs([0, 10, len(text)], m2)
        e.encode_split(m2)
        assert (e.ids() == _oracle(docs, m2)[0]).all()
        e.load(text)
        with pytest.raises(api.BpeError, match=ESTATE):
            e.encode_split(m1)
        with pytest.raises(api.BpeError, match=ESTATE):
            e.split_offsets()
        # training drops it too; the context stays usable
        assert e.split("lines") == len(text.splitlines())
        e.train(10)
        with pytest.raises(api.BpeError, match=ESTATE):
            e.encode_split(m1)
        e.load(b"")
        assert e.split("words") == 0 and e.split_offsets().tolist() == [0]
        e.encode_split(m1)
        assert e.ids().size == 0 and e.doc_offsets().tolist() == [0]
    finally:
        e.close()


def test_no_plan_fallback():
    """a 300-deep chain has more layers than the window encoder's batch masks hold (test_gpu_encode_docs.py)"""
    chain = [(97, 97)] + [(256 + r, 256 + r) for r in range(299)]
    merges = np.array(chain, dtype=np.uint32)
    rng = random.Random(3)
    text = b"".join(b"a" * rng.randint(1, 40) + rng.choice([b" ", b"\n", b" b"]) for _ in range(30))[:300]
    assert len(text) == 300
    for rule in ("lines", "words"):
        info = _check_split_encode(text, rule, merges, oracle=True, what=rule)
        assert info["docs_fallback"] == info["ndocs"] and info["windows"] == 0


def test_partial_fallback(monkeypatch):
    """test_gpu_encode_docs.py's failed windows (a run of 20001 `a` under (97, 97) inside one long
    piece) with the pieces cut by the lines rule: only some pieces go through the fallback"""
    rng = random.Random(21)
    halo = 48
    monkeypatch.setenv("BPE_EW_HALO", str(halo))
    merges = np.vstack([np.array([[97, 97]], dtype=np.uint32), _random_merges(rng, sorted(set(b"ab ")), 200, eq=0.3)])
    short = [bytes(rng.choice(b"ab ") for _ in range(rng.randint(0, halo - 1))) + b"\n" for _ in range(100)]
    text = b"".join(short[:70] + [b"." * 2100 + b"a" * 20001 + b" b" * 20 + b"\n"] + short[70:])
    info = _check_split_encode(text, "lines", merges, oracle=True)
    assert info["ndocs"] == 101 and info["windows_failed"] >= 1
    assert 1 <= info["docs_fallback"] < 50


def test_c_layer():
    rng = random.Random(51)
    text = bytes(rng.choice(b"ab ab\n7") for _ in range(3000))
    merges = _random_merges(rng, sorted(set(b"ab \n7")), 100, eq=0.3)
    cls, brk = api.split_rule("words")
    want_boff = restate(text, cls, brk)
    want_ids, want_off = api.encode_batch(cut(text, want_boff), merges)
    ids, id_off, byte_off = api.encode_split(text, merges)  # (passes byte_off)
    assert (ids == want_ids).all() and id_off.tolist() == want_off.tolist() and byte_off.tolist() == want_boff.tolist()
    ids, id_off, byte_off = api.encode_split(text, merges, rule=(cls, brk))
    assert (ids == want_ids).all() and byte_off.tolist() == want_boff.tolist()
    # without byte_off, through ctypes
    L = _lib.load()
    free = ctypes.CDLL(None).free
    free.argtypes = [ctypes.c_void_p]
    buf = np.frombuffer(text, dtype=np.uint8)
    arr = api._merges_to_arr(merges)
    n, nd = ctypes.c_size_t(0), ctypes.c_size_t(0)
    ido = ctypes.POINTER(ctypes.c_uint64)()
    vp = ctypes.c_void_p
    p = L.bpe_encode_split(buf.ctypes.data_as(vp), buf.size, cls.ctypes.data_as(vp), brk.ctypes.data_as(vp), arr, 0,
                           ctypes.byref(n), ctypes.byref(ido), None, ctypes.byref(nd))
    L.dyn_arr_free(arr)
    assert p and ido and nd.value == want_boff.size - 1
    got = np.ctypeslib.as_array(p, shape=(max(n.value, 1),))[: n.value].copy()
    got_off = np.ctypeslib.as_array(ido, shape=(nd.value + 1,)).copy()
    free(ctypes.cast(p, vp))
    free(ctypes.cast(ido, vp))
    assert (got == want_ids).all() and got_off.tolist() == want_off.tolist()
    assert api.last_stats()["n_out"] == got.size

"""Document batches (encode_docs.hip, bpe_gpu_encode_docs & co.): the ids of a
batch are the oracle's ids of every document on its own, concatenated, with
the cumulative lengths as offsets -- bit-exact, for any merge list."""
import ctypes
import random

import numpy as np
import pytest

import golden_lib as G
import oracle_lib as O
from llmtokenizer_amd import _lib, api

pytestmark = pytest.mark.gpu

ALPHABETS = [b"ab", b"abc", b"a", b"aab", b"abcdefgh"]


def _random_merges(rng, alphabet, k, eq=0.3):
    ids = list(alphabet)
    out = []
    for r in range(k):
        u, v = rng.choice(ids), rng.choice(ids)
        if rng.random() < eq:
            v = u
        out.append((u, v))
        ids.append(256 + r)
    return np.array(out, dtype=np.uint32).reshape(-1, 2)


def _skipped_records(rng, merges):
    """records the plan skips: a forward reference and a pair that repeats an earlier record"""
    m = merges.copy()
    q = rng.randrange(1, len(m))
    m[q] = [256 + len(m) - 1, m[0][1]]
    return np.vstack([m, m[:1]])


def _merge_list(rng, alpha):
    merges = _random_merges(rng, sorted(set(alpha)), rng.randint(1, 600), eq=rng.choice([0.0, 0.3]))
    if rng.random() < 0.3 and len(merges) > 2:
        merges = _skipped_records(rng, merges)
    return merges


def _oracle(docs, merges):
    parts = [O.encode(d, merges) for d in docs]
    ids = np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint32)
    return ids.astype(np.uint32), np.cumsum([0] + [p.size for p in parts]).astype(np.uint64)


def _offsets(docs):
    return np.cumsum([0] + [len(d) for d in docs]).astype(np.uint64)


def _engine_docs(docs, merges):
    """(ids, id offsets, docs_info, stats) through the resident path"""
    e = api.Engine(0)
    try:
        e.load(b"".join(docs))
        e.encode_docs(_offsets(docs), merges)
        return e.ids(), e.doc_offsets(), e.docs_info(), e.stats()
    finally:
        e.close()


def _check(docs, merges, what=None):
    ids, off, info, st = _engine_docs(docs, merges)
    oids, ooff = _oracle(docs, merges)
    assert off.tolist() == ooff.tolist(), what
    assert ids.size == oids.size and (ids == oids).all(), what
    assert info["ndocs"] == len(docs)
    assert st["n_in"] == sum(len(d) for d in docs) and st["n_out"] == ids.size
    return info


def _text(rng, alpha, n):
    return bytes(rng.choice(alpha) for _ in range(n))


def test_boundary_matters():
    merges = np.array([[97, 98], [256, 256]], dtype=np.uint32)
    ids, off = api.encode_batch([b"ab", b"ab"], merges)
    assert ids.tolist() == [256, 256] and off.tolist() == [0, 1, 2]
    assert off.dtype == np.uint64
    # what concatenating the documents gets wrong
    assert api.encode(b"abab", merges).tolist() == [257]


def test_forward_reference_and_repeated_pair():
    rng = random.Random(77)
    merges = _skipped_records(rng, _random_merges(rng, sorted(set(b"abc")), 200, eq=0.3))
    docs = [_text(rng, b"abc", rng.choice([0, 1, 2, 17, 300, 2500])) for _ in range(60)]
    ids, off = api.encode_batch(docs, merges)
    oids, ooff = _oracle(docs, merges)
    assert off.tolist() == ooff.tolist() and (ids == oids).all()


@pytest.mark.parametrize("name", ["zero_docs", "one_empty", "all_empty", "one_doc", "one_byte_docs", "two_byte_docs",
                                  "empties_around"])
def test_degenerate_shapes(name):
    rng = random.Random(11)
    merges = _random_merges(rng, sorted(set(b"ab")), 120, eq=0.3)
    text = _text(rng, b"ab", 5000)
    docs = {
        "zero_docs": [],
        "one_empty": [b""],
        "all_empty": [b""] * 37,
        "one_doc": [text],
        "one_byte_docs": [text[i:i + 1] for i in range(4500)],  # (more than two windows of document starts)
        "two_byte_docs": [text[i:i + 2] for i in range(0, 5000, 2)],
        "empties_around": [b"", b"", text[:700], b"", b"", b"", text[700:703], b"", text[703:], b"", b""],
    }[name]
    ids, off = api.encode_batch(docs, merges)
    oids, ooff = _oracle(docs, merges)
    assert off.tolist() == ooff.tolist() and off.size == len(docs) + 1
    assert ids.size == oids.size and (ids == oids).all()
    if name == "one_doc":
        assert (ids == api.encode(text, merges)).all()
    if name == "one_byte_docs":
        assert ids.tolist() == list(text[:4500])
    if name in ("zero_docs", "one_empty", "all_empty"):
        assert ids.size == 0 and not off.any()
    _check(docs, merges, name)  # the resident path too


DOC_LENGTHS = [lambda r: 0, lambda r: 1, lambda r: 2, lambda r: r.randint(3, 40), lambda r: r.randint(200, 900),
               lambda r: r.randint(2500, 7000)]


def _random_docs(rng, alpha, total):
    docs, n = [], 0
    while n < total and len(docs) < 400:
        k = rng.choices(DOC_LENGTHS, weights=[2, 2, 2, 6, 3, 1])[0](rng)
        docs.append(_text(rng, alpha, k))
        n += k
    return docs


@pytest.mark.parametrize("halo", [16, 48, 256])
def test_random_batches_any_halo(halo, monkeypatch):
    monkeypatch.setenv("BPE_EW_HALO", str(halo))
    rng = random.Random(300 + halo)
    for case in range(5):
        alpha = ALPHABETS[case % len(ALPHABETS)]
        docs = _random_docs(rng, alpha, rng.randint(8000, 40000))
        info = _check(docs, _merge_list(rng, alpha), (halo, case))
        assert info["halo"] == halo and info["core"] == 2048 - 2 * halo


def test_boundaries_at_window_edges():
    """document starts at k * core + {-1, 0, 1} and k * core +- halo + {-1, 0, 1}, every k"""
    rng = random.Random(5)
    n = 30000
    info = _engine_docs([b"ab"], np.array([[97, 98]], dtype=np.uint32))[2]
    core, halo = info["core"], info["halo"]
    assert core + 2 * halo == 2048
    for alpha, eq in ((b"ab", 0.3), (b"abc", 0.0)):
        text = _text(rng, alpha, n)
        merges = _random_merges(rng, sorted(set(alpha)), 400, eq=eq)
        for centre in (0, -halo, halo):
            cuts = {0, n}
            for k in range(n // core + 2):
                for d in (-1, 0, 1):
                    x = k * core + centre + d
                    if 0 < x < n:
                        cuts.add(x)
            cuts = sorted(cuts)
            docs = [text[a:b] for a, b in zip(cuts, cuts[1:])]
            got = _check(docs, merges, (alpha, centre))
            assert got["windows"] == (n + core - 1) // core


def test_runs_across_boundaries():
    merges = np.array([[97, 97], [256, 256]], dtype=np.uint32)
    docs = []
    for m in range(1, 10):  # b"a" * m split at every position
        for cut in range(m + 1):
            docs += [b"a" * cut, b"a" * (m - cut)]
    info = _check(docs, merges, "short runs")
    assert info["docs_fallback"] == 0
    # long runs cut at seeded points, mixed into ab text
    rng = random.Random(9)
    merges = np.vstack([merges, _random_merges(rng, sorted(set(b"ab")), 150, eq=0.3)])
    docs = []
    for _ in range(12):
        run = b"a" * rng.randint(50, 3000)
        cuts = sorted({0, len(run)} | {rng.randrange(len(run)) for _ in range(rng.randint(1, 6))})
        docs += [run[a:b] for a, b in zip(cuts, cuts[1:])]
        docs[-1] += _text(rng, b"ab", rng.randint(0, 300))
        docs.append(_text(rng, b"ab", rng.randint(1, 500)) + b"a" * rng.randint(0, 40))
    _check(docs, merges, "long runs")


def test_fallback_of_some_documents_only():
    """A run of 20001 `a` under (97, 97): the windows inside it cannot know the
    run's parity and the window holding its end never can, so they fail, and
    with them every document that has a byte in one of their cores.

    Which documents those can be follows from the geometry.  The short
    documents are no longer than the halo, so a window among them is clipped at
    document starts on both sides: no unknown neighbour, it cannot fail.  The
    long document opens with more than a window of `.`, a byte no merge uses:
    an edge token `.` has no role in any batch, so the window shared by the 70
    documents before it and its first bytes stays certain too.  The 30
    documents after it (at most 30 * halo bytes, less than a core) share the
    window of the run's end or the one after it: the fallback takes the long
    document and at most those 30, spliced between first-pass neighbours."""
    rng = random.Random(21)
    halo = _engine_docs([b"ab"], np.array([[97, 98]], dtype=np.uint32))[2]["halo"]
    merges = np.vstack([np.array([[97, 97]], dtype=np.uint32), _random_merges(rng, sorted(set(b"ab ")), 200, eq=0.3)])
    short = [_text(rng, b"ab ", rng.randint(0, halo)) for _ in range(100)]
    docs = short[:70] + [b"." * 2100 + b"a" * 20001 + b" b" * 20] + short[70:]
    info = _check(docs, merges)
    assert info["windows_failed"] >= 1
    assert 1 <= info["docs_fallback"] < len(docs) // 2
    info = _check(short, merges)
    assert info["docs_fallback"] == 0 and info["windows_failed"] == 0


def test_no_plan_every_document_through_the_fallback():
    """a 300-deep chain has more layers than the window encoder's batch masks hold"""
    chain = [(97, 97)] + [(256 + r, 256 + r) for r in range(299)]
    merges = np.array(chain, dtype=np.uint32)
    rng = random.Random(3)
    docs = [b"a" * rng.randint(1, 700) + _text(rng, b"ab", rng.randint(0, 20)) for _ in range(20)]
    info = _check(docs, merges)
    assert info["docs_fallback"] == len(docs) and info["windows"] == 0


def test_resident_path():
    rng = random.Random(31)
    docs = _random_docs(rng, b"abc", 30000)
    merges = _random_merges(rng, sorted(set(b"abc")), 300, eq=0.3)
    oids, ooff = _oracle(docs, merges)
    e = api.Engine(0)
    e.load(b"".join(docs))
    e.encode_docs(_offsets(docs), merges)
    assert e.ids_checksum() == G.ids_checksum(oids)
    assert e.ids_checksum(base=99) == G.ids_checksum(oids, base=99)
    ids, off = api.encode_batch(docs, merges)
    assert (e.ids() == ids).all() and e.doc_offsets().tolist() == off.tolist() == ooff.tolist()
    # the single-stream encoder on the same context afterwards: the document offsets are gone
    e.encode(merges)
    assert (e.ids() == O.encode(b"".join(docs), merges)).all()
    with pytest.raises(api.BpeError):
        e.doc_offsets()
    e.close()


def test_bad_offsets():
    merges = np.array([[97, 98]], dtype=np.uint32)
    e = api.Engine(0)
    e.load(b"abababab")
    for bad in ([1, 8], [0, 7], [0, 9], [0, 5, 4, 8]):
        with pytest.raises(api.BpeError):
            e.encode_docs(bad, merges)
    e.encode_docs([0, 3, 8], merges)  # the context is still usable
    assert e.ids().tolist() == [256, 97, 98, 256, 256] and e.doc_offsets().tolist() == [0, 2, 5]
    e.close()
    e = api.Engine(0)
    e.load(b"")
    with pytest.raises(api.BpeError):
        e.encode_docs([0, 1], merges)
    e.close()


def test_round_trip():
    rng = random.Random(41)
    merges = _random_merges(rng, sorted(set(b"abc\0")), 250, eq=0.2)
    plain = [_text(rng, b"abc", rng.choice([0, 1, 5, 90, 3000])) for _ in range(40)]
    with_nul = [_text(rng, b"abc\0", rng.choice([0, 1, 5, 90, 3000])) for _ in range(40)]
    for docs in (plain, with_nul):
        ids, off = api.encode_batch(docs, merges)
        assert api.decode_batch(ids, off, merges) == [d.replace(b"\0", b"") for d in docs]
        # the C-ABI call's byte offsets against the oracle's decoder, document by document
        e = api.Engine(0)
        raw, boff = e.decode_docs(ids, off, merges)
        e.close()
        want = [O.decode(ids[int(off[d]):int(off[d + 1])], merges) for d in range(len(docs))]
        assert boff.tolist() == np.cumsum([0] + [len(x) for x in want]).tolist()
        assert raw == b"".join(want)
    with pytest.raises(api.BpeError):
        api.decode_batch(np.array([97, 256 + len(merges)], dtype=np.uint32), [0, 1, 2], merges)


def test_c_layer_matches_api():
    rng = random.Random(51)
    docs = [_text(rng, b"ab", rng.choice([0, 1, 2, 33, 700])) for _ in range(30)]
    merges = _random_merges(rng, sorted(set(b"ab")), 100, eq=0.3)
    want_ids, want_off = api.encode_batch(docs, merges)
    L = _lib.load()
    free = ctypes.CDLL(None).free
    free.argtypes = [ctypes.c_void_p]
    buf = np.frombuffer(b"".join(docs), dtype=np.uint8)
    off = _offsets(docs)
    arr = api._merges_to_arr(merges)
    n = ctypes.c_size_t(0)
    ido = ctypes.POINTER(ctypes.c_uint64)()
    p = L.bpe_encode_docs(buf.ctypes.data_as(ctypes.c_void_p), buf.size, off.ctypes.data_as(ctypes.c_void_p), len(docs),
                          arr, 0, ctypes.byref(n), ctypes.byref(ido))
    assert p and ido
    ids = np.ctypeslib.as_array(p, shape=(max(n.value, 1),))[: n.value].copy()
    id_off = np.ctypeslib.as_array(ido, shape=(len(docs) + 1,)).copy()
    free(ctypes.cast(p, ctypes.c_void_p))
    free(ctypes.cast(ido, ctypes.c_void_p))
    assert (ids == want_ids).all() and id_off.tolist() == want_off.tolist()
    assert api.last_stats()["n_out"] == ids.size
    m = ctypes.c_size_t(0)
    bo = ctypes.POINTER(ctypes.c_uint64)()
    q = L.bpe_decode_docs(ids.ctypes.data_as(ctypes.c_void_p), ids.size, id_off.ctypes.data_as(ctypes.c_void_p),
                          len(docs), arr, 0, ctypes.byref(m), ctypes.byref(bo))
    L.dyn_arr_free(arr)
    assert q and bo
    raw = ctypes.string_at(q, m.value)
    boff = [int(bo[d]) for d in range(len(docs) + 1)]
    free(q)
    free(ctypes.cast(bo, ctypes.c_void_p))
    assert [raw[boff[d]:boff[d + 1]] for d in range(len(docs))] == api.decode_batch(want_ids, want_off, merges) == docs

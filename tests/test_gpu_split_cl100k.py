"""BPE_SPLIT_CL100K on the device (split.hip k_cl_summary, the scan of the chain effects, k_split_mark_cl100k;
special.hip's cover bitmap read while marking): the offsets equal api.split_host(data, "cl100k"), bit for bit,
which tests/test_split_cl100k_host.py pins to the regular expression.  The cases put the three unbounded chains
(the index in a run of numbers, a run of newlines after punctuation, white space before a later newline) and
the window across every edge of the geometry: 16 bytes a thread, 1,024 a wave, a tile a workgroup, a grid step."""
import numpy as np
import pytest

import golden_lib as G
import train_split_ref as R
from llmtokenizer_amd import api

pytestmark = pytest.mark.gpu

RULE = "cl100k"
# bytes one workgroup handles per step and bytes one grid step covers (test_the_geometry_is_the_library_s)
T, GB = 4096, 4096 * 2048
ESTATE = "call out of order"
EOT = b"<|endoftext|>"
SPECIALS = [EOT, b"\xac|x|"]
ITEMS = [b"'", b"s", b"T", b"re", b"LL", b"v", b"a", b"Z", b"1", b"23", b"4567", b"!", b"\n", b"\n\n", b"\r\n", b" ", b" ", b"  ",
         b"\t", b"word", b" the", b"!\n", b" \n", b"\n  "]
ITEMS += [s.encode() for s in ("ſ", "é", "Ж", "中", "\U00010400", "٣", "²", "½", "\U0001d7d8", " ", "　", "\u0085",
                               "—", "€", "\U0001f600")]
ITEMS += [b"\x80", b"\xc3", b"\xe2\x82", b"\xf0\x9f\x98", b"\xc0\x80", b"\xff"]


def mixed(n, seed):
    """n bytes of the items above in random order (cut at n: the text may end inside a sequence)"""
    rng = np.random.default_rng(seed)
    out, size = [], 0
    while size < n:
        for k in rng.integers(0, len(ITEMS), 4096).tolist():
            out.append(ITEMS[k])
            size += len(ITEMS[k])
    return b"".join(out)[:n]


def cut(data, off):
    return [data[int(a):int(b)] for a, b in zip(off, off[1:])]


@pytest.fixture(scope="module")
def eng():
    e = api.Engine(0)
    yield e
    e.close()


def _split(eng, data, specials=None, rule=RULE):
    eng.load(data)
    nd = eng.split(rule, specials)
    off = eng.split_offsets()
    assert off.dtype == np.uint64 and off.size == nd + 1
    return off


def _same(eng, data, what=None):
    got, want = _split(eng, data), api.split_host(data, RULE)
    assert got.size == want.size and (got == want).all(), what if what is not None else len(data)


def _edges(lo, hi):
    """lo..hi around every 16-byte edge up to 128, 1,024 and the tile"""
    centres = [16 * k for k in range(1, 9)] + [1024, T]
    return sorted({c + d for c in centres for d in range(lo, hi + 1)})


def _probe_at_the_edges(eng, probes, fill, lo, hi):
    n = T + 96
    for name, probe in probes:
        for p in _edges(lo, hi):
            buf = bytearray(fill * n)
            buf[p:p + len(probe)] = probe
            _same(eng, bytes(buf[:n]), (name, p))


def test_the_geometry_is_the_library_s():
    assert api.split_info() == {"tile": T, "grid_bytes": GB}


@pytest.mark.parametrize("n", [0, 1, 15, 16, 17, 1023, 1024, 1025, T - 1, T, T + 1])
def test_offsets_equal_the_host_definition(eng, n):
    for seed in range(4):
        _same(eng, mixed(n, 100 * n + seed), (n, seed))


def test_the_grid_stride(eng):
    big = mixed(GB + 1, 7)
    for n in (GB - 1, GB + 1):
        _same(eng, big[:n], n)


@pytest.mark.parametrize("digits", ["ascii", "mixed"])
def test_runs_of_numbers_across_every_edge(eng, digits):
    """runs of 1..7 numbers from -4..+4 of every edge; mixed: two-byte numbers, so the index in the run is not the
    byte index and a character straddles the edge"""
    pool = [b"1"] if digits == "ascii" else ["٣".encode(), b"7", "½".encode()]
    probes = [(k, b"".join(pool[(j + k) % len(pool)] for j in range(k))) for k in range(1, 8)]
    _probe_at_the_edges(eng, probes, b"a", -4, 4)


@pytest.mark.parametrize("r", [0, 1, 2])
def test_one_run_of_numbers_longer_than_a_grid_step(eng, r):
    """the run crosses every kind of edge at each residue of its length and of its first byte"""
    run = b"0123456789" * ((GB + 3 * 1024 + r) // 10 + 1)
    for head in (b"", b"a", b"a "):
        _same(eng, head + run[:GB + 3 * 1024 + r] + b"x", (r, head))


def test_newlines_after_punctuation_across_every_edge(eng):
    """chain A: ! and a run of 1..5 newlines, then spaces, with and without a later newline in the run"""
    probes = [((k, tail), b"!" + b"\n" * k + tail) for k in range(1, 6) for tail in (b"  x", b"  \nx", b" \r\n ")]
    _probe_at_the_edges(eng, probes, b"a", -4, 4)


@pytest.mark.parametrize("length", [T + 5, GB + 5])
def test_a_long_run_of_newlines(eng, length):
    for head in (b"!", b"a"):
        for tail in (b"  \nx", b"  x"):
            _same(eng, head + b"\n" * length + tail, (length, head, tail))


def test_spaces_between_newlines_across_every_edge(eng):
    """chain B: a newline, k spaces and a newline or none: the first space starts a piece only when none follows"""
    probes = [((k, tail), b"\n" + b" " * k + tail) for k in range(5) for tail in (b"\n x", b" x", "　\nx".encode())]
    _probe_at_the_edges(eng, probes, b"a", -4, 4)


@pytest.mark.parametrize("length", [T + 5, GB + 5])
def test_a_long_run_of_spaces(eng, length):
    for head in (b"x\n", b"!\n"):
        for tail in (b"\n x", b"x", b""):  # the final newline present, absent, and the run up to the end of the text
            _same(eng, head + b" " * length + tail, (length, head, tail))


def test_contractions_across_every_edge(eng):
    probes = [(s, s.encode()) for s in ("'S", "'Re", "'ll", "'ſ", "1'T", " 've", "!'d")]
    _probe_at_the_edges(eng, probes, b"a", -8, 8)
    _probe_at_the_edges(eng, probes[:4], b" ", -8, 8)


def test_the_text_ends_inside_a_contraction(eng):
    """the slack past n holds the letters that would complete it: a longer text of them was resident just before"""
    for n in _edges(-8, 8):
        for tail, slack in ((b"'l", b"l"), (b"'\xc5", b"\xbf"), (b"'r", b"e"), (b"'", b"s")):
            eng.load(slack * (n + 64))
            _same(eng, b"a" * (n - len(tail)) + tail, (n, tail))


@pytest.mark.parametrize("at", [5, 1023, 1030, 2 * T + 100])
def test_one_character_in_one_wave(eng, at):
    """the only byte >= 0x80 sits in one wave's windows: that wave decodes, the others of the launch do not"""
    buf = bytearray((b"it's a word, isn't it?  12345 DON'T\n\n  go \n \n" * 400)[:3 * T + 9])
    ascii_off = _split(eng, bytes(buf))
    assert (ascii_off == api.split_host(bytes(buf), RULE)).all()
    buf[at:at + 3] = "　".encode()
    _same(eng, bytes(buf), at)


@pytest.fixture(scope="module")
def text():
    """20 kB of prose with non-ASCII words, numbers, white space and punctuation, the host's offsets and pieces"""
    fx = G.load("prose")
    words = G.input_bytes(fx).split(b" ")
    extra = [s.encode() for s in (" café", " naïve", " Привет", " 中文", " ٣٤٥٦", " 7½", " 1234567", "　", " x", " —", "…",
                                  " don't", " IT'LL", " l'été", "\n\n", "!\n\n  ", " \n \n", " \U0001f600", "é's")]
    rng = np.random.default_rng(4)
    out, size = [], 0
    while size < 20000:
        w = (b" " + words[int(rng.integers(len(words)))]) if rng.random() < 0.6 else extra[int(rng.integers(len(extra)))]
        out.append(w)
        size += len(w)
    data = b"".join(out)[:20000]
    off = api.split_host(data, RULE)
    return data, off, cut(data, off), np.asarray(fx["merges"], dtype=np.uint32).reshape(-1, 2)


def test_encode_split_equals_encode_batch_over_the_host_pieces(eng, text):
    data, off, pieces, merges = text
    want_ids, want_off = api.encode_batch(pieces, merges)
    eng.load(data)
    assert eng.split(RULE) == len(pieces)
    assert (eng.split_offsets() == off).all()
    eng.encode_split(merges)
    ids, id_off = eng.ids(), eng.doc_offsets()
    assert id_off.tolist() == want_off.tolist()
    assert ids.size == want_ids.size and (ids == want_ids).all()
    ids, id_off, byte_off = api.encode_split(data, merges, rule=RULE)
    assert (ids == want_ids).all() and id_off.tolist() == want_off.tolist() and byte_off.tolist() == off.tolist()


def test_train_split_equals_the_restatement_over_the_host_pieces(eng, text):
    data, off, pieces, _ = text
    want, stop, _ = R.train(pieces, 200)
    assert len(want) == 200
    got = api.train_split(data, rule=RULE, max_merges=200)
    assert got.dtype == np.uint32 and [tuple(m) for m in got.tolist()] == want
    eng.load(data)
    assert eng.split(RULE) == len(pieces) and eng.train_split(200) == 200
    assert [tuple(m) for m in eng.split_merges().tolist()] == want
    assert eng.train_split_info()["stop_reason"] == stop


def _same_special(eng, data, what):
    want, wp, wi = api.split_host_special(data, RULE, SPECIALS)
    got = _split(eng, data, SPECIALS)
    assert got.size == want.size and (got == want).all(), what
    piece, index = eng.special_pieces()
    assert piece.tolist() == wp.tolist() and index.tolist() == wi.tolist(), what


@pytest.mark.parametrize("centre", [64, 1024, T])
def test_a_special_around_an_edge(eng, centre):
    """a match at -66..+6 of the edge: its bytes, the bytes before it and the bytes after it fall on both sides"""
    background = mixed(T + 1024 + 300, 9)
    for d in range(-66, 7):
        p = centre + d
        if p < 0:
            continue
        for sp in (EOT, b"\xe2\x82" + SPECIALS[1]):
            buf = bytearray(background)
            buf[p:p + len(sp)] = sp
            _same_special(eng, bytes(buf), (centre, d, sp))


def test_a_special_breaks_every_chain(eng):
    for at in (T + 7, T + 8, T + 9, 5, 2 * T + 1000):  # inside a run of numbers longer than a tile
        _same_special(eng, b"a" + b"7" * at + EOT + b"7" * (T + 11) + b"x", ("numbers", at))
    for at in (T + 7, 5, 2 * T + 1000):  # inside a run of spaces longer than a tile, before its last newline
        for head in (b"x\n", b"!\n"):
            _same_special(eng, head + b" " * at + EOT + b" " * (T + 11) + b"\n x", ("spaces", at, head))
            _same_special(eng, head + b" " * at + SPECIALS[1] + b"\n" * (T + 11) + b"  \nx", ("newlines", at, head))
    for fill in (b"a", b" "):
        for p in _edges(-4, 4):  # directly after !\n\n: the run after the match has no P before it
            buf = bytearray(fill * (T + 96))
            probe = b"!\n\n" + EOT + b"\n\n  \nx"
            buf[p:p + len(probe)] = probe
            _same_special(eng, bytes(buf), ("after !", p))
    rng = np.random.default_rng(10)  # many matches, some adjacent, in a mixed text
    parts = []
    for _ in range(3000):
        r = rng.random()
        parts.append(EOT if r < 0.1 else SPECIALS[1] if r < 0.2 else ITEMS[int(rng.integers(len(ITEMS)))])
    _same_special(eng, b"".join(parts), "many")


def test_state():
    e = api.Engine(0)
    try:
        with pytest.raises(api.BpeError, match=ESTATE):
            e.split(RULE)  # nothing loaded
        data = mixed(3 * T + 5, 11)
        assert (_split(e, data) == api.split_host(data, RULE)).all()
        assert e.split("gpt2") == api.split_host(data, "gpt2").size - 1
        assert (e.split_offsets() == api.split_host(data, "gpt2")).all()
        assert (_split(e, data, SPECIALS) == api.split_host(data, RULE, specials=SPECIALS)).all()
        assert (_split(e, data) == api.split_host(data, RULE)).all()  # ... and without them again
        e.load(b"")
        assert e.split(RULE) == 0 and e.split_offsets().tolist() == [0]
    finally:
        e.close()


def test_the_preset_has_no_tables(eng):
    with pytest.raises(api.BpeError, match="no tables"):
        api.split_rule(RULE)
    cls = np.zeros(256, np.uint8)
    brk = np.zeros(16, np.uint16)
    import ctypes
    rc = eng.L.bpe_gpu_split_rule(api.SPLIT_PRESETS[RULE], cls.ctypes.data_as(ctypes.c_void_p), brk.ctypes.data_as(ctypes.c_void_p))
    assert eng.L.bpe_gpu_strerror(rc) == b"invalid argument"

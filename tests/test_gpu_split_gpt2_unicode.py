"""BPE_SPLIT_GPT2_UNICODE on the device (split.hip k_split_mark_gpt2u, special.hip k_sp_patch,
bpe_gpu_split_preset): the offsets equal api.split_host(data, "gpt2_unicode"), which
tests/test_split_gpt2_unicode_host.py pins to the regular expression, and encode_split /
train_split over them equal encode_batch / the restatement (tests/train_split_ref.py) over
the host's pieces."""
import numpy as np
import pytest

import golden_lib as G
import train_split_ref as R
from llmtokenizer_amd import api

pytestmark = pytest.mark.gpu

RULE = "gpt2_unicode"
# bytes one workgroup handles per step and bytes one grid step covers: the cases below are parametrised by them
# before the library is loaded, and test_the_geometry_is_the_library_s holds them to bpe_gpu_split_info
T, GB = 4096, 4096 * 2048
EOT = b"<|endoftext|>"
SPECIALS = [EOT, b"\xac|x|"]
ITEMS = [b"'", b"s", b"t", b"re", b"ll", b"v", b"a", b"Z", b"1", b"!", b"\n", b" ", b" ", b" ", b"\x1c", b"word", b" the"]
ITEMS += [s.encode() for s in ("é", "ß", "Ж", "中", "\U00010400", "٣", "²", "½", "\U0001d7d8", "\u00a0", "\u2003", "\u3000",
                               "\u2028", "\u0085", "—", "€", "\U0001f600", "\u0301")]
ITEMS += [b"\x80", b"\xc3", b"\xe2\x82", b"\xf0\x9f\x98", b"\xc0\x80", b"\xed\xa0\x80", b"\xf4\x90\x80\x80", b"\xff"]


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


def _split(eng, data, specials=None):
    eng.load(data)
    nd = eng.split(RULE, specials)
    off = eng.split_offsets()
    assert off.dtype == np.uint64 and off.size == nd + 1
    return off


def _same(eng, data, what=None):
    got, want = _split(eng, data), api.split_host(data, RULE)
    assert got.size == want.size and (got == want).all(), what if what is not None else len(data)


def test_the_geometry_is_the_library_s():
    """a tile or grid of another size would leave the edge cases of this file off the edges: fail then"""
    assert api.split_info() == {"tile": T, "grid_bytes": GB}


@pytest.mark.parametrize("n", [0, 1, 15, 16, 17, 1023, 1024, 1025, T - 1, T, T + 1])
def test_offsets_equal_the_host_definition(eng, n):
    for seed in range(4):
        _same(eng, mixed(n, 100 * n + seed), (n, seed))


def test_the_grid_stride(eng):
    big = mixed(GB + 1, 7)
    for n in (GB - 1, GB + 1):
        _same(eng, big[:n], n)


def _edges():
    centres = [16 * k for k in range(1, 9)] + [1024, T]
    return sorted({c + d for c in centres for d in range(-8, 9)})


PROBES = {
    "two-byte letter": "é".encode(), "three-byte letter": "中".encode(), "four-byte letter": "\U00010400".encode(),
    "U+3000 before text": "\u3000\u3000b".encode(), "truncated four-byte sequence": b"\xf0\x9f\x98", "e-acute 's": "é's".encode(),
}


@pytest.mark.parametrize("name", sorted(PROBES))
@pytest.mark.parametrize("fill", [b"a", b"!"])
def test_the_window_across_every_edge(eng, name, fill):
    """a probe whose first byte falls at -8..+8 of every 16-byte edge up to 128, of 1,024 and of the tile: the
    eight bytes before and after a thread's 16 come from its neighbours in the wave, or lanes 0 and 63 load them"""
    probe, n = PROBES[name], T + 64
    for p in _edges():
        buf = bytearray(fill * n)
        buf[p:p + len(probe)] = probe
        _same(eng, bytes(buf), (name, p))


@pytest.mark.parametrize("ch", ["é", "\u3000", "中", "\U00010400"])
def test_the_text_end_inside_a_sequence_at_the_same_edges(eng, ch):
    """the end of the text cuts a sequence: its bytes are ill-formed, whatever continuation bytes the slack past n holds
    (a longer text of continuation bytes was resident just before).  n runs over -8..+8 of every 16-byte edge up
    to 128, of 1,024 and of the tile: every number of text bytes in a thread's own 16 and in the eight bytes lane
    63 loads past them"""
    full = ch.encode()
    for n in _edges():
        for k in range(1, len(full) + 1):
            for head in (b"a", b" "):
                eng.load(b"\x80" * (n + 64))
                data = head * (n - k) + full[:k]
                _same(eng, data, (ch, n, k, head))


def test_ascii_text_equals_gpt2(eng):
    data = G.input_bytes(G.load("prose"))[:3 * T + 5] + b" don't it'll've  'd\n\n x"
    assert max(data) < 0x80
    want = _split(eng, data)
    eng.load(data)
    eng.split("gpt2")
    assert (eng.split_offsets() == want).all() and (want == api.split_host(data, "gpt2")).all()


@pytest.mark.parametrize("at", [5, 1023, 1030, 2 * T + 100])
def test_one_character_in_one_wave(eng, at):
    """the only byte >= 0x80 sits in one wave's windows: that wave decodes, the others of the launch run gpt2's body"""
    buf = bytearray((b"it's a word, isn't it?  " * 700)[:3 * T + 9])
    buf[at:at + 3] = "\u3000".encode()
    _same(eng, bytes(buf), at)


@pytest.fixture(scope="module")
def text():
    """20 kB of prose with non-ASCII words, numbers, white space and punctuation, the host's offsets and pieces"""
    fx = G.load("prose")
    words = G.input_bytes(fx).split(b" ")
    extra = [s.encode() for s in (" café", " naïve", " Привет", " мир", " 中文", "中", " ٣٤٥", " 7½", "\u3000", " x", " —", "…",
                                  " don't", " it'll", " l'été", "\n\n", " \U0001f600", "é's")]
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


def test_specials(eng):
    """matches at -8..+8 of a 16-byte and a 1,024-byte edge and directly after E2 82: the positions around a match are
    decided again over the bytes the definition substitutes"""
    background = mixed(2 * 1024 + 300, 9)
    for centre in (64, 1024):
        for d in range(-8, 9):
            for sp in (EOT, b"\xe2\x82" + SPECIALS[1], SPECIALS[1] + b"'s"):
                buf = bytearray(background)
                p = centre + d
                buf[p:p + len(sp)] = sp
                data = bytes(buf)
                want, wp, wi = api.split_host_special(data, RULE, SPECIALS)
                got = _split(eng, data, SPECIALS)
                assert got.size == want.size and (got == want).all(), (centre, d, sp)
                piece, index = eng.special_pieces()
                assert piece.tolist() == wp.tolist() and index.tolist() == wi.tolist()
    # many matches, some adjacent, in a mixed text
    rng = np.random.default_rng(10)
    parts = []
    for _ in range(3000):
        r = rng.random()
        parts.append(EOT if r < 0.1 else SPECIALS[1] if r < 0.2 else ITEMS[int(rng.integers(len(ITEMS)))])
    data = b"".join(parts)
    want = api.split_host(data, RULE, specials=SPECIALS)
    got = _split(eng, data, SPECIALS)
    assert got.size == want.size and (got == want).all()


def test_the_preset_has_no_tables(eng):
    with pytest.raises(api.BpeError, match="no tables"):
        api.split_rule(RULE)
    cls = np.zeros(256, np.uint8)
    brk = np.zeros(16, np.uint16)
    import ctypes
    rc = eng.L.bpe_gpu_split_rule(api.SPLIT_PRESETS[RULE], cls.ctypes.data_as(ctypes.c_void_p), brk.ctypes.data_as(ctypes.c_void_p))
    assert eng.L.bpe_gpu_strerror(rc) == b"invalid argument"

"""BPE_TEXT_REPLACE / BPE_TEXT_HOLD on the device (llmtokenizer_amd/csrc/utf8.hip; the contract: include/bpe_gpu.h,
"Decoded text"): Engine.decode_docs(errors=) byte for byte against api.utf8_repair_host, with byte_off and held, where
the kernels can go wrong: the host test's edge cases across a lane's, a wave's and a tile's edge, an ASCII tile beside
a dirty one, the direct-store path, text bounds around a character on a tile edge, the sizes around a lane, a tile
and the grid; then the RAW mode against the old decoders and Tokenizer.decode_rows against CPython.  Ids are byte
values under an empty merge list, so any byte sequence can be decoded (but NUL, which the decoders drop)."""
import ctypes
import json
import os

import numpy as np
import pytest

import golden_lib as G
from llmtokenizer_amd import api
from llmtokenizer_amd.vocab import Tokenizer, Vocab
from test_utf8_host import ALPHABET, FIXED, cpython

pytestmark = pytest.mark.gpu

NONE = np.zeros((0, 2), dtype=np.uint32)  # the empty merge list
MODES = ["replace", "hold"]
BAD = ALPHABET[1:]  # the alphabet's bytes >= 0x80


@pytest.fixture(scope="module")
def eng():
    e = api.Engine(0)
    yield e
    e.close()


def same(eng, data, off, errors):
    """the device against the host definition over `data` held as texts by `off`"""
    data = bytes(data)
    out, bo, held = eng.decode_docs(np.frombuffer(data, dtype=np.uint8), off, NONE, errors=errors)
    ref, ref_bo, ref_held = api.utf8_repair_host(data, off, errors)
    assert np.array_equal(bo, ref_bo) and np.array_equal(held, ref_held), (bo[:8], ref_bo[:8], held[:8], ref_held[:8])
    assert len(out) == len(ref), (len(out), len(ref))
    assert out == ref, np.flatnonzero(np.frombuffer(out, np.uint8) != np.frombuffer(ref, np.uint8))[:5]
    return out, held


def sprinkled(n):
    """n ASCII bytes with a byte >= 0x80 every 997 and at both ends"""
    d = np.full(n, 0x61, dtype=np.uint8)
    d[::997] = np.resize(np.frombuffer(BAD, np.uint8), len(d[::997]))
    d[-1:] = 0xE0
    return d.tobytes()


@pytest.mark.parametrize("errors", MODES)
@pytest.mark.parametrize("edge", ["thread", "wave", "tile"])
def test_edges(eng, edge, errors):
    """every fixed case twice across the edge: its first byte alone before it, and its last byte alone behind it; as
    one text, and each case the end of a text of its own"""
    info = api.utf8_info()
    E = {"thread": info["thread"], "wave": 64 * info["thread"], "tile": info["tile"]}[edge]
    buf, off = bytearray(), [0]
    for s in (s for s in FIXED if len(s) > 1):
        for before in (1, len(s) - 1):
            buf += b"a" * (-len(buf) % E + E - before) + s
            off.append(len(buf))
    buf += b"a" * 40
    same(eng, buf, [0, len(buf)], errors)
    same(eng, buf, off + [len(buf)], errors)


@pytest.mark.parametrize("errors", MODES)
def test_fast_path_beside_a_dirty_tile(eng, errors):
    """an all-ASCII tile on both sides of a tile with a bad byte at its first and its last position, and bad bytes 3
    before to 3 behind a lane's edge, each in a lane pair of its own"""
    info = api.utf8_info()
    P, T = info["thread"], info["tile"]
    d = np.full(4 * T, 0x62, dtype=np.uint8)
    d[T], d[2 * T - 1] = 0xFF, 0xE0
    for j, k in enumerate(range(-3, 4)):
        d[3 * T + 4 * P * (j + 1) + k] = BAD[j]
    same(eng, d, [0, d.size], errors)


@pytest.mark.parametrize("k", [1, 2])
def test_direct_path(eng, k):
    """a tile of FF triples: more than the staging holds, so it is stored directly; k FF in the tile before it put it
    and the ASCII tiles behind it at offsets 2 k past a multiple of 16 (2: their lanes store bytes; 4: words)"""
    info = api.utf8_info()
    T = info["tile"]
    assert 3 * T > info["stage"]
    d = b"\xFF" * k + b"c" * (T - k) + b"\xFF" * T + b"d" * (T + 1000)
    out, _ = same(eng, d, [0, len(d)], "replace")
    assert len(out) == len(d) + 2 * k + 2 * T


@pytest.mark.parametrize("errors", MODES)
@pytest.mark.parametrize("d", range(-3, 4))
def test_text_bounds(eng, d, errors):
    """texts bounded d bytes from the start of a 4-byte character on a tile edge, empty texts before, between and
    after, a text that is nothing but a held tail, the last text ending at n"""
    T = api.utf8_info()["tile"]
    ch = "\U0001F600".encode()
    data = b"a" * (T - 2) + ch + b"b" * 50 + ch[:3]
    n = len(data)
    out, held = same(eng, data, [0, 0, T - 2 + d, T - 2 + d, n - 3, n, n], errors)
    assert held.tolist() == ([0, 0 if d <= 0 else d, 0, 0, 3, 0] if errors == "hold" else [0] * 6)


@pytest.mark.parametrize("errors", MODES)
def test_sizes(eng, errors):
    info = api.utf8_info()
    P, T = info["thread"], info["tile"]
    for n in (0, 1, P - 1, P, P + 1, T - 1, T, T + 1):
        same(eng, sprinkled(n), [0, n], errors)
        same(eng, sprinkled(n), [0, n // 3, n // 3, n], errors)
    n = info["grid"] * T + 5  # the grid-stride turn
    same(eng, sprinkled(n), [0, 0, n - 2, n], errors)


def test_raw_and_none(eng):
    """BPE_TEXT_RAW through the new entry points is the old decoders' output (documents, rows, the flat sequence), held
    all 0; errors=None returns what it always returned; another mode is refused"""
    data = b"".join(FIXED)
    ids = np.frombuffer(data, dtype=np.uint8).astype(np.uint32)
    off = np.array([0, 7, 7, ids.size], dtype=np.uint64)
    vp = ctypes.c_void_p
    old = eng.decode_docs(ids, off, NONE)
    assert isinstance(old, tuple) and len(old) == 2 and old[0] == data and np.array_equal(old[1], off)
    docs = (eng.ctx, ids.ctypes.data_as(vp), ids.size, off.ctypes.data_as(vp), 3, None, 0, None, None)
    flat = (eng.ctx, ids.ctypes.data_as(vp), ids.size, None, 0, None, 0, None, None)
    got = eng._decode_text(eng.L.bpe_gpu_decode_text, docs + (0,), 3, "raw")
    assert got[0] == data and np.array_equal(got[1], off) and not got[2].any()
    assert eng._decode_text(eng.L.bpe_gpu_decode_text, flat + (0,), 1, "raw")[0] == data
    text, _, held = eng._decode_text(eng.L.bpe_gpu_decode_text, flat + (2,), 1, "flat")
    assert (text, int(held[0])) == cpython(data, "hold")
    rows = np.resize(ids, (5, 9))
    eng.unpack_rows(rows)
    old = eng.decode_rows(NONE)
    got = eng._decode_text(eng.L.bpe_gpu_decode_rows_text, (eng.ctx, None, 0, None, None, 0), 5, "raw")
    assert len(old) == 2 and got[0] == old[0] and np.array_equal(got[1], old[1]) and not got[2].any()
    rep = eng.decode_rows(NONE, errors="replace")
    assert [rep[0][int(a):int(b)] for a, b in zip(rep[1], rep[1][1:])] == [cpython(r.astype(np.uint8).tobytes(), "replace")[0] for r in rows]
    for fn, args in ((eng.L.bpe_gpu_decode_text, docs), (eng.L.bpe_gpu_decode_rows_text, (eng.ctx, None, 0, None, None))):
        with pytest.raises(api.BpeError, match="invalid argument"):
            eng._decode_text(fn, args + (3,), 5, "mode 3")
    with pytest.raises(api.BpeError, match="errors must be"):
        eng.decode_docs(ids, off, NONE, errors="strict")


def test_tokenizer_decode_rows_hold(tmp_path):
    """the public path: a [B, L] int64 grid whose rows end inside a character, with a special that is skipped and an
    EOS, through a vocabulary's ids: the strings and held counts are CPython's incremental decoder's over the bytes"""
    with open(os.path.join(G.GOLD, "vocab", "vocab_cl100k.json"), encoding="utf-8") as f:
        (tmp_path / "tokenizer.json").write_text(json.dumps(json.load(f)["tokenizer_json"], ensure_ascii=False), encoding="utf-8")
    tok = Tokenizer(Vocab.from_tokenizer_json(tmp_path / "tokenizer.json"))
    try:
        eos, ims = (int(x) for x in tok.vocab.special_ids[:2])
        ids, _ = tok.encode_batch(["é€😀 a 😀€é".encode()])
        B, L = ids.size + 1, ids.size + 3
        rows = np.full((B, L), eos, dtype=np.int64)
        for k in range(B):  # row k: a special, then the first k ids, then the EOS
            rows[k, 0], rows[k, 1:1 + k] = ims, ids[:k]
        kw = dict(pad_id=None, eos=eos, skip_specials=True)
        raw = tok.decode_rows(rows, **kw)
        assert all(isinstance(t, bytes) for t in raw) and raw[B - 1] == "é€😀 a 😀€é".encode()
        texts, held = tok.decode_rows(rows, errors="hold", **kw)
        want = [cpython(t, "hold") for t in raw]
        assert texts == [w.decode() for w, _ in want] and held.dtype == np.uint32 and held.tolist() == [h for _, h in want]
        assert held.any() and all(isinstance(t, str) for t in texts)
        assert tok.decode_rows(rows, errors="replace", **kw) == [t.decode("utf-8", "replace") for t in raw]
        assert tok.decode_batch(ids[:3], [0, 1, 3], errors="replace") == [t.decode("utf-8", "replace") for t in tok.decode_batch(ids[:3], [0, 1, 3])]
        text, h = tok.decode(ids[:-1], errors="hold")
        assert (text.encode(), int(h[0])) == cpython(tok.decode(ids[:-1]), "hold")
    finally:
        tok.close()

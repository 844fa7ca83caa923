"""BPE_SPLIT_GPT2 on the device (split.hip k_split_mark_gpt2, bpe_gpu_split_preset):
the offsets equal Python's re over the bytes pattern of bpe_gpu.h (and, where re
is too slow, api.split_host, which tests/test_split_gpt2_host.py pins to re), and
encode_split / train_split over them equal encode_batch / the restatement
(tests/train_split_ref.py) over the same pieces."""
import ctypes
import re

import numpy as np
import pytest

import golden_lib as G
import train_split_ref as R
from llmtokenizer_amd import _lib, api

pytestmark = pytest.mark.gpu

# bpe_gpu.h BPE_GPU_SPLIT_TILE and BPE_GPU_SPLIT_TILE * BPE_GPU_SPLIT_GRID (tests/test_gpu_split.py holds them to the library)
T, GB = 4096, 4096 * 2048
ESTATE = "call out of order"
PATTERN = re.compile(rb"'s|'t|'re|'ve|'m|'ll|'d| ?[A-Za-z\x80-\xff]+| ?[0-9]+| ?[^\sA-Za-z0-9\x80-\xff]+|\s+(?!\S)|\s+")
# rich in apostrophes, contraction letters, spaces and newlines
ALPHABET = np.frombuffer(b"'''  \n\nsstrevmlda1!,\t\xc3", np.uint8)


def re_offsets(data):
    out, pos = [], 0
    for m in PATTERN.finditer(data):
        assert m.start() == pos and m.end() > pos
        out.append(pos)
        pos = m.end()
    assert pos == len(data)
    return np.array(out + [len(data)], dtype=np.uint64)


def cut(data, off):
    return [data[int(a):int(b)] for a, b in zip(off, off[1:])]


def rich(n, seed):
    return np.random.default_rng(seed).choice(ALPHABET, n).tobytes()


@pytest.fixture(scope="module")
def eng():
    e = api.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def text():
    """64 KiB of prose with contractions, its re offsets and pieces, and the golden merge list learnt on the prose"""
    fx = G.load("prose")
    prose = G.input_bytes(fx)
    extra = [b" don't", b" it'll've", b" I'm", b" we're", b" you'd", b" 'tis", b"  'd", b" they've\n\n", b" x's 42",
             b" rock'n'roll", b"\t'S", b" caf\xc3\xa9's  \n"]
    rng = np.random.default_rng(3)
    words = prose.split(b" ")
    out, size = [], 0
    while size < 65536:
        w = words[int(rng.integers(len(words)))]
        w = (b" " + w) if rng.random() < 0.8 else extra[int(rng.integers(len(extra)))]
        out.append(w)
        size += len(w)
    data = b"".join(out)[:65536]
    off = re_offsets(data)
    assert data.count(b"'") > 500
    return data, off, cut(data, off), np.asarray(fx["merges"], dtype=np.uint32).reshape(-1, 2)


def _split(eng, data):
    eng.load(data)
    nd = eng.split("gpt2")
    off = eng.split_offsets()
    assert off.dtype == np.uint64 and off.size == nd + 1
    return off


@pytest.mark.parametrize("n", [0, 1, 2, 15, 16, 17, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1])
def test_offsets_equal_re(eng, n):
    for seed in range(4):
        data = rich(n, 100 * n + seed)
        assert _split(eng, data).tolist() == re_offsets(data).tolist(), (n, seed)


def test_the_grid_stride_against_split_host(eng):
    data = rich(GB + T + 5, 5)
    want = api.split_host(data, "gpt2")
    k = 3 * T  # (the head once more against re itself)
    head = re_offsets(data[:k])[:-8]
    assert want[:head.size].tolist() == head.tolist()
    got = _split(eng, data)
    assert got.size == want.size and (got == want).all()


def _edges():
    centres = [16 * k for k in range(1, 9)] + [1024, T]
    return sorted({c + d for c in centres for d in range(-6, 7)})


@pytest.mark.parametrize("probe,starts", [(b"'ll", (0, 3)), (b"'s", (0, 2)), (b"  ", (0, 1))])
def test_the_window_across_every_edge(eng, probe, starts):
    """a background of `a` and one probe at p: the four bytes before and the byte after a thread's 16 come from
    its neighbours in the wave, or are loaded by the wave's first and last lane"""
    n = T + 64
    for p in _edges():
        buf = bytearray(b"a" * n)
        buf[p:p + len(probe)] = probe
        data = bytes(buf)
        want = [0] + [p + s for s in starts] + [n]
        assert re_offsets(data).tolist() == want
        assert _split(eng, data).tolist() == want, (probe, p)


@pytest.mark.parametrize("tail", [b"  ", b" \n", b"'l", b"'s"])
@pytest.mark.parametrize("n", [16, 17, 1024, 1025, T - 1, T, T + 1])
def test_the_text_end_at_the_same_edges(eng, n, tail):
    """the end of the text is part of the rule: what lies past n in the buffer is no text (a longer text of
    contraction letters was resident just before)"""
    eng.load(b"l" * (n + 64))
    data = b"a" * (n - len(tail)) + tail
    want = re_offsets(data)
    assert _split(eng, data).tolist() == want.tolist(), (n, tail)
    # one byte shorter and longer: the same tail one byte off the edge
    for data in (data[1:], b"a" + data):
        assert _split(eng, data).tolist() == re_offsets(data).tolist(), (len(data), tail)


def test_encode_split_equals_encode_batch_over_the_re_pieces(eng, text):
    data, off, pieces, merges = text
    want_ids, want_off = api.encode_batch(pieces, merges)
    eng.load(data)
    assert eng.split("gpt2") == len(pieces)
    assert (eng.split_offsets() == off).all()
    eng.encode_split(merges)
    assert (eng.split_offsets() == off).all()
    ids, id_off = eng.ids(), eng.doc_offsets()
    assert id_off.tolist() == want_off.tolist()
    assert ids.size == want_ids.size and (ids == want_ids).all()
    assert ids.size < len(data)  # the merges did apply


def test_api_encode_split(text):
    data, off, pieces, merges = text
    want_ids, want_off = api.encode_batch(pieces, merges)
    ids, id_off, byte_off = api.encode_split(data, merges, rule="gpt2")
    assert (ids == want_ids).all() and id_off.tolist() == want_off.tolist() and byte_off.tolist() == off.tolist()
    ids, id_off, byte_off = api.encode_split(b"", merges, rule="gpt2")
    assert ids.size == 0 and id_off.tolist() == [0] and byte_off.tolist() == [0]


@pytest.fixture(scope="module")
def trained(text):
    """the restatement's 200 merges over the re pieces"""
    want, stop, _ = R.train(text[2], 200)
    assert len(want) == 200
    return want, stop


def test_api_train_split(text, trained):
    got = api.train_split(text[0], rule="gpt2", max_merges=200)
    assert got.dtype == np.uint32 and [tuple(m) for m in got.tolist()] == trained[0]


def test_engine_train_split_and_state(text, trained):
    data, off, pieces, merges = text
    L = _lib.load()
    e = api.Engine(0)
    try:
        with pytest.raises(api.BpeError, match=ESTATE):
            e.split("gpt2")  # nothing loaded
        e.load(data)
        nd = ctypes.c_size_t(0)
        for bad in (3, -1, 1000):
            rc = L.bpe_gpu_split_preset(e.ctx, bad, ctypes.byref(nd))
            assert L.bpe_gpu_strerror(rc) == b"invalid argument"
        with pytest.raises(api.BpeError, match=ESTATE):
            e.split_offsets()  # a refused preset leaves no offsets
        assert e.split("gpt2") == len(pieces)
        assert e.train_split(200) == 200
        assert [tuple(m) for m in e.split_merges().tolist()] == trained[0]
        info = e.train_split_info()
        assert info["pieces"] == len(pieces) and info["stop_reason"] == trained[1]
        assert (e.split_offsets() == off).all()  # training keeps them
        # a later split replaces the offsets and drops the training that described the earlier ones
        want = api.split_host(data, "words")
        assert e.split("words") == want.size - 1
        assert (e.split_offsets() == want).all()
        with pytest.raises(api.BpeError, match=ESTATE):
            e.split_merges()
        with pytest.raises(api.BpeError, match=ESTATE):
            e.train_split_info()
        assert e.split("gpt2") == len(pieces) and (e.split_offsets() == off).all()
        e.load(b"")
        assert e.split("gpt2") == 0 and e.split_offsets().tolist() == [0]
    finally:
        e.close()


@pytest.mark.parametrize("rule", ["lines", "words"])
def test_table_presets_through_the_preset_call(eng, text, rule):
    data = text[0]
    L = _lib.load()
    eng.load(data)
    want_n = eng.split(rule)  # bpe_gpu_split with the tables
    want = eng.split_offsets()
    assert (want == api.split_host(data, rule)).all()
    eng.split("gpt2")  # (other offsets in between)
    nd = ctypes.c_size_t(0)
    _lib.check(L.bpe_gpu_split_preset(eng.ctx, api.SPLIT_PRESETS[rule], ctypes.byref(nd)), "split_preset")
    assert nd.value == want_n and (eng.split_offsets() == want).all()

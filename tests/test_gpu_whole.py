"""Whole-text rows on the device (whole.hip, bpe_gpu_pack_whole, Engine.whole_rows / pack_whole,
Tokenizer.encode_packed(whole=True)), held bit for bit to api.pack_whole_host (the contract in plain loops, itself held to
the contract by test_whole_host.py) over Engine.ids() and Engine.text_offsets() of the same batch."""
import ctypes
import json
import os

import numpy as np
import pytest

import golden_lib as G
from llmtokenizer_amd import _lib, api
from llmtokenizer_amd.api import BpeError
from llmtokenizer_amd.vocab import Tokenizer, Vocab

pytestmark = pytest.mark.gpu

PAD, BOS, EOS = 0xFFFFFFF0, 70001, 70002
# texts per workgroup step and per grid step of the placement kernels (api.whole_info(), held to these below)
WG, GR = 256, 1 << 18
# one merge that no text here holds: every byte stays one id
MERGES = np.array([[0xF0, 0xF1]], dtype=np.uint32)
ALPHA = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz    ", dtype=np.uint8)
KEYS = ("rows", "seg", "pos", "text_row", "text_col")


@pytest.fixture(scope="module")
def eng():
    e = api.Engine(0)
    yield e
    e.close()


def load_lengths(eng, lens, seed=3):
    """a resident text batch whose texts have exactly lens ids; returns (ids, text_off)"""
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    eng.load_texts(np.random.default_rng(seed).choice(ALPHA, int(off[-1])).tobytes(), offsets=off)
    eng.split("words")
    eng.encode_split(MERGES)
    toff = eng.text_offsets()
    assert np.array_equal(toff, off)
    return eng.ids(), toff


def check(eng, ids, toff, L, bos=None, eos=None):
    """the query and every output of the resident batch against the host's"""
    want = api.pack_whole_host(ids, toff, L, PAD, bos, eos)
    assert eng.whole_rows(L, bos, eos) == (want["rows"].shape[0], want["cells"], want["n_long"])
    got = eng.pack_whole(L, PAD, bos, eos, segments=True, positions=True, placement=True)
    for g, key in zip(got, KEYS):
        w = want[key]
        assert g.dtype == np.uint32 and g.shape == w.shape, key
        assert np.array_equal(g, w), (key, L, bos, eos, np.flatnonzero(g.reshape(-1) != w.reshape(-1))[:5])
    return want


def test_whole_info():
    assert api.whole_info() == {"per_thread": 1, "per_block": WG, "per_grid": GR, "fill_per_thread": 4}


@pytest.mark.parametrize("T", [1, 2, 63, 64, 65, WG - 1, WG, WG + 1, GR - 1, GR, GR + 1])
def test_text_counts_around_the_placement_steps(eng, T):
    ids, toff = load_lengths(eng, np.random.default_rng(T).integers(0, 4, T), seed=T)
    check(eng, ids, toff, 8)
    check(eng, ids, toff, 8, BOS, EOS)


@pytest.mark.parametrize("lens,openers", [([5], 1), ([4], 2), ([3, 2, 2], 3)], ids=["alone", "two_a_row", "every_third"])
def test_longest_chain(eng, lens, openers):
    """row openers at every text, every second and every third: every round of the doubling has members to mark"""
    T = 70001
    ids, toff = load_lengths(eng, np.resize(lens, T))
    want = check(eng, ids, toff, 8)
    assert want["rows"].shape[0] == -(-T // openers) and (want["text_col"][::openers] == 0).all()


# text lengths that end at, before and behind a row's, a 16-byte vector's, a wave's and a tile's last cell
EDGES = {1: [0, 1, 2, 3], 5: [0, 1, 2, 3, 4, 5, 6, 14, 15], 8: [0, 1, 3, 4, 5, 7, 8, 9, 16, 23],
         1024: [0, 1, 3, 4, 5, 252, 255, 256, 257, 767, 768, 1020, 1023, 1024, 1025, 2048, 3071]}


@pytest.mark.parametrize("bos,eos", [(None, None), (BOS, None), (BOS, EOS)], ids=["plain", "bos", "bos_eos"])
@pytest.mark.parametrize("L", [1, 5, 8, 1024])
def test_lengths_around_the_fill_edges(eng, L, bos, eos):
    w = (bos is not None) + (eos is not None)
    rng = np.random.default_rng(L + w)
    mid = rng.choice(EDGES[L], 90)
    for first, last in ((L - w, L - w), (L - w - 1, 1), (L - w + 1, L - w - 1), (0, 0)):  # the first and last row: exact, off by one
        ids, toff = load_lengths(eng, np.concatenate([[max(first, 0)], mid, [max(last, 0)]]), seed=L)
        check(eng, ids, toff, L, bos, eos)


@pytest.mark.parametrize("L", [5, 8])
def test_long_texts(eng, L):
    """w_k = L + 1, 2 L and 3 L - 1: first, last, adjacent, and followed by a text that would fit their last row"""
    for bos, eos in ((None, None), (BOS, EOS)):
        w = (bos is not None) + (eos is not None)
        a, b, c = L + 1 - w, 2 * L - w, 3 * L - 1 - w
        lens = [a, 1, 2, c, b, a, 1, 0, 3, b, 1, c]
        want = check(eng, *load_lengths(eng, lens, seed=L), L, bos, eos)
        assert want["n_long"] == 6 and want["text_col"][1] == 0 and want["text_row"][1] == 2  # (not in the long text's last row)
        assert check(eng, *load_lengths(eng, [a, c, b] * 50, seed=L + 1), L, bos, eos)["n_long"] == 150  # all texts long


def test_empty_texts_and_no_text(eng):
    ids, toff = load_lengths(eng, [0, 0, 3, 0, 0, 2, 0, 4] + [0] * 9 + [1, 0])
    check(eng, ids, toff, 4)
    check(eng, ids, toff, 4, BOS, EOS)
    for lens in ([0] * 300, []):
        ids, toff = load_lengths(eng, lens)
        assert eng.whole_rows(4) == (0, 0, 0)
        check(eng, ids, toff, 4)
        check(eng, ids, toff, 4, None, EOS)


def test_outputs_numpy_and_torch(eng):
    import torch
    L = 8
    ids, toff = load_lengths(eng, np.random.default_rng(5).choice(EDGES[8], 700))
    want = check(eng, ids, toff, L, BOS, EOS)
    R = want["rows"].shape[0]
    new = lambda: torch.full((R, L), -7, dtype=torch.int32, device="cuda:0")  # noqa: E731
    host = lambda t: t.cpu().numpy().view(np.uint32)  # noqa: E731
    for seg in (False, True):  # every choice of the optional outputs, as numpy arrays and as tensors
        for pos in (False, True):
            for place in (False, True):
                keys = ["rows"] + ["seg"] * seg + ["pos"] * pos + ["text_row", "text_col"] * place
                got = eng.pack_whole(L, PAD, BOS, EOS, seg, pos, place)
                got = got if isinstance(got, tuple) else (got,)
                assert len(got) == len(keys) and all(np.array_equal(g, want[k]) for g, k in zip(got, keys))
                out = eng.pack_whole(L, PAD, BOS, EOS, placement=place, out=(new(), new() if seg else None, new() if pos else None))
                got = [t for t in out if t is not None]
                assert len(got) == len(keys) and all(np.array_equal(host(g), want[k]) for g, k in zip(got, keys))
    # tensors that are only 4-byte aligned (each one in turn): one cell per lane at a row length the other variant takes
    for odd_one in range(3):
        flats = [torch.full((R * L + 1,), -7, dtype=torch.int32, device="cuda:0") for _ in range(3)]
        out = tuple(f[1:].view(R, L) if j == odd_one else f[:-1].view(R, L) for j, f in enumerate(flats))
        assert out[odd_one].data_ptr() % 16 == 4
        eng.pack_whole(L, PAD, BOS, EOS, out=out)
        for j, (t, f, key) in enumerate(zip(out, flats, KEYS)):
            assert np.array_equal(host(t), want[key]) and int(f[0 if j == odd_one else -1]) == -7  # (the cell beside is untouched)


def test_query_fill_and_a_new_batch_between(eng):
    ids, toff = load_lengths(eng, [3, 5, 8, 9, 1])
    want = api.pack_whole_host(ids, toff, 8, PAD)
    assert eng.whole_rows(8) == eng.whole_rows(8) == (5, 26, 1)  # the query twice
    assert eng.whole_rows(4) == (9, 26, 3) and eng.whole_rows(8, BOS) == (7, 31, 2)  # another description: placed anew
    assert eng.whole_rows(8) == (5, 26, 1) and np.array_equal(eng.pack_whole(8, PAD), want["rows"])
    # a new batch between the query and the fill: the fill places it anew (the C call, so that no query comes between)
    assert eng.whole_rows(8) == (5, 26, 1)
    ids, toff = load_lengths(eng, [8, 8, 1, 8, 2, 6, 1], seed=9)
    want = api.pack_whole_host(ids, toff, 8, PAD)
    rows, R = np.zeros((6, 8), dtype=np.uint32), ctypes.c_size_t(0)
    _lib.check(eng.L.bpe_gpu_pack_whole(eng.ctx, ctypes.byref(api.check_whole(8, PAD)), rows.ctypes.data_as(ctypes.c_void_p), None,
                                        None, None, None, 0, 6, ctypes.byref(R), None, None), "pack_whole")
    assert R.value == 6 and np.array_equal(rows, want["rows"])


def test_refusals_and_the_engine_goes_on(eng):
    eng.load(b"abc")
    with pytest.raises(BpeError, match="call out of order.*no text batch"):
        eng.whole_rows(8)
    eng.load_texts(b"abcdefgh", offsets=[0, 3, 8])
    eng.split("words")
    with pytest.raises(BpeError, match="call out of order.*encode_split first"):
        eng.pack_whole(8, PAD)
    ids, toff = load_lengths(eng, [3, 5, 8, 8, 1])
    host, vp = np.zeros(64, dtype=np.uint32), ctypes.c_void_p
    for s, dev, cap, code, word in ((_lib.Whole(0, 0, 0, 0, 0), 0, 4, "invalid argument", "seq_len is 0"),
                                    (_lib.Whole(8, 4, 0, 0, 0), 0, 4, "invalid argument", "flags 0x4"),
                                    (_lib.Whole((1 << 24) + 1, 0, 0, 0, 0), 0, 4, "out of range", "above 2^24"),
                                    (api.check_whole(8, PAD), 0, 3, "invalid argument", "rows_cap 3 is below the 4 rows"),
                                    (api.check_whole(8, PAD), 1, 4, "invalid argument", "no device pointer")):
        rc = eng.L.bpe_gpu_pack_whole(eng.ctx, ctypes.byref(s), host.ctypes.data_as(vp), None, None, None, None, dev, cap, None, None, None)
        assert eng.L.bpe_gpu_strerror(rc).decode().startswith(code) and word in eng.L.bpe_gpu_last_error().decode()
        assert not host.any()
        check(eng, ids, toff, 8, BOS, EOS)  # the engine goes on


def test_encode_packed_whole(tmp_path):
    import torch
    with open(os.path.join(G.GOLD, "vocab", "vocab_cl100k.json"), encoding="utf-8") as f:
        fx = json.load(f)
    (tmp_path / "tokenizer.json").write_text(json.dumps(fx["tokenizer_json"], ensure_ascii=False), encoding="utf-8")
    tok = Tokenizer(Vocab.from_tokenizer_json(tmp_path / "tokenizer.json"))
    try:
        texts = [b"", b"the quick brown fox", b"jumps", b"", "over the lazy dog, é€😀 12345 it's".encode(), b"a" * 90, b"end"]
        ims_id, eot_id = int(tok.vocab.special_ids[1]), int(tok.vocab.special_ids[0])
        ids, toff = tok.encode_batch(texts)
        want = api.pack_whole_host(ids, toff, 16, 3, ims_id, eot_id)
        got = tok.encode_packed(texts, 16, 3, bos="<|im_start|>", eos="<|endoftext|>", return_segments=True, return_positions=True,
                                return_tensors="pt", whole=True, return_placement=True)
        assert len(got) == 6 and got[5] == want["cells"] and want["n_long"] >= 1
        for t, key in zip(got, KEYS):
            assert t.dtype == torch.int32 and t.is_cuda and np.array_equal(t.cpu().numpy().view(np.uint32), want[key]), key
        rows, N = tok.encode_packed(texts, 16, 3, bos="<|im_start|>", eos="<|endoftext|>", whole=True)
        assert N == want["cells"] and np.array_equal(rows, want["rows"])
        with pytest.raises(BpeError, match="drop_last"):
            tok.encode_packed(texts, 16, 3, drop_last=True, whole=True)
    finally:
        tok.close()

"""Whole-text rows on the host (src/bpe_whole.c: bpe_whole_check, bpe_pack_whole_host; api.pack_whole_host): the plain
loops against the contract of bpe_gpu.h, "Whole-text rows", restated here, over every row length, BOS / EOS
combination and text length at which a text just fits or just does not, the named cases, and every refusal."""
import ctypes

import numpy as np
import pytest

from llmtokenizer_amd import _lib, api
from llmtokenizer_amd.api import BpeError

PAD, NO_TEXT = 0xFFFFFFF0, 0xFFFFFFFF
BOS_EOS = [(None, None), (70001, None), (None, 70002), (70001, 70002)]
KEYS = ("rows", "seg", "pos", "text_row", "text_col", "cells", "n_long")


def contract(ids, toff, L, pad, bos, eos):
    """the contract: a cursor in cells; a text that does not fit moves it to the next row's first cell"""
    cur, cells, place, n_long = 0, {}, [], 0
    for k in range(len(toff) - 1):
        body = ([bos] if bos is not None else []) + [int(i) for i in ids[toff[k]:toff[k + 1]]] + ([eos] if eos is not None else [])
        if len(body) > L or cur % L + len(body) > L:
            cur = -(-cur // L) * L
        place.append(divmod(cur, L))
        for o, v in enumerate(body):
            cells[cur + o] = (v, k, min(o, (cur + o) % L))
        cur += len(body)
        if len(body) > L:
            cur, n_long = -(-cur // L) * L, n_long + 1
    R = (max(cells) // L + 1) if cells else 0
    grid = [cells.get(c, (pad, NO_TEXT, 0)) for c in range(R * L)]
    out = [np.array([g[j] for g in grid], dtype=np.uint32).reshape(R, L) for j in range(3)]
    out += [np.array([p[j] for p in place], dtype=np.uint32) for j in range(2)]
    return dict(zip(KEYS, out + [len(cells), n_long]))


def same(got, want, note):
    for key in KEYS:
        assert np.array_equal(got[key], want[key]) and np.shape(got[key]) == np.shape(want[key]), (key, note)


def batch(lens, seed=0):
    toff = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    return np.random.default_rng(seed).integers(0, 60000, int(toff[-1])).astype(np.uint32), toff


@pytest.mark.parametrize("bos,eos", BOS_EOS, ids=["plain", "bos", "eos", "bos_eos"])
@pytest.mark.parametrize("L", [1, 4, 5, 8])
def test_lengths_around_a_row(L, bos, eos):
    w = (bos is not None) + (eos is not None)
    pool = sorted({v for v in (0, 1, L - w - 1, L - w, L - w + 1, L, L + 1, 3 * L) if v >= 0})
    rng = np.random.default_rng(L * 4 + w)
    for T in (1, 2, 3, 7, 40):
        for rep in range(6):
            lens = rng.choice(pool, T)
            ids, toff = batch(lens, rep)
            same(api.pack_whole_host(ids, toff, L, PAD, bos, eos), contract(ids, toff, L, PAD, bos, eos), (L, bos, eos, lens.tolist()))


@pytest.mark.parametrize("lens,L,bos,eos,R,n_long,place", [
    ([3, 5, 8, 4, 4], 8, None, None, 3, 0, [(0, 0), (0, 3), (1, 0), (2, 0), (2, 4)]),       # exact fits
    ([2, 2], 4, 7, 9, 2, 0, [(0, 0), (1, 0)]),                                              # ... with BOS and EOS
    ([0, 0, 3, 0, 0, 2, 0, 4, 0], 4, None, None, 3, 0,                                      # empty texts, w == 0
     [(0, 0), (0, 0), (0, 0), (0, 3), (0, 3), (1, 0), (1, 2), (2, 0), (3, 0)]),
    ([0, 0, 0], 4, None, None, 0, 0, [(0, 0)] * 3),                                         # ... and nothing else
    ([9, 5, 16, 17], 4, None, None, 14, 4, [(0, 0), (3, 0), (5, 0), (9, 0)]),               # all texts long
    ([1, 5, 1], 4, None, None, 4, 1, [(0, 0), (1, 0), (3, 0)]),                             # a long text's last row is its own
    ([], 8, 1, 2, 0, 0, []),                                                                # T == 0
], ids=["exact", "exact_bos_eos", "empties", "only_empties", "all_long", "long_between", "no_text"])
def test_named_cases(lens, L, bos, eos, R, n_long, place):
    ids, toff = batch(lens)
    got = api.pack_whole_host(ids, toff, L, PAD, bos, eos)
    same(got, contract(ids, toff, L, PAD, bos, eos), lens)
    assert got["rows"].shape == (R, L) and got["n_long"] == n_long
    assert list(zip(got["text_row"].tolist(), got["text_col"].tolist())) == place
    assert got["cells"] == sum(lens) + len(lens) * ((bos is not None) + (eos is not None))


def c_host(s, ids, toff, rows_cap, with_rows=True):
    """bpe_pack_whole_host as it is; returns (the code's text or None, the rows array)"""
    L, vp = _lib.load(), ctypes.c_void_p
    rows = np.full(64, 5, dtype=np.uint32)
    rc = L.bpe_pack_whole_host(ids.ctypes.data_as(vp), ids.size, toff.ctypes.data_as(vp), toff.size - 1,
                               ctypes.byref(s) if s is not None else None, rows.ctypes.data_as(vp) if with_rows else None,
                               None, None, None, None, rows_cap, None, None, None)
    return (L.bpe_gpu_strerror(rc).decode() if rc else None), rows


@pytest.mark.parametrize("kw,code,word", [
    ({"seq_len": 0}, "invalid argument", "seq_len is 0"),
    ({"seq_len": 8, "flags": 4}, "invalid argument", "flags 0x4"),
    ({"seq_len": 8, "flags": 8}, "invalid argument", "flags 0x8"),
    ({"seq_len": (1 << 24) + 1}, "out of range", "seq_len 16777217 above 2^24"),
    ({"seq_len": 8, "pad_id": 1 << 32}, "uint32", "uint32"),
], ids=["zero", "drop_last_bit", "flag_bit", "too_long", "not_uint32"])
def test_check_refuses_and_names_the_field(kw, code, word):
    with pytest.raises(BpeError, match=code) as e:
        api.check_whole(**kw)
    assert word in str(e.value)


def test_host_refusals():
    ids, toff = batch([3, 5, 8])
    good = api.check_whole(8, PAD)
    assert api.check_whole(1 << 24).seq_len == 1 << 24
    assert c_host(good, ids, toff, 2)[0] is None and c_host(good, ids, toff, 0, with_rows=False)[0] is None
    for s, t, cap in ((good, toff, 1), (None, toff, 2), (_lib.Whole(8, 4, 0, 0, 0), toff, 2), (_lib.Whole(0, 0, 0, 0, 0), toff, 2),
                      (good, np.array([0, 9, 8, 16], dtype=np.uint64), 2), (good, np.array([1, 3, 8, 16], dtype=np.uint64), 2),
                      (good, np.array([0, 3, 8, 15], dtype=np.uint64), 2)):
        code, rows = c_host(s, ids, t, cap)
        assert code.startswith("invalid argument") and (rows == 5).all()  # nothing was written
    assert c_host(_lib.Whole((1 << 24) + 1, 0, 0, 0, 0), ids, toff, 2)[0].startswith("out of range")

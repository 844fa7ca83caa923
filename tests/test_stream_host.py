"""Packed streams on the host (llmtokenizer_amd/src/bpe_stream.c: bpe_stream_check and bpe_pack_stream_host, through
api.check_stream / pack_stream_host) against the contract in plain Python (tests/stream_ref.py): the matrix of row
lengths, BOS / EOS combinations, drop_last and text lengths, the empty and exact cases, the query-only call, every
refusal with its message, and the kernel's sizes as bpe_gpu_stream_info reports them.  CPU only."""
import ctypes

import numpy as np
import pytest

import stream_ref as SR
from llmtokenizer_amd import _lib, api
from llmtokenizer_amd.api import BpeError

EINVAL, ERANGE = "invalid argument", "out of range"
PAD = 0xFFFFFFFF


def check(ids, off, L, bos, eos, drop):
    want = SR.pack_stream(ids, off, L, PAD, bos, eos, drop)
    got = api.pack_stream_host(ids, off, L, PAD, bos, eos, drop)
    assert got[3] == want[3]
    for g, w, name in zip(got[:3], want[:3], ("rows", "seg", "pos")):
        assert g.dtype == np.uint32 and g.shape == w.shape, name
        assert np.array_equal(g, w), (name, L, bos, eos, drop, np.flatnonzero(g.reshape(-1) != w.reshape(-1))[:5])
    return got


@pytest.mark.parametrize("drop", [False, True])
@pytest.mark.parametrize("bos,eos", SR.BOS_EOS)
@pytest.mark.parametrize("L", [1, 3, 4, 5, 64, 257])
def test_matrix_equals_the_reference(L, bos, eos, drop):
    lens = SR.matrix_lengths(L, seed=L)
    off = SR.offsets(lens)
    ids = np.random.default_rng(L + 1).integers(0, 60000, int(off[-1]), dtype=np.uint32)
    rows, seg, pos, N = check(ids, off, L, bos, eos, drop)
    w = (bos is not None) + (eos is not None)
    assert N == ids.size + len(lens) * w
    assert rows.shape[0] == (N // L if drop else -(-N // L))
    flat = rows.reshape(-1)[:N]
    if w == 0:
        assert np.array_equal(flat, ids[:flat.size])
    # the cells of one seg value inside one row count 0, 1, 2, ...
    for r in range(rows.shape[0]):
        for k in np.unique(seg[r]):
            sel = seg[r] == k
            assert k == SR.NO_TEXT and not pos[r][sel].any() or np.array_equal(pos[r][sel], np.arange(sel.sum()))


@pytest.mark.parametrize("bos,eos", SR.BOS_EOS)
def test_no_text_and_empty_texts(bos, eos):
    w = (bos is not None) + (eos is not None)
    for drop in (False, True):
        rows, seg, pos, N = check([], [0], 4, bos, eos, drop)  # T == 0
        assert N == 0 and rows.shape == (0, 4)
        rows, seg, pos, N = check([], [0] * 8, 4, bos, eos, drop)  # seven empty texts
        assert N == 7 * w and rows.shape[0] == (N // 4 if drop else -(-N // 4))
    if w == 2:
        rows, seg, pos, N = check([], [0] * 8, 4, bos, eos, False)
        assert rows.reshape(-1)[:14].tolist() == [bos, eos] * 7 and rows.reshape(-1)[14:].tolist() == [PAD, PAD]
        assert seg.reshape(-1).tolist() == [k for k in range(7) for _ in range(2)] + [SR.NO_TEXT] * 2
        assert pos.reshape(-1).tolist() == [0, 1] * 7 + [0, 0]


def test_exact_multiple_and_a_stream_below_one_row():
    ids = np.arange(100, 124, dtype=np.uint32)
    off = [0, 5, 5, 12, 24]
    for bos, eos in SR.BOS_EOS:
        w = (bos is not None) + (eos is not None)
        L = (24 + 4 * w) // 4  # N == 4 L
        a, b = check(ids, off, L, bos, eos, False), check(ids, off, L, bos, eos, True)
        assert a[3] == 4 * L and a[0].shape == (4, L) and all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3]))
        assert (a[1] != SR.NO_TEXT).all()
        big = check(ids, off, 100, bos, eos, False)  # N < L
        assert big[0].shape == (1, 100) and (big[0][0, big[3]:] == PAD).all() and (big[1][0, big[3]:] == SR.NO_TEXT).all()
        assert check(ids, off, 100, bos, eos, True)[0].shape == (0, 100)


def test_a_text_longer_than_many_rows_restarts_its_positions():
    ids = np.arange(50, dtype=np.uint32)
    rows, seg, pos, N = check(ids, [0, 3, 50], 8, 7, 9, False)
    assert N == 54 and rows.shape == (7, 8)
    assert rows[0].tolist() == [7, 0, 1, 2, 9, 7, 3, 4] and pos[0].tolist() == [0, 1, 2, 3, 4, 0, 1, 2]
    assert (seg[1:6] == 1).all() and (pos[1:6] == np.arange(8)).all()
    assert rows[6].tolist() == [45, 46, 47, 48, 49, 9, PAD, PAD] and seg[6].tolist() == [1] * 6 + [SR.NO_TEXT] * 2


def c_call(ids, off, s, rows=None, seg=None, pos=None, cap=0):
    L = _lib.load()
    vp = ctypes.c_void_p
    ids = np.ascontiguousarray(ids, dtype=np.uint32)
    off = np.ascontiguousarray(off, dtype=np.uint64)
    R, N = ctypes.c_size_t(12345), ctypes.c_uint64(12345)
    ptr = lambda a: a.ctypes.data_as(vp) if a is not None else None  # noqa: E731
    rc = L.bpe_pack_stream_host(ptr(ids) if ids.size else None, ids.size, ptr(off), off.size - 1,
                                ctypes.byref(s) if s is not None else None, ptr(rows), ptr(seg), ptr(pos), cap,
                                ctypes.byref(R), ctypes.byref(N))
    return rc, R.value, N.value


def test_query_optional_outputs_and_capacity():
    ids = np.arange(10, dtype=np.uint32)
    off = [0, 4, 10]
    s = api.check_stream(4, PAD, 1, 2)
    assert c_call(ids, off, s) == (0, 4, 14)  # the query: rows == NULL
    assert c_call(ids, off, api.check_stream(4, PAD, 1, 2, drop_last=True)) == (0, 3, 14)
    want = SR.pack_stream(ids, off, 4, PAD, 1, 2)
    for use_seg, use_pos in ((False, False), (True, False), (False, True), (True, True)):
        rows = np.zeros((4, 4), dtype=np.uint32)
        seg = np.full((4, 4), 99, dtype=np.uint32) if use_seg else None
        pos = np.full((4, 4), 99, dtype=np.uint32) if use_pos else None
        assert c_call(ids, off, s, rows, seg, pos, 4) == (0, 4, 14)
        assert np.array_equal(rows, want[0])
        assert seg is None or np.array_equal(seg, want[1])
        assert pos is None or np.array_equal(pos, want[2])
    rows = np.full((4, 4), 77, dtype=np.uint32)
    rc, R, N = c_call(ids, off, s, rows, cap=3)  # a row too little room: refused, the sizes reported, nothing written
    assert _lib.load().bpe_gpu_strerror(rc).decode() == EINVAL and (R, N) == (4, 14) and (rows == 77).all()
    # offsets that do not describe the ids
    for bad in ([1, 4, 10], [0, 11, 10], [0, 4, 9], [0, 4, 11]):
        rc, _, _ = c_call(ids, bad, s, rows, cap=4)
        assert _lib.load().bpe_gpu_strerror(rc).decode() == EINVAL
    with pytest.raises(BpeError, match=EINVAL) as e:
        api.pack_stream_host(ids, [0, 4, 9], 4, PAD)
    assert "text_off" in str(e.value)
    rc, _, _ = c_call(ids, off, None)
    assert _lib.load().bpe_gpu_strerror(rc).decode() == EINVAL


def test_refusals_name_the_field():
    for call, code, word in ((lambda: api.check_stream(0, PAD), EINVAL, "stream: seq_len is 0"),
                             (lambda: api.check_stream((1 << 24) + 1, PAD), ERANGE, "stream: seq_len 16777217 above 2^24"),
                             (lambda: api.check_stream(8, PAD, flags=8), EINVAL, "stream: flags 0x8"),
                             (lambda: api.check_stream(8, PAD, flags=0x80000001), EINVAL, "stream: flags 0x80000001"),
                             (lambda: api.pack_stream_host([1], [0, 1], 0, PAD), EINVAL, "seq_len is 0"),
                             (lambda: api.pack_stream_host([1], [0, 1], 1 << 25, PAD), ERANGE, "above 2^24")):
        with pytest.raises(BpeError, match=code) as e:
            call()
        assert word in str(e.value)
    with pytest.raises(BpeError, match="uint32"):
        api.check_stream(8, 1 << 32)
    with pytest.raises(BpeError, match="uint32"):
        api.check_stream(8, 0, bos_id=-1)
    L = _lib.load()
    assert L.bpe_gpu_strerror(L.bpe_stream_check(None, None, 0)).decode() == EINVAL
    s = _lib.Stream(0, 0, 0, 0, 0)
    tiny = ctypes.create_string_buffer(12)
    assert L.bpe_gpu_strerror(L.bpe_stream_check(ctypes.byref(s), tiny, len(tiny))).decode() == EINVAL
    assert tiny.value == b"stream: seq"  # cut to its room
    ok = api.check_stream(1 << 24, 5, 6, 7, True)
    assert (ok.seq_len, ok.flags, ok.bos_id, ok.eos_id, ok.pad_id) == (1 << 24, 7, 6, 7, 5)
    assert api.check_stream(1, 0).flags == 0 and api.check_stream(1, 0, bos_id=0).flags == 1  # (id 0 is a BOS all the same)


def test_stream_info():
    info = api.stream_info()
    assert info == {"per_thread": 4, "per_block": 1024, "per_grid": 1 << 21, "walk": info["walk"]}
    assert 1 <= info["walk"] <= 64
    assert _lib.load().bpe_gpu_strerror(_lib.load().bpe_gpu_stream_info(None)).decode() == EINVAL

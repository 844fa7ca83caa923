"""Packed streams on the device (stream.hip, bpe_gpu_pack_stream / _stream_info, Engine.stream_rows / pack_stream,
Tokenizer.encode_packed).  The expectation is always tests/stream_ref.py (the contract in plain Python) over
Engine.ids() and Engine.text_offsets() of the same batch, so it does not depend on how the ids arose: the matrix of row
lengths, BOS / EOS combinations, drop_last and text lengths before and after map_ids, text starts around every step of
the kernel (a lane's cells, a wave's, a workgroup's tile, a row edge, the edge between two workgroups, the cell count
past which a workgroup takes several tiles), empty texts, many tiny texts, both
variants of the kernel through torch tensors, the refusals by code and message, Tokenizer.encode_packed against a loop
of Tokenizer.encode, and the kernels' scratch size."""
import ctypes
import importlib.util
import json
import os
import re

import numpy as np
import pytest

import golden_lib as G
import stream_ref as SR
from llmtokenizer_amd import _lib, api
from llmtokenizer_amd.api import BpeError
from llmtokenizer_amd.synth import english_like
from llmtokenizer_amd.vocab import Tokenizer, Vocab

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ESTATE, EINVAL, ERANGE = "call out of order", "invalid argument", "out of range"
PAD = 0xFFFFFFFF
BOS, EOS = SR.BOS_EOS[3]
# cells per lane and per workgroup step of k_pack_stream<true> and the cells its largest grid takes in one step:
# api.stream_info(), held to these by test_stream_info (the library is not loaded while pytest collects); the one-cell
# variant takes a quarter of each
TH, WG, GR = 4, 1024, 1 << 21
# one merge of two bytes that no text here holds: every byte stays one id, so a text's id count is its byte count
MERGES = np.array([[0xF0, 0xF1]], dtype=np.uint32)
ALPHA = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz    ", dtype=np.uint8)


@pytest.fixture(scope="module")
def eng():
    e = api.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def voc():
    """shuffled ids with holes for the one-merge list, no specials"""
    ids = np.random.default_rng(21).permutation(60000)[:257]
    return Vocab(MERGES, ids[:256], ids[256:], [], [], "words")


def load_lengths(eng, lens, seed=3, vocab=None):
    """a resident text batch whose texts have exactly lens ids; returns (ids, text_off)"""
    off = SR.offsets(lens)
    data = np.random.default_rng(seed).choice(ALPHA, int(off[-1])).tobytes()
    eng.load_texts(data, offsets=off)
    eng.split("words")
    eng.encode_split(MERGES)
    if vocab is not None:
        eng.map_ids(vocab)
    toff = eng.text_offsets()
    assert np.array_equal(toff, off)
    return eng.ids(), toff


def check(eng, ids, toff, L, bos, eos, drop=False, pad=PAD):
    """rows, seg and pos of the resident batch, cell for cell, with every choice of the optional outputs"""
    want = SR.pack_stream(ids, toff, L, pad, bos, eos, drop)
    assert eng.stream_rows(L, bos, eos, drop) == (want[0].shape[0], want[3])
    got = eng.pack_stream(L, pad, bos, eos, drop, segments=True, positions=True)
    for g, w, name in zip(got, want[:3], ("rows", "seg", "pos")):
        assert g.dtype == np.uint32 and g.shape == w.shape, name
        assert np.array_equal(g, w), (name, L, bos, eos, drop, np.flatnonzero(g.reshape(-1) != w.reshape(-1))[:5])
    return got


def test_stream_info():
    assert api.stream_info() == {"per_thread": TH, "per_block": WG, "per_grid": GR, "walk": api.stream_info()["walk"]}


# ---------------------------------------------------------------- the matrix

@pytest.mark.parametrize("mapped", [False, True], ids=["internal", "mapped"])
@pytest.mark.parametrize("L", [1, 3, 4, 5, 64, 257])
def test_matrix_equals_the_reference(eng, voc, L, mapped):
    ids, toff = load_lengths(eng, SR.matrix_lengths(L, seed=L), seed=L, vocab=voc if mapped else None)
    assert (ids.max() > 255) == mapped
    for bos, eos in SR.BOS_EOS:
        for drop in (False, True):
            check(eng, ids, toff, L, bos, eos, drop)
    # the optional outputs one by one
    want = SR.pack_stream(ids, toff, L, 7, BOS, EOS)
    rows = eng.pack_stream(L, 7, BOS, EOS)
    assert isinstance(rows, np.ndarray) and np.array_equal(rows, want[0])
    rows, seg = eng.pack_stream(L, 7, BOS, EOS, segments=True)
    assert np.array_equal(rows, want[0]) and np.array_equal(seg, want[1])
    rows, pos = eng.pack_stream(L, 7, BOS, EOS, positions=True)
    assert np.array_equal(rows, want[0]) and np.array_equal(pos, want[2])


# ---------------------------------------------------------------- text starts around the kernel's steps

def lengths_for_starts(starts, w, last):
    """text lengths that put the texts' first cells at the stream positions `starts` (rising from 0), each text
    wrapped in w cells"""
    starts = sorted(set(starts))
    assert starts[0] == 0 and min(np.diff(starts)) >= w
    return [b - a - w for a, b in zip(starts, starts[1:])] + [last]


@pytest.mark.parametrize("d", range(-5, 6))
def test_text_starts_around_every_step(eng, d):
    """a text's first cell at d of a lane's four cells, of a wave's 256 (64 in the one-cell variant), of a workgroup's
    1,024 (256), of a row edge, of the edge between two workgroups' cells and of the cell count past which a workgroup
    takes more than one step (2^21, 2^19 in the one-cell variant), in a batch a little longer than that"""
    last = 777
    marks = [TH * 10, 64 * 3, 256 * 3, WG * 3, WG * 5 + TH * 7, 64 * 100, 5 * 2001, 256 * 64, GR // 4, GR // 4 + WG * 3, GR]
    for L, bos, eos in ((64, None, None), (64, BOS, EOS), (5, BOS, None)):
        w = (bos is not None) + (eos is not None)
        # the cells of one workgroup, from the launch's arithmetic (bpe_gpu.h, bpe_gpu_stream_info)
        tile = WG if L % 4 == 0 else WG // 4
        cells = -(-(GR + d + w + last) // L) * L
        span = -(-(-(-cells // tile)) // (GR // WG)) * tile
        assert span > tile  # (more than one step: a lane carries its text from one step to the next)
        starts = sorted({0} | {m + d for m in marks + [span * 3, span * 7 + tile, span * 100]})
        ids, toff = load_lengths(eng, lengths_for_starts(starts, w, last), seed=d + 10)
        rows, seg, pos = check(eng, ids, toff, L, bos, eos)
        assert rows.size == cells
        flat_seg, flat_pos = seg.reshape(-1), pos.reshape(-1)
        for k, s in enumerate(starts):  # (the starts are where they were meant to be)
            assert flat_seg[s] == k and flat_pos[s] == 0 and (s == 0 or flat_seg[s - 1] == k - 1)


def test_one_text_longer_than_a_grid_step(eng):
    ids, toff = load_lengths(eng, [3, 0, GR + 1000, 1, 0, 40], seed=8)
    for L, bos, eos in ((64, BOS, EOS), (2048, None, EOS), (3, None, None)):
        rows, seg, pos = check(eng, ids, toff, L, bos, eos)
        assert (seg[5] == 2).all() and (pos[5] == np.arange(L)).all()  # a row inside the long text counts from 0


# ---------------------------------------------------------------- empty texts

@pytest.mark.parametrize("bos,eos", [(None, None), (BOS, EOS)], ids=["plain", "bos_eos"])
def test_empty_texts(eng, bos, eos):
    w = (bos is not None) + (eos is not None)
    for wave in (256, 64):  # a wave's cells in the four-cell and in the one-cell variant
        for L in (64, 3):
            # three empty texts whose cells (or, without BOS / EOS, whose equal starts) sit at a wave's first cell
            ids, toff = load_lengths(eng, [wave - w, 0, 0, 0, 300, 0])
            rows, seg, pos = check(eng, ids, toff, L, bos, eos)
            assert seg.reshape(-1)[wave] == (1 if w else 4)
            check(eng, ids, toff, L, bos, eos, drop=True)
    # empties first and last, and runs of them longer than a lane walks
    walk = api.stream_info()["walk"]
    lens = [0, 0, 5, 0, 9] + [0] * (walk + 3) + [70] + [0] * (3 * walk) + [1, 0, 0]
    ids, toff = load_lengths(eng, lens)
    for L in (4, 5, 64):
        check(eng, ids, toff, L, bos, eos)
    # all texts empty
    ids, toff = load_lengths(eng, [0] * 300)
    assert ids.size == 0
    for L in (4, 5):
        rows, seg, pos = check(eng, ids, toff, L, bos, eos)
        assert rows.shape == (-(-300 * w // L), L)
        if w:
            assert rows.reshape(-1)[:600].tolist() == [BOS, EOS] * 300 and (seg.reshape(-1)[:600:2] == np.arange(300)).all()
    # no text
    ids, toff = load_lengths(eng, [])
    assert eng.stream_rows(8, bos, eos) == (0, 0)
    rows, seg, pos = check(eng, ids, toff, 8, bos, eos)
    assert rows.shape == (0, 8)


# ---------------------------------------------------------------- many tiny texts

@pytest.mark.parametrize("bos,eos", [(None, None), (BOS, EOS)], ids=["plain", "bos_eos"])
def test_one_id_texts_every_lane_searches(eng, bos, eos):
    """70,000 texts of one id: a wave's cells lie in far more texts than a lane walks, so every lane searches"""
    ids, toff = load_lengths(eng, [1] * 70000)
    for L in (64, 5):
        rows, seg, pos = check(eng, ids, toff, L, bos, eos)
    if bos is None:
        assert (seg.reshape(-1)[:70000] == np.arange(70000)).all() and not pos.any()


# ---------------------------------------------------------------- both variants through torch tensors

def test_torch_outputs_take_both_variants(eng):
    import torch
    dev = torch.device("cuda", 0)
    L = 64
    ids, toff = load_lengths(eng, SR.matrix_lengths(L, seed=2, copies=8))
    want = SR.pack_stream(ids, toff, L, 5, BOS, EOS)
    R = want[0].shape[0]
    assert eng.stream_rows(L, BOS, EOS) == (R, want[3])
    # 16-byte aligned tensors: four cells per lane
    out = tuple(torch.full((R, L), -7, dtype=torch.int32, device=dev) for _ in range(3))
    assert all(t.data_ptr() % 16 == 0 for t in out)
    got = eng.pack_stream(L, 5, BOS, EOS, out=out)
    assert all(g is o for g, o in zip(got, out))
    for t, w in zip(out, want[:3]):
        assert np.array_equal(t.cpu().numpy().view(np.uint32), w)
    # rows alone, and rows with one of the two
    for pick in ((1, 0, 0), (1, 1, 0), (1, 0, 1)):
        out = tuple(torch.full((R, L), -7, dtype=torch.int32, device=dev) if p else None for p in pick)
        got = eng.pack_stream(L, 5, BOS, EOS, out=out)
        for t, w in zip(got, want[:3]):
            assert t is None or np.array_equal(t.cpu().numpy().view(np.uint32), w)
    # tensors that are only 4-byte aligned (each one in turn): one cell per lane at a row length the other variant takes
    for odd_one in range(3):
        flats = [torch.full((R * L + 1,), -7, dtype=torch.int32, device=dev) for _ in range(3)]
        out = tuple(f[1:].view(R, L) if j == odd_one else f[:-1].view(R, L) for j, f in enumerate(flats))
        assert out[odd_one].data_ptr() % 16 == 4 and all(t.is_contiguous() for t in out)
        eng.pack_stream(L, 5, BOS, EOS, out=out)
        for j, (t, f, w) in enumerate(zip(out, flats, want[:3])):
            assert np.array_equal(t.cpu().numpy().view(np.uint32), w)
            assert int(f[0 if j == odd_one else -1]) == -7  # (the cell beside the tensor is untouched)


# ---------------------------------------------------------------- drop_last

def test_drop_last(eng):
    import torch
    ids, toff = load_lengths(eng, [5, 0, 7, 12])  # 24 ids; with BOS and EOS 32 cells
    # N < L: no row, and nothing is written
    assert eng.stream_rows(64, BOS, EOS, drop_last=True) == (0, 32)
    rows, seg, pos = check(eng, ids, toff, 64, BOS, EOS, drop=True)
    assert rows.shape == (0, 64)
    guard = torch.full((1, 64), -7, dtype=torch.int32, device="cuda:0")
    rc = eng.L.bpe_gpu_pack_stream(eng.ctx, ctypes.byref(api.check_stream(64, 1, BOS, EOS, True)),
                                   ctypes.c_void_p(guard.data_ptr()), None, None, 1, 1, None, None)
    assert rc == 0 and bool((guard == -7).all())
    out = (torch.empty((0, 64), dtype=torch.int32, device="cuda:0"), None, None)
    assert eng.pack_stream(64, 1, BOS, EOS, True, out=out)[0] is out[0]
    # N == R L: the same with and without
    for L, bos, eos in ((8, BOS, EOS), (4, None, None), (3, None, None), (7, BOS, None)):
        a, b = check(eng, ids, toff, L, bos, eos, drop=False), check(eng, ids, toff, L, bos, eos, drop=True)
        assert a[0].shape[0] * L == 24 + 4 * ((bos is not None) + (eos is not None))
        assert all(np.array_equal(x, y) for x, y in zip(a, b)) and (a[1] != SR.NO_TEXT).all()
    # N == R L + 1: one row less
    ids, toff = load_lengths(eng, [5, 0, 7, 13])
    assert check(eng, ids, toff, 8, None, None, drop=True)[0].shape == (3, 8)
    assert check(eng, ids, toff, 8, None, None, drop=False)[0].shape == (4, 8)


# ---------------------------------------------------------------- refusals

def refused(eng, call, code, word):
    with pytest.raises(BpeError, match=code) as e:
        call()
    assert word in str(e.value), str(e.value)


def c_pack(eng, s, rows, seg=None, pos=None, dev=1, cap=0):
    """bpe_gpu_pack_stream as it is; returns (the code's text or None, the message)"""
    vp = ctypes.c_void_p
    rc = eng.L.bpe_gpu_pack_stream(eng.ctx, ctypes.byref(s), vp(rows) if rows else None, vp(seg) if seg else None,
                                   vp(pos) if pos else None, dev, cap, None, None)
    return (eng.L.bpe_gpu_strerror(rc).decode(), eng.L.bpe_gpu_last_error().decode()) if rc else (None, "")


def test_refusals_and_the_engine_goes_on(eng):
    import torch
    dev = torch.device("cuda", 0)
    fresh = api.Engine(0)
    try:
        refused(fresh, lambda: fresh.pack_stream(8, PAD), ESTATE, "no text batch")
        refused(fresh, lambda: fresh.stream_rows(8), ESTATE, "no text batch")
    finally:
        fresh.close()
    lens = [5, 0, 7, 12]
    off = SR.offsets(lens)
    data = np.random.default_rng(1).choice(ALPHA, 24).tobytes()
    eng.load_texts(data, offsets=off)
    refused(eng, lambda: eng.pack_stream(8, PAD), ESTATE, "encode_split first")
    eng.split("words")
    refused(eng, lambda: eng.pack_stream(8, PAD), ESTATE, "encode_split first")
    eng.encode_split(MERGES)
    ids, toff = eng.ids(), eng.text_offsets()

    def still_works():
        check(eng, ids, toff, 8, BOS, EOS)

    still_works()
    for call, code, word in ((lambda: eng.pack_stream(0, PAD), EINVAL, "seq_len is 0"),
                             (lambda: eng.stream_rows(0), EINVAL, "seq_len is 0"),
                             (lambda: eng.pack_stream((1 << 24) + 1, PAD), ERANGE, "above 2^24"),
                             (lambda: eng.pack_stream(8, 1 << 32), "uint32", "uint32")):
        refused(eng, call, code, word)
        still_works()
    # the C entry point as it is: a flag bit, too little room, pointers that are not the device's or not aligned
    good = api.check_stream(8, PAD, BOS, EOS)  # 4 rows
    buf = torch.full((3 * 4 * 8 + 4,), -7, dtype=torch.int32, device=dev)
    p = buf.data_ptr()
    host = np.zeros(4 * 8, dtype=np.uint32)
    cases = [(_lib.Stream(8, 8, 0, 0, 0), p, None, None, 1, 4, EINVAL, "flags 0x8"),
             (_lib.Stream(0, 0, 0, 0, 0), p, None, None, 1, 4, EINVAL, "seq_len is 0"),
             (_lib.Stream((1 << 24) + 1, 0, 0, 0, 0), p, None, None, 1, 4, ERANGE, "above 2^24"),
             (good, p, None, None, 1, 3, EINVAL, "rows_cap 3 is below the 4 rows"),
             (good, host.ctypes.data, None, None, 0, 3, EINVAL, "rows_cap 3 is below the 4 rows"),
             (good, host.ctypes.data, None, None, 1, 4, EINVAL, "no device pointer of the context's device"),
             (good, p, host.ctypes.data, None, 1, 4, EINVAL, "no device pointer of the context's device"),
             (good, p, None, host.ctypes.data, 1, 4, EINVAL, "no device pointer of the context's device"),
             (good, p + 2, None, None, 1, 4, EINVAL, "not 4-byte aligned"),
             (good, p, p + 4 * 32 + 1, None, 1, 4, EINVAL, "not 4-byte aligned"),
             (good, p, None, p + 4 * 64 + 3, 1, 4, EINVAL, "not 4-byte aligned")]
    for s, rows, seg, pos, is_dev, cap, code, word in cases:
        got = c_pack(eng, s, rows, seg, pos, is_dev, cap)
        assert got[0].startswith(code) and word in got[1], (got, word)
        assert bool((buf == -7).all()) and not host.any()  # nothing was written
        still_works()
    assert c_pack(eng, good, p, p + 4 * 32, p + 4 * 64, 1, 4) == (None, "")
    want = SR.pack_stream(ids, toff, 8, PAD, BOS, EOS)
    got = buf.cpu().numpy().view(np.uint32)
    assert all(np.array_equal(got[32 * j:32 * j + 32].reshape(4, 8), want[j]) for j in range(3)) and (got[96:] == 0xFFFFFFF9).all()
    if torch.cuda.device_count() > 1:  # a tensor of another device
        other = torch.zeros((4, 8), dtype=torch.int32, device="cuda:1")
        refused(eng, lambda: eng.pack_stream(8, PAD, BOS, EOS, out=(other, None, None)), EINVAL, "no device pointer")
        still_works()
    # out= with a wrong shape, dtype or device, or not the triple
    ok = lambda: torch.zeros((4, 8), dtype=torch.int32, device=dev)  # noqa: E731
    for bad in ((torch.zeros((4, 8), dtype=torch.int32), None, None), (torch.zeros((5, 8), dtype=torch.int32, device=dev), None, None),
                (torch.zeros((4, 9), dtype=torch.int32, device=dev), None, None),
                (torch.zeros((4, 8), dtype=torch.float32, device=dev), None, None),
                (torch.zeros((4, 8), dtype=torch.int64, device=dev), None, None),
                (torch.zeros((4, 16), dtype=torch.int32, device=dev)[:, ::2], None, None),
                (ok(), torch.zeros((4, 8), dtype=torch.int32), None), (ok(), None, torch.zeros((3, 8), dtype=torch.int32, device=dev)),
                (ok(), None, np.zeros((4, 8), dtype=np.uint32)), (None, ok(), ok()), (ok(), ok()), ok()):
        refused(eng, lambda: eng.pack_stream(8, PAD, BOS, EOS, out=bad), "pack_stream: out must", "out must")
        still_works()
    # a load ends the batch
    eng.load(data)
    refused(eng, lambda: eng.pack_stream(8, PAD), ESTATE, "no text batch")
    ids, toff = load_lengths(eng, lens)
    still_works()


# ---------------------------------------------------------------- Tokenizer.encode_packed

EOT, IMS = "<|endoftext|>", "<|im_start|>"


@pytest.fixture(scope="module")
def tok(tmp_path_factory):
    with open(os.path.join(G.GOLD, "vocab", "vocab_cl100k.json"), encoding="utf-8") as f:
        fx = json.load(f)
    p = tmp_path_factory.mktemp("vocab") / "tokenizer.json"
    p.write_text(json.dumps(fx["tokenizer_json"], ensure_ascii=False), encoding="utf-8")
    v = Vocab.from_tokenizer_json(p)
    assert v.specials == [EOT.encode(), IMS.encode()]
    t = Tokenizer(v)
    yield t
    t.close()


def test_encode_packed(tok):
    import torch
    src = english_like(6000) + " 12345 it's \n\n \té€😀 ".encode("utf-8") * 3
    cuts = [0, 0, 700, 701, 701, 2500, 2503, 5000, len(src), len(src)]
    texts = [src[a:b] for a, b in zip(cuts, cuts[1:])]
    v = tok.vocab
    eos_id, ims_id = int(v.special_ids[0]), int(v.special_ids[1])
    single = [tok.encode(t).tolist() if t else [] for t in texts]
    L = 32
    rows, N = tok.encode_packed(texts, L, PAD, bos=None, eos=EOT)
    want = [i for x in single for i in x + [eos_id]]
    assert rows.dtype == np.uint32 and rows.shape == (-(-len(want) // L), L) and N == len(want)
    assert rows.reshape(-1)[:N].tolist() == want and (rows.reshape(-1)[N:] == PAD).all()
    # cut at the EOS id and decoded, the rows give back the texts
    flat, back, at = rows.reshape(-1)[:N], [], 0
    for end in np.flatnonzero(flat == eos_id).tolist():
        back.append(tok.decode(flat[at:end]) if end > at else b"")
        at = end + 1
    assert back == texts
    # the segments and positions are the reference's over the batch's own ids
    ids, toff = tok.encode_batch(texts)
    for drop in (False, True):
        got = tok.encode_packed(texts, L, PAD, bos=IMS, eos=EOT, drop_last=drop, return_segments=True, return_positions=True)
        ref = SR.pack_stream(ids, toff, L, PAD, ims_id, eos_id, drop)
        assert len(got) == 4 and got[3] == ref[3] and all(np.array_equal(g, w) for g, w in zip(got[:3], ref[:3]))
    # a BOS as an int and as a name (str or bytes) agree
    by_name = tok.encode_packed(texts, L, 0, bos=IMS, eos=EOT.encode(), return_positions=True)
    by_id = tok.encode_packed(texts, L, 0, bos=ims_id, eos=eos_id, return_positions=True)
    assert len(by_name) == 3 and by_name[2] == by_id[2] and all(np.array_equal(a, b) for a, b in zip(by_name[:2], by_id[:2]))
    assert by_name[0][0, 0] == ims_id
    for kw in ({"bos": "<|nope|>"}, {"eos": b"<|im_end|>"}):
        with pytest.raises(BpeError, match=re.escape(repr(list(kw.values())[0]))):
            tok.encode_packed(texts, L, 0, **kw)
    with pytest.raises(BpeError, match="return_tensors"):
        tok.encode_packed(texts, L, 0, return_tensors="np")
    with pytest.raises(BpeError, match="seq_len is 0"):
        tok.encode_packed(texts, 0, 0)
    # torch tensors, filled on the device
    want = tok.encode_packed(texts, L, 3, bos=IMS, eos=EOT, return_segments=True, return_positions=True)
    got = tok.encode_packed(texts, L, 3, bos=IMS, eos=EOT, return_segments=True, return_positions=True, return_tensors="pt")
    assert len(got) == 4 and got[3] == want[3]
    for t, w in zip(got[:3], want[:3]):
        assert t.dtype == torch.int32 and t.device == torch.device("cuda", 0) and tuple(t.shape) == w.shape
        assert np.array_equal(t.cpu().numpy().view(np.uint32), w)
    rows_pt, n_pt = tok.encode_packed(texts, L, 3, eos=EOT, drop_last=True, return_tensors="pt")
    assert n_pt == N and np.array_equal(rows_pt.cpu().numpy().view(np.uint32), rows[:N // L])
    assert got[3] % L == 0 or int(got[1][-1, -1]) == -1  # (a pad cell's seg as int32)


# ---------------------------------------------------------------- scratch

def test_both_variants_have_no_scratch_segment():
    spec = importlib.util.spec_from_file_location("kernel_scratch", os.path.join(ROOT, "tools", "kernel_scratch.py"))
    ks = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ks)
    kd = ks.scan(os.environ.get("BPE_LIB") or os.path.join(ROOT, "llmtokenizer_amd", "libbpe_amd.so"))
    found = {name: scratch for name, (lds, scratch) in kd.items() if re.search(r"\dk_pack_streamI", name)}
    assert len(found) == 2 and {("Lb1E" in n) for n in found} == {True, False}, sorted(found)
    assert all(v == 0 for v in found.values()), found

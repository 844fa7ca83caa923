"""Rows back to texts on the device (llmtokenizer_amd/csrc/rows.hip; the contract: include/bpe_gpu.h): Engine.unpack_rows
cell for cell against the plain-Python statement of the contract (tests/rows_ref.py) on ids, text_off and bounds, over
a matrix of shapes and options, with the starts and ends of the texts around every step of the kernels, through torch
tensors that take either kernel variant, past the largest grid, with cells that must not be judged and cells that must,
the refusals, the independence from the resident ids of an encode, Tokenizer.decode_rows' round trips, and the kernels'
scratch size.  The bytes are held to the existing decoders (decode_docs / decode_batch) run over the reference's ids.

The issue's "cells that must not be judged ... inside the leading pad" has no instance under its own contract: the
leading pad is by definition the cells equal to pad_id, so any other value there ends it and begins the text.  Such
cells sit behind the stop and behind the window (lens) here, the two places a foreign value can be."""
import ctypes
import importlib.util
import itertools
import json
import os
import re

import numpy as np
import pytest

import golden_lib as G
import rows_ref as RR
from llmtokenizer_amd import _lib, api
from llmtokenizer_amd.api import BpeError
from llmtokenizer_amd.synth import english_like
from llmtokenizer_amd.vocab import Tokenizer, Vocab

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ESTATE, EINVAL, EDATA = "call out of order", "invalid argument", "unknown token id or corrupt merge list"
# cells per lane and per wave step of the vector variants, rows per workgroup and rows of the largest grid's one step:
# api.rows_info(), held to these by test_rows_info (the library is not loaded while pytest collects); the one-cell
# variants take a quarter of the first two
PER, WAVE, RPW, RPG = 4, 256, 4, 8192
PAD, STOP = 3, 7
SKIPS = [250, 5, 251, 5, 255, 31]  # unsorted, with a duplicate
# one merge of two bytes: the internal ids are 0 .. 256
MERGES = np.array([[0xF0, 0xF1]], dtype=np.uint32)
DTYPES = {4: np.uint32, 8: np.int64}


@pytest.fixture(scope="module")
def eng():
    e = api.Engine(0)
    yield e
    e.close()


def same(got, want, note=None):
    for g, w, name in zip(got, want, ("ids", "text_off", "bounds")):
        assert g.dtype == w.dtype and g.shape == w.shape, (name, note, g.shape, w.shape)
        assert np.array_equal(g, w), (name, note, np.flatnonzero(g.reshape(-1) != w.reshape(-1))[:5])


def decoded(eng, want):
    """decode_rows of the last unpack against decode_docs over the reference's ids"""
    got, off = eng.decode_rows(MERGES)
    ref, ref_off = eng.decode_docs(want[0], want[1], MERGES)
    assert got == ref and np.array_equal(off, ref_off)


def refused(call, code, word):
    with pytest.raises(BpeError) as e:
        call()
    assert code in str(e.value) and word in str(e.value), str(e.value)


def test_rows_info():
    assert api.rows_info() == {"per_lane": PER, "per_wave": WAVE, "rows_per_block": RPW, "rows_per_grid": RPG}


# ---------------------------------------------------------------- the matrix

@pytest.mark.parametrize("cell_bytes", [4, 8])
@pytest.mark.parametrize("L", [0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1029])
def test_matrix_equals_the_reference(eng, L, cell_bytes):
    rng = np.random.default_rng(1000 * L + cell_bytes)
    for B, pad_on, lens_on, skip_on in itertools.product((0, 1, 4, 5, 67), (False, True), (False, True), (False, True)):
        pad = PAD if pad_on else None
        stops = [STOP, 11] + ([PAD] if pad_on else [])  # (pad_id == a stop)
        skip = SKIPS if skip_on else None
        rows = RR.batch(rng, B, L, DTYPES[cell_bytes], pad, stops, skip, vocab=257)
        lens = rng.integers(0, L + 1, B).astype(np.uint32) if lens_on else None
        want = RR.unpack(rows, lens, pad, stops, skip)
        same(eng.unpack_rows(rows, lens, pad, stops, skip), want, (B, pad_on, lens_on, skip_on))
        if B == 67 and not skip_on:
            decoded(eng, want)
        if B == 5:  # host rows that lie in a wider array: the upload honours row_stride
            wide = np.concatenate([rows[:, ::-1], rows, rows[:, :3]], axis=1)
            assert L == 0 or wide[:, L:2 * L].strides[0] > L * cell_bytes
            same(eng.unpack_rows(wide[:, L:2 * L], lens, pad, stops, skip), want, ("wide", pad_on, lens_on, skip_on))


# ---------------------------------------------------------------- starts and ends around the kernels' steps

@pytest.mark.parametrize("L", [520, 521], ids=["vector", "one-cell"])
@pytest.mark.parametrize("cell_bytes", [4, 8])
def test_starts_and_ends_around_every_step(eng, L, cell_bytes):
    """a_k and z_k at d = -2 .. 2 around a lane's four cells, a wave step of either variant (64, 256) and two of them
    (128, 512), with skipped ids on both sides of each edge: a wrong carry of the rank from step to step, or a wrong
    rank inside a step, moves an id"""
    rng = np.random.default_rng(L)
    plain = np.array([x for x in range(257) if x not in (PAD, STOP) and x not in SKIPS], dtype=np.int64)
    rows, lens = [], []
    for mark, d in itertools.product((8, 64, 128, 256, 512), range(-2, 3)):
        e = mark + d
        for a, z in ((e, L), (0, e), (e, min(e + 70, L)), (max(e - 70, 0), e), (e, e), (e, e + 1)):
            row = rng.choice(plain, L)
            row[:a] = PAD
            for c in (a, a + 1, a + 3, z - 1, z - 2, z - 4, (a + z) // 2):
                if a <= c < z:
                    row[c] = SKIPS[c % len(SKIPS)]
            row[z:] = rng.choice(np.array(SKIPS + [STOP, PAD, 9], dtype=np.int64), L - z)  # behind the end: anything
            if z < L:
                row[z] = STOP if (a + z) % 2 else PAD
            rows.append(row)
            lens.append(L if z < L or (mark + d) % 2 else z)
    rows = np.array(rows).astype(DTYPES[cell_bytes])
    for lens_on, skip_on in itertools.product((False, True), (False, True)):
        ln = np.array(lens, dtype=np.uint32) if lens_on else None
        skip = SKIPS if skip_on else None
        want = RR.unpack(rows, ln, PAD, [STOP], skip)
        same(eng.unpack_rows(rows, ln, PAD, [STOP], skip), want, (lens_on, skip_on))
    assert len({tuple(b) for b in want[2].tolist()}) > 100


# ---------------------------------------------------------------- both variants through torch tensors

@pytest.mark.parametrize("dtype", ["int32", "int64"])
def test_torch_tensors_take_both_variants(eng, dtype):
    import torch
    dev = torch.device("cuda", 0)
    tdt = getattr(torch, dtype)
    rng = np.random.default_rng(7)
    B, L, P = 37, 264, 8
    data = RR.batch(rng, B, L, np.dtype(dtype), PAD, [STOP], SKIPS, vocab=257)
    want = RR.unpack(data, None, PAD, [STOP], SKIPS)
    args = (None, PAD, [STOP], SKIPS)
    # contiguous, L a multiple of 4: four cells per lane
    t = torch.from_numpy(data).to(dev)
    assert t.data_ptr() % 16 == 0 and t.is_contiguous()
    same(eng.unpack_rows(t, *args), want, "contiguous")
    # t[:, 1:]: the first cell is not 16-byte aligned; and an odd L: a cell per lane
    wide = torch.full((B, L + 1), STOP, dtype=tdt, device=dev)
    wide[:, 1:] = t
    assert wide[:, 1:].data_ptr() % 16 != 0
    same(eng.unpack_rows(wide[:, 1:], *args), want, "t[:, 1:]")
    same(eng.unpack_rows(t[:, :L - 1], *args), RR.unpack(data[:, :L - 1], None, PAD, [STOP], SKIPS), "odd L")
    # t[:, P:], P a multiple of 4: four cells per lane again, with row_stride > L
    wide = torch.full((B, P + L), 9, dtype=tdt, device=dev)
    wide[:, P:] = t
    view = wide[:, P:]
    assert view.data_ptr() % 16 == 0 and view.stride(0) == P + L and not view.is_contiguous()
    same(eng.unpack_rows(view, *args), want, "t[:, P:]")
    # lens as a tensor beside them
    lens = rng.integers(0, L + 1, B).astype(np.int32)
    want = RR.unpack(data, lens, PAD, [STOP], SKIPS)
    same(eng.unpack_rows(view, torch.from_numpy(lens).to(dev), PAD, [STOP], SKIPS), want, "lens tensor")
    same(eng.unpack_rows(view, lens, PAD, [STOP], SKIPS), want, "lens array")
    decoded(eng, want)
    assert int(wide[0, 0]) == 9  # (the tensor is read, never written)


# ---------------------------------------------------------------- more rows than the largest grid takes in one step

@pytest.mark.parametrize("cell_bytes", [4, 8])
def test_grid_stride(eng, cell_bytes):
    B, L = 2 * RPG + 3, 8
    k = np.arange(B)
    a, z = k % (L + 1), (k // (L + 1)) % (L + 1)
    z = np.maximum(a, z)
    col = np.arange(L)[None, :]
    rows = 20 + (k[:, None] * 7 + col) % 200  # no 3, no 7
    rows = np.where(col < a[:, None], PAD, rows)
    rows = np.where(col == z[:, None], STOP, rows).astype(DTYPES[cell_bytes])
    want = RR.unpack(rows, None, PAD, [STOP])
    assert np.array_equal(want[2], np.stack([a, z], axis=1))
    same(eng.unpack_rows(rows, None, PAD, [STOP]), want)
    decoded(eng, want)


# ---------------------------------------------------------------- cells that must not be judged, and cells that must

def test_cells_outside_the_text_are_never_judged(eng):
    import torch
    rows = np.full((6, 12), 65, dtype=np.int64)
    rows[:, :2] = PAD
    rows[:, 8] = STOP
    rows[0, 9:] = [-100, 1 << 40, 9999]  # behind the stop: an ignore index, no id at all, an id no list holds
    rows[1, 9:] = [1 << 32, -1, 257]
    lens = np.array([12, 12, 12, 5, 12, 12], dtype=np.uint32)
    rows[3, 5:] = [-100, 1 << 40, 9999, 1 << 63 - 1, -(1 << 63), 300, 4000]  # behind the window
    want = RR.unpack(rows, lens, PAD, [STOP])
    for r in (rows, torch.from_numpy(rows).to("cuda:0")):
        same(eng.unpack_rows(r, lens, PAD, [STOP]), want)
        decoded(eng, want)
        assert eng.decode_rows(MERGES)[0] == b"A" * (6 * 5 + 3)
    # the same values inside [a, z): the unpack refuses what is no id and names the lowest row
    for bad in (-100, 1 << 40, 1 << 32, -1):
        r2 = rows.copy()
        r2[5, 7] = bad
        r2[2, 2] = bad
        with pytest.raises(RR.RowsError) as e:
            RR.unpack(r2, lens, PAD, [STOP])
        assert (e.value.code, e.value.row) == ("EDATA", 2)
        for r in (r2, torch.from_numpy(r2).to("cuda:0")):
            refused(lambda: eng.unpack_rows(r, lens, PAD, [STOP]), EDATA, "row 2 keeps a cell outside 0 .. 2^32 - 1")
            refused(lambda: eng.decode_rows(MERGES), ESTATE, "no rows")  # nothing is kept after a refusal
            refused(eng.fetch_rows, ESTATE, "no rows")
    # ... and an id no list holds passes the unpack and is the decoders' unknown token id
    r2 = rows.copy()
    r2[4, 4] = 9999
    same(eng.unpack_rows(r2, lens, PAD, [STOP]), RR.unpack(r2, lens, PAD, [STOP]))
    refused(lambda: eng.decode_rows(MERGES), EDATA, "unknown token id")
    r2[4, 4] = 257  # the first id past the list's
    eng.unpack_rows(r2, lens, PAD, [STOP])
    refused(lambda: eng.decode_rows(MERGES), EDATA, "unknown token id")
    # skipped, it never reaches the decoder
    skipped = RR.unpack(r2, lens, PAD, [STOP], [257])
    same(eng.unpack_rows(r2, lens, PAD, [STOP], [257]), skipped)
    decoded(eng, skipped)
    # the engine goes on
    same(eng.unpack_rows(rows, lens, PAD, [STOP]), want)
    decoded(eng, want)
    # 32-bit cells are ids whatever they hold
    r32 = np.array([[1, -1, -100, STOP, -5]], dtype=np.int32)
    same(eng.unpack_rows(r32, None, None, [STOP]), RR.unpack(r32, None, None, [STOP]))
    assert eng.fetch_rows()[0].tolist() == [1, 0xFFFFFFFF, 0xFFFFFF9C]


# ---------------------------------------------------------------- refusals

def c_unpack(eng, rows_ptr, is_dev, cb, B, L, stride, lens_ptr=None, lens_dev=0, desc=None):
    d = desc or api.check_rows(PAD, [STOP])
    vp = ctypes.c_void_p
    n = ctypes.c_size_t(0)
    rc = eng.L.bpe_gpu_unpack_rows(eng.ctx, vp(rows_ptr) if rows_ptr else None, is_dev, cb, B, L, stride,
                                   vp(lens_ptr) if lens_ptr else None, lens_dev, d.ref if hasattr(d, "ref") else ctypes.byref(d),
                                   ctypes.byref(n))
    return (eng.L.bpe_gpu_strerror(rc).decode(), eng.L.bpe_gpu_last_error().decode()) if rc else (None, "")


def test_refusals_and_the_engine_goes_on(eng):
    import torch
    dev = torch.device("cuda", 0)
    fresh = api.Engine(0)
    try:
        refused(lambda: fresh.decode_rows(MERGES), ESTATE, "bpe_gpu_unpack_rows first")
        refused(fresh.fetch_rows, ESTATE, "bpe_gpu_unpack_rows first")
    finally:
        fresh.close()
    rng = np.random.default_rng(2)
    data = RR.batch(rng, 9, 16, np.int64, PAD, [STOP], None, vocab=257)
    want = RR.unpack(data, None, PAD, [STOP])
    t = torch.from_numpy(data).to(dev)

    def still_works():
        same(eng.unpack_rows(t, None, PAD, [STOP]), want)
        decoded(eng, want)

    still_works()
    # a window above L: host and device lens, the lowest row named
    lens = np.array([16, 3, 0, 17, 16, 99, 16, 16, 16], dtype=np.int32)
    for ln in (lens, lens.astype(np.uint32), torch.from_numpy(lens).to(dev)):
        for r in (data, t):
            refused(lambda: eng.unpack_rows(r, ln, PAD, [STOP]), EINVAL, "lens[3] is 17, above the row length 16")
            refused(eng.fetch_rows, ESTATE, "no rows")
            still_works()
    # the C entry point as it is
    p = t.data_ptr()
    host = np.zeros(16, dtype=np.int64)
    l32 = torch.zeros(12, dtype=torch.int32, device=dev)
    stop8 = (ctypes.c_uint32 * 8)()
    cases = [((p + 4, 1, 8, 9, 16, 16), "rows is a device pointer that is not 8-byte aligned"),
             ((p + 2, 1, 4, 9, 16, 32), "rows is a device pointer that is not 4-byte aligned"),
             ((host.ctypes.data, 1, 8, 1, 16, 16), "rows is no device pointer of the context's device"),
             ((p, 1, 8, 9, 16, 16, l32.data_ptr() + 2, 1), "lens is a device pointer that is not 4-byte aligned"),
             ((p, 1, 8, 9, 16, 16, host.ctypes.data, 1), "lens is no device pointer of the context's device"),
             ((p, 1, 2, 9, 16, 16), "cell_bytes is neither 4 nor 8"),
             ((p, 1, 8, 9, 16, 15), "row_stride 15 below L 16"),
             ((None, 1, 8, 9, 16, 16), "rows is NULL"),
             ((p, 1, 8, 9, 16, 16, None, 0, _lib.Rows(4, 0, 0, stop8, 0, None)), "flags 0x4"),
             ((p, 1, 8, 9, 16, 16, None, 0, _lib.Rows(0, 0, 9, stop8, 0, None)), "n_stop 9 above 8"),
             ((p, 1, 8, 9, 16, 16, None, 0, _lib.Rows(2, 0, 0, stop8, 257, None)), "n_skip 257 above 256")]
    for args, word in cases:
        got = c_unpack(eng, *args)
        assert got[0] is not None and got[0].startswith(EINVAL) and word in got[1], (got, word)
        still_works()
    got = c_unpack(eng, p, 1, 8, 0, (1 << 24) + 1, 1 << 25)
    assert got[0].startswith("out of range") and "L above 2^24" in got[1], got
    assert c_unpack(eng, p, 1, 8, 9, 16, 16) == (None, "")
    same(eng.fetch_rows(), want)
    # tensors the Python layer does not take: 3-D, strided in the columns, rows that overlap, another dtype, the CPU
    for bad in (t.reshape(3, 3, 16), t[:, ::2], t.t(), t.to(torch.int16), t.to(torch.float32), t.cpu(), t[0],
                t[:1].expand(4, 16)):
        refused(lambda: eng.unpack_rows(bad, None, PAD, [STOP]), "unpack_rows: rows of shape", "pass a 2-D numpy array")
        still_works()
    refused(lambda: eng.unpack_rows(t.cpu(), None, PAD, [STOP]), "on cpu", "on the engine's device")
    for bad in (torch.zeros(9, dtype=torch.int64, device=dev), torch.zeros(8, dtype=torch.int32, device=dev),
                torch.zeros(9, dtype=torch.int32), torch.zeros(18, dtype=torch.int32, device=dev)[::2]):
        refused(lambda: eng.unpack_rows(t, bad, PAD, [STOP]), "unpack_rows: lens must be", "int32")
        still_works()
    if torch.cuda.device_count() > 1:  # a tensor of another device
        refused(lambda: eng.unpack_rows(t.to("cuda:1"), None, PAD, [STOP]), EINVAL, "no device pointer of the context's device")
        still_works()
    refused(lambda: eng.unpack_rows(t, None, PAD, range(9)), EINVAL, "n_stop 9 above 8")
    refused(lambda: eng.unpack_rows(t, None, PAD, [STOP], range(257)), EINVAL, "n_skip 257 above 256")
    still_works()


# ---------------------------------------------------------------- the resident ids of an encode and the rows: apart

def test_unpack_and_encode_do_not_disturb_each_other(eng):
    rng = np.random.default_rng(4)
    voc = Vocab(MERGES, np.arange(1000, 1256), np.array([77]), [], [], "words")
    texts = [bytes(rng.choice(np.frombuffer(b"abcdefgh  ", dtype=np.uint8), n)) for n in (40, 0, 700, 3)]

    def encode():
        eng.load_texts(texts)
        eng.split("words")
        eng.encode_split(MERGES)
        eng.map_ids(voc)
        return eng.ids(), eng.text_offsets(), eng.ids_checksum()

    ids, toff, chk = encode()
    rows = RR.batch(rng, 40, 300, np.int64, PAD, [STOP], SKIPS, vocab=257)
    want = RR.unpack(rows, None, PAD, [STOP], SKIPS)
    same(eng.unpack_rows(rows, None, PAD, [STOP], SKIPS), want)
    text = eng.decode_rows(MERGES)
    assert np.array_equal(eng.ids(), ids) and np.array_equal(eng.text_offsets(), toff) and eng.ids_checksum() == chk
    rows2, lens2 = eng.pack_texts(64, PAD)
    assert np.array_equal(rows2[0, :40], ids[:40]) and lens2.tolist() == [40, 0, 64, 3]
    # and the reverse: an encode, a decode of other ids and a pack leave the unpacked rows as they were
    ids2, toff2, chk2 = encode()
    assert np.array_equal(ids2, ids) and chk2 == chk
    eng.decode_docs(ids, toff, MERGES, vocab=voc)
    eng.pack_stream(32, PAD)
    same(eng.fetch_rows(), want)
    again = eng.decode_rows(MERGES)
    assert again[0] == text[0] and np.array_equal(again[1], text[1])
    decoded(eng, want)
    # the mapped rows of the encode, unpacked and decoded with the vocabulary, are the texts
    t_ids, t_off, t_b = eng.unpack_rows(rows2, lens2)
    assert np.array_equal(t_ids[:40], ids[:40]) and t_b.tolist() == [[0, 40], [0, 0], [0, 64], [0, 3]]
    out, bo = eng.decode_rows(MERGES, vocab=voc)
    assert [out[int(bo[k]):int(bo[k + 1])] for k in range(4)] == [texts[0], b"", eng.decode_docs(ids[int(toff[2]):int(toff[2]) + 64], [0, 64], MERGES, vocab=voc)[0], texts[3]]


# ---------------------------------------------------------------- Tokenizer.decode_rows

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


def test_tokenizer_round_trips(tok):
    import torch
    src = english_like(3000) + " 12345 it's \n\n \té€😀 ".encode("utf-8") * 3
    cuts = [0, 0, 300, 301, 301, 1200, 1203, 2500, len(src), len(src)]
    texts = [src[a:b] for a, b in zip(cuts, cuts[1:])]
    texts[3] = IMS.encode() + texts[3] + IMS.encode() + b" tail"  # specials inside a text
    v = tok.vocab
    eos_id, ims_id = int(v.special_ids[0]), int(v.special_ids[1])
    ids, toff = tok.encode_batch(texts)
    counts = np.diff(toff.astype(np.int64))
    M = 48
    assert (counts > M).any() and (counts < M).any()
    pad = eos_id  # pad_id == eos, as generate is usually set up
    for side in ("right", "left"):
        # (1) encode_batch's rows, decoded: decode_batch over what the reference selects
        rows, lens = tok.encode_batch(texts, M, pad, truncation_side=side, return_tensors="pt")
        want = RR.unpack(rows.cpu().numpy(), None, pad, [])
        ref = tok.decode_batch(want[0], want[1])
        got, bounds = tok.decode_rows(rows, pad_id=pad, return_bounds=True)
        assert got == ref and np.array_equal(bounds, want[2])
        assert tok.decode_rows(rows, lens=lens) == ref  # (right padding: the windows say the same)
        assert tok.decode_rows(rows.cpu().numpy(), pad_id=pad) == ref
        fit = [k for k in range(len(texts)) if counts[k] <= M]
        assert all(got[k] == texts[k] for k in fit)
        # (2) the shape generate returns: left padding, the text, an EOS, garbage; int64
        # (without the empty texts: with pad_id == eos the leading pads of an empty row run on through its EOS, and
        # what lies behind it is the text, as the contract says)
        P = 4
        some = [k for k, n in enumerate(lens.cpu().tolist()) if n]
        fit = [j for j, k in enumerate(some) if counts[k] <= M]
        texts_s, rows_s = [texts[k] for k in some], rows[some]
        gen = torch.full((len(some), P + M + 6), pad, dtype=torch.int64)
        for k, n in enumerate(lens[some].cpu().tolist()):
            gen[k, P + M - n:P + M] = rows_s[k, :n].cpu().to(torch.int64)
            gen[k, P + M + 1:] = torch.tensor([-100, 1 << 40, ims_id, 999999, 5])
        gen[:, :P] = ims_id  # a prompt of specials in front, cut off below
        gen = gen.to(rows.device)
        plain = [t.replace(IMS.encode(), b"") for t in texts_s]
        got = tok.decode_rows(gen[:, P:], pad_id=pad, eos=EOT, skip_specials=True)
        assert fit and all(got[k] == plain[k] for k in fit) and any(got[k] != texts_s[k] for k in fit)
        want = RR.unpack(gen[:, P:].cpu().numpy(), None, pad, [eos_id], v.special_ids)
        assert got == tok.decode_batch(want[0], want[1])
        # the specials kept; eos by id, by name as bytes and in a list agree
        kept = tok.decode_rows(gen[:, P:], pad_id=pad, eos=eos_id)
        assert all(kept[k] == texts_s[k] for k in fit)
        assert tok.decode_rows(gen[:, P:], pad_id=pad, eos=[EOT.encode(), 999999]) == kept
        # (3) the suffix alone
        S = P + M - 10
        want = RR.unpack(gen[:, S:].cpu().numpy(), None, pad, [eos_id])
        assert tok.decode_rows(gen[:, S:], pad_id=pad, eos=EOT) == tok.decode_batch(want[0], want[1])
    # an id the vocabulary does not hold inside a text; refused arguments
    bad = torch.tensor([[5, 999999, eos_id]], dtype=torch.int64, device=rows.device)
    with pytest.raises(BpeError, match="unknown token id"):
        tok.decode_rows(bad, eos=EOT)
    assert tok.decode_rows(bad, eos=EOT, pad_id=5, lens=[1]) == [b""]
    with pytest.raises(BpeError, match=re.escape("decode_rows: eos '<|nope|>'")):
        tok.decode_rows(bad, eos="<|nope|>")
    with pytest.raises(BpeError, match="n_stop 9 above 8"):
        tok.decode_rows(bad, eos=list(range(9)))
    with pytest.raises(BpeError, match="pass a 2-D numpy array"):
        tok.decode_rows(bad[0])
    assert tok.decode_rows(np.zeros((0, 5), dtype=np.int64)) == [] and tok.decode_rows(np.zeros((2, 0), dtype=np.int32)) == [b"", b""]


# ---------------------------------------------------------------- scratch

def test_kernels_have_no_scratch_segment():
    spec = importlib.util.spec_from_file_location("kernel_scratch", os.path.join(ROOT, "tools", "kernel_scratch.py"))
    ks = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ks)
    kd = ks.scan(os.environ.get("BPE_LIB") or os.path.join(ROOT, "llmtokenizer_amd", "libbpe_amd.so"))
    found = {name: v for name, v in kd.items() if re.search(r"\dk_rows_(bounds|gather)I", name)}
    # bounds and gather, 4- and 8-byte cells, the vector and the one-cell variant
    assert len(found) == 8 and {(("bounds" in n), ("Ij" in n), ("Lb1E" in n)) for n in found} == set(itertools.product((True, False), repeat=3)), sorted(found)
    assert all(scratch == 0 and lds <= 1024 for lds, scratch in found.values()), found

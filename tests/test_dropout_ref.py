"""dropout_ref._replay, the Python yardstick of the dropout kernels, held to the C oracle where the contract makes
the two coincide: a drop probability so small that its threshold floor(p * 2^32) is 0 drops nothing, and "with
p = 0 the ids are those of BPE_ENC_PIECE_LONG", which are the oracle's.  The inputs are those of the two
deterministic piece-encoder test files (rank order, a == a runs, the tile and long-piece geometry); the builders
below are shared with test_gpu_encode_piece_edges.py.  No GPU."""
import functools
import random

import numpy as np
import pytest

import encode_limits_lib as EL
import oracle_lib as O
import test_gpu_encode_long as TL
import test_gpu_encode_piece as TP
from dropout_ref import _dropped, _mix64, _rank, _replay, _replay_batch
from llmtokenizer_amd import api

TINY = 1e-12  # a probability above 0 whose threshold is 0


@functools.lru_cache(maxsize=None)
def sizes():
    """(C, P, M, max_ids): a tile's core and longest piece, the long kernel's longest piece, the id limit"""
    pi = api.piece_info()
    return pi["core"], pi["piece_max"], api.long_piece_info()["piece_max"], pi["max_ids"]


@functools.lru_cache(maxsize=None)
def merges300():
    m = EL._random_merges(random.Random(5), b"abcd", 300, eq=0.2)
    m.setflags(write=False)
    return m


def letters(rng, n):
    return bytes(rng.choice(b"abcd") for _ in range(n))


def order_docs(name):
    """(documents, merges) of test_gpu_encode_piece.ORDER[name]"""
    docs, merges = next((d, m) for n, d, m in TP.ORDER if n == name)
    return (docs(sizes()[1]) if callable(docs) else docs), merges


def piece_geometry_docs(name):
    """the documents of test_gpu_encode_piece.test_tile_geometry(name) (under merges300)"""
    rng = random.Random(len(name))
    return [letters(rng, n) for n in TP.GEOMETRY[name](*sizes()[:2])]


def long_geometry_docs(name):
    """the documents of test_gpu_encode_long.test_long_pieces_among_the_tiles(name) (under merges300)"""
    rng = random.Random(len(name))
    return [letters(rng, n) for n in TL.GEOMETRY[name](*sizes()[:3])]


def replay_docs(docs, merges, p, seed, rank=None, batch=False):
    """the replay of every document at its resident offset in the joined batch (batch: by _replay_batch)"""
    rank, bases = _rank(merges) if rank is None else rank, np.cumsum([0] + [len(d) for d in docs]).tolist()
    if batch:
        return _replay_batch(docs, bases, rank, p, seed)
    return [_replay(d, b, rank, p, seed) for d, b in zip(docs, bases)]


def _same_as_the_oracle(docs, merges):
    assert int(TINY * 2**32) == 0 and TINY > 0
    for seed in (0, 2**64 - 1):
        got = replay_docs(docs, merges, TINY, seed)
        for d, g in zip(docs, got):
            assert g == O.encode(d, merges).tolist(), (len(d), seed)


def test_the_draw():
    """a threshold of 0 drops nothing, one of 2^32 everything, and the round keys are 32-bit and differ"""
    keys = [_mix64((7 + 0x9E3779B97F4A7C15 * (t + 1)) & (2**64 - 1)) & 0xFFFFFFFF for t in range(64)]
    assert len(set(keys)) == 64
    for g in (0, 1, 12345, 2**32 - 1):
        assert not any(_dropped(g, k, 0) for k in keys) and all(_dropped(g, k, 1 << 32) for k in keys)
    rank = _rank(merges300())
    text = letters(random.Random(1), 200)
    assert _replay(text, 5, rank, 1.0, 3) == list(text)
    assert _replay(text, 5, rank, 0.5, 3) != _replay(text, 6, rank, 0.5, 3)  # keyed by the resident offset


@pytest.mark.parametrize("p", [TINY, 0.1, 0.3, 0.5, 0.9, 1 - 2.0**-33, 1.0])
def test_the_batch_form_equals_the_replay(p):
    """_replay_batch, which the GPU tests use for their largest batches, against _replay: mixed letters over three
    tile lengths, empty and one-byte pieces, a == a runs kept and dropped in stretches, rank order"""
    P = sizes()[1]
    rng = random.Random(9)
    mixed = [letters(rng, n) for n in (300, 1, 0, P, P + 1, 2, 2500, 0)]
    runs = [b"a" * k + b"b" for k in range(2, 10)]
    runs += [b"ba" + b"a" * 150 + b"b" + b"a" * 31, b"", b"a" * 1500 + b"b" + b"a" * 777]
    odd, odd_merges = order_docs("odd_records")
    for docs, merges in ((mixed, merges300()), (runs, TL.RUNS), (odd, odd_merges)):
        for seed in (0, 0xDEADBEEFCAFEF00D, 2**64 - 1):
            assert replay_docs(docs, merges, p, seed, batch=True) == replay_docs(docs, merges, p, seed)


@pytest.mark.parametrize("name", [o[0] for o in TP.ORDER])
def test_rank_order(name):
    _same_as_the_oracle(*order_docs(name))


@pytest.mark.parametrize("name", list(TL.RUN_DOCS))
def test_runs(name):
    _same_as_the_oracle(TL.RUN_DOCS[name](sizes()[2]), TL.RUNS)


@pytest.mark.parametrize("name", list(TP.GEOMETRY))
def test_tile_geometry(name):
    _same_as_the_oracle(piece_geometry_docs(name), merges300())


@pytest.mark.parametrize("name", list(TL.GEOMETRY))
def test_long_geometry(name):
    _same_as_the_oracle(long_geometry_docs(name), merges300())

"""The packed streams' contract (include/bpe_gpu.h, "Packed streams") in plain Python, for the tests: the stream is
built literally, by list concatenation text by text, with (text, start of the text) recorded per cell, and then cut
into rows.  No closed form for a text's start is used.  Test infrastructure only."""
import numpy as np

NO_TEXT = 0xFFFFFFFF


def pack_stream(ids, text_off, seq_len, pad_id, bos_id=None, eos_id=None, drop_last=False):
    """(rows, seg, pos, N): uint32[R, seq_len] each and the cells of the stream"""
    ids = np.asarray(ids, dtype=np.uint32).reshape(-1).tolist()
    off = [int(o) for o in np.asarray(text_off).reshape(-1)]
    L = int(seq_len)
    stream, text, start = [], [], []  # per cell: its id, its text, the stream position of that text's first cell
    for k in range(len(off) - 1):
        cells = ([bos_id] if bos_id is not None else []) + ids[off[k]:off[k + 1]] + ([eos_id] if eos_id is not None else [])
        text += [k] * len(cells)
        start += [len(stream)] * len(cells)
        stream += cells
    N = len(stream)
    R = N // L if drop_last else -(-N // L)
    rows = np.full(R * L, pad_id, dtype=np.uint32)
    seg = np.full(R * L, NO_TEXT, dtype=np.uint32)
    pos = np.zeros(R * L, dtype=np.uint32)
    m = min(N, R * L)
    c = np.arange(m, dtype=np.int64)
    rows[:m] = stream[:m]
    seg[:m] = text[:m]
    pos[:m] = c - np.maximum(np.asarray(start[:m], dtype=np.int64), c // L * L)
    return rows.reshape(R, L), seg.reshape(R, L), pos.reshape(R, L), N


def matrix_lengths(L, seed, copies=4):
    """text lengths 0, 1, L - 1, L, L + 1 and 3 L, `copies` of each, shuffled with a fixed seed"""
    lens = [0, 1, L - 1, L, L + 1, 3 * L] * copies
    np.random.default_rng(seed).shuffle(lens)
    return [int(x) for x in lens]


def offsets(lens):
    return np.concatenate([[0], np.cumsum(np.asarray(lens, dtype=np.int64))]).astype(np.uint64)


BOS_EOS = [(None, None), (70001, None), (None, 70002), (70001, 70002)]  # ids no test vocabulary holds

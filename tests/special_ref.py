"""The split with special tokens restated in Python (bpe_gpu.h, "Special tokens"), for
tests/test_special_host.py and tests/test_gpu_special.py: the matches are re.finditer of the
escaped alternation, every segment between them goes through `seg_split`, a function of a
segment's bytes that returns its offsets (starts followed by its length)."""
import re

import numpy as np

GPT2_SET = [b"<|endoftext|>"]
CHATML_SET = [b"<|endoftext|>", b"<|im_start|>", b"<|im_end|>", b"<|fim_prefix|>", b"<|fim_middle|>", b"<|fim_suffix|>"]
RESERVED_SET = [b"<|begin_of_text|>", b"<|end_of_text|>", b"<|start_header_id|>", b"<|end_header_id|>", b"<|eot_id|>"] + \
               [b"<|reserved_special_token_%d|>" % i for i in range(251)]
assert len(RESERVED_SET) == 256


def matches(data, specials):
    """[(start, end, j)] of every occurrence of a special, in order"""
    if not specials:
        return []
    pat = re.compile(b"|".join(b"(" + re.escape(bytes(s)) + b")" for s in specials), re.S)
    return [(m.start(), m.end(), m.lastindex - 1) for m in pat.finditer(data)]


def restate(data, specials, seg_split):
    """(offsets, special piece indices, their specials' indices)"""
    out, piece, index, pos = [], [], [], 0
    for s, e, j in matches(data, specials) + [(len(data), len(data), None)]:
        if s > pos:
            off = [int(x) for x in seg_split(data[pos:s])]
            assert off[0] == 0 and off[-1] == s - pos
            out += [pos + x for x in off[:-1]]
        if j is not None:
            piece.append(len(out))
            index.append(j)
            out.append(s)
        pos = e
    return np.array(out + [len(data)], np.uint64), np.array(piece, np.uint64), np.array(index, np.uint32)


def table_split(cls, brk):
    """seg_split of a two-table rule"""
    cls, brk = np.asarray(cls), np.asarray(brk)

    def f(seg):
        b = np.frombuffer(seg, np.uint8)
        c = cls[b]
        st = np.ones(b.size, bool)
        st[1:] = (brk[c[:-1]] >> c[1:]) & 1
        return np.append(np.flatnonzero(st), b.size)
    return f


def random_rule(seed):
    """a random two-table rule (cls uint8[256] in 0..15, brk uint16[16])"""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 16, 256).astype(np.uint8), rng.integers(0, 1 << 16, 16).astype(np.uint16)

"""Plain-Python restatement of training on pieces (bpe_gpu.h, bpe_gpu_train_split):
the yardstick of tests/test_gpu_train_split.py, pinned to the oracle by
tests/test_train_split_ref.py.  Not a test module.

The corpus is a multiset of pieces, each its bytes as ids 0..255.  count(a, b) is
the number of positions, over all pieces, where a is followed by b inside one
piece.  Merge r takes the pair with the largest count (ties: the smaller a, then
the smaller b), names it 256 + r and applies it inside every piece from left to
right.  Stop: no pair or the largest count <= 1 (reason 1, checked first), then
max_merges merges made (2), then the engine's cap (3).
"""
from collections import Counter, defaultdict

import numpy as np


def pieces_of(data, cls, brk):
    """the pieces of data under the two-table rule (bpe_gpu.h, bpe_gpu_split), in order"""
    b = np.frombuffer(data, np.uint8)
    if b.size == 0:
        return []
    c = np.asarray(cls)[b]
    st = np.ones(b.size, bool)
    st[1:] = (np.asarray(brk)[c[:-1]] >> c[1:]) & 1
    off = np.append(np.flatnonzero(st), b.size)
    return [data[int(x):int(y)] for x, y in zip(off, off[1:])]


def _apply(s, a, b, z):
    """s with every (a, b) replaced by z, left to right (list.index finds the next a)"""
    out, i, n = [], 0, len(s)
    while True:
        try:
            j = s.index(a, i)
        except ValueError:
            out.extend(s[i:])
            return out
        if j + 1 < n and s[j + 1] == b:
            out.extend(s[i:j])
            out.append(z)
            i = j + 2
        else:
            out.extend(s[i:j + 1])
            i = j + 1


def train(pieces, max_merges=-1, engine_cap=1 << 24):
    """(merges, stop_reason, first_tie): merges a list of (a, b); first_tie the index of the
    first merge whose largest count two or more pairs shared (None: there was none)"""
    entries = [(list(p), w) for p, w in Counter(pieces).items()]
    merges, first_tie = [], None
    while True:
        cnt = defaultdict(int)
        for s, w in entries:
            if len(s) == 2:
                cnt[(s[0], s[1])] += w
            elif len(s) > 64:
                for pair, k in Counter(zip(s, s[1:])).items():
                    cnt[pair] += k * w
            else:
                for pair in zip(s, s[1:]):
                    cnt[pair] += w
        if not cnt:
            return merges, 1, first_tie
        top = max(cnt.values())
        if top <= 1:
            return merges, 1, first_tie
        r = len(merges)
        if 0 <= max_merges <= engine_cap and r == max_merges:
            return merges, 2, first_tie
        if r == engine_cap:
            return merges, 3, first_tie
        best = sorted(p for p, k in cnt.items() if k == top)
        if len(best) > 1 and first_tie is None:
            first_tie = r
        a, b = best[0]
        merges.append((a, b))
        entries = [(_apply(s, a, b, 256 + r) if a in s else s, w) for s, w in entries]

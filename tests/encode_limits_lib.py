"""Input builders for test_encode_limits.py: merge lists and texts that reach
the window encoders' plan limits (encode_win.hip EW_MAX_MERGES = 65279 merges,
EW_MAX_BATCHES = 256 layers).  Pure Python and numpy; nothing here touches the
library under test.  layers() restates the layered rule of the comment above
engine.hip ew_plan, only to choose and guard inputs; pin_last() asks the
oracle."""
import random

import numpy as np

A_BYTES = range(1, 129)    # two_layer_list: left bytes
B_BYTES = range(129, 256)  # right bytes
N_LAYER0 = len(A_BYTES) * len(B_BYTES)  # 16256
FILLER = b" \n.,"  # what text_for puts between expansions by default (and what the tests' split rule breaks after)


def _arr(pairs):
    return np.array(pairs, dtype=np.uint32).reshape(-1, 2)


class _Layering:
    """the layer of every record, one record at a time (ew_plan, step 1)"""

    def __init__(self, cap):
        V = 256 + cap
        # per id: latest layer creating it / using it left / right / in an
        # a == a merge / at all (-1: none); per pair: latest layer holding it
        self.cre, self.asl, self.asr, self.aeq, self.any = ([-1] * V for _ in range(5))
        self.key = {}
        self.batch = []

    def peek(self, u, v):
        """the layer a record (u, v) would get as the next one"""
        r = len(self.batch)
        if not (u < 256 + r and v < 256 + r):
            return 0  # can never match: it changes nothing, so it goes first
        dep = max(self.cre[u], self.cre[v], self.aeq[u], self.aeq[v], self.asr[u], self.asl[v], self.key.get((u, v), -1))
        if u == v:
            dep = max(dep, self.any[u])
        return dep + 1

    def add(self, u, v):
        r = len(self.batch)
        L = self.peek(u, v)
        if u < 256 + r and v < 256 + r:
            self.asl[u] = max(self.asl[u], L)
            self.asr[v] = max(self.asr[v], L)
            self.any[u] = max(self.any[u], L)
            self.any[v] = max(self.any[v], L)
            if u == v:
                self.aeq[u] = max(self.aeq[u], L)
            self.key[(u, v)] = L
        self.cre[256 + r] = L
        self.batch.append(L)
        return L


def _layering(merges):
    m = np.asarray(merges).reshape(-1, 2).tolist()
    s = _Layering(len(m) + 1)
    for u, v in m:
        s.add(u, v)
    return s


def layers(merges):
    """(number of layers, layer of each merge)"""
    batch = _layering(merges).batch
    return (max(batch) + 1 if batch else 0), batch


def relabeled(merges):
    """the replay order differs from the list's: the layers do not come in order"""
    batch = layers(merges)[1]
    return any(a > b for a, b in zip(batch, batch[1:]))


def two_layer_list(m, seed=1):
    """layer 0: every pair (a, b), a in 1..128, b in 129..255; layer 1: m - 16256
    distinct pairs (256 + i, b) over the layer-0 ids, seeded and sorted"""
    assert N_LAYER0 <= m <= N_LAYER0 + N_LAYER0 * len(B_BYTES)
    out = [(a, b) for a in A_BYTES for b in B_BYTES]
    nB = len(B_BYTES)
    for x in sorted(random.Random(seed).sample(range(N_LAYER0 * nB), m - N_LAYER0)):
        out.append((256 + x // nB, B_BYTES[0] + x % nB))
    return _arr(out)


def _random_merges(rng, alphabet, k, eq=0.3):
    """as in test_gpu_encode_win.py (the same draws from the same rng)"""
    ids = list(alphabet)
    out = []
    for r in range(k):
        u, v = rng.choice(ids), rng.choice(ids)
        if rng.random() < eq:
            v = u
        out.append((u, v))
        ids.append(256 + r)
    return np.array(out, dtype=np.uint32).reshape(-1, 2)


def random_list(rng, m):
    return _random_merges(rng, range(1, 256), m, eq=0.2)


def chain_list(k):
    """k records, each using the id the one before creates: exactly k layers"""
    return _arr([(97, 98)] + [(256 + r, 99 + r % 3) for r in range(k - 1)])


TAIL_ALPHABET = range(110, 118)


def chain_with_tail(k, rng, tail=3000):
    """the chain, then random records over letters the chain does not use
    (their ids shifted past the chain's): the tail's early layers come after
    the chain's late ones in the list, so the plan reorders it"""
    t = _random_merges(rng, TAIL_ALPHABET, tail, eq=0.2).astype(np.int64)
    t[t >= 256] += k
    return np.vstack([chain_list(k), t.astype(np.uint32)])


def expansion_lengths(merges):
    """bytes of every id (Python ints: a random list's grow past 2^64)"""
    ln = [1] * 256
    for r, (u, v) in enumerate(np.asarray(merges).reshape(-1, 2).tolist()):
        assert u < 256 + r and v < 256 + r
        ln.append(ln[u] + ln[v])
    return ln


def expand(merges, x):
    """the bytes of id x"""
    m = np.asarray(merges).reshape(-1, 2)
    out, stack = bytearray(), [int(x)]
    while stack:
        t = stack.pop()
        if t < 256:
            out.append(t)
        else:
            stack.append(int(m[t - 256][1]))
            stack.append(int(m[t - 256][0]))
    return bytes(out)


def text_for(merges, rng, ids, max_len, filler=FILLER, starts=None):
    """the expansions of ids, in order, 0-5 filler bytes between them, as many
    as fit into max_len bytes (starts: a list that receives where each expansion begins)"""
    out = bytearray()
    for x in ids:
        piece = expand(merges, x) + bytes(rng.choice(filler) for _ in range(rng.randint(0, 5)))
        if len(out) + len(piece) > max_len:
            break
        if starts is not None:
            starts.append(len(out))
        out += piece
    return bytes(out)


def pin_last(merges, text, layer=None):
    """the list with its last record overwritten by an adjacent pair of the
    oracle's output for merges[:-1] that is no record yet: the last id then
    occurs in the oracle's output for the whole list, whatever the list is.
    layer: the layer the new record must land in (None: any)."""
    import oracle_lib as O
    m = np.array(merges, dtype=np.uint32).reshape(-1, 2)
    head = m[:-1]
    ids = O.encode(text, head).tolist()
    have = set(map(tuple, head.tolist()))
    state = _layering(head) if layer is not None else None
    for u, v in zip(ids, ids[1:]):
        if (u, v) in have or (state is not None and state.peek(u, v) != layer):
            continue
        m[-1] = (u, v)
        return m
    raise AssertionError("pin_last: no free adjacent pair in the oracle's output")

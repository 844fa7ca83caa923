"""Corpora and a numpy replay for tests/test_gpu_regimes.py -- TEST ONLY.

Default-mode training changes machinery as the live token count n falls:
untracked iterations and batches at n >= TRACK_LIMIT (2^21), tracked
iterations over the chunked schedule down to DYN_LIMIT (2^20), the
reference's static 1/16 split below (csrc/engine_common.h, mirrored by
oracle/bpe_oracle.c).  The corpora here put n at chosen distances from those
limits within the first few merges; the replay turns a merge list (the
oracle's) into the live count before every merge and the merged pair's count,
so a test knows without the engine which merge is the first of each regime.
"""
import hashlib
import json
import os

import numpy as np

from llmtokenizer_amd.synth import synth_bytes

DYN_LIMIT = 1 << 20
TRACK_LIMIT = 1 << 21

RUN_BYTE = 1  # synth_bytes holds 32..126 only: the run never touches the tail


def run_tail(L, d, seed=905, tail_len=9000):
    """A run of one byte, then a small random tail: the run halves per merge
    and the live count after the first merge is exactly L + d"""
    R = 2 * (L + d - tail_len)
    return bytes([RUN_BYTE]) * R + synth_bytes(seed, tail_len)


def run_tail_both(seed=907, tail_len=30000, R=TRACK_LIMIT + 5000):
    """n0 > 2^21; the halving run crosses both limits within three merges"""
    return bytes([RUN_BYTE]) * R + synth_bytes(seed, tail_len)


def _segment(x, y, fill, reps):
    """x y f0 x y f1 ... (reps triples, the filler cycling): (x, y) counts
    reps, every other pair of the segment about reps / len(fill)"""
    seg = np.empty((reps, 3), dtype=np.uint8)
    seg[:, 0] = x
    seg[:, 1] = y
    seg[:, 2] = np.resize(np.asarray(fill, dtype=np.uint8), reps)
    return seg.tobytes()


def batch_cut(d, seed=905, tail_len=9000, B=258000, C=255000):
    """Three bulk pairs over disjoint bytes (none of them in the tail) with
    counts A > B > C far above every other pair's: they commute, so the first
    selection of the batch engine lists them as members 0, 1, 2.  A is chosen
    so that the live count after member 0 alone is 2^21 + d."""
    rest = TRACK_LIMIT + d - tail_len - 3 * C
    B += (rest - 3 * B) & 1  # n0 - A = 2 A + 3 B + 3 C + tail: make 2 A even
    A = (rest - 3 * B) // 2
    assert A > B > C > A // 4
    return (_segment(0x80, 0x81, range(0x90, 0x98), A) + _segment(0x82, 0x83, range(0x98, 0xA0), B) +
            _segment(0x84, 0x85, range(0xA0, 0xA8), C) + synth_bytes(seed, tail_len))


def reference_golden(name="run_tail_2m"):
    """(corpus, fixture) of tests/golden/regimes/<name>.json: the md5 of the merges and of the ids the
    unmodified reference gave for a run_tail corpus, which the fixture describes by its recipe"""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "regimes", name + ".json")) as f:
        fx = json.load(f)
    r = fx["recipe"]
    return bytes([r["run_byte"]]) * r["run_len"] + synth_bytes(r["tail_seed"], r["tail_len"]), fx


def check_golden(fx, merges, ids):
    merges, ids = np.ascontiguousarray(merges, dtype="<u4"), np.ascontiguousarray(ids, dtype="<u4")
    assert (merges.shape[0], ids.size) == (fx["n_merges"], fx["ids_len"])
    assert hashlib.md5(merges.tobytes()).hexdigest() == fx["merges_md5"]
    assert hashlib.md5(ids.tobytes()).hexdigest() == fx["ids_md5"]


def replay(data, merges):
    """The reference's replace pass (bpe.c:760-779: greedy, left to right)
    applied merge by merge.  Returns (live, count, tokens): live[k] the token
    count before merge k (live[len(merges)] the final one), count[k] the
    adjacent occurrences of pair k then (overlapping ones included, as the
    reference counts them), tokens the final ids."""
    tok = np.frombuffer(data, dtype=np.uint8).astype(np.uint32)
    merges = np.asarray(merges).reshape(-1, 2)
    live = np.empty(merges.shape[0] + 1, dtype=np.int64)
    count = np.empty(merges.shape[0], dtype=np.int64)
    for k, (a, b) in enumerate(merges.tolist()):
        live[k] = tok.size
        hit = np.flatnonzero((tok[:-1] == a) & (tok[1:] == b))
        count[k] = hit.size
        if a == b and hit.size:
            # a run of a's pairs up from its first token: hits at consecutive
            # positions form a group, and every second one of a group merges
            i = np.arange(hit.size)
            start = np.ones(hit.size, dtype=bool)
            start[1:] = hit[1:] != hit[:-1] + 1
            first = np.maximum.accumulate(np.where(start, i, 0))
            hit = hit[((i - first) & 1) == 0]
        keep = np.ones(tok.size, dtype=bool)
        keep[hit + 1] = False
        tok[hit] = 256 + k
        tok = tok[keep]
    live[-1] = tok.size
    return live, count, tok


def first_below(live, limit):
    """index of the first merge selected at fewer than `limit` live tokens
    (len(live) - 1 when there is none)"""
    below = np.flatnonzero(live[:-1] < limit)
    return int(below[0]) if below.size else live.size - 1


def diff_merges(m0, m1):
    """indices at which two merge lists differ (a length difference counts
    from the shorter one's end)"""
    k = min(m0.shape[0], m1.shape[0])
    idx = np.flatnonzero((m0[:k] != m1[:k]).any(axis=1)).tolist()
    return idx + list(range(k, max(m0.shape[0], m1.shape[0])))

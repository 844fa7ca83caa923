"""The dropout contract of bpe_gpu.h ("Dropout") written out over lists of ids and byte offsets, the draw in
Python ints: the yardstick of the GPU tests of encode_drop.hip.  Pure Python; nothing here touches the library
under test.  test_dropout_ref.py holds it to the C oracle where the two must coincide (a threshold of 0)."""

M32, M64 = (1 << 32) - 1, (1 << 64) - 1


def _mix64(x):
    x ^= x >> 33
    x = x * 0xff51afd7ed558ccd & M64
    x ^= x >> 33
    x = x * 0xc4ceb9fe1a85ec53 & M64
    return x ^ x >> 33


def _dropped(g, kt, thr):
    x = (g ^ kt) & M32
    x ^= x >> 16
    x = x * 0x7feb352d & M32
    x ^= x >> 15
    x = x * 0x846ca68b & M32
    return (x ^ x >> 16) < thr


def _replay(piece, base, rank, p, seed):
    """the ids of one piece whose first byte lies at resident offset base"""
    thr = min(1 << 32, int(p * 4294967296.0))
    ids, off, t = list(piece), list(range(base, base + len(piece))), 0
    while True:
        kt = _mix64((seed + 0x9E3779B97F4A7C15 * (t + 1)) & M64) & M32
        kept = [(rank[ids[i], ids[i + 1]], i) for i in range(len(ids) - 1)
                if (ids[i], ids[i + 1]) in rank and not _dropped(off[i], kt, thr)]
        if not kept:
            return ids
        r = min(kept)[0]
        win = {i for q, i in kept if q == r}
        out, oo, i = [], [], 0
        while i < len(ids):
            merge = i in win
            out.append(256 + r if merge else ids[i])
            oo.append(off[i])
            i += 2 if merge else 1
        ids, off, t = out, oo, t + 1


def _rank(merges):
    return {tuple(m): r for r, m in reversed(list(enumerate(merges.tolist())))}


def _replay_batch(pieces, bases, rank, p, seed):
    """[_replay(piece, base, rank, p, seed) for every piece], all pieces side by side in numpy arrays, for batches
    that _replay would take a quarter of a minute for: the same rounds (every piece starts at t = 0), one array
    pass each.  Of a stretch of adjacent winners (an a == a run) those at an even distance from its first merge,
    which is what _replay's left-to-right walk takes.  test_dropout_ref.py holds it to _replay."""
    import numpy as np
    none = np.int64(1 << 62)
    thr = min(1 << 32, int(p * 4294967296.0))
    order = sorted(rank)
    keys = np.array([a << 32 | b for a, b in order] + [(1 << 63) - 1], dtype=np.int64)
    vals = np.array([rank[k] for k in order] + [0], dtype=np.int64)
    lens = [len(x) for x in pieces]
    ids = np.frombuffer(b"".join(bytes(x) for x in pieces), dtype=np.uint8).astype(np.int64)
    off = np.concatenate([np.arange(b, b + n, dtype=np.int64) for b, n in zip(bases, lens)] + [np.zeros(0, np.int64)])
    pid = np.repeat(np.arange(len(pieces)), lens)
    out, t = [[] for _ in pieces], 0
    while ids.size:
        kt = _mix64((seed + 0x9E3779B97F4A7C15 * (t + 1)) & M64) & M32
        pair = ids[:-1] << 32 | ids[1:]
        j = np.searchsorted(keys, pair)
        x = ((off[:-1] ^ kt) & M32).astype(np.uint64)
        x ^= x >> np.uint64(16)
        x = x * np.uint64(0x7feb352d) & np.uint64(M32)
        x ^= x >> np.uint64(15)
        x = x * np.uint64(0x846ca68b) & np.uint64(M32)
        x ^= x >> np.uint64(16)
        kept = (keys[j] == pair) & (pid[:-1] == pid[1:]) & (x >= np.uint64(thr))
        rk = np.append(np.where(kept, vals[j], none), none)  # (a piece's last token has no pair)
        first = np.flatnonzero(np.append(True, pid[1:] != pid[:-1]))
        best = np.repeat(np.minimum.reduceat(rk, first), np.diff(np.append(first, ids.size)))
        live = best != none
        ends = np.append(first[1:], ids.size)
        for i in np.flatnonzero(~live[first]).tolist():  # no kept candidate: the piece is finished
            out[pid[first[i]]] = ids[first[i]:ends[i]].tolist()
        win = live & (rk == best)
        at = np.arange(ids.size)
        head = np.maximum.accumulate(np.where(win & ~np.append(False, win[:-1]), at, -1))
        merge = win & ((at - head) % 2 == 0)
        stay = live & ~np.append(False, merge[:-1])
        ids, off, pid = np.where(merge, 256 + rk, ids)[stay], off[stay], pid[stay]
        t += 1
    return out

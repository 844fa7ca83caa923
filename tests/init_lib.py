"""Corpora aimed at the edges of the training init -- TEST ONLY.

Every training run starts with the skew probe (k_pair_skew_sample), the count
pass in one of its forms (launch_count_pass, csrc/engine.hip), the column
sums and scan, and the two-pass counting sort of byte-pair positions
(k_sort_a / k_sort_b).  The corpora here put a byte pair whose count decides
the first merges at a chosen position (a tile, block, lane or group edge of
those kernels, or the corpus's last pair), or load the kernels' same-address
paths (one byte, two alternating, a dominant pair, a dominant first byte, a
long run inside random text, two hot pairs in one packed word).

Nothing here touches the engine: numpy only.  probe() and form_code() restate
the probe's sampling and the dispatch's documented LDS bounds, so a test knows
which form a corpus and a set of knobs must select before it asks stats().
"""
import functools

import numpy as np

TILE = 65536          # the init's default tile: pair positions per count-pass / sort block
BLOCK = 1024          # bytes a wave takes at a time; 16 waves, two blocks each per round
SKEW_SAMPLES = 16384  # dwords the probe samples
SPAN_MAX = 128        # widest byte-value span the span forms bin directly
HBINS = 16384         # bins of one part of the generic form
LDS_SMALL, LDS_LARGE = 80 * 1024, 160 * 1024
CAP = 300             # merges per run; corpora of at most SMALL bytes train to the stop rule
SMALL = 8192


def plant_count(n):
    return max(40, n // 100)


def planted_pairs(lo, S, swap=False):
    """(the pair on the edge, the other pair): Y = (lo+S-2, lo+S-1) straddles
    the edge and X = (lo, lo+1) does not, or the reverse with swap"""
    X, Y = (lo, lo + 1), (lo + S - 2, lo + S - 1)
    return (X, Y) if swap else (Y, X)


def planted(n, edge, lo, S, dense=False, swap=False, tail=False):
    """n bytes over [lo, lo+S): a filler uniform over about 24 middle values
    (dense: over every value of the span but the four planted ones) and two
    pairs X = (lo, lo+1), Y = (lo+S-2, lo+S-1), whose bytes occur nowhere
    else, each planted exactly plant_count(n) times at spread positions.  One
    occurrence of Y (of X with swap) has its first byte at edge - 1, the last
    pair position before the edge, and no other plant within 8 bytes of it.
    tail: one occurrence of the other pair is the corpus's last pair."""
    c = plant_count(n)
    assert S >= 6 and 1 <= lo and lo + S <= 256 and 1 <= edge <= n - 1
    rng = np.random.default_rng([n, edge, lo, S, int(dense), int(swap)])
    if dense:
        vals = np.arange(lo + 2, lo + S - 2)
    else:
        k = min(24, S - 4)
        first = lo + 2 + (S - 4 - k) // 2
        vals = np.arange(first, first + k)
    a = vals[rng.integers(0, vals.size, n)].astype(np.uint8)
    on_edge, other = planted_pairs(lo, S, swap)
    tail = tail and edge != n - 1
    # one slot per plant and a few to spare: a random offset inside each slot keeps plants at least 5
    # bytes apart and off any fixed phase of the kernels' 16-byte and 1-KB grids
    m = 2 * c + 6
    stride = n // m
    assert stride >= 9, "corpus too small for its plants"
    pos = np.arange(m) * stride + rng.integers(0, stride - 4, m)
    keep = np.abs(pos - (edge - 1)) >= 8
    if tail:
        keep &= pos < n - 10
    pos = pos[keep]
    need = 2 * c - 1 - int(tail)
    assert pos.size >= need
    pos = pos[np.round(np.linspace(0, pos.size - 1, need)).astype(np.int64)]
    assert np.unique(pos).size == need and pos.max() <= n - 2
    is_other = np.zeros(need, dtype=bool)
    is_other[rng.permutation(need)[: c - int(tail)]] = True
    for p, pair in ((pos[is_other], other), (pos[~is_other], on_edge)):
        a[p], a[p + 1] = pair
    a[edge - 1], a[edge] = on_edge
    if tail:
        a[n - 2], a[n - 1] = other
    return a.tobytes()


def one_byte(n, b=97):
    return bytes([b]) * n


def alternating(n, a=97, b=98):
    return (bytes([a, b]) * (n // 2 + 1))[:n]


def two_values(n, lo, S, seed=5):
    """only lo and lo + S - 1 present: a span with holes, A = 2"""
    rng = np.random.default_rng([seed, n, lo, S])
    return np.where(rng.random(n) < 0.6, lo, lo + S - 1).astype(np.uint8).tobytes()


def _text(rng, n, lo=32, S=95):
    return rng.integers(lo, lo + S, n).astype(np.uint8)


def small_text(n, seed=3):
    """a few values, for the tiny sizes"""
    return np.random.default_rng([seed, n]).integers(97, 100, n).astype(np.uint8).tobytes()


def dominant_pair(n, pair=(101, 32), seed=7):
    """random text over 32..126 with `pair` once in every 10 bytes, at a random
    offset: 1/10 of the pairs, more than the probe's 1/16"""
    rng = np.random.default_rng([seed, n])
    a = _text(rng, n)
    p = np.arange(n // 10) * 10 + rng.integers(0, 9, n // 10)
    a[p], a[p + 1] = pair
    return a.tobytes()


def dominant_first_byte(n, seed=9):
    """a space at every even position, one of 24 letters at every odd one: half
    the pairs start with a space (the probe's skew[2], which shrinks the sort's
    groups), yet no pair holds more than about 1/48 of them"""
    rng = np.random.default_rng([seed, n])
    a = rng.integers(97, 121, n).astype(np.uint8)
    a[0::2] = 32
    return a.tobytes()


def locally_skewed(n, run=50000, at=300001, seed=11):
    """random text with one run of a single byte inside it, at an odd offset:
    skewed for the blocks that meet the run, not for the probe"""
    rng = np.random.default_rng([seed, n])
    a = _text(rng, n)
    assert at + run < n
    a[at:at + run] = 97
    return a.tobytes()


def packed_word(n, lo=32, S=95, x=100, seed=13):
    """'x x y' with y = x + 1 over nine tenths of the corpus, random text over
    [lo, lo+S) for the rest: the hot pairs (x, x) and (x, y) hold more than 1/4
    of all pairs each, and their packed-form bins differ in the lowest bit"""
    rng = np.random.default_rng([seed, n])
    a = _text(rng, n, lo, S)
    k = n * 9 // 10 // 3 * 3
    a[:k] = np.resize(np.array([x, x, x + 1], dtype=np.uint8), k)
    a[n - 2], a[n - 1] = lo, lo + S - 1  # the span's ends are present
    return a.tobytes()


def packed_bin(pair, lo, S):
    return pair[0] * S + pair[1] - (lo * S + lo)


def alphabet(data):
    """(lo, S, A) of the byte values present"""
    v = np.flatnonzero(np.bincount(np.frombuffer(data, dtype=np.uint8), minlength=256))
    return int(v[0]), int(v[-1] - v[0] + 1), int(v.size)


def pair_hist(data):
    """counts of the byte pairs, index 256 * first + second"""
    a = np.frombuffer(data, dtype=np.uint8).astype(np.int64)
    return np.bincount(a[:-1] * 256 + a[1:], minlength=65536)


def probe(data):
    """what k_pair_skew_sample reports: the three pairs inside each of up to
    SKEW_SAMPLES whole dwords spread evenly over the corpus -> (largest pair
    count, pairs sampled, largest count of one first byte)"""
    nwords = len(data) // 4
    ns = min(SKEW_SAMPLES, nwords)
    if ns == 0:
        return 0, 0, 0
    w = np.frombuffer(data, dtype=np.uint8, count=4 * nwords).reshape(-1, 4).astype(np.int64)
    w = w[(np.arange(ns, dtype=np.int64) * nwords) // ns]
    first, second = w[:, :3].reshape(-1), w[:, 1:].reshape(-1)
    return (int(np.bincount(first * 256 + second).max()), 3 * ns, int(np.bincount(first).max()))


def skewed(data):
    """the probe's verdict: a pair holds more than 1/16 of the sampled pairs"""
    top, tot, _ = probe(data)
    return tot > 0 and top * 16 > tot


def form_code(S, skew, env=None):
    """stats()["count_pass_span"] for a corpus of span S with the probe's
    verdict `skew` under the knobs in env: 0 the generic form, 200 + R the
    vector form, 300 + R its run-folding variant, R the shuffle form, 100 + R
    the packed form.  R copies of S * S bins (packed: two to a word) and a
    256-word table fit 80 KiB of LDS for R <= 2 and the packed R = 4, 160 KiB
    for R = 4 and the packed R = 8."""
    env = env or {}
    if S > SPAN_MAX or env.get("BPE_HIST_SPAN", "1") == "0":
        return 0
    if "BPE_HIST_SKEW" in env:
        skew = env["BPE_HIST_SKEW"] != "0"
    R = max(1, int(env.get("BPE_HIST_R", "2")))
    form = env.get("BPE_HIST_FORM", "v")

    def fits(words, limit):
        return (words + 256) * 4 <= limit

    if form == "v":
        R = 4 if R >= 4 else 2 if R >= 2 else 1
        while R > 1 and not fits(R * S * S, LDS_LARGE if R == 4 else LDS_SMALL):
            R >>= 1
        return (300 if skew else 200) + R
    W = (S * S + 1) // 2
    if form == "pk":
        if R >= 8 and fits(8 * W, LDS_LARGE):
            return 108
        if fits(4 * W, LDS_SMALL):
            return 104
    R = min(R, 2)
    while R > 1 and not fits(R * S * S, LDS_SMALL):
        R >>= 1
    return R


# ------------------------------------------------------------------ the cases
# A corpus is named by a tuple (kind, args...) so that tests share its oracle
# runs through one cache; corpus(key) builds it.

def corpus(key):
    kind, args = key[0], key[1:]
    return {"planted": planted, "one": one_byte, "alt": alternating, "two": two_values, "small": small_text,
            "pair": dominant_pair, "first": dominant_first_byte, "local": locally_skewed,
            "packed": packed_word}[kind](*args)


def planted_key(n, edge, lo, S, dense=False, swap=False, tail=False):
    return ("planted", n, edge, lo, S, dense, swap, tail)


N_FORM, EDGE_FORM = 70000, TILE  # the forms' corpus: one full tile, then four full blocks and a partial one
N_SORT = 17 * TILE + 3           # 18 tiles, two pairs in the last
N_SORT17 = 16 * TILE + 12        # 17 tiles, eleven pairs in the last
N_TILES3 = 3 * (1 << 20) + 5     # the sort-tile knob's corpus
N_FOLD = 4 * (1 << 20) + 3       # the packed folds' one-byte corpus
N_PACKED = (1 << 20) + 77
N_SHARD, SHARD_CUTS = 2 * TILE + 3, [0, TILE + 1, TILE + 1 + 1025, 2 * TILE + 3]

SKEWED_KEYS = [("one", N_FORM), ("alt", N_FORM), ("pair", N_FORM)]

# (lo, S, dense, knobs, code): the issue's table of forms, each on the planted corpus in both orientations
FORM_TABLE = [
    (32, 95, False, {}, 202),
    (32, 100, False, {}, 202),
    (32, 101, False, {}, 201),
    (1, 128, False, {}, 201),
    (32, 95, False, {"BPE_HIST_R": "4"}, 204),
    (32, 100, False, {"BPE_HIST_R": "4"}, 204),
    (32, 101, False, {"BPE_HIST_R": "4"}, 201),
    (32, 95, False, {"BPE_HIST_R": "1"}, 201),
    (32, 95, False, {"BPE_HIST_SKEW": "1", "BPE_HIST_R": "1"}, 301),
    (32, 95, False, {"BPE_HIST_SKEW": "1"}, 302),
    (32, 95, False, {"BPE_HIST_SKEW": "1", "BPE_HIST_R": "4"}, 304),
    (32, 95, False, {"BPE_HIST_FORM": "span"}, 2),
    (32, 95, False, {"BPE_HIST_FORM": "span", "BPE_HIST_R": "1"}, 1),
    (1, 128, False, {"BPE_HIST_FORM": "span"}, 1),
    (32, 95, False, {"BPE_HIST_FORM": "pk"}, 104),
    (32, 100, False, {"BPE_HIST_FORM": "pk"}, 104),
    (32, 95, False, {"BPE_HIST_FORM": "pk", "BPE_HIST_R": "8"}, 108),
    (32, 100, False, {"BPE_HIST_FORM": "pk", "BPE_HIST_R": "8"}, 108),
    (32, 101, False, {"BPE_HIST_FORM": "pk"}, 1),
    (1, 128, False, {"BPE_HIST_FORM": "pk"}, 1),
    (32, 95, False, {"BPE_HIST_SPAN": "0"}, 0),
    (1, 129, True, {}, 0),
    (1, 255, True, {}, 0),
]

# (lo, S, dense, knobs): alphabet edges under the default knobs; the dense A = 128 case also under
# BPE_HIST_SPAN=0, where its A * A = 16384 keys are exactly one bin part of the generic form
ALPHABET_CASES = [
    (1, 128, False, {}), (128, 128, False, {}), (1, 129, False, {}), (1, 255, False, {}), (1, 100, False, {}),
    (1, 101, False, {}), (1, 128, True, {}), (1, 128, True, {"BPE_HIST_SPAN": "0"}), (1, 129, True, {}),
    (1, 255, True, {}),
]

# (n - 1) % TILE of the size cases, on top of one and of two full tiles
RESIDUES = [0, 1, 1023, 1024, 1025, 15 * 1024 + 7, 16 * 1024, 16 * 1024 + 1, 17 * 1024 + 5, 32 * 1024 + 1, 33 * 1024]
EDGE_KINDS = ["tile", "last_full_block", "last_pair", "lane", "block"]
SIZE_FORMS = [{}, {"BPE_HIST_SKEW": "1"}, {"BPE_HIST_FORM": "span"}, {"BPE_HIST_FORM": "pk"}]
TINY = [2, 3, 4, 5, 16, 17]


def edge_at(kind, n, tiles):
    """the planted edge of a size case; the pair before it is the last one of
    a tile, of the last full 1-KB block, of the corpus, of a lane's 16 bytes,
    or of the 16th block of a tile (where the waves' second round starts)"""
    base = (tiles - 1) * TILE
    return {"tile": tiles * TILE, "last_full_block": (n - 1) // BLOCK * BLOCK, "last_pair": n - 1,
            "lane": base + 7 * BLOCK + 9 * 16, "block": base + 16 * BLOCK}[kind]


def size_cases():
    """(residue, tiles, edge kind, planted key): every residue twice, on one
    and on two full tiles, with two of the five edges and both orientations;
    every edge kind meets both tile counts"""
    out = []
    for i, r in enumerate(RESIDUES):
        for v in range(2):
            tiles = 1 + (i + v) % 2
            n = tiles * TILE + r + 1
            kind = EDGE_KINDS[(i + 2 * v) % 5]
            out.append((r, tiles, kind, planted_key(n, edge_at(kind, n, tiles), 32, 95, swap=bool((i // 2 + v) % 2))))
    return out


def gpu_planted_keys():
    """every planted corpus the GPU tests train on (CPU preconditions: tests/test_init_lib.py)"""
    keys = []
    for lo, S, dense, _, _ in FORM_TABLE:
        keys += [planted_key(N_FORM, EDGE_FORM, lo, S, dense, swap) for swap in (False, True)]
    for lo, S, dense, _ in ALPHABET_CASES:
        keys += [planted_key(N_FORM, EDGE_FORM, lo, S, dense, swap) for swap in (False, True)]
    keys += [c[3] for c in size_cases()]
    keys += [planted_key(t * TILE + 1, t * TILE, 32, 95, swap=swap) for t in (1, 2) for swap in (False, True)]
    keys += [planted_key(n, 16 * TILE, 32, 95, tail=True) for n in (N_SORT, N_SORT17)]
    keys += [planted_key(N_TILES3, 2 << 20, 32, 95, tail=True), planted_key(N_SHARD, TILE, 32, 95)]
    return list(dict.fromkeys(keys))


def merge_cap(key):
    """the run's cap: at most 4 merges above 1.2 MiB, the stop rule up to SMALL bytes"""
    n = key[1]
    return 4 if n > 1200000 else -1 if n <= SMALL else CAP


@functools.lru_cache(maxsize=None)
def reference(key):
    """corpus, its pair histogram, and per mode the oracle's merges and ids
    under merge_cap(key) with the replay's count before every merge (computed
    once per corpus; nothing here touches the engine)"""
    import oracle_lib as O
    import regime_lib as RL
    data, cap = corpus(key), merge_cap(key)
    out = {"data": data, "cap": cap, "hist": pair_hist(data), "alphabet": alphabet(data), "skewed": skewed(data)}
    for name, mode in (("rule", O.RULE), ("emu", O.EMU)):
        merges, ids, _ = O.train(data, cap, mode)
        if name == "emu" and merges.shape == out["rule"][0].shape and (merges == out["rule"][0]).all():
            count = out["rule"][2]
        else:
            _, count, tok = RL.replay(data, merges)
            assert tok.size == ids.size and (tok == ids).all()  # the replay is the oracle's replace pass
        for a in (merges, ids, count):
            a.setflags(write=False)
        out[name] = (merges, ids, count)
    return out

"""The training init at its edges: every form of the count pass, the column
scan and the two-pass counting sort, on corpora built for them (init_lib).

Every run starts with the skew probe, the count pass in the form that
launch_count_pass (csrc/engine.hip) picks from the span of byte values, two
LDS bounds, the probe's verdict and the BPE_HIST_* knobs, the column sums and
scan, and k_sort_a / k_sort_b over groups of G tiles.  Each case here trains a
fresh engine in both modes and asserts, all by equality:

  * merges and ids: the oracle's (fast=True against O.RULE, default against
    O.EMU);
  * merge_log()["count"]: the replay's count before every merge;
  * the first record's distinct_pairs and tokens: numpy's pair histogram;
  * stats()["count_pass_span"]: the form the case is about, so that each test
    proves which kernel it ran.

The planted corpora tie two pairs at the top, one occurrence of one of them
ending on the edge under test (tests/test_init_lib.py holds the CPU
preconditions): an occurrence dropped or counted twice there changes the first
two logged counts, and the first merge in one of the two orientations; a
position missing from the sorted lists changes the ids."""
import numpy as np
import pytest

import init_lib as IL
from llmtokenizer_amd import api

pytestmark = pytest.mark.gpu

KNOBS = ("BPE_HIST_FORM", "BPE_HIST_R", "BPE_HIST_SKEW", "BPE_HIST_SPAN", "BPE_SORT_TILE", "BPE_SORT_G",
         "BPE_HIST_PK_SUB")
T = IL.TILE


def _env_id(env):
    return ",".join("%s=%s" % (k[4:], v) for k, v in env.items()) or "default"


def _key_id(key):
    return "-".join(str(int(x)) if not isinstance(x, str) else x for x in key)


def _set(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _train(key, env, monkeypatch, code=None):
    """train on corpus `key` under the knobs in env, in both modes; code = the
    expected form (default: what the span, the probe and the knobs select)"""
    ref = IL.reference(key)
    data, cap = ref["data"], ref["cap"]
    _set(monkeypatch, env)
    _, S, _ = ref["alphabet"]
    want = IL.form_code(S, ref["skewed"], env)
    if code is not None:
        assert want == code  # (the table's code is also what the bounds give)
    for mode in ("rule", "emu"):
        merges, ids, count = ref[mode]
        e = api.Engine(0)
        try:
            e.set_merge_log(True)
            e.load(data)
            e.train(cap, fast=mode == "rule")
            got_m, got_i, log, st = e.merges(), e.ids(), e.merge_log(), e.stats()
        finally:
            e.close()
        print(key[:3], _env_id(env), mode, "count_pass_span", st["count_pass_span"], "merges", got_m.shape[0],
              "count[:2]", log["count"][:2].tolist())
        assert st["count_pass_span"] == want
        assert log.size == got_m.shape[0]
        assert (log["count"][:2].astype(np.int64) == count[:2]).all(), (log["count"][:2], count[:2])
        assert got_m.shape == merges.shape, (got_m.shape, merges.shape)
        bad = np.flatnonzero((got_m != merges).any(axis=1))
        assert bad.size == 0, ("first differing merges", bad[:4], got_m[bad[:2]], merges[bad[:2]])
        assert (log["count"].astype(np.int64) == count).all(), np.flatnonzero(log["count"] != count)[:4]
        assert got_i.size == ids.size and (got_i == ids).all()
        if log.size:
            assert int(log["distinct_pairs"][0]) == np.count_nonzero(ref["hist"])
            assert int(log["tokens"][0]) == len(data)
    return want


# ---------------------------------------------------------------------- forms
def _form_cases():
    cases, seen = [], set()
    for lo, S, dense, env, code in IL.FORM_TABLE:
        for swap in (False, True):
            cases.append((IL.planted_key(IL.N_FORM, IL.EDGE_FORM, lo, S, dense, swap), env, code))
        for key in (("one", IL.N_FORM), ("alt", IL.N_FORM)):  # once per set of knobs
            if (key, _env_id(env)) not in seen:
                seen.add((key, _env_id(env)))
                cases.append((key, env, None))
    return cases


@pytest.mark.parametrize("key,env,code", _form_cases(), ids=lambda v: _env_id(v) if isinstance(v, dict) else
                         _key_id(v) if isinstance(v, tuple) else str(v))
def test_forms(key, env, code, monkeypatch):
    """the table of forms: the planted corpus in both orientations under every
    row (its code asserted as the table states it), the one-byte and the
    alternating corpus under every row's knobs (their span is 1 or 2 and the
    probe calls them skewed: the vector rows give 300 + R there)"""
    _train(key, env, monkeypatch, code)


@pytest.mark.parametrize("env,code", [({}, 302), ({"BPE_HIST_SKEW": "0"}, 202)], ids=["default", "plain-forced"])
@pytest.mark.parametrize("key", IL.SKEWED_KEYS, ids=_key_id)
def test_skewed_corpora(key, env, code, monkeypatch):
    """one byte, two alternating, a dominant pair: the probe picks the
    run-folding variant; BPE_HIST_SKEW=0 forces the plain one on the same data"""
    _train(key, env, monkeypatch, code)


@pytest.mark.parametrize("R,code", [("1", 301), ("2", 302), ("4", 304)])
@pytest.mark.parametrize("key", [("pair", IL.N_FORM), ("local", IL.N_SORT)], ids=_key_id)
def test_skew_variant_forced(key, R, code, monkeypatch):
    """the run-folding variant on corpora whose lanes see runs of every length
    between other pairs (its two-entry cache evicts and refills)"""
    _train(key, {"BPE_HIST_SKEW": "1", "BPE_HIST_R": R}, monkeypatch, code)


# ------------------------------------------------------------- alphabet edges
@pytest.mark.parametrize("swap", [False, True], ids=["Y-on-edge", "X-on-edge"])
@pytest.mark.parametrize("lo,S,dense,env", IL.ALPHABET_CASES,
                         ids=["%d+%d%s%s" % (c[0], c[1], "-dense" * c[2], "-generic" * bool(c[3]))
                              for c in IL.ALPHABET_CASES])
def test_alphabet_edges(lo, S, dense, env, swap, monkeypatch):
    """spans of 100 / 101 (the LDS bound of two copies), 128 / 129 (the widest
    span form / the generic form), a span that ends at byte 255; dense
    alphabets of 128, 129 and 255 values: one, two and four bin parts"""
    code = _train(IL.planted_key(IL.N_FORM, IL.EDGE_FORM, lo, S, dense, swap), env, monkeypatch)
    assert (code == 0) == (S > IL.SPAN_MAX or bool(env))


@pytest.mark.parametrize("n", [2, 3, IL.N_FORM])
def test_one_value(n, monkeypatch):
    """S = 1, A = 1; below 4 bytes the probe samples nothing"""
    assert _train(("one", n), {}, monkeypatch) == (302 if n >= 4 else 202)


def test_span_with_holes(monkeypatch):
    """S = 128 with only its two end values present: A = 2"""
    assert _train(("two", IL.N_FORM, 1, 128), {}, monkeypatch) == 301


# ---------------------------------------------------- size and position edges
@pytest.mark.parametrize("env", IL.SIZE_FORMS, ids=_env_id)
@pytest.mark.parametrize("r,tiles,kind,key", IL.size_cases(),
                         ids=["r%d-t%d-%s-%s" % (c[0], c[1], c[2], "X" if c[3][6] else "Y") for c in IL.size_cases()])
def test_sizes(r, tiles, kind, key, env, monkeypatch):
    """(n - 1) % 65536 at and around the 1-KB block, the 16-block wave round
    and the two-block-per-wave round, on one and two full tiles, the planted
    edge on a tile, block, lane or corpus end"""
    _train(key, env, monkeypatch)


@pytest.mark.parametrize("tiles", [1, 2])
def test_last_token_after_a_reload(tiles, monkeypatch):
    """n - 1 an exact number of tiles: the corpus's last token lies one past
    the last tile's pair positions, and the sort's first pass still has to
    write it.  One engine trains on two corpora of that size whose last pairs
    differ: a last token left over from the first run would show in the
    second run's ids (on a fresh engine it is whatever the allocation held)"""
    _set(monkeypatch, {})
    n = tiles * T + 1
    e = api.Engine(0)
    try:
        for swap in (False, True, False):
            ref = IL.reference(IL.planted_key(n, n - 1, 32, 95, swap=swap))
            merges, ids, count = ref["rule"]
            e.set_merge_log(True)
            e.load(ref["data"])
            e.train(ref["cap"], fast=True)
            got_m, got_i, log = e.merges(), e.ids(), e.merge_log()
            assert got_m.shape == merges.shape and (got_m == merges).all()
            assert (log["count"].astype(np.int64) == count).all()
            assert got_i.size == ids.size and (got_i == ids).all(), (got_i[-4:], ids[-4:])
    finally:
        e.close()


@pytest.mark.parametrize("env", IL.SIZE_FORMS, ids=_env_id)
@pytest.mark.parametrize("n", IL.TINY)
def test_tiny(n, env, monkeypatch):
    for key in (("one", n), ("small", n)):
        _train(key, env, monkeypatch)


# ----------------------------------------------------------------------- sort
@pytest.mark.parametrize("n,G", [(IL.N_SORT, "1"), (IL.N_SORT, "3"), (IL.N_SORT, "16"), (IL.N_SORT17, "3"),
                                 (IL.N_SORT17, "16")])
def test_sort_groups(n, G, monkeypatch):
    """18 and 17 tiles in groups of 1, 3 and 16: the planted edge at 16 * 65536
    is a tile edge and a group edge; the last tile holds a few pairs, the last
    of them planted, and is the last of a partial group for 18 tiles in 16s
    and 17 in 3s"""
    _train(IL.planted_key(n, 16 * T, 32, 95, tail=True), {"BPE_SORT_G": G}, monkeypatch, 202)


@pytest.mark.parametrize("tile", ["131072", "1048576"])
def test_sort_tile(tile, monkeypatch):
    """3 MiB + 5 bytes in tiles of 128 Ki and 1 Mi positions (4 merges)"""
    _train(IL.planted_key(IL.N_TILES3, 2 << 20, 32, 95, tail=True), {"BPE_SORT_TILE": tile}, monkeypatch, 202)


@pytest.mark.parametrize("env", [{}, {"BPE_SORT_TILE": "1048576"}], ids=_env_id)
@pytest.mark.parametrize("key,code", [(("one", IL.N_SORT), 302), (("first", IL.N_SORT), 202)], ids=["one", "first"])
def test_sort_skewed(key, code, env, monkeypatch):
    """one first byte in all or half of the pairs: the probe's skew[2] cuts the
    groups to 4 and 8 tiles (18 tiles: a partial last group), and to 1 under
    1 Mi-position tiles"""
    _train(key, env, monkeypatch, code)


def test_locally_skewed(monkeypatch):
    """a 50000-byte run inside 1.1 MB of random text: the probe says unskewed,
    so the plain vector form and the sort's one-by-one ranking meet the run"""
    _train(("local", IL.N_SORT), {}, monkeypatch, 202)


# --------------------------------------------------------------- packed folds
@pytest.mark.parametrize("R,code", [("4", 104), ("8", 108)])
@pytest.mark.parametrize("key", [("one", IL.N_FOLD), ("packed", IL.N_PACKED)], ids=["one-4M", "packed-word"])
def test_packed_folds(key, R, code, monkeypatch):
    """1 Mi-position tiles: a block folds its 16-bit bins after every sub-tile.
    One byte: every add of a lane class lands in one bin, 32768 per sub-tile
    (the documented bound).  Packed word: both halves of one word are hot."""
    _train(key, {"BPE_HIST_FORM": "pk", "BPE_HIST_R": R, "BPE_SORT_TILE": "1048576"}, monkeypatch, code)


# --------------------------------------------------------------- sharded init
@pytest.mark.parametrize("env,code", [({}, 202), ({"BPE_HIST_FORM": "span"}, 2)], ids=["default", "span"])
def test_sharded_init(env, code, monkeypatch):
    """three shards on one device: one of 65537 bytes (one tile's pairs
    exactly, the planted pair its last) and one of 1025 (one 1-KB block's)"""
    key = IL.planted_key(IL.N_SHARD, T, 32, 95)
    ref = IL.reference(key)
    _set(monkeypatch, env)
    merges, ids, _ = ref["rule"]
    g = api.ShardGroup(0, local_shards=3)
    try:
        g.load_split(ref["data"], IL.SHARD_CUTS)
        g.train(ref["cap"])
        got_m, got_i, st = g.merges(), g.all_ids(), g.stats()
    finally:
        g.close()
    assert st["count_pass_span"] == code
    assert got_m.shape == merges.shape and (got_m == merges).all(), np.flatnonzero((got_m != merges).any(axis=1))[:4]
    assert got_i.size == ids.size and (got_i == ids).all()

"""CPU preconditions of the init corpora (tests/init_lib.py): numpy and the
oracle only, no engine.  tests/test_gpu_init.py trains on these corpora and
relies on what is asserted here: that the two planted pairs tie at the top, so
that one occurrence dropped or doubled at the edge changes the first merge or
its logged count; that the probe's verdict on each skewed corpus is the one
its test expects; and that the form codes the GPU tests assert are the
issue's table."""
import numpy as np
import pytest

import init_lib as IL
import oracle_lib as O
import regime_lib as RL


def _pre_planted(key, modes=(O.RULE, O.EMU)):
    _, n, edge, lo, S, dense, swap, tail = key
    data = IL.corpus(key)
    assert len(data) == n
    c = IL.plant_count(n)
    on_edge, other = IL.planted_pairs(lo, S, swap)
    a = np.frombuffer(data, dtype=np.uint8)
    # the straddling pair is the last pair before the edge, with no other plant near it
    assert (a[edge - 1], a[edge]) == on_edge
    near = a[max(0, edge - 5): edge - 1].tolist() + a[edge + 1: edge + 5].tolist()
    assert not set(near) & set(on_edge + other), near
    if tail:
        assert (a[n - 2], a[n - 1]) == other
    # the four planted bytes occur nowhere else
    for v in on_edge + other:
        assert np.count_nonzero(a == v) == c, v
    assert IL.alphabet(data)[:2] == (lo, S)
    if dense:
        assert IL.alphabet(data)[2] == S
    hist = IL.pair_hist(data)
    top = np.sort(hist)[::-1]
    assert hist[on_edge[0] * 256 + on_edge[1]] == c and hist[other[0] * 256 + other[1]] == c
    assert top[0] == c and top[1] == c and top[2] * 2 <= c, top[:4]
    assert not IL.skewed(data)
    # the oracle's first two merges are the two planted pairs, c occurrences each; which of them wins the
    # tie is the tie rule's business (the smaller hash bucket), not the corpus's
    winner = {}
    for mode in modes:
        m, _, _ = O.train(data, 2, mode)
        assert sorted(m.tolist()) == sorted([list(on_edge), list(other)]), m
        _, count, _ = RL.replay(data, m)
        assert count.tolist() == [c, c]
        winner[mode] = tuple(m[0].tolist())
    return winner


@pytest.mark.parametrize("key", IL.gpu_planted_keys(), ids=lambda k: "-".join(str(int(x)) for x in k[1:]))
def test_planted_preconditions(key):
    _pre_planted(key)


@pytest.mark.parametrize("n,edge", [(65538, 65536), (65537, 65536), (131075, 131072), (5000, 1024), (70000, 69999)])
@pytest.mark.parametrize("swap", [False, True])
def test_planted_recipe(n, edge, swap):
    """the recipe at further (n, edge) pairs, among them the smallest corpus
    it is used at and an edge that is the corpus's last pair"""
    _pre_planted(IL.planted_key(n, edge, 32, 95, swap=swap))


@pytest.mark.parametrize("lo,S,dense", sorted({row[:3] for row in IL.FORM_TABLE + IL.ALPHABET_CASES}))
def test_planted_orientations(lo, S, dense):
    """the same pair wins the tie in both orientations (the schedule-free rule
    looks at the pairs' hash buckets only), so the straddling pair is the
    tie's winner in one orientation and its loser in the other"""
    w = [_pre_planted(IL.planted_key(IL.N_FORM, IL.EDGE_FORM, lo, S, dense, swap), modes=(O.RULE,))[O.RULE]
         for swap in (False, True)]
    assert w[0] == w[1]


def test_planted_breaks_show():
    """what the GPU tests rely on: without the edge occurrence the first merge
    changes in one orientation, with it counted twice in the other, and the
    first two counts change in both"""
    key = IL.planted_key(IL.N_FORM, IL.EDGE_FORM, 32, 95)
    win = O.train(IL.corpus(key), 2, O.RULE)[0][0].tolist()
    changed = {}
    for swap in (False, True):
        key = IL.planted_key(IL.N_FORM, IL.EDGE_FORM, 32, 95, swap=swap)
        a = np.frombuffer(IL.corpus(key), dtype=np.uint8)
        c = IL.plant_count(IL.N_FORM)
        filler = a[100]
        dropped = a.copy()
        dropped[IL.EDGE_FORM - 1: IL.EDGE_FORM + 1] = filler
        doubled = a.copy()
        doubled[IL.EDGE_FORM + 3: IL.EDGE_FORM + 5] = a[IL.EDGE_FORM - 1: IL.EDGE_FORM + 1]
        for name, b in (("dropped", dropped), ("doubled", doubled)):
            m, _, _ = O.train(b.tobytes(), 2, O.RULE)
            _, count, _ = RL.replay(b.tobytes(), m)
            assert count.tolist() != [c, c]
            changed[name, swap] = m[0].tolist() != win
    # the tie's winner loses merge 0 when its edge occurrence is dropped, and when the loser's is doubled
    assert changed["dropped", False] != changed["dropped", True]
    assert changed["doubled", False] != changed["doubled", True]
    assert changed["dropped", False] != changed["doubled", False]


def test_skewed_corpora():
    for key in IL.SKEWED_KEYS + [("one", IL.N_SORT), ("one", IL.N_FOLD), ("two", IL.N_FORM, 1, 128),
                                 ("packed", IL.N_PACKED)]:
        assert IL.skewed(IL.corpus(key)), key
    for key in [("first", IL.N_SORT), ("local", IL.N_SORT)]:
        assert not IL.skewed(IL.corpus(key)), key
    # below 4 bytes the probe samples nothing
    assert IL.probe(IL.one_byte(3)) == (0, 0, 0) and IL.probe(IL.one_byte(4)) == (3, 3, 3)
    assert IL.alphabet(IL.one_byte(IL.N_FORM)) == (97, 1, 1)
    assert IL.alphabet(IL.alternating(IL.N_FORM)) == (97, 2, 2)
    assert IL.alphabet(IL.corpus(("two", IL.N_FORM, 1, 128))) == (1, 128, 2)
    assert IL.alphabet(IL.dominant_pair(IL.N_FORM)) == (32, 95, 95)
    h = IL.pair_hist(IL.dominant_pair(IL.N_FORM))
    assert h[101 * 256 + 32] * 16 > IL.N_FORM - 1
    # a dominant first byte: half the sampled pairs, which shrinks the sort's groups; no dominant pair
    top, tot, first = IL.probe(IL.dominant_first_byte(IL.N_SORT))
    assert first * 4 > tot and top * 32 < tot
    # the run is skewed for the blocks that hold it, not for the sample of the whole corpus
    data = IL.locally_skewed(IL.N_SORT)
    assert IL.skewed(data[300001: 300001 + 50000]) and len(data) <= 1200000
    assert IL.pair_hist(data)[97 * 256 + 97] >= 49999


def test_packed_word_corpus():
    data = IL.packed_word(IL.N_PACKED)
    lo, S, A = IL.alphabet(data)
    assert (lo, S) == (32, 95) and len(data) <= 1200000
    b0, b1 = IL.packed_bin((100, 100), lo, S), IL.packed_bin((100, 101), lo, S)
    assert (b0 ^ b1) == 1  # the two bins are the halves of one packed word
    h = IL.pair_hist(data)
    npairs = len(data) - 1
    assert h[100 * 256 + 100] * 4 > npairs and h[100 * 256 + 101] * 4 > npairs


def test_form_codes_are_the_table():
    """form_code() gives the issue's table, row by row, on the planted corpus
    (unskewed) and on the skewed corpora"""
    for lo, S, dense, env, code in IL.FORM_TABLE:
        assert IL.form_code(S, False, env) == code, (S, env, code)
    for S in (1, 2, 95):  # one byte, alternating, dominant pair
        assert IL.form_code(S, True) == 302 and IL.form_code(S, True, {"BPE_HIST_SKEW": "0"}) == 202
    codes = {row[4] for row in IL.FORM_TABLE}
    assert codes == {0, 1, 2, 104, 108, 201, 202, 204, 301, 302, 304}


def test_size_cases_cover_the_edges():
    cases = IL.size_cases()
    assert {(r, t) for r, t, _, _ in cases} == {(r, t) for r in IL.RESIDUES for t in (1, 2)}
    assert {(k, t) for _, t, k, _ in cases} == {(k, t) for k in IL.EDGE_KINDS for t in (1, 2)}
    assert {key[6] for _, _, _, key in cases} == {False, True}
    for r, tiles, kind, key in cases:
        n, edge = key[1], key[2]
        assert (n - 1) % IL.TILE == r and (n - 1) // IL.TILE == tiles and n <= 1200000
        assert 1 <= edge <= n - 1
        if kind == "tile":
            assert edge % IL.TILE == 0
        elif kind == "last_full_block":
            assert edge % IL.BLOCK == 0 and n - 1 - edge < IL.BLOCK
        elif kind == "last_pair":
            assert edge == n - 1
        elif kind == "lane":
            assert edge % 16 == 0 and edge % IL.BLOCK != 0
        else:
            assert edge % IL.BLOCK == 0 and edge % IL.TILE == 16 * IL.BLOCK
    # the sort's corpora: 17 * 65536 + 3 bytes are 18 tiles, the last of two pairs (no multiple of the group
    # sizes 16, nor of the 4 and 8 that skew[2] leaves); 16 * 65536 + 12 bytes are 17 (no multiple of 3 either)
    assert (IL.N_SORT - 2) // IL.TILE + 1 == 18 and (IL.N_SORT17 - 2) // IL.TILE + 1 == 17
    # the sharded run's cuts: a shard of one tile's pairs exactly, and one of a single 1-KB block's
    cuts = IL.SHARD_CUTS
    assert cuts[1] - cuts[0] == IL.TILE + 1 and cuts[2] - cuts[1] == 1025 and cuts[3] == IL.N_SHARD

"""BPE_SPLIT_O200K on the device (split_o200k.hip: k_o2_summary, the scan of the wave tiles' maps,
k_split_mark_o200k): the offsets equal api.split_host(data, "o200k"), bit for bit, which
tests/test_split_o200k_host.py pins to the regular expression.  The probes put every chain that no window bounds
across every edge of the geometry: 16 bytes a thread, 1,024 a wave, a tile a workgroup, a grid step.  The
composition of the maps has no host probe: it is covered here, by the runs longer than a grid step, whose state
passes through the wave scan and the scan of the tiles at every residue."""
import numpy as np
import pytest

import train_split_ref as R
from llmtokenizer_amd import api

pytestmark = pytest.mark.gpu

RULE = "o200k"
EOT = b"<|endoftext|>"
M = "́".encode()
ITEMS = [b"'", b"s", b"T", b"re", b"LL", b"v", b"a", b"Z", b"AB", b"1", b"23", b"4567", b"!", b"/", b"\n", b"\r\n", b" ", b"  ",
         b"\t", b"word", b" The", b"!\n", b" \n", b"/\n/"]
ITEMS += [s.encode() for s in ("ſ", "é", "Ж", "ǅ", "ʰ", "中", "́", "\U00010400", "٣", "½", " ", "　", "—", "\U0001f600")]
ITEMS += [b"\x80", b"\xc3", b"\xe2\x82", b"\xf0\x9f\x98", b"\xff"]


def mixed(n, seed):
    """n bytes of the items above in random order (cut at n: the text may end inside a sequence)"""
    rng = np.random.default_rng(seed)
    out, size = [], 0
    while size < n:
        for k in rng.integers(0, len(ITEMS), 4096).tolist():
            out.append(ITEMS[k])
            size += len(ITEMS[k])
    return b"".join(out)[:n]


@pytest.fixture(scope="module")
def eng():
    e = api.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def geo():
    g = api.split_info()
    return g["tile"], g["grid_bytes"]


def _same(eng, data, what=None, specials=None):
    eng.load(data)
    nd = eng.split(RULE, specials)
    got = eng.split_offsets()
    want = api.split_host(data, RULE) if specials is None else api.split_host_special(data, RULE, specials)[0]
    assert got.size == nd + 1 == want.size and (got == want).all(), what if what is not None else len(data)


def _edges(tile):
    """-4..+4 around every 16-byte edge up to 64, 1,024 and the tile"""
    return sorted({c + d for c in (16, 32, 48, 64, 1024, tile) for d in range(-4, 5)})


@pytest.mark.parametrize("n", [0, 1, 15, 16, 17, 1023, 1024, 1025, -1, 0x10000, 0x10001])
def test_offsets_equal_the_host_definition(eng, geo, n):
    n = {-1: geo[0] - 1, 0x10000: geo[0], 0x10001: geo[0] + 1}.get(n, n)
    for seed in range(4):
        _same(eng, mixed(n, 100 * n + seed), (n, seed))


PROBES = {
    "aBBBA": ["a中中中A".encode(), "aʰ".encode() + M * 3 + b"Ab"],
    "ABBA.": ["A中中A.".encode(), "A中ʰA".encode(), b"A" + M * 2 + b"AA!"],
    "BAAAA.": ["中AAAA.".encode(), "a中AAAA ".encode(), "中AAAAa".encode()],
    "x's's's'sb": [b"x's's's'sb", b"x's's's's'sb", "x'ſ'S't'db".encode()],
    "A'LL'LL'LLb": [b"A'LL'LL'LLb", b"a'll're've'llb", b"A'LL'L'LLb"],
    "!!Mx": [b"!!" + M * k + b"x" for k in (1, 2, 9)] + [b"a!" + M * k + b"x" for k in (1, 2, 9)] + [b" !" + M * 3 + b"x"],
    "!n/n/!": [b"!\n/\n/!", b"a\n/\n/!", b"!\r\n//\n/x", b"a\n//x"],
    "numbers": [b"1" * k for k in range(1, 8)] + ["٣7½".encode() * 2],
    "!nn ": [b"!\n\n ", b"!\n\n  \nx", b"a\n\n  x", b"!/\n \n"],
    "n spaces": [b"\n   x", b"\n  \n  ", b" \n \n !", "\n 　x".encode()],
}


@pytest.mark.parametrize("chain", sorted(PROBES))
def test_every_chain_across_every_edge(eng, geo, chain):
    n = geo[0] + 96
    for probe in PROBES[chain]:
        for fill in (b"a", b" "):
            for p in _edges(geo[0]):
                buf = bytearray(fill * n)
                buf[p:p + len(probe)] = probe
                _same(eng, bytes(buf[:n]), (probe, fill, p))


LONG = {  # head, the unit of the run, tail
    "numbers 0": (b"a", b"1", b"x"), "numbers 1": (b"a1", b"1", b"x"), "numbers 2": (b"a11", b"1", b"x"),
    "contraction phase 0": (b"a", b"'s", b"b"), "contraction phase 1": (b"a'", b"s'", b"sb"), "contraction 'll": (b"A", b"'LL", b"b"),
    "U run to its end": ("a中".encode(), b"A", b"."), "U run to a": ("a中".encode(), b"A", b"a"),
    "B run behind a": (b"a", "中".encode(), b"A."), "B run behind A": (b"A", "中".encode(), b"A."),
    "M run behind !!": (b"!!", M, b"x"), "M run behind a!": (b"a!", M, b"x"),
    "tail behind !": (b"!", b"\n/", b"!x"), "tail behind a": (b"a", b"\n/", b"!x"),
    "newlines behind !": (b"!", b"\n", b"  x"), "spaces before a newline": (b"a\n", b" ", b"\nx"), "spaces": (b"a\n", b" ", b"x"),
}


@pytest.mark.parametrize("chain", sorted(LONG))
def test_one_run_longer_than_a_grid_step(eng, geo, chain):
    head, unit, tail = LONG[chain]
    reps = (geo[1] + 5) // len(unit) + 1
    _same(eng, head + unit * reps + tail, chain)


@pytest.mark.parametrize("end", [b"it's", b"it'", b"we'l", b"we'll", "aé".encode()[:-1], "a中".encode()[:-1], "a\U0001f600".encode()[:-2]])
def test_the_text_ends_inside_a_contraction_or_a_character(eng, geo, end):
    for n in (16, 1024, geo[0]):
        _same(eng, (b"ab " * n)[:n - len(end)] + end, (end, n))


@pytest.mark.parametrize("pos", [5, 1023, 1030, -1])
def test_one_character_beyond_ascii_in_an_ascii_wave(eng, geo, pos):
    pos = 2 * geo[0] + 100 if pos < 0 else pos
    for ch in ("É", "中", "́", "\U0001f600"):
        buf = bytearray((b"Ab c!" * (3 * geo[0]))[:3 * geo[0]])
        buf[pos:pos + len(ch.encode())] = ch.encode()
        _same(eng, bytes(buf), (ch, pos))


@pytest.mark.parametrize("run", ["AAAA", "a's's's's", "!" + "́" * 6, "!\n/\n/\n", "1111111", "\n    ", "ab "])
def test_a_special_at_the_edges_and_inside_every_run(eng, geo, run):
    unit = run.encode()
    for edge in (64, 1024, geo[0]):
        for d in (-len(EOT), -3, 0, 2):
            buf = bytearray((unit * (2 * geo[0]))[:geo[0] + 200])
            buf[edge + d:edge + d + len(EOT)] = EOT
            _same(eng, bytes(buf), (run, edge, d), [EOT])


def test_encode_and_train_equal_their_restatements_over_the_host_pieces(eng):
    data = mixed(0x10000, 3)
    off = api.split_host(data, RULE)
    pieces = [data[int(a):int(b)] for a, b in zip(off, off[1:])]
    merges = api.train_split(data, rule=RULE, max_merges=60)
    assert [tuple(m) for m in merges.tolist()] == R.train(pieces, 60)[0]
    ids, id_off, byte_off = api.encode_split(data, merges, rule=RULE)
    want, want_off = api.encode_batch(pieces, merges)
    assert (byte_off == off).all() and (id_off == want_off).all() and (ids == want).all()

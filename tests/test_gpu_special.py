"""Special tokens on the device (special.hip, bpe_gpu_split_special & co.): the offsets and the
special pieces equal the host definition (api.split_host_special, held to the Python restatement
by tests/test_special_host.py), encode_split leaves one reserved id per special piece and
encode_batch's ids for every other piece, train_split trains on the ordinary pieces alone,
decode_batch gives the pieces back, and the specials live and die with the split's offsets."""
import ctypes
import random

import numpy as np
import pytest

import golden_lib as G
import special_ref as R
import train_split_ref as TR
from llmtokenizer_amd import api
from llmtokenizer_amd.synth import english_like

pytestmark = pytest.mark.gpu

T, GB = 4096, 4096 * 2048  # bpe_gpu.h BPE_GPU_SPLIT_TILE, and the bytes one grid step covers (test_gpu_split.py)
EOT = b"<|endoftext|>"
LONG = b"<" + b"0123456789" * 6 + b"ab>"  # 64 bytes
ESTATE = "call out of order"
RULES = ["lines", "words", "gpt2", R.random_rule(1), R.random_rule(2)]
ALPHA = np.frombuffer(b"ab  '\n\tst1<|>e", np.uint8)


@pytest.fixture(scope="module")
def eng():
    e = api.Engine(0)
    yield e
    e.close()


def cut(data, off):
    return [data[int(a):int(b)] for a, b in zip(off, off[1:])]


def text(n, seed, specials, every=40):
    """n bytes over ALPHA with a special about every `every` bytes (a block of at most 64 KiB, tiled)"""
    rng = np.random.default_rng(seed)
    parts, total = [], 0
    while total < min(n, 1 << 16) + 64:
        parts.append(rng.choice(ALPHA, int(rng.integers(0, 2 * every))).tobytes())
        parts.append(specials[int(rng.integers(0, len(specials)))])
        total += len(parts[-2]) + len(parts[-1])
    block = b"".join(parts)
    return (block * (n // len(block) + 1))[:n]


def check_split(eng, data, rule, specials, what=None):
    """one split of the loaded bytes against the host definition; returns (offsets, pieces, indices)"""
    want, piece, index = api.split_host_special(data, rule, specials)
    assert eng.split(rule, specials) == want.size - 1, what
    got = eng.split_offsets()
    assert got.dtype == np.uint64 and got.size == want.size and (got == want).all(), what
    gp, gi = eng.special_pieces()
    assert gp.tolist() == piece.tolist() and gi.tolist() == index.tolist(), what
    info = eng.split_special_info()
    assert info["specials"] == len(specials) and info["matches"] == piece.size, what
    return want, piece, index


# ---------------------------------------------------------------- the split

SIZES = [15, 16, 17, 1023, 1024, 1025, T - 1, T, T + 1, GB - 1, GB, GB + 1, GB + 3]


@pytest.mark.parametrize("n", SIZES)
def test_offsets_equal_the_host_definition(eng, n):
    assert api.split_info()["grid_bytes"] == GB
    specials = R.CHATML_SET[:3]
    data = text(n, 100 + n % 977, specials)
    eng.load(data)
    for k, rule in enumerate(RULES):
        _, piece, _ = check_split(eng, data, rule, specials, what=(n, k))
        assert piece.size > 0 or n < 64


BEFORE = [b"a'", b"  ", b" \n", b"1 "]
AFTER = [b"'s x", b"  a", b" \na", b"'ll", b" 's"]


@pytest.mark.parametrize("special", [EOT, LONG], ids=["13", "64"])
def test_a_match_around_every_edge(eng, special):
    """a match starting at -66..+6 of the 16-byte edges up to 128, of 1,024 and of the tile; the bytes next
    to it are what BPE_SPLIT_GPT2 decides again at s - 1 and e .. e + 3: 's, two spaces, space-newline"""
    rng = np.random.default_rng(5)
    stride = 16 * ((len(special) + 15) // 16)  # small edges that one text can hold without its matches touching
    for d in range(-66, 7):
        for first in range(16, 16 + stride, 16):
            edges = [e for e in range(first, 129, stride)] + [1024, T]
            buf = bytearray(rng.choice(ALPHA, T + 200).tobytes())
            for e in edges:
                s = e + d
                if s < 0:
                    continue
                b, a = BEFORE[(d + e // 16) % len(BEFORE)], AFTER[(d + e // 16) % len(AFTER)]
                buf[s:s + len(special)] = special
                buf[s + len(special):s + len(special) + len(a)] = a
                if s >= len(b) and d % 2:
                    buf[s - len(b):s] = b
            data = bytes(buf)
            eng.load(data)
            for rule in ("words", "gpt2"):
                check_split(eng, data, rule, [special], what=(d, first, rule))


def test_adjacent_matches_and_short_segments(eng):
    sp = [EOT, b"<|im_end|>", b"\x01"]
    for fill in (b"a's  \n x", b"  \n\n 's", b"'ll 1 ", b"\n'd 't"):
        for n in range(0, 6):
            seg = (fill * 2)[:n]
            data = (EOT + seg + sp[1] + seg + sp[2] + seg + EOT + seg) * 3 + EOT
            eng.load(data)
            for rule in ("lines", "words", "gpt2"):
                check_split(eng, data, rule, sp, what=(fill, n, rule))


def test_a_text_ending_in_a_prefix_of_a_special(eng, tmp_path):
    """no match where the text ends inside a special.  The loaders zero the 64 bytes past n, so the rest
    of the special cannot be left there through the API; the file below has it right after the NUL that
    ends the text, which is as close as a caller gets."""
    for k in range(1, len(EOT)):
        for head in (b"", b"ab " * 5 + EOT + b" ", b"x" * 15, b"y" * (T - k)):
            data = head + EOT[:k]
            eng.load(data)
            for rule in ("words", "gpt2"):
                _, piece, _ = check_split(eng, data, rule, [EOT], what=(k, len(head)))
                assert piece.size == head.count(EOT)
    p = tmp_path / "cut.txt"
    data = b"ab " * 7 + EOT + b" x" + EOT[:9]
    p.write_bytes(data + b"\0" + EOT[9:] + b" tail")
    assert eng.load_file(str(p)) == len(data)
    check_split(eng, data, "gpt2", [EOT])


def test_256_specials_sharing_a_27_byte_prefix(eng):
    prefix = b"<|reserved_special_token_xx"
    assert len(prefix) == 27
    specials = [prefix + b"%03d|>" % i for i in range(256)]
    api.check_specials(specials)
    rng = np.random.default_rng(9)
    parts = []
    for i in rng.permutation(256).tolist() + [0, 255, 128]:
        parts += [specials[i], rng.choice(ALPHA, int(rng.integers(0, 9))).tobytes(), prefix[: int(rng.integers(1, 28))]]
    data = b"".join(parts)
    eng.load(data)
    for rule in ("words", "gpt2"):
        _, piece, index = check_split(eng, data, rule, specials)
        assert piece.size == 259 and sorted(set(index.tolist())) == list(range(256))
    check_split(eng, data, "gpt2", R.RESERVED_SET)


def test_only_candidates_and_only_matches(eng):
    data = b"<" * (T + 17)
    eng.load(data)
    _, piece, _ = check_split(eng, data, "gpt2", R.CHATML_SET)
    assert piece.size == 0
    data = EOT * 700
    eng.load(data)
    for rule in ("words", "gpt2"):
        off, piece, _ = check_split(eng, data, rule, [EOT])
        assert piece.tolist() == list(range(700)) and off.size == 701
    assert eng.split_special_info()["find_passes"] == 1
    data = b"\x01" * 5000  # more matches than the match list first has room for
    eng.load(data)
    _, piece, _ = check_split(eng, data, "words", [b"\x01"])
    assert piece.size == 5000 and eng.split_special_info()["find_passes"] == 2


def test_no_specials_is_the_plain_split(eng):
    data = text(3 * T + 5, 3, [EOT])
    eng.load(data)
    for rule in RULES[:4]:
        n = eng.split(rule)
        plain = eng.split_offsets()
        assert eng.split(rule, []) == n and (eng.split_offsets() == plain).all()
        assert eng.special_pieces()[0].size == 0 and eng.split_special_info()["specials"] == 0


# ---------------------------------------------------------------- encode

def _random_merges(rng, alphabet, k, eq=0.3):
    """as tests/test_gpu_split.py builds them (a == a records included)"""
    ids = list(alphabet)
    out = []
    for r in range(k):
        u, v = rng.choice(ids), rng.choice(ids)
        if rng.random() < eq:
            v = u
        out.append((u, v))
        ids.append(256 + r)
    return np.array(out, dtype=np.uint32).reshape(-1, 2)


def expected_ids(data, rule, merges, specials):
    """(ids, id offsets, byte offsets): [256 + k + j] for a special piece, encode_batch of the others"""
    off, piece, index = api.split_host_special(data, rule, specials)
    pieces = cut(data, off)
    which = dict(zip(piece.tolist(), index.tolist()))
    plain = [p for i, p in enumerate(pieces) if i not in which]
    bids, boff = api.encode_batch(plain, merges)
    parts, k = [], 0
    for i in range(len(pieces)):
        if i in which:
            parts.append(np.array([256 + len(merges) + which[i]], np.uint32))
        else:
            parts.append(bids[int(boff[k]):int(boff[k + 1])])
            k += 1
    ids = np.concatenate(parts) if parts else np.zeros(0, np.uint32)
    return ids, np.cumsum([0] + [p.size for p in parts]).astype(np.uint64), off


def check_encode(eng, data, rule, merges, specials, what=None):
    want, want_off, want_boff = expected_ids(data, rule, merges, specials)
    eng.encode_split(merges)
    ids, id_off = eng.ids(), eng.doc_offsets()
    assert id_off.tolist() == want_off.tolist(), what
    assert ids.size == want.size and (ids == want).all(), what
    assert eng.stats()["n_out"] == ids.size
    return eng.docs_info()


@pytest.fixture(scope="module")
def english():
    base = english_like(120000)
    parts = [base[i:i + 2048] for i in range(0, len(base), 2048)]
    data = EOT.join(parts) + EOT + b"<|im_end|>" + EOT
    merges, _ = api.train_bytes(base[: 1 << 16], 300)
    return data, merges


@pytest.mark.parametrize("halo", [16, 48, 256])
@pytest.mark.parametrize("rule", ["words", "gpt2"])
def test_encode_split_english(eng, english, rule, halo, monkeypatch):
    monkeypatch.setenv("BPE_EW_HALO", str(halo))
    data, merges = english
    eng.load(data)
    eng.split(rule, R.CHATML_SET)
    info = check_encode(eng, data, rule, merges, R.CHATML_SET, what=(rule, halo))
    assert info["halo"] == halo and info["docs_fallback"] == 0
    assert (eng.ids() >= 256 + len(merges)).sum() == data.count(EOT) + 1


@pytest.mark.parametrize("halo", [16, 48, 256])
def test_encode_split_random_texts(eng, halo, monkeypatch):
    monkeypatch.setenv("BPE_EW_HALO", str(halo))
    rng = random.Random(800 + halo)
    sp = [EOT, b"\x01", LONG]
    for rule in ("lines", "gpt2", RULES[3]):
        data = text(rng.randint(6000, 9000), rng.randint(0, 999), sp, every=25)
        merges = _random_merges(rng, sorted(set(ALPHA.tolist()) | set(EOT)), rng.randint(50, 400), eq=rng.choice([0.0, 0.3]))
        eng.load(data)
        eng.split(rule, sp)
        check_encode(eng, data, rule, merges, sp, what=(halo, str(rule)[:8]))


def test_two_merge_lists_over_one_split(eng):
    """the special id moves with the length of the merge list"""
    rng = random.Random(45)
    sp = [EOT, b"<|im_end|>"]
    data = text(5000, 4, sp)
    m1 = _random_merges(rng, sorted(set(ALPHA.tolist())), 120, eq=0.3)
    m2 = _random_merges(rng, sorted(set(ALPHA.tolist())), 77, eq=0.0)
    eng.load(data)
    eng.split("gpt2", sp)
    for m in (m1, m2, m1):
        check_encode(eng, data, "gpt2", m, sp)
        ids = eng.ids()
        assert (ids == 256 + len(m)).sum() == data.count(EOT) and (ids == 256 + len(m) + 1).sum() == data.count(sp[1])
        assert ids.max() == 256 + len(m) + 1
        assert eng.ids_checksum() == G.ids_checksum(ids)


def test_no_plan_fallback(eng):
    """test_gpu_split.py's 300-deep chain: every piece goes through the fallback, then the post-pass"""
    chain = [(97, 97)] + [(256 + r, 256 + r) for r in range(299)]
    merges = np.array(chain, dtype=np.uint32)
    rng = random.Random(3)
    data = b"".join(b"a" * rng.randint(1, 40) + rng.choice([b" ", EOT, b" b", b"\n" + EOT + EOT]) for _ in range(30))
    eng.load(data)
    for rule in ("lines", "words", "gpt2"):
        eng.split(rule, [EOT])
        info = check_encode(eng, data, rule, merges, [EOT], what=rule)
        assert info["docs_fallback"] == info["ndocs"] and info["windows"] == 0


def test_partial_fallback(eng, monkeypatch):
    """test_gpu_split.py's failed windows (a run of 20001 `a` under (97, 97) inside one long piece) with
    specials among the short lines: only some pieces go through the fallback"""
    rng = random.Random(21)
    halo = 48
    monkeypatch.setenv("BPE_EW_HALO", str(halo))
    merges = np.vstack([np.array([[97, 97]], dtype=np.uint32), _random_merges(rng, sorted(set(b"ab ")), 200, eq=0.3)])
    short = [bytes(rng.choice(b"ab ") for _ in range(rng.randint(0, halo - 1))) + rng.choice([b"\n", EOT + b"\n", EOT])
             for _ in range(100)]
    data = b"".join(short[:70] + [b"." * 2100 + b"a" * 20001 + b" b" * 20 + EOT + b"\n"] + short[70:])
    eng.load(data)
    eng.split("lines", [EOT])
    info = check_encode(eng, data, "lines", merges, [EOT])
    assert info["windows_failed"] >= 1 and 1 <= info["docs_fallback"] < info["ndocs"] // 2


# ---------------------------------------------------------------- train, decode, lifetime

def test_train_split_leaves_the_specials_out(eng):
    sp = [EOT, b"<|im_end|>"]
    rng = random.Random(7)
    words = [b"ab", b"abab", b" ab", b" tex", b"\n", b" 12", b"end"]
    data = b"".join(rng.choice(words) * rng.randint(1, 3) + rng.choice([b"", EOT, sp[1], EOT + EOT]) for _ in range(400))
    off, piece, _ = api.split_host_special(data, "gpt2", sp)
    special = set(piece.tolist())
    plain = [p for i, p in enumerate(cut(data, off)) if i not in special]
    want, _, _ = TR.train(plain, 40)
    eng.load(data)
    eng.split("gpt2", sp)
    assert len(want) >= 20
    assert eng.train_split(40) == len(want)
    got = eng.split_merges()
    assert got.tolist() == [list(m) for m in want]
    info = eng.train_split_info()
    assert info["pieces"] == off.size - 1
    st, ln, ct = eng.piece_table()
    table = [data[int(s):int(s) + int(n)] for s, n in zip(st, ln)]
    assert not set(table) & set(sp) and sorted(set(table)) == sorted(set(plain))
    assert int(ct.sum()) == len(plain) == off.size - 1 - piece.size
    # the same text without specials trains on the fragments of <|endoftext|> as well
    eng.split("gpt2")
    eng.train_split(40)
    assert eng.split_merges().tolist() != got.tolist()
    assert set(b"endoftext") & {int(x) for x in eng.split_merges().reshape(-1) if x < 256}
    assert not {ord("<"), ord("|"), ord(">")} & {int(x) for x in got.reshape(-1)}
    # through the C layer (bpe_train_split_special)
    assert api.train_split(data, "gpt2", 40, specials=sp).tolist() == got.tolist()
    assert api.train_split(data, "gpt2", 40).tolist() == eng.split_merges().tolist()
    # a text of specials alone has nothing to train on
    eng.load(EOT * 5)
    eng.split("words", sp)
    assert eng.train_split(10) == 0 and eng.piece_table()[0].size == 0


def test_round_trip_and_the_c_layer(eng):
    sp = R.CHATML_SET
    rng = random.Random(8)
    data = text(4000, 12, sp)
    merges = _random_merges(rng, sorted(set(ALPHA.tolist())), 150, eq=0.3)
    for rule in ("gpt2", "words", RULES[4]):
        want, want_off, want_boff = expected_ids(data, rule, merges, sp)
        ids, id_off, byte_off = api.encode_split(data, merges, rule=rule, specials=sp)  # bpe_encode_split_special
        assert (ids == want).all() and id_off.tolist() == want_off.tolist() and byte_off.tolist() == want_boff.tolist()
        back = api.decode_batch(ids, id_off, merges, specials=sp)  # bpe_decode_docs_special
        assert back == cut(data, byte_off)
        raw, boff = eng.decode_docs(ids, id_off, merges, specials=sp)
        assert raw == data and boff.tolist() == byte_off.tolist()
    top = 256 + len(merges) + len(sp)
    assert api.decode_batch([top - 1], [0, 1], merges, specials=sp) == [sp[-1]]
    with pytest.raises(api.BpeError):
        api.decode_batch([top], [0, 1], merges, specials=sp)
    with pytest.raises(api.BpeError, match="unknown token id"):
        eng.decode_docs([97, top], [0, 2], merges, specials=sp)
    with pytest.raises(api.BpeError, match="unknown token id"):
        eng.decode_docs([256 + len(merges)], [0, 1], merges)  # without specials the id is unknown, as before


def test_lifetime(eng):
    sp = [EOT]
    rng = random.Random(9)
    data = b"ab cd" + EOT + b" ef" + EOT
    merges = _random_merges(rng, sorted(set(b"abcdef ")), 20, eq=0.0)
    eng.load(data)
    assert eng.split("gpt2", sp) == 5
    assert eng.special_pieces()[0].tolist() == [2, 4]
    # a plain split forgets the specials
    plain = api.split_host(data, "gpt2")
    assert eng.split("gpt2") == plain.size - 1
    assert eng.special_pieces()[0].size == 0 and eng.split_special_info()["specials"] == 0
    eng.encode_split(merges)
    pids, poff = api.encode_batch(cut(data, plain), merges)
    assert (eng.ids() == pids).all() and eng.doc_offsets().tolist() == poff.tolist()
    # a load drops them with the offsets
    eng.split("gpt2", sp)
    eng.load(data)
    for call in (eng.special_pieces, eng.split_special_info, lambda: eng.encode_split(merges)):
        with pytest.raises(api.BpeError, match=ESTATE):
            call()
    # the cached context of the C layer: a call without specials after one with them gives today's ids
    with_sp = api.encode_split(data, merges, rule="gpt2", specials=sp)
    without = api.encode_split(data, merges, rule="gpt2")
    assert (without[0] == pids).all() and without[1].tolist() == poff.tolist() and without[2].tolist() == plain.tolist()
    assert with_sp[0].size < without[0].size and (with_sp[0] == 256 + len(merges)).sum() == 2
    # a bad set raises before any launch: the split of before is still there
    eng.split("gpt2", sp)
    for bad in ([b"aa"], [b"<a>", b"a"], [b""], [b"x" * 65], [b"a\0"]):
        with pytest.raises(api.BpeError):
            eng.split("gpt2", bad)
    assert eng.special_pieces()[0].tolist() == [2, 4]
    # ... also past the Python check, in the engine itself
    bad = api._Specials([b"aa"])
    nd = ctypes.c_size_t(0)
    rc = eng.L.bpe_gpu_split_special(eng.ctx, 2, None, None, bad.ref, ctypes.byref(nd))
    assert rc != 0 and b"suffix" in eng.L.bpe_gpu_last_error()
    assert eng.special_pieces()[0].tolist() == [2, 4]

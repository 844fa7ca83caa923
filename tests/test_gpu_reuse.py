"""One context across runs and call orders (tests/reuse_lib.py holds the operations, the model and the sequences): no
state of an earlier call may leak into a later one.  Every expected value is a host reference's or the oracle's.

  a. every ordered pair (A, B) of state-changing calls on one context: B's result and every reader the model says is
     valid, or the refusal and a context that still works;
  b. a context that holds the pool and the scratch of a large training, then small runs at the init's tile edges in
     every table layout, and the other way round;
  c. a text batch of 300, 1, 0 and 300 texts through the whole text path;
  d. the users of the decoders' offset slot and of the scans' temporary, interleaved with shrinking and growing inputs;
  e. trim after every operation;
  f. a group of three shards trained twice with other cuts and sizes, then encoding."""
import numpy as np
import pytest

import golden_lib as G
import oracle_lib as O
import reuse_lib as R
import rows_ref
import stream_ref
import texts_ref
from llmtokenizer_amd import api
from llmtokenizer_amd.api import BpeError
from llmtokenizer_amd.synth import synth_bytes
from llmtokenizer_amd.vocab import vocab_tables

pytestmark = pytest.mark.gpu


def run_expect(eng, op, st, what):
    got = op.run(eng, st)
    want = op.expect(st)
    assert want is None or R.same(got, want), f"{what}: {op.name} returned another value than its reference"
    return got


def check_readers(eng, st, what):
    for r in R.READERS:
        if r.needs(st):
            assert R.same(r.run(eng, st), r.expect(st)), f"{what}: {r.name}() differs from its reference"
        else:
            with pytest.raises(BpeError, match=R.ESTATE):
                r.run(eng, st)
    if not st.rows:
        with pytest.raises(BpeError, match=R.ESTATE):
            eng.fetch_rows()


def check_still_works(eng, what):
    eng.load(R.DATA)
    eng.encode(R.merges_fixed())
    assert R.same(eng.ids(), R.h_encode(R.DATA)), f"{what}: load + encode after the refusal"
    return R.step(R.step(R.St(), R.BY_NAME["load"])[1], R.BY_NAME["encode_win"])[1]


# ---------------------------------------------------------------- a. every ordered pair

@pytest.mark.parametrize("a", [op.name for op in R.CHANGING])
def test_every_ordered_pair(a):
    eng = api.Engine(0)
    st = R.St()
    try:
        for seq in R.pairs(a):
            what = " -> ".join(seq)
            if not R.shortest_path(a):  # (A is allowed on a fresh context: that is where this pair starts)
                eng.trim()
                st = R.St()
            for name in seq[:-1]:
                op = R.BY_NAME[name]
                legal, after = R.step(st, op)
                assert legal, what
                run_expect(eng, op, st, what)
                st = after
            b = R.BY_NAME[seq[-1]]
            legal, after = R.step(st, b)
            if legal:
                run_expect(eng, b, st, what)
                st = after
                check_readers(eng, st, what)
            else:
                with pytest.raises(BpeError, match=R.ESTATE):
                    b.run(eng, st)
                check_readers(eng, st, what + " (refused)")  # nothing half-written: the state is A's
                rows = st.rows
                st = check_still_works(eng, what)
                st.rows = rows
    finally:
        eng.close()


# ---------------------------------------------------------------- e. trim after every operation

@pytest.mark.parametrize("a", [op.name for op in R.CHANGING])
def test_trim_after_every_operation(a):
    eng = api.Engine(0)
    st = R.St()
    try:
        for name in R.shortest_path(a) + (a,):
            run_expect(eng, R.BY_NAME[name], st, name)
            st = R.step(st, R.BY_NAME[name])[1]
        eng.trim()
        check_readers(eng, R.St(), f"{a} -> trim")  # (merges() alone answers: with no pair)
        for name in ("decode_rows", "train", "encode_win", "split_cl100k", "encode_split", "map_ids", "token_spans_byte"):
            with pytest.raises(BpeError, match=R.ESTATE):
                R.BY_NAME[name].run(eng, R.St())
        st = R.St()
        for name in ("load", "train_hash", "split_cl100k_sp", "encode_split"):  # the next load starts clean
            run_expect(eng, R.BY_NAME[name], st, f"{a} -> trim -> {name}")
            st = R.step(st, R.BY_NAME[name])[1]
            check_readers(eng, st, f"{a} -> trim -> {name}")
    finally:
        eng.close()


# ---------------------------------------------------------------- b. a dirty pool, then a small run

RICH = G.load("synth_s1_1m")  # 1 MiB of synth_bytes(1), 1024 merges: the recorded reference run
RICH_CAP = RICH["max_merges"]
SMALL_CAP = 40


def small_jobs():
    seen = set(synth_bytes(1, 1 << 20))
    unseen = bytes(b for b in range(1, 256) if b not in seen)
    assert len(unseen) >= 8
    rng = np.random.default_rng(17)
    jobs = [(f"one_byte_{n}", b"a" * n) for n in (2, 3, 65536, 65537, 131073)]
    jobs.append(("abab_run", b"ab" * 700 + b"a" * 37 + b"ab" * 700))
    jobs.append(("two_letters", rng.choice(np.frombuffer(b"xy", np.uint8), 4096).tobytes()))
    jobs.append(("unseen_bytes", rng.choice(np.frombuffer(unseen, np.uint8), 3000).tobytes()))
    return jobs


def dense_expected(n, cap):
    """bpe_gpu.h, table_dense: the run has a merge cap and the square of 256 + cap ids is no larger than the hash
    table would be (engine.hip, setup_run_body: the hash table's slots from the keys a run of that cap can make, at
    least 2^17; the square padded to rows of 32 ids, 4 bytes a count against 12 a slot)"""
    if cap < 0:
        return 0
    m = min(n - 1, cap)
    keys = min(n, 65536 + 512 * m + m * m)
    want = max(min(max(2 * keys, 4 * (65536 + 16 * (256 + min(m, 4096)))), 1 << 28), 1 << 17)
    hcap = 1
    while hcap < want:
        hcap <<= 1
    V = 256 + m
    P = (V + 31) & ~31
    return int(4 * P * V <= 12 * hcap)


def train_and_check(eng, data, cap, fast, what):
    eng.load(data)
    k = eng.train(cap, fast=fast)
    want_m, want_ids, _ = O.train(data, cap, O.RULE if fast else O.EMU)
    assert k == len(want_m) and R.same(eng.merges(), want_m), f"{what}: merges"
    assert R.same(eng.ids(), want_ids), f"{what}: ids"
    assert eng.stats()["table_dense"] == dense_expected(len(data), cap), what
    log = eng.merge_log()
    assert log.size == k, what
    # every count: the adjacent (a, b) positions in the tokens before the merge, replayed as the reference's replace
    # pass does it (left to right, a run a a a gives z a); the replay itself is held to the oracle's ids
    ids = np.frombuffer(data, np.uint8).astype(np.uint32)
    for r, (x, y) in enumerate(want_m.tolist()):
        idx = np.flatnonzero((ids[:-1] == x) & (ids[1:] == y))
        assert int(log["count"][r]) == idx.size, f"{what}: count of merge {r}"
        if x == y and idx.size:  # of overlapping positions every second one of a run merges
            starts = np.concatenate([[True], np.diff(idx) != 1])
            first = np.maximum.accumulate(np.where(starts, np.arange(idx.size), 0))
            idx = idx[(np.arange(idx.size) - first) % 2 == 0]
        ids[idx] = 256 + r
        ids = np.delete(ids, idx + 1)
    assert R.same(ids, want_ids), f"{what}: the replay of the oracle's merges does not give the oracle's ids"


def rich_run(eng, what):
    eng.synth(RICH["synth"]["seed"], RICH["synth"]["n"])
    # default mode tracks the schedule below 2^21 tokens and commits one merge at a time; the schedule-free rule, which
    # from 2^20 tokens on is the same training (bpe_gpu.h, BPE_GPU_FAST), runs in batches: both, the batches last
    for fast in (False, True):
        assert eng.train(RICH_CAP, fast=fast) == RICH_CAP
        st = eng.stats()
        assert st["table_dense"] == 1 and st["hot_mode"] in (1, 2) and (st["batches"] > 0) == fast, (what, fast, st)
        merges = eng.merges()
        G.check(RICH, merges, eng.ids())
    eng.encode(merges)  # (the replay of a run's own merges over its own corpus gives the run's ids)
    G.check(RICH, merges, eng.ids())
    n = RICH["synth"]["n"]
    eng.encode_docs([0, n], merges)
    G.check(RICH, merges, eng.ids())
    assert eng.doc_offsets().tolist() == [0, RICH["ids_len"]], what
    return merges


@pytest.fixture(scope="module")
def dirty():
    """a context after the rich job: 1 MiB of synth_bytes(1) trained with the recorded cap of 1 024 in default mode and
    by the schedule-free rule (the hot set, the dense table and, under that rule, batches are all in use), then encode
    and encode_docs.  A cap of 2 000 has no recorded
    reference and the oracle takes 91 s for it at this size (51 s with the schedule-free rule; 1 MiB, measured on the
    CPU), so the recorded run, which the suite already trusts, stands in: same corpus, same layouts."""
    eng = api.Engine(0)
    eng.set_merge_log(True)
    rich_run(eng, "rich")
    yield eng
    eng.close()


@pytest.mark.parametrize("fast", [False, True], ids=["default", "fast"])
@pytest.mark.parametrize("cap", [-1, RICH_CAP, SMALL_CAP], ids=["no_cap", "rich_cap", "small_cap"])
def test_small_runs_on_a_dirty_context(dirty, cap, fast):
    for name, data in small_jobs():
        train_and_check(dirty, data, cap, fast, f"rich -> {name} cap {cap} fast {fast}")


def test_small_then_rich_regrows():
    """the other order on a fresh context: grow-only scratch and pooled buffers sized by a 3-byte run are regrown for
    the 1 MiB run, whose merges and ids are the recorded reference's"""
    eng = api.Engine(0)
    try:
        eng.set_merge_log(True)
        for name, data in small_jobs()[1:3] + small_jobs()[5:]:
            train_and_check(eng, data, SMALL_CAP, False, f"fresh -> {name}")
        rich_run(eng, "small -> rich")
    finally:
        eng.close()


# ---------------------------------------------------------------- c. a shrinking then growing batch

def batch_texts(T, seed):
    rng = np.random.default_rng(seed)
    lens = rng.choice([0, 1, 2, 63, 64, 65, 150], T) if T > 1 else [70] * T
    return tuple(R.mixed(int(n), seed + 7 * i, every=30) for i, n in enumerate(lens))


def test_shrinking_then_growing_batch():
    eng = api.Engine(0)
    L, pad, sp, m = 65, R.PAD_ID, R.SPECIALS, R.merges_fixed()
    v = R.vocab_for(R.K, sp)
    fwd, inv = vocab_tables(v)
    try:
        for rnd, T in enumerate((300, 1, 0, 300)):
            what = f"round {rnd}, {T} texts"
            texts = batch_texts(T, 100 + rnd)
            data = b"".join(texts)
            off, piece, index, _ = R.h_split(data, texts, "cl100k", sp)
            ids, ido, toff = R.h_encode_split(data, texts, "cl100k", sp)
            assert eng.load_texts(list(texts)) == T, what
            assert eng.split("cl100k", list(sp)) == off.size - 1, what
            assert R.same(eng.split_offsets(), off) and R.same(eng.special_pieces(), (piece, index)), what
            eng.encode_split(m)
            assert R.same(eng.ids(), ids) and R.same(eng.doc_offsets(), ido) and R.same(eng.text_offsets(), toff), what
            eng.map_ids(v)
            assert R.same(eng.ids(), fwd[ids]), what
            spans = R.h_spans(ids, m, sp, texts, toff, "char")
            assert R.same(eng.token_spans(m, list(sp), v, unit="char"), spans), what
            rows, lens = texts_ref.pack_rows(fwd[ids], toff, L, pad, "right")
            assert R.same(eng.pack_texts(L, pad), (rows, lens)), what
            assert R.same(eng.pack_spans(L), R.pack_span_rows(spans, toff, L, "right")), what
            want = stream_ref.pack_stream(fwd[ids], toff, 64, pad, R.BOS, R.EOS)
            assert R.same(eng.pack_stream(64, pad, R.BOS, R.EOS, segments=True, positions=True), want[:3]), what
            assert eng.stream_rows(64, R.BOS, R.EOS) == (want[0].shape[0], want[3]), what
            uids, uoff, ubounds = rows_ref.unpack(rows, None, pad)
            assert R.same(eng.unpack_rows(rows, None, pad), (uids, uoff, ubounds)), what
            assert R.same(eng.decode_rows(m, list(sp), v), R.h_decode_docs(inv[uids], uoff, m, sp)), what
    finally:
        eng.close()


# ---------------------------------------------------------------- d. the decoders' slots, interleaved

def test_decoders_interleaved():
    """decode_docs of N ids, decode_rows of fewer, token_spans, decode_docs of more than N, decode of one id that
    expands to 2^13 bytes: the offset slot and the scans' temporary serve a shorter scan, then a longer one"""
    m, sp = R.merges_fixed(), R.SPECIALS
    ids, ido, _ = R.h_encode_split(R.DATA, None, "cl100k", sp)
    big = R.DATA + R.FILE_DATA + R.DATA
    ids3, ido3, _ = R.h_encode_split(big, None, "o200k", sp)
    rids, roff, _ = R.h_rows()
    assert rids.size < ids.size < ids3.size
    chain = np.array([[0x61, 0x61]] + [[255 + r, 255 + r] for r in range(1, 14)], np.uint32)
    assert O.decode(np.array([256 + 12], np.uint32), chain) == b"a" * 8192
    eng = api.Engine(0)
    try:
        eng.load(R.DATA)
        eng.split("cl100k", list(sp))
        eng.encode_split(m)
        for rnd in range(2):
            what = f"round {rnd}"
            assert R.same(eng.decode_docs(ids, ido, m, specials=list(sp)), R.h_decode_docs(ids, ido, m, sp)), what
            eng.unpack_rows(R.rows_fixed(), None, R.ROWS_PAD, R.ROWS_STOP, R.ROWS_SKIP)
            assert R.same(eng.decode_rows(m), R.h_decode_rows()), what
            spans = R.h_spans(ids, m, sp, (R.DATA,), np.array([0, ids.size]), "byte")
            assert R.same(eng.token_spans(m, list(sp)), spans), what
            assert R.same(eng.decode_rows(m), R.h_decode_rows()), what  # (the unpacked ids stay)
            got = eng.decode_docs(ids3, ido3, m, specials=list(sp))
            assert got[0] == big and R.same(got, R.h_decode_docs(ids3, ido3, m, sp)), what
            assert eng.decode([256 + 12], chain) == b"a" * 8192, what
            assert eng.decode([256 + 13, 0x62], chain) == O.decode(np.array([256 + 13, 0x62], np.uint32), chain), what
            assert R.same(eng.decode_rows(m), R.h_decode_rows()), what
            assert R.same(eng.ids(), ids) and R.same(eng.doc_offsets(), ido), what  # the resident ids were not touched
    finally:
        eng.close()


# ---------------------------------------------------------------- f. a group of shards, reused

def test_shard_group_reused():
    big, small = synth_bytes(3, 65537), R.mixed(3001, 5)
    g = api.ShardGroup(0, local_shards=3)
    try:
        for data, cuts, cap in ((big, [0, 20000, 20001, len(big)], 120), (small, [0, 1, 2000, len(small)], 60)):
            g.load_split(data, cuts)
            assert g.train(cap) == cap
            want_m, want_ids, _ = O.train(data, cap, O.RULE)
            assert R.same(g.merges(), want_m) and R.same(g.all_ids(), want_ids), len(data)
        g.encode(R.merges_fixed())
        assert R.same(g.all_ids(), O.encode(small, R.merges_fixed()))
        g.load_split(big, [0, 30000, 65536, len(big)])
        g.encode(want_m)
        assert R.same(g.all_ids(), O.encode(big, want_m))
    finally:
        g.close()

"""The dense pair table (one count per pair of ids, count[u * P + v], chosen by
setup_run when the run has a merge cap and the square of its 256 + cap ids is no
larger than the hash table) against the hash table (BPE_TAB_DENSE=0) and the
oracle: the table is a map from key to count in both layouts, so merges, ids and
every count derived from it (distinct pairs, buckets, batches) are the same.

Each run asserts stats()["table_dense"] is what was asked for."""
import contextlib
import os

import numpy as np
import pytest

import oracle_lib as O
from llmtokenizer_amd import api
from llmtokenizer_amd.synth import synth_bytes

pytestmark = pytest.mark.gpu

KNOBS = ("BPE_TAB_DENSE", "BPE_TABLE_SLOTS", "BPE_TAB_IL", "BPE_BATCH", "BPE_TIE_TEST", "BPE_SKIP_TEST")


@contextlib.contextmanager
def _env(**kv):
    """the table knobs as given (None / absent: unset), put back afterwards"""
    old = {k: os.environ.get(k) for k in KNOBS}
    try:
        for k in KNOBS:
            v = kv.get(k)
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _run(data, mm, dense, fast=True, expect=None, **kv):
    """one training run; dense: "1" / "0" forced, None the default choice.
    expect: table_dense the run must report (default: what was forced)"""
    with _env(BPE_TAB_DENSE=dense, **kv):
        e = api.Engine(0)
        try:
            e.load(data)
            n = e.train(mm, fast=fast)
            st = e.stats()
            out = {"n": n, "merges": e.merges(), "ids": e.ids(), "csum": e.ids_checksum(), "st": st}
        finally:
            e.close()
    want = int(dense) if expect is None else expect
    assert st["table_dense"] == want, (dense, kv, st["table_dense"])
    if st["table_dense"]:
        assert st["table_grows"] == 0
    return out


def _same(a, b, what):
    assert a["n"] == b["n"], (what, a["n"], b["n"])
    assert a["merges"].shape == b["merges"].shape and (a["merges"] == b["merges"]).all(), (what, "merges differ")
    assert a["csum"] == b["csum"], (what, "ids checksum differs")
    assert a["ids"].size == b["ids"].size and (a["ids"] == b["ids"]).all(), (what, "ids differ")
    for k in ("distinct_pairs", "merged_buckets"):
        assert a["st"][k] == b["st"][k], (what, k, a["st"][k], b["st"][k])


@pytest.fixture(scope="module")
def case1():
    """24 MiB x 2500 merges (test_table_layouts_agree_on_batches' input), fast=False as there:
    the default choice and the forced hash table"""
    data = synth_bytes(77, 24 << 20)
    return {"default": _run(data, 2500, None, fast=False, expect=1), "hash": _run(data, 2500, "0", fast=False)}


def test_batches_dense_equals_hash(case1):
    d, h = case1["default"], case1["hash"]
    print({k: (d["st"][k], h["st"][k]) for k in ("batches", "distinct_pairs", "merged_buckets", "keys", "table_grows")})
    assert d["n"] == 2500
    _same(d, h, "24 MiB x 2500")
    assert d["st"]["batches"] == h["st"]["batches"] and d["st"]["batches"] > 0
    assert d["st"]["table_grows"] == 0


@pytest.mark.parametrize("batch", [None, "0"])
def test_one_merge_engine_dense_equals_oracle(batch):
    """the tracked / one-merge engine (k_apply's role B) on the dense table == the oracle's EMU order,
    as test_table_regrowth_matches_presized asks of the hash table; again with BPE_BATCH=0"""
    data = synth_bytes(905, 1 << 20)
    d = _run(data, 400, "1", fast=False, BPE_BATCH=batch)
    om, oids, _ = O.train(data, 400, O.EMU)
    assert d["merges"].shape == om.shape and (d["merges"] == om).all()
    assert d["ids"].size == oids.size and (d["ids"] == oids).all()


@pytest.mark.parametrize("cap,P", [(70, 352), (64, 320)])
def test_pitch_is_not_width(cap, P):
    """V = 256 + cap ids in rows of pitch P = V rounded up to 32 (352 > 326; 320 == 320); all cap merges
    are made, so the last id V - 1 is created and is a neighbour in the last row and column"""
    V = 256 + cap
    assert (V + 31) // 32 * 32 == P
    data = synth_bytes(31, 3 << 20)
    d, h = _run(data, cap, "1"), _run(data, cap, "0")
    assert d["n"] == cap and int(d["ids"].max()) == V - 1
    _same(d, h, ("pitch", cap))


def _diag_cases():
    n = 1 << 20
    ab = b"ab" * n
    cut = 2 * 300001
    return [("one byte", b"a" * (2 << 20), 64),
            ("ab + a run", ab[:cut] + b"a" * 70001 + ab[cut:2 * n - 70001], 200)]


@pytest.mark.parametrize("k", [0, 1])
def test_diagonal_and_long_runs(k):
    """keys on the diagonal ((a, a), then (z, z) of the ids made from them) and long a == b runs:
    dense == hash on 2 MiB, and == the oracle's RULE order on a 64 KiB prefix"""
    what, data, mm = _diag_cases()[k]
    assert len(data) == 2 << 20
    d, h = _run(data, mm, "1"), _run(data, mm, "0")
    _same(d, h, what)
    assert d["n"] > 0
    pre = data[:64 << 10] if k == 0 else data[2 * 300001 - (16 << 10):2 * 300001 - (16 << 10) + (64 << 10)]
    p = _run(pre, mm, "1")
    om, oids, _ = O.train(pre, mm, O.RULE)
    assert p["merges"].shape == om.shape and (p["merges"] == om).all(), what
    assert p["ids"].size == oids.size and (p["ids"] == oids).all(), what


@pytest.mark.parametrize("knob", ["BPE_TIE_TEST", "BPE_SKIP_TEST"])
def test_revert_and_retry_paths(knob):
    """every tie-order check fails (BPE_TIE_TEST: the undo log is replayed through the slots) / every
    skipped-key check fails (BPE_SKIP_TEST): same merges and ids as the hash table, and batches were
    formed again"""
    data = synth_bytes(411, 8 << 20)
    d, h = _run(data, 800, "1", **{knob: "1"}), _run(data, 800, "0", **{knob: "1"})
    print(knob, {k2: (d["st"][k2], h["st"][k2]) for k2 in ("batches", "batch_retries", "tie_failed", "skip_failed",
                                                            "batch_dropped")})
    _same(d, h, knob)
    assert d["st"]["batch_retries"] > 0 and h["st"]["batch_retries"] > 0


def test_selection(case1):
    small = synth_bytes(905, 1 << 20)
    r = _run(small, 400, None, fast=False, expect=0, BPE_TABLE_SLOTS=32768)
    assert r["st"]["table_grows"] >= 1
    _run(small, 400, None, fast=False, expect=0, BPE_TAB_IL=1)
    # no merge cap of the caller's: the hash table, forced or not
    tiny = synth_bytes(1, 4096)
    _run(tiny, -1, None, fast=False, expect=0)
    _run(tiny, -1, "1", fast=False, expect=0)
    # BPE_TAB_DENSE=1 forces it past BPE_TABLE_SLOTS / BPE_TAB_IL
    _run(small, 400, "1", fast=False, BPE_TAB_IL=1)
    assert case1["default"]["st"]["table_dense"] == 1


def _group(data, cuts, mm, dense):
    with _env(BPE_TAB_DENSE=dense):
        g = api.ShardGroup(0, local_shards=len(cuts) - 1)
        try:
            g.load_split(data, cuts)
            n = g.train(mm)
            st = g.stats()
            out = {"n": n, "merges": g.merges(), "ids": g.all_ids(), "st": st}
        finally:
            g.close()
    assert st["table_dense"] == int(dense)
    return out


def test_sharded_dense_equals_hash_and_single():
    """four shards on one device (every shard's table dense, the same shape): == the hash table == one context"""
    data = synth_bytes(612, 8 << 20)
    n = len(data)
    cuts = [0, n // 4 + 2, n // 2, 3 * n // 4 - 7, n]  # uneven shards, odd and even sizes
    d, h = _group(data, cuts, 600, "1"), _group(data, cuts, 600, "0")
    s = _run(data, 600, "1")
    for a, what in ((h, "hash group"), (s, "single context")):
        assert d["n"] == a["n"] == 600, what
        assert (d["merges"] == a["merges"]).all(), what
        assert d["ids"].size == a["ids"].size and (d["ids"] == a["ids"]).all(), what
    assert d["st"]["distinct_pairs"] == h["st"]["distinct_pairs"]

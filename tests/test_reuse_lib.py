"""The model of tests/reuse_lib.py, on the CPU: held to hand-written sequences taken from the lifetime tests that pass
on the device (test_gpu_texts, test_gpu_spans, test_gpu_vocab, test_gpu_train_split, test_gpu_rows,
test_gpu_encode_docs), so that it cannot drift from them, and the sequence generator held to its own condition: every
operation reached, every ordered pair of state-changing operations generated."""
import itertools

import numpy as np
import pytest

import reuse_lib as R
import texts_ref
from llmtokenizer_amd import api

OK, NO = True, False


def legality(names):
    return [legal for _, legal, _, _ in R.walk(names)]


def final(names):
    return R.walk(names)[-1][3]


# (sequence, which calls succeed): the lifetime tests named above, call by call
SEQUENCES = [
    # test_gpu_train_split.test_state_and_lifetime
    (["train_split", "load", "train_split", "split_merges", "piece_table", "split_table", "split_merges", "train_split",
      "split_merges", "encode_split", "split_merges", "train_split", "split_cl100k", "split_merges", "train_split", "load",
      "split_merges", "piece_table", "train_split", "split_table", "train_split", "train", "split_merges", "trim",
      "train_split", "load", "split_table", "train_split", "split_merges"],
     [NO, OK, NO, NO, NO, OK, NO, OK, OK, OK, OK, OK, OK, NO, OK, OK, NO, NO, NO, OK, OK, OK, NO, OK, NO, OK, OK, OK, OK]),
    # test_gpu_vocab.test_state
    (["map_ids", "load", "map_ids", "split_cl100k", "encode_split", "map_ids", "ids", "doc_offsets", "map_ids", "ids",
      "encode_split", "map_ids", "load", "map_ids", "encode_win", "map_ids"],
     [NO, OK, NO, OK, OK, OK, OK, OK, NO, OK, OK, OK, OK, NO, OK, OK]),
    # test_gpu_texts.test_refusals_and_lifetime
    (["load", "text_offsets", "load_texts", "encode_win", "train", "encode_docs", "text_offsets", "pack_texts",
      "split_cl100k_sp", "train_split", "split_offsets", "encode_split", "ids", "text_offsets", "doc_offsets",
      "split_table_sp", "split_offsets", "encode_split", "text_offsets", "load", "split_cl100k_sp", "encode_split",
      "ids_checksum", "doc_offsets", "text_offsets", "pack_texts", "encode_win"],
     [OK, NO, OK, NO, NO, NO, NO, NO, OK, NO, OK, OK, OK, OK, OK, OK, OK, OK, OK, OK, OK, OK, OK, OK, NO, NO, OK]),
    # test_gpu_spans.test_refusals_and_lifetime
    (["token_spans_byte", "load", "token_spans_byte", "encode_win", "token_spans_byte", "split_cl100k", "encode_split",
      "token_spans_byte", "token_spans_char", "pack_spans", "load_texts", "split_cl100k_sp", "encode_split", "pack_spans",
      "token_spans_byte", "pack_spans", "encode_split", "pack_spans"],
     [NO, OK, NO, OK, NO, OK, OK, OK, OK, NO, OK, OK, OK, NO, OK, OK, OK, NO]),
    # test_gpu_rows.test_unpack_and_encode_do_not_disturb_each_other, and trim
    (["fetch_rows", "decode_rows", "unpack_rows", "load", "encode_win", "fetch_rows", "decode", "decode_rows", "load_texts",
      "fetch_rows", "trim", "fetch_rows", "decode_rows", "unpack_rows", "decode_rows"],
     [NO, NO, OK, OK, OK, OK, OK, OK, OK, OK, OK, NO, NO, OK, OK]),
    # test_gpu_encode_docs: the document offsets go with an encode that leaves none
    (["load", "encode_docs", "doc_offsets", "encode_win", "doc_offsets", "ids", "encode_docs", "train_fast", "doc_offsets",
      "merges", "ids"],
     [OK, OK, OK, OK, NO, OK, OK, OK, NO, OK, OK]),
]


@pytest.mark.parametrize("k", range(len(SEQUENCES)))
def test_model_agrees_with_the_lifetime_tests(k):
    names, want = SEQUENCES[k]
    assert len(names) == len(want)
    got = legality(names)
    assert got == want, [(n, g, w) for n, g, w in zip(names, got, want) if g != w]


def test_what_each_call_leaves():
    """the header's lifetime sentences, flag by flag"""
    f = final(["load", "split_cl100k_sp", "train_split", "encode_split", "map_ids", "token_spans_char", "unpack_rows"]).flags()
    assert f == {"loaded": True, "ids_ready": True, "ids_mapped": True, "spans_ready": True, "docs_ready": True,
                 "split_ready": True, "sp_S": 2, "tx_on": False, "rows_ready": True, "ts_ready": True, "pres_valid": True}
    base = ["load", "split_cl100k_sp", "train_split", "encode_split", "map_ids", "token_spans_char", "unpack_rows"]
    everything = R.valid_readers(final(base))
    assert everything == {r.name for r in R.READERS} - {"text_offsets"}
    # encode, encode_docs, encode_split and decode keep the split and what was trained on it; the ids are new
    for call in ("encode_win", "encode_glob", "encode_docs", "encode_split", "decode", "decode_docs_vocab"):
        f = final(base + [call]).flags()
        assert f["split_ready"] and f["ts_ready"] and f["rows_ready"], call
        assert f["ids_mapped"] == f["spans_ready"] == call.startswith("decode"), call
    # a training drops the split, a split keeps the ids and drops train_split's results
    f = final(base + ["train"]).flags()
    assert not f["split_ready"] and not f["ts_ready"] and f["ids_ready"] and not f["docs_ready"] and f["rows_ready"]
    f = final(base + ["split_table"]).flags()
    assert f["split_ready"] and f["sp_S"] == 0 and not f["ts_ready"] and f["ids_mapped"] and f["spans_ready"]
    # every load ends all but the rows; trim ends those too
    for call in ("load", "load_file", "synth", "load_texts", "load_texts_off"):
        st = final(base + [call])
        assert R.valid_readers(st) == {"merges"} and st.flags()["rows_ready"] and st.flags()["loaded"], call
        assert st.flags()["tx_on"] == call.startswith("load_texts")
    st = final(base + ["trim"])
    assert R.valid_readers(st) == {"merges"} and not any(st.flags().values())
    # the merges go with the run buffers of their training
    assert final(["load", "train"]).trained and final(["load", "train", "split_table", "unpack_rows", "map_ids"]).trained
    for call in ("load", "synth", "trim", "encode_win", "encode_docs"):
        assert final(["load", "train", call]).trained is None, call


def test_a_refused_call_changes_nothing():
    for op, legal, before, after in R.walk(["load_texts", "split_cl100k", "encode_split", "train", "encode_docs", "train_split"]):
        assert legal or after is before


def test_every_operation_and_every_ordered_pair_is_generated():
    assert len(R.OPS) == len({op.name for op in R.OPS}) and len(R.CHANGING) >= 30
    seqs = list(R.pairs())
    got = {(s[-2], s[-1]) for s in seqs}
    assert got == set(itertools.product([op.name for op in R.CHANGING], repeat=2)) and len(seqs) == len(got)
    reached_legal, ran = set(), set()
    for s in seqs:
        steps = R.walk(s)
        assert all(legal for _, legal, _, _ in steps[:-1]), s  # the path and A itself are allowed
        ran |= {op.name for op, _, _, _ in steps}
        reached_legal |= {op.name for op, legal, _, _ in steps if legal}
        reached_legal |= R.valid_readers(steps[-1][3])
        # the path is a shortest one: no call of it can be left out
        assert len(s) - 2 == len(R.shortest_path(s[-2]))
    every = {op.name for op in R.OPS + R.READERS}
    assert ran | {r.name for r in R.READERS} == every and reached_legal == every
    # each operation is refused in some pair and each reader in some state, but for the calls that are always allowed
    refused = {s[-1] for s in seqs if not R.walk(s)[-1][1]}
    always = {op.name for op in R.CHANGING if op.needs(R.St())}
    assert refused == {op.name for op in R.CHANGING} - always
    assert always == {"load", "load_texts", "load_texts_off", "load_file", "synth", "trim", "decode", "decode_docs",
                      "decode_docs_sp", "decode_docs_vocab", "unpack_rows"}


def test_paths_are_short():
    assert R.shortest_path("load") == () and R.shortest_path("train") == ("load",)
    assert R.shortest_path("pack_spans") == ("load_texts", "split_table", "encode_split", "token_spans_byte")
    assert max(len(R.shortest_path(op.name)) for op in R.CHANGING) == 4


def test_fixed_inputs_cross_the_edges_they_are_meant_to():
    assert api.split_info()["tile"] == R.TILE and len(R.DATA) == R.TILE + 1 and len(R.FILE_DATA) == R.TILE - 1
    assert len(R.TEXTS) == 65 and len(R.TEXTS2) == 63 and R.TEXTS[0] == b"" and b"" in R.TEXTS2
    assert all(R.DATA.count(s) >= 2 for s in R.SPECIALS) and 0 not in R.DATA and 0 not in R.FILE_DATA
    rows = R.rows_fixed()
    assert rows.shape == (65, 63) and rows.dtype == np.int64
    ids, off, bounds = R.h_rows()
    want = api.unpack_rows_host(rows, None, R.ROWS_PAD, R.ROWS_STOP, R.ROWS_SKIP)  # (the second witness)
    assert R.same((ids, off, bounds), want) and 0 < ids.size < rows.size and 0 not in ids


def test_host_expectations_agree_with_their_second_witness():
    """texts_ref for a preset rule, api.pack_stream_host and api.token_spans_host for the batch's ids"""
    for sp in (None, R.SPECIALS):
        off, piece, index, _ = R.h_split(b"".join(R.TEXTS), R.TEXTS, "cl100k", sp)
        woff, _, wsp = texts_ref.split_texts(R.TEXTS, "cl100k", list(sp) if sp else None)
        assert off.tolist() == woff.tolist() and list(zip(piece.tolist(), index.tolist())) == wsp
    st = final(["load_texts", "split_cl100k_sp", "encode_split", "token_spans_char"])
    ids, ido, toff, merges = st.ids.value()
    assert toff.size == 66 and int(toff[-1]) == ids.size == int(ido[-1]) and (256 + R.K) in ids
    rows, seg, pos = R.BY_NAME["pack_stream"].expect(st)
    assert R.same((rows, seg, pos), api.pack_stream_host(ids, toff, R.SEQ_LEN, R.PAD_ID, R.BOS, R.EOS)[:3])
    boff = texts_ref.byte_offsets(R.TEXTS)
    lens = api.span_lens(merges, list(R.SPECIALS))
    want = api.token_spans_host(ids, toff, st.data, boff, lens, "char")
    assert R.same(R.BY_NAME["token_spans_char"].expect(st), want)
    # the decoders' inputs decode to the text they came from
    for name in ("decode", "decode_docs", "decode_docs_sp", "decode_docs_vocab"):
        got = R.BY_NAME[name].expect(R.St())
        assert (got if name == "decode" else got[0]) == R.DATA, name
    assert R.BY_NAME["decode_docs_sp"].expect(R.St())[1].tolist() == R.h_split(R.DATA, None, "cl100k", R.SPECIALS)[0].tolist()

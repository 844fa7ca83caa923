"""One context across calls of every kind: a table of operations, a model of the context's state, and the sequences
the reuse tests walk (tests/test_reuse_lib.py on the CPU, tests/test_gpu_reuse.py on the device).

An operation is a small object: run(eng, st) makes the API call on an api.Engine (st: the model's state before the
call, from which it takes the arguments a caller would know, such as the vocabulary of the resident ids), needs(st)
says whether include/bpe_gpu.h allows the call in that state (else it must raise "call out of order"), leave(st)
gives the state after it, and expect(st) the value run() must return.  Every expected value comes from the host
references the suite has (oracle_lib, api.split_host_special, train_split_ref, texts_ref, spans_ref, stream_ref,
rows_ref, api.pack_stream_host, api.unpack_rows_host), never from a device call.

The state (St) is bpe_gpu_ctx's readiness flags, as the header states them, beside the host-side facts the
expectations need: which bytes are resident, which split stands, what the resident ids are.  St.flags() names the
ten flags as the engine does.  No GPU is used at import or by the model; the expectations load the oracle."""
import functools
import os

import numpy as np

ESTATE = "call out of order"
K = 24                      # merges of the fixed list
EOT = b"<|endoftext|>"
SPECIALS = (EOT, b"\xac|x|")
TILE = 4096                 # api.split_info()["tile"], held to it by test_reuse_lib
ROW_LEN, PAD_ID = 5, 70000  # pack_texts / pack_spans
SEQ_LEN, BOS, EOS = 7, 70001, 70002  # pack_stream
ITEMS = [b"'", b"s", b"T", b"re", b"LL", b"a", b"1", b"23", b"4567", b"!", b"\n", b"\n\n", b"\r\n", b" ", b"  ", b"\t",
         b"word", b" the", b" the", b"!\n", b" \n", b"\n  ", b"\x80", b"\xe2\x82", b"\xff"]
ITEMS += [s.encode() for s in ("é", "Ж", "中", "\U00010400", "٣", "½", "　", "—", "\U0001f600")]


def mixed(n, seed, every=80):
    """n bytes of the items above in random order, one item in `every` a special (cut at n)"""
    rng = np.random.default_rng(seed)
    out, size = [], 0
    while size < n:
        for k, r in zip(rng.integers(0, len(ITEMS), 256).tolist(), rng.integers(0, every, 256).tolist()):
            out.append(SPECIALS[r] if r < len(SPECIALS) else ITEMS[k])
            size += len(out[-1])
    return b"".join(out)[:n]


DATA = mixed(TILE + 1, 21)          # load: one byte into the split's second tile
FILE_DATA = mixed(TILE - 1, 22)     # load_file
SYNTH = (5, TILE)                   # synth: seed, bytes
TEXTS = tuple(mixed(n, 30 + i) for i, n in enumerate([0, 1, 63, 64, 65, 0, 200, 13] * 8 + [TILE - 700]))  # 65 texts
TEXTS2 = tuple(mixed(n, 90 + i) for i, n in enumerate([7, 0, 0, 64] * 15 + [1, 2, 3]))                 # 63, by offsets


def synth_data():
    from llmtokenizer_amd.synth import synth_bytes
    return synth_bytes(SYNTH[0], SYNTH[1])


# ---------------------------------------------------------------- host references, computed once

@functools.lru_cache(maxsize=None)
def merges_fixed():
    import oracle_lib as O
    m, _, _ = O.train(DATA, K, O.RULE)
    assert m.shape == (K, 2)
    return m


@functools.lru_cache(maxsize=None)
def h_train(data, cap, fast):
    import oracle_lib as O
    m, ids, _ = O.train(data, cap, O.RULE if fast else O.EMU)
    return m, ids


@functools.lru_cache(maxsize=None)
def h_encode(data):
    import oracle_lib as O
    return O.encode(data, merges_fixed())


def doc_cuts(n):
    """encode_docs' byte offsets over n resident bytes: an empty document first and last, one of one byte"""
    return np.array(sorted([0, 0, min(1, n), n // 3, min(n // 3 + 64, n), n, n]), dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def h_encode_docs(data):
    import oracle_lib as O
    off = doc_cuts(len(data))
    parts = [O.encode(data[int(a):int(b)], merges_fixed()) if b > a else np.zeros(0, np.uint32) for a, b in zip(off, off[1:])]
    return np.concatenate(parts), np.cumsum([0] + [p.size for p in parts]).astype(np.uint64)


RULES = ("table", "cl100k", "o200k")


def rule_arg(rule):
    if rule == "table":
        import special_ref
        return special_ref.random_rule(1)
    return rule


@functools.lru_cache(maxsize=None)
def h_split(data, texts, rule, specials):
    """(offsets in the plain join, special piece indices, their specials' indices, pieces per text or None): the
    host split of `data`, or of every text of `texts` alone (tests/texts_ref.py's definition, with the call that
    also takes a table rule)"""
    from llmtokenizer_amd import api
    sp = list(specials or ())
    if texts is None:
        off, piece, index = api.split_host_special(data, rule_arg(rule), sp)
        return off, piece, index, None
    starts, per_text, pieces, indices, base = [], [], [], [], 0
    for t in texts:
        if t:
            off, piece, index = api.split_host_special(t, rule_arg(rule), sp)
            pieces += [len(starts) + int(p) for p in piece]
            indices += [int(j) for j in index]
            starts += [base + int(o) for o in off[:-1]]
            base += len(t)
        per_text.append(len(starts))
    return (np.array(starts + [base], np.uint64), np.array(pieces, np.uint64), np.array(indices, np.uint32),
            np.array([0] + per_text, np.uint64))


def plain_pieces(data, texts, rule, specials):
    off, piece, _, _ = h_split(data, texts, rule, specials)
    sp = set(piece.tolist())
    return [(int(a), data[int(a):int(b)]) for i, (a, b) in enumerate(zip(off, off[1:])) if i not in sp]


@functools.lru_cache(maxsize=None)
def h_train_split(data, rule, specials):
    """(merges, the piece table as (start, length, count) lists in start order)"""
    import train_split_ref as TR
    pieces = plain_pieces(data, None, rule, specials)
    want, _, _ = TR.train([p for _, p in pieces], K)
    first, count, order = {}, {}, []
    for s, p in pieces:
        key = p if len(p) <= 64 else (s, p)  # (a piece above the deduplicated length is an entry of its own)
        if key not in first:
            first[key] = s
            order.append(key)
        count[key] = count.get(key, 0) + 1
    table = [(first[k], len(k if isinstance(k, bytes) else k[1]), count[k]) for k in order]
    return np.array(want, dtype=np.uint32).reshape(-1, 2), table


@functools.lru_cache(maxsize=None)
def h_encode_split(data, texts, rule, specials):
    """(ids, id offsets of the pieces, id offsets of the texts or None) under merges_fixed()"""
    import oracle_lib as O
    off, piece, index, per_text = h_split(data, texts, rule, specials)
    which = dict(zip(piece.tolist(), index.tolist()))
    parts = [np.array([256 + K + which[i]], np.uint32) if i in which else O.encode(data[int(a):int(b)], merges_fixed())
             for i, (a, b) in enumerate(zip(off, off[1:]))]
    ido = np.cumsum([0] + [p.size for p in parts]).astype(np.uint64)
    ids = np.concatenate(parts) if parts else np.zeros(0, np.uint32)
    return ids, ido, None if per_text is None else ido[per_text.astype(np.int64)]


@functools.lru_cache(maxsize=None)
def vocab_for(n_merges, specials):
    """a shuffled numbering with holes over n_merges merges and the specials (the merges' pairs are not read by the
    calls under test: a chain of valid ones stands in)"""
    from llmtokenizer_amd.vocab import Vocab
    sp = list(specials or ())
    ids = np.random.default_rng(11).permutation(256 + n_merges + len(sp) + 100)[: 256 + n_merges + len(sp)]
    pairs = np.stack([np.arange(n_merges) % 256, np.arange(n_merges) % 7 + 0x61], axis=1)
    return Vocab(pairs, ids[:256], ids[256:256 + n_merges], ids[256 + n_merges:], sp, "cl100k")


def fwd_of(vocab):
    from llmtokenizer_amd.vocab import vocab_tables
    return vocab_tables(vocab)[0]


def h_spans(ids, merges, specials, texts, text_off, unit):
    """spans of internal ids held as texts (spans_ref's formulas over the tokens' lengths)"""
    import spans_ref
    lens = np.array([len(t) for t in spans_ref.internal_token_bytes(merges, specials or ())], np.int64)
    out = [spans_ref.spans_fast(lens[ids[int(a):int(b)]], t, unit) for t, a, b in zip(texts, text_off, text_off[1:])]
    return np.concatenate(out + [np.zeros((0, 2), np.uint32)]).astype(np.uint32)


def pack_span_rows(spans, text_off, row_len, side):
    """api.Engine.pack_spans with numpy: cut as texts_ref.pack_rows cuts the ids, (0, 0) behind them"""
    T = len(text_off) - 1
    rows = np.zeros((T, row_len, 2), dtype=np.uint32)
    for k in range(T):
        seq = spans[int(text_off[k]):int(text_off[k + 1])]
        if len(seq) > row_len:
            seq = seq[:row_len] if side == "right" else seq[len(seq) - row_len:]
        rows[k, :len(seq)] = seq
    return rows


ROWS_PAD, ROWS_STOP, ROWS_SKIP = 0, (256 + K - 1,), (0x41, 256 + 3)


@functools.lru_cache(maxsize=None)
def rows_fixed():
    """65 rows of 63 int64 cells over the ids of merges_fixed() (one wave + 1 rows, one wave - 1 cells)"""
    import rows_ref
    return rows_ref.batch(np.random.default_rng(8), 65, 63, np.int64, ROWS_PAD, list(ROWS_STOP), list(ROWS_SKIP), vocab=256 + K)


@functools.lru_cache(maxsize=None)
def h_rows():
    import rows_ref
    return rows_ref.unpack(rows_fixed(), None, ROWS_PAD, ROWS_STOP, ROWS_SKIP)


@functools.lru_cache(maxsize=None)
def h_decode_rows():
    import oracle_lib as O
    ids, off, _ = h_rows()
    parts = [O.decode(ids[int(a):int(b)], merges_fixed()) if b > a else b"" for a, b in zip(off, off[1:])]
    return b"".join(parts), np.cumsum([0] + [len(p) for p in parts]).astype(np.uint64)


def h_decode_docs(ids, id_off, merges, specials=()):
    """(bytes, byte offsets) of internal ids held as documents: oracle_lib.decode over every stretch between two
    special ids, the specials' bytes between them"""
    import oracle_lib as O
    V0, out, bo = 256 + len(merges), [], [0]
    for a, b in zip(id_off, id_off[1:]):
        doc, run = [], []
        for x in ids[int(a):int(b)].tolist() + [None]:
            if x is not None and x < V0:
                run.append(x)
                continue
            if run:
                doc.append(O.decode(np.array(run, np.uint32), merges))
                run = []
            if x is not None:
                doc.append(bytes(specials[x - V0]))
        out.append(b"".join(doc))
        bo.append(bo[-1] + len(out[-1]))
    return b"".join(out), np.array(bo, np.uint64)


# ---------------------------------------------------------------- the state

class Ids:
    """the resident ids: kind "train", "encode" or "docs" (encode_docs / encode_split), and how to compute them"""

    def __init__(self, kind, fn, n_merges, specials=None, texts=None, data=None):
        self.kind, self.fn, self.n_merges, self.specials, self.texts, self.data = kind, fn, n_merges, specials, texts, data

    def value(self):
        """(ids, id offsets of the documents or None, id offsets of the texts or None, merges)"""
        return self.fn()


class St:
    def __init__(self):
        self.data = None      # the resident bytes (a text batch: the plain join); None: nothing loaded
        self.texts = None     # the texts of a text batch
        self.split = None     # (rule, specials or None)
        self.ts = False       # train_split's results stand
        self.ids = None       # Ids
        self.mapped = False
        self.spans = None     # unit
        self.rows = False
        self.trained = None   # (data, cap, fast) of the training whose run buffers stand

    def copy(self):
        s = St()
        s.__dict__.update(self.__dict__)
        return s

    def flags(self):
        """the engine's ten readiness flags in this state"""
        ids = self.ids is not None
        sp = self.split[1] if self.split else None
        return {"loaded": self.data is not None, "ids_ready": ids, "ids_mapped": self.mapped,
                "spans_ready": self.spans is not None, "docs_ready": ids and self.ids.kind == "docs",
                "split_ready": self.split is not None, "sp_S": len(sp) if sp else 0, "tx_on": self.texts is not None,
                "rows_ready": self.rows, "ts_ready": self.ts, "pres_valid": self.data is not None}

    def key(self):
        """what the search for shortest paths tells states apart by"""
        f = self.flags()
        return tuple(sorted(f.items())) + (self.ids.kind if self.ids else None, self.trained is not None)

    def drop_ids(self):
        self.ids, self.mapped, self.spans, self.trained = None, False, None, None

    def drop_bytes(self):
        self.drop_ids()
        self.data = self.texts = self.split = None
        self.ts = False

    def cur_ids(self):
        """the resident ids as the readers serve them (vocabulary ids once mapped)"""
        ids = self.ids.value()[0]
        return fwd_of(vocab_for(n_merges_of(self.ids), self.ids.specials))[ids] if self.mapped else ids

    def text_view(self):
        """(texts, their id offsets) the spans are relative to: the batch's, or the resident bytes as one text"""
        ids, _, toff, _ = self.ids.value()
        if self.ids.texts is not None:
            return self.ids.texts, toff
        return (self.ids.data,), np.array([0, ids.size], np.uint64)


# ---------------------------------------------------------------- the operations

def same(got, want):
    """equality of numpy arrays, bytes, ints and tuples / lists of them"""
    if isinstance(want, (tuple, list)):
        return isinstance(got, (tuple, list)) and len(got) == len(want) and all(same(g, w) for g, w in zip(got, want))
    if isinstance(want, np.ndarray):
        got = np.asarray(got)
        return got.shape == want.shape and bool((got == want).all())
    return got == want


class Op:
    """changes: the call may write device state (flags, run buffers or scratch), so it takes part in the pairs;
    a reader only fetches"""
    name, changes = "", True

    def needs(self, st):
        return True

    def leave(self, st):
        return st

    def run(self, eng, st):
        raise NotImplementedError

    def expect(self, st):
        return None

    def __repr__(self):
        return self.name


class Load(Op):
    """load, load_file, synth, load_texts with and without offsets: always allowed; the bytes' owners (split, text
    batch, train_split's results) and the ids go, the unpacked rows stay"""

    def __init__(self, name, how):
        self.name, self.how = name, how

    def leave(self, st):
        st = st.copy()
        st.drop_bytes()
        if self.how == "load":
            st.data = DATA
        elif self.how == "file":
            st.data = FILE_DATA
        elif self.how == "synth":
            st.data = synth_data()
        else:
            st.texts = TEXTS if self.how == "texts" else TEXTS2
            st.data = b"".join(st.texts)
        return st

    def run(self, eng, st):
        if self.how == "load":
            return eng.load(DATA)
        if self.how == "synth":
            return eng.synth(*SYNTH)
        if self.how == "file":
            import tempfile
            with tempfile.NamedTemporaryFile() as f:
                f.write(FILE_DATA + b"\0ignored")  # (the corpus ends at the first NUL)
                f.flush()
                return eng.load_file(f.name)
        if self.how == "texts":
            return eng.load_texts(list(TEXTS))
        off = np.cumsum([0] + [len(t) for t in TEXTS2]).astype(np.uint64)
        return eng.load_texts(b"".join(TEXTS2), off)

    def expect(self, st):
        return {"file": len(FILE_DATA), "texts": len(TEXTS), "texts_off": len(TEXTS2)}.get(self.how)


class Trim(Op):
    name = "trim"

    def leave(self, st):
        return St()

    def run(self, eng, st):
        return eng.trim()


class Train(Op):
    """needs bytes that are no text batch; drops the split; leaves ids and merges"""

    def __init__(self, name, cap, fast):
        self.name, self.cap, self.fast = name, cap, fast

    def needs(self, st):
        return st.data is not None and st.texts is None

    def leave(self, st):
        st = st.copy()
        st.drop_ids()
        st.split, st.ts = None, False
        data, cap, fast = st.data, self.cap, self.fast
        st.trained = (data, cap, fast)
        st.ids = Ids("train", lambda: (h_train(data, cap, fast)[1], None, None, h_train(data, cap, fast)[0]),
                     lambda: len(h_train(data, cap, fast)[0]), data=data)
        return st

    def run(self, eng, st):
        return eng.train(self.cap, fast=self.fast)

    def expect(self, st):
        return len(h_train(st.data, self.cap, self.fast)[0])


class Encode(Op):
    """needs bytes that are no text batch; keeps the split and what was trained on it; leaves ids, no documents"""

    def __init__(self, name, win):
        self.name, self.win = name, win

    def needs(self, st):
        return st.data is not None and st.texts is None

    def leave(self, st):
        st = st.copy()
        st.drop_ids()
        data = st.data
        st.ids = Ids("encode", lambda: (h_encode(data), None, None, merges_fixed()), K, data=data)
        return st

    def run(self, eng, st):
        old = os.environ.get("BPE_ENC_WIN")
        os.environ["BPE_ENC_WIN"] = self.win
        try:
            eng.encode(merges_fixed())
            return eng.stats()["enc_path"]
        finally:
            if old is None:
                del os.environ["BPE_ENC_WIN"]
            else:
                os.environ["BPE_ENC_WIN"] = old

    def expect(self, st):
        return None  # (which replay ran is asserted by the GPU test where it matters: a fallback is legal)


class EncodeDocs(Op):
    name = "encode_docs"

    def needs(self, st):
        return st.data is not None and st.texts is None

    def leave(self, st):
        st = st.copy()
        st.drop_ids()
        data = st.data
        st.ids = Ids("docs", lambda: h_encode_docs(data) + (None, merges_fixed()), K, data=data)
        return st

    def run(self, eng, st):
        return eng.encode_docs(doc_cuts(len(st.data) if st.data is not None and st.texts is None else 0), merges_fixed())


class Split(Op):
    """needs bytes; replaces the split and drops train_split's results; the ids stay"""

    def __init__(self, rule, specials):
        self.name = f"split_{rule}" + ("_sp" if specials else "")
        self.rule, self.specials = rule, specials

    def needs(self, st):
        return st.data is not None

    def leave(self, st):
        st = st.copy()
        st.split, st.ts = (self.rule, self.specials), False
        return st

    def run(self, eng, st):
        return eng.split(rule_arg(self.rule), list(self.specials) if self.specials else None)

    def expect(self, st):
        return h_split(st.data, st.texts, self.rule, self.specials)[0].size - 1


class TrainSplit(Op):
    name = "train_split"

    def needs(self, st):
        return st.data is not None and st.texts is None and st.split is not None

    def leave(self, st):
        st = st.copy()
        st.ts = True
        return st

    def run(self, eng, st):
        return eng.train_split(K)

    def expect(self, st):
        return len(h_train_split(st.data, *st.split)[0])


class EncodeSplit(Op):
    name = "encode_split"

    def needs(self, st):
        return st.data is not None and st.split is not None

    def leave(self, st):
        st = st.copy()
        st.drop_ids()
        data, texts, (rule, sp) = st.data, st.texts, st.split
        st.ids = Ids("docs", lambda: h_encode_split(data, texts, rule, sp) + (merges_fixed(),), K, sp, texts, data)
        return st

    def run(self, eng, st):
        return eng.encode_split(merges_fixed())


class MapIds(Op):
    name = "map_ids"

    def needs(self, st):
        return st.ids is not None and not st.mapped

    def leave(self, st):
        st = st.copy()
        st.mapped = True
        return st

    def run(self, eng, st):
        if st.ids is None:
            return eng.map_ids(vocab_for(K, None))
        return eng.map_ids(vocab_for(n_merges_of(st.ids), st.ids.specials))


def n_merges_of(ids):
    return ids.n_merges() if callable(ids.n_merges) else ids.n_merges


class Decode(Op):
    """the decoders take their ids from the caller: always allowed, nothing of the context's state moves"""

    def __init__(self, name, kind):
        self.name, self.kind = name, kind

    def args(self):
        sp = SPECIALS if self.kind in ("special", "vocab") else None
        ids, ido, _ = h_encode_split(DATA, None, "cl100k", sp)
        return ids, ido, sp

    def run(self, eng, st):
        if self.kind == "flat":
            return eng.decode(h_encode(DATA), merges_fixed())
        ids, ido, sp = self.args()
        if self.kind == "vocab":
            v = vocab_for(K, sp)
            return eng.decode_docs(fwd_of(v)[ids], ido, merges_fixed(), specials=list(sp), vocab=v)
        return eng.decode_docs(ids, ido, merges_fixed(), specials=list(sp) if sp else None)

    def expect(self, st):
        import oracle_lib as O
        if self.kind == "flat":
            return O.decode(h_encode(DATA), merges_fixed())
        ids, ido, sp = self.args()
        return h_decode_docs(ids, ido, merges_fixed(), sp or ())


class TokenSpans(Op):
    """needs the ids of encode_docs / encode_split; the caller passes the vocabulary exactly when the ids are mapped"""

    def __init__(self, unit):
        self.name, self.unit = f"token_spans_{unit}", unit

    def needs(self, st):
        return st.ids is not None and st.ids.kind == "docs"

    def leave(self, st):
        st = st.copy()
        st.spans = self.unit
        return st

    def run(self, eng, st):
        if st.ids is None:
            return eng.token_spans(merges_fixed(), unit=self.unit)
        n = n_merges_of(st.ids)
        m = merges_fixed() if n == K else np.stack([np.arange(n) % 256, np.arange(n) % 256], axis=1).astype(np.uint32)
        return eng.token_spans(m, list(st.ids.specials) if st.ids.specials else None,
                               vocab_for(n, st.ids.specials) if st.mapped else None, unit=self.unit)

    def expect(self, st):
        texts, toff = st.text_view()
        ids, _, _, merges = st.ids.value()
        return h_spans(ids, merges, st.ids.specials, texts, toff, self.unit)


class Pack(Op):
    """pack_texts / pack_stream need a text batch and its ids; pack_spans its spans too.  Nothing moves."""

    def __init__(self, what):
        self.name, self.what = f"pack_{what}", what

    def needs(self, st):
        ok = st.texts is not None and st.ids is not None and st.ids.kind == "docs"
        return ok and (self.what != "spans" or st.spans is not None)

    def run(self, eng, st):
        if self.what == "texts":
            return eng.pack_texts(ROW_LEN, PAD_ID, "left")
        if self.what == "spans":
            return eng.pack_spans(ROW_LEN, "left")
        return eng.pack_stream(SEQ_LEN, PAD_ID, BOS, EOS, segments=True, positions=True)

    def expect(self, st):
        import stream_ref
        import texts_ref
        toff = st.ids.value()[2]
        if self.what == "texts":
            return texts_ref.pack_rows(st.cur_ids(), toff, ROW_LEN, PAD_ID, "left")
        if self.what == "spans":
            return pack_span_rows(TokenSpans(st.spans).expect(st), toff, ROW_LEN, "left")
        return stream_ref.pack_stream(st.cur_ids(), toff, SEQ_LEN, PAD_ID, BOS, EOS)[:3]


class Rows(Op):
    """unpack_rows is always allowed and keeps its results in slots of their own until the next unpack or trim;
    fetch_rows and decode_rows need them"""

    def __init__(self, what):
        self.name, self.what = what, what

    def needs(self, st):
        return self.what == "unpack_rows" or st.rows

    def leave(self, st):
        st = st.copy()
        st.rows = True
        return st

    def run(self, eng, st):
        if self.what == "unpack_rows":
            return eng.unpack_rows(rows_fixed(), None, ROWS_PAD, ROWS_STOP, ROWS_SKIP)
        return eng.fetch_rows() if self.what == "fetch_rows" else eng.decode_rows(merges_fixed())

    def expect(self, st):
        return h_decode_rows() if self.what == "decode_rows" else h_rows()


class Reader(Op):
    """a fetch: refused ("call out of order") exactly when what it serves is not there"""
    changes = False

    def __init__(self, name, needs, expect):
        self.name, self._needs, self._expect = name, needs, expect

    def needs(self, st):
        return self._needs(st)

    def run(self, eng, st):
        return getattr(eng, self.name)()

    def expect(self, st):
        return self._expect(st)


def _merges(st):
    # the last training's merges, as long as its run buffers stand; none (0 pairs) otherwise: never an error
    return h_train(*st.trained)[0] if st.trained else np.zeros((0, 2), np.uint32)


def _docs(st):
    return st.ids is not None and st.ids.kind == "docs"


def _special_pieces(st):
    _, piece, index, _ = h_split(st.data, st.texts, *st.split)
    return piece, index


def _piece_table(st):
    t = h_train_split(st.data, *st.split)[1]
    return (np.array([r[0] for r in t], np.uint64), np.array([r[1] for r in t], np.uint32),
            np.array([r[2] for r in t], np.uint32))


def _checksum(st):
    import golden_lib
    return golden_lib.ids_checksum(st.cur_ids())


READERS = [
    Reader("ids", lambda st: st.ids is not None, lambda st: st.cur_ids()),
    Reader("merges", lambda st: True, _merges),
    Reader("doc_offsets", _docs, lambda st: st.ids.value()[1]),
    Reader("split_offsets", lambda st: st.split is not None, lambda st: h_split(st.data, st.texts, *st.split)[0]),
    Reader("special_pieces", lambda st: st.split is not None, _special_pieces),
    Reader("split_merges", lambda st: st.split is not None and st.ts, lambda st: h_train_split(st.data, *st.split)[0]),
    Reader("piece_table", lambda st: st.split is not None and st.ts, _piece_table),
    Reader("text_offsets", lambda st: st.texts is not None and _docs(st), lambda st: st.ids.value()[2]),
    Reader("ids_checksum", lambda st: st.ids is not None, _checksum),
]

OPS = [
    Load("load", "load"), Load("load_texts", "texts"), Load("load_texts_off", "texts_off"), Load("load_file", "file"),
    Load("synth", "synth"),
    Train("train", K, False), Train("train_fast", K, True), Train("train_hash", -1, False), Train("train_fast_hash", -1, True),
    Encode("encode_win", "1"), Encode("encode_glob", "0"), EncodeDocs(), Decode("decode", "flat"), Trim(),
    Split("table", None), Split("table", SPECIALS), Split("cl100k", None), Split("cl100k", SPECIALS),
    Split("o200k", None), Split("o200k", SPECIALS), TrainSplit(), EncodeSplit(),
    MapIds(), Decode("decode_docs", "plain"), Decode("decode_docs_sp", "special"), Decode("decode_docs_vocab", "vocab"),
    TokenSpans("byte"), TokenSpans("char"), Pack("texts"), Pack("spans"), Pack("stream"),
    Rows("unpack_rows"), Rows("fetch_rows"), Rows("decode_rows"),
]
BY_NAME = {op.name: op for op in OPS + READERS}
CHANGING = [op for op in OPS if op.changes]


# ---------------------------------------------------------------- the model and the sequences

def step(st, op):
    """(legal, the state after the call): a refused call leaves the state as it was"""
    if not op.needs(st):
        return False, st
    return True, op.leave(st)


def walk(names):
    """the model over a sequence of operation names: [(op, legal, state before, state after)]"""
    st, out = St(), []
    for name in names:
        op = BY_NAME[name]
        legal, after = step(st, op)
        out.append((op, legal, st, after))
        st = after
    return out


def valid_readers(st):
    return {r.name for r in READERS if r.needs(st)}


@functools.lru_cache(maxsize=None)
def shortest_path(name):
    """the fewest state-changing calls after which a fresh context allows `name` (breadth first, in OPS' order)"""
    target = BY_NAME[name]
    seen, queue = {St().key()}, [((), St())]
    while queue:
        path, st = queue.pop(0)
        if target.needs(st):
            return path
        for op in CHANGING:
            legal, after = step(st, op)
            if legal and after.key() not in seen:
                seen.add(after.key())
                queue.append((path + (op.name,), after))
    raise AssertionError(f"no sequence of calls allows {name}")


def pairs(first=None):
    """every ordered pair (A, B) of state-changing operations as a sequence of names: the shortest path to A's
    precondition, A, B.  first: the pairs of that A alone."""
    for a in CHANGING:
        if first is None or a.name == first:
            for b in CHANGING:
                yield shortest_path(a.name) + (a.name, b.name)

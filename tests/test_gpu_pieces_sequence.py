"""The pieces path as one sequence on one context: split, train_split, encode_split and decode under one rule
after another, with and without specials.  Every step leaves device scratch behind that a later step of
another kind reuses or replaces (the cover bitmap and the match list, the piece table and its entries, the
post-pass's lists, the chain effects), so two buffers that share memory while both are live show up here as a
wrong result of a later step; the per-rule tests run one kind of operation per context and would not see it.
The expected offsets, special pieces and merges come from the host definitions (api.split_host,
api.split_host_special, train_split_ref.train).  The expected ids are what the per-rule tests compare against:
api.encode_batch over the host's pieces, which runs the document encoder on the device through another context
(the C layer's), so they are independent of this context's scratch but not of that encoder; the decode of the ids
back to the text is the check of them that shares nothing with it."""
import numpy as np
import pytest

import special_ref as SR
import train_split_ref as TR
from llmtokenizer_amd import api

pytestmark = pytest.mark.gpu

EOT = b"<|endoftext|>"
SPECIALS = [EOT, b"\xac|x|"]
ITEMS = [b"'", b"s", b"T", b"re", b"LL", b"a", b"1", b"23", b"4567", b"!", b"\n", b"\n\n", b"\r\n", b" ", b"  ", b"\t",
         b"word", b" the", b" the", b"!\n", b" \n", b"\n  ", b"\x80", b"\xe2\x82", b"\xff"]
ITEMS += [s.encode() for s in ("é", "Ж", "中", "\U00010400", "٣", "½", "　", "—", "\U0001f600")]
MERGES = 16


def mixed(n, seed):
    """n bytes of the items above in random order, one item in 600 a special (cut at n)"""
    rng = np.random.default_rng(seed)
    out, size = [], 0
    while size < n:
        for k, r in zip(rng.integers(0, len(ITEMS), 1024).tolist(), rng.integers(0, 600, 1024).tolist()):
            out.append(SPECIALS[r] if r < len(SPECIALS) else ITEMS[k])
            size += len(out[-1])
    return b"".join(out)[:n]


def cut(data, off):
    return [data[int(a):int(b)] for a, b in zip(off, off[1:])]


class Host:
    """what the host definitions say of one split of `data`: the offsets, the special pieces, the pieces that
    are no specials, the first MERGES merges trained on those, and the ids and id offsets under these merges"""

    def __init__(self, data, rule, specials):
        self.data, self.specials = data, specials
        if specials is None:
            self.off = api.split_host(data, rule)
            self.piece, self.index = np.zeros(0, np.uint64), np.zeros(0, np.uint32)
        else:
            self.off, self.piece, self.index = api.split_host_special(data, rule, specials)
        self.pieces = cut(data, self.off)
        self.which = dict(zip(self.piece.tolist(), self.index.tolist()))
        self.plain = [p for i, p in enumerate(self.pieces) if i not in self.which]

    def train(self):
        want, self.stop, _ = TR.train(self.plain, MERGES)
        assert len(want) == MERGES
        self.merges = np.array(want, dtype=np.uint32).reshape(-1, 2)

    def ids(self):
        """[256 + MERGES + j] for a piece that is special j, encode_batch's ids for every other piece"""
        bids, boff = api.encode_batch(self.plain, self.merges)
        parts, k = [], 0
        for i in range(len(self.pieces)):
            if i in self.which:
                parts.append(np.array([256 + MERGES + self.which[i]], np.uint32))
            else:
                parts.append(bids[int(boff[k]):int(boff[k + 1])])
                k += 1
        return np.concatenate(parts), np.cumsum([0] + [p.size for p in parts]).astype(np.uint64)


def check_split(eng, host, rule, step):
    assert eng.split(rule, host.specials) == len(host.pieces), step
    got = eng.split_offsets()
    assert got.dtype == np.uint64 and got.size == host.off.size and (got == host.off).all(), step
    piece, index = eng.special_pieces()
    assert piece.tolist() == host.piece.tolist() and index.tolist() == host.index.tolist(), step
    assert eng.split_special_info()["matches"] == host.piece.size, step


def check_train(eng, host, step):
    host.train()
    assert eng.train_split(MERGES) == MERGES, step
    assert eng.split_merges().tolist() == host.merges.tolist(), step
    info = eng.train_split_info()
    assert info["pieces"] == len(host.pieces) and info["stop_reason"] == host.stop, step
    st, ln, ct = eng.piece_table()
    table = {host.data[int(s):int(s) + int(n)] for s, n in zip(st, ln)}
    assert int(ct.sum()) == len(host.plain) and table == set(host.plain), step


def check_encode(eng, host, step):
    want, want_off = host.ids()
    eng.encode_split(host.merges)
    ids, id_off = eng.ids(), eng.doc_offsets()
    assert id_off.tolist() == want_off.tolist(), step
    assert ids.size == want.size and (ids == want).all(), step
    return ids, id_off


def test_one_context_through_the_whole_pieces_path():
    T = api.split_info()["tile"]
    assert T == 4096
    data = mixed(3 * T + 17, 21)
    assert len(data) == 3 * T + 17 and all(data.count(s) >= 3 for s in SPECIALS)
    tables = SR.random_rule(1)
    eng = api.Engine(0)
    try:
        eng.load(data)
        h = Host(data, "cl100k", SPECIALS)
        assert h.piece.size >= 6
        check_split(eng, h, "cl100k", 1)
        check_train(eng, h, 2)
        ids, id_off = check_encode(eng, h, 3)
        raw, byte_off = eng.decode_docs(ids, id_off, h.merges, specials=SPECIALS)
        assert raw == data and byte_off.tolist() == h.off.tolist(), 4
        check_split(eng, Host(data, "words", SPECIALS), "words", 5)
        h = Host(data, "gpt2_unicode", None)
        check_split(eng, h, "gpt2_unicode", 6)
        check_train(eng, h, 7)
        ids, id_off = check_encode(eng, h, 8)
        raw, byte_off = eng.decode_docs(ids, id_off, h.merges)
        assert raw == data and byte_off.tolist() == h.off.tolist(), 8
        h = Host(data, tables, [])  # (the host definition takes tables only through the call with specials)
        h.specials = None
        check_split(eng, h, tables, 9)
        assert h.off.tolist() == [0] + [int(a) for a in np.flatnonzero(_starts(data, *tables)) + 1] + [len(data)]
        check_split(eng, Host(data, "cl100k", None), "cl100k", 10)
    finally:
        eng.close()


def _starts(data, cls, brk):
    """the two-table rule restated (bpe_gpu.h): a piece starts at i > 0 where bit cls[b[i]] of brk[cls[b[i - 1]]] is set"""
    c = np.asarray(cls)[np.frombuffer(data, np.uint8)].astype(np.int64)
    return (np.asarray(brk).astype(np.int64)[c[:-1]] >> c[1:]) & 1

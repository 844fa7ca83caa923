"""The definition of a text batch's split, restated in Python over the host split of one text
(api.split_host): the pieces of text k are those of a split of text k alone, shifted to the bytes of the
texts joined with nothing between them; an empty text has no piece.  No GPU."""
import numpy as np

from llmtokenizer_amd import api


def as_bytes(texts):
    return [t.encode("utf-8") if isinstance(t, str) else bytes(t) for t in texts]


def byte_offsets(texts):
    """uint64[T + 1]: where each text begins in the plain join"""
    off = np.zeros(len(texts) + 1, dtype=np.uint64)
    if len(texts):
        off[1:] = np.cumsum([len(t) for t in as_bytes(texts)], dtype=np.uint64)
    return off


def split_texts(texts, rule, specials=None):
    """(piece offsets uint64 in the plain join, the piece starts followed by the joined length;
    pieces per text int64[T]; the special pieces as (piece index, special index) pairs in order)"""
    texts = as_bytes(texts)
    starts, per_text, special_pieces, base = [], [], [], 0
    for t in texts:
        if not t:
            per_text.append(0)
            continue
        if specials:
            off, piece, index = api.split_host_special(t, rule, specials)
            special_pieces += [(len(starts) + int(p), int(j)) for p, j in zip(piece, index)]
        else:
            off = api.split_host(t, rule)
        assert int(off[0]) == 0 and int(off[-1]) == len(t)
        starts += [base + int(o) for o in off[:-1]]
        per_text.append(off.size - 1)
        base += len(t)
    return np.array(starts + [base], dtype=np.uint64), np.array(per_text, dtype=np.int64), special_pieces


def gapped(texts):
    """the bytes a context keeps: every text followed by one NUL"""
    return b"".join(t + b"\0" for t in as_bytes(texts))


def pack_rows(ids, text_off, row_len, pad_id, side):
    """(rows uint32[T, row_len], lens uint32[T]) of api.Engine.pack_texts, with numpy"""
    T = len(text_off) - 1
    rows = np.full((T, row_len), pad_id, dtype=np.uint32)
    lens = np.zeros(T, dtype=np.uint32)
    for k in range(T):
        seq = ids[int(text_off[k]):int(text_off[k + 1])]
        if seq.size > row_len:
            seq = seq[:row_len] if side == "right" else seq[seq.size - row_len:]
        rows[k, :seq.size] = seq
        lens[k] = seq.size
    return rows, lens

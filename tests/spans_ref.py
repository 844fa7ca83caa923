"""Token spans in pure Python (test infrastructure): the bytes of every token from Vocab.token_bytes() and the
specials, then the two formulas of bpe_gpu.h, "Token spans".  The yardstick beside the host C definition
(bpe_token_spans_host) for tests/test_spans_host.py and tests/test_gpu_spans.py."""
import numpy as np


def token_bytes_by_id(vocab):
    """{vocabulary id: the token's bytes} of a vocab.Vocab"""
    tb = vocab.token_bytes()
    ids = list(vocab.byte_ids) + list(vocab.merge_ids)
    out = {int(i): tb[k] for k, i in enumerate(ids)}
    out.update({int(i): s for s, i in zip(vocab.specials, vocab.special_ids)})
    return out


def internal_token_bytes(merges, specials=()):
    """the token's bytes by internal id: bytes, merges, specials"""
    out = [bytes([b]) for b in range(256)]
    for a, b in np.asarray(merges, dtype=np.uint32).reshape(-1, 2).tolist():
        out.append(out[a] + out[b])
    return out + [bytes(s) for s in specials]


def lead(t, p):
    """bytes of t[0:p] that are no UTF-8 continuation bytes"""
    return sum((b & 0xC0) != 0x80 for b in t[:p])


def spans_of_text(tokens, text, unit):
    """[(s, e)] of the tokens (a list of bytes) that tile text; AssertionError when they do not"""
    out, p = [], 0
    for tok in tokens:
        bs, be = p, p + len(tok)
        assert text[bs:be] == tok, (bs, be, tok, text[bs:be])
        out.append((bs, be) if unit == "byte" else (max(lead(text, bs + 1), 1) - 1, lead(text, be)))
        p = be
    assert p == len(text), (p, len(text))
    return out


def spans_fast(lens, text, unit):
    """the same from the tokens' lengths alone, in numpy (for large texts): uint32[n, 2]"""
    lens = np.asarray(lens, dtype=np.int64)
    be = np.cumsum(lens)
    bs = be - lens
    assert (int(be[-1]) if lens.size else 0) == len(text)
    if unit == "byte":
        return np.stack([bs, be], axis=1).astype(np.uint32)
    b = np.frombuffer(bytes(text), dtype=np.uint8)
    pref = np.concatenate([[0], np.cumsum((b & 0xC0) != 0x80)]).astype(np.int64)  # pref[p] = lead(p)
    return np.stack([np.maximum(pref[bs + 1], 1) - 1, pref[be]], axis=1).astype(np.uint32)


def batch_spans(token_of, ids, text_off, texts, unit):
    """uint32[n, 2]: text k has the ids ids[text_off[k]:text_off[k + 1]]; token_of maps an id to its bytes"""
    out = []
    for k, t in enumerate(texts):
        toks = [token_of[int(i)] for i in ids[int(text_off[k]):int(text_off[k + 1])]]
        out += spans_of_text(toks, t, unit)
    return np.array(out, dtype=np.uint32).reshape(-1, 2)

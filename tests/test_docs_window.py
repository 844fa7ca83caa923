"""Window geometry of the document encoder (bpe_gpu_docs_window, the function
k_enc_docs itself uses) against a brute-force restatement; no GPU."""
import random

import numpy as np
import pytest

from llmtokenizer_amd import api

W = 2048  # positions of a window (core + 2 * halo)


def _brute(off, n, core, halo, w):
    """the definition, by linear scans over the offsets"""
    s0 = w * core
    s1 = min(n, s0 + core)
    starts = [int(x) for x in off]  # off[ndocs] == n counts as a document start
    dl = max(x for x in starts if x <= s0)
    dr = min(x for x in starts if x >= s1)
    L = max(s0 - halo, dl)
    R = min(s1 + halo, dr)
    return {"L": L, "R": R, "lunk": L not in starts, "runk": R not in starts,
            "first_doc": min(d for d, x in enumerate(starts) if x >= L),
            "doc_starts": sum(1 for x in starts if L <= x <= R)}


def _offsets(rng, n, core):
    """document starts over [0, n]: empty, 1-byte and short documents, some
    longer than three cores, and starts next to every core boundary"""
    cuts = {0, n}
    kind = rng.randrange(4)
    if kind == 0:  # boundaries at k * core + {-1, 0, 1}
        for k in range(n // core + 2):
            for dlt in (-1, 0, 1):
                if rng.random() < 0.7:
                    cuts.add(min(n, max(0, k * core + dlt)))
    pos = 0
    while pos < n:
        pos += rng.choice([1, 1, 2, rng.randint(3, 40), rng.randint(200, 900), rng.randint(3 * core, 4 * core)])
        if kind != 3 or rng.random() < 0.2:  # (kind 3: few, long documents)
            cuts.add(min(pos, n))
    off = sorted(cuts)
    out = []
    for x in off:  # runs of empty documents, leading and trailing ones included
        out.extend([x] * (1 + (rng.random() < 0.15) * rng.randint(1, 3)))
    return np.array(out, dtype=np.uint64)


@pytest.mark.parametrize("halo", [16, 48, 512])
def test_docs_window_matches_brute_force(halo):
    rng = random.Random(1000 + halo)
    core = W - 2 * halo
    sizes = [1, 2, core - 1, core, core + 1, 3 * core, 20000] + [rng.randint(1, 20000) for _ in range(6)]
    seen = set()
    for n in sizes:
        off = _offsets(rng, n, core)
        assert off[0] == 0 and off[-1] == n and (np.diff(off.astype(np.int64)) >= 0).all()
        for w in range((n + core - 1) // core):
            got = api.docs_window(off, n, core, halo, w)
            assert got == _brute(off, n, core, halo, w), (halo, n, w, off.tolist())
            assert got["R"] - got["L"] <= W
            seen.add((got["lunk"], got["runk"]))
    assert seen == {(False, False), (False, True), (True, False), (True, True)}


def test_docs_window_one_document_is_the_plain_window():
    """no interior boundary: the window of the single-stream encoder, clipped at the stream's ends"""
    core, halo, n = 1952, 48, 7000
    for w in range(4):
        got = api.docs_window([0, n], n, core, halo, w)
        s0, s1 = w * core, min(n, (w + 1) * core)
        assert (got["L"], got["R"]) == (max(0, s0 - halo), min(n, s1 + halo))
        assert (got["lunk"], got["runk"]) == (got["L"] > 0, got["R"] < n)


def test_docs_window_rejects_bad_arguments():
    with pytest.raises(api.BpeError):
        api.docs_window([1, 10], 10, 1952, 48, 0)  # first offset not 0
    with pytest.raises(api.BpeError):
        api.docs_window([0, 9], 10, 1952, 48, 0)  # last offset not n
    with pytest.raises(api.BpeError):
        api.docs_window([0, 6, 5, 10], 10, 1952, 48, 0)  # a decrease
    with pytest.raises(api.BpeError):
        api.docs_window([0, 10], 10, 1952, 48, 1)  # no such window

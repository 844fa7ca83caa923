"""The restatement of training on pieces (tests/train_split_ref.py) against the CPU
oracle and the examples of bpe_gpu.h.  CPU only."""
import numpy as np

import oracle_lib as O
import train_split_ref as R
from llmtokenizer_amd.synth import english_like

LINES_CLS = np.zeros(256, np.uint8)
LINES_CLS[10] = 1
LINES_BRK = np.zeros(16, np.uint16)
LINES_BRK[1] = 0x3


def test_one_piece_equals_the_oracle_before_the_first_tie():
    """a corpus held as one piece is the stream: up to the first tied argmax no tie rule is needed"""
    data = english_like(65536)
    merges, stop, first_tie = R.train([data], 40)
    assert stop == 2 and len(merges) == 40
    assert first_tie is None or first_tie >= 32, first_tie
    for mode in (O.EMU, O.RULE):
        om = O.train(data, 32, mode)[0]
        assert [tuple(int(x) for x in m) for m in om] == merges[:32], mode


def test_the_line_example():
    data = b"ab\n" * 8
    pieces = R.pieces_of(data, LINES_CLS, LINES_BRK)
    assert pieces == [b"ab\n"] * 8
    assert R.train(pieces) == ([(97, 98), (256, 10)], 1, 0)  # (97, 98) and (98, 10) tie at 8: the smaller a
    # the stream goes on to pairs no line holds
    stream = R.train([data])[0]
    assert stream[:4] == [(97, 98), (256, 10), (257, 257), (258, 258)]


def test_runs_ties_and_stops():
    assert R.train([b"aaa"]) == ([(97, 97)], 1, None)          # z a: no pair seen twice is left
    assert R.train([b"aaaa"])[0] == [(97, 97), (256, 256)][:1]  # z z once: count 1 stops
    assert R.train([b"ab", b"ab", b"cd", b"cd"]) == ([(97, 98), (99, 100)], 1, 0)
    assert R.train([b"abab"] * 2, 1) == ([(97, 98)], 2, None)
    assert R.train([b"abab"] * 2, 5, engine_cap=1) == ([(97, 98)], 3, None)
    assert R.train([b"ab"] * 2, 1) == ([(97, 98)], 1, None)     # the rule is checked before the cap
    assert R.train([]) == ([], 1, None) and R.train([b"a"]) == ([], 1, None)
    assert R.train([b"ab"], 0) == ([], 1, None) and R.train([b"ab"] * 2, 0) == ([], 2, None)
    assert R.pieces_of(b"", LINES_CLS, LINES_BRK) == []

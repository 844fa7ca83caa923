"""regime_lib (the helper of test_gpu_regimes.py) against the oracle, on the CPU:
the vectorised replay is the oracle's replace pass, a == a runs included, and
the corpora put the live count where they say."""
import numpy as np
import pytest

import oracle_lib as O
import regime_lib as RL


def _slow_replay(data, merges):
    """token by token, as the oracle's replace pass is written"""
    tok = list(data)
    live, count = [], []
    for k, (a, b) in enumerate(merges.tolist()):
        live.append(len(tok))
        count.append(sum(1 for i in range(len(tok) - 1) if tok[i] == a and tok[i + 1] == b))
        out, i = [], 0
        while i < len(tok):
            if i + 1 < len(tok) and tok[i] == a and tok[i + 1] == b:
                out.append(256 + k)
                i += 2
            else:
                out.append(tok[i])
                i += 1
        tok = out
    return live + [len(tok)], count, tok


def _runs(seed):
    """runs of every length 1..12 of two bytes, odd and even, abutting and apart"""
    rng = np.random.default_rng(seed)
    return b"".join(bytes([97 + int(c)]) * int(k) + (b"" if c else b"-" * int(k % 3))
                    for k, c in zip(rng.integers(1, 13, 400), rng.integers(0, 2, 400)))


@pytest.mark.parametrize("data", [_runs(1), _runs(2), b"a" * 1001 + b"b" + b"a" * 1000, b"a" * 7, b"aaa" * 3 + b"ab" * 50],
                         ids=["runs1", "runs2", "two_runs", "pair", "mixed"])
def test_replay_is_the_oracles_replace_pass(data):
    merges, ids, _ = O.train(data, -1, O.EMU)
    assert (merges[:, 0] == merges[:, 1]).any()  # an a == a merge is among them
    live, count, tok = RL.replay(data, merges)
    slive, scount, stok = _slow_replay(data, merges)
    assert live.tolist() == slive and count.tolist() == scount
    assert tok.tolist() == stok == ids.tolist()


def test_run_tail_live_counts():
    first = np.array([[RL.RUN_BYTE, RL.RUN_BYTE]])
    for L in (RL.TRACK_LIMIT, RL.DYN_LIMIT):
        for d in (-1, 0, 1):
            data = RL.run_tail(L, d)
            live, count, _ = RL.replay(data, first)
            assert live.tolist() == [2 * (L + d) - 9000, L + d] and count[0] == len(data) - 9000 - 1
    live, _, _ = RL.replay(RL.run_tail_both(), first)
    assert live[0] > RL.TRACK_LIMIT > live[1] > RL.DYN_LIMIT > (live[1] - 30000) // 2 + 30000


def test_oracle_gives_the_reference_golden():
    """the reference's own result on run_tail(2^21, 0) (five runs of the unmodified reference agreed) is
    the oracle's emulation, not the schedule-free rule"""
    data, fx = RL.reference_golden()
    assert data == RL.run_tail(RL.TRACK_LIMIT, 0)
    em, ei, _ = O.train(data, -1, O.EMU)
    RL.check_golden(fx, em, ei)
    rm, _, _ = O.train(data, -1, O.RULE)
    assert RL.diff_merges(em, rm)


def test_batch_cut_live_counts():
    for d in (-1, 0, 1):
        data = RL.batch_cut(d)
        bulk = np.array([[0x80, 0x81], [0x82, 0x83], [0x84, 0x85]])
        live, count, _ = RL.replay(data, bulk)
        assert live[1] == RL.TRACK_LIMIT + d and live[0] - count[0] == live[1]
        assert count[0] > count[1] > count[2] and live[2] < RL.TRACK_LIMIT
        # every other pair is far behind the three
        t = np.frombuffer(data, np.uint8).astype(np.int64)
        _, c = np.unique(t[:-1] * 256 + t[1:], return_counts=True)
        assert np.sort(c)[-4] * 4 < count[2]

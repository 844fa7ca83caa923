#!/usr/bin/env python3
"""decode_rows(errors="replace") against what it replaces, and what the new entry points cost unused (DESIGN section
7.13).

The workload: --rows rows of --len byte-level ids (an empty merge list: an id is a byte), unpacked once and left on
the device, in two fillings: "ascii" (english_like) and "mixed" (the same with about 1 % of its bytes in 2-byte
characters and 0.01 % replaced by FF, so rows also end inside characters).  Per filling one checked warm pass (both
routes give the same strings), then --repeats alternated repeats of every leg in one process, reported as median
[min .. max]:

  device        Engine.decode_rows(errors="replace") and a strict str(bytes, "utf-8") per row: what
                Tokenizer.decode_rows does with errors="replace"
  host          the parent commit's way to the same strings: Engine.decode_rows() and bytes.decode("utf-8",
                "replace") per row
  device_hold   the same with errors="hold": the strings and the held counts
  host_hold     the parent's way to those: an incremental decoder per row, decode(final=False) and getstate()
  device_bytes  Engine.decode_rows(errors="replace") alone: against raw_old, what the repair adds to a decode
  raw_new       bpe_gpu_decode_rows_text with BPE_TEXT_RAW, by its C call
  raw_old       bpe_gpu_decode_rows, by Engine.decode_rows()

The legs of a group (device / host; device_hold / host_hold; device_bytes / raw_new / raw_old) alternate, and the
one that goes first rotates from repeat to repeat.  One JSON line.  Needs a GPU; there is no CPU path.
"""
import argparse
import codecs
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from llmtokenizer_amd import api  # noqa: E402
from llmtokenizer_amd.synth import english_like  # noqa: E402
from split_bench import med  # noqa: E402

NONE = np.zeros((0, 2), dtype=np.uint32)


def filling(kind, n):
    d = np.frombuffer(english_like(n), dtype=np.uint8)[:n].copy()
    if kind == "mixed":
        rng = np.random.default_rng(7)
        at = rng.choice(n // 2, n // 200, replace=False) * 2  # 0.5 % of the byte pairs: 1 % of the bytes
        d[at], d[at + 1] = 0xC3, 0xA9
        d[rng.choice(n, n // 10000, replace=False)] = 0xFF
    return d


def cut(out, bo):
    return [out[int(a):int(b)] for a, b in zip(bo, bo[1:])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=8192)
    ap.add_argument("--len", type=int, default=2048)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    eng = api.Engine(a.device)

    def host_hold():
        out = []
        for t in cut(*eng.decode_rows(NONE)):
            d = codecs.getincrementaldecoder("utf-8")("replace")
            out.append((d.decode(t, final=False), len(d.getstate()[0])))
        return out

    def device_hold():
        out, bo, held = eng.decode_rows(NONE, errors="hold")
        return list(zip((str(t, "utf-8") for t in cut(out, bo)), held.tolist()))

    legs = {
        "device": lambda: [str(t, "utf-8") for t in cut(*eng.decode_rows(NONE, errors="replace")[:2])],
        "host": lambda: [t.decode("utf-8", "replace") for t in cut(*eng.decode_rows(NONE))],
        "device_hold": device_hold,
        "host_hold": host_hold,
        "device_bytes": lambda: eng.decode_rows(NONE, errors="replace"),
        "raw_new": lambda: eng._decode_text(eng.L.bpe_gpu_decode_rows_text, (eng.ctx, None, 0, None, None, 0), a.rows, "raw"),
        "raw_old": lambda: eng.decode_rows(NONE),
    }
    groups = [["device", "host"], ["device_hold", "host_hold"], ["device_bytes", "raw_new", "raw_old"]]
    res = {"rows": a.rows, "len": a.len, "bytes": a.rows * a.len}
    for kind in ("ascii", "mixed"):
        eng.unpack_rows(filling(kind, a.rows * a.len).astype(np.uint32).reshape(a.rows, a.len))
        if legs["device"]() != legs["host"]() or legs["device_hold"]() != legs["host_hold"]() or \
                legs["raw_new"]()[0] != legs["raw_old"]()[0]:
            sys.exit(f"utf8_bench: the two routes differ on {kind}")
        times = {k: [] for k in legs}
        for g in groups:  # a group's legs alternate, and the one that goes first rotates from repeat to repeat
            for r in range(a.repeats):
                for k in g[r % len(g):] + g[:r % len(g)]:
                    t0 = time.perf_counter()
                    legs[k]()
                    times[k].append(time.perf_counter() - t0)
        res[kind] = {k: med(v) for k, v in times.items()}
    eng.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The long-piece kernel (encode_long.hip) against the per-document fallback.

The merge list is the first --merges merges train_split learns on an english_like sample under "cl100k", padded
beyond 65,279 merges by records that never match, as encode_piece_bench.py's "no plan" leg.  A batch is --short
short documents (the sample's words) with --count long pieces of one kind and one length spread evenly among
them; kinds: random letters, one repeated letter, english_like text without its spaces; lengths: 2 KiB, 8 KiB and
the kernel's limit.  Documents go through Engine.encode_docs, which ends in the engine's own stream synchronise.

  short        the short documents alone, encoder="piece_long" and encoder="piece": what the extra launch costs
  piece_long   every (kind, length) batch: median of --repeats alternated repeats after a checked warm pass, the
               time beyond the short-only batch per long piece, and the rounds of the slowest piece
  parent       encoder="piece" (the parent's path: each long piece alone through the fallback) on --parent-count
               long pieces of each (kind, length), one run each, not warmed: about a second a piece

One JSON line.  Needs a GPU; there is no CPU path.
"""
import argparse
import json
import os
import random
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from llmtokenizer_amd import api  # noqa: E402
from llmtokenizer_amd.synth import english_like  # noqa: E402


def med(xs):
    xs = sorted(xs)
    return {"median": round(xs[len(xs) // 2], 3), "min": round(xs[0], 3), "max": round(xs[-1], 3), "n": len(xs)}


def long_pieces(kind, length, count, sample, rng):
    if kind == "repeat":
        return [b"l" * length] * count
    if kind == "letters":
        g = np.random.default_rng(rng.randrange(1 << 30))
        return [bytes(row) for row in g.integers(97, 123, size=(count, length), dtype=np.uint8)]
    dense = sample.replace(b" ", b"").replace(b"\n", b"")
    return [dense[s:s + length] for s in (rng.randrange(len(dense) - length) for _ in range(count))]


def batch(short, longs):
    """the short documents with the long ones spread evenly among them"""
    docs, step = [], max(1, len(short) // max(1, len(longs)))
    for i, d in enumerate(longs):
        docs += short[i * step:(i + 1) * step] + [d]
    return docs + short[len(longs) * step:]


def main():
    t0 = time.perf_counter()
    ap = argparse.ArgumentParser()
    ap.add_argument("--sample", type=int, default=1 << 22)
    ap.add_argument("--merges", type=int, default=8192)
    ap.add_argument("--pad-to", type=int, default=70000)
    ap.add_argument("--short", type=int, default=200000)
    ap.add_argument("--count", type=int, default=512)
    ap.add_argument("--parent-count", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    if api.device_count() < 1:
        sys.exit("encode_long_bench: no GPU")
    M = api.long_piece_info()["piece_max"]
    sample = english_like(args.sample)
    merges = api.train_split(sample, rule="cl100k", max_merges=args.merges, device=args.device)
    k = args.pad_to - len(merges)
    pad = np.stack([np.ones(k, np.uint32), 255 + len(merges) + np.arange(k, dtype=np.uint32)], axis=1)
    pad[0] = (1, 2)
    padded = np.vstack([merges, pad])
    print(f"encode_long_bench: {len(padded)} merges ({time.perf_counter() - t0:.1f} s)", file=sys.stderr, flush=True)
    short = sample.split(b" ")[:args.short]
    rng = random.Random(11)
    e = api.Engine(args.device)

    def run(docs, encoder):
        """ms of one encode_docs of docs (loaded before the clock starts)"""
        e.load(b"".join(docs))
        off = np.cumsum([0] + [len(d) for d in docs]).astype(np.uint64)
        t = time.perf_counter()
        e.encode_docs(off, padded, encoder=encoder)
        return (time.perf_counter() - t) * 1e3

    cases = {(kind, n): batch(short, long_pieces(kind, n, args.count, sample, rng))
             for kind in ("letters", "repeat", "english") for n in (2048, 8192, M)}
    info = {}
    for key, docs in cases.items():  # warm
        run(docs, "piece_long")
        info[key] = dict(e.long_info(), docs_fallback=e.docs_info()["docs_fallback"])
        if info[key]["long_pieces"] != args.count or info[key]["docs_fallback"]:
            sys.exit(f"encode_long_bench: {key}: {info[key]}")
    run(short, "piece_long")
    run(short, "piece")
    times = {key: [] for key in cases}
    t_short = {"piece_long": [], "piece": []}
    for _ in range(args.repeats):
        for enc in t_short:
            t_short[enc].append(run(short, enc))
        for key, docs in cases.items():
            times[key].append(run(docs, "piece_long"))
    base = med(t_short["piece_long"])["median"]
    res = {"bench": "encode_long", "merges": len(padded), "short_docs": len(short), "short_bytes": sum(map(len, short)),
           "count": args.count, "long_piece_info": api.long_piece_info(),
           "short_ms": {enc: med(t) for enc, t in t_short.items()}, "piece_long": {}, "parent": {}}
    for key, ts in times.items():
        m = med(ts)
        res["piece_long"]["%s-%d" % key] = {"ms": m, "ms_per_long_piece": round((m["median"] - base) / args.count, 5),
                                            "long_rounds": info[key]["long_rounds"], "workgroups": info[key]["workgroups"]}
    for key, docs in cases.items():  # the parent's path on a handful of the same pieces, checked against the new one
        few = batch(short[:1000], [d for d in docs if len(d) == key[1]][:args.parent_count])
        tp = run(few, "piece")
        fb, want = e.docs_info()["docs_fallback"], e.ids_checksum()
        tn = run(few, "piece_long")
        if e.ids_checksum() != want or fb != args.parent_count:
            sys.exit(f"encode_long_bench: {key}: the two encoders disagree")
        res["parent"]["%s-%d" % key] = {"ms_per_long_piece": round((tp - tn) / args.parent_count, 2), "pieces": fb}
        print(f"encode_long_bench: parent {key} ({time.perf_counter() - t0:.1f} s)", file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    e.close()


if __name__ == "__main__":
    main()

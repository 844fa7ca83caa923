#!/usr/bin/env python3
"""BPE-dropout (encode_drop.hip) against the deterministic piece-local replay of the same build.

The merge list is encode_piece_bench.py's "no plan" list: the first --merges merges train_split learns on an
english_like sample under "cl100k", padded beyond 65,279 merges by records that never match.

  tiles   --size bytes of the sample, split by "cl100k" (no piece longer than a tile takes): Engine.encode_split,
          encoder="piece_long", without dropout and with dropout=--p
  long    encode_long_bench.py's batches at the long kernel's limit: --short short documents with --count long
          pieces of one kind among them (random letters, one repeated letter, english_like without its spaces):
          Engine.encode_docs, the same two ways

Each pair is alternated, --repeats times after a warm pass; a fresh seed every dropout run.  Per leg: the median
and range in ms, the ids, and the rounds of the slowest tile and long piece, which tell where the time goes.  One
JSON line.  Needs a GPU; there is no CPU path.
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
from encode_long_bench import batch, long_pieces, med  # noqa: E402


def main():
    t0 = time.perf_counter()
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1 << 26)
    ap.add_argument("--sample", type=int, default=1 << 22)
    ap.add_argument("--merges", type=int, default=8192)
    ap.add_argument("--pad-to", type=int, default=70000)
    ap.add_argument("--short", type=int, default=200000)
    ap.add_argument("--count", type=int, default=512)
    ap.add_argument("--p", type=float, default=0.1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    if api.device_count() < 1:
        sys.exit("encode_drop_bench: no GPU")
    M = api.long_piece_info()["piece_max"]
    sample = english_like(args.sample)
    merges = api.train_split(sample, rule="cl100k", max_merges=args.merges, device=args.device)
    k = args.pad_to - len(merges)
    pad = np.stack([np.ones(k, np.uint32), 255 + len(merges) + np.arange(k, dtype=np.uint32)], axis=1)
    pad[0] = (1, 2)
    padded = np.vstack([merges, pad])
    print(f"encode_drop_bench: {len(padded)} merges ({time.perf_counter() - t0:.1f} s)", file=sys.stderr, flush=True)
    e = api.Engine(args.device)
    seeds = iter(range(1, 1 << 30))

    def timed(call, p):
        kw = {"dropout": p, "seed": next(seeds)} if p else {}
        t = time.perf_counter()
        call(padded, encoder="piece_long", **kw)
        ms = (time.perf_counter() - t) * 1e3
        return ms, {"ids": e.stats()["n_out"], "tile_rounds": e.docs_info()["rounds"], "long_rounds": e.long_info()["long_rounds"],
                    "docs_fallback": e.docs_info()["docs_fallback"]}

    def pair(call):
        """{"piece_long", "dropout"}: alternated runs of the batch the engine holds"""
        legs = {"piece_long": 0.0, "dropout": args.p}
        info = {name: timed(call, p)[1] for name, p in legs.items()}  # warm
        if any(i["docs_fallback"] for i in info.values()):
            sys.exit(f"encode_drop_bench: a document went through the fallback: {info}")
        ts = {name: [] for name in legs}
        for _ in range(args.repeats):
            for name, p in legs.items():
                ts[name].append(timed(call, p)[0])
        out = {name: dict(info[name], ms=med(ts[name])) for name in legs}
        out["ratio"] = round(out["dropout"]["ms"]["median"] / out["piece_long"]["ms"]["median"], 3)
        return out

    res = {"bench": "encode_drop", "p": args.p, "merges": len(padded), "long_piece_info": api.long_piece_info()}
    text = (sample * (args.size // len(sample) + 1))[:args.size]
    e.load(text)
    pieces = e.split("cl100k")
    res["tiles"] = dict(pair(e.encode_split), bytes=len(text), pieces=pieces)
    print(f"encode_drop_bench: tiles ({time.perf_counter() - t0:.1f} s)", file=sys.stderr, flush=True)
    short = sample.split(b" ")[:args.short]
    rng = random.Random(11)
    res["long"] = {}
    for kind in ("letters", "repeat", "english"):
        docs = batch(short, long_pieces(kind, M, args.count, sample, rng))
        off = np.cumsum([0] + [len(d) for d in docs]).astype(np.uint64)
        e.load(b"".join(docs))
        res["long"][kind] = dict(pair(lambda m, **kw: e.encode_docs(off, m, **kw)), bytes=int(off[-1]), long_pieces=args.count)
        print(f"encode_drop_bench: long {kind} ({time.perf_counter() - t0:.1f} s)", file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    e.close()


if __name__ == "__main__":
    main()

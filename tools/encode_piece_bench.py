#!/usr/bin/env python3
"""The piece-local replay (encode_piece.hip) against the window encoder and the per-document fallback
(DESIGN section 7.12).

--size bytes of english_like (a --sample byte sample repeated), resident and split by "cl100k"; the merge list
is the first --merges merges train_split learns on the sample under the same rule.  One checked warm pass of
every leg, then --repeats alternated repeats in one process, reported as median [min .. max] in ms.  Every
timed call ends with the engine's own stream synchronise (it reads the id count back).

  plan_window / plan_piece  Engine.encode_split(encoder="window" / "piece") with the trained list: what the piece
                            path costs where a plan exists
  noplan_piece              the piece path with the same list padded beyond 65,279 merges by records that never
                            match (byte 1 before the id of the record before)
  noplan_auto               the same under encoder="auto", which puts the long-piece kernel's launch behind the tiles
  noplan_parent             encoder="window" with the padded list, i.e. the per-document fallback, on the first
                            --fallback-pieces pieces only, scaled per piece (--fallback-repeats runs, none warm:
                            each takes many seconds)
  copy                      a device-to-device copy of the same bytes (Tensor.copy_ and a synchronise)

One JSON line.  Needs a GPU; there is no CPU path.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from llmtokenizer_amd import api  # noqa: E402
from llmtokenizer_amd.synth import english_like  # noqa: E402


def med(xs):
    xs = sorted(xs)
    return {"median": round(xs[len(xs) // 2], 3), "min": round(xs[0], 3), "max": round(xs[-1], 3), "n": len(xs)}


def say(what, t0):
    print(f"encode_piece_bench: {what} ({time.perf_counter() - t0:.1f} s)", file=sys.stderr, flush=True)


def main():
    t0 = time.perf_counter()
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1 << 26)
    ap.add_argument("--sample", type=int, default=1 << 24)
    ap.add_argument("--merges", type=int, default=8192)
    ap.add_argument("--pad-to", type=int, default=70000)
    ap.add_argument("--fallback-pieces", type=int, default=10000)
    ap.add_argument("--fallback-repeats", type=int, default=3, help="the first of them is the leg's warm pass too")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    # torch first: its wheel brings a HIP runtime of its own, and the runtime loaded first is the one that owns the GPU
    import torch
    if not torch.cuda.is_available() or api.device_count() < 1:
        sys.exit("encode_piece_bench: no GPU")
    dev = torch.device("cuda", args.device)
    sample = english_like(args.sample)
    text = (sample * (args.size // len(sample) + 1))[:args.size]
    merges = api.train_split(sample, rule="cl100k", max_merges=args.merges, device=args.device)
    say(f"{len(merges)} merges trained", t0)
    k = args.pad_to - len(merges)
    pad = np.stack([np.ones(k, np.uint32), 255 + len(merges) + np.arange(k, dtype=np.uint32)], axis=1)
    pad[0] = (1, 2)
    padded = np.vstack([merges, pad])
    e = api.Engine(args.device)
    e.load(text)
    pieces = e.split("cl100k")
    off = e.split_offsets()
    longest = int(np.diff(off.astype(np.int64)).max())

    def leg(m, encoder):
        t0 = time.perf_counter()
        e.encode_split(m, encoder=encoder)
        return (time.perf_counter() - t0) * 1e3

    legs = {"plan_window": (merges, "window"), "plan_piece": (merges, "piece"), "noplan_piece": (padded, "piece"),
            "noplan_auto": (padded, "auto")}
    sums, info = {}, {}
    for name, (m, enc) in legs.items():  # warm, and checked against each other
        leg(m, enc)
        sums[name], info[name] = e.ids_checksum(), dict(e.docs_info(), enc_path=e.stats()["enc_path"])
        say(f"{name} warm", t0)
    if len(set(sums.values())) != 1:
        sys.exit(f"encode_piece_bench: the legs disagree: {sums}")
    # the parent's behaviour beyond the limits, on a prefix
    fp = min(args.fallback_pieces, pieces)
    f = api.Engine(args.device)
    f.load(text[:int(off[fp])])
    f.split("cl100k")
    src = torch.frombuffer(bytearray(text), dtype=torch.uint8).to(dev)
    dst = torch.empty_like(src)

    def fallback():
        t0 = time.perf_counter()
        f.encode_split(padded, encoder="window")
        return (time.perf_counter() - t0) * 1e3

    def copy():
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        dst.copy_(src)
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3

    copy()
    times = {name: [] for name in list(legs) + ["noplan_parent", "copy"]}
    for r in range(max(5, args.repeats)):
        for name, (m, enc) in legs.items():
            times[name].append(leg(m, enc))
        if r < args.fallback_repeats:  # (many seconds each: a helper context's whole encode per piece)
            times["noplan_parent"].append(fallback())
            say(f"noplan_parent {r}", t0)
        times["copy"].append(copy())
    info["noplan_parent"] = dict(f.docs_info(), enc_path=f.stats()["enc_path"])
    res = {"bench": "encode_piece", "bytes": len(text), "pieces": pieces, "longest_piece": longest,
           "merges": len(merges), "padded_merges": len(padded), "piece_info": api.piece_info(),
           "fallback_pieces": fp, "ms": {n: med(t) for n, t in times.items()}, "info": info}
    res["pieces_per_s"] = {n: round((fp if n == "noplan_parent" else pieces) / (res["ms"][n]["median"] / 1e3))
                           for n in list(legs) + ["noplan_parent"]}
    res["gb_per_s"] = {n: round(len(text) / res["ms"][n]["median"] / 1e6, 2) for n in list(legs) + ["copy"]}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    e.close()
    f.close()


if __name__ == "__main__":
    main()

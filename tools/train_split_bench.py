#!/usr/bin/env python3
"""Training on pieces timed on resident corpora.

Two corpora in HBM, as tools/split_bench.py holds them: the seed-3 synthetic
corpus (Engine.synth; printable bytes, no newline) and english_like (a 32 MiB
sample generated on the host and repeated to the size).  Per corpus and rule
("words", "lines"), alternated in one process, host clock around each call
(every call ends with a stream synchronise):

  split     Engine.split(rule)
  stage_a   Engine.train_split(0): the piece table, the gather of the entries'
            bytes and the one count that finds no merge is wanted; beside it a
            device-to-device hipMemcpyAsync of the corpus' bytes, the streaming
            yardstick of the box
  train     Engine.train_split(k) for every k of --merges; stage B is that
            minus stage_a, per merge that over the merges made
  stream    Engine.train(--stream-merges, fast=True) over the same resident
            bytes: the stream trainer, which ignores the pieces (it drops the
            split, so every repeat splits again)

and the counters of train_split_info (pieces, entries, entry bytes).  A leg
that would start after --budget-s seconds of the run is skipped and listed under
"skipped".  Writes one JSON object to --out and prints it.  Needs a GPU.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from llmtokenizer_amd import api  # noqa: E402
from llmtokenizer_amd.synth import english_like  # noqa: E402
from split_bench import DeviceCopy, med  # noqa: E402


def timed(f, *a):
    t0 = time.perf_counter()
    r = f(*a)
    return time.perf_counter() - t0, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1 << 30)
    ap.add_argument("--merges", default="1024,8192")
    ap.add_argument("--rules", default="words,lines")
    ap.add_argument("--corpora", default="english_like,seed3")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--stream-merges", type=int, default=1024)
    ap.add_argument("--sample", type=int, default=1 << 25, help="bytes of english_like generated, then repeated")
    ap.add_argument("--budget-s", type=float, default=1e9)
    ap.add_argument("--slow-merges", type=int, default=0,
                    help="legs whose entries hold more than 2^28 bytes train at most this many merges (0: no limit)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "profiles", "train_split_bench.json"))
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    if api.device_count() < 1:
        sys.exit("train_split_bench: no GPU")
    t_start = time.perf_counter()
    n, reps = args.size, args.repeats
    ks = [int(k) for k in args.merges.split(",")]
    out = {"tool": "train_split_bench", "bytes": n, "repeats": reps, "legs": {}, "skipped": []}
    cp = DeviceCopy(n)
    e = api.Engine(args.device)
    for corpus in args.corpora.split(","):
        if corpus == "seed3":
            e.synth(3, n)
        else:
            sample = np.frombuffer(english_like(min(args.sample, n)), np.uint8)
            e.load(np.tile(sample, (n + sample.size - 1) // sample.size)[:n].tobytes())
        for rule in args.rules.split(","):
            key = f"{corpus}/{rule}"
            if time.perf_counter() - t_start > args.budget_s:
                out["skipped"].append(key)
                continue
            e.split(rule)  # warm: the first calls allocate
            e.train_split(0)
            info0 = e.train_split_info()
            cp.run()
            legs = [k for k in ks if not (args.slow_merges and info0["entry_bytes"] > 1 << 28 and k > args.slow_merges)]
            t = {"split": [], "stage_a": [], "copy": [], "stream": [], **{f"train_{k}": [] for k in legs}}
            made, stops, stream_made = {}, {}, 0
            for _ in range(reps):  # alternated: other work shares the box
                t["split"].append(timed(e.split, rule)[0])
                t["stage_a"].append(timed(e.train_split, 0)[0])
                t["copy"].append(cp.run())
                for k in legs:
                    dt, made[k] = timed(e.train_split, k)
                    t[f"train_{k}"].append(dt)
                    stops[k] = e.train_split_info()["stop_reason"]
                dt, stream_made = timed(e.train, args.stream_merges, True)
                t["stream"].append(dt)
            a = med(t["stage_a"])
            leg = {"info": {k: info0[k] for k in ("pieces", "entries", "entry_bytes", "long_pieces", "table_slots")},
                   "entries_per_piece": round(info0["entries"] / max(info0["pieces"], 1), 6),
                   "entry_bytes_per_byte": round(info0["entry_bytes"] / n, 6),
                   "split": med(t["split"]), "stage_a": a, "copy": med(t["copy"]),
                   "stage_a_algorithmic_bytes": int(n + 8 * info0["pieces"]),
                   "stream": {**med(t["stream"]), "merges": int(stream_made)}, "train": {}}
            leg["stage_a_over_copy"] = round(a["ms_median"] / leg["copy"]["ms_median"], 2)
            for k in legs:
                m = med(t[f"train_{k}"])
                b = m["ms_median"] - a["ms_median"]
                leg["train"][str(k)] = {**m, "merges": int(made[k]), "stop_reason": int(stops[k]),
                                        "stage_b_ms": round(b, 3), "stage_b_ms_per_merge": round(b / max(made[k], 1), 4)}
            for k in ks:
                if k not in legs:
                    out["skipped"].append(f"{key}/{k}")
            out["legs"][key] = leg
            print(json.dumps({"progress": key, **leg}), file=sys.stderr, flush=True)
    e.close()
    cp.close()
    out["seconds"] = round(time.perf_counter() - t_start, 1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Document-batch encode against its ceiling and its floor.

A seeded 1 GiB corpus resident in HBM (Engine.synth, seed 3) and the merge
list bench.py's encode leg uses (the first --merges merges the GPU trainer
learns on the 1 GiB seed-2 corpus).  For three batch shapes over the same
bytes -- every document 64 B, seeded lengths with a mean of about 512 B, every
document 4 KiB -- it times, alternated in this one process:

  docs    Engine.encode_docs(offsets, merges)   the document path
  single  Engine.encode(merges)                 the unchanged single-stream path:
                                                the same window design without
                                                boundary work, the ceiling

(each is warmed first; both calls end in a stream synchronise inside the
library, when the id total is fetched, so the host clock around a call is the
whole encode), and a loop of api.encode(doc) over the first --loop-docs
documents, the floor users have without the batch call, extrapolated per
document.  One JSON line: GB/s (median) and the spread (min, max) of each,
docs_info(), and docs / single per shape.  Needs a GPU; there is no CPU path.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from llmtokenizer_amd import api  # noqa: E402
from llmtokenizer_amd.synth import synth_bytes  # noqa: E402


def shape_offsets(name, n, seed):
    if name == "fixed64":
        step = 64
    elif name == "fixed4k":
        step = 4096
    else:  # seeded lengths 1..1023, mean 512
        rng = np.random.default_rng(seed)
        lens = rng.integers(1, 1024, size=n // 400, dtype=np.uint64)
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        off = off[off < n]
        return np.concatenate([off, [n]]).astype(np.uint64)
    off = np.arange(0, n, step, dtype=np.uint64)
    return np.concatenate([off, [n]]).astype(np.uint64)


def rate(n, secs):
    g = sorted(n / 1e9 / s for s in secs)
    return {"gbps_median": round(g[len(g) // 2], 2), "gbps_min": round(g[0], 2), "gbps_max": round(g[-1], 2),
            "repeats": len(g)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1 << 30)
    ap.add_argument("--merges", type=int, default=32768)
    ap.add_argument("--train-size", type=int, default=1 << 30)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--loop-docs", type=int, default=2000)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    if api.device_count() < 1:
        sys.exit("docs_bench: no GPU")
    reps = max(5, args.repeats)
    n = args.size
    tr = api.Engine(args.device)
    tr.synth(2, args.train_size)
    tr.train(args.merges)
    merges = tr.merges()
    tr.close()
    e = api.Engine(args.device)
    e.synth(3, n)
    out = {"tool": "docs_bench", "bytes": n, "merges": int(len(merges)), "shapes": {}}
    for name in ("fixed64", "mean512", "fixed4k"):
        off = shape_offsets(name, n, 17)
        e.encode_docs(off, merges)  # warm (pools, the plan's upload path)
        info = e.docs_info()
        n_out = e.stats()["n_out"]
        e.encode(merges)
        t_docs, t_single = [], []
        for _ in range(reps):  # alternated: other work shares the host
            t0 = time.perf_counter()
            e.encode_docs(off, merges)
            t1 = time.perf_counter()
            e.encode(merges)
            t2 = time.perf_counter()
            t_docs.append(t1 - t0)
            t_single.append(t2 - t1)
        single_path = e.stats()["enc_path"]
        # the floor: one api.encode per document (its own load, plan upload, launch, scan, fetch)
        k = min(args.loop_docs, off.size - 1)
        head = synth_bytes(3, int(off[k]))
        docs = [head[int(off[d]):int(off[d + 1])] for d in range(k)]
        api.encode(docs[0], merges)  # warm
        t0 = time.perf_counter()
        for d in docs:
            api.encode(d, merges)
        loop_s = time.perf_counter() - t0
        rd, rs = rate(n, t_docs), rate(n, t_single)
        out["shapes"][name] = {
            "ndocs": int(off.size - 1), "docs": rd, "single": rs, "single_enc_path": int(single_path),
            "docs_over_single": round(rd["gbps_median"] / rs["gbps_median"], 3),
            "single_spread": round((rs["gbps_max"] - rs["gbps_min"]) / rs["gbps_median"], 3),
            "docs_info": info, "n_out_docs": int(n_out),
            "loop": {"docs": k, "bytes": int(off[k]), "ms_per_doc": round(loop_s / k * 1e3, 3),
                     "mb_per_s": round(int(off[k]) / 1e6 / loop_s, 4),
                     "extrapolated_s_for_batch": round(loop_s / k * (off.size - 1), 1)},
        }
    e.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What rewriting resident ids to a vocabulary's ids costs.

1 GiB of english_like bytes (a 32 MiB sample repeated) resident in HBM, split by "cl100k" and encoded
with the merge list of tools/split_bench.py (the first --merges merges the trainer learns on the 1 GiB
seed-2 corpus), numbered by a shuffled vocabulary with holes.

  map      Engine.map_ids(vocab) after a fresh Engine.encode_split, alternated in one loop with a
           device-to-device hipMemcpyAsync of the same id buffer's size (4 bytes per id) timed the same
           way (host clock around the call and a stream synchronise): the map reads and writes every id
           once, as the copy does, plus table reads that should stay in L2, so the copy is its yardstick.
           Engine.map_ids also checks the vocabulary and uploads the forward table on the host's clock;
           map_fixed is the same call over a 4 KiB text, where that is all there is, reported beside it
           and taken off in map_less_fixed.
  e2e      vocab.Tokenizer.encode(data) (load, split, encode_split, map_ids, fetch the ids) against the
           same steps without map_ids, alternated.

Medians and ranges of --repeats alternated repeats.  One JSON line; --out writes it to a file as well.
Needs a GPU; there is no CPU path.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from llmtokenizer_amd import api  # noqa: E402
from llmtokenizer_amd.synth import english_like  # noqa: E402
from llmtokenizer_amd.vocab import Tokenizer, Vocab, vocab_tables  # noqa: E402
from split_bench import DeviceCopy, med  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1 << 30)
    ap.add_argument("--merges", type=int, default=32768)
    ap.add_argument("--train-size", type=int, default=1 << 30)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--sample", type=int, default=1 << 25, help="bytes of english_like generated, then repeated")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if api.device_count() < 1:
        sys.exit("vocab_bench: no GPU")
    reps, n = max(5, args.repeats), args.size
    tr = api.Engine(args.device)
    tr.synth(2, args.train_size)
    tr.train(args.merges)
    merges = tr.merges()
    tr.close()
    k = int(len(merges))
    ids = np.random.default_rng(1).permutation(256 + k + k // 8)[: 256 + k]
    vocab = Vocab(merges, ids[:256], ids[256:], [], [], "cl100k")
    fwd, _ = vocab_tables(vocab)
    sample = np.frombuffer(english_like(min(args.sample, n)), np.uint8)
    data = np.tile(sample, (n + sample.size - 1) // sample.size)[:n].tobytes()
    small = data[:4096]
    out = {"tool": "vocab_bench", "bytes": n, "merges": k, "table_bytes": int(fwd.size * 4)}

    e = api.Engine(args.device)
    e.load(data)
    e.split("cl100k")
    e.encode_split(merges)
    n_ids = int(e.stats()["n_out"])
    cp = DeviceCopy(4 * n_ids)
    es = api.Engine(args.device)
    es.load(small)
    es.split("cl100k")
    # one checked pass: the mapped ids' checksum against the host's over the fetched internal ids
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import golden_lib as G  # the numpy form of the checksum
    internal = e.ids()
    e.map_ids(vocab)
    want = G.ids_checksum(fwd[internal])
    if e.ids_checksum() != want:
        sys.exit("vocab_bench: the mapped ids' checksum differs from the host's")
    del internal
    cp.run()
    t_map, t_copy, t_fixed = [], [], []
    for _ in range(reps):  # alternated: other work shares the box
        e.encode_split(merges)
        t0 = time.perf_counter()
        e.map_ids(vocab)
        t_map.append(time.perf_counter() - t0)
        t_copy.append(cp.run())
        es.encode_split(merges)
        t0 = time.perf_counter()
        es.map_ids(vocab)
        t_fixed.append(time.perf_counter() - t0)
    mm, mc, mf = med(t_map), med(t_copy), med(t_fixed)
    less = max(mm["ms_median"] - mf["ms_median"], 1e-6)
    moved = 8 * n_ids
    out["map"] = {"ids": int(n_ids), "bytes_per_id": round(n / n_ids, 3), "map": mm, "copy": mc, "map_fixed": mf,
                  "map_less_fixed_ms": round(less, 3), "bytes_moved": int(moved),
                  "gbps": round(moved / (mm["ms_median"] * 1e-3) / 1e9, 1),
                  "gbps_less_fixed": round(moved / (less * 1e-3) / 1e9, 1),
                  "copy_gbps": round(moved / (mc["ms_median"] * 1e-3) / 1e9, 1),
                  "map_over_copy_time": round(mm["ms_median"] / mc["ms_median"], 3),
                  "map_less_fixed_over_copy_time": round(less / mc["ms_median"], 3)}
    cp.close()
    es.close()
    e.close()

    tok = Tokenizer(vocab, args.device)
    plain = api.Engine(args.device)

    def without_map():
        plain.load(data)
        plain.split("cl100k")
        plain.encode_split(merges)
        return plain.ids()

    tok.encode(data)  # warm both
    without_map()
    t_with, t_without = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        tok.encode(data)
        t1 = time.perf_counter()
        without_map()
        t2 = time.perf_counter()
        t_with.append(t1 - t0)
        t_without.append(t2 - t1)
    w, wo = med(t_with), med(t_without)
    out["e2e"] = {"with_map": w, "without_map": wo, "with_over_without": round(w["ms_median"] / wo["ms_median"], 4),
                  "with_gbps": round(n / w["ms_median"] / 1e6, 2), "without_gbps": round(n / wo["ms_median"] / 1e6, 2)}
    tok.close()
    plain.close()
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()

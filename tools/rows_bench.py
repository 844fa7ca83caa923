#!/usr/bin/env python3
"""Rows back to texts against a copy and against the route through the host.

The workload: a [B, L] tensor on the device as generate leaves it (default 4,096 x 2,048), int32 and int64: a left
padding of 0 .. 63 cells, ids of the vocabulary of tests/golden/vocab/vocab_cl100k.json with one special in a
hundred, an EOS at a uniformly random column, the pad (== EOS) behind it.  Per cell type, kernel variant (four cells per
lane: the contiguous tensor; one: the same cells in a view whose first cell is not 16-byte aligned) and skip list (off,
the vocabulary's specials) one leg:

  unpack_*         Engine.unpack_rows' device part (bpe_gpu_unpack_rows: upload of the skip list, k_rows_bounds, the
                   scan, the read-back of the count and the error words, k_rows_gather), host clock around the call
  copy_*           a device-to-device copy (torch's Tensor.copy_ and a synchronise) of as many bytes as k_rows_bounds
                   must read (every row up to its end) and of as many as k_rows_gather must read (the kept cells)
  short_*          the same cells as 64 times the rows of L / 64 cells: a wave per row with most lanes idle
  decode_rows      Tokenizer.decode_rows(t, pad_id, eos, skip_specials=True), end to end
  host_route       the only route without it: t.cpu(), a numpy search for the ends, Tokenizer.decode_batch

--repeats alternated repeats of every leg in one process, reported as median [min .. max]; the first pass warms every
leg and is checked, not timed (unpack against api.unpack_rows_host, the two decode routes against each other).  With
--trace nothing is timed: every unpack configuration runs --trace times in a fixed order, then every copy, the order printed as
JSON, for a kernel and memory-copy trace taken around the process (the kernels' and the copies' own times).  One JSON line.  Needs a GPU; there is no CPU path.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from llmtokenizer_amd import api  # noqa: E402
from llmtokenizer_amd.vocab import Tokenizer, Vocab  # noqa: E402
from split_bench import med  # noqa: E402


def make_rows(rng, B, L, plain, specials, eos):
    rows = rng.choice(plain, (B, L))
    rows[rng.random((B, L)) < 0.01] = specials[-1]
    col = np.arange(L)[None, :]
    lead = rng.integers(0, min(64, L), B)[:, None]
    end = np.maximum(rng.integers(0, L, B)[:, None], lead)
    rows[col < lead] = eos
    rows[col >= end] = eos
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--L", type=int, default=2048)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--trace", type=int, default=0)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    # torch first: its wheel brings a HIP runtime of its own, and the runtime loaded first is the one that owns the GPU
    import torch
    if not torch.cuda.is_available() or api.device_count() < 1:
        sys.exit("rows_bench: no GPU")
    dev = torch.device("cuda", args.device)
    torch.zeros(1, device=dev)
    with open(os.path.join(ROOT, "tests", "golden", "vocab", "vocab_cl100k.json"), encoding="utf-8") as f:
        fx = json.load(f)
    path = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"rows_bench_{os.getpid()}.json")
    with open(path, "w", encoding="utf-8") as f:
        json.dump(fx["tokenizer_json"], f, ensure_ascii=False)
    vocab = Vocab.from_tokenizer_json(path)
    os.unlink(path)
    tok = Tokenizer(vocab, args.device)
    e = tok._eng()
    specials = [int(x) for x in vocab.special_ids]
    eos = specials[0]
    # (no NUL byte: the decoders drop it, and the bytes are compared)
    plain = np.array([int(x) for x in list(vocab.byte_ids[1:]) + list(vocab.merge_ids)], dtype=np.int64)
    rng = np.random.default_rng(9)
    B, L, reps = args.B, args.L, max(5, args.repeats)
    host = make_rows(rng, B, L, plain, specials, eos)
    short = host.reshape(B * 64, L // 64)
    want = api.unpack_rows_host(host, None, eos, [eos], specials)
    z = want[2][:, 1].astype(np.int64)
    out = {"tool": "rows_bench", "B": B, "L": L, "vocab_ids": int(plain.size), "repeats": reps, "ids_kept": int(want[0].size),
           "cells_to_the_ends": int((np.minimum(z + 1, L)).sum())}
    configs = []  # (name, tensor, skip)
    for dt in (torch.int32, torch.int64):
        name = str(dt).split(".")[1]
        t = torch.from_numpy(host).to(dev).to(dt)
        wide = torch.zeros((B, L + 4), dtype=dt, device=dev)
        wide[:, 1:L + 1] = t
        view = wide[:, 1:L + 1]
        assert t.data_ptr() % 16 == 0 and view.data_ptr() % 16 != 0
        ts = torch.from_numpy(short).to(dev).to(dt)
        for skip in (None, specials):
            sk = "skip" if skip else "noskip"
            configs += [(f"unpack_{name}_vec_{sk}", t, skip), (f"unpack_{name}_one_{sk}", view, skip)]
        configs.append((f"short_{name}_vec_skip", ts, specials))
    copies = []  # (name, source, destination): as many bytes as k_rows_bounds / k_rows_gather must read
    for name, cb in (("int32", 4), ("int64", 8)):
        for what, cells in (("bounds", out["cells_to_the_ends"]), ("gather", out["ids_kept"])):
            n = cells * cb
            copies.append((f"copy_{name}_{what}", torch.ones(n, dtype=torch.uint8, device=dev),
                           torch.empty(n, dtype=torch.uint8, device=dev)))
            out[f"copy_{name}_{what}_bytes"] = n
    if args.trace:
        for name, t, skip in configs:
            for _ in range(args.trace):
                e._unpack_rows(t, None, eos, [eos], skip)
        for name, s, d in copies:
            for _ in range(args.trace):
                d.copy_(s)
                torch.cuda.synchronize(dev)
        print(json.dumps({"tool": "rows_bench", "trace": args.trace, "order": [c[0] for c in configs],
                          "copies": [[c[0], c[1].numel()] for c in copies]}))
        return
    t64 = [c[1] for c in configs if c[0] == "unpack_int64_vec_skip"][0]
    times = {}

    def leg(key, run):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        r = run()
        torch.cuda.synchronize(dev)
        times.setdefault(key, []).append(time.perf_counter() - t0)
        return r

    def host_route():
        a = t64.cpu().numpy()
        notpad = a != eos
        lead = np.where(notpad.any(1), notpad.argmax(1), L)
        col = np.arange(L)[None, :]
        stop = (a == eos) & (col >= lead[:, None])
        end = np.where(stop.any(1), stop.argmax(1), L)
        keep = (col >= lead[:, None]) & (col < end[:, None]) & ~np.isin(a, specials)
        ids = a[keep].astype(np.uint32)
        off = np.concatenate([[0], np.cumsum(keep.sum(1))]).astype(np.uint64)
        return tok.decode_batch(ids, off)

    legs = [(name, (lambda t=t, skip=skip: e._unpack_rows(t, None, eos, [eos], skip))) for name, t, skip in configs]
    legs += [(name, (lambda s=s, d=d: d.copy_(s))) for name, s, d in copies]
    legs += [("decode_rows", lambda: tok.decode_rows(t64, pad_id=eos, eos=eos, skip_specials=True)), ("host_route", host_route)]
    for rep in range(reps + 1):
        res = {key: leg(key, run) for key, run in (legs if rep % 2 == 0 else legs[::-1])}  # (the order swapped every repeat)
        if rep == 0:  # warmed and checked, not timed
            times.clear()
            ok = res["decode_rows"] == res["host_route"]
            for name, t, skip in configs:
                if name.startswith("unpack"):
                    got = e.unpack_rows(t, None, eos, [eos], skip)
                    ref = want if skip else api.unpack_rows_host(host, None, eos, [eos], None)
                    ok = ok and all(np.array_equal(g, w) for g, w in zip(got, ref))
            out["equal_host"] = bool(ok)
            out["decoded_bytes"] = sum(len(x) for x in res["decode_rows"])
            if not ok:
                sys.exit(f"rows_bench: the device's results are not the host's: {json.dumps(out)}")
    out.update({key: med(v) for key, v in times.items()})
    out["host_route_over_decode_rows_time"] = round(out["host_route"]["ms_median"] / out["decode_rows"]["ms_median"], 3)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

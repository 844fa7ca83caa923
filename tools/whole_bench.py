#!/usr/bin/env python3
"""Whole-text rows against the packed stream and a copy.

Two resident batches, ids = bytes (one merge that no text holds, rule "words"), BOS and EOS around every text:

  lines   --size bytes of english_like cut at its newlines (173 bytes a line on average), seq_len 2,048
  tiny    --tiny texts of 0 .. 7 bytes, seq_len 8: a row opener every text or two, the doubling's worst case

Per batch, --repeats alternated repeats of every leg in one process (the order swapped every repeat), host clock
around the call and a synchronise, reported as median [min .. max]:

  whole   Engine.pack_whole into torch tensors (rows, seg, pos) after another description's query, so that the
          placement runs again: query + fill, what a caller pays
  place   the query alone, the placement run again
  fill    Engine.pack_whole with the placement kept from the query before it
  stream  Engine.pack_stream (rows, seg, pos) of the same batch
  copy    a device-to-device copy of the bytes `whole` writes

The first pass warms every leg and is checked, not timed: rows, seg, pos and the placement of the texts that fill the
first --check-rows rows against api.pack_whole_host.  One JSON line.  Needs a GPU; there is no CPU path.
"""
import argparse
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

MERGES = np.array([[0xF0, 0xF1]], dtype=np.uint32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1 << 28)
    ap.add_argument("--sample", type=int, default=1 << 25, help="bytes of english_like generated, then repeated")
    ap.add_argument("--tiny", type=int, default=1 << 24, help="texts of the tiny batch")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--check-rows", type=int, default=64)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    # torch first: its wheel brings a HIP runtime of its own, and the runtime loaded first is the one that owns the GPU
    import torch
    if not torch.cuda.is_available() or api.device_count() < 1:
        sys.exit("whole_bench: no GPU")
    dev = torch.device("cuda", args.device)
    torch.zeros(1, device=dev)
    reps, pad, bos, eos = max(5, args.repeats), 0xFFFFFFFF, 257, 258
    sample = np.frombuffer(english_like(min(args.sample, args.size)), np.uint8)
    lines = np.tile(sample, (args.size + sample.size - 1) // sample.size)[:args.size]
    cuts = np.flatnonzero(lines == 10) + 1
    line_off = np.concatenate([[0], cuts[cuts < lines.size], [lines.size]]).astype(np.uint64)
    tiny_off = np.concatenate([[0], np.cumsum(np.random.default_rng(1).integers(0, 8, args.tiny))]).astype(np.uint64)
    tiny = np.tile(sample, (int(tiny_off[-1]) + sample.size - 1) // sample.size)[:int(tiny_off[-1])]
    out = {"tool": "whole_bench", "bos_eos": True, "repeats": reps, "batches": {}}
    e = api.Engine(args.device)
    for name, raw, off, L in (("lines", lines, line_off, 2048), ("tiny", tiny, tiny_off, 8)):
        T = off.size - 1
        e.load_texts(raw.tobytes(), offsets=off)
        e.split("words")
        e.encode_split(MERGES)
        R, N, n_long = e.whole_rows(L, bos, eos)
        Rs = e.stream_rows(L, bos, eos)[0]
        rows, seg, pos = (torch.empty((R, L), dtype=torch.int32, device=dev) for _ in range(3))
        srow, sseg, spos = (torch.empty((Rs, L), dtype=torch.int32, device=dev) for _ in range(3))
        src, dst = torch.ones((3, R, L), dtype=torch.int32, device=dev), torch.empty((3, R, L), dtype=torch.int32, device=dev)
        other = lambda: e.whole_rows(L, bos)  # noqa: E731  (another description: the kept placement goes)
        same = lambda: e.whole_rows(L, bos, eos)  # noqa: E731
        whole = lambda: e.pack_whole(L, pad, bos, eos, out=(rows, seg, pos))  # noqa: E731
        legs = [("whole", other, whole), ("place", other, same), ("fill", same, whole),
                ("stream", None, lambda: e.pack_stream(L, pad, bos, eos, out=(srow, sseg, spos))),
                ("copy", None, lambda: dst.copy_(src))]
        t = {key: [] for key, _, _ in legs}
        for rep in range(reps + 1):
            for key, prep, run in (legs if rep % 2 == 0 else legs[::-1]):
                if prep:
                    prep()
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                run()
                torch.cuda.synchronize(dev)
                t[key].append(time.perf_counter() - t0)
            if rep == 0:  # warmed and checked, not timed
                for v in t.values():
                    v.clear()
                ids, toff = e.ids(), e.text_offsets()
                k = min(args.check_rows, R)
                trow, tcol = (x.cpu().numpy().view(np.uint32) for x in e.pack_whole(L, pad, bos, eos, placement=True, out=(rows, seg, pos))[3:])
                head_T = int(np.searchsorted(trow, k, side="left"))  # the texts that begin in the first k rows
                want = api.pack_whole_host(ids[:int(toff[head_T])], toff[:head_T + 1], L, pad, bos, eos)
                k = min(k, want["rows"].shape[0] - 1)  # (the head's last row may go on in the batch)
                ok = all(np.array_equal(x[:k].cpu().numpy().view(np.uint32), want[key][:k]) for x, key in zip((rows, seg, pos), ("rows", "seg", "pos")))
                ok = ok and np.array_equal(trow[:head_T], want["text_row"]) and np.array_equal(tcol[:head_T], want["text_col"])
                if not ok:
                    sys.exit(f"whole_bench: {name}: the device rows are not the host's")
                del ids, toff, want
        res = {"texts": T, "ids": int(off[-1]), "seq_len": L, "rows": R, "cells": N, "n_long": n_long, "stream_rows": Rs,
               "fill_ratio": round(N / max(R * L, 1), 4), "doubling_rounds": int(T).bit_length(), "first_rows_equal_host": True}
        res.update({key: med(v) for key, v in t.items()})
        res["whole_over_stream_time"] = round(res["whole"]["ms_median"] / res["stream"]["ms_median"], 3)
        res["whole_over_copy_time"] = round(res["whole"]["ms_median"] / res["copy"]["ms_median"], 3)
        res["place_share_of_whole"] = round(res["place"]["ms_median"] / res["whole"]["ms_median"], 3)
        out["batches"][name] = res
        print(json.dumps({"progress": name, **res}), file=sys.stderr, flush=True)
        del rows, seg, pos, srow, sseg, spos, src, dst, legs
        torch.cuda.empty_cache()
    e.close()
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Packed training rows against a copy and against the padded rows.

The workload of tools/texts_bench.py: 1 GiB of english_like (a 32 MiB sample repeated) cut into texts of --cuts bytes
each (512 and 2,048), the rule "cl100k" around <|endoftext|> and <|im_start|>, the first --merges merges the trainer
learns on the 1 GiB seed-2 corpus, numbered the engine's own way.  Per cut the batch is loaded, split, encoded and
mapped once; then --repeats alternated repeats of every leg in one process, reported as median [min .. max]:

  stream_rows      Engine.pack_stream(seq_len, BOS and EOS) into a torch tensor on the device, rows alone
  stream_all       ... rows, seg and pos
  copy_rows        a device-to-device copy of the bytes stream_rows writes (torch's Tensor.copy_, which is
  copy_all         hipMemcpyAsync, and a synchronise), and of the bytes stream_all writes
  pack_texts       Engine.pack_texts(row_len = seq_len) on the same resident batch: the padded rows, one text per row

The first pass warms every leg and is checked, not timed: the rows, seg and pos of the first --check-rows rows are
compared with api.pack_stream_host over the fetched ids, the stream's last cell must be the EOS and every cell behind
it the pad.  One JSON line.  Needs a GPU; there is no CPU path.
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
from llmtokenizer_amd.vocab import Vocab  # noqa: E402
from split_bench import med  # noqa: E402

SPECIALS = [b"<|endoftext|>", b"<|im_start|>"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1 << 30)
    ap.add_argument("--merges", type=int, default=32768)
    ap.add_argument("--train-size", type=int, default=1 << 30)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--sample", type=int, default=1 << 25, help="bytes of english_like generated, then repeated")
    ap.add_argument("--cuts", default="512,2048", help="bytes per text, comma separated")
    ap.add_argument("--seq-len", type=int, default=2048)
    ap.add_argument("--check-rows", type=int, default=64)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    # torch first: its wheel brings a HIP runtime of its own, and the runtime loaded first is the one that owns the GPU
    import torch
    if not torch.cuda.is_available() or api.device_count() < 1:
        sys.exit("stream_bench: no GPU")
    dev = torch.device("cuda", args.device)
    torch.zeros(1, device=dev)
    reps, n, L, pad = max(5, args.repeats), args.size, args.seq_len, 0xFFFFFFFF
    tr = api.Engine(args.device)
    tr.synth(2, args.train_size)
    tr.train(args.merges)
    vocab = Vocab.from_merges(tr.merges(), "cl100k", SPECIALS)
    tr.close()
    bos, eos = int(vocab.special_ids[1]), int(vocab.special_ids[0])
    sample = np.frombuffer(english_like(min(args.sample, n)), np.uint8)
    raw = np.tile(sample, (n + sample.size - 1) // sample.size)[:n].tobytes()
    out = {"tool": "stream_bench", "bytes": n, "merges": int(vocab.merges.shape[0]), "rule": "cl100k", "seq_len": L,
           "bos_eos": True, "repeats": reps, "cuts": {}}
    e = api.Engine(args.device)
    for cut in (int(c) for c in args.cuts.split(",")):
        off = np.arange(0, n + cut, cut, dtype=np.uint64)
        off[-1] = n
        T = off.size - 1
        e.load_texts(raw, offsets=off)
        e.split("cl100k", SPECIALS)
        e.encode_split(vocab.merges)
        e.map_ids(vocab)
        R, N = e.stream_rows(L, bos, eos)
        rows, seg, pos = (torch.empty((R, L), dtype=torch.int32, device=dev) for _ in range(3))
        src3, dst3 = torch.ones((3, R, L), dtype=torch.int32, device=dev), torch.empty((3, R, L), dtype=torch.int32, device=dev)
        src1, dst1 = src3[0], dst3[0]
        padded = torch.empty((T, L), dtype=torch.int32, device=dev)
        t = {key: [] for key in ("stream_rows", "stream_all", "copy_rows", "copy_all", "pack_texts")}

        def leg(key, run):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            run()
            torch.cuda.synchronize(dev)
            t[key].append(time.perf_counter() - t0)

        legs = [("stream_rows", lambda: e.pack_stream(L, pad, bos, eos, out=(rows, None, None))),
                ("copy_rows", lambda: dst1.copy_(src1)),
                ("stream_all", lambda: e.pack_stream(L, pad, bos, eos, out=(rows, seg, pos))),
                ("copy_all", lambda: dst3.copy_(src3)),
                ("pack_texts", lambda: e.pack_texts(L, pad, "right", out=padded))]
        res = {}
        for rep in range(reps + 1):
            for key, run in (legs if rep % 2 == 0 else legs[::-1]):  # (the order swapped every repeat)
                leg(key, run)
            if rep == 0:  # warmed and checked, not timed
                for v in t.values():
                    v.clear()
                ids, toff = e.ids(), e.text_offsets()
                k = min(args.check_rows, R)
                # the texts that fill the first k rows, as a stream of their own
                head_T = min(T, int(np.searchsorted(toff + 2 * np.arange(T + 1, dtype=np.uint64), k * L, side="right")))
                want = api.pack_stream_host(ids[:int(toff[head_T])], toff[:head_T + 1], L, pad, bos, eos)
                got = [x[:k].cpu().numpy().view(np.uint32) for x in (rows, seg, pos)]
                ok = all(np.array_equal(g, w[:k]) for g, w in zip(got, want[:3]))
                flat = rows.reshape(-1)
                last_eos = int(flat[N - 1].item()) & 0xFFFFFFFF
                tail_pad = bool((flat[N:].cpu().numpy().view(np.uint32) == pad).all())
                kept = int(np.minimum(np.diff(toff.astype(np.int64)), L).sum())
                res = {"texts": T, "ids": int(ids.size), "stream_cells": N, "rows": R, "ids_checksum": e.ids_checksum(),
                       "first_rows_equal_host": ok, "last_cell_is_eos": last_eos == eos, "tail_is_pad": tail_pad,
                       "padded_rows_ids_kept": kept}
                if not (ok and last_eos == eos and tail_pad):
                    sys.exit(f"stream_bench: cut {cut}: the device rows are not the host's: {json.dumps(res)}")
                del ids, toff, want, got
        m = {key: med(v) for key, v in t.items()}
        cells = R * L
        # written cells, the ids read (every id once) and text_off read
        moved_rows, moved_all = cells * 4 + N * 4 + (T + 1) * 8, 3 * cells * 4 + N * 4 + (T + 1) * 8
        moved_texts = T * L * 4 + T * 4 + res["padded_rows_ids_kept"] * 4 + (T + 1) * 8
        res.update(m)
        res.update({
            "stream_rows_bytes_written": cells * 4, "stream_all_bytes_written": 3 * cells * 4, "pack_texts_bytes_written": T * L * 4,
            "stream_rows_gbps": round(moved_rows / m["stream_rows"]["ms_median"] / 1e6, 1),
            "stream_all_gbps": round(moved_all / m["stream_all"]["ms_median"] / 1e6, 1),
            "pack_texts_gbps": round(moved_texts / m["pack_texts"]["ms_median"] / 1e6, 1),
            "copy_rows_gbps": round(2 * cells * 4 / m["copy_rows"]["ms_median"] / 1e6, 1),
            "copy_all_gbps": round(2 * 3 * cells * 4 / m["copy_all"]["ms_median"] / 1e6, 1),
            "stream_rows_over_copy_time": round(m["stream_rows"]["ms_median"] / m["copy_rows"]["ms_median"], 3),
            "stream_all_over_copy_time": round(m["stream_all"]["ms_median"] / m["copy_all"]["ms_median"], 3),
            "pack_texts_over_stream_rows_time": round(m["pack_texts"]["ms_median"] / m["stream_rows"]["ms_median"], 3)})
        out["cuts"][str(cut)] = res
        print(json.dumps({"progress": cut, **res}), file=sys.stderr, flush=True)
        del rows, seg, pos, src1, dst1, src3, dst3, padded, legs
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

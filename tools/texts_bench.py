#!/usr/bin/env python3
"""Text batches against what they replace.

1 GiB of english_like (a 32 MiB sample repeated) cut into texts of --cuts bytes each (512 and 2,048), the rule
"cl100k" around <|endoftext|> and <|im_start|>, the merge list of tools/split_bench.py (the first --merges merges
the trainer learns on the 1 GiB seed-2 corpus), numbered the engine's own way.  Per cut, --repeats alternated
repeats of every leg in one process, reported as median [min .. max]:

  a  batch     Engine.load_texts + split + encode_split + map_ids over the texts
     one_text  the same bytes as one text through load + split + encode_split + map_ids, run by the library of
               the parent commit (--parent-lib, loaded beside this one): what the breaks cost
  b  encode_batch  Tokenizer.encode_batch(texts) end to end, the ids and text_off fetched; per text
     loop          a Python loop of Tokenizer.encode over the first --loop-texts of the same texts (the only
                   exact way before), per text; their ids are compared with the batch's
  c  pack      Engine.pack_texts(row_len 512) into a torch tensor on the device
     copy      a device-to-device copy of texts * row_len * 4 bytes (torch's Tensor.copy_, which is
               hipMemcpyAsync, and a synchronise), timed the same way
     host_pad  Engine.ids() + Engine.text_offsets() and the padding done with numpy on the host

One JSON line.  Needs a GPU; there is no CPU path.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from llmtokenizer_amd import api  # noqa: E402
from llmtokenizer_amd.synth import english_like  # noqa: E402
from llmtokenizer_amd.vocab import Tokenizer, Vocab  # noqa: E402
from split_bench import med  # noqa: E402

SPECIALS = [b"<|endoftext|>", b"<|im_start|>"]
CL100K = 6  # bpe_gpu.h BPE_SPLIT_CL100K


class OtherLibrary:
    """load + split + encode_split + map_ids through another build of the library (the parent commit's), by its C
    calls alone: nothing of this tree's Python is between the clock and that library"""

    def __init__(self, path, device, vocab):
        self.L = L = ctypes.CDLL(path)
        vp, sz = ctypes.c_void_p, ctypes.c_size_t
        L.bpe_gpu_create.argtypes = [ctypes.c_int, ctypes.POINTER(vp)]
        L.bpe_gpu_destroy.argtypes = [vp]
        L.bpe_gpu_destroy.restype = None
        L.bpe_gpu_load.argtypes = [vp, vp, sz]
        L.bpe_gpu_split_special.argtypes = [vp, ctypes.c_int, vp, vp, vp, ctypes.POINTER(sz)]
        L.bpe_gpu_encode_split.argtypes = [vp, vp, sz]
        L.bpe_gpu_map_ids.argtypes = [vp, vp]
        L.bpe_gpu_ids_checksum.argtypes = [vp, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]
        L.bpe_gpu_last_error.restype = ctypes.c_char_p
        self.ctx = vp()
        self.ok(L.bpe_gpu_create(device, ctypes.byref(self.ctx)))
        self.sp = api._Specials(SPECIALS)
        self.cv = vocab.c_vocab()
        self.merges = np.ascontiguousarray(vocab.merges, dtype=np.uint32).reshape(-1)

    def ok(self, rc):
        if rc:
            sys.exit(f"texts_bench: the other library: error {rc} ({self.L.bpe_gpu_last_error().decode()})")

    def run(self, buf):
        L, vp, nd = self.L, ctypes.c_void_p, ctypes.c_size_t(0)
        ts = [time.perf_counter()]
        self.ok(L.bpe_gpu_load(self.ctx, buf.ctypes.data_as(vp), buf.size))
        ts.append(time.perf_counter())
        self.ok(L.bpe_gpu_split_special(self.ctx, CL100K, None, None, self.sp.ref, ctypes.byref(nd)))
        ts.append(time.perf_counter())
        self.ok(L.bpe_gpu_encode_split(self.ctx, self.merges.ctypes.data_as(vp), self.merges.size // 2))
        ts.append(time.perf_counter())
        self.ok(L.bpe_gpu_map_ids(self.ctx, self.cv.ref))
        ts.append(time.perf_counter())
        return nd.value, np.diff(ts).tolist()

    def checksum(self):
        s = ctypes.c_uint64(0)
        self.ok(self.L.bpe_gpu_ids_checksum(self.ctx, 0, ctypes.byref(s)))
        return s.value

    def close(self):
        self.L.bpe_gpu_destroy(self.ctx)


def _mix64(x):
    x = x ^ (x >> np.uint64(33))
    x = x * np.uint64(0xFF51AFD7ED558CCD)
    x = x ^ (x >> np.uint64(33))
    x = x * np.uint64(0xC4CEB9FE1A85EC53)
    return x ^ (x >> np.uint64(33))


def checksum(ids, chunk=1 << 24):
    """bpe_gpu_ids_checksum with numpy"""
    tot = 0
    with np.errstate(over="ignore"):
        for s in range(0, ids.size, chunk):
            part = ids[s:s + chunk].astype(np.uint64)
            pos = np.arange(s, s + part.size, dtype=np.uint64)
            tot = (tot + int(_mix64(_mix64(pos) ^ part).sum(dtype=np.uint64))) & ((1 << 64) - 1)
    return tot


def host_pad(ids, toff, row_len, pad):
    """rows and lens with numpy, right side: what a caller did with the ids on the host"""
    T = toff.size - 1
    lens = np.minimum(np.diff(toff.astype(np.int64)), row_len)
    rows = np.full((T, row_len), pad, dtype=np.uint32)
    for lo in range(0, T, 1 << 16):  # (chunks: the index arrays stay small)
        ln = lens[lo:lo + (1 << 16)]
        col = np.arange(row_len, dtype=np.int64)[None, :]
        keep = col < ln[:, None]
        src = (toff[lo:lo + ln.size].astype(np.int64)[:, None] + col)[keep]
        rows[lo:lo + ln.size][keep] = ids[src]
    return rows, lens.astype(np.uint32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1 << 30)
    ap.add_argument("--merges", type=int, default=32768)
    ap.add_argument("--train-size", type=int, default=1 << 30)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sample", type=int, default=1 << 25, help="bytes of english_like generated, then repeated")
    ap.add_argument("--cuts", default="512,2048", help="bytes per text, comma separated")
    ap.add_argument("--row-len", type=int, default=512)
    ap.add_argument("--loop-texts", type=int, default=10000)
    ap.add_argument("--parent-lib", required=True, help="libbpe_amd.so built from the parent commit")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    # torch first: its wheel brings a HIP runtime of its own, and the runtime loaded first is the one that owns the
    # GPU (the library then binds to it); the other way round torch finds no device
    import torch
    if not torch.cuda.is_available() or api.device_count() < 1:
        sys.exit("texts_bench: no GPU")
    torch.zeros(1, device=torch.device("cuda", args.device))
    reps, n, row_len, pad = max(5, args.repeats), args.size, args.row_len, 0xFFFFFFFF
    tr = api.Engine(args.device)
    tr.synth(2, args.train_size)
    tr.train(args.merges)
    vocab = Vocab.from_merges(tr.merges(), "cl100k", SPECIALS)
    tr.close()
    sample = np.frombuffer(english_like(min(args.sample, n)), np.uint8)
    host = np.tile(sample, (n + sample.size - 1) // sample.size)[:n]
    raw = host.tobytes()
    out = {"tool": "texts_bench", "bytes": n, "merges": int(vocab.merges.shape[0]), "rule": "cl100k",
           "specials": len(SPECIALS), "row_len": row_len, "repeats": reps, "cuts": {}}
    e = api.Engine(args.device)
    other = OtherLibrary(args.parent_lib, args.device, vocab)
    tok, tok1 = Tokenizer(vocab, args.device), Tokenizer(vocab, args.device)
    for cut in (int(c) for c in args.cuts.split(",")):
        off = np.arange(0, n + cut, cut, dtype=np.uint64)
        off[-1] = n
        T = off.size - 1
        texts = [raw[int(a):int(b)] for a, b in zip(off[:-1], off[1:])]
        k = min(args.loop_texts, T)
        dev = torch.device("cuda", args.device)
        rows_dev = torch.empty((T, row_len), dtype=torch.int32, device=dev)
        copy_src, copy_dst = torch.ones_like(rows_dev), torch.empty_like(rows_dev)
        t = {key: [] for key in ("batch", "one_text", "encode_batch", "loop", "pack", "copy", "host_pad")}
        steps = ("load", "split", "encode_split", "map_ids")
        t.update({f"{leg}_{st}": [] for leg in ("batch", "one_text") for st in steps})
        res = {}
        for rep in range(reps + 1):  # (the first pass warms every leg and is checked, not timed)
            t0 = time.perf_counter()
            e.load_texts(raw, offsets=off)
            ta = time.perf_counter()
            pieces = e.split("cl100k", SPECIALS)
            tb = time.perf_counter()
            e.encode_split(vocab.merges)
            tc = time.perf_counter()
            e.map_ids(vocab)
            t1 = time.perf_counter()
            pieces_one, one_steps = other.run(host)
            t2 = time.perf_counter()
            e.pack_texts(row_len, pad, "right", out=rows_dev)
            t3 = time.perf_counter()
            copy_dst.copy_(copy_src)
            torch.cuda.synchronize(dev)
            t4 = time.perf_counter()
            ids, toff = e.ids(), e.text_offsets()
            rows_host, lens_host = host_pad(ids, toff, row_len, pad)
            t5 = time.perf_counter()
            if rep == 0:
                kept = int(lens_host.sum(dtype=np.int64))
                res = {"ids_in_rows": kept, "texts": T, "pieces": int(pieces), "pieces_as_one_text": int(pieces_one), "ids": int(ids.size),
                       "ids_checksum_batch": e.ids_checksum(), "ids_checksum_one_text": other.checksum(),
                       "rows_equal_host_pad": bool((rows_dev.cpu().numpy().view(np.uint32) == rows_host).all())}
            del rows_host, lens_host
            t6 = time.perf_counter()
            b_ids, b_toff = tok.encode_batch(texts)
            t7 = time.perf_counter()
            loop = [tok1.encode(x) for x in texts[:k]]
            t8 = time.perf_counter()
            if rep == 0:
                loop_ids = np.concatenate(loop)
                head = b_ids[:int(b_toff[k])]
                res.update({"ids_checksum_encode_batch": checksum(b_ids), "ids_checksum_batch_first_texts": checksum(head),
                            "ids_checksum_loop_first_texts": checksum(loop_ids),
                            "loop_equals_batch": bool(np.array_equal(head, loop_ids)) and
                            [x.size for x in loop] == np.diff(b_toff[:k + 1].astype(np.int64)).tolist(),
                            "encode_batch_equals_batch": checksum(b_ids) == res["ids_checksum_batch"]})
                if not (res["loop_equals_batch"] and res["encode_batch_equals_batch"] and res["rows_equal_host_pad"]):
                    sys.exit(f"texts_bench: cut {cut}: the legs disagree: {json.dumps(res)}")
                continue
            del b_ids, loop
            for key, dt in (("batch", t1 - t0), ("one_text", t2 - t1), ("pack", t3 - t2), ("copy", t4 - t3),
                            ("host_pad", t5 - t4), ("encode_batch", t7 - t6), ("loop", t8 - t7)):
                t[key].append(dt)
            for st, dt in zip(steps, (ta - t0, tb - ta, tc - tb, t1 - tc)):
                t[f"batch_{st}"].append(dt)
            for st, dt in zip(steps, one_steps):
                t[f"one_text_{st}"].append(dt)
        m = {key: med(v) for key, v in t.items()}
        # rows and lens written, the ids kept in the rows and text_off read
        moved = T * row_len * 4 + T * 4 + res["ids_in_rows"] * 4 + (T + 1) * 8
        res.update(m)
        res.update({
            "batch_over_one_text": round(m["batch"]["ms_median"] / m["one_text"]["ms_median"], 3),
            "encode_batch_us_per_text": round(m["encode_batch"]["ms_median"] * 1e3 / T, 3),
            "loop_us_per_text": round(m["loop"]["ms_median"] * 1e3 / k, 3), "loop_texts": k,
            "loop_over_encode_batch_per_text": round((m["loop"]["ms_median"] / k) / (m["encode_batch"]["ms_median"] / T), 1),
            "pack_bytes_moved": int(moved), "pack_gbps": round(moved / m["pack"]["ms_median"] / 1e6, 1),
            "copy_gbps": round(2 * T * row_len * 4 / m["copy"]["ms_median"] / 1e6, 1),
            "pack_over_copy_time": round(m["pack"]["ms_median"] / m["copy"]["ms_median"], 3),
            "host_pad_over_pack_time": round(m["host_pad"]["ms_median"] / m["pack"]["ms_median"], 1)})
        out["cuts"][str(cut)] = res
        print(json.dumps({"progress": cut, **res}), file=sys.stderr, flush=True)
        del rows_dev, copy_src, copy_dst, texts
    tok.close()
    tok1.close()
    other.close()
    e.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Token spans against what they replace, and what they cost a caller who asks for none.

The workload of tools/texts_bench.py: 1 GiB of english_like (a 32 MiB sample repeated) cut into texts of --cuts
bytes each (512 and 2,048), the rule "cl100k" around <|endoftext|> and <|im_start|>, the first --merges merges the
trainer learns on the 1 GiB seed-2 corpus, numbered the engine's own way.  Per cut one checked warm pass, then
--repeats alternated repeats of every leg in one process, reported as median [min .. max]:

  1  spans_byte / spans_char  bpe_gpu_token_spans over the resident (mapped) ids, the spans left on the device
     pack_spans               bpe_gpu_pack_spans(row_len 512) into a torch tensor on the device
     copy                     a device-to-device copy of the bytes pack_spans writes (Tensor.copy_ and a synchronise)
     each with GB/s over the bytes it must move (ids read and spans written; the char unit reads the text too)
  2  host_spans               today's only alternative: Engine.ids() + Engine.text_offsets() fetched and the byte
                              spans computed with numpy (a cumsum of the length table over the ids, the text's
                              first byte taken off)
  3  encode / encode_parent   load_texts + split + encode_split + map_ids, the calls of encode_batch without
                              return_spans, through this build and through the library of the parent commit
                              (--parent-lib, loaded beside this one), by their C calls alone, alternated

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
from llmtokenizer_amd import _lib, api  # noqa: E402
from llmtokenizer_amd.synth import english_like  # noqa: E402
from llmtokenizer_amd.vocab import Vocab  # noqa: E402
from split_bench import med  # noqa: E402

SPECIALS = [b"<|endoftext|>", b"<|im_start|>"]
CL100K = 6  # bpe_gpu.h BPE_SPLIT_CL100K


class Library:
    """load_texts + split + encode_split + map_ids through a build of the library by its C calls alone: nothing of
    this tree's Python is between the clock and the library, and both builds are driven alike"""

    def __init__(self, path, device, vocab):
        self.L = L = ctypes.CDLL(path)
        vp, sz = ctypes.c_void_p, ctypes.c_size_t
        L.bpe_gpu_create.argtypes = [ctypes.c_int, ctypes.POINTER(vp)]
        L.bpe_gpu_destroy.argtypes = [vp]
        L.bpe_gpu_destroy.restype = None
        L.bpe_gpu_load_texts.argtypes = [vp, vp, sz, vp, sz]
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
            sys.exit(f"spans_bench: error {rc} ({self.L.bpe_gpu_last_error().decode()})")

    def run(self, buf, off):
        L, vp, nd = self.L, ctypes.c_void_p, ctypes.c_size_t(0)
        t0 = time.perf_counter()
        self.ok(L.bpe_gpu_load_texts(self.ctx, buf.ctypes.data_as(vp), buf.size, off.ctypes.data_as(vp), off.size - 1))
        self.ok(L.bpe_gpu_split_special(self.ctx, CL100K, None, None, self.sp.ref, ctypes.byref(nd)))
        self.ok(L.bpe_gpu_encode_split(self.ctx, self.merges.ctypes.data_as(vp), self.merges.size // 2))
        self.ok(L.bpe_gpu_map_ids(self.ctx, self.cv.ref))
        return time.perf_counter() - t0

    def checksum(self):
        s = ctypes.c_uint64(0)
        self.ok(self.L.bpe_gpu_ids_checksum(self.ctx, 0, ctypes.byref(s)))
        return s.value

    def close(self):
        self.L.bpe_gpu_destroy(self.ctx)


def host_spans(ids, toff, lens):
    """the byte spans with numpy: what a caller did with the ids on the host"""
    ln = lens[ids].astype(np.int64)
    be = np.cumsum(ln)
    bs = be - ln
    first = np.concatenate([bs, be[-1:]])[toff[:-1].astype(np.int64)] if ids.size else np.zeros(toff.size - 1, np.int64)
    base = np.repeat(first, np.diff(toff.astype(np.int64)))
    return np.stack([bs - base, be - base], axis=1).astype(np.uint32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1 << 30)
    ap.add_argument("--merges", type=int, default=32768)
    ap.add_argument("--train-size", type=int, default=1 << 30)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sample", type=int, default=1 << 25, help="bytes of english_like generated, then repeated")
    ap.add_argument("--cuts", default="512,2048", help="bytes per text, comma separated")
    ap.add_argument("--row-len", type=int, default=512)
    ap.add_argument("--parent-lib", required=True, help="libbpe_amd.so built from the parent commit")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    # torch first: its wheel brings a HIP runtime of its own, and the runtime loaded first is the one that owns the GPU
    import torch
    if not torch.cuda.is_available() or api.device_count() < 1:
        sys.exit("spans_bench: no GPU")
    dev = torch.device("cuda", args.device)
    torch.zeros(1, device=dev)
    reps, n, row_len = max(5, args.repeats), args.size, args.row_len
    tr = api.Engine(args.device)
    tr.synth(2, args.train_size)
    tr.train(args.merges)
    vocab = Vocab.from_merges(tr.merges(), "cl100k", SPECIALS)
    tr.close()
    lens = api.span_lens(vocab.merges, SPECIALS, vocab)
    sample = np.frombuffer(english_like(min(args.sample, n)), np.uint8)
    host = np.ascontiguousarray(np.tile(sample, (n + sample.size - 1) // sample.size)[:n])
    out = {"tool": "spans_bench", "bytes": n, "merges": int(vocab.merges.shape[0]), "rule": "cl100k",
           "specials": len(SPECIALS), "row_len": row_len, "repeats": reps, "cuts": {}}
    e = api.Engine(args.device)
    here, parent = Library(_lib.LIB_PATH, args.device, vocab), Library(args.parent_lib, args.device, vocab)
    for cut in (int(c) for c in args.cuts.split(",")):
        off = np.arange(0, n + cut, cut, dtype=np.uint64)
        off[-1] = n
        T = off.size - 1
        rows_dev = torch.empty((T, row_len, 2), dtype=torch.int32, device=dev)
        copy_src, copy_dst = torch.ones_like(rows_dev), torch.empty_like(rows_dev)
        e.load_texts(host, offsets=off)
        e.split("cl100k", SPECIALS)
        e.encode_split(vocab.merges)
        e.map_ids(vocab)
        pairs, k, sp, cv, keep = api._span_args(vocab.merges, SPECIALS, vocab)
        t = {key: [] for key in ("spans_byte", "spans_char", "pack_spans", "copy", "host_spans", "encode", "encode_parent")}
        res = {}
        for rep in range(reps + 1):  # (the first pass warms every leg and is checked, not timed)
            t0 = time.perf_counter()
            _lib.check(e.L.bpe_gpu_token_spans(e.ctx, pairs, k, sp, cv, 1), "token_spans")
            t1 = time.perf_counter()
            _lib.check(e.L.bpe_gpu_token_spans(e.ctx, pairs, k, sp, cv, 0), "token_spans")
            t2 = time.perf_counter()
            # (the C call: Engine.pack_spans fetches text_off first, to check the tensor's shape)
            _lib.check(e.L.bpe_gpu_pack_spans(e.ctx, row_len, 0, ctypes.c_void_p(rows_dev.data_ptr()), 1), "pack_spans")
            t3 = time.perf_counter()
            copy_dst.copy_(copy_src)
            torch.cuda.synchronize(dev)
            t4 = time.perf_counter()
            ids, toff = e.ids(), e.text_offsets()
            hs = host_spans(ids, toff, lens)
            t5 = time.perf_counter()
            # the two builds in turn, the order swapped every repeat
            order = (here, parent) if rep % 2 else (parent, here)
            dt = {lib: lib.run(host, off) for lib in order}
            if rep == 0:
                kept = int(np.minimum(np.diff(toff.astype(np.int64)), row_len).sum())
                nid = ctypes.c_size_t(0)
                _lib.check(e.L.bpe_gpu_fetch_token_spans(e.ctx, None, 0, ctypes.byref(nid)), "fetch_token_spans")
                dev_spans = np.zeros((nid.value, 2), dtype=np.uint32)
                _lib.check(e.L.bpe_gpu_fetch_token_spans(e.ctx, dev_spans.ctypes.data_as(ctypes.c_void_p), nid.value,
                                                         ctypes.byref(nid)), "fetch_token_spans")
                first_row = rows_dev[0].cpu().numpy().view(np.uint32)
                res = {"texts": T, "ids": int(ids.size), "ids_in_rows": kept,
                       "spans_equal_host": bool(np.array_equal(dev_spans, hs)),
                       "first_row_equal": bool(np.array_equal(first_row[:min(row_len, int(toff[1]))], hs[:min(row_len, int(toff[1]))])),
                       "ids_checksum": here.checksum(), "ids_checksum_parent": parent.checksum()}
                if not (res["spans_equal_host"] and res["first_row_equal"] and res["ids_checksum"] == res["ids_checksum_parent"]):
                    sys.exit(f"spans_bench: cut {cut}: the legs disagree: {json.dumps(res)}")
                del dev_spans
            del hs
            if rep == 0:
                continue
            for key, d in (("spans_char", t1 - t0), ("spans_byte", t2 - t1), ("pack_spans", t3 - t2), ("copy", t4 - t3),
                           ("host_spans", t5 - t4), ("encode", dt[here]), ("encode_parent", dt[parent])):
                t[key].append(d)
        m = {key: med(v) for key, v in t.items()}
        nid = res["ids"]
        moved = {"spans_byte": 12 * nid, "spans_char": 12 * nid + n + T,
                 "pack_spans": T * row_len * 8 + res["ids_in_rows"] * 8 + (T + 1) * 8}
        res.update(m)
        res.update({f"{key}_bytes_moved": int(b) for key, b in moved.items()})
        res.update({f"{key}_gbps": round(b / m[key]["ms_median"] / 1e6, 1) for key, b in moved.items()})
        res.update({
            "copy_gbps": round(2 * T * row_len * 8 / m["copy"]["ms_median"] / 1e6, 1),
            "pack_spans_over_copy_time": round(m["pack_spans"]["ms_median"] / m["copy"]["ms_median"], 3),
            "host_spans_over_spans_byte_time": round(m["host_spans"]["ms_median"] / m["spans_byte"]["ms_median"], 1),
            "encode_over_parent": round(m["encode"]["ms_median"] / m["encode_parent"]["ms_median"], 4)})
        out["cuts"][str(cut)] = res
        print(json.dumps({"progress": cut, **res}), file=sys.stderr, flush=True)
        del rows_dev, copy_src, copy_dst
    here.close()
    parent.close()
    e.close()
    line = json.dumps(out)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()

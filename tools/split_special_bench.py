#!/usr/bin/env python3
"""What the special tokens cost on the device, in tools/split_bench.py's
loop: a corpus resident in HBM, alternated repeats, median and spread, the device-to-device
copy of the same bytes as the yardstick.

Two corpora of --size bytes: english_like with <|endoftext|> inserted about every 2 KiB (a
sample generated on the host and repeated), and the seed-3 synthetic corpus (no special occurs
in it).  Per corpus and rule ("words", "gpt2"), alternated in one loop:
  none     Engine.split(rule)
  absent   Engine.split(rule, [a special that never occurs]): the cost of looking
  real     Engine.split(rule, the ChatML set)
  copy     hipMemcpyAsync device to device of the same bytes
and, with a merge list trained on the sample,
  plain    Engine.split(rule) + Engine.encode_split(merges)
  special  Engine.split(rule, set) + Engine.encode_split(merges): the post-pass included
  parent   the same two calls of another build of the library (--parent-lib: the parent
           commit's libbpe_amd.so, driven through its C-ABI in this process), when given.
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
from split_bench import DeviceCopy, med  # noqa: E402

EOT = b"<|endoftext|>"
REAL = [EOT, b"<|im_start|>", b"<|im_end|>", b"<|fim_prefix|>", b"<|fim_middle|>", b"<|fim_suffix|>"]
ABSENT = [b"<|never_occurs|>"]


class ParentLib:
    """split_preset + encode_split of another libbpe_amd.so on a context of its own"""

    def __init__(self, path, device, data):
        L = self.L = ctypes.CDLL(path)
        vp, sz = ctypes.c_void_p, ctypes.c_size_t
        L.bpe_gpu_create.argtypes = [ctypes.c_int, ctypes.POINTER(vp)]
        L.bpe_gpu_destroy.argtypes = [vp]
        L.bpe_gpu_destroy.restype = None
        L.bpe_gpu_load.argtypes = [vp, vp, sz]
        L.bpe_gpu_synth.argtypes = [vp, ctypes.c_uint64, sz, ctypes.c_uint64]
        L.bpe_gpu_split_preset.argtypes = [vp, ctypes.c_int, ctypes.POINTER(sz)]
        L.bpe_gpu_encode_split.argtypes = [vp, vp, sz]
        L.bpe_gpu_ids_checksum.argtypes = [vp, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]
        self.ctx = vp()
        self.ok(L.bpe_gpu_create(device, ctypes.byref(self.ctx)))
        if isinstance(data, int):
            self.ok(L.bpe_gpu_synth(self.ctx, 3, data, 0))
        else:
            self.ok(L.bpe_gpu_load(self.ctx, data.ctypes.data_as(vp), data.size))

    def ok(self, rc):
        if rc:
            sys.exit(f"split_special_bench: the parent library failed ({rc})")

    def run(self, rule, merges):
        nd = ctypes.c_size_t(0)
        m = np.ascontiguousarray(merges, dtype=np.uint32).reshape(-1)
        self.ok(self.L.bpe_gpu_split_preset(self.ctx, api.SPLIT_PRESETS[rule], ctypes.byref(nd)))
        self.ok(self.L.bpe_gpu_encode_split(self.ctx, m.ctypes.data_as(ctypes.c_void_p), m.size // 2))

    def checksum(self):
        s = ctypes.c_uint64(0)
        self.ok(self.L.bpe_gpu_ids_checksum(self.ctx, 0, ctypes.byref(s)))
        return s.value

    def close(self):
        self.L.bpe_gpu_destroy(self.ctx)


def timed(f):
    t0 = time.perf_counter()
    f()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1 << 30)
    ap.add_argument("--merges", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sample", type=int, default=1 << 25, help="bytes of english_like generated, then repeated")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    if api.device_count() < 1:
        sys.exit("split_special_bench: no GPU")
    reps, n = max(5, args.repeats), args.size
    base = english_like(min(args.sample, n))
    sample = np.frombuffer(EOT.join(base[i:i + 2048] for i in range(0, len(base), 2048)), np.uint8)
    merges, _ = api.train_bytes(base[: 1 << 26], args.merges, device=args.device)
    out = {"tool": "split_special_bench", "bytes": n, "merges": int(len(merges)), "repeats": reps, "split": {}, "encode": {}}
    cp = DeviceCopy(n)
    e = api.Engine(args.device)
    for corpus in ("english_like+eot", "seed3"):
        if corpus == "seed3":
            e.synth(3, n)
            host = n
        else:
            host = np.tile(sample, (n + sample.size - 1) // sample.size)[:n]
            e.load(host.tobytes())
        par = ParentLib(args.parent_lib, args.device, host) if args.parent_lib else None
        for rule in ("words", "gpt2"):
            key = f"{corpus}/{rule}"
            runs = {"none": lambda: e.split(rule), "absent": lambda: e.split(rule, ABSENT), "real": lambda: e.split(rule, REAL),
                    "copy": cp.run}
            ts = {k: [] for k in runs}
            for f in runs.values():  # warm
                f()
            for _ in range(reps):  # alternated: other work shares the machine
                for k, f in runs.items():
                    ts[k].append(timed(f))
            res = {k: med(v) for k, v in ts.items()}
            pieces = e.split(rule, REAL)
            res["pieces_real"], res["special"] = int(pieces), e.split_special_info()
            res["pieces_none"] = int(e.split(rule))
            c = res["copy"]["ms_median"]
            res["copy_gbps"] = round(2 * n / c / 1e6, 1)
            for k in ("none", "absent", "real"):
                res[k + "_over_copy"] = round(res[k]["ms_median"] / c, 3)
            out["split"][key] = res

            def plain():
                e.split(rule)
                e.encode_split(merges)

            def special():
                e.split(rule, REAL)
                e.encode_split(merges)

            runs = {"plain": plain, "special": special}
            if par:
                runs["parent"] = lambda: par.run(rule, merges)
            ts = {k: [] for k in runs}
            plain()
            sums = {"plain": e.ids_checksum()}
            if par:
                par.run(rule, merges)
                sums["parent"] = par.checksum()
                if sums["parent"] != sums["plain"]:
                    sys.exit(f"split_special_bench: {key}: the parent's ids differ from the plain path's")
            special()
            sums["special"], ids_special = e.ids_checksum(), int(e.stats()["n_out"])
            for _ in range(reps):
                for k, f in runs.items():
                    ts[k].append(timed(f))
            enc = {k: med(v) for k, v in ts.items()}
            enc["ids_special"], enc["checksums"] = ids_special, {k: f"{v:016x}" for k, v in sums.items()}
            enc["special_over_plain"] = round(enc["special"]["ms_median"] / enc["plain"]["ms_median"], 3)
            if par:
                enc["plain_over_parent"] = round(enc["plain"]["ms_median"] / enc["parent"]["ms_median"], 3)
            out["encode"][key] = enc
            print(json.dumps({"progress": key, "split": res, "encode": enc}), file=sys.stderr, flush=True)
        if par:
            par.close()
    e.close()
    cp.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The on-device split against the streaming rate of the card, and split +
encode_split against the host-offset path it replaces.

Two 1 GiB corpora resident in HBM: the seed-3 synthetic corpus (Engine.synth;
printable bytes, no newline) and english_like (a 32 MiB sample generated on the
host and repeated to the size).  Three rules: the table rules "lines" and
"words", and "gpt2", "gpt2_unicode" and "cl100k" (bpe_gpu_split_preset; their own
marking kernels).  A third corpus, english_nonascii, is english_like with every
--nonascii-th letter replaced by a two-byte Cyrillic letter (D0 B0..BF): the
ASCII corpora take gpt2_unicode's all-ASCII path, this one its decoding path.
Two more are one run each, for the rules whose starts depend on the position in
a run ("cl100k"): digits (the ten digits over and over) and spaces_newline
(spaces and one final newline).  --corpora selects among the five.

  split    Engine.split(rule) alone, alternated with a device-to-device
           hipMemcpyAsync of the same number of bytes timed the same way (host
           clock around launch + stream synchronise): the streaming yardstick
           of the box.  Reported: ms, pieces, the bytes the design moves
           (n read, n / 8 of start masks written and read again, 8 B per offset
           written, 12 B per 1,024 bytes of counts and their scan; for "cl100k" n
           read once more by its summary pass and 16 B per 1,024 bytes of chain
           effects and their scan) per second,
           and that rate over the copy's (2 n bytes per copy).
  split_ab per corpus, Engine.split("words") and Engine.split("gpt2") alternated in
           one loop: the two marking kernels side by side (their emit passes
           differ by the piece counts only).
  e2e      per corpus and rule, alternated in one process:
             resident  Engine.split + Engine.encode_split
             host      Engine.encode_docs(offsets, merges) with the same offsets
                       from host memory (what the library offered before), and
                       the time the host takes to make them (numpy's
                       restatement of the tables in 32 MiB chunks; for
                       "gpt2" api.split_host, the rule in plain C),
                       reported apart
             single    Engine.encode(merges), the single-stream ceiling
           with the merge list of tools/docs_bench.py (the first --merges
           merges the trainer learns on the 1 GiB seed-2 corpus).

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
from llmtokenizer_amd import api  # noqa: E402
from llmtokenizer_amd.synth import english_like, synth_bytes  # noqa: E402


def restate(buf, cls, brk, chunk=1 << 25):
    """the rule's numpy restatement over a uint8 array, chunked (a carry of one class)"""
    parts, prev = [], None
    for lo in range(0, buf.size, chunk):
        c = cls[buf[lo:lo + chunk]]
        st = np.empty(c.size, bool)
        st[0] = True if prev is None else (brk[prev] >> c[0]) & 1
        st[1:] = (brk[c[:-1]] >> c[1:]) & 1
        parts.append(np.flatnonzero(st).astype(np.uint64) + np.uint64(lo))
        prev = c[-1]
    parts.append(np.array([buf.size], dtype=np.uint64))
    return np.concatenate(parts)


def nonascii(sample, every):
    """sample with every `every`-th ASCII letter replaced by the two bytes D0, B0 + (letter & 15)"""
    letters = np.flatnonzero(((sample | 0x20) >= ord("a")) & ((sample | 0x20) <= ord("z")))[::every]
    width = np.ones(sample.size, np.int64)
    width[letters] = 2
    at = np.cumsum(width) - width
    out = np.empty(int(width.sum()), np.uint8)
    out[at] = sample
    out[at[letters]] = 0xD0
    out[at[letters] + 1] = 0xB0 + (sample[letters] & 15)
    return out


NO_TABLES = ("gpt2", "gpt2_unicode", "cl100k")
CORPORA = ("seed3", "english_like", "english_nonascii", "digits", "spaces_newline")


def med(xs):
    s = sorted(xs)
    return {"ms_median": round(s[len(s) // 2] * 1e3, 3), "ms_min": round(s[0] * 1e3, 3),
            "ms_max": round(s[-1] * 1e3, 3), "repeats": len(s)}


class DeviceCopy:
    """hipMemcpyAsync device to device of n bytes on a stream of its own, through the HIP runtime the
    library already loaded"""

    def __init__(self, n):
        root = os.environ.get("ROCM_PATH", "/opt/rocm")
        try:
            self.hip = ctypes.CDLL("libamdhip64.so")
        except OSError:
            self.hip = ctypes.CDLL(os.path.join(root, "lib", "libamdhip64.so"))
        h = self.hip
        vp = ctypes.c_void_p
        h.hipMalloc.argtypes = [ctypes.POINTER(vp), ctypes.c_size_t]
        h.hipFree.argtypes = [vp]
        h.hipMemsetAsync.argtypes = [vp, ctypes.c_int, ctypes.c_size_t, vp]
        h.hipMemcpyAsync.argtypes = [vp, vp, ctypes.c_size_t, ctypes.c_int, vp]
        h.hipStreamCreate.argtypes = [ctypes.POINTER(vp)]
        h.hipStreamSynchronize.argtypes = [vp]
        h.hipStreamDestroy.argtypes = [vp]
        self.n = n
        self.src, self.dst, self.st = vp(), vp(), vp()
        for rc in (h.hipMalloc(ctypes.byref(self.src), n), h.hipMalloc(ctypes.byref(self.dst), n),
                   h.hipStreamCreate(ctypes.byref(self.st)), h.hipMemsetAsync(self.src, 1, n, self.st),
                   h.hipStreamSynchronize(self.st)):
            if rc:
                sys.exit(f"split_bench: HIP error {rc} setting up the copy")

    def run(self):
        t0 = time.perf_counter()
        rc = self.hip.hipMemcpyAsync(self.dst, self.src, self.n, 3, self.st)  # 3: hipMemcpyDeviceToDevice
        rc = rc or self.hip.hipStreamSynchronize(self.st)
        t1 = time.perf_counter()
        if rc:
            sys.exit(f"split_bench: HIP error {rc} in the copy")
        return t1 - t0

    def close(self):
        self.hip.hipStreamDestroy(self.st)
        self.hip.hipFree(self.src)
        self.hip.hipFree(self.dst)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1 << 30)
    ap.add_argument("--merges", type=int, default=32768)
    ap.add_argument("--train-size", type=int, default=1 << 30)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sample", type=int, default=1 << 25, help="bytes of english_like generated, then repeated")
    ap.add_argument("--no-e2e", action="store_true", help="the split alone")
    ap.add_argument("--rules", default="lines,words,gpt2,gpt2_unicode,cl100k", help="the rules to run, comma separated")
    ap.add_argument("--corpora", default=",".join(CORPORA), help="the corpora to run, comma separated")
    ap.add_argument("--nonascii", type=int, default=4, help="english_nonascii: one letter in this many is two bytes")
    ap.add_argument("--check-bytes", type=int, default=0,
                    help="with --no-e2e: compare the device's offsets with split_host over this many leading bytes")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    if api.device_count() < 1:
        sys.exit("split_bench: no GPU")
    reps = max(5, args.repeats)
    n = args.size
    out = {"tool": "split_bench", "bytes": n, "split": {}, "split_ab": {}, "e2e": {}}
    merges = None
    if not args.no_e2e:
        tr = api.Engine(args.device)
        tr.synth(2, args.train_size)
        tr.train(args.merges)
        merges = tr.merges()
        tr.close()
        out["merges"] = int(len(merges))
    cp = DeviceCopy(n)
    e = api.Engine(args.device)
    sample = np.frombuffer(english_like(min(args.sample, n)), np.uint8)
    for corpus in args.corpora.split(","):
        if corpus not in CORPORA:
            sys.exit(f"split_bench: no corpus {corpus!r} (have {CORPORA})")
        if corpus == "seed3":
            e.synth(3, n)
            host = None
        elif corpus in ("digits", "spaces_newline"):  # one run as long as the text
            host = np.tile(np.frombuffer(b"0123456789", np.uint8), n // 10 + 1)[:n] if corpus == "digits" else np.full(n, 0x20, np.uint8)
            if corpus == "spaces_newline":
                host[-1] = 0x0A
            e.load(host.tobytes())
        else:
            part = sample if corpus == "english_like" else nonascii(sample, args.nonascii)
            host = np.tile(part, (n + part.size - 1) // part.size)[:n]
            e.load(host.tobytes())
        for rule in args.rules.split(","):
            key = f"{corpus}/{rule}"
            nd = e.split(rule)  # warm
            cp.run()
            t_split, t_copy = [], []
            for _ in range(reps):  # alternated: other work shares the box
                t0 = time.perf_counter()
                e.split(rule)
                t1 = time.perf_counter()
                t_split.append(t1 - t0)
                t_copy.append(cp.run())
            moved = n + n // 4 + 8 * (nd + 1) + 12 * (n // 1024) + (n + 16 * (n // 1024) if rule == "cl100k" else 0)
            ms, mc = med(t_split), med(t_copy)
            rate = moved / (ms["ms_median"] * 1e-3) / 1e9
            copy_rate = 2 * n / (mc["ms_median"] * 1e-3) / 1e9
            out["split"][key] = {
                "pieces": int(nd), "bytes_per_piece": round(n / max(nd, 1), 2), "split": ms, "copy": mc,
                "bytes_moved": int(moved), "algorithmic_bytes": int(n + 8 * (nd + 1)),
                "gbps": round(rate, 1), "copy_gbps": round(copy_rate, 1), "over_copy": round(rate / copy_rate, 3)}
            if args.no_e2e:
                if args.check_bytes and rule in NO_TABLES:
                    k = min(args.check_bytes, n)
                    head = synth_bytes(3, k) if host is None else host[:k].tobytes()
                    want = api.split_host(head, rule)[:-16]  # (the last pieces of the head see its end)
                    if not (e.split_offsets()[:want.size] == want).all():
                        sys.exit(f"split_bench: {key}: the device's offsets differ from split_host")
                    out["split"][key]["offsets_equal_split_host_over_bytes"] = int(want[-1]) if want.size else 0
                continue
            if host is None:  # the parent path's user holds the text on the host
                host = np.frombuffer(synth_bytes(3, n), np.uint8)
            t0 = time.perf_counter()
            off = api.split_host(host, rule) if rule in NO_TABLES else restate(host, *api.split_rule(rule))
            t_numpy = time.perf_counter() - t0
            if off.size - 1 != nd or not (e.split_offsets() == off).all():
                sys.exit(f"split_bench: {key}: the device's offsets differ from the restatement")
            e.encode_split(merges)  # warm all three
            sum_split = e.ids_checksum()
            info = e.docs_info()
            e.encode_docs(off, merges)
            if e.ids_checksum() != sum_split:
                sys.exit(f"split_bench: {key}: encode_split and encode_docs disagree")
            e.encode(merges)
            t_res, t_res_split, t_host, t_single = [], [], [], []
            for _ in range(reps):
                t0 = time.perf_counter()
                e.split(rule)
                t1 = time.perf_counter()
                e.encode_split(merges)
                t2 = time.perf_counter()
                e.encode_docs(off, merges)
                t3 = time.perf_counter()
                e.encode(merges)
                t4 = time.perf_counter()
                t_res.append(t2 - t0)
                t_res_split.append(t1 - t0)
                t_host.append(t3 - t2)
                t_single.append(t4 - t3)
            r, h, s = med(t_res), med(t_host), med(t_single)
            out["e2e"][key] = {
                "pieces": int(nd), "resident": r, "resident_split_part": med(t_res_split),
                "resident_encode_part": med([a - b for a, b in zip(t_res, t_res_split)]), "host_offsets": h,
                "numpy_offsets_ms": round(t_numpy * 1e3, 1), "offsets_made_by": "split_host" if rule in NO_TABLES else "numpy",
                "single": s, "docs_info": info,
                "resident_gbps": round(n / r["ms_median"] / 1e6, 2), "host_gbps": round(n / h["ms_median"] / 1e6, 2),
                "host_with_numpy_gbps": round(n / (h["ms_median"] + t_numpy * 1e3) / 1e6, 3),
                "single_gbps": round(n / s["ms_median"] / 1e6, 2),
                "resident_over_host": round(h["ms_median"] / r["ms_median"], 3),
                "resident_over_single": round(s["ms_median"] / r["ms_median"], 3),
                "single_spread": round((s["ms_max"] - s["ms_min"]) / s["ms_median"], 4)}
            del off
            print(json.dumps({"progress": key, **out["e2e"][key]}), file=sys.stderr, flush=True)
        ab = {rule: [] for rule in ("words", "gpt2", "gpt2_unicode", "cl100k") if rule in args.rules.split(",")}
        for _ in range(reps):
            for rule, ts in ab.items():
                t0 = time.perf_counter()
                e.split(rule)
                ts.append(time.perf_counter() - t0)
        out["split_ab"][corpus] = {rule: med(ts) for rule, ts in ab.items()}
    e.close()
    cp.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

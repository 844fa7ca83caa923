#!/usr/bin/env python3
"""Engine.normalize("nfc") against a copy and against the split it feeds.

Three inputs of --mib MiB each, a sample repeated: "ascii" (english_like), "mixed" (Latin with accents in NFC,
Cyrillic and CJK sentences in turn: clean, but nearly every lane has to look its characters up) and "dirty" (the
ASCII sample with a decomposed "e" + U+0301 written over it about every hundred characters: about 1 % of the
segments are dirty, and the result is shorter than the input).  Per input:

  normalize   the load is not timed; host clock around Engine.normalize, which ends in a synchronise
  copy        a device-to-device copy of as many bytes, same process, alternated with the other legs
  split       Engine.split("cl100k") of the same resident bytes (the stage behind the normalizer)

--repeats alternated repeats, reported as median [min .. max]; the first pass warms every leg and is checked
(the normalized bytes against api.nfc_host on the first 8 MiB).  One JSON line.  Needs a GPU; there is no CPU path.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from llmtokenizer_amd import api  # noqa: E402
from llmtokenizer_amd.synth import english_like  # noqa: E402
from split_bench import DeviceCopy, med  # noqa: E402

MIXED = ("Größe und Straße: die Füchse springen über den faulen Hund. Ça va très bien, merci à vous. "
         "Быстрая коричневая лиса прыгает через ленивую собаку, а собака спит. "
         "日本語のテキストも少しだけ入れておきます。狐は犬を飛び越える。\n")


def inputs(size, sample):
    ascii_ = bytes(english_like(sample, 7))
    dirty = bytearray(ascii_)
    mark = "e\u0301".encode()
    for p in range(50, len(dirty) - 3, 100):
        dirty[p:p + 3] = mark
    mixed = MIXED.encode()
    rep = lambda b: (b * (size // len(b) + 1))[:size]  # noqa: E731
    return {"ascii": rep(ascii_), "mixed": rep(mixed * 64), "dirty": rep(bytes(dirty))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--sample", type=int, default=1 << 24, help="bytes of english_like generated, then repeated")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    if api.device_count() < 1:
        sys.exit("normalize_bench: no GPU")
    size = args.mib << 20
    e = api.Engine(args.device)
    copy = DeviceCopy(size)
    res = {"bytes": size, "info": api.normalize_info(), "inputs": {}}
    for name, data in inputs(size, min(args.sample, size)).items():
        legs = {"normalize": [], "copy": [], "split": []}
        out_len = None
        for it in range(args.repeats + 1):
            e.load(data)
            t0 = time.perf_counter()
            out_len = e.normalize("nfc")
            t_norm = time.perf_counter() - t0
            t_copy = copy.run()
            t0 = time.perf_counter()
            e.split("cl100k")
            t_split = time.perf_counter() - t0
            if it == 0:  # warm, and checked
                head = 8 << 20
                want = api.nfc_host(data[:head])
                e.load(data[:head])
                e.normalize("nfc")
                if e.bytes() != want:
                    sys.exit(f"normalize_bench: {name}: the device and nfc_host disagree")
                continue
            legs["normalize"].append(t_norm)
            legs["copy"].append(t_copy)
            legs["split"].append(t_split)
        r = {k: med(v) for k, v in legs.items()}
        r["out_bytes"] = out_len
        r["normalize_GBps"] = round(size / (r["normalize"]["ms_median"] * 1e6), 1)
        r["copy_GBps"] = round(size / (r["copy"]["ms_median"] * 1e6), 1)
        res["inputs"][name] = r
    copy.close()
    e.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

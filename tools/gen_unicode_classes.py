#!/usr/bin/env python3
"""Write llmtokenizer_amd/csrc/unicode_classes.h: the class of every code point for
BPE_SPLIT_GPT2_UNICODE (bpe_gpu.h), asked of the `regex` module installed here.

    python tools/gen_unicode_classes.py            # writes the header
    python tools/gen_unicode_classes.py --check    # exit 1 unless the header on disk is what would be written

Classes, in this order: S U+0020; W White_Space (regex's \\s: 25 code points with the
space); L \\p{L}; N \\p{N}; P the rest.  The header holds a two-stage table (a block index
per 256 code points, then the distinct blocks at 2 bits per code point: 0 P, 1 L, 2 N,
3 W; the one S is U+0020 and is told apart in code), the regex version the classes came
from and the FNV-1a 64 digest of the 0x110000 classes as bytes 0 P, 1 L, 2 N, 3 S, 4 W.
Plain C only: the host C and the HIP side both include it.  Not run by any test.
"""
import argparse
import os
import sys

import regex

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "llmtokenizer_amd", "csrc", "unicode_classes.h")
NCP = 0x110000
P, L, N, S, W = 0, 1, 2, 3, 4


def classes():
    """bytes of length 0x110000: the class of every code point"""
    text = "".join(chr(c) for c in range(NCP))
    out = bytearray(NCP)
    for pat, k in ((r"\p{N}", N), (r"\p{L}", L), (r"\s", W)):  # (later ones win: the order of the definition)
        for m in regex.finditer(pat, text):
            out[ord(m.group())] = k
    out[0x20] = S
    return bytes(out)


def fnv1a64(data):
    h = 0xCBF29CE484222325
    for b in data:
        h = ((h ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


def render():
    cl = classes()
    ws = [c for c in range(NCP) if cl[c] in (S, W)]
    assert len(ws) == 25, ws
    two = bytes({P: 0, L: 1, N: 2, S: 3, W: 3}[k] for k in cl)
    blocks, index = {}, []
    for b in range(NCP >> 8):
        blk = two[b << 8:(b + 1) << 8]
        index.append(blocks.setdefault(blk, len(blocks)))
    assert len(blocks) <= 256
    words = []
    for blk in blocks:  # (insertion order: the block numbers)
        for w in range(16):
            v = 0
            for k in range(16):
                v |= blk[16 * w + k] << (2 * k)
            words.append(v)
    size = len(index) + 4 * len(words)
    o = []
    o.append("/* unicode_classes.h -- written by tools/gen_unicode_classes.py; do not edit.")
    o.append(" *")
    o.append(" * The classes of BPE_SPLIT_GPT2_UNICODE (bpe_gpu.h) for every code point, from the `regex` module")
    o.append(f" * {regex.__version__}: L \\p{{L}}, N \\p{{N}}, W White_Space (S is U+0020 alone, told apart in code), P the rest.")
    o.append(" * Two stages: BPE_UC_STAGE1[cp >> 8] names one of BPE_UC_BLOCKS distinct blocks of 256 code points;")
    o.append(" * a block is 16 words, 2 bits per code point (0 P, 1 L, 2 N, 3 W), code point cp in word")
    o.append(" * (cp >> 4) & 15 at bits 2 * (cp & 15).")
    o.append(f" * {len(index)} + 4 * {len(words)} = {size} bytes.  Plain C: the host C and the HIP side include it")
    o.append(" * (BPE_UC_STORAGE: the storage class of the two arrays, `static const` unless defined). */")
    o.append("#ifndef BPE_UNICODE_CLASSES_H")
    o.append("#define BPE_UNICODE_CLASSES_H")
    o.append("#include <stdint.h>")
    o.append("")
    o.append(f'#define BPE_UC_SOURCE "regex {regex.__version__}"')
    o.append(f"#define BPE_UC_DIGEST 0x{fnv1a64(cl):016X}ull /* FNV-1a 64 of the 0x110000 classes (0 P, 1 L, 2 N, 3 S, 4 W) */")
    o.append(f"#define BPE_UC_BLOCKS {len(blocks)}")
    o.append(f"#define BPE_UC_TABLE_BYTES {size}")
    o.append("#ifndef BPE_UC_STORAGE")
    o.append("#define BPE_UC_STORAGE static const")
    o.append("#endif")
    o.append("")
    o.append(f"BPE_UC_STORAGE uint8_t BPE_UC_STAGE1[{len(index)}] = {{")
    for i in range(0, len(index), 32):
        o.append("    " + ",".join(str(v) for v in index[i:i + 32]) + ",")
    o.append("};")
    o.append("")
    o.append(f"BPE_UC_STORAGE uint32_t BPE_UC_STAGE2[{len(words)}] = {{")
    for i in range(0, len(words), 8):
        o.append("    " + ",".join(f"0x{v:08X}u" for v in words[i:i + 8]) + ",")
    o.append("};")
    o.append("")
    o.append("#endif")
    return "\n".join(o) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    text = render()
    if a.check:
        with open(OUT) as f:
            same = f.read() == text
        print("unicode_classes.h:", "up to date" if same else "differs")
        return 0 if same else 1
    with open(OUT, "w") as f:
        f.write(text)
    print(f"wrote {OUT} ({len(text)} bytes)")
    return 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Write llmtokenizer_amd/csrc/unicode_case_classes.h: the case class of every code point for
BPE_SPLIT_O200K (bpe_gpu.h), asked of the `regex` module installed here.  The sibling of
gen_unicode_classes.py, whose header stays what it is.

    python tools/gen_unicode_case_classes.py            # writes the header
    python tools/gen_unicode_case_classes.py --check    # exit 1 unless the header on disk is what would be written

Case classes: 0 other, 1 U (\\p{Lu} \\p{Lt}), 2 l (\\p{Ll}), 3 B (\\p{Lm} \\p{Lo}), 4 M (\\p{M}).  The header
holds a two-stage table (a block index per 256 code points, then the distinct blocks at 4 bits per code
point), the regex version and the FNV-1a 64 digest of the 0x110000 case classes as bytes.  So that the
device asks one table per character, a code point of case class 0 carries 5 when it is \\p{N} and 6 when
it is White_Space; bpe_unicode_case_class reports both as 0.  Plain C only.  Not run by any test.
"""
import argparse
import os
import sys

import regex

from gen_unicode_classes import NCP, fnv1a64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "llmtokenizer_amd", "csrc", "unicode_case_classes.h")
O, U, LL, B, M, N, W = range(7)


def classes():
    """(case classes, table codes): two bytes objects of length 0x110000"""
    text = "".join(chr(c) for c in range(NCP))
    case, code = bytearray(NCP), bytearray(NCP)
    for pat, k in ((r"\p{N}", N), (r"\s", W), (r"[\p{Lu}\p{Lt}]", U), (r"\p{Ll}", LL), (r"[\p{Lm}\p{Lo}]", B), (r"\p{M}", M)):
        for m in regex.finditer(pat, text):
            code[ord(m.group())] = k
            if k <= M:
                case[ord(m.group())] = k
    letters = sum(1 for _ in regex.finditer(r"\p{L}", text))
    assert letters == sum(1 for k in case if k in (U, LL, B)), "Lu Lt Ll Lm Lo are all of \\p{L}"
    return bytes(case), bytes(code)


def render():
    case, code = classes()
    blocks, index = {}, []
    for b in range(NCP >> 8):
        index.append(blocks.setdefault(code[b << 8:(b + 1) << 8], len(blocks)))
    assert len(blocks) <= 256
    words = []
    for blk in blocks:  # (insertion order: the block numbers)
        for w in range(32):
            v = 0
            for k in range(8):
                v |= blk[8 * w + k] << (4 * k)
            words.append(v)
    size = len(index) + 4 * len(words)
    o = []
    o.append("/* unicode_case_classes.h -- written by tools/gen_unicode_case_classes.py; do not edit.")
    o.append(" *")
    o.append(" * The case classes of BPE_SPLIT_O200K (bpe_gpu.h) for every code point, from the `regex` module")
    o.append(f" * {regex.__version__}: 1 U \\p{{Lu}} \\p{{Lt}}, 2 l \\p{{Ll}}, 3 B \\p{{Lm}} \\p{{Lo}}, 4 M \\p{{M}}, 0 the rest; a code point of")
    o.append(" * class 0 carries 5 when it is \\p{N} and 6 when it is White_Space (unicode_classes.h's N and W).")
    o.append(" * Two stages: BPE_UCC_STAGE1[cp >> 8] names one of BPE_UCC_BLOCKS distinct blocks of 256 code points;")
    o.append(" * a block is 32 words, 4 bits per code point, code point cp in word (cp >> 3) & 31 at bits 4 * (cp & 7).")
    o.append(f" * {len(index)} + 4 * {len(words)} = {size} bytes.  Plain C: the host C and the HIP side include it")
    o.append(" * (BPE_UCC_STORAGE: the storage class of the two arrays, `static const` unless defined). */")
    o.append("#ifndef BPE_UNICODE_CASE_CLASSES_H")
    o.append("#define BPE_UNICODE_CASE_CLASSES_H")
    o.append("#include <stdint.h>")
    o.append("")
    o.append(f'#define BPE_UCC_SOURCE "regex {regex.__version__}"')
    o.append(f"#define BPE_UCC_DIGEST 0x{fnv1a64(case):016X}ull /* FNV-1a 64 of the 0x110000 case classes (0 .. 4) */")
    o.append(f"#define BPE_UCC_BLOCKS {len(blocks)}")
    o.append(f"#define BPE_UCC_TABLE_BYTES {size}")
    o.append("#ifndef BPE_UCC_STORAGE")
    o.append("#define BPE_UCC_STORAGE static const")
    o.append("#endif")
    o.append("")
    o.append(f"BPE_UCC_STORAGE uint8_t BPE_UCC_STAGE1[{len(index)}] = {{")
    for i in range(0, len(index), 32):
        o.append("    " + ",".join(str(v) for v in index[i:i + 32]) + ",")
    o.append("};")
    o.append("")
    o.append(f"BPE_UCC_STORAGE uint32_t BPE_UCC_STAGE2[{len(words)}] = {{")
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
        print("unicode_case_classes.h:", "up to date" if same else "differs")
        return 0 if same else 1
    with open(OUT, "w") as f:
        f.write(text)
    print(f"wrote {OUT} ({len(text)} bytes)")
    return 0


if __name__ == "__main__":
    sys.exit(main())

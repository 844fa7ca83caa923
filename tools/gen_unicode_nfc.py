#!/usr/bin/env python3
"""Write llmtokenizer_amd/csrc/unicode_nfc.h: the tables of BPE_NORM_NFC (bpe_gpu.h,
"Normalization"), asked of Python's `unicodedata`.

    python tools/gen_unicode_nfc.py            # writes the header
    python tools/gen_unicode_nfc.py --check    # exit 1 unless the header on disk is what would be written

Per code point one 32-bit record, in two stages (a block index per 256 code points, then the
distinct blocks; block 0 is the all-zero one):
    bit 31      work: ccc != 0, or NFC_Quick_Check is No or Maybe
    bits 16-23  ccc
    bits 13-15  the length of the full canonical decomposition (0: none), at most 4
    bits 0-12   its first entry in BPE_NFC_DECOMP
BPE_NFC_DECOMP holds the decompositions, expanded recursively and in canonical order, each
entry (ccc << 21 | code point).  BPE_NFC_PAIR_KEY / _VAL are the primary composites sorted by
(first << 21 | second): the exclusions are left out.  Hangul is in neither table: it is done
in code.  NFC_Quick_Check is derived: No when NFC(c) != c, Maybe when c is the second of a
listed pair or a Hangul V or T jamo.  The header records `unicodedata.unidata_version` and
the FNV-1a 64 digest of records, decompositions and pairs as little-endian 32-bit words.
Plain C only: the host C and the HIP side both include it.  Not run by any test.
"""
import argparse
import os
import struct
import sys
import unicodedata as ud

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "llmtokenizer_amd", "csrc", "unicode_nfc.h")
NCP = 0x110000
SBASE, SCOUNT = 0xAC00, 11172


def fnv1a64(data):
    h = 0xCBF29CE484222325
    for b in data:
        h = ((h ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


def tables():
    """(records[0x110000], decomp words, [(first, second, composite)] sorted)"""
    def hangul(c):
        return SBASE <= c < SBASE + SCOUNT

    def cps(c):
        return not 0xD800 <= c < 0xE000

    pairs = []
    for c in filter(cps, range(NCP)):
        d = ud.decomposition(chr(c))
        if not d or d.startswith("<") or hangul(c):
            continue
        raw = [int(x, 16) for x in d.split()]
        if len(raw) == 2 and ud.normalize("NFC", chr(raw[0]) + chr(raw[1])) == chr(c):
            pairs.append((raw[0], raw[1], c))
    pairs.sort()
    seconds = {b for _, b, _ in pairs}
    decomp, rec = [0], [0] * NCP  # (entry 0 is never named: a record's length says whether it has one)
    for c in filter(cps, range(NCP)):
        ch = chr(c)
        ccc = ud.combining(ch)
        maybe = c in seconds or 0x1161 <= c <= 0x1175 or 0x11A8 <= c <= 0x11C2
        work = ccc != 0 or maybe or ud.normalize("NFC", ch) != ch
        r = (work << 31) | (ccc << 16)
        full = ud.normalize("NFD", ch)
        if full != ch and not hangul(c):
            assert 1 <= len(full) <= 4 and len(decomp) < (1 << 13), (hex(c), full)
            r |= (len(full) << 13) | len(decomp)
            decomp += [(ud.combining(x) << 21) | ord(x) for x in full]
        rec[c] = r
    assert all(not rec[c] >> 31 for c in range(0x300)), "a flagged code point below U+0300"
    return rec, decomp, pairs


def render():
    rec, decomp, pairs = tables()
    blocks, index = {(0,) * 256: 0}, []
    for b in range(NCP >> 8):
        index.append(blocks.setdefault(tuple(rec[b << 8:(b + 1) << 8]), len(blocks)))
    assert len(blocks) <= 256 and len(pairs) < 1000
    words = [w for blk in blocks for w in blk]
    keys = [(a << 21) | b for a, b, _ in pairs]
    digest = fnv1a64(struct.pack(f"<{NCP}I", *rec) + struct.pack(f"<{len(decomp)}I", *decomp) +
                     struct.pack(f"<{3 * len(pairs)}I", *[x for p in pairs for x in p]))
    size = len(index) + 4 * len(words) + 4 * len(decomp) + 12 * len(pairs)
    o = []
    o.append("/* unicode_nfc.h -- written by tools/gen_unicode_nfc.py; do not edit.")
    o.append(" *")
    o.append(f" * The tables of BPE_NORM_NFC (bpe_gpu.h) from Python's unicodedata, Unicode {ud.unidata_version}.")
    o.append(" * BPE_NFC_STAGE1[cp >> 8] names one of BPE_NFC_BLOCKS blocks of 256 records (block 0: all zero);")
    o.append(" * a record is work << 31 | ccc << 16 | decomposition length << 13 | its first entry in BPE_NFC_DECOMP,")
    o.append(" * whose entries are ccc << 21 | code point.  BPE_NFC_PAIR_KEY (first << 21 | second, ascending) and")
    o.append(" * BPE_NFC_PAIR_VAL are the primary composites without the exclusions.  Hangul is done in code.")
    o.append(f" * {size} bytes.  Plain C: the host C and the HIP side include it (BPE_NFC_STORAGE: the storage")
    o.append(" * class of the arrays, `static const` unless defined). */")
    o.append("#ifndef BPE_UNICODE_NFC_H")
    o.append("#define BPE_UNICODE_NFC_H")
    o.append("#include <stdint.h>")
    o.append("")
    o.append(f'#define BPE_NFC_SOURCE "unicodedata {ud.unidata_version}"')
    o.append(f"#define BPE_NFC_DIGEST 0x{digest:016X}ull /* FNV-1a 64 of records, decompositions and pairs (LE words) */")
    o.append(f"#define BPE_NFC_BLOCKS {len(blocks)}")
    o.append(f"#define BPE_NFC_DECOMP_N {len(decomp)}")
    o.append(f"#define BPE_NFC_PAIRS {len(pairs)}")
    o.append(f"#define BPE_NFC_TABLE_BYTES {size}")
    o.append("#ifndef BPE_NFC_STORAGE")
    o.append("#define BPE_NFC_STORAGE static const")
    o.append("#endif")
    for decl, vals, fmt, per in (
            (f"uint8_t BPE_NFC_STAGE1[{len(index)}]", index, "{}", 32),
            (f"uint32_t BPE_NFC_STAGE2[{len(words)}]", words, "0x{:X}u", 12),
            (f"uint32_t BPE_NFC_DECOMP[{len(decomp)}]", decomp, "0x{:X}u", 12),
            (f"uint64_t BPE_NFC_PAIR_KEY[{len(keys)}]", keys, "0x{:X}ull", 8),
            (f"uint32_t BPE_NFC_PAIR_VAL[{len(pairs)}]", [c for _, _, c in pairs], "0x{:X}u", 12)):
        o.append("")
        o.append(f"BPE_NFC_STORAGE {decl} = {{")
        for i in range(0, len(vals), per):
            o.append("    " + ",".join(fmt.format(v) for v in vals[i:i + per]) + ",")
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
        print("unicode_nfc.h:", "up to date" if same else "differs")
        return 0 if same else 1
    with open(OUT, "w") as f:
        f.write(text)
    print(f"wrote {OUT} ({len(text)} bytes)")
    return 0


if __name__ == "__main__":
    sys.exit(main())

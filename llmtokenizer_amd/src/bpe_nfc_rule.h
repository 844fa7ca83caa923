/*
 * bpe_nfc_rule.h -- the steps of BPE_NORM_NFC (bpe_gpu.h, "Normalization") on one character or one buffer, in
 * plain C over the tables of csrc/unicode_nfc.h: decoding, the record of a code point, decomposition, canonical
 * ordering, composition, encoding.  The host definition (bpe_normalize.c) runs them over a whole text; the engine
 * (csrc/normalize.hip) runs the same statements over one segment per lane.  Not part of the API.
 *
 * A buffer entry is ccc << 21 | code point.  A byte in no well-formed sequence is the entry NFC_RAW + byte: ccc
 * 0, no record, no pair, and it encodes as that byte.
 */
#ifndef BPE_NFC_RULE_H
#define BPE_NFC_RULE_H

#include <stddef.h>
#include <stdint.h>

#include "../csrc/unicode_nfc.h"

#ifndef NFC_FN
#define NFC_FN static inline
#endif

#define NFC_RAW 0x110000u
#define NFC_CP(e) ((e) & 0x1FFFFFu)
#define NFC_CCC(e) ((e) >> 21)
enum { NFC_SBASE = 0xAC00, NFC_LBASE = 0x1100, NFC_VBASE = 0x1161, NFC_TBASE = 0x11A7, NFC_LCOUNT = 19,
       NFC_VCOUNT = 21, NFC_TCOUNT = 28, NFC_NCOUNT = 21 * 28, NFC_SCOUNT = 19 * 21 * 28 };

/* the character at b[p] (p < n): its length, and *e = its code point or NFC_RAW + b[p] (Unicode Table 3-7) */
NFC_FN uint32_t nfc_decode(const uint8_t *b, uint64_t n, uint64_t p, uint32_t *e) {
    const uint32_t b0 = b[p];
    *e = b0 < 0x80 ? b0 : NFC_RAW + b0;
    if (b0 < 0xC2 || b0 > 0xF4 || p + 1 >= n) return 1;
    const uint32_t b1 = b[p + 1];
    if (b0 < 0xE0) {
        if ((b1 & 0xC0) != 0x80) return 1;
        *e = (b0 & 0x1F) << 6 | (b1 & 0x3F);
        return 2;
    }
    const uint32_t lo = b0 == 0xE0 ? 0xA0 : b0 == 0xF0 ? 0x90 : 0x80;
    const uint32_t hi = b0 == 0xED ? 0x9F : b0 == 0xF4 ? 0x8F : 0xBF;
    if (b1 < lo || b1 > hi || p + 2 >= n || (b[p + 2] & 0xC0) != 0x80) return 1;
    if (b0 < 0xF0) {
        *e = (b0 & 0x0F) << 12 | (b1 & 0x3F) << 6 | (b[p + 2] & 0x3F);
        return 3;
    }
    if (p + 3 >= n || (b[p + 3] & 0xC0) != 0x80) return 1;
    *e = (b0 & 0x07) << 18 | (b1 & 0x3F) << 12 | (b[p + 2] & 0x3F) << 6 | (b[p + 3] & 0x3F);
    return 4;
}

/* the first byte of the character that holds b[p]: a lead byte never lies inside another sequence, so the
   sequences that begin at p - 1, p - 2 and p - 3 are judged each on its own */
NFC_FN uint64_t nfc_char_start(const uint8_t *b, uint64_t n, uint64_t p) {
    if ((b[p] & 0xC0) != 0x80) return p;
    for (uint32_t k = 1; k <= 3 && k <= p; k++) {
        uint32_t e;
        if (nfc_decode(b, n, p - k, &e) > k) return p - k;
    }
    return p;
}

NFC_FN uint32_t nfc_utf8_len(uint32_t e) {
    const uint32_t cp = NFC_CP(e);
    return cp < 0x80 || cp >= NFC_RAW ? 1 : cp < 0x800 ? 2 : cp < 0x10000 ? 3 : 4;
}

NFC_FN uint32_t nfc_encode(uint32_t e, uint8_t *out) {
    const uint32_t cp = NFC_CP(e);
    if (cp < 0x80 || cp >= NFC_RAW) { out[0] = (uint8_t)cp; return 1; }
    if (cp < 0x800) { out[0] = (uint8_t)(0xC0 | cp >> 6); out[1] = (uint8_t)(0x80 | (cp & 0x3F)); return 2; }
    if (cp < 0x10000) {
        out[0] = (uint8_t)(0xE0 | cp >> 12); out[1] = (uint8_t)(0x80 | ((cp >> 6) & 0x3F)); out[2] = (uint8_t)(0x80 | (cp & 0x3F));
        return 3;
    }
    out[0] = (uint8_t)(0xF0 | cp >> 18); out[1] = (uint8_t)(0x80 | ((cp >> 12) & 0x3F));
    out[2] = (uint8_t)(0x80 | ((cp >> 6) & 0x3F)); out[3] = (uint8_t)(0x80 | (cp & 0x3F));
    return 4;
}

/* the record of a code point (unicode_nfc.h); 0 for a raw byte */
NFC_FN uint32_t nfc_record(uint32_t cp) {
    if (cp >= NFC_RAW) return 0;
    const uint32_t blk = BPE_NFC_STAGE1[cp >> 8];
    return blk ? BPE_NFC_STAGE2[256u * blk + (cp & 255u)] : 0;
}
#define NFC_WORK(rec) ((rec) >> 31)

/* the full canonical decomposition of a character with record rec as entries: 1 to 4 of them */
NFC_FN uint32_t nfc_decompose(uint32_t cp, uint32_t rec, uint32_t out[4]) {
    if (cp - NFC_SBASE < NFC_SCOUNT) {
        const uint32_t s = cp - NFC_SBASE, t = s % NFC_TCOUNT;
        out[0] = NFC_LBASE + s / NFC_NCOUNT;
        out[1] = NFC_VBASE + (s % NFC_NCOUNT) / NFC_TCOUNT;
        out[2] = NFC_TBASE + t;
        return t ? 3 : 2;
    }
    const uint32_t len = (rec >> 13) & 7u;
    if (!len) { out[0] = ((rec >> 16) & 0xFFu) << 21 | cp; return 1; }
    for (uint32_t k = 0; k < len; k++) out[k] = BPE_NFC_DECOMP[(rec & 0x1FFFu) + k];
    return len;
}

/* the primary composite of two code points, or 0 */
NFC_FN uint32_t nfc_compose_pair(uint32_t a, uint32_t b) {
    if (a - NFC_LBASE < NFC_LCOUNT) return b - NFC_VBASE < NFC_VCOUNT ? NFC_SBASE + ((a - NFC_LBASE) * NFC_VCOUNT + (b - NFC_VBASE)) * NFC_TCOUNT : 0;
    if (a - NFC_SBASE < NFC_SCOUNT && (a - NFC_SBASE) % NFC_TCOUNT == 0) return b - (NFC_TBASE + 1) < NFC_TCOUNT - 1 ? a + (b - NFC_TBASE) : 0;
    const uint64_t key = (uint64_t)a << 21 | b;
    uint32_t lo = 0, hi = BPE_NFC_PAIRS;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (BPE_NFC_PAIR_KEY[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo < BPE_NFC_PAIRS && BPE_NFC_PAIR_KEY[lo] == key ? BPE_NFC_PAIR_VAL[lo] : 0;
}

/* canonical ordering of buf[0 .. n): a stable insertion sort of every run of entries with ccc != 0 */
NFC_FN void nfc_reorder(uint32_t *buf, size_t n) {
    for (size_t i = 1; i < n; i++) {
        const uint32_t e = buf[i];
        if (!NFC_CCC(e)) continue;
        size_t j = i;
        for (; j && NFC_CCC(buf[j - 1]) > NFC_CCC(e); j--) buf[j] = buf[j - 1];
        buf[j] = e;
    }
}

/* canonical composition of the ordered buf[0 .. n) in place; the new count.  A character composes with the last
   starter when nothing between them has ccc 0 or a ccc at least its own (UAX #15, D115: not blocked); `last` is the
   ccc of the entry kept last behind that starter, -1 when there is none. */
NFC_FN size_t nfc_compose(uint32_t *buf, size_t n) {
    size_t out = 0, sp = (size_t)-1;
    int last = -1;
    for (size_t i = 0; i < n; i++) {
        const uint32_t e = buf[i];
        const int cc = (int)NFC_CCC(e);
        if (sp != (size_t)-1 && last < cc) {
            const uint32_t c = nfc_compose_pair(NFC_CP(buf[sp]), NFC_CP(e));
            if (c) { buf[sp] = c; continue; }  /* (a composite of a starter has ccc 0) */
        }
        if (!cc) sp = out, last = -1; else last = cc;
        buf[out++] = e;
    }
    return out;
}

#endif

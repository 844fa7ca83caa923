/*
 * bpe_utf8_rule.h -- the fate of one decoded byte under BPE_TEXT_REPLACE and BPE_TEXT_HOLD (bpe_gpu.h, "Decoded
 * text"), in plain C.  The host definition (bpe_utf8.c) runs it over a whole text from the left; the engine
 * (csrc/utf8.hip) runs the same statements on the bytes of one lane.  Not part of the API.
 *
 * Every function reads b[i - 3 .. i + 3] at most, and only inside the text [lo, hi): a lead byte looks ahead for
 * its continuation bytes, a continuation byte looks back for the lead that covers it, and that is all the context
 * there is (Unicode Table 3-7: a lead byte is never a continuation byte, so no sequence begins inside another).
 */
#ifndef BPE_UTF8_RULE_H
#define BPE_UTF8_RULE_H

#include <stddef.h>
#include <stdint.h>

#ifndef U8_FN
#define U8_FN static inline
#endif

enum { U8_RAW = 0, U8_REPLACE = 1, U8_HOLD = 2 };  /* bpe_gpu.h BPE_TEXT_* */

/* the bytes a sequence with the lead c has: 2, 3 or 4, and 0 when c is no lead (below C2, above F4) */
U8_FN uint32_t u8_need(uint32_t c) { return c < 0xC2 || c > 0xF4 ? 0 : c < 0xE0 ? 2 : c < 0xF0 ? 3 : 4; }

/* may c follow the lead directly?  (Table 3-7's second column: E0, ED, F0 and F4 narrow it) */
U8_FN int u8_second(uint32_t lead, uint32_t c) {
    const uint32_t lo = lead == 0xE0 ? 0xA0 : lead == 0xF0 ? 0x90 : 0x80;
    const uint32_t hi = lead == 0xED ? 0x9F : lead == 0xF4 ? 0x8F : 0xBF;
    return c >= lo && c <= hi;
}

/* the bytes of the sequence of the lead b[i] (need > 0 of them asked for) that are valid and lie below hi: 1 ..
   need.  need: complete; fewer: a maximal subpart, ended by the byte b[i + it] or by the text. */
U8_FN uint32_t u8_prefix(const uint8_t *b, uint64_t i, uint64_t hi, uint32_t need) {
    if (i + 1 >= hi || !u8_second(b[i], b[i + 1])) return 1;
    uint32_t k = 2;
    while (k < need && i + k < hi && (b[i + k] & 0xC0) == 0x80) k++;
    return k;
}

/* Is the continuation byte b[i] part of a lead's sequence or maximal subpart?  The nearest byte before it in the
   text that is no continuation byte, at most 3 back, must be a lead whose valid bytes reach i; the bytes between
   are continuation bytes, so only the lead's second byte and its length decide. */
U8_FN int u8_covered(const uint8_t *b, uint64_t i, uint64_t lo) {
    for (uint32_t k = 1; k <= 3 && i >= lo + k; k++) {
        const uint32_t c = b[i - k];
        if ((c & 0xC0) == 0x80) continue;
        return k < u8_need(c) && u8_second(c, b[i - k + 1]);
    }
    return 0;
}

/* CPython's one exception under U8_HOLD: is b[i] the ED of a text that ends ED A0..BF, a truncated surrogate?  Its
   incremental decoder keeps those two bytes back (for errors="surrogatepass"), though no well-formed sequence begins
   with them; the next step's bytes then see both replaced. */
U8_FN int u8_cut_surrogate(const uint8_t *b, uint64_t i, uint64_t hi) {
    return i + 2 == hi && b[i] == 0xED && b[i + 1] >= 0xA0 && b[i + 1] <= 0xBF;
}

/* The output bytes the byte b[i] of the text [lo, hi) stands for, written to out unless out == NULL: 1 for an ASCII
   byte, the whole sequence for the lead of a complete one, 3 (EF BF BD) for a lead whose sequence is cut short
   and for a byte in no sequence, 0 for a continuation byte that a lead accounts for and, under U8_HOLD, for the
   lead of a subpart that only the text's end cut short (and the two bytes of u8_cut_surrogate). */
U8_FN uint32_t u8_byte(const uint8_t *b, uint64_t i, uint64_t lo, uint64_t hi, int errors, uint8_t *out) {
    const uint32_t c = b[i];
    if (c < 0x80) {
        if (out) out[0] = (uint8_t)c;
        return 1;
    }
    const uint32_t need = u8_need(c);
    if (need) {
        const uint32_t got = u8_prefix(b, i, hi, need);
        if (got == need) {
            if (out)
                for (uint32_t k = 0; k < need; k++) out[k] = b[i + k];
            return need;
        }
        if (errors == U8_HOLD && (i + got == hi || u8_cut_surrogate(b, i, hi))) return 0;
    } else if ((c & 0xC0) == 0x80 &&
               (u8_covered(b, i, lo) || (errors == U8_HOLD && i > lo && i + 1 == hi && u8_cut_surrogate(b, i - 1, hi)))) {
        return 0;
    }
    if (out) out[0] = 0xEF, out[1] = 0xBF, out[2] = 0xBD;
    return 3;
}

/* the bytes at the end of the text [lo, hi) that U8_HOLD keeps back: 1 .. 3 when they are a proper prefix of a
   well-formed sequence (or u8_cut_surrogate's two), else 0 */
U8_FN uint32_t u8_held(const uint8_t *b, uint64_t lo, uint64_t hi) {
    for (uint32_t k = 1; k <= 3 && hi >= lo + k; k++) {
        const uint32_t c = b[hi - k];
        if ((c & 0xC0) == 0x80) continue;
        const uint32_t need = u8_need(c);
        return (need > k && u8_prefix(b, hi - k, hi, need) == k) || u8_cut_surrogate(b, hi - k, hi) ? k : 0;
    }
    return 0;
}

#endif

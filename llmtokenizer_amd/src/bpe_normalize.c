/*
 * bpe_normalize.c -- BPE_NORM_NFC (bpe_gpu.h, "Normalization") in plain C, no GPU: the definition the device is
 * held to (bpe_ex.h bpe_nfc_host, bpe_nfc_info).  One pass from the left over the steps of bpe_nfc_rule.h: the
 * text is cut at every character whose work flag is clear; a stretch with no flagged character is copied, any
 * other is decomposed into a buffer that grows with it, ordered, composed and encoded.
 */
#include <stdlib.h>
#include <string.h>

#include "../../include/bpe_ex.h"
#include "bpe_nfc_rule.h"

int bpe_nfc_info(const char **source, uint64_t *digest) {
    if (source) *source = BPE_NFC_SOURCE;
    if (digest) *digest = BPE_NFC_DIGEST;
    return 0;
}

int bpe_nfc_host(const uint8_t *bytes, size_t n, uint8_t *out, size_t cap, size_t *out_len) {
    if ((!bytes && n) || !out_len || (!out && cap)) return -1;
    uint32_t *buf = NULL;
    size_t buf_cap = 0, len = 0, p = 0;
    while (p < n) {
        /* the segment [p, q): the character at p, which is a boundary or the text's first, and every flagged
           character behind it */
        uint32_t e, d[4];
        size_t q = p + nfc_decode(bytes, n, p, &e), cnt = 0;
        int dirty = p == 0 && NFC_WORK(nfc_record(e));
        while (q < n) {
            const uint32_t l = nfc_decode(bytes, n, q, &e);
            if (!NFC_WORK(nfc_record(e))) break;
            dirty = 1;
            q += l;
        }
        if (!dirty) {
            if (len + (q - p) <= cap) memcpy(out + len, bytes + p, q - p);
            len += q - p;
            p = q;
            continue;
        }
        for (size_t i = p; i < q;) {
            i += nfc_decode(bytes, n, i, &e);
            if (cnt + 4 > buf_cap) {
                buf_cap = buf_cap ? 2 * buf_cap : 64;
                uint32_t *nb = (uint32_t *)realloc(buf, buf_cap * sizeof *buf);
                if (!nb) { free(buf); return -3; }
                buf = nb;
            }
            const uint32_t k = nfc_decompose(e, nfc_record(e), d);
            memcpy(buf + cnt, d, k * sizeof *d);
            cnt += k;
        }
        nfc_reorder(buf, cnt);
        cnt = nfc_compose(buf, cnt);
        for (size_t i = 0; i < cnt; i++) {
            uint8_t u[4];
            const uint32_t l = nfc_encode(buf[i], u);
            if (len + l <= cap) memcpy(out + len, u, l);
            len += l;
        }
        p = q;
    }
    free(buf);
    *out_len = len;
    return 0;
}

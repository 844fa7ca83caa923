/*
 * bpe_spans.c -- token spans on the host, in plain C and without a GPU (bpe_ex.h):
 * bpe_span_lens (the byte length of every token id: a byte 1, NUL included, merge r
 * the sum of its halves, special j its length; by internal id or, with a vocabulary,
 * scattered to the vocabulary's ids through bpe_vocab_tables' forward table, a hole 0)
 * and bpe_token_spans_host (the spans of ids per text in bytes or characters, in plain
 * loops: the written definition bpe_gpu_token_spans is held to).  The engine uploads
 * what the first builds.
 */
#include "../../include/bpe_ex.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static int refuse(int code, char *msg, size_t cap, const char *text)
{
    if (msg && cap) snprintf(msg, cap, "spans: %s", text);
    return code;
}

int bpe_span_lens(const uint32_t *pairs, size_t n_merges, const bpe_gpu_specials *specials, const bpe_gpu_vocab *vocab,
                  uint32_t *out, size_t cap, size_t *count, char *msg, size_t msg_cap)
{
    char text[200];
    if (msg && msg_cap) msg[0] = '\0';
    if (!count || (!pairs && n_merges)) return refuse(BPE_GPU_EINVAL, msg, msg_cap, "a missing argument");
    const size_t S = specials ? specials->count : 0;
    if (S > BPE_GPU_SPECIAL_MAX_COUNT || (S && !specials->len)) return refuse(BPE_GPU_EINVAL, msg, msg_cap, "a bad set of specials");
    if (n_merges > 0xFFFFFEFFull - BPE_GPU_SPECIAL_MAX_COUNT) return refuse(BPE_GPU_ERANGE, msg, msg_cap, "merge list too long");
    if (vocab && (vocab->n_merges != n_merges || vocab->n_specials != S)) {
        snprintf(text, sizeof text, "the vocabulary numbers %zu merges and %zu specials, the lists hold %zu and %zu",
                 vocab->n_merges, vocab->n_specials, n_merges, S);
        return refuse(BPE_GPU_EINVAL, msg, msg_cap, text);
    }
    const size_t total = 256 + n_merges + S;
    uint32_t *len = malloc(total * sizeof *len), *fwd = NULL;
    if (!len) return refuse(BPE_GPU_ENOMEM, msg, msg_cap, "out of memory");
    for (size_t b = 0; b < 256; b++) len[b] = 1;
    for (size_t r = 0; r < n_merges; r++) {
        const uint32_t a = pairs[2 * r], b = pairs[2 * r + 1];
        if (a >= 256 + r || b >= 256 + r) {
            snprintf(text, sizeof text, "merge %zu names the id %u, which is not below its own id %zu", r,
                     a >= 256 + r ? a : b, 256 + r);
            free(len);
            return refuse(BPE_GPU_EINVAL, msg, msg_cap, text);
        }
        const uint64_t sum = (uint64_t)len[a] + len[b];
        if (sum > 0xFFFFFFFFull) {
            snprintf(text, sizeof text, "merge %zu makes a token of %llu bytes, more than 2^32 - 1", r, (unsigned long long)sum);
            free(len);
            return refuse(BPE_GPU_ERANGE, msg, msg_cap, text);
        }
        len[256 + r] = (uint32_t)sum;
    }
    for (size_t j = 0; j < S; j++) len[256 + n_merges + j] = specials->len[j];
    int rc = 0;
    if (!vocab) {
        *count = total;
        if (out) memcpy(out, len, (total < cap ? total : cap) * sizeof *len);
    } else {
        size_t nf = 0, ni = 0;
        fwd = malloc(total * sizeof *fwd);
        if (!fwd) rc = refuse(BPE_GPU_ENOMEM, msg, msg_cap, "out of memory");
        else if ((rc = bpe_vocab_tables(vocab, fwd, total, NULL, 0, &nf, &ni))) refuse(rc, msg, msg_cap, "a vocabulary bpe_vocab_check refuses");
        else {
            *count = ni;
            if (out) {
                const size_t n = ni < cap ? ni : cap;
                memset(out, 0, n * sizeof *out);
                for (size_t k = 0; k < total; k++)
                    if (fwd[k] < n) out[fwd[k]] = len[k];
            }
        }
    }
    free(fwd);
    free(len);
    return rc;
}

/* off[0 .. T] runs from 0 to n without falling */
static int offsets_ok(const uint64_t *off, size_t T, uint64_t n)
{
    if (!off || off[0] != 0 || off[T] != n) return 0;
    for (size_t k = 0; k < T; k++)
        if (off[k] > off[k + 1]) return 0;
    return 1;
}

static inline unsigned is_lead(uint8_t b) { return (b & 0xC0u) != 0x80u; }

int bpe_token_spans_host(const uint32_t *ids, size_t n_ids, const uint64_t *text_off, size_t T, const uint8_t *bytes,
                         size_t n, const uint64_t *byte_off, const uint32_t *lens, size_t n_lens, int unit, uint32_t *out,
                         char *msg, size_t msg_cap)
{
    char text[200];
    if (msg && msg_cap) msg[0] = '\0';
    if ((!ids && n_ids) || (!lens && n_lens) || (!out && n_ids) || (unit != BPE_SPAN_BYTE && unit != BPE_SPAN_CHAR) ||
        (unit == BPE_SPAN_CHAR && !bytes && n))
        return refuse(BPE_GPU_EINVAL, msg, msg_cap, "a missing argument or an unknown unit");
    if (!offsets_ok(text_off, T, n_ids)) return refuse(BPE_GPU_EINVAL, msg, msg_cap, "the id offsets do not run from 0 to the id count without falling");
    if (!offsets_ok(byte_off, T, n)) return refuse(BPE_GPU_EINVAL, msg, msg_cap, "the byte offsets do not run from 0 to the byte count without falling");
    for (size_t k = 0; k < T; k++) {
        const uint64_t i0 = text_off[k], i1 = text_off[k + 1], L = byte_off[k + 1] - byte_off[k];
        if (L > 0xFFFFFFFFull) {
            snprintf(text, sizeof text, "text %zu holds %llu bytes, more than a span can say", k, (unsigned long long)L);
            return refuse(BPE_GPU_ERANGE, msg, msg_cap, text);
        }
        /* first the sum, so that the walk below stays inside the text */
        uint64_t sum = 0;
        for (uint64_t i = i0; i < i1; i++) {
            if (ids[i] >= n_lens || lens[ids[i]] == 0) {
                snprintf(text, sizeof text, "unknown token id %u at index %llu (text %zu)", ids[i], (unsigned long long)i, k);
                return refuse(BPE_GPU_EDATA, msg, msg_cap, text);
            }
            sum += lens[ids[i]];
        }
        if (sum != L) {
            snprintf(text, sizeof text, "the ids of text %zu have lengths that sum to %llu, the text holds %llu bytes", k,
                     (unsigned long long)sum, (unsigned long long)L);
            return refuse(BPE_GPU_EDATA, msg, msg_cap, text);
        }
        const uint8_t *t = bytes ? bytes + byte_off[k] : NULL;
        uint64_t p = 0, q = 0, lead = 0; /* lead = non-continuation bytes in t[0 .. q) */
        for (uint64_t i = i0; i < i1; i++) {
            const uint64_t bs = p, be = p + lens[ids[i]];
            if (unit == BPE_SPAN_BYTE) {
                out[2 * i] = (uint32_t)bs;
                out[2 * i + 1] = (uint32_t)be;
            } else {
                for (; q < bs + 1; q++) lead += is_lead(t[q]);
                out[2 * i] = (uint32_t)((lead > 1 ? lead : 1) - 1);
                for (; q < be; q++) lead += is_lead(t[q]);
                out[2 * i + 1] = (uint32_t)lead;
            }
            p = be;
        }
    }
    return 0;
}

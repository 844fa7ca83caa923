/*
 * bpe_texts.c -- a batch of texts on the host, in plain C and without a GPU
 * (bpe_ex.h): bpe_texts_check (the byte offsets of the texts: the first 0, rising,
 * the last n, and n + T positions within the engine's limit; the message names the
 * offending index), bpe_texts_gap (the bytes as the engine keeps them: every
 * text followed by one gap byte 0x00) and bpe_texts_gap_range (any stretch of
 * them).  bpe_gpu_load_texts checks with the first and uploads what the last
 * builds, chunk by chunk.
 */
#include "../../include/bpe_ex.h"

#include <stdio.h>
#include <string.h>

static int refuse(char *msg, size_t cap, const char *text)
{
    if (msg && cap) snprintf(msg, cap, "texts: %s", text);
    return BPE_GPU_EINVAL;
}

int bpe_texts_check(const uint64_t *text_off, size_t T, size_t n, char *msg, size_t cap)
{
    char text[200];
    if (msg && cap) msg[0] = '\0';
    if (!text_off) return refuse(msg, cap, "no offsets given");
    if (T > BPE_TEXTS_MAX_POSITIONS || n > BPE_TEXTS_MAX_POSITIONS - T) {
        snprintf(text, sizeof text, "%zu bytes and %zu gap bytes (one per text) are more than the %llu positions a context holds",
                 n, T, (unsigned long long)BPE_TEXTS_MAX_POSITIONS);
        return refuse(msg, cap, text);
    }
    if (text_off[0] != 0) {
        snprintf(text, sizeof text, "offset 0 is %llu, not 0", (unsigned long long)text_off[0]);
        return refuse(msg, cap, text);
    }
    for (size_t k = 0; k < T; k++)
        if (text_off[k + 1] < text_off[k]) {
            snprintf(text, sizeof text, "offset %zu (%llu) is below offset %zu (%llu)", k + 1,
                     (unsigned long long)text_off[k + 1], k, (unsigned long long)text_off[k]);
            return refuse(msg, cap, text);
        }
    if (text_off[T] != n) {
        snprintf(text, sizeof text, "offset %zu, the last, is %llu, not the number of bytes %zu", T,
                 (unsigned long long)text_off[T], n);
        return refuse(msg, cap, text);
    }
    return 0;
}

int bpe_texts_gap_range(const uint8_t *bytes, size_t n, const uint64_t *text_off, size_t T, size_t lo, size_t hi,
                        uint8_t *out)
{
    if (!text_off || (!bytes && n) || lo > hi || hi > n + T || (!out && hi > lo)) return BPE_GPU_EINVAL;
    if (lo == hi) return 0;
    /* the first text whose gap, at text_off[k + 1] + k, is at or past lo: it holds position lo */
    size_t a = 0, b = T;
    while (a < b) {
        const size_t mid = a + (b - a) / 2;
        if (text_off[mid + 1] + mid < lo) a = mid + 1;
        else b = mid;
    }
    size_t k = a, p = lo;
    while (p < hi) {
        const size_t gap = (size_t)text_off[k + 1] + k; /* (k < T: position hi - 1 <= the last gap) */
        if (p < gap) {
            const size_t len = (gap < hi ? gap : hi) - p;
            memcpy(out + (p - lo), bytes + (p - k), len); /* resident p of text k is byte p - k of the join */
            p += len;
        }
        if (p == gap && p < hi) {
            out[p++ - lo] = 0;
            k++;
        }
    }
    return 0;
}

int bpe_texts_gap(const uint8_t *bytes, size_t n, const uint64_t *text_off, size_t T, uint8_t *out, size_t out_cap)
{
    if (bpe_texts_check(text_off, T, n, NULL, 0) || out_cap < n + T) return BPE_GPU_EINVAL;
    return bpe_texts_gap_range(bytes, n, text_off, T, 0, n + T, out);
}

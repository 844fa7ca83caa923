/*
 * bpe_vocab.c -- a vocabulary's numbering on the host, in plain C and without a
 * GPU (bpe_ex.h): bpe_vocab_check (the ids pairwise distinct and below 2^24, every
 * merge made of earlier ids, the counts in agreement; the message names the
 * offender) and bpe_vocab_tables (the forward table internal id -> vocabulary id
 * and its inverse with 0xFFFFFFFF for a hole).  The engine checks with the first
 * and uploads what the second builds (bpe_gpu_map_ids, bpe_gpu_decode_docs_vocab);
 * the entry points that drive the engine are in bpe_vocab_gpu.c.
 */
#include "../../include/bpe_ex.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

/* "byte 0x21", "merge 17" or "special 1" for entry k of the three arrays in order */
static void name_of(size_t k, size_t n_merges, char *out, size_t cap)
{
    if (k < 256) snprintf(out, cap, "byte 0x%02zx", k);
    else if (k < 256 + n_merges) snprintf(out, cap, "merge %zu", k - 256);
    else snprintf(out, cap, "special %zu", k - 256 - n_merges);
}

static uint32_t id_of(const bpe_gpu_vocab *v, size_t k)
{
    if (k < 256) return v->byte_id[k];
    if (k < 256 + v->n_merges) return v->merge_id[k - 256];
    return v->special_id[k - 256 - v->n_merges];
}

static int refuse(char *msg, size_t cap, const char *text)
{
    if (msg && cap) snprintf(msg, cap, "vocabulary: %s", text);
    return BPE_GPU_EINVAL;
}

int bpe_vocab_check(const bpe_gpu_vocab *v, const uint32_t *pairs, size_t n_merges, char *msg, size_t cap)
{
    char a[48], b[48], text[200];
    if (msg && cap) msg[0] = '\0';
    if (!v) return refuse(msg, cap, "none given");
    if (!v->byte_id || (v->n_merges && !v->merge_id) || (v->n_specials && !v->special_id))
        return refuse(msg, cap, "an id array is missing");
    if (v->n_merges != n_merges) {
        snprintf(text, sizeof text, "it numbers %zu merges, the merge list holds %zu", v->n_merges, n_merges);
        return refuse(msg, cap, text);
    }
    if (v->n_specials > BPE_GPU_SPECIAL_MAX_COUNT) {
        snprintf(text, sizeof text, "%zu specials, at most %d", v->n_specials, BPE_GPU_SPECIAL_MAX_COUNT);
        return refuse(msg, cap, text);
    }
    if (v->n_merges > BPE_VOCAB_ID_LIMIT - 256) {
        snprintf(text, sizeof text, "%zu merges, more than there are ids below 2^24", v->n_merges);
        return refuse(msg, cap, text);
    }
    const size_t total = 256 + v->n_merges + v->n_specials;
    for (size_t k = 0; k < total; k++)
        if (id_of(v, k) >= BPE_VOCAB_ID_LIMIT) {
            name_of(k, v->n_merges, a, sizeof a);
            snprintf(text, sizeof text, "%s has the id %u, at or above 2^24", a, id_of(v, k));
            return refuse(msg, cap, text);
        }
    /* a bit per possible id (2 MB) */
    uint8_t *seen = calloc(BPE_VOCAB_ID_LIMIT / 8, 1);
    if (!seen) return BPE_GPU_ENOMEM;
    for (size_t k = 0; k < total; k++) {
        const uint32_t id = id_of(v, k);
        if (seen[id >> 3] & (1u << (id & 7u))) {
            size_t first = 0;
            while (id_of(v, first) != id) first++;
            free(seen);
            name_of(first, v->n_merges, a, sizeof a);
            name_of(k, v->n_merges, b, sizeof b);
            snprintf(text, sizeof text, "%s and %s share the id %u", a, b, id);
            return refuse(msg, cap, text);
        }
        seen[id >> 3] |= (uint8_t)(1u << (id & 7u));
    }
    free(seen);
    if (pairs)
        for (size_t r = 0; r < n_merges; r++)
            for (int h = 0; h < 2; h++)
                if (pairs[2 * r + h] >= 256 + r) {
                    snprintf(text, sizeof text,
                             "merge %zu names the id %u as its %s part, which is not below its own id %zu", r,
                             pairs[2 * r + h], h ? "second" : "first", 256 + r);
                    return refuse(msg, cap, text);
                }
    return 0;
}

int bpe_vocab_tables(const bpe_gpu_vocab *v, uint32_t *fwd, size_t fwd_cap, uint32_t *inv, size_t inv_cap, size_t *n_fwd,
                     size_t *n_inv)
{
    if (!v || !n_fwd || !n_inv) return BPE_GPU_EINVAL;
    const int rc = bpe_vocab_check(v, NULL, v->n_merges, NULL, 0);
    if (rc) return rc;
    const size_t total = 256 + v->n_merges + v->n_specials;
    uint32_t top = 0;
    for (size_t k = 0; k < total; k++)
        if (id_of(v, k) > top) top = id_of(v, k);
    *n_fwd = total;
    *n_inv = (size_t)top + 1;
    if (fwd)
        for (size_t k = 0; k < total && k < fwd_cap; k++) fwd[k] = id_of(v, k);
    if (inv) {
        const size_t n = *n_inv < inv_cap ? *n_inv : inv_cap;
        memset(inv, 0xFF, n * sizeof(uint32_t));
        for (size_t k = 0; k < total; k++)
            if (id_of(v, k) < n) inv[id_of(v, k)] = (uint32_t)k;
    }
    return 0;
}

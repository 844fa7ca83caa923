/*
 * bpe_vocab_gpu.c -- the vocabulary entry points of bpe_ex.h over the engine:
 * bpe_encode_split_vocab is bpe_encode_split_special with bpe_gpu_map_ids between
 * the encode and the fetch, bpe_decode_docs_vocab is bpe_decode_docs_special over
 * bpe_gpu_decode_docs_vocab.  Each loads, does one thing and returns malloc'd
 * results, like the _special pair in bpe_special_gpu.c.
 */
#include "bpe_internal.h"

#include <stdio.h>
#include <stdlib.h>

uint32_t *bpe_encode_split_vocab(const uint8_t *bytes, size_t n, int preset, const uint8_t *cls, const uint16_t *brk,
                                 const bpe_gpu_specials *specials, dyn_arr_t *pair_arr, const bpe_gpu_vocab *vocab,
                                 int device, size_t *len, uint64_t **id_off, uint64_t **byte_off, size_t *ndocs)
{
    if ((!bytes && n) || !pair_arr || !vocab || !len || !id_off || !ndocs) return NULL;
    bpe_gpu_ctx *ctx = NULL;
    size_t k = 0, n_ids = 0, n_off = 0, pieces = 0;
    uint32_t *pairs = arr_to_pairs(pair_arr, &k), *ids = NULL;
    uint64_t *offs = NULL, *boffs = NULL;
    char msg[400];
    int rc, ok = 0;
    if (!pairs) return NULL;
    if ((rc = bpe_vocab_check(vocab, pairs, k, msg, sizeof msg))) {
        fprintf(stderr, "bpe: %s\n", msg);
        goto done;
    }
    if ((specials ? specials->count : 0) != vocab->n_specials) {
        fprintf(stderr, "bpe: the vocabulary numbers %zu specials, %zu are given\n", vocab->n_specials,
                specials ? specials->count : (size_t)0);
        goto done;
    }
    if ((rc = open_engine(device, &ctx))) goto done;
    if ((rc = bpe_gpu_load(ctx, bytes, n))) { report("load", rc); goto done; }
    if ((rc = bpe_gpu_split_special(ctx, preset, cls, brk, specials, &pieces))) { report("split", rc); goto done; }
    if ((rc = bpe_gpu_encode_split(ctx, pairs, k))) { report("encode split", rc); goto done; }
    if ((rc = bpe_gpu_map_ids(ctx, vocab))) { report("map ids", rc); goto done; }
    if ((rc = bpe_gpu_fetch_ids(ctx, NULL, 0, &n_ids))) { report("fetch ids", rc); goto done; }
    ids = alloc_ids(n_ids);
    offs = malloc((pieces + 1) * sizeof(uint64_t));
    if (byte_off) boffs = malloc((pieces + 1) * sizeof(uint64_t));
    if (!ids || !offs || (byte_off && !boffs)) goto done;
    if ((rc = bpe_gpu_fetch_ids(ctx, ids, n_ids, &n_ids))) { report("fetch ids", rc); goto done; }
    if ((rc = bpe_gpu_fetch_doc_offsets(ctx, offs, pieces + 1, &n_off))) { report("fetch doc offsets", rc); goto done; }
    if (boffs && (rc = bpe_gpu_fetch_split_offsets(ctx, boffs, pieces + 1, &n_off))) {
        report("fetch split offsets", rc);
        goto done;
    }
    bpe_gpu_get_stats(ctx, &g_last_stats);
    ok = 1;
done:
    close_engine(device, ctx, ok);
    free(pairs);
    if (!ok) {
        free(ids);
        free(offs);
        free(boffs);
        return NULL;
    }
    *len = n_ids;
    *id_off = offs;
    if (byte_off) *byte_off = boffs;
    *ndocs = pieces;
    return ids;
}

char *bpe_decode_docs_vocab(const uint32_t *ids, size_t len, const uint64_t *id_off, size_t ndocs, dyn_arr_t *pair_arr,
                            const bpe_gpu_specials *specials, const bpe_gpu_vocab *vocab, int device, size_t *out_len,
                            uint64_t **byte_off)
{
    if ((!ids && len) || !pair_arr || !vocab || !out_len) return NULL;
    if (!id_off && ndocs) return NULL; /* (no offsets: the ids as one flat sequence, no *byte_off) */
    if (id_off && !byte_off) return NULL;
    if (!id_off) byte_off = NULL;
    bpe_gpu_ctx *ctx = NULL;
    size_t k = 0, total = 0;
    uint32_t *pairs = arr_to_pairs(pair_arr, &k);
    uint64_t *offs = NULL;
    char *out = NULL;
    int rc, ok = 0;
    if (!pairs) return NULL;
    if ((rc = open_engine(device, &ctx))) goto done;
    if ((rc = bpe_gpu_decode_docs_vocab(ctx, ids, len, id_off, ndocs, pairs, k, specials, vocab, NULL, 0, &total, NULL))) {
        report("decode docs", rc);
        goto done;
    }
    out = malloc(total + 1);
    if (byte_off) offs = malloc((ndocs + 1) * sizeof(uint64_t));
    if (!out || (byte_off && !offs)) goto done;
    if ((rc = bpe_gpu_decode_docs_vocab(ctx, ids, len, id_off, ndocs, pairs, k, specials, vocab, (uint8_t *)out, total,
                                        &total, offs))) {
        report("decode docs", rc);
        goto done;
    }
    out[total] = '\0';
    ok = 1;
done:
    close_engine(device, ctx, ok);
    free(pairs);
    if (!ok) {
        free(out);
        free(offs);
        return NULL;
    }
    *out_len = total;
    if (byte_off) *byte_off = offs;
    return out;
}

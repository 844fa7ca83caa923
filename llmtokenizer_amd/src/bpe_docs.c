/*
 * bpe_docs.c -- document batches of bpe_ex.h: bpe_encode_docs / bpe_decode_docs
 * over the engine's bpe_gpu_encode_docs / bpe_gpu_decode_docs, and
 * bpe_encode_split over bpe_gpu_split / bpe_gpu_encode_split, on the cached
 * engine contexts of bpe.c.  encode_split_with is its body with the split step
 * passed in: bpe_split_preset.c runs it over bpe_gpu_split_preset.
 */
#include "bpe_internal.h"

#include <stdlib.h>

uint32_t *bpe_encode_docs(const uint8_t *bytes, size_t n, const uint64_t *doc_off, size_t ndocs, dyn_arr_t *pair_arr,
                          int device, size_t *len, uint64_t **id_off)
{
    if ((!bytes && n) || !doc_off || !pair_arr || !len || !id_off) return NULL;
    bpe_gpu_ctx *ctx = NULL;
    size_t k = 0, n_ids = 0, n_off = 0;
    uint32_t *pairs = arr_to_pairs(pair_arr, &k), *ids = NULL;
    uint64_t *offs = NULL;
    int rc, ok = 0;
    if (!pairs) return NULL;
    if ((rc = open_engine(device, &ctx))) goto done;
    if ((rc = bpe_gpu_load(ctx, bytes, n))) { report("load", rc); goto done; }
    if ((rc = bpe_gpu_encode_docs(ctx, doc_off, ndocs, pairs, k))) { report("encode docs", rc); goto done; }
    if ((rc = bpe_gpu_fetch_ids(ctx, NULL, 0, &n_ids))) { report("fetch ids", rc); goto done; }
    ids = alloc_ids(n_ids);
    offs = malloc((ndocs + 1) * sizeof(uint64_t));
    if (!ids || !offs) goto done;
    if ((rc = bpe_gpu_fetch_ids(ctx, ids, n_ids, &n_ids))) { report("fetch ids", rc); goto done; }
    if ((rc = bpe_gpu_fetch_doc_offsets(ctx, offs, ndocs + 1, &n_off))) { report("fetch doc offsets", rc); goto done; }
    bpe_gpu_get_stats(ctx, &g_last_stats);
    ok = 1;
done:
    close_engine(device, ctx, ok);
    free(pairs);
    if (!ok) {
        free(ids);
        free(offs);
        return NULL;
    }
    *len = n_ids;
    *id_off = offs;
    return ids;
}

uint32_t *bpe_encode_split(const uint8_t *bytes, size_t n, const uint8_t *cls, const uint16_t *brk, dyn_arr_t *pair_arr,
                           int device, size_t *len, uint64_t **id_off, uint64_t **byte_off, size_t *ndocs)
{
    if (!cls || !brk) return NULL;
    const struct split_tables t = {cls, brk};
    return encode_split_with(bytes, n, split_tables, &t, pair_arr, device, len, id_off, byte_off, ndocs);
}

uint32_t *encode_split_with(const uint8_t *bytes, size_t n, bpe_split_fn split, const void *rule, dyn_arr_t *pair_arr,
                            int device, size_t *len, uint64_t **id_off, uint64_t **byte_off, size_t *ndocs)
{
    if ((!bytes && n) || !pair_arr || !len || !id_off || !ndocs) return NULL;
    bpe_gpu_ctx *ctx = NULL;
    size_t k = 0, n_ids = 0, n_off = 0, pieces = 0;
    uint32_t *pairs = arr_to_pairs(pair_arr, &k), *ids = NULL;
    uint64_t *offs = NULL, *boffs = NULL;
    int rc, ok = 0;
    if (!pairs) return NULL;
    if ((rc = open_engine(device, &ctx))) goto done;
    if ((rc = bpe_gpu_load(ctx, bytes, n))) { report("load", rc); goto done; }
    if ((rc = split(ctx, rule, &pieces))) { report("split", rc); goto done; }
    if ((rc = bpe_gpu_encode_split(ctx, pairs, k))) { report("encode split", rc); goto done; }
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

char *bpe_decode_docs(const uint32_t *ids, size_t len, const uint64_t *id_off, size_t ndocs, dyn_arr_t *pair_arr,
                      int device, size_t *out_len, uint64_t **byte_off)
{
    if ((!ids && len) || !id_off || !pair_arr || !out_len || !byte_off) return NULL;
    bpe_gpu_ctx *ctx = NULL;
    size_t k = 0, total = 0;
    uint32_t *pairs = arr_to_pairs(pair_arr, &k);
    uint64_t *offs = NULL;
    char *out = NULL;
    int rc, ok = 0;
    if (!pairs) return NULL;
    if ((rc = open_engine(device, &ctx))) goto done;
    if ((rc = bpe_gpu_decode_docs(ctx, ids, len, id_off, ndocs, pairs, k, NULL, 0, &total, NULL))) {
        report("decode docs", rc);
        goto done;
    }
    out = malloc(total + 1);
    offs = malloc((ndocs + 1) * sizeof(uint64_t));
    if (!out || !offs) goto done;
    if ((rc = bpe_gpu_decode_docs(ctx, ids, len, id_off, ndocs, pairs, k, (uint8_t *)out, total, &total, offs))) {
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
    *byte_off = offs;
    return out;
}

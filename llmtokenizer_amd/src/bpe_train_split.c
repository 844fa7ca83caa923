/*
 * bpe_train_split.c -- bpe_train_split of bpe_ex.h: load, bpe_gpu_split and
 * bpe_gpu_train_split on the cached engine contexts of bpe.c, the merges
 * returned in the shape compress() returns them.  train_split_with is its body
 * with the split step passed in: bpe_split_preset.c runs it over
 * bpe_gpu_split_preset.
 */
#include "bpe_internal.h"

#include <stdlib.h>

dyn_arr_t *bpe_train_split(const uint8_t *bytes, size_t n, const uint8_t *cls, const uint16_t *brk, long max_merges,
                           int device)
{
    if (!cls || !brk) return NULL;
    const struct split_tables t = {cls, brk};
    return train_split_with(bytes, n, split_tables, &t, max_merges, device);
}

dyn_arr_t *train_split_with(const uint8_t *bytes, size_t n, bpe_split_fn split, const void *rule, long max_merges,
                            int device)
{
    if (!bytes && n) return NULL;
    bpe_gpu_ctx *ctx = NULL;
    size_t k = 0, got = 0, pieces = 0;
    uint32_t *pairs = NULL;
    dyn_arr_t *arr = NULL;
    int rc;
    if ((rc = open_engine(device, &ctx))) goto done;
    if ((rc = bpe_gpu_load(ctx, bytes, n))) { report("load", rc); goto done; }
    if ((rc = split(ctx, rule, &pieces))) { report("split", rc); goto done; }
    if ((rc = bpe_gpu_train_split(ctx, max_merges, &k))) { report("train split", rc); goto done; }
    pairs = malloc((k ? k : 1) * 2 * sizeof(uint32_t));
    if (!pairs) goto done;
    if ((rc = bpe_gpu_fetch_split_merges(ctx, pairs, k, &got))) { report("fetch split merges", rc); goto done; }
    if (got != k) goto done;
    arr = pairs_to_arr(pairs, k);
done:
    close_engine(device, ctx, arr != NULL);
    free(pairs);
    return arr;
}

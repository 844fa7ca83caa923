/*
 * bpe_special_gpu.c -- the special-token entry points of bpe_ex.h over the engine:
 * bpe_encode_split_special and bpe_train_split_special run the bodies of their
 * siblings (bpe_docs.c, bpe_train_split.c) with bpe_gpu_split_special as the split
 * step, bpe_decode_docs_special is bpe_decode_docs over
 * bpe_gpu_decode_docs_special.  Every call loads its bytes first, which drops the
 * split of the call before it on a cached context, specials included.
 */
#include "bpe_internal.h"

#include <stdlib.h>

struct split_special {
    int preset;
    const uint8_t *cls;
    const uint16_t *brk;
    const bpe_gpu_specials *sp;
};

static int split_special(bpe_gpu_ctx *ctx, const void *rule, size_t *pieces)
{
    const struct split_special *r = rule;
    return bpe_gpu_split_special(ctx, r->preset, r->cls, r->brk, r->sp, pieces);
}

uint32_t *bpe_encode_split_special(const uint8_t *bytes, size_t n, int preset, const uint8_t *cls, const uint16_t *brk,
                                   const bpe_gpu_specials *specials, dyn_arr_t *pair_arr, int device, size_t *len,
                                   uint64_t **id_off, uint64_t **byte_off, size_t *ndocs)
{
    const struct split_special r = {preset, cls, brk, specials};
    return encode_split_with(bytes, n, split_special, &r, pair_arr, device, len, id_off, byte_off, ndocs);
}

dyn_arr_t *bpe_train_split_special(const uint8_t *bytes, size_t n, int preset, const uint8_t *cls, const uint16_t *brk,
                                   const bpe_gpu_specials *specials, long max_merges, int device)
{
    const struct split_special r = {preset, cls, brk, specials};
    return train_split_with(bytes, n, split_special, &r, max_merges, device);
}

char *bpe_decode_docs_special(const uint32_t *ids, size_t len, const uint64_t *id_off, size_t ndocs, dyn_arr_t *pair_arr,
                              const bpe_gpu_specials *specials, int device, size_t *out_len, uint64_t **byte_off)
{
    if ((!ids && len) || !pair_arr || !out_len) return NULL;
    if (!id_off && ndocs) return NULL; /* (no offsets: the ids as one flat sequence, no *byte_off) */
    if (id_off && !byte_off) return NULL;
    if (!id_off) byte_off = NULL;
    const uint64_t *io = id_off;
    bpe_gpu_ctx *ctx = NULL;
    size_t k = 0, total = 0;
    uint32_t *pairs = arr_to_pairs(pair_arr, &k);
    uint64_t *offs = NULL;
    char *out = NULL;
    int rc, ok = 0;
    if (!pairs) return NULL;
    if ((rc = open_engine(device, &ctx))) goto done;
    if ((rc = bpe_gpu_decode_docs_special(ctx, ids, len, io, ndocs, pairs, k, specials, NULL, 0, &total, NULL))) {
        report("decode docs", rc);
        goto done;
    }
    out = malloc(total + 1);
    if (byte_off) offs = malloc((ndocs + 1) * sizeof(uint64_t));
    if (!out || (byte_off && !offs)) goto done;
    if ((rc = bpe_gpu_decode_docs_special(ctx, ids, len, io, ndocs, pairs, k, specials, (uint8_t *)out, total, &total,
                                          offs))) {
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

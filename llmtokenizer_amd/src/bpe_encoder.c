/*
 * bpe_encoder.c -- bpe_encode_docs_mode and bpe_encode_split_mode of bpe_ex.h: the
 * bodies of bpe_encode_docs and bpe_encode_split_special (bpe_docs.c) with the
 * device encoder chosen, over bpe_gpu_encode_docs_mode / bpe_gpu_encode_split_mode.
 * A file of its own: the host models of the tests' stand-alone programs have
 * neither engine call.
 */
#include "bpe_internal.h"

struct split_any {
    int preset;
    const uint8_t *cls;
    const uint16_t *brk;
    const bpe_gpu_specials *sp;
};

static int split_any(bpe_gpu_ctx *ctx, const void *rule, size_t *pieces)
{
    const struct split_any *r = rule;
    return bpe_gpu_split_special(ctx, r->preset, r->cls, r->brk, r->sp, pieces);
}

static int encode_split_mode(bpe_gpu_ctx *ctx, const uint32_t *pairs, size_t k, int mode)
{
    return bpe_gpu_encode_split_mode(ctx, pairs, k, mode);
}

uint32_t *bpe_encode_docs_mode(const uint8_t *bytes, size_t n, const uint64_t *doc_off, size_t ndocs, dyn_arr_t *pair_arr,
                               int device, int mode, size_t *len, uint64_t **id_off)
{
    return encode_docs_body(bytes, n, doc_off, ndocs, pair_arr, device, bpe_gpu_encode_docs_mode, mode, len, id_off);
}

uint32_t *bpe_encode_split_mode(const uint8_t *bytes, size_t n, int preset, const uint8_t *cls, const uint16_t *brk,
                                const bpe_gpu_specials *specials, dyn_arr_t *pair_arr, int device, int mode, size_t *len,
                                uint64_t **id_off, uint64_t **byte_off, size_t *ndocs)
{
    const struct split_any r = {preset, cls, brk, specials};
    return encode_split_body(bytes, n, split_any, &r, pair_arr, device, encode_split_mode, mode, len, id_off, byte_off,
                             ndocs);
}

/*
 * bpe_internal.h -- helpers of bpe.c shared with the library's other C files
 * (bpe_docs.c, bpe_train_split.c, bpe_split_preset.c).  Not part of the API: hidden from the shared library's exports.
 */
#ifndef BPE_INTERNAL_H
#define BPE_INTERNAL_H

#include "../../include/bpe.h"
#include "../../include/bpe_ex.h"
#include "../../include/bpe_gpu.h"

#define BPE_PRIVATE __attribute__((visibility("hidden")))

/* statistics of the last call (bpe_last_stats) */
extern BPE_PRIVATE bpe_gpu_stats g_last_stats;

/* "bpe: <what> failed: ..." on stderr */
BPE_PRIVATE void report(const char *what, int rc);
/* the cached engine context of `device` (or a new one); give it back with close_engine */
BPE_PRIVATE int open_engine(int device, bpe_gpu_ctx **ctx);
BPE_PRIVATE void close_engine(int device, bpe_gpu_ctx *ctx, int ok);
/* flat pairs for ids 256.. -> a reference-shaped merge list (NULL: out of memory) */
BPE_PRIVATE dyn_arr_t *pairs_to_arr(const uint32_t *pairs, size_t k);
/* reference-shaped merge list -> flat pairs for ids 256..last_index (malloc'd) */
BPE_PRIVATE uint32_t *arr_to_pairs(dyn_arr_t *arr, size_t *k);
/* id buffer of n entries (huge pages for multi-GB ones) */
BPE_PRIVATE uint32_t *alloc_ids(size_t n);

/* the split step of the calls below: bpe_gpu_split with the tables `rule` points to, or
 * bpe_gpu_split_preset with the preset it points to (bpe_split_preset.c); 0 or a BPE_GPU_E* code */
typedef int (*bpe_split_fn)(bpe_gpu_ctx *ctx, const void *rule, size_t *pieces);
/* ... the first of the two: rule points to a struct split_tables */
struct split_tables {
    const uint8_t *cls;
    const uint16_t *brk;
};
static inline int split_tables(bpe_gpu_ctx *ctx, const void *rule, size_t *pieces)
{
    const struct split_tables *t = rule;
    return bpe_gpu_split(ctx, t->cls, t->brk, pieces);
}
/* the body of bpe_encode_split and bpe_encode_split_preset (bpe_docs.c): their arguments, results and ownership */
BPE_PRIVATE uint32_t *encode_split_with(const uint8_t *bytes, size_t n, bpe_split_fn split, const void *rule,
                                        dyn_arr_t *pair_arr, int device, size_t *len, uint64_t **id_off,
                                        uint64_t **byte_off, size_t *ndocs);
/* the body of bpe_train_split and bpe_train_split_preset (bpe_train_split.c) */
BPE_PRIVATE dyn_arr_t *train_split_with(const uint8_t *bytes, size_t n, bpe_split_fn split, const void *rule,
                                        long max_merges, int device);

#endif

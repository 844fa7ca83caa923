/*
 * bpe_internal.h -- helpers of bpe.c shared with the library's other C files
 * (bpe_docs.c, bpe_train_split.c).  Not part of the API: hidden from the shared library's exports.
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

#endif

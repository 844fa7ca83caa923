/*
 * bpe_ex.h -- extensions of the drop-in API (not in the reference).
 *
 * The reference trains only from a file path with no merge cap and no device
 * choice (bpe/inc/bpe.h:32).  These entry points expose what the MI355X build
 * adds: a merge cap, a device ordinal, in-memory corpora, a standalone encoder
 * (the replace pass of bpe.c:760-779 applied merge by merge to new text) and
 * run statistics.  All return the same ownership as compress(): the caller
 * frees *encoding with free() and the dyn_arr_t with dyn_arr_free().
 */
#ifndef BPE_EX_H
#define BPE_EX_H

#include "bpe.h"
#include "bpe_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* compress() with an explicit merge cap (< 0: unbounded) and device */
dyn_arr_t *compress_ex(const char *path, long max_merges, int device, uint32_t **encoding, size_t *len);

/* train on bytes already in memory (no NUL truncation: pass the length the
 * reference would see, i.e. strlen of the file contents) */
dyn_arr_t *bpe_train_bytes(const uint8_t *bytes, size_t n, long max_merges, int device,
                           uint32_t **encoding, size_t *len);

/* One training job over ndev devices in this process (rank r on devices[r];
 * a device may repeat): contiguous shards, per-merge exchanges through P2P
 * mailboxes, identical merges; the encoding is the shards' ids concatenated.
 * Corpora below 2^20 bytes train on devices[0] alone (the sharded tie rule
 * equals the reference's from there on); an unbounded
 * run (max_merges < 0) over several devices stops at 2^22 merges.
 * compress() takes this path when BPE_NUM_GPUS > 1 (devices BPE_DEVICE ..) or
 * BPE_DEVICES="d0,d1,..." lists several devices (device count). */
dyn_arr_t *bpe_train_bytes_devices(const uint8_t *bytes, size_t n, long max_merges, int ndev, const int *devices,
                                   uint32_t **encoding, size_t *len);
/* compress() over ngpu devices BPE_DEVICE, BPE_DEVICE + 1, ... */
dyn_arr_t *compress_multi(const char *path, long max_merges, int ngpu, uint32_t **encoding, size_t *len);

/* encode bytes with a trained merge list (dyn_arr_t from compress/read_pairs) */
uint32_t *bpe_encode_bytes(const uint8_t *bytes, size_t n, dyn_arr_t *pair_arr, int device, size_t *len);

/* Encode a batch of documents in one pass: document d is bytes [doc_off[d],
 * doc_off[d + 1]) (doc_off[0] == 0, doc_off[ndocs] == n, non-decreasing) and no
 * merge crosses a document start, so ids [(*id_off)[d], (*id_off)[d + 1]) are
 * bpe_encode_bytes of document d alone.  The caller frees the returned ids
 * and *id_off (ndocs + 1 entries) with free(). */
uint32_t *bpe_encode_docs(const uint8_t *bytes, size_t n, const uint64_t *doc_off, size_t ndocs,
                          dyn_arr_t *pair_arr, int device, size_t *len, uint64_t **id_off);
/* The inverse: the documents' bytes concatenated (NUL bytes vanish, as in
 * decompress; NUL-terminated, *out_len without it) and *byte_off (ndocs + 1
 * entries): document d is out [(*byte_off)[d], (*byte_off)[d + 1]).  The
 * caller frees both with free(). */
char *bpe_decode_docs(const uint32_t *ids, size_t len, const uint64_t *id_off, size_t ndocs,
                      dyn_arr_t *pair_arr, int device, size_t *out_len, uint64_t **byte_off);

/* Split bytes into pieces on the device by a two-table rule (cls[256], brk[16]:
 * bpe_gpu.h, bpe_gpu_split / bpe_gpu_split_rule) and encode the pieces as
 * documents, without the offsets passing through the host on the way.  *ndocs =
 * pieces; *id_off and, unless byte_off is NULL, *byte_off (the piece starts
 * followed by n) have *ndocs + 1 entries.  The caller frees the returned ids,
 * *id_off and *byte_off with free(). */
uint32_t *bpe_encode_split(const uint8_t *bytes, size_t n, const uint8_t *cls, const uint16_t *brk,
                           dyn_arr_t *pair_arr, int device, size_t *len, uint64_t **id_off, uint64_t **byte_off,
                           size_t *ndocs);

/* Split bytes into pieces on the device by the same two-table rule and train on
 * the pieces (bpe_gpu.h, bpe_gpu_train_split): the merges never cross a piece
 * boundary, so bpe_encode_split with the same rule can apply every one of them.
 * max_merges < 0: until the stop rule.  Returns the merge list in the shape
 * compress() returns it (the caller frees it with dyn_arr_free()), NULL on failure. */
dyn_arr_t *bpe_train_split(const uint8_t *bytes, size_t n, const uint8_t *cls, const uint16_t *brk, long max_merges,
                           int device);

/* The preset split rules (bpe_gpu.h: BPE_SPLIT_LINES, BPE_SPLIT_WORDS, BPE_SPLIT_GPT2, BPE_SPLIT_GPT2_UNICODE, BPE_SPLIT_CL100K) in plain C, on
 * the host and without a GPU: the written definition bpe_gpu_split_preset is held to, and the
 * yardstick for inputs too large for a regular-expression engine.  Two-phase like the fetch calls:
 * out may be NULL, *count = pieces + 1 (the piece starts followed by n; n == 0: the single offset 0),
 * and at most cap entries are written.  BPE_GPU_EINVAL for another preset or a bad argument. */
int bpe_split_offsets_host(int preset, const uint8_t *bytes, size_t n, uint64_t *out, size_t cap, size_t *count);

/* The classes of BPE_SPLIT_GPT2_UNICODE (bpe_gpu.h), pure host functions.  bpe_unicode_class: the class of a
 * code point, 0 P, 1 L (\p{L}), 2 N (\p{N}), 3 S (U+0020), 4 W (the other White_Space); P above U+10FFFF.
 * bpe_unicode_info: *source = where the committed table came from ("regex <version>", a static string),
 * *digest = the FNV-1a 64 of the 0x110000 classes as bytes in code point order; either may be NULL.  Returns 0. */
int bpe_unicode_class(uint32_t cp);
int bpe_unicode_info(const char **source, uint64_t *digest);

/* bpe_encode_split with a preset in place of the tables (bpe_gpu_split_preset): the way to
 * BPE_SPLIT_GPT2, which no two tables express.  Results and ownership as bpe_encode_split. */
uint32_t *bpe_encode_split_preset(const uint8_t *bytes, size_t n, int preset, dyn_arr_t *pair_arr, int device,
                                  size_t *len, uint64_t **id_off, uint64_t **byte_off, size_t *ndocs);
/* bpe_train_split with a preset in place of the tables */
dyn_arr_t *bpe_train_split_preset(const uint8_t *bytes, size_t n, int preset, long max_merges, int device);

/* Special tokens (bpe_gpu.h, "Special tokens": the set, the overlap-free condition, the split, the ids).
 * bpe_specials_check: 0 when `specials` (NULL or count 0: the empty set) keeps the limits and the
 * overlap-free condition; else BPE_GPU_EINVAL and, unless msg is NULL, a message in msg[0 .. msg_cap)
 * that names the special or the pair at fault by index and text.  No GPU. */
int bpe_specials_check(const bpe_gpu_specials *specials, char *msg, size_t msg_cap);
/* bpe_split_offsets_host with specials, for a preset or, with preset < 0, for the tables cls[256] / brk[16]:
 * the matches found byte by byte, every segment between them split as a text of its own.  This is the
 * written definition bpe_gpu_split_special is held to.  out / cap / count as bpe_split_offsets_host;
 * sp_piece / sp_index (either may be NULL) receive at most sp_cap special pieces in order, the piece's
 * index among the offsets and the special's index in the caller's list, *sp_count (may be NULL) their
 * number.  BPE_GPU_EINVAL for a set bpe_specials_check refuses, a class above 15 or a bad argument. */
int bpe_split_offsets_host_special(int preset, const uint8_t *cls, const uint16_t *brk, const uint8_t *bytes, size_t n,
                                   const bpe_gpu_specials *specials, uint64_t *out, size_t cap, size_t *count,
                                   uint64_t *sp_piece, uint32_t *sp_index, size_t sp_cap, size_t *sp_count);
/* bpe_encode_split / bpe_encode_split_preset with specials (preset < 0: the tables): every occurrence of
 * special j is one piece with the one id 256 + merges + j.  Results and ownership as bpe_encode_split. */
uint32_t *bpe_encode_split_special(const uint8_t *bytes, size_t n, int preset, const uint8_t *cls, const uint16_t *brk,
                                   const bpe_gpu_specials *specials, dyn_arr_t *pair_arr, int device, size_t *len,
                                   uint64_t **id_off, uint64_t **byte_off, size_t *ndocs);
/* bpe_train_split / bpe_train_split_preset with specials: the special pieces are no part of the corpus */
dyn_arr_t *bpe_train_split_special(const uint8_t *bytes, size_t n, int preset, const uint8_t *cls, const uint16_t *brk,
                                   const bpe_gpu_specials *specials, long max_merges, int device);
/* bpe_decode_docs with specials: id 256 + merges + j expands to special j's bytes.  id_off may be NULL
 * with ndocs == 0: the ids are one flat sequence and *byte_off is not written. */
char *bpe_decode_docs_special(const uint32_t *ids, size_t len, const uint64_t *id_off, size_t ndocs, dyn_arr_t *pair_arr,
                              const bpe_gpu_specials *specials, int device, size_t *out_len, uint64_t **byte_off);

/* Vocabularies (bpe_gpu.h, "Vocabularies").  bpe_vocab_check: 0 when the ids of `vocab` are pairwise distinct
 * across its three arrays and below BPE_VOCAB_ID_LIMIT, vocab->n_merges == n_merges, it has at most
 * BPE_GPU_SPECIAL_MAX_COUNT specials and, unless pairs is NULL, both parts of merge r (pairs[2 r], pairs[2 r + 1])
 * are below 256 + r; else BPE_GPU_EINVAL and, unless msg is NULL, a message in msg[0 .. msg_cap) that names
 * the offender ("byte 0x21 and merge 7 share the id 5").  No GPU. */
int bpe_vocab_check(const bpe_gpu_vocab *vocab, const uint32_t *pairs, size_t n_merges, char *msg, size_t msg_cap);
/* The two tables of a vocabulary bpe_vocab_check accepts (else its code): fwd[k] = the vocabulary id of internal
 * id k, *n_fwd = 256 + n_merges + n_specials entries; inv[id] = the internal id of vocabulary id `id` or
 * 0xFFFFFFFF for a hole, *n_inv = the largest id + 1 entries.  Two-phase: either array may be NULL, at most
 * fwd_cap / inv_cap entries are written.  No GPU. */
int bpe_vocab_tables(const bpe_gpu_vocab *vocab, uint32_t *fwd, size_t fwd_cap, uint32_t *inv, size_t inv_cap,
                     size_t *n_fwd, size_t *n_inv);
/* bpe_encode_split_special whose ids are the vocabulary's (bpe_gpu_map_ids after the encode); specials may be
 * NULL when vocab->n_specials == 0.  Results and ownership as bpe_encode_split. */
uint32_t *bpe_encode_split_vocab(const uint8_t *bytes, size_t n, int preset, const uint8_t *cls, const uint16_t *brk,
                                 const bpe_gpu_specials *specials, dyn_arr_t *pair_arr, const bpe_gpu_vocab *vocab,
                                 int device, size_t *len, uint64_t **id_off, uint64_t **byte_off, size_t *ndocs);
/* bpe_decode_docs_special over vocabulary ids (bpe_gpu_decode_docs_vocab) */
char *bpe_decode_docs_vocab(const uint32_t *ids, size_t len, const uint64_t *id_off, size_t ndocs, dyn_arr_t *pair_arr,
                            const bpe_gpu_specials *specials, const bpe_gpu_vocab *vocab, int device, size_t *out_len,
                            uint64_t **byte_off);

/* Text batches (bpe_gpu.h, "Text batches").  bpe_texts_check: 0 when text_off[0 .. T] are the byte offsets of T
 * texts in n bytes: text_off[0] == 0, none below the one before it, text_off[T] == n, and n + T (a gap byte per
 * text) at most BPE_TEXTS_MAX_POSITIONS; else BPE_GPU_EINVAL and, unless msg is NULL, a message in
 * msg[0 .. msg_cap) that names the offending offset by its index.  No GPU. */
#define BPE_TEXTS_MAX_POSITIONS 0xFFFFFFFEull
int bpe_texts_check(const uint64_t *text_off, size_t T, size_t n, char *msg, size_t msg_cap);
/* The bytes as a context keeps a text batch: out[0 .. n + T) = every text followed by one gap byte 0x00, so
 * text k begins at text_off[k] + k and its gap is position text_off[k + 1] + k.  BPE_GPU_EINVAL for offsets
 * bpe_texts_check refuses or out_cap < n + T.  No GPU. */
int bpe_texts_gap(const uint8_t *bytes, size_t n, const uint64_t *text_off, size_t T, uint8_t *out, size_t out_cap);
/* ... and the stretch [lo, hi) of them alone: out[0 .. hi - lo).  The offsets must be ones bpe_texts_check accepts
 * (they are not checked again: bpe_gpu_load_texts calls this per chunk and thread); BPE_GPU_EINVAL for
 * lo > hi or hi > n + T.  No GPU. */
int bpe_texts_gap_range(const uint8_t *bytes, size_t n, const uint64_t *text_off, size_t T, size_t lo, size_t hi,
                        uint8_t *out);

/* Token spans (bpe_gpu.h, "Token spans").  bpe_span_lens: the byte length of every token id, the table the spans
 * are summed from: a byte 1 (NUL included), merge r the sum of its two halves, special j specials->len[j].
 * Without a vocabulary it is indexed by internal id, *count = 256 + n_merges + specials entries; with one by
 * vocabulary id, *count = the largest id + 1 entries and a hole 0 (bpe_vocab_tables' forward table; the
 * vocabulary's counts must be the lists').  Two-phase: out may be NULL, at most cap entries are written.
 * BPE_GPU_EINVAL for a merge that names an id at or above its own (its rank is in the message),
 * BPE_GPU_ERANGE for a length above 2^32 - 1; msg (may be NULL) receives the message.  No GPU. */
int bpe_span_lens(const uint32_t *pairs, size_t n_merges, const bpe_gpu_specials *specials, const bpe_gpu_vocab *vocab,
                  uint32_t *out, size_t cap, size_t *count, char *msg, size_t msg_cap);
/* The spans of ids[0 .. n_ids) held as T texts: text k has the ids [text_off[k], text_off[k + 1]) and the bytes
 * [byte_off[k], byte_off[k + 1]) of bytes[0 .. n) (both offset arrays run from 0 to their count without
 * falling); lens[0 .. n_lens) is bpe_span_lens' table in the ids' numbering.  out[2 i], out[2 i + 1] = the span
 * of id i relative to its text's first byte, in bytes (unit BPE_SPAN_BYTE; bytes may be NULL) or in characters
 * (BPE_SPAN_CHAR), as bpe_gpu.h defines them.  Plain loops: this is the definition the device is held to.
 * BPE_GPU_EDATA for an id outside the table (or of length 0: a hole) and for a text whose lengths do not sum to
 * its byte count (the text's index is in the message); BPE_GPU_ERANGE for a text above 2^32 - 1 bytes;
 * BPE_GPU_EINVAL for bad offsets or another unit.  msg (may be NULL) receives the message.  No GPU. */
int bpe_token_spans_host(const uint32_t *ids, size_t n_ids, const uint64_t *text_off, size_t T, const uint8_t *bytes,
                         size_t n, const uint64_t *byte_off, const uint32_t *lens, size_t n_lens, int unit, uint32_t *out,
                         char *msg, size_t msg_cap);

/* Packed streams (bpe_gpu.h, "Packed streams").  bpe_stream_check: 0 for a description bpe_gpu_pack_stream takes;
 * BPE_GPU_EINVAL for s == NULL, seq_len == 0 or a flag bit that is none of BPE_STREAM_BOS, _EOS and _DROP_LAST,
 * BPE_GPU_ERANGE for seq_len above 2^24; msg (may be NULL) receives a message that names the field.  No GPU. */
int bpe_stream_check(const bpe_gpu_stream *s, char *msg, size_t msg_cap);
/* The rows of ids[0 .. n) held as T texts (text k has the ids [text_off[k], text_off[k + 1]); the offsets run from 0
 * to n without falling): rows[R][seq_len], and seg and pos of the same shape unless NULL, as bpe_gpu.h defines them.
 * Plain loops, text by text and cell by cell: this is the definition the device is held to.  *n_rows = R and
 * *n_stream = N (each may be NULL); with rows == NULL nothing else happens.  BPE_GPU_EINVAL for rows_cap < R and for
 * bad offsets, and what bpe_stream_check refuses.  No GPU. */
int bpe_pack_stream_host(const uint32_t *ids, size_t n, const uint64_t *text_off, size_t T, const bpe_gpu_stream *s,
                         uint32_t *rows, uint32_t *seg, uint32_t *pos, size_t rows_cap, size_t *n_rows,
                         uint64_t *n_stream);

/* Rows back to texts (bpe_gpu.h, "Rows back to texts").  bpe_rows_check: 0 for a description bpe_gpu_unpack_rows
 * takes; BPE_GPU_EINVAL for desc == NULL, a flag bit that is neither BPE_ROWS_PAD nor BPE_ROWS_SKIP, n_stop above 8
 * and, under BPE_ROWS_SKIP, n_skip above 256 or n_skip ids without a skip pointer; msg (may be NULL) receives a
 * message that names the field.  No GPU. */
int bpe_rows_check(const bpe_gpu_rows *desc, char *msg, size_t msg_cap);
/* The kept ids of rows[B][L] (cells of cell_bytes = 4 or 8, row k at rows + k * row_stride cells; lens: uint32[B] or
 * NULL), as bpe_gpu.h defines them.  Plain loops, row by row and cell by cell: this is the definition the device is
 * held to.  *n = the kept ids (may be NULL); text_off (B + 1 entries) and bounds (2 B entries) are written unless
 * NULL, ids (ids_cap entries of room) too: with ids == NULL the call is the query.  BPE_GPU_EINVAL for what
 * bpe_rows_check refuses, another cell_bytes, row_stride < L, no rows where there are cells, lens[k] > L (the lowest
 * such row is in the message; no row is read then) and ids_cap < n; BPE_GPU_ERANGE for L above 2^24; BPE_GPU_EDATA
 * for a kept 8-byte cell outside 0 .. 2^32 - 1 (the lowest such row is in the message).  After a refusal nothing has
 * been written but msg (may be NULL).  No GPU. */
int bpe_unpack_rows_host(const void *rows, int cell_bytes, size_t B, uint32_t L, size_t row_stride, const uint32_t *lens,
                         const bpe_gpu_rows *desc, uint32_t *ids, size_t ids_cap, size_t *n, uint64_t *text_off,
                         uint32_t *bounds, char *msg, size_t msg_cap);

/* statistics of the last compress/compress_ex/bpe_train_bytes/bpe_encode_bytes/bpe_encode_docs/bpe_encode_split(_preset) */
int bpe_last_stats(bpe_gpu_stats *out);

/* compress / compress_ex / bpe_train_bytes / bpe_encode_bytes / decompress keep
 * one engine context per device between calls.  By default its device memory
 * is given back when the call returns (bpe_gpu_trim: only the stream and the
 * pinned host staging stay); BPE_KEEP_CONTEXT=1 keeps the HBM pool too,
 * BPE_KEEP_CONTEXT=0 creates and destroys a context per call.  Free them: */
void bpe_release_engines(void);

#ifdef __cplusplus
}
#endif
#endif

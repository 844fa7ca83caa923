/*
 * bpe_gpu.h -- C-ABI of the MI355X (gfx950) BPE engine in libbpe_amd.so.
 *
 * This is the thin shim the drop-in host library (bpe.h's compress /
 * decompress, implemented in C in llmtokenizer_amd/src/bpe.c) drives.  Plain
 * pointers and sizes only; every call returns an int status (0 = ok, < 0 =
 * error, see bpe_gpu_strerror) and is made from one host thread per context.
 *
 * Reference interfaces replaced (neofytr/LLMTokenizer):
 *   bpe_gpu_train      -- the merge-training loop of compress():
 *                         get_freq workers + hash_table_merge + flatten +
 *                         dyn_arr_max + replace pass
 *                         (bpe/src/bpe.c:428-527, 669-783;
 *                          hash_table/src/hash_table.c:109-193, 195-307;
 *                          dyn_arr/src/dyn_arr.c:136-181)
 *   bpe_gpu_fetch_ids  -- compress()'s *encoding output (bpe.c:785-794)
 *   bpe_gpu_encode     -- the replace pass (bpe.c:760-779) applied merge by
 *                         merge to new text (standalone encoder)
 *   bpe_gpu_decode     -- decompress()/resolve_pair (bpe.c:23-92, 341-394):
 *                         expansion lengths, prefix sum and byte gather
 *                         on the device
 *   bpe_gpu_load_fd    -- get_file + strlen (bpe.c:130-180, 555), streamed
 */
#ifndef BPE_GPU_H
#define BPE_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
    BPE_GPU_OK = 0,
    BPE_GPU_EINVAL = -1,   /* bad argument                                  */
    BPE_GPU_EHIP = -2,     /* HIP runtime error (bpe_gpu_last_error() tells) */
    BPE_GPU_ENOMEM = -3,   /* device allocation failed                      */
    BPE_GPU_ENODEV = -4,   /* no GPU / device index out of range            */
    BPE_GPU_ESTATE = -5,   /* call out of order (e.g. train before load)    */
    BPE_GPU_ERANGE = -6,   /* corpus larger than 2^32-2 bytes per device, or a
                              token longer than 2^31-3 bytes (its end code)   */
    BPE_GPU_EDATA = -7,    /* unknown token id (decode) / corrupt merge list */
    BPE_GPU_EINTERNAL = -8,/* engine invariant violated (reported, not hidden) */
    BPE_GPU_EIO = -9       /* file read error (errno is set)                */
};

typedef struct bpe_gpu_ctx bpe_gpu_ctx;

typedef struct {
    uint64_t n_in;            /* tokens loaded (bytes after truncation)        */
    uint64_t n_out;           /* tokens after training / encoding              */
    uint64_t merges;          /* merges learned / applied                      */
    uint64_t iterations;      /* training iterations run (incl. the last one)  */
    uint64_t distinct_pairs;  /* D at the last argmax                          */
    uint64_t merged_buckets;  /* B_final at the last argmax                    */
    uint64_t tracked_iters;   /* iterations with per-thread table tracking     */
    uint64_t tie_events;      /* chain-order ties resolved by emulation        */
    uint64_t edge_events;     /* D == resize threshold resolved by emulation   */
    uint64_t rule_ties;       /* schedule-dependent ties decided by the rule (approximate in hot-set mode) */
    uint64_t table_grows;     /* pair-count table regrowths                    */
    uint64_t keys;            /* slots in use in the pair-count table (informational; dense table: keys created) */
    double ms_init;           /* device-side setup (counting sort, table)      */
    double ms_train;          /* merge loop                                    */
    double ms_total;          /* init + loop (what bench.py times end to end)  */
    double ms_count_pass;     /* the one corpus-wide pair-count pass (k_pair_hist*, reads the bytes) */
    uint64_t candidates;      /* candidate positions examined by the scans      */
    uint64_t occurrences;     /* pair occurrences replaced                       */
    uint64_t l1_rescanned;    /* level-1 summary blocks rescanned                 */
    uint64_t spec_hits;       /* next merges found by the speculative scan        */
    uint64_t spec_misses;     /* mispredicted next merges (host re-scan)          */
    uint64_t count_pass_span; /* >0: the count pass ran in span form, its histogram copies R and kernel:
                                 200 + R k_pair_hist_v (default), 300 + R its run-folding variant for
                                 skewed corpora, R k_pair_hist_span, 100 + R k_pair_hist_pk (BPE_HIST_FORM) */
    uint64_t hot_rebuilds;    /* hot-set argmax: full-table rebuilds of the listed keys */
    uint64_t hot_mode;        /* 0 level summaries, 1 hot set, 2 hot set given up mid-run */
    uint64_t hot_scanned;     /* hot-set entries reduced, summed over the merges */
    uint64_t enc_path;        /* encode: 1 window-local replay, 3 the same after its wide-halo
                                 retry, 2 global batched replay                 */
    uint64_t enc_windows;     /* encode: windows replayed (window path)           */
    uint64_t relists;         /* training: byte-pair position lists rebuilt       */
    uint64_t batches;         /* training: merge batches (several merges per scan/apply pair) */
    uint64_t batch_dropped;   /* training: batch members that failed the verification (or came after one) */
    uint64_t batch_retries;   /* training: batches formed again (shorter) after a failed member; a failed
                                 batch whose verified prefix abuts no dropped member applies that prefix
                                 instead (counted in batches and batch_dropped, not here) */
    uint64_t table_updates;   /* training, batches: pair-table updates of the applies */
    double ms_scan_span;      /* training, batches: average k_bscan span (device wall clock) */
    double ms_apply_span;     /* training, batches: average k_bapply span (device wall clock) */
    uint64_t track_exact;     /* tracked iterations: exact (thread, pair) passes run */
    uint64_t track_skipped;   /* tracked iterations whose exact pass the distinct-count
                                 bounds proved unnecessary (no per-thread table grows) */
    uint64_t track_violations;/* BPE_TRACK=2 check runs: skipped passes the exact one
                                 contradicts (must stay 0)                         */
    uint64_t track_light;     /* tracked iterations: on-device exact counts of only the
                                 threads whose bound reached a growth threshold   */
    uint64_t batch_end[8];    /* training, batches: what ended each batch's formation --
                                 [0] the lists used up or 127 members [1] merge cap / count <= 1 /
                                 hot threshold [2] a member predicted to lose to a skipped key
                                 [3] a key listed twice [4] a tie whose
                                 order the batch could change [5] a member that does not commute
                                 with an earlier one [6] pair-table margin [7] occurrence staging */
    double ms_select_span;    /* training, batches: average k_bsel span (the selection beside the
                                 previous batch's token rewrite; device wall clock) */
    uint64_t select_launches; /* ... over this many k_bsel launches */
    uint64_t tie_verified;    /* training, batches: batches with a member admitted on a tie order that
                                 holds only if the earlier members zero few keys (checked in k_bapply) */
    uint64_t tie_failed;      /* ... of them re-formed shorter (the check failed) */
    uint64_t keys_zeroed;     /* training, batches: pair keys the applied batches took to count 0 */
    uint64_t keys_skipped;    /* training, batches: listed keys the applied batches skipped (they do not
                                 commute with an earlier member; its merge lowers their count) */
    uint64_t skip_failed;     /* ... batches whose first failed member failed on a skipped key */
    uint64_t stop_reason;     /* training: why the run ended -- 1 the reference's stop rule (no pair
                                 left or max count <= 1, bpe.c:730-750), 2 the caller's merge cap,
                                 3 the engine's own cap on an unbounded run (2^24 merges; 2^22 over
                                 several devices in compress_multi) before that rule: reported on
                                 stderr too, since the reference has no cap */
    uint64_t table_dense;     /* training: 1 when the pair table was the dense one (a count per pair of ids,
                                 chosen when the run has a merge cap and the square of 256 + cap ids is no
                                 larger than the hash table; BPE_TAB_DENSE=0 / 1 forces either), else 0.
                                 `keys` then counts the keys created (counts that left 0), not slots taken */
} bpe_gpu_stats;

/* Per-merge record (training): the structured per-iteration metrics the
   reference only prints (bpe.c:560).  Off by default; when on, every committed
   merge writes one record on the device (no host round trip).  The batch
   engine commits several merges per kernel chain: its records share the
   batch's pre-batch D and token count.                                      */
typedef struct {
    uint32_t count;           /* occurrences of the merged pair (the argmax count) */
    uint32_t ties;            /* one-merge engine: keys sharing its (count, bucket); batches: 0 */
    uint32_t batch;           /* batch engine: the batch that committed it; else the merge index */
    uint32_t batch_pos;       /* its position in that batch (0: one-merge engine)  */
    uint64_t distinct_pairs;  /* D when it was selected                            */
    uint64_t tokens;          /* tokens when it was selected                       */
    double t_us;              /* device wall clock at its selection, us after the first record's */
} bpe_gpu_merge_rec;

/* records for the next trainings on ctx (on != 0), up to 2^20 merges */
int bpe_gpu_set_merge_log(bpe_gpu_ctx *ctx, int on);
/* the last training's records: *count = records held; out may be NULL */
int bpe_gpu_fetch_merge_log(bpe_gpu_ctx *ctx, bpe_gpu_merge_rec *out, size_t cap, size_t *count);

/* Run events of the last training, in order: each entry is
   (kind << 56) | merges committed before the event.  The hot-set rebuild at
   the start of a run is recorded with 0 merges.  *count = events held. */
enum {
    BPE_GPU_EV_RELIST = 1,       /* byte-pair position lists rebuilt from the live tokens */
    BPE_GPU_EV_HOT_REBUILD = 2,  /* hot set (listed keys with count >= hot_T) rebuilt */
    BPE_GPU_EV_TABLE_GROW = 3,   /* pair-count table regrown (x4) */
    BPE_GPU_EV_MODE = 4          /* hot set given up for the level summaries / tracked phase */
};
int bpe_gpu_fetch_events(bpe_gpu_ctx *ctx, uint64_t *out, size_t cap, size_t *count);

/* Free the context's device memory (buffer pool, corpus, scratch) but keep
   the stream, events and pinned host staging, so the next load on it pays no
   stream / staging set-up.  The context must be loaded again before use. */
int bpe_gpu_trim(bpe_gpu_ctx *ctx);

/* number of visible GPUs */
int bpe_gpu_device_count(int *count);

/* PCI bus id of device `device` ("dddd:bb:dd.f", NUL-terminated into buf[len]):
   the identity ranks compare before mapping each other's mailboxes */
int bpe_gpu_device_pci(int device, char *buf, int len);

/* *ok = 1 when `device` can access `peer`'s memory directly (hipDeviceCanAccessPeer;
   1 for device == peer): checked on every pair of ranks before the P2P transport
   maps the peers' mailboxes */
int bpe_gpu_peer_access(int device, int peer, int *ok);

/* create a context bound to device `device` (HIP ordinal) */
int bpe_gpu_create(int device, bpe_gpu_ctx **out);
void bpe_gpu_destroy(bpe_gpu_ctx *ctx);

/* Load a byte corpus (host memory) into HBM.  No NUL truncation is applied
 * here; compress() applies the reference's strlen semantics before calling. */
int bpe_gpu_load(bpe_gpu_ctx *ctx, const uint8_t *bytes, size_t n);

/* Stream the first `size` bytes of file descriptor fd (positional reads from
 * offset 0) into HBM through pinned,
 * double-buffered staging (disk reads overlap the host-to-device copies).  The
 * corpus ends at the first NUL byte, as the reference's get_file + strlen
 * (bpe/src/bpe.c:130-180, 555); *n_loaded receives its length. */
int bpe_gpu_load_fd(bpe_gpu_ctx *ctx, int fd, size_t size, size_t *n_loaded);

/* Generate bytes [offset, offset+n) of the seeded random_text.txt-shaped corpus
 * (llmtokenizer_amd/synth.py) directly in HBM. */
int bpe_gpu_synth(bpe_gpu_ctx *ctx, uint64_t seed, size_t n, uint64_t offset);

/* Train until the reference's stop rule (no pair, or max count <= 1) or
 * max_merges (< 0 = unbounded).  *n_merges receives the merge count. */
int bpe_gpu_train(bpe_gpu_ctx *ctx, long max_merges, size_t *n_merges);

/* Train flags.  BPE_GPU_FAST: decide every tie by the schedule-free rule
 * (smallest (a, b) among the keys with the maximal count and bucket) instead
 * of emulating the reference's static 16-thread schedule below 2^20 tokens.
 * For corpora of >= 2^20 tokens both are the same (the reference itself is
 * schedule-dependent there); sharded training always uses it. */
enum { BPE_GPU_FAST = 1 };
int bpe_gpu_train_ex(bpe_gpu_ctx *ctx, long max_merges, unsigned flags, size_t *n_merges);

/* merges as (a, b) pairs, ids 256.. in order; cap in pairs */
int bpe_gpu_fetch_merges(bpe_gpu_ctx *ctx, uint32_t *pairs, size_t cap, size_t *count);

/* final token ids of the loaded corpus (after train or encode) */
int bpe_gpu_fetch_ids(bpe_gpu_ctx *ctx, uint32_t *ids, size_t cap, size_t *len);
/* ids [first, first + count) of them */
int bpe_gpu_fetch_ids_range(bpe_gpu_ctx *ctx, size_t first, uint32_t *ids, size_t count);

/* Encode the loaded corpus with a given merge list (pairs, id 256 + r). */
int bpe_gpu_encode(bpe_gpu_ctx *ctx, const uint32_t *pairs, size_t n_merges);

/* Decode ids with a merge list into bytes (NUL bytes vanish, as in the
 * reference's C-string decoder).  Two-phase: out == NULL returns the length
 * in *out_len. */
int bpe_gpu_decode(bpe_gpu_ctx *ctx, const uint32_t *ids, size_t len,
                   const uint32_t *pairs, size_t n_merges,
                   uint8_t *out, size_t cap, size_t *out_len);

/* ------------------------------------------------------------------------
 * Document batches.  A batch is the loaded bytes plus ndocs + 1 offsets:
 * doc_off[0] == 0, doc_off[ndocs] == the loaded length, non-decreasing (empty
 * documents are allowed); document d is bytes [doc_off[d], doc_off[d + 1]).
 * Merges never cross a document start: the ids of document d are exactly
 * bpe_gpu_encode's of its bytes alone, for any merge list that call accepts.
 * One device, at most 2^32 - 2 bytes and documents per batch.
 * ---------------------------------------------------------------------- */

/* Encode the loaded bytes as ndocs documents (doc_off[ndocs + 1], see above).  Afterwards
   bpe_gpu_fetch_ids / _fetch_ids_range / _ids_checksum serve the concatenated ids. */
int bpe_gpu_encode_docs(bpe_gpu_ctx *ctx, const uint64_t *doc_off, size_t ndocs,
                        const uint32_t *pairs, size_t n_merges);
/* id_off[0..ndocs] of the last bpe_gpu_encode_docs; out may be NULL, *count = ndocs + 1 */
int bpe_gpu_fetch_doc_offsets(bpe_gpu_ctx *ctx, uint64_t *out, size_t cap, size_t *count);
/* out8 = {ndocs, docs through the fallback, windows, windows failed, core, halo, 0, 0} */
int bpe_gpu_docs_info(bpe_gpu_ctx *ctx, uint64_t *out8);
/* bpe_gpu_decode plus byte_off[0..ndocs] (bytes of document d = out[byte_off[d], byte_off[d+1])) */
int bpe_gpu_decode_docs(bpe_gpu_ctx *ctx, const uint32_t *ids, size_t len, const uint64_t *id_off,
                        size_t ndocs, const uint32_t *pairs, size_t n_merges,
                        uint8_t *out, size_t cap, size_t *out_len, uint64_t *byte_off);
/* The window geometry of the document encoder (pure function, no GPU; exported
 * for the host-side tests): window w of cores of `core` bytes over the batch,
 * clipped at the document starts around its core.
 * out8 = {L, R, lunk, runk, first doc with off >= L, doc starts in [L, R], 0, 0} */
int bpe_gpu_docs_window(const uint64_t *doc_off, size_t ndocs, uint64_t n,
                        uint32_t core, uint32_t halo, uint64_t w, uint64_t *out8);

/* ------------------------------------------------------------------------
 * Splitting the loaded bytes into pieces on the device.  A rule is two tables:
 * cls[256], the class (0..15) of every byte value, and brk[16]: bit c of brk[p]
 * says that a piece starts at byte i when cls[b[i - 1]] == p and cls[b[i]] == c.
 * Byte 0 always starts a piece.  The split's offsets are the piece starts in
 * order followed by n: ndocs + 1 of them, no piece empty (n == 0: ndocs == 0 and
 * the single offset 0).  They stay in HBM and are bpe_gpu_encode_docs' doc_off
 * for bpe_gpu_encode_split: no host copy of them is made on the way.
 *
 * The two table presets are this project's own rules, NOT GPT-2's regular
 * expression: no contractions, no look-ahead, no Unicode classes.
 *   BPE_SPLIT_LINES  class 1 is '\n', the rest 0; brk[1] = 0x3: a piece ends
 *                    after each newline and keeps it.
 *   BPE_SPLIT_WORDS  class 1 letters A-Z a-z and every byte >= 0x80 (a UTF-8
 *                    sequence never splits), 2 digits, 3 the space 0x20, 4 the
 *                    other white space \t \n \v \f \r, 0 the rest.  A piece
 *                    starts wherever the class changes, except that nothing
 *                    starts after a space unless class 4 follows (spaces
 *                    attach to what follows them): brk[p] = 0x1F & ~(1 << p)
 *                    for p in 0, 1, 2, 4 and brk[3] = 1 << 4.
 *
 * BPE_SPLIT_GPT2 is no table rule (bpe_gpu_split_rule returns BPE_GPU_EINVAL
 * for it; bpe_gpu_split_preset runs it).  Its pieces are the successive matches
 * of the bytes pattern
 *   's|'t|'re|'ve|'m|'ll|'d| ?[A-Za-z\x80-\xff]+| ?[0-9]+| ?[^\sA-Za-z0-9\x80-\xff]+|\s+(?!\S)|\s+
 * which is GPT-2's alternation with \p{L}, \p{N} and \s replaced by the byte
 * classes of BPE_SPLIT_WORDS (L letters and bytes >= 0x80, N digits, S the
 * space, W \t \n \v \f \r, P the rest, NUL and the apostrophe included; "ws" is
 * S or W).  On printable ASCII text with \t \n \v \f \r that is GPT-2's
 * alternation by construction; on any other input it is this project's
 * byte-level reading of the pattern (every byte >= 0x80 a letter, no Unicode
 * classes), and nothing more is claimed.  The contractions are lower case only.
 * As a function of the bytes around i (0 < i < n; c, p the classes of b[i],
 * b[i - 1]), with clen(j) = the length of a contraction at j: 0 unless b[j] is
 * the apostrophe, j == 0 or the class of b[j - 1] is L, N or W, and the bytes
 * after j inside the text begin with s, t, re, ve, m, ll or d; then 2 or 3:
 *   c ws:               a start if p is not ws, or if i + 1 < n and b[i + 1] is
 *                       not ws (the last white-space byte before text splits
 *                       off; a run that reaches the end stays whole);
 *   c not ws, p is S:   no start (the space belongs to what follows it);
 *   c not ws, p is W:   a start;
 *   neither is ws:      no start if clen(i - 1) >= 2 or clen(i - 2) == 3 (inside
 *                       a contraction); else a start if clen(i - 2) == 2 or
 *                       clen(i - 3) == 3 (one ended at i - 1); else c != p.
 * So a start depends on b[i - 4 .. i + 1] and on n alone.  bpe_ex.h's
 * bpe_split_offsets_host is this rule in plain C.
 *
 * BPE_SPLIT_GPT2_UNICODE is the pattern with its Unicode classes, over the text
 * decoded as UTF-8 (no table rule either).  Its pieces are the successive
 * matches of
 *   's|'t|'re|'ve|'m|'ll|'d| ?\p{L}+| ?\p{N}+| ?[^\s\p{L}\p{N}]+|\s+(?!\S)|\s+
 * reported as byte offsets, with \s Unicode White_Space (25 code points:
 * U+0009-000D, 0020, 0085, 00A0, 1680, 2000-200A, 2028, 2029, 202F, 205F, 3000;
 * not U+001C-001F) and the text decoded as Python's errors="surrogateescape"
 * does.  As a function of the bytes:
 *   Characters.  Byte i leads a character when b[i ..] inside the text begins
 *     with a well-formed UTF-8 sequence (Unicode Table 3-7: no overlong form, no
 *     surrogate, nothing above U+10FFFF, no sequence cut by n); the sequence's
 *     other bytes are its continuation bytes.  Every byte in no well-formed
 *     sequence is a character of its own with class P.  A lead byte never lies
 *     inside another sequence, so "well-formed at i" is a function of
 *     b[i .. i + 3] and n alone.
 *   Classes.  A character is S if it is U+0020, else W if it is White_Space,
 *     else L if \p{L}, else N if \p{N}, else P (csrc/unicode_classes.h: the
 *     classes of every code point, the source they came from and their digest;
 *     bpe_ex.h bpe_unicode_class / bpe_unicode_info).  K[i] is the class of the
 *     character byte i belongs to, end(i) the offset just past that character.
 *   Starts.  Byte 0 starts a piece; a continuation byte never does; any other i
 *     is decided by the BPE_SPLIT_GPT2 rule above with c = K[i], p = K[i - 1],
 *     clen(j) unchanged but for its look-back, which reads K[j - 1], and with
 *     the white-space look-ahead at end(i) in place of i + 1: c ws is a start if
 *     p is not ws, or if end(i) < n and K[end(i)] is not ws.
 * So a start depends on b[i - 7 .. i + 7] and n alone, and on a window whose
 * bytes are all below 0x80 the rule equals BPE_SPLIT_GPT2.  Where this
 * formulation and the regular expression disagree the expression is the
 * definition.
 *
 * BPE_SPLIT_CL100K is the pre-tokenizer of cl100k_base and of Llama 3 (no table
 * rule either).  Its pieces are the successive matches of
 *   (?i:'s|'t|'re|'ve|'m|'ll|'d)|[^\r\n\p{L}\p{N}]?\p{L}+|\p{N}{1,3}| ?[^\s\p{L}\p{N}]+[\r\n]*|\s*[\r\n]+|\s+(?!\S)|\s+
 * as the `regex` module (V0) finds them, reported as byte offsets, over the text
 * decoded as BPE_SPLIT_GPT2_UNICODE decodes it: the same characters (a byte in no
 * well-formed sequence is a character of class P), the same class table, and a
 * continuation byte starts nothing.  Six classes: R is \r and \n, S is U+0020,
 * W the other White_Space, L, N, and P the rest; "ws" is R, S or W.  Per
 * character, with indices that count characters, c = K[i], p = K[i - 1]:
 *   Character 0 starts a piece; before the text everything reads as R.
 *   Contractions.  The apostrophe at j opens one when K[j - 1] is L, N, R or W.
 *     clen(j) is then 2 when the next character folds to s, t, m or d, 3 when
 *     the next two fold to re, ve or ll, and 0 otherwise or when the text ends
 *     before them.  Folding maps A-Z to a-z and U+017F to s and nothing else, so
 *     a contraction is 2, 3 or (with U+017F) 3 bytes for 2 characters.
 *   c is N:   a start when (the index of i within its run of N) mod 3 is 0.
 *   c is ws, p is not:  a start, unless p is P and c is R (the newlines right
 *     after punctuation belong to its piece).
 *   c is R, p is ws:    no start.
 *   c is S or W, p is ws, q the end of this white-space run: a start when
 *     (C) i == q - 1 and q < n, or
 *     (B) p is R and no R occurs in [i, q), or
 *     (A) p is R, every character from the run's first up to i - 1 is R, and the
 *         character before the run is P.
 *   c is L, the first that fits: no start when clen(i - 1) >= 2 or
 *     clen(i - 2) == 3; a start when clen(i - 2) == 2 or clen(i - 3) == 3; no
 *     start when p is L; a start when p is N or R; no start when p is S or W
 *     (that character is the piece's prefix); when p is P, a start exactly when
 *     K[i - 2] is P or S (the P then belongs to a punctuation piece).
 *   c is P:   a start when p is L, N, R or W; no start when p is P or S.
 * Three conditions reach through runs of any length: the index in a run of N,
 * (A) back through a run of R, (B) ahead through white space.  The rest depends
 * on b[i - 8 .. i + 7] and n.  Where this formulation and the regular expression
 * disagree the expression is the definition.  bpe_ex.h's bpe_split_offsets_host
 * is this rule in plain C, one pass from the left.  o200k's pattern (case classes)
 * is another pattern and not offered.
 *
 * The offsets belong to the loaded bytes.  bpe_gpu_load / _load_fd / _synth /
 * _trim, bpe_gpu_train / _train_ex and a sharded group's load, synth and train
 * on the context drop them; bpe_gpu_encode, _encode_docs, _encode_split and
 * _decode keep them (several merge lists may be encoded over one split); a new
 * bpe_gpu_split replaces them.  A call that needs them and finds none returns
 * BPE_GPU_ESTATE.
 * ---------------------------------------------------------------------- */
enum { BPE_SPLIT_LINES = 0, BPE_SPLIT_WORDS = 1, BPE_SPLIT_GPT2 = 2, BPE_SPLIT_GPT2_UNICODE = 4, BPE_SPLIT_CL100K = 6 }; /* (3 and 5 are no presets) */
/* bytes one workgroup of the split kernels handles per step, and the largest grid
   (a corpus of more than TILE * GRID bytes is walked in grid strides) */
#define BPE_GPU_SPLIT_TILE 4096
#define BPE_GPU_SPLIT_GRID 2048
/* fill cls[256] / brk[16] with a table preset (pure function, no GPU); BPE_SPLIT_GPT2, BPE_SPLIT_GPT2_UNICODE and
   BPE_SPLIT_CL100K have no tables: BPE_GPU_EINVAL */
int bpe_gpu_split_rule(int preset, uint8_t *cls, uint16_t *brk);
/* out4 = {BPE_GPU_SPLIT_TILE, BPE_GPU_SPLIT_TILE * BPE_GPU_SPLIT_GRID, 0, 0} (pure function, no GPU) */
int bpe_gpu_split_info(uint64_t *out4);
/* split the loaded bytes; *ndocs = pieces.  A cls entry above 15 is BPE_GPU_EINVAL. */
int bpe_gpu_split(bpe_gpu_ctx *ctx, const uint8_t *cls, const uint16_t *brk, size_t *ndocs);
/* the same by a preset: BPE_SPLIT_LINES / BPE_SPLIT_WORDS are bpe_gpu_split with their tables, BPE_SPLIT_GPT2,
   BPE_SPLIT_GPT2_UNICODE and BPE_SPLIT_CL100K mark the starts with kernels of their own; the offsets and all that is said of them above are the same.
   BPE_GPU_EINVAL for another preset, BPE_GPU_ESTATE before a load. */
int bpe_gpu_split_preset(bpe_gpu_ctx *ctx, int preset, size_t *ndocs);
/* the last split's offsets; out may be NULL, *count = ndocs + 1 */
int bpe_gpu_fetch_split_offsets(bpe_gpu_ctx *ctx, uint64_t *out, size_t cap, size_t *count);
/* bpe_gpu_encode_docs over the last split's offsets (resident: neither checked nor uploaded);
   bpe_gpu_fetch_ids / _fetch_ids_range / _ids_checksum / _fetch_doc_offsets / _docs_info / _get_stats
   serve what bpe_gpu_encode_docs leaves for the same offsets */
int bpe_gpu_encode_split(bpe_gpu_ctx *ctx, const uint32_t *pairs, size_t n_merges);

/* ------------------------------------------------------------------------
 * Training on the pieces of the last split: merges that never cross a piece
 * boundary, the list bpe_gpu_encode_split can apply in full.
 *
 * The corpus is the multiset of pieces, each its bytes as ids 0..255.
 * count(a, b) is the number of positions, over all pieces, where a is followed
 * by b inside one piece.  Merge r takes the pair with the largest count, ties to
 * the smaller a and then the smaller b, gives it the id 256 + r and applies it
 * inside every piece from left to right (a run a a a under (a, a) becomes z a; a
 * run ends with its piece).  Training stops when no pair is left or the largest
 * count is <= 1 (stop_reason 1, checked first), when max_merges merges are made
 * (2; max_merges < 0: no cap of the caller's), or at the engine's own cap (3), as
 * bpe_gpu_stats.stop_reason counts them.  The resident bytes, the split's
 * offsets and the ids of an earlier encode stay as they are.
 *
 * The results (merges, the info fields, the piece table) belong to the split's
 * offsets and go with them: whatever drops those (above) drops these, and so
 * does a new bpe_gpu_split.  A call that needs them and finds none returns
 * BPE_GPU_ESTATE.
 * ---------------------------------------------------------------------- */
/* BPE_GPU_ESTATE before a load or without a split of the loaded bytes */
int bpe_gpu_train_split(bpe_gpu_ctx *ctx, long max_merges, size_t *n_merges);
/* the merges of the last bpe_gpu_train_split as (a, b) pairs; out may be NULL, *count = merges */
int bpe_gpu_fetch_split_merges(bpe_gpu_ctx *ctx, uint32_t *out, size_t cap, size_t *count);
/* out8 = {pieces, entries (distinct pieces; one per piece longer than the next-to-last field), bytes of the
   entries, pieces longer than that, merges, stop_reason, the longest piece that is deduplicated, slots of
   the piece table} */
int bpe_gpu_train_split_info(bpe_gpu_ctx *ctx, uint64_t *out8);
/* the entries in start order: the start of the first piece with these bytes, their length and how many
   pieces hold them; any of the three arrays may be NULL, *entries = their number */
int bpe_gpu_fetch_piece_table(bpe_gpu_ctx *ctx, uint64_t *start, uint32_t *len, uint32_t *count, size_t cap,
                              size_t *entries);

/* ------------------------------------------------------------------------
 * Special tokens: literals such as <|endoftext|> that are found in the raw
 * bytes before the rule runs, become exactly one reserved id each, never merge
 * with their neighbours and take no part in training.  This project's
 * definition:
 *
 * The set.  S byte strings, 0 <= S <= 256, each 1..64 bytes long (64 is the
 * longest piece bpe_gpu_train_split deduplicates, so a special is always one
 * entry of the piece table) and without a NUL byte (the loaders end the text at
 * the first NUL and the decoders drop NULs).
 *
 * The overlap-free condition.  No special is a substring of another (which
 * makes them distinct), and no non-empty proper suffix of a special is a prefix
 * of a special, the same one included ("aa" is refused).  Two occurrences of
 * specials in a text then never overlap and never start at the same byte, so
 * "all occurrences" is a pure function of at most 64 bytes from each position
 * and equals the successive matches of the alternation of the specials in any
 * list order.  <|endoftext|>, the ChatML markers and <|reserved_special_token_N|>
 * satisfy it.  Any other set is BPE_GPU_EINVAL, the message naming the pair
 * (bpe_ex.h bpe_specials_check); leftmost / list-order matching of overlapping
 * sets is not offered.
 *
 * The split.  Every occurrence [s, e) of a special in the loaded bytes is one
 * piece.  Each maximal stretch between two matches (and from byte 0 to the first,
 * from the last to n) is a segment, split by the rule as a text of its own with
 * its offsets shifted by its start.  For a table rule a piece therefore starts
 * at every s and every e < n, none inside a match, and every other byte is
 * decided as without specials.  For BPE_SPLIT_GPT2 the bytes near a match read
 * differently: looking back from byte i, everything at or before the nearest
 * match byte reads as a newline; looking ahead, a match byte reads as a space, as
 * the bytes at and past n do.  Only positions s - 1 and e .. e + 3 can differ
 * from the marks without specials.  BPE_SPLIT_GPT2_UNICODE reads the bytes near
 * a match the same way, before decoding (a sequence a match cuts is ill-formed);
 * there positions s - 7 .. s - 1 and e .. e + 6 can differ.  BPE_SPLIT_CL100K
 * reads them the same way again; a match thereby ends every run: the numbers
 * after it count from it, the newlines after it follow no P, and white space
 * before it has no newline beyond it.  No fixed set of positions bounds what can
 * differ there, so its marking pass reads the matches itself.  With S == 0 the offsets are those of
 * bpe_gpu_split / bpe_gpu_split_preset.
 *
 * Ids.  Special j (the caller's list order) has the id 256 + n_merges + j for
 * the merge list of the call at hand.  bpe_gpu_encode_split after such a split
 * leaves exactly that one id for a special piece, counted by the id offsets;
 * every other piece encodes as without specials.  bpe_gpu_train_split leaves
 * the special pieces out of the corpus: they add no pair and the piece table
 * does not list them; out8[0] stays the split's piece count.
 * bpe_gpu_decode_docs_special expands an id in [256 + n_merges, 256 + n_merges +
 * S) to its special's bytes; larger ids remain unknown.
 *
 * The specials and the list of special pieces belong to the split's offsets:
 * what drops those drops these, and a bpe_gpu_split or bpe_gpu_split_preset
 * afterwards is a split without specials.
 * ---------------------------------------------------------------------- */
#define BPE_GPU_SPECIAL_MAX_COUNT 256
#define BPE_GPU_SPECIAL_MAX_LEN 64
/* special j is bytes[len[0] + .. + len[j - 1] ..] of len[j] bytes */
typedef struct {
    const uint8_t *bytes;
    const uint32_t *len;
    size_t count;
} bpe_gpu_specials;
/* split the loaded bytes by a preset, or with preset < 0 by the tables cls / brk (ignored otherwise), around
   the specials (NULL or count 0: exactly bpe_gpu_split / bpe_gpu_split_preset).  BPE_GPU_EINVAL, before any
   launch, for a set that breaks the limits or the overlap-free condition. */
int bpe_gpu_split_special(bpe_gpu_ctx *ctx, int preset, const uint8_t *cls, const uint16_t *brk,
                          const bpe_gpu_specials *specials, size_t *ndocs);
/* out4 = {S, matches, passes of the find kernel (2 when the match list had to grow), entries the match list
   holds} of the last split (zeros after one without specials) */
int bpe_gpu_split_special_info(bpe_gpu_ctx *ctx, uint64_t *out4);
/* the special pieces of the last split in order: the piece's index among the offsets and the special's index;
   either array may be NULL, *count = matches */
int bpe_gpu_fetch_special_pieces(bpe_gpu_ctx *ctx, uint64_t *piece, uint32_t *index, size_t cap, size_t *count);
/* bpe_gpu_decode_docs with specials.  id_off may be NULL with ndocs == 0: the ids are one flat sequence
   (bpe_gpu_decode) and byte_off is not written. */
int bpe_gpu_decode_docs_special(bpe_gpu_ctx *ctx, const uint32_t *ids, size_t len, const uint64_t *id_off,
                                size_t ndocs, const uint32_t *pairs, size_t n_merges,
                                const bpe_gpu_specials *specials, uint8_t *out, size_t cap, size_t *out_len,
                                uint64_t *byte_off);

/* ------------------------------------------------------------------------
 * Vocabularies: a tokenizer's own numbering of the tokens.  The engine's ids
 * are byte b = b, merge r = 256 + r, special j = 256 + n_merges + j (the
 * internal ids).  A vocabulary gives each of them another id: pairwise distinct
 * over the three arrays, each below BPE_VOCAB_ID_LIMIT (2^24, the engine's own
 * merge cap; it bounds the inverse table at 64 MB), holes allowed.  The merge
 * list it belongs to names, for merge r, only ids below 256 + r: replaying such
 * a list in rank order (what the encoders do) is the usual lowest-rank-first BPE
 * (bpe_ex.h bpe_vocab_check).
 *
 * bpe_gpu_map_ids rewrites the resident ids in place, ids[i] = fwd[ids[i]]
 * (k_ids_map); the offsets of a document batch do not move.  The context
 * remembers that its ids are vocabulary ids: the mark goes when the ids go
 * (any load, synth, trim, encode or training that replaces them), and while it
 * stands a second bpe_gpu_map_ids is BPE_GPU_ESTATE, as is any call that would
 * read the resident ids as internal ones.  bpe_gpu_decode_docs_vocab turns the
 * caller's ids back on the device first (k_ids_unmap); an id past the inverse
 * table or in a hole is an unknown token id, BPE_GPU_EDATA.
 * ---------------------------------------------------------------------- */
#define BPE_VOCAB_ID_LIMIT (1u << 24)
typedef struct {
    const uint32_t *byte_id;    /* 256: vocabulary id of byte b            */
    const uint32_t *merge_id;   /* n_merges: vocabulary id of merge r      */
    const uint32_t *special_id; /* n_specials: vocabulary id of special j  */
    size_t n_merges, n_specials;
} bpe_gpu_vocab;
/* Rewrite the ids of the last bpe_gpu_encode / _encode_docs / _encode_split (or training) to vocabulary ids;
   bpe_gpu_fetch_ids / _fetch_ids_range / _ids_checksum / _fetch_doc_offsets serve them afterwards.
   BPE_GPU_ESTATE without resident ids or when they are mapped already; BPE_GPU_EINVAL for a vocabulary
   bpe_vocab_check refuses or whose merge count is not the encode's; BPE_GPU_EINTERNAL should an id lie at or
   above 256 + n_merges + n_specials (it is compared before the lookup and never used as an index; the ids
   are dropped then). */
int bpe_gpu_map_ids(bpe_gpu_ctx *ctx, const bpe_gpu_vocab *vocab);
/* out4 = {ids one thread moves per step, ids per workgroup step, ids per grid step, 0} of k_ids_map and
   k_ids_unmap (pure function, no GPU; for the tests) */
int bpe_gpu_map_info(uint64_t *out4);
/* bpe_gpu_decode_docs_special over vocabulary ids (specials may be NULL when vocab->n_specials == 0; the two
   counts must agree, as must vocab->n_merges and n_merges) */
int bpe_gpu_decode_docs_vocab(bpe_gpu_ctx *ctx, const uint32_t *ids, size_t len, const uint64_t *id_off, size_t ndocs,
                              const uint32_t *pairs, size_t n_merges, const bpe_gpu_specials *specials,
                              const bpe_gpu_vocab *vocab, uint8_t *out, size_t cap, size_t *out_len,
                              uint64_t *byte_off);

/* ------------------------------------------------------------------------
 * Text batches: T texts in one context, each split and encoded on its own.  (A
 * batch member is a text; "doc" keeps meaning a piece, as in bpe_gpu_encode_docs.)
 *
 * The contract.  For texts t[0 .. T) (any bytes, NUL included, length 0 allowed)
 * the pieces of text k are those of a split of t[k] alone and its ids those of an
 * encode of t[k] alone: no piece, special match, merge or UTF-8 sequence reaches
 * across the break between two texts; seen from inside a text, the break before
 * it is the start of a text and the break after it the end of one.  An empty text
 * has no piece and no id.  The batch's pieces and ids are the texts' in order;
 * text_off[0 .. T] counts the ids, text_off[0] == 0 and text_off[T] == their
 * number.  Byte offsets handed out (bpe_gpu_fetch_split_offsets) count the bytes
 * of the texts joined with nothing between them.
 *
 * How.  bpe_gpu_load_texts keeps the texts with one gap byte 0x00 after each
 * (n + T resident bytes, built on the host by bpe_ex.h bpe_texts_gap) and the
 * offsets on the device.  Every split of such a context (bpe_gpu_split,
 * _split_preset, _split_special) treats gap k, at resident position
 * text_off[k + 1] + k, as it treats a special's match: a covered byte that ends
 * the segment before it and begins one after it.  The offsets alone say where a
 * gap is; a NUL inside a text is an ordinary byte, and since no special holds a
 * NUL none matches across a gap.  In the match list a break carries the reserved
 * index 255 (BPE_GPU_TEXT_BREAK): a split of a text batch therefore takes at most
 * 255 specials, and 256 are refused with BPE_GPU_EINVAL by that name.
 * bpe_gpu_encode_split removes every id of a break piece, writes text_off where
 * they vanished and drops the break pieces from the id offsets;
 * bpe_gpu_fetch_split_offsets, _fetch_doc_offsets, _fetch_special_pieces and
 * _split_special_info report the pieces without the breaks.  bpe_gpu_map_ids
 * works as ever: no id of a break is left.
 *
 * Lifetime.  The breaks belong to the bytes: bpe_gpu_load, _load_fd, _synth and
 * _trim end the text batch.  While it stands, bpe_gpu_encode, bpe_gpu_train,
 * _train_ex, bpe_gpu_encode_docs and bpe_gpu_train_split return BPE_GPU_ESTATE
 * (they would read the gap bytes as text; training on text batches is not
 * offered).  A context loaded any other way launches what it always launched.
 * ---------------------------------------------------------------------- */
#define BPE_GPU_TEXT_BREAK 255
/* Load T texts: text k is bytes[text_off[k] .. text_off[k + 1]).  BPE_GPU_EINVAL, with the offending index in
   the message, for offsets bpe_texts_check (bpe_ex.h) refuses: the first not 0, one below the one before it,
   the last not n, or n + T above 2^32 - 2. */
int bpe_gpu_load_texts(bpe_gpu_ctx *ctx, const uint8_t *bytes, size_t n, const uint64_t *text_off, size_t T);
/* text_off of the last bpe_gpu_encode_split over a text batch; out may be NULL, *count = T + 1.
   BPE_GPU_ESTATE without a text batch or before its encode. */
int bpe_gpu_fetch_text_offsets(bpe_gpu_ctx *ctx, uint64_t *out, size_t cap, size_t *count);
/* The resident ids (mapped or not) as rows: out[T][row_len] uint32 and lens[T] uint32 (k_pack_rows).
   lens[k] = min(ids of text k, row_len); a longer text keeps its first row_len ids (side 0) or its last
   (side 1); pad_id, any uint32, fills the row behind the ids.  out_is_device != 0: out and lens are device
   pointers on the context's device (a tensor's data pointer), written on the context's stream, which is
   synchronised before the call returns; else host memory, filled through a device buffer.  lens may be NULL.
   BPE_GPU_EINVAL for row_len == 0, another side or a device pointer that is none of this device;
   BPE_GPU_ERANGE for row_len above 2^24; BPE_GPU_ESTATE without a text batch or without its ids. */
int bpe_gpu_pack_texts(bpe_gpu_ctx *ctx, uint32_t row_len, uint32_t pad_id, int side, uint32_t *out,
                       int out_is_device, uint32_t *lens);

/* ------------------------------------------------------------------------
 * Token spans: where in its text every resident id comes from.
 *
 * The contract.  For a text t (bytes) encoded to the ids x[0 .. m), token i
 * stands for the bytes t[bs_i .. be_i) with bs_0 = 0, be_i = bs_(i + 1) and
 * be_(m - 1) = len(t).  A token's length is fixed by its id: a byte is 1 (NUL
 * included, unlike the decoders' table, which drops NULs), merge r the sum of its
 * two halves, special j the length of special j.  In a text batch every text has
 * spans of its own, relative to its own first byte; an empty text has none.
 * Without a text batch the resident bytes are the one text.
 *
 * Two units.  BPE_SPAN_BYTE: (bs_i, be_i).  BPE_SPAN_CHAR: with lead(p) = the
 * number of bytes in t[0 .. p) that are no UTF-8 continuation byte
 * ((b & 0xC0) != 0x80), the span is (max(lead(bs_i + 1), 1) - 1, lead(be_i)).
 * For valid UTF-8 that is the index of the code point holding the token's first
 * byte and one past the code point holding its last, so a token that holds only
 * a part of a character reports the whole character, as Encoding.offsets of the
 * `tokenizers` library does (for a tokenizer.json without a post-processor;
 * trim_offsets belongs to a ByteLevel post-processor, which is not applied).  For
 * bytes that are no UTF-8 the formula is the definition; the max keeps a text
 * that begins with a continuation byte at 0.  Spans are uint32 pairs.
 *
 * bpe_gpu_token_spans computes them on the device (spans.hip) from a length
 * table built on the host (bpe_ex.h bpe_span_lens) and keeps them in HBM.  They
 * live as long as the ids they describe and go where those go; a later
 * bpe_gpu_map_ids does not touch them (numbering is not position).
 * ---------------------------------------------------------------------- */
#define BPE_SPAN_BYTE 0
#define BPE_SPAN_CHAR 1
/* The spans of the resident ids of the last bpe_gpu_encode_split / bpe_gpu_encode_docs, with or without a text
   batch, before or after bpe_gpu_map_ids: mapped ids need `vocab` (the table is then in its numbering), unmapped
   ids with one are BPE_GPU_ESTATE, as are mapped ids without, no such ids, and the ids of bpe_gpu_encode or a
   training.  specials: those of the split (NULL: none).  BPE_GPU_EINVAL when n_merges is not the encode's, for
   another unit, a list bpe_span_lens refuses or a vocabulary bpe_vocab_check refuses.  BPE_GPU_EDATA, nothing
   kept, for an id outside the table ("spans: unknown token id") and when the lengths do not sum to the bytes of
   the texts ("... not the merge list of this encode"); the context goes on as it was. */
int bpe_gpu_token_spans(bpe_gpu_ctx *ctx, const uint32_t *pairs, size_t n_merges, const bpe_gpu_specials *specials,
                        const bpe_gpu_vocab *vocab, int unit);
/* the spans, out[2 i] and out[2 i + 1] for id i; out may be NULL, *count = the ids, at most cap spans are
   written.  BPE_GPU_ESTATE without spans. */
int bpe_gpu_fetch_token_spans(bpe_gpu_ctx *ctx, uint32_t *out, size_t cap, size_t *count);
/* The spans of a text batch as rows: out[T][row_len][2] uint32, cut as bpe_gpu_pack_texts cuts the ids (the same
   side, the same lens), the cells behind the ids (0, 0).  With side 1 the spans stay relative to the whole
   text: they are not rebased to the cut.  out_is_device as bpe_gpu_pack_texts; a device pointer must be 8-byte
   aligned.  Refusals as bpe_gpu_pack_texts; BPE_GPU_ESTATE without a text batch or without spans. */
int bpe_gpu_pack_spans(bpe_gpu_ctx *ctx, uint32_t row_len, int side, uint32_t *out, int out_is_device);
/* out4 = {ids one thread of k_spans takes per step, ids per workgroup step, ids per grid step, bytes per grid
   step of k_span_lead} (pure function, no GPU; for the tests) */
int bpe_gpu_span_info(uint64_t *out4);

/* ------------------------------------------------------------------------
 * Packed streams: a text batch's ids as training rows.
 *
 * The contract.  Given the resident ids x[0 .. n) of a text batch (mapped or
 * not), their text_off[0 .. T], a row length L (1 <= L <= 2^24), an optional BOS
 * id and an optional EOS id (any uint32, not checked against a vocabulary), a pad
 * id and a drop_last flag; b = 1 with a BOS, else 0, e the same for the EOS,
 * w = b + e.
 *
 * The stream: for k = 0 .. T - 1 in order, [bos] if b, then
 * x[text_off[k] .. text_off[k + 1]), then [eos] if e.  An empty text contributes
 * its BOS and EOS like any other; with w == 0 it contributes nothing.  Text k
 * starts at stream position S[k] = text_off[k] + k w, and the stream has
 * N = n + T w cells.
 *
 * The rows: R = N / L, rounded down with drop_last and up without (so R == 0
 * when N == 0, and with drop_last when N < L).  For cell c = r L + col:
 *   rows[c] = stream[c] for c < N, else pad_id;
 *   seg[c]  = k, the index of cell c's text in the batch, for c < N, else
 *             BPE_STREAM_NO_TEXT (0xFFFFFFFF);
 *   pos[c]  = c - max(S[k], r L) for c < N, else 0: it counts from the text's
 *             first cell (its BOS if there is one) or, for a text that began in
 *             an earlier row, from the row's first cell, so the cells of one seg
 *             value inside one row count 0, 1, 2, ...
 * Nothing is truncated and only the last row holds pad cells.  seg (for a
 * block-diagonal attention mask) and pos (for position ids) are optional.
 *
 * bpe_gpu_pack_stream computes the rows on the device (stream.hip) from what
 * bpe_gpu_encode_split left resident: text_off is a prefix sum already, so S has
 * the closed form above and no scan runs.  bpe_ex.h bpe_pack_stream_host is the
 * same in plain loops.
 * ---------------------------------------------------------------------- */
#define BPE_STREAM_BOS 1u        /* flags: bos_id opens every text */
#define BPE_STREAM_EOS 2u        /* ... eos_id closes every text */
#define BPE_STREAM_DROP_LAST 4u  /* ... a last row that the stream does not fill is dropped, not padded */
#define BPE_STREAM_FLAGS 7u
#define BPE_STREAM_SEQ_MAX (1u << 24)
#define BPE_STREAM_NO_TEXT 0xFFFFFFFFu
typedef struct {
    uint32_t seq_len, flags, bos_id, eos_id, pad_id;
} bpe_gpu_stream;
/* The rows of the resident text batch: rows[R][seq_len] uint32, and seg and pos of the same shape unless NULL.
   rows == NULL is the query: *n_rows = R and *n_stream = N are reported and nothing is launched (both may be
   NULL).  rows_cap: the rows that rows, seg and pos each have room for.  out_is_device as bpe_gpu_pack_texts:
   != 0: device pointers on the context's device, written on the context's stream, which is synchronised before
   the call returns; else host memory, filled through a device buffer.
   BPE_GPU_EINVAL for seq_len == 0, an unknown flag bit, rows_cap < R, a device pointer that is none of the
   context's device or not 4-byte aligned; BPE_GPU_ERANGE for seq_len above 2^24; BPE_GPU_ESTATE without a text
   batch or without its ids.  The message names the cause, and the context goes on working. */
int bpe_gpu_pack_stream(bpe_gpu_ctx *ctx, const bpe_gpu_stream *s, uint32_t *rows, uint32_t *seg, uint32_t *pos,
                        int out_is_device, size_t rows_cap, size_t *n_rows, uint64_t *n_stream);
/* out4 = {cells one lane of k_pack_stream<true> takes per step, cells per workgroup step (a tile), cells the largest
   grid takes in one step (past that many cells a workgroup takes several consecutive tiles), texts a lane walks
   forward before it searches for itself}; k_pack_stream<false> takes a quarter of the first three (pure function,
   no GPU; for the tests) */
int bpe_gpu_stream_info(uint64_t *out4);

/* ------------------------------------------------------------------------
 * Rows back to texts: the ids of a [B, L] grid of cells, as a model hands it
 * back, cut to the text of every row and decoded; the inverse of
 * bpe_gpu_pack_texts.  No id passes through the host.
 *
 * The contract.  rows[B][L] is a grid of cells of cell_bytes = 4 or 8 bytes; row
 * k begins row_stride cells after row k - 1 (row_stride >= L, so a column slice
 * of a contiguous tensor is taken as it lies).  0 <= L <= 2^24; B is any count for
 * which B * row_stride cells can be addressed.  A 4-byte cell is an id.  An 8-byte
 * cell is a signed 64-bit value and an id only when it lies in 0 .. 2^32 - 1; no
 * other value equals a pad, stop or skip id.
 *
 * The window of row k is the cells [0, lens[k]) with lens (uint32[B]), else
 * [0, L).  lens[k] > L is BPE_GPU_EINVAL; the message names the lowest such row.
 *
 * The start a_k: with BPE_ROWS_PAD the number of leading window cells equal to
 * pad_id, else 0.  The end z_k: the first cell c >= a_k of the window whose value
 * is one of stop[0 .. n_stop) or, with BPE_ROWS_PAD, pad_id; the window's end when
 * there is none.  The stop cell is not part of the text.  "Leading pads, then the
 * first stop or pad" reads left-padded rows with pad_id == eos_id as they are
 * meant; a text whose first token is the pad id loses it (and a text that is
 * nothing else is empty).
 *
 * The kept cells of row k are the cells of [a_k, z_k) in order, without those
 * whose id is in skip[0 .. n_skip) under BPE_ROWS_SKIP.  A kept 8-byte cell outside
 * 0 .. 2^32 - 1 is BPE_GPU_EDATA; the message names the lowest such row.  A cell
 * outside [a_k, z_k) is never judged, whatever it holds (an ignore index of -100,
 * garbage behind the EOS), nor is a skipped one.
 *
 * The results: ids uint32[n], the kept cells of all rows joined; text_off
 * uint64[B + 1], row k's ids being ids[text_off[k] .. text_off[k + 1]); bounds
 * uint32[B][2] = (a_k, z_k), so z_k - a_k is the length of what row k generated.
 * bpe_gpu_unpack_rows computes them on the device (rows.hip) and keeps them in
 * scratch slots of their own: they disturb no resident ids of an encode and no
 * encode, load or decode disturbs them; bpe_gpu_trim drops them.
 * bpe_gpu_decode_rows decodes them as bpe_gpu_decode_docs_vocab / _special /
 * bpe_gpu_decode_docs would decode ids and text_off fetched and handed back (NUL
 * bytes dropped; an id the list or the vocabulary does not hold is BPE_GPU_EDATA
 * "unknown token id", which only a kept cell can raise).  bpe_ex.h
 * bpe_unpack_rows_host is the same in plain loops.
 * ---------------------------------------------------------------------- */
#define BPE_ROWS_PAD 1u   /* flags: pad_id counts */
#define BPE_ROWS_SKIP 2u  /* ... the skip list counts */
#define BPE_ROWS_FLAGS 3u
#define BPE_ROWS_LEN_MAX (1u << 24)
#define BPE_ROWS_STOP_MAX 8
#define BPE_ROWS_SKIP_MAX 256
typedef struct {
    uint32_t flags, pad_id;
    uint32_t n_stop, stop[BPE_ROWS_STOP_MAX];
    uint32_t n_skip;
    const uint32_t *skip; /* n_skip ids in any order, duplicates allowed (the library sorts a copy); read under BPE_ROWS_SKIP */
} bpe_gpu_rows;
/* Unpack rows[B][L] (cells of cell_bytes, row_stride cells from row to row) as `desc` says and keep ids, text_off
   and bounds on the device; *n = the ids.  rows_is_device != 0: a device pointer on the context's device (a tensor's
   data pointer), aligned to its cell size, read on the context's stream; else host memory, uploaded row by row
   (a 2-D copy that honours row_stride).  lens (may be NULL) and lens_is_device the same for the windows.
   BPE_GPU_EINVAL for what bpe_rows_check (bpe_ex.h) refuses, another cell_bytes, row_stride < L, a device pointer
   that is none of the context's device or not aligned, and lens[k] > L; BPE_GPU_ERANGE for L above 2^24;
   BPE_GPU_EDATA for a kept 8-byte cell that is no id.  After a refusal nothing is kept (bpe_gpu_fetch_rows and
   bpe_gpu_decode_rows return BPE_GPU_ESTATE) and the context goes on working. */
int bpe_gpu_unpack_rows(bpe_gpu_ctx *ctx, const void *rows, int rows_is_device, int cell_bytes, size_t B, uint32_t L,
                        size_t row_stride, const uint32_t *lens, int lens_is_device, const bpe_gpu_rows *desc, size_t *n);
/* The last unpack's results.  Two-phase: *n = the ids and *B = the rows are always reported (each may be NULL);
   ids (ids_cap entries of room), text_off (B_cap + 1) and bounds (2 * B_cap) are each written unless NULL.
   BPE_GPU_EINVAL for ids_cap < n with ids, B_cap < B with text_off or bounds; BPE_GPU_ESTATE without an unpack. */
int bpe_gpu_fetch_rows(bpe_gpu_ctx *ctx, uint32_t *ids, size_t ids_cap, size_t *n, uint64_t *text_off, uint32_t *bounds,
                       size_t B_cap, size_t *B);
/* Decode the last unpack's ids, row by row: out[byte_off[k] .. byte_off[k + 1]) is row k's text (byte_off: B + 1
   entries, may be NULL).  specials and vocab may each be NULL: with a vocabulary the ids are its ids, checked as
   bpe_gpu_decode_docs_vocab checks them; without, internal ids.  Two-phase as the decoders: out == NULL reports
   *out_len alone.  The unpacked ids stay as they are and can be fetched or decoded again.  BPE_GPU_ESTATE when
   nothing has been unpacked. */
int bpe_gpu_decode_rows(bpe_gpu_ctx *ctx, const uint32_t *pairs, size_t n_merges, const bpe_gpu_specials *specials,
                        const bpe_gpu_vocab *vocab, uint8_t *out, size_t cap, size_t *out_len, uint64_t *byte_off);
/* out4 = {cells one lane of the vector variants (k_rows_bounds / k_rows_gather <., true>) takes per step, cells a wave
   takes per step then (a wave owns a row; the one-cell variants take a quarter), rows per workgroup, rows the largest
   grid takes in one step (more rows: a wave goes on to further rows)} (pure function, no GPU; for the tests) */
int bpe_gpu_rows_info(uint64_t *out4);

int bpe_gpu_get_stats(bpe_gpu_ctx *ctx, bpe_gpu_stats *st);

/* Position-keyed checksum of the ids of the last train / encode, computed in
 * HBM: sum over i of mix64(mix64(base + i) ^ ids[i]) mod 2^64 (mix64 = the
 * splitmix64 / murmur3 fmix64 finalizer).  A sequence held in pieces sums to
 * the checksum of the whole when each piece passes its global start index. */
int bpe_gpu_ids_checksum(bpe_gpu_ctx *ctx, uint64_t base, uint64_t *sum);

/* device pointer of the loaded corpus bytes / ids (for in-HBM benchmarking) */
int bpe_gpu_device_tokens(bpe_gpu_ctx *ctx, const void **dev_tok, size_t *n);

/* Record HIP events around every k_scan node of the iteration graphs (the
 * dominant kernel of the merge loop) during the next train() calls. */
int bpe_gpu_set_profile(bpe_gpu_ctx *ctx, int on);

/* Average duration (ms) of the engine's dominant kernel (k_scan) over the
 * last train call, measured live with the device wall clock (block 0 entry to
 * the last block's exit; no effect on the run), and its algorithmic bytes per
 * launch (bench.py's roofline object). */
int bpe_gpu_kernel_profile(bpe_gpu_ctx *ctx, const char **name, double *avg_ms,
                           double *bytes_per_launch, uint64_t *launches);

/* Average k_scan duration from HIP event-record nodes spliced around every
 * k_scan node of the iteration graphs (only when bpe_gpu_set_profile(1) was
 * set for the last train call; the event nodes slow the loop down). */
int bpe_gpu_event_profile(bpe_gpu_ctx *ctx, double *avg_ms, uint64_t *launches);

/* ------------------------------------------------------------------------
 * Sharded training.  The corpus is cut into contiguous
 * shards in order; shard s holds bytes [off_s, off_s + n_s).  Every shard
 * keeps the replicated pair-count table; per merge the shards allreduce the
 * count deltas and allgather 16-word edge records (pairs across an edge
 * belong to the left shard).  Merges are identical on every shard; the
 * global ids are the concatenation of the shards' ids.
 *
 * Two kinds of group:
 *   comm_id == NULL: `local_shards` shards on one device (nranks must be 1);
 *   comm_id != NULL: one shard per rank, ranks exchange over RCCL (xGMI);
 *                    comm_id = the 128-byte id rank 0 got from
 *                    bpe_gpu_comm_id(), passed to every rank.
 * and bpe_gpu_group_create_p2p: one shard per rank, each exchange is one
 * push kernel over xGMI into the peers' IPC-mapped mailboxes (no RCCL on the
 * per-merge path).  Every rank creates its group, the host side gathers the
 * BPE_GPU_P2P_HANDLE_BYTES handles in rank order (any host collective) and
 * passes them to bpe_gpu_group_p2p_connect.  max_merges bounds the merges a
 * train call may make (it sizes the mailbox).  A rank that waits longer than
 * BPE_P2P_TIMEOUT_S seconds (default 30) for a peer fails with
 * BPE_GPU_EINTERNAL instead of hanging.
 * ---------------------------------------------------------------------- */
#define BPE_GPU_P2P_HANDLE_BYTES 64
#define BPE_GPU_P2P_MAX_RANKS 16
typedef struct bpe_gpu_group bpe_gpu_group;

int bpe_gpu_comm_id(uint8_t *id, size_t cap);
int bpe_gpu_group_create(int device, int local_shards, int nranks, int rank, const uint8_t *comm_id,
                         bpe_gpu_group **out);
int bpe_gpu_group_create_p2p(int device, int nranks, int rank, long max_merges, uint8_t *handle, size_t cap,
                             bpe_gpu_group **out);
int bpe_gpu_group_p2p_connect(bpe_gpu_group *g, const uint8_t *handles, size_t each);
/* One process, several devices: nranks P2P groups (rank r on devices[r]; a
 * device may repeat) connected through direct pointers to each other's
 * mailboxes (peer access between distinct devices) instead of IPC handles.
 * out[r] receives rank r's group (at most 3 ranks per device: ranks sharing
 * a device need hardware queues of their own).  Each group must then be driven by a host
 * thread of its own (the ranks' kernels wait for each other's pushes), e.g.
 * bpe_train_bytes_devices (bpe_ex.h). */
int bpe_gpu_group_create_local_p2p(int nranks, const int *devices, long max_merges, bpe_gpu_group **out);
void bpe_gpu_group_destroy(bpe_gpu_group *g);
int bpe_gpu_group_shards(bpe_gpu_group *g, int *local_shards, int *nshards, int *first_shard);
/* shard k (local index) of the group */
int bpe_gpu_group_load(bpe_gpu_group *g, int k, const uint8_t *bytes, size_t n);
int bpe_gpu_group_synth(bpe_gpu_group *g, int k, uint64_t seed, size_t n, uint64_t offset);
int bpe_gpu_group_train(bpe_gpu_group *g, long max_merges, size_t *n_merges);
/* Encode the shards' bytes with a merge list (ids 256 + r); the corpus ids are
 * the shards' ids (bpe_gpu_group_fetch_ids) concatenated.  Exact across
 * shard edges; a group of several shards on one device encodes corpora
 * larger than 4 GiB. */
int bpe_gpu_group_encode(bpe_gpu_group *g, const uint32_t *pairs, size_t n_merges);
int bpe_gpu_group_fetch_merges(bpe_gpu_group *g, uint32_t *pairs, size_t cap, size_t *count);
int bpe_gpu_group_fetch_ids(bpe_gpu_group *g, int k, uint32_t *ids, size_t cap, size_t *len);
/* ids [first, first + count) of local shard k (ranged reads of huge outputs) */
int bpe_gpu_group_fetch_ids_range(bpe_gpu_group *g, int k, size_t first, uint32_t *ids, size_t count);
int bpe_gpu_group_get_stats(bpe_gpu_group *g, bpe_gpu_stats *st);
/* bpe_gpu_ids_checksum over the group's local shards in order (the first
 * starting at global index `base`); *n_ids = the local ids counted */
int bpe_gpu_group_ids_checksum(bpe_gpu_group *g, uint64_t base, uint64_t *sum, uint64_t *n_ids);
/* bpe_gpu_kernel_profile of local shard k after a group train */
int bpe_gpu_group_kernel_profile(bpe_gpu_group *g, int k, const char **name, double *avg_ms,
                                 double *bytes_per_launch, uint64_t *launches);
/* 1 when the per-merge exchange runs inside captured HIP graphs */
int bpe_gpu_group_exchange_mode(bpe_gpu_group *g, int *graph_captured);
/* transport of the exchange: 0 one device, 1 RCCL, 2 P2P mailboxes */
int bpe_gpu_group_transport(bpe_gpu_group *g, int *kind);

/* The halo shard `me` derives from all edge records for a merge (a, b):
 * out8 = {HL[0..2], HR[0..2], hlrun, myidx} (pure function, no GPU; exported
 * for the host-side protocol tests). */
int bpe_gpu_shard_halo(const uint32_t *records, uint32_t nshards, uint32_t me, uint32_t a, uint32_t *out8);

const char *bpe_gpu_strerror(int code);
const char *bpe_gpu_last_error(void);

#ifdef __cplusplus
}
#endif
#endif

/* Stand-alone sanitizer check of the preset rules' host code (src/bpe_split_preset.c:
 * bpe_split_offsets_host, bpe_encode_split_preset, bpe_train_split_preset, and the
 * bodies in src/bpe_docs.c and src/bpe_train_split.c they run): built with
 * -fsanitize=address,undefined against a HOST MODEL of the engine calls (below:
 * load keeps a copy of the bytes, split_preset takes its offsets from
 * bpe_split_offsets_host, encode_split emits one id per byte, train_split
 * returns two fixed merges).  Test infrastructure only; `make asan-split-preset`,
 * run by tests/test_asan_split_preset.py.  Exits 0 and prints
 * "asan_split_preset: ok". */
#include "../../include/bpe_ex.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

struct bpe_gpu_ctx {
    uint8_t *bytes;
    size_t n;
    uint64_t *off; /* the split's offsets, NULL when there are none */
    size_t ndocs;
    int encoded, trained;
};

static int g_fail_split; /* the model's bpe_gpu_split_preset fails once armed */
static int g_fail_train; /* ... its bpe_gpu_train_split */
static int g_fail_fetch; /* ... its bpe_gpu_fetch_split_merges */
static int g_live;       /* contexts alive */

static void drop(bpe_gpu_ctx *c)
{
    free(c->bytes);
    free(c->off);
    c->bytes = NULL;
    c->off = NULL;
    c->n = c->ndocs = 0;
    c->encoded = c->trained = 0;
}

int bpe_gpu_create(int device, bpe_gpu_ctx **out)
{
    (void)device;
    *out = calloc(1, sizeof **out);
    if (!*out) return BPE_GPU_ENOMEM;
    g_live++;
    return 0;
}
void bpe_gpu_destroy(bpe_gpu_ctx *c)
{
    if (!c) return;
    drop(c);
    free(c);
    g_live--;
}
int bpe_gpu_trim(bpe_gpu_ctx *c) { drop(c); return 0; }
int bpe_gpu_load(bpe_gpu_ctx *c, const uint8_t *b, size_t n)
{
    drop(c);
    c->bytes = malloc(n ? n : 1);
    if (!c->bytes) return BPE_GPU_ENOMEM;
    if (n) memcpy(c->bytes, b, n);
    c->n = n;
    return 0;
}
int bpe_gpu_split_preset(bpe_gpu_ctx *c, int preset, size_t *ndocs)
{
    if (g_fail_split) return BPE_GPU_EHIP;
    size_t cnt = 0;
    int rc = bpe_split_offsets_host(preset, c->bytes, c->n, NULL, 0, &cnt);
    if (rc) return rc;
    free(c->off);
    c->trained = 0;
    c->off = malloc(cnt * sizeof(uint64_t)); /* exactly the count: a write past it is reported */
    if (!c->off) return BPE_GPU_ENOMEM;
    if ((rc = bpe_split_offsets_host(preset, c->bytes, c->n, c->off, cnt, &cnt))) return rc;
    *ndocs = c->ndocs = cnt - 1;
    return 0;
}
int bpe_gpu_encode_split(bpe_gpu_ctx *c, const uint32_t *p, size_t n)
{
    (void)p; (void)n;
    if (!c->off) return BPE_GPU_ESTATE;
    c->encoded = 1;
    return 0;
}
int bpe_gpu_fetch_ids(bpe_gpu_ctx *c, uint32_t *ids, size_t cap, size_t *len)
{
    if (!c->encoded) return BPE_GPU_ESTATE;
    *len = c->n;
    for (size_t i = 0; ids && i < c->n && i < cap; i++) ids[i] = c->bytes[i];
    return 0;
}
static int copy_off(bpe_gpu_ctx *c, uint64_t *out, size_t cap, size_t *count)
{
    if (!c->off) return BPE_GPU_ESTATE;
    *count = c->ndocs + 1;
    for (size_t i = 0; out && i <= c->ndocs && i < cap; i++) out[i] = c->off[i];
    return 0;
}
/* one id per byte: the id offsets are the byte offsets */
int bpe_gpu_fetch_doc_offsets(bpe_gpu_ctx *c, uint64_t *out, size_t cap, size_t *count)
{
    return c->encoded ? copy_off(c, out, cap, count) : BPE_GPU_ESTATE;
}
int bpe_gpu_fetch_split_offsets(bpe_gpu_ctx *c, uint64_t *out, size_t cap, size_t *count) { return copy_off(c, out, cap, count); }
/* two fixed merges, or as many as the cap allows */
static const uint32_t MODEL_MERGES[4] = {'a', 'b', 256, 'c'};
static size_t model_k(long max_merges) { return max_merges < 0 || max_merges > 2 ? 2 : (size_t)max_merges; }
int bpe_gpu_train_split(bpe_gpu_ctx *c, long max_merges, size_t *n_merges)
{
    if (g_fail_train) return BPE_GPU_EHIP;
    if (!c->off) return BPE_GPU_ESTATE;
    c->trained = 1 + (int)model_k(max_merges);
    *n_merges = model_k(max_merges);
    return 0;
}
int bpe_gpu_fetch_split_merges(bpe_gpu_ctx *c, uint32_t *out, size_t cap, size_t *count)
{
    if (g_fail_fetch) return BPE_GPU_EHIP;
    if (!c->trained) return BPE_GPU_ESTATE;
    *count = (size_t)c->trained - 1;
    for (size_t i = 0; out && i < *count && i < cap; i++) out[2 * i] = MODEL_MERGES[2 * i], out[2 * i + 1] = MODEL_MERGES[2 * i + 1];
    return 0;
}
int bpe_gpu_get_stats(bpe_gpu_ctx *c, bpe_gpu_stats *st)
{
    memset(st, 0, sizeof *st);
    st->n_in = st->n_out = c->n;
    return 0;
}
const char *bpe_gpu_strerror(int code) { (void)code; return "host model"; }
const char *bpe_gpu_last_error(void) { return "host model"; }

/* the rest of what bpe.c, bpe_docs.c and bpe_train_split.c link against: not reached here */
#define UNUSED_CALL(name, ...) int name(__VA_ARGS__) { return BPE_GPU_ENODEV; }
UNUSED_CALL(bpe_gpu_split, bpe_gpu_ctx *c, const uint8_t *cls, const uint16_t *brk, size_t *nd)
UNUSED_CALL(bpe_gpu_load_fd, bpe_gpu_ctx *c, int fd, size_t s, size_t *n)
UNUSED_CALL(bpe_gpu_train, bpe_gpu_ctx *c, long m, size_t *n)
UNUSED_CALL(bpe_gpu_fetch_merges, bpe_gpu_ctx *c, uint32_t *p, size_t cap, size_t *n)
UNUSED_CALL(bpe_gpu_encode, bpe_gpu_ctx *c, const uint32_t *p, size_t n)
UNUSED_CALL(bpe_gpu_decode, bpe_gpu_ctx *c, const uint32_t *ids, size_t len, const uint32_t *p, size_t n, uint8_t *out,
            size_t cap, size_t *olen)
UNUSED_CALL(bpe_gpu_encode_docs, bpe_gpu_ctx *c, const uint64_t *o, size_t nd, const uint32_t *p, size_t n)
UNUSED_CALL(bpe_gpu_decode_docs, bpe_gpu_ctx *c, const uint32_t *ids, size_t len, const uint64_t *io, size_t nd,
            const uint32_t *p, size_t n, uint8_t *out, size_t cap, size_t *olen, uint64_t *bo)
UNUSED_CALL(bpe_gpu_group_create_local_p2p, int nr, const int *d, long m, bpe_gpu_group **out)
UNUSED_CALL(bpe_gpu_group_load, bpe_gpu_group *g, int k, const uint8_t *b, size_t n)
UNUSED_CALL(bpe_gpu_group_train, bpe_gpu_group *g, long m, size_t *n)
UNUSED_CALL(bpe_gpu_group_fetch_merges, bpe_gpu_group *g, uint32_t *p, size_t cap, size_t *n)
UNUSED_CALL(bpe_gpu_group_fetch_ids, bpe_gpu_group *g, int k, uint32_t *p, size_t cap, size_t *n)
UNUSED_CALL(bpe_gpu_group_get_stats, bpe_gpu_group *g, bpe_gpu_stats *st)
void bpe_gpu_group_destroy(bpe_gpu_group *g) { (void)g; }

#define CHECK(x)                                                         \
    do {                                                                 \
        if (!(x)) {                                                      \
            fprintf(stderr, "asan_split_preset: %s:%d: %s\n", __FILE__, __LINE__, #x); \
            return 1;                                                    \
        }                                                                \
    } while (0)

/* the offsets of `text` under `preset`, the text held in a buffer of exactly its length and the
 * offsets in one of exactly their count: a read or a write past either end is reported.
 * Returns the pieces' lengths as a string of digits ("" for no bytes), NULL on failure. */
static char *piece_lengths(int preset, const char *text)
{
    const size_t n = strlen(text);
    uint8_t *buf = n ? malloc(n) : NULL;
    if (n && !buf) return NULL;
    if (n) memcpy(buf, text, n);
    size_t cnt = 0, again = 0;
    char *res = NULL;
    uint64_t *off = NULL;
    if (bpe_split_offsets_host(preset, buf, n, NULL, 0, &cnt) || cnt < 1) goto done;
    off = malloc(cnt * sizeof *off);
    res = calloc(cnt, 1);
    if (!off || !res) goto fail;
    if (bpe_split_offsets_host(preset, buf, n, off, cnt, &again) || again != cnt) goto fail;
    if (off[0] != 0 || off[cnt - 1] != n) goto fail;
    for (size_t d = 0; d + 1 < cnt; d++) {
        if (off[d + 1] <= off[d] || off[d + 1] - off[d] > 9) goto fail;
        res[d] = (char)('0' + (off[d + 1] - off[d]));
    }
    goto done;
fail:
    free(res);
    res = NULL;
done:
    free(off);
    free(buf);
    return res;
}

static int lengths_are(int preset, const char *text, const char *want)
{
    char *got = piece_lengths(preset, text);
    const int ok = got && !strcmp(got, want);
    if (!ok) fprintf(stderr, "asan_split_preset: \"%s\": pieces %s, expected %s\n", text, got ? got : "(failed)", want);
    free(got);
    return ok;
}

int main(void)
{
    static const char text[] = "Hello, world  42x\n\nfoo's it'll've 'tis don't  'd";
    const size_t n = sizeof text - 1;

    /* ---- bpe_split_offsets_host: the example of each preset */
    CHECK(lengths_are(BPE_SPLIT_GPT2, text, "51613111323332342121"));
    CHECK(lengths_are(BPE_SPLIT_WORDS, "Hello, world  42x\n\nfoo's", "516412311"));
    CHECK(lengths_are(BPE_SPLIT_LINES, "one\ntwo\n\nthree", "4415"));
    /* the probes at the buffer's very end: a contraction the end cuts is none, white space that reaches it stays whole */
    CHECK(lengths_are(BPE_SPLIT_GPT2, "a'l", "111") && lengths_are(BPE_SPLIT_GPT2, "a'r", "111"));
    CHECK(lengths_are(BPE_SPLIT_GPT2, "a'll", "13") && lengths_are(BPE_SPLIT_GPT2, "a're", "13"));
    CHECK(lengths_are(BPE_SPLIT_GPT2, "a'", "11") && lengths_are(BPE_SPLIT_GPT2, "'", "1") && lengths_are(BPE_SPLIT_GPT2, "a's", "12"));
    CHECK(lengths_are(BPE_SPLIT_GPT2, "'s", "2") && lengths_are(BPE_SPLIT_GPT2, "'ll", "3") && lengths_are(BPE_SPLIT_GPT2, "'l", "11"));
    CHECK(lengths_are(BPE_SPLIT_GPT2, "a  ", "12") && lengths_are(BPE_SPLIT_GPT2, "a ", "11") && lengths_are(BPE_SPLIT_GPT2, "a\n\n", "12"));
    CHECK(lengths_are(BPE_SPLIT_GPT2, "a  b", "112") && lengths_are(BPE_SPLIT_GPT2, "a \n", "12") && lengths_are(BPE_SPLIT_GPT2, " ", "1"));
    CHECK(lengths_are(BPE_SPLIT_GPT2, "", "") && lengths_are(BPE_SPLIT_WORDS, "", "") && lengths_are(BPE_SPLIT_LINES, "", ""));
    CHECK(lengths_are(BPE_SPLIT_GPT2, "x", "1") && lengths_are(BPE_SPLIT_WORDS, " ", "1") && lengths_are(BPE_SPLIT_LINES, "\n", "1"));
    {
        /* a cap below the count: the count is whole and nothing is written past the cap; no cap at all; no bytes */
        size_t cnt = 0;
        for (size_t cap = 0; cap < 5; cap++) {
            uint64_t *out = malloc((cap ? cap : 1) * sizeof *out);
            CHECK(out);
            CHECK(bpe_split_offsets_host(BPE_SPLIT_GPT2, (const uint8_t *)text, n, out, cap, &cnt) == 0 && cnt == 21);
            CHECK(cap < 2 || (out[0] == 0 && out[1] == 5));
            free(out);
        }
        uint64_t one = 7;
        CHECK(bpe_split_offsets_host(BPE_SPLIT_GPT2, NULL, 0, &one, 1, &cnt) == 0 && cnt == 1 && one == 0);
        CHECK(bpe_split_offsets_host(BPE_SPLIT_GPT2, NULL, 0, &one, 0, &cnt) == 0 && cnt == 1);
        CHECK(bpe_split_offsets_host(3, (const uint8_t *)text, n, NULL, 0, &cnt) == BPE_GPU_EINVAL);
        CHECK(bpe_split_offsets_host(-1, (const uint8_t *)text, n, NULL, 0, &cnt) == BPE_GPU_EINVAL);
        CHECK(bpe_split_offsets_host(BPE_SPLIT_GPT2, NULL, 3, NULL, 0, &cnt) == BPE_GPU_EINVAL);
        CHECK(bpe_split_offsets_host(BPE_SPLIT_GPT2, (const uint8_t *)text, n, NULL, 0, NULL) == BPE_GPU_EINVAL);
    }

    /* ---- bpe_encode_split_preset */
    static const uint64_t want[] = {0, 5, 6, 12, 13, 16, 17, 18, 19, 22, 24, 27, 30, 33, 35, 38, 42, 44, 45, 47, 48};
    dyn_arr_t *arr = dyn_arr_create(300, sizeof(pair_t));
    CHECK(arr);
    pair_t p = {1000, 1001}; /* a merge of ids the text never holds */
    CHECK(dyn_arr_set(arr, 256, &p));
    for (int with_byte_off = 0; with_byte_off < 2; with_byte_off++) {
        size_t len = 0, nd = 0;
        uint64_t *ido = NULL, *bo = NULL;
        uint32_t *ids = bpe_encode_split_preset((const uint8_t *)text, n, BPE_SPLIT_GPT2, arr, 0, &len, &ido,
                                                with_byte_off ? &bo : NULL, &nd);
        CHECK(ids && ido && len == n && nd == 20);
        for (size_t i = 0; i < n; i++) CHECK(ids[i] == (uint8_t)text[i]);
        for (size_t d = 0; d <= nd; d++) CHECK(ido[d] == want[d] && (!with_byte_off || bo[d] == want[d]));
        CHECK(with_byte_off ? bo != NULL : bo == NULL);
        free(ids);
        free(ido);
        free(bo);
    }
    {
        /* the table presets go the same way; no bytes: no pieces, the single offset 0 */
        size_t len = 7, nd = 7;
        uint64_t *ido = NULL, *bo = NULL;
        uint32_t *ids = bpe_encode_split_preset((const uint8_t *)text, n, BPE_SPLIT_LINES, arr, 0, &len, &ido, &bo, &nd);
        CHECK(ids && nd == 3 && bo[1] == 18 && bo[2] == 19 && bo[3] == n);
        free(ids);
        free(ido);
        free(bo);
        ids = bpe_encode_split_preset(NULL, 0, BPE_SPLIT_GPT2, arr, 0, &len, &ido, &bo, &nd);
        CHECK(ids && len == 0 && nd == 0 && ido[0] == 0 && bo[0] == 0);
        free(ids);
        free(ido);
        free(bo);
    }
    {
        /* failures give NULL, touch no output and leak nothing: bad arguments, no such preset, an engine error */
        size_t len = 0, nd = 0;
        uint64_t *ido = NULL, *bo = NULL;
        CHECK(!bpe_encode_split_preset((const uint8_t *)text, n, BPE_SPLIT_GPT2, NULL, 0, &len, &ido, &bo, &nd));
        CHECK(!bpe_encode_split_preset((const uint8_t *)text, n, BPE_SPLIT_GPT2, arr, 0, &len, NULL, &bo, &nd));
        CHECK(!bpe_encode_split_preset(NULL, n, BPE_SPLIT_GPT2, arr, 0, &len, &ido, &bo, &nd));
        CHECK(!bpe_encode_split_preset((const uint8_t *)text, n, 3, arr, 0, &len, &ido, &bo, &nd));
        g_fail_split = 1;
        CHECK(!bpe_encode_split_preset((const uint8_t *)text, n, BPE_SPLIT_GPT2, arr, 0, &len, &ido, &bo, &nd));
        g_fail_split = 0;
        CHECK(!ido && !bo && len == 0 && nd == 0);
        uint32_t *ids = bpe_encode_split_preset((const uint8_t *)text, n, BPE_SPLIT_GPT2, arr, 0, &len, &ido, &bo, &nd);
        CHECK(ids && nd == 20); /* and the next call works */
        free(ids);
        free(ido);
        free(bo);
    }
    bpe_gpu_stats st;
    CHECK(bpe_last_stats(&st) == 0 && st.n_out == n);
    dyn_arr_free(arr);

    /* ---- bpe_train_split_preset: the merges in the shape compress() returns (ids 0..255 first) */
    pair_t q = {0, 0};
    arr = bpe_train_split_preset((const uint8_t *)text, n, BPE_SPLIT_GPT2, -1, 0);
    CHECK(arr && arr->last_index == 257);
    CHECK(dyn_arr_get(arr, 256, &q) && q.a == 'a' && q.b == 'b' && dyn_arr_get(arr, 257, &q) && q.a == 256 && q.b == 'c');
    dyn_arr_free(arr);
    arr = bpe_train_split_preset((const uint8_t *)text, n, BPE_SPLIT_WORDS, 1, 0);
    CHECK(arr && arr->last_index == 256);
    dyn_arr_free(arr);
    arr = bpe_train_split_preset(NULL, 0, BPE_SPLIT_GPT2, 0, 0);
    CHECK(arr && arr->last_index == 255);
    dyn_arr_free(arr);
    CHECK(!bpe_train_split_preset(NULL, n, BPE_SPLIT_GPT2, -1, 0));
    CHECK(!bpe_train_split_preset((const uint8_t *)text, n, 3, -1, 0));
    g_fail_split = 1;
    CHECK(!bpe_train_split_preset((const uint8_t *)text, n, BPE_SPLIT_GPT2, -1, 0));
    g_fail_split = 0;
    g_fail_train = 1;
    CHECK(!bpe_train_split_preset((const uint8_t *)text, n, BPE_SPLIT_GPT2, -1, 0));
    g_fail_train = 0;
    g_fail_fetch = 1;
    CHECK(!bpe_train_split_preset((const uint8_t *)text, n, BPE_SPLIT_GPT2, -1, 0));
    g_fail_fetch = 0;
    arr = bpe_train_split_preset((const uint8_t *)text, n, BPE_SPLIT_GPT2, -1, 0); /* and the next call works */
    CHECK(arr && arr->last_index == 257);
    dyn_arr_free(arr);
    bpe_release_engines();
    CHECK(g_live == 0);
    printf("asan_split_preset: ok\n");
    return 0;
}

/* Stand-alone sanitizer check of bpe_train_split's host code
 * (src/bpe_train_split.c) and the context cache it shares with bpe.c: built
 * with -fsanitize=address,undefined against a HOST MODEL of the engine calls it
 * makes (below: load keeps a copy of the bytes, split applies the two-table
 * rule, train_split is a small recount-per-merge trainer over the pieces with
 * the tie rule of bpe_gpu.h).  Test infrastructure only; `make
 * asan-train-split`, run by tests/test_asan_train_split.py.  Exits 0 and
 * prints "asan_train_split: ok". */
#include "../../include/bpe_ex.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define MODEL_IDS 320 /* ids the model can hold: 256 bytes + 64 merges */

struct bpe_gpu_ctx {
    uint8_t *bytes;
    size_t n;
    uint64_t *off; /* the split's offsets, NULL when there are none */
    size_t ndocs;
    uint32_t *merges; /* the last train_split's pairs, NULL when there are none */
    size_t k;
};

static int g_fail_train; /* the model's bpe_gpu_train_split fails once armed */
static int g_fail_fetch; /* ... its bpe_gpu_fetch_split_merges */
static int g_live;       /* contexts alive */

static void drop(bpe_gpu_ctx *c)
{
    free(c->bytes);
    free(c->off);
    free(c->merges);
    c->bytes = NULL;
    c->off = NULL;
    c->merges = NULL;
    c->n = c->ndocs = c->k = 0;
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
int bpe_gpu_split(bpe_gpu_ctx *c, const uint8_t *cls, const uint16_t *brk, size_t *ndocs)
{
    for (int b = 0; b < 256; b++)
        if (cls[b] > 15) return BPE_GPU_EINVAL;
    free(c->off);
    free(c->merges);
    c->merges = NULL;
    c->off = malloc((c->n + 1) * sizeof(uint64_t));
    if (!c->off) return BPE_GPU_ENOMEM;
    size_t k = 0;
    for (size_t i = 0; i < c->n; i++)
        if (i == 0 || ((brk[cls[c->bytes[i - 1]]] >> cls[c->bytes[i]]) & 1)) c->off[k++] = i;
    c->off[k] = c->n;
    *ndocs = c->ndocs = k;
    return 0;
}
/* tokens with a flag on every piece's first one; recount, argmax (count desc, a asc, b asc), apply */
int bpe_gpu_train_split(bpe_gpu_ctx *c, long max_merges, size_t *n_merges)
{
    if (g_fail_train) return BPE_GPU_EHIP;
    if (!c->off) return BPE_GPU_ESTATE;
    free(c->merges);
    c->merges = NULL;
    c->k = 0;
    size_t T = c->n;
    uint32_t *tok = malloc((T ? T : 1) * sizeof *tok);
    uint8_t *head = calloc(T ? T : 1, 1);
    static uint32_t cnt[MODEL_IDS][MODEL_IDS];
    uint32_t *m = malloc(2 * (MODEL_IDS - 256) * sizeof *m);
    if (!tok || !head || !m) {
        free(tok);
        free(head);
        free(m);
        return BPE_GPU_ENOMEM;
    }
    for (size_t i = 0; i < T; i++) tok[i] = c->bytes[i];
    for (size_t d = 0; d < c->ndocs; d++) head[c->off[d]] = 1;
    size_t k = 0;
    for (;;) {
        memset(cnt, 0, sizeof cnt);
        for (size_t i = 0; i + 1 < T; i++)
            if (!head[i + 1]) cnt[tok[i]][tok[i + 1]]++;
        uint32_t best = 0, a = 0, b = 0;
        for (uint32_t x = 0; x < MODEL_IDS; x++)
            for (uint32_t y = 0; y < MODEL_IDS; y++)
                if (cnt[x][y] > best) best = cnt[x][y], a = x, b = y;
        if (best <= 1 || (max_merges >= 0 && k == (size_t)max_merges) || k == MODEL_IDS - 256) break;
        size_t o = 0;
        for (size_t i = 0; i < T; o++) {
            const int hit = i + 1 < T && !head[i + 1] && tok[i] == a && tok[i + 1] == b;
            head[o] = head[i];
            tok[o] = hit ? 256 + (uint32_t)k : tok[i];
            i += hit ? 2 : 1;
        }
        T = o;
        m[2 * k] = a;
        m[2 * k + 1] = b;
        k++;
    }
    free(tok);
    free(head);
    c->merges = m;
    c->k = k;
    *n_merges = k;
    return 0;
}
int bpe_gpu_fetch_split_merges(bpe_gpu_ctx *c, uint32_t *out, size_t cap, size_t *count)
{
    if (g_fail_fetch) return BPE_GPU_EHIP;
    if (!c->merges) return BPE_GPU_ESTATE;
    *count = c->k;
    for (size_t i = 0; out && i < c->k && i < cap; i++) out[2 * i] = c->merges[2 * i], out[2 * i + 1] = c->merges[2 * i + 1];
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

/* the rest of what bpe.c links against: not reached here */
#define UNUSED_CALL(name, ...) int name(__VA_ARGS__) { return BPE_GPU_ENODEV; }
UNUSED_CALL(bpe_gpu_load_fd, bpe_gpu_ctx *c, int fd, size_t s, size_t *n)
UNUSED_CALL(bpe_gpu_train, bpe_gpu_ctx *c, long m, size_t *n)
UNUSED_CALL(bpe_gpu_fetch_merges, bpe_gpu_ctx *c, uint32_t *p, size_t cap, size_t *n)
UNUSED_CALL(bpe_gpu_fetch_ids, bpe_gpu_ctx *c, uint32_t *ids, size_t cap, size_t *len)
UNUSED_CALL(bpe_gpu_encode, bpe_gpu_ctx *c, const uint32_t *p, size_t n)
UNUSED_CALL(bpe_gpu_decode, bpe_gpu_ctx *c, const uint32_t *ids, size_t len, const uint32_t *p, size_t n, uint8_t *out,
            size_t cap, size_t *olen)
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
            fprintf(stderr, "asan_train_split: %s:%d: %s\n", __FILE__, __LINE__, #x); \
            return 1;                                                    \
        }                                                                \
    } while (0)

/* the lines preset as bpe_gpu.h defines it (bpe_gpu_split_rule lives in the engine, not in this build) */
static void lines_rule(uint8_t *cls, uint16_t *brk)
{
    memset(cls, 0, 256);
    memset(brk, 0, 16 * sizeof *brk);
    cls['\n'] = 1;
    brk[1] = 0x3;
}

static int pair_is(dyn_arr_t *arr, size_t id, uint32_t a, uint32_t b)
{
    pair_t p = {0, 0};
    return dyn_arr_get(arr, id, &p) && p.a == a && p.b == b;
}

int main(void)
{
    static const char text[] = "ab\nab\nab\nab\nab\nab\nab\nab\n";
    const size_t n = sizeof text - 1;
    uint8_t cls[256];
    uint16_t brk[16];
    lines_rule(cls, brk);

    /* the example of the lines rule: two merges, in the shape compress() returns (ids 0..255 first) */
    dyn_arr_t *arr = bpe_train_split((const uint8_t *)text, n, cls, brk, -1, 0);
    CHECK(arr && arr->last_index == 257);
    CHECK(pair_is(arr, 97, 97, 0) && pair_is(arr, 256, 97, 98) && pair_is(arr, 257, 256, 10));
    dyn_arr_free(arr);
    /* a cap of the caller's, a cap of 0 and no bytes */
    arr = bpe_train_split((const uint8_t *)text, n, cls, brk, 1, 0);
    CHECK(arr && arr->last_index == 256 && pair_is(arr, 256, 97, 98));
    dyn_arr_free(arr);
    arr = bpe_train_split((const uint8_t *)text, n, cls, brk, 0, 0);
    CHECK(arr && arr->last_index == 255);
    dyn_arr_free(arr);
    arr = bpe_train_split(NULL, 0, cls, brk, -1, 0);
    CHECK(arr && arr->last_index == 255);
    dyn_arr_free(arr);
    /* one piece (no rule bit set): the stream's merges, pairs across the newlines included */
    memset(brk, 0, sizeof brk);
    arr = bpe_train_split((const uint8_t *)text, n, cls, brk, -1, 0);
    CHECK(arr && arr->last_index >= 259 && pair_is(arr, 258, 257, 257));
    dyn_arr_free(arr);
    lines_rule(cls, brk);
    /* failures give NULL and leak nothing: bad arguments, a bad class, engine errors at both calls */
    CHECK(!bpe_train_split((const uint8_t *)text, n, NULL, brk, -1, 0));
    CHECK(!bpe_train_split((const uint8_t *)text, n, cls, NULL, -1, 0));
    CHECK(!bpe_train_split(NULL, n, cls, brk, -1, 0));
    cls[200] = 16;
    CHECK(!bpe_train_split((const uint8_t *)text, n, cls, brk, -1, 0));
    cls[200] = 0;
    g_fail_train = 1;
    CHECK(!bpe_train_split((const uint8_t *)text, n, cls, brk, -1, 0));
    g_fail_train = 0;
    g_fail_fetch = 1;
    CHECK(!bpe_train_split((const uint8_t *)text, n, cls, brk, -1, 0));
    g_fail_fetch = 0;
    arr = bpe_train_split((const uint8_t *)text, n, cls, brk, -1, 0); /* and the next call works */
    CHECK(arr && arr->last_index == 257);
    dyn_arr_free(arr);
    bpe_release_engines();
    CHECK(g_live == 0);
    printf("asan_train_split: ok\n");
    return 0;
}

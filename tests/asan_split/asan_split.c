/* Stand-alone sanitizer check of bpe_encode_split's host code (src/bpe_docs.c)
 * and the context cache it shares with bpe.c: built with -fsanitize=address,
 * undefined against a HOST MODEL of the engine calls (below: load keeps a copy
 * of the bytes, split applies the two-table rule, encode_split emits one id
 * per byte, since no merge applies to ids the test's merge list never
 * names).  Test infrastructure only; `make asan-split`, run by
 * tests/test_asan_split.py.  Exits 0 and prints "asan_split: ok". */
#include "../../include/bpe_ex.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

struct bpe_gpu_ctx {
    uint8_t *bytes;
    size_t n;
    uint64_t *off;   /* the split's offsets, NULL when there are none */
    size_t ndocs;
    int encoded;
};

static int g_fail_split;   /* the model's bpe_gpu_split fails once armed */
static int g_live;         /* contexts alive */

static void drop(bpe_gpu_ctx *c)
{
    free(c->bytes);
    free(c->off);
    c->bytes = NULL;
    c->off = NULL;
    c->n = c->ndocs = 0;
    c->encoded = 0;
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
    if (g_fail_split) return BPE_GPU_EHIP;
    for (int b = 0; b < 256; b++)
        if (cls[b] > 15) return BPE_GPU_EINVAL;
    free(c->off);
    c->off = malloc((c->n + 1) * sizeof(uint64_t));
    if (!c->off) return BPE_GPU_ENOMEM;
    size_t k = 0;
    for (size_t i = 0; i < c->n; i++)
        if (i == 0 || ((brk[cls[c->bytes[i - 1]]] >> cls[c->bytes[i]]) & 1)) c->off[k++] = i;
    c->off[k] = c->n;
    *ndocs = c->ndocs = k;
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
int bpe_gpu_get_stats(bpe_gpu_ctx *c, bpe_gpu_stats *st)
{
    memset(st, 0, sizeof *st);
    st->n_in = st->n_out = c->n;
    return 0;
}
const char *bpe_gpu_strerror(int code) { (void)code; return "host model"; }
const char *bpe_gpu_last_error(void) { return "host model"; }

/* the rest of what bpe.c and bpe_docs.c link against: not reached here */
#define UNUSED_CALL(name, ...) int name(__VA_ARGS__) { return BPE_GPU_ENODEV; }
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
            fprintf(stderr, "asan_split: %s:%d: %s\n", __FILE__, __LINE__, #x); \
            return 1;                                                    \
        }                                                                \
    } while (0)

/* the words preset as bpe_gpu.h defines it (bpe_gpu_split_rule lives in the engine, not in this build) */
static void words_rule(uint8_t *cls, uint16_t *brk)
{
    memset(cls, 0, 256);
    memset(brk, 0, 16 * sizeof *brk);
    for (int b = 0; b < 256; b++)
        cls[b] = (b >= 'A' && b <= 'Z') || (b >= 'a' && b <= 'z') || b >= 0x80 ? 1
                 : b >= '0' && b <= '9' ? 2 : b == ' ' ? 3 : b >= '\t' && b <= '\r' ? 4 : 0;
    for (int p = 0; p < 5; p++) brk[p] = (uint16_t)(0x1F & ~(1 << p));
    brk[3] = 1 << 4;
}

int main(void)
{
    static const char text[] = "Hello, world  42x\n\nfoo's";
    static const uint64_t want[] = {0, 5, 6, 12, 16, 17, 19, 22, 23, 24};
    const size_t n = sizeof text - 1;
    uint8_t cls[256];
    uint16_t brk[16];
    words_rule(cls, brk);
    dyn_arr_t *arr = dyn_arr_create(300, sizeof(pair_t));
    CHECK(arr);
    pair_t p = {1000, 1001};  /* a merge of ids the text never holds */
    CHECK(dyn_arr_set(arr, 256, &p));

    for (int with_byte_off = 0; with_byte_off < 2; with_byte_off++) {
        size_t len = 0, nd = 0;
        uint64_t *ido = NULL, *bo = NULL;
        uint32_t *ids = bpe_encode_split((const uint8_t *)text, n, cls, brk, arr, 0, &len, &ido,
                                         with_byte_off ? &bo : NULL, &nd);
        CHECK(ids && ido && len == n && nd == 9);
        for (size_t i = 0; i < n; i++) CHECK(ids[i] == (uint8_t)text[i]);
        for (size_t d = 0; d <= nd; d++) CHECK(ido[d] == want[d] && (!with_byte_off || bo[d] == want[d]));
        CHECK(with_byte_off ? bo != NULL : bo == NULL);
        free(ids);
        free(ido);
        free(bo);
    }
    /* no bytes: no pieces, the single offset 0 */
    {
        size_t len = 7, nd = 7;
        uint64_t *ido = NULL, *bo = NULL;
        uint32_t *ids = bpe_encode_split(NULL, 0, cls, brk, arr, 0, &len, &ido, &bo, &nd);
        CHECK(ids && len == 0 && nd == 0 && ido[0] == 0 && bo[0] == 0);
        free(ids);
        free(ido);
        free(bo);
    }
    /* failures give NULL, touch no output and leak nothing: bad arguments, a bad class, an engine error */
    {
        size_t len = 0, nd = 0;
        uint64_t *ido = NULL, *bo = NULL;
        CHECK(!bpe_encode_split((const uint8_t *)text, n, NULL, brk, arr, 0, &len, &ido, &bo, &nd));
        CHECK(!bpe_encode_split((const uint8_t *)text, n, cls, brk, arr, 0, &len, NULL, &bo, &nd));
        CHECK(!bpe_encode_split(NULL, n, cls, brk, arr, 0, &len, &ido, &bo, &nd));
        cls[200] = 16;
        CHECK(!bpe_encode_split((const uint8_t *)text, n, cls, brk, arr, 0, &len, &ido, &bo, &nd));
        cls[200] = 1;
        g_fail_split = 1;
        CHECK(!bpe_encode_split((const uint8_t *)text, n, cls, brk, arr, 0, &len, &ido, &bo, &nd));
        g_fail_split = 0;
        CHECK(!ido && !bo && len == 0 && nd == 0);
        uint32_t *ids = bpe_encode_split((const uint8_t *)text, n, cls, brk, arr, 0, &len, &ido, &bo, &nd);
        CHECK(ids && nd == 9);  /* and the next call works */
        free(ids);
        free(ido);
        free(bo);
    }
    bpe_gpu_stats st;
    CHECK(bpe_last_stats(&st) == 0 && st.n_out == n);
    dyn_arr_free(arr);
    bpe_release_engines();
    CHECK(g_live == 0);
    printf("asan_split: ok\n");
    return 0;
}

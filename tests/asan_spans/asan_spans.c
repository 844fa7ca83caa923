/* Stand-alone sanitizer check of the token spans' host code (src/bpe_spans.c: bpe_span_lens and
 * bpe_token_spans_host): built with -fsanitize=address,undefined.  The code under test calls no engine function.
 * Every buffer handed over is malloc'd to exactly the size the call may touch, so a table entry, an id, an
 * offset or a byte read past its array, or a span written past 2 n_ids, is reported.  Test infrastructure only;
 * `make asan-spans`, run by tests/test_asan_spans.py.  Exits 0 and prints "asan_spans: ok". */
#include "../../include/bpe_ex.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define CHECK(x)                                                         \
    do {                                                                 \
        if (!(x)) {                                                      \
            fprintf(stderr, "asan_spans: %s:%d: %s\n", __FILE__, __LINE__, #x); \
            exit(1);                                                     \
        }                                                                \
    } while (0)

/* a copy of src[0 .. bytes) in a block of exactly that size (NULL for 0) */
static void *exact(const void *src, size_t bytes)
{
    if (!bytes) return NULL;
    void *p = malloc(bytes);
    CHECK(p);
    memcpy(p, src, bytes);
    return p;
}

/* merges: 256 = "ab", 257 = "ab" + "c", 258 = 0xE2 0x82, 259 = (0xE2 0x82) 0xAC = the euro sign; specials "<s>", "<|e|>" */
static const uint32_t PAIRS[8] = {'a', 'b', 256, 'c', 0xE2, 0x82, 258, 0xAC};
static const uint8_t SP_BYTES[8] = {'<', 's', '>', '<', '|', 'e', '|', '>'};
static const uint32_t SP_LEN[2] = {3, 5};

static uint32_t *table(const bpe_gpu_vocab *vocab, size_t *count)
{
    uint32_t *pairs = exact(PAIRS, sizeof PAIRS), *splen = exact(SP_LEN, sizeof SP_LEN);
    uint8_t *spb = exact(SP_BYTES, sizeof SP_BYTES);
    const bpe_gpu_specials sp = {spb, splen, 2};
    char msg[400];
    CHECK(bpe_span_lens(pairs, 4, &sp, vocab, NULL, 0, count, msg, sizeof msg) == 0 && msg[0] == '\0');
    uint32_t *out = malloc(*count * sizeof *out);
    CHECK(out);
    size_t again = 0;
    CHECK(bpe_span_lens(pairs, 4, &sp, vocab, out, *count, &again, NULL, 0) == 0 && again == *count);
    /* a shorter buffer takes its share */
    uint32_t *part = malloc(3 * sizeof *part);
    CHECK(part && bpe_span_lens(pairs, 4, &sp, vocab, part, 3, &again, NULL, 0) == 0 && again == *count);
    CHECK(memcmp(part, out, 3 * sizeof *part) == 0);
    free(part);
    free(pairs);
    free(splen);
    free(spb);
    return out;
}

/* the spans of ids over the texts, each array exactly sized; returns the code, the spans in *out (caller frees) */
static int spans(const uint32_t *ids, size_t n_ids, const uint64_t *toff, const uint64_t *boff, size_t T,
                 const uint8_t *bytes, size_t n, const uint32_t *lens, size_t n_lens, int unit, uint32_t **out, char *msg)
{
    uint32_t *i2 = exact(ids, n_ids * sizeof *ids), *l2 = exact(lens, n_lens * sizeof *lens);
    uint64_t *t2 = exact(toff, (T + 1) * sizeof *toff), *b2 = exact(boff, (T + 1) * sizeof *boff);
    uint8_t *y2 = exact(bytes, n);
    *out = n_ids ? malloc(2 * n_ids * sizeof **out) : NULL;
    CHECK(!n_ids || *out);
    const int rc = bpe_token_spans_host(i2, n_ids, t2, T, y2, n, b2, l2, n_lens, unit, *out, msg, msg ? 400 : 0);
    free(i2);
    free(l2);
    free(t2);
    free(b2);
    free(y2);
    return rc;
}

int main(void)
{
    char msg[400];
    size_t nl = 0;
    uint32_t *lens = table(NULL, &nl);
    CHECK(nl == 256 + 4 + 2);
    CHECK(lens[0] == 1 && lens['a'] == 1 && lens[256] == 2 && lens[257] == 3 && lens[258] == 2 && lens[259] == 3);
    CHECK(lens[260] == 3 && lens[261] == 5);

    /* a vocabulary with holes: byte b is 2 b + 1, the merges 1000 .. 1003 backwards, the specials 0 and 2000 */
    uint32_t byte_id[256], merge_id[4] = {1003, 1002, 1001, 1000}, special_id[2] = {0, 2000};
    for (uint32_t b = 0; b < 256; b++) byte_id[b] = 2 * b + 1;
    uint32_t *bi = exact(byte_id, sizeof byte_id), *mi = exact(merge_id, sizeof merge_id), *si = exact(special_id, sizeof special_id);
    const bpe_gpu_vocab v = {bi, mi, si, 4, 2};
    size_t nv = 0;
    uint32_t *vl = table(&v, &nv);
    CHECK(nv == 2001 && vl[0] == 3 && vl[2000] == 5 && vl[1] == 1 && vl[2] == 0 && vl[1003] == 2 && vl[1000] == 3 && vl[999] == 0);
    const bpe_gpu_vocab wrong = {bi, mi, si, 3, 2};
    CHECK(bpe_span_lens(PAIRS, 4, NULL, &wrong, NULL, 0, &nv, msg, sizeof msg) == BPE_GPU_EINVAL && strstr(msg, "vocabulary"));

    /* refusals of the table */
    const uint32_t later[6] = {'a', 'b', 258, 'c', 'x', 'y'};
    uint32_t *lp = exact(later, sizeof later);
    CHECK(bpe_span_lens(lp, 3, NULL, NULL, NULL, 0, &nl, msg, sizeof msg) == BPE_GPU_EINVAL);
    CHECK(strncmp(msg, "spans: ", 7) == 0 && strstr(msg, "merge 1 names the id 258"));
    char *tiny = malloc(8);
    CHECK(tiny && bpe_span_lens(lp, 3, NULL, NULL, NULL, 0, &nl, tiny, 8) == BPE_GPU_EINVAL && strlen(tiny) == 7);
    free(tiny);
    free(lp);
    /* doubling 32 times passes 2^32 - 1 */
    uint32_t dbl[2 * 33];
    for (uint32_t r = 0; r < 33; r++) dbl[2 * r] = dbl[2 * r + 1] = r ? 255 + r : 'a';
    uint32_t *dp = exact(dbl, sizeof dbl);
    CHECK(bpe_span_lens(dp, 31, NULL, NULL, NULL, 0, &nl, msg, sizeof msg) == 0 && nl == 256 + 31);
    CHECK(bpe_span_lens(dp, 33, NULL, NULL, NULL, 0, &nl, msg, sizeof msg) == BPE_GPU_ERANGE && strstr(msg, "merge 31"));
    free(dp);
    nl = 262;

    /* three texts: "abc<s>" + euro, "", euro cut: 0xE2 0x82 | (next text) 0xAC 'a' */
    const uint8_t bytes[] = {'a', 'b', 'c', '<', 's', '>', 0xE2, 0x82, 0xAC, 0xE2, 0x82, 0xAC, 'a'};
    const uint32_t ids[] = {257, 260, 258, 0xAC, 258, 0xAC, 'a'};
    const uint64_t toff[] = {0, 4, 4, 5, 7}, boff[] = {0, 9, 9, 11, 13};
    uint32_t *out;
    CHECK(spans(ids, 7, toff, boff, 4, bytes, 13, lens, nl, BPE_SPAN_BYTE, &out, msg) == 0 && msg[0] == '\0');
    const uint32_t want_b[14] = {0, 3, 3, 6, 6, 8, 8, 9, 0, 2, 0, 1, 1, 2};
    CHECK(memcmp(out, want_b, sizeof want_b) == 0);
    free(out);
    CHECK(spans(ids, 7, toff, boff, 4, bytes, 13, lens, nl, BPE_SPAN_CHAR, &out, msg) == 0);
    /* the euro's two tokens both report character 6..7; the cut euro is one character; 0xAC 'a': the clamp */
    const uint32_t want_c[14] = {0, 3, 3, 6, 6, 7, 6, 7, 0, 1, 0, 0, 0, 1};
    CHECK(memcmp(out, want_c, sizeof want_c) == 0);
    free(out);
    /* the byte unit needs no bytes */
    {
        uint32_t *o2 = malloc(14 * sizeof *o2);
        CHECK(o2 && bpe_token_spans_host(ids, 7, toff, 4, NULL, 13, boff, lens, nl, BPE_SPAN_BYTE, o2, NULL, 0) == 0);
        CHECK(memcmp(o2, want_b, sizeof want_b) == 0);
        CHECK(bpe_token_spans_host(ids, 7, toff, 4, NULL, 13, boff, lens, nl, BPE_SPAN_CHAR, o2, NULL, 0) == BPE_GPU_EINVAL);
        CHECK(bpe_token_spans_host(ids, 7, toff, 4, bytes, 13, boff, lens, nl, 2, o2, NULL, 0) == BPE_GPU_EINVAL);
        free(o2);
    }
    /* texts that begin with continuation bytes and end inside a character */
    const uint8_t cont[] = {0x80, 0x80, 'a', 0xE2, 0x82};
    const uint32_t cid[] = {0x80, 0x80, 'a', 258};
    const uint64_t ct[] = {0, 3, 4}, cb[] = {0, 3, 5};
    CHECK(spans(cid, 4, ct, cb, 2, cont, 5, lens, nl, BPE_SPAN_CHAR, &out, msg) == 0);
    const uint32_t want_k[8] = {0, 0, 0, 0, 0, 1, 0, 1};
    CHECK(memcmp(out, want_k, sizeof want_k) == 0);
    free(out);
    /* T = 0, and texts that are all empty */
    const uint64_t zero[4] = {0, 0, 0, 0};
    CHECK(spans(NULL, 0, zero, zero, 0, NULL, 0, lens, nl, BPE_SPAN_CHAR, &out, msg) == 0);
    CHECK(spans(NULL, 0, zero, zero, 3, NULL, 0, lens, nl, BPE_SPAN_CHAR, &out, msg) == 0);
    /* refusals: an id outside the table, a hole, a wrong sum (the text named), bad offsets */
    const uint32_t big[] = {257, 262};
    const uint64_t t1[] = {0, 2}, b1[] = {0, 4};
    CHECK(spans(big, 2, t1, b1, 1, bytes, 4, lens, nl, BPE_SPAN_BYTE, &out, msg) == BPE_GPU_EDATA && strstr(msg, "unknown token id 262"));
    free(out);
    const uint32_t hole[] = {1003, 2};
    CHECK(spans(hole, 2, t1, b1, 1, bytes, 4, vl, 2001, BPE_SPAN_BYTE, &out, msg) == BPE_GPU_EDATA && strstr(msg, "unknown token id 2 "));
    free(out);
    const uint64_t t2[] = {0, 1, 2}, b2[] = {0, 3, 5};
    const uint32_t two[] = {257, 257};
    CHECK(spans(two, 2, t2, b2, 2, bytes, 5, lens, nl, BPE_SPAN_CHAR, &out, msg) == BPE_GPU_EDATA);
    CHECK(strstr(msg, "text 1") && strstr(msg, "sum to 3") && strstr(msg, "holds 2 bytes"));
    free(out);
    const uint64_t falls[] = {0, 2, 1};
    CHECK(spans(two, 2, falls, b2, 2, bytes, 5, lens, nl, BPE_SPAN_BYTE, &out, msg) == BPE_GPU_EINVAL);
    free(out);
    CHECK(spans(two, 2, t2, falls, 2, bytes, 5, lens, nl, BPE_SPAN_BYTE, &out, msg) == BPE_GPU_EINVAL);
    free(out);

    free(lens);
    free(vl);
    free(bi);
    free(mi);
    free(si);
    printf("asan_spans: ok\n");
    return 0;
}

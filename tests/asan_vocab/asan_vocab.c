/* Stand-alone sanitizer check of the vocabularies' host code (src/bpe_vocab.c: bpe_vocab_check and
 * bpe_vocab_tables): built with -fsanitize=address,undefined.  The code under test calls no engine
 * function.  Every buffer handed over is malloc'd to exactly the size the call may touch, so an entry
 * read past an id array or written past `cap` entries of a table is reported.  Test infrastructure
 * only; `make asan-vocab`, run by tests/test_asan_vocab.py.  Exits 0 and prints "asan_vocab: ok". */
#include "../../include/bpe_ex.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define CHECK(x)                                                         \
    do {                                                                 \
        if (!(x)) {                                                      \
            fprintf(stderr, "asan_vocab: %s:%d: %s\n", __FILE__, __LINE__, #x); \
            exit(1);                                                     \
        }                                                                \
    } while (0)

/* a vocabulary in exactly sized heap buffers, with its merge list */
struct voc {
    bpe_gpu_vocab v;
    uint32_t *byte_id, *merge_id, *special_id, *pairs;
};

/* byte b = (b * 7 + 3) % 256 (a permutation), merge r = base + 2 r, special j = far + 5 j;
   merge r joins (r % 256, 255 + r) for r > 0 (the second part is the merge before it) */
static struct voc make_voc(size_t nm, size_t ns, uint32_t base, uint32_t far)
{
    struct voc s;
    s.byte_id = malloc(256 * sizeof(uint32_t));
    s.merge_id = nm ? malloc(nm * sizeof(uint32_t)) : NULL;
    s.special_id = ns ? malloc(ns * sizeof(uint32_t)) : NULL;
    s.pairs = nm ? malloc(2 * nm * sizeof(uint32_t)) : NULL;
    CHECK(s.byte_id && (!nm || (s.merge_id && s.pairs)) && (!ns || s.special_id));
    for (uint32_t b = 0; b < 256; b++) s.byte_id[b] = (b * 7 + 3) % 256;
    for (size_t r = 0; r < nm; r++) {
        s.merge_id[r] = base + 2 * (uint32_t)r;
        s.pairs[2 * r] = (uint32_t)(r % 256);
        s.pairs[2 * r + 1] = r ? 255 + (uint32_t)r : 65;
    }
    for (size_t j = 0; j < ns; j++) s.special_id[j] = far + 5 * (uint32_t)j;
    s.v.byte_id = s.byte_id;
    s.v.merge_id = s.merge_id;
    s.v.special_id = s.special_id;
    s.v.n_merges = nm;
    s.v.n_specials = ns;
    return s;
}

static void free_voc(struct voc *s)
{
    free(s->byte_id);
    free(s->merge_id);
    free(s->special_id);
    free(s->pairs);
}

/* the tables in exactly sized buffers, held against a restatement */
static void check_tables(const struct voc *s)
{
    size_t nf = 0, ni = 0;
    CHECK(bpe_vocab_tables(&s->v, NULL, 0, NULL, 0, &nf, &ni) == 0);
    CHECK(nf == 256 + s->v.n_merges + s->v.n_specials);
    uint32_t *fwd = malloc(nf * sizeof(uint32_t)), *inv = malloc(ni * sizeof(uint32_t));
    CHECK(fwd && inv);
    CHECK(bpe_vocab_tables(&s->v, fwd, nf, inv, ni, &nf, &ni) == 0);
    uint32_t top = 0;
    for (size_t k = 0; k < nf; k++) {
        const uint32_t id = k < 256 ? s->byte_id[k] : k < 256 + s->v.n_merges ? s->merge_id[k - 256]
                                                                               : s->special_id[k - 256 - s->v.n_merges];
        CHECK(fwd[k] == id);
        CHECK(id < ni && inv[id] == k);
        if (id > top) top = id;
    }
    CHECK(ni == (size_t)top + 1);
    size_t holes = 0;
    for (size_t i = 0; i < ni; i++) holes += inv[i] == 0xFFFFFFFFu;
    CHECK(holes == ni - nf);
    free(fwd);
    free(inv);
    /* a short cap: nothing past it is written (the buffers are exactly that long) */
    const size_t cf = nf / 2, ci = ni / 3;
    fwd = malloc((cf ? cf : 1) * sizeof(uint32_t));
    inv = malloc((ci ? ci : 1) * sizeof(uint32_t));
    CHECK(fwd && inv);
    CHECK(bpe_vocab_tables(&s->v, fwd, cf, inv, ci, &nf, &ni) == 0);
    for (size_t i = 0; i < ci; i++) CHECK(inv[i] == 0xFFFFFFFFu || (inv[i] < nf));
    free(fwd);
    free(inv);
}

static void expect_refusal(const struct voc *s, const uint32_t *pairs, size_t nm, const char *word)
{
    char msg[400];
    size_t nf, ni;
    CHECK(bpe_vocab_check(&s->v, pairs, nm, msg, sizeof msg) == BPE_GPU_EINVAL);
    if (!strstr(msg, word)) {
        fprintf(stderr, "asan_vocab: \"%s\" does not name \"%s\"\n", msg, word);
        exit(1);
    }
    CHECK(bpe_vocab_check(&s->v, pairs, nm, NULL, 0) == BPE_GPU_EINVAL); /* (no message wanted) */
    char tiny[8];                                                       /* (a message cut short stays in its buffer) */
    CHECK(bpe_vocab_check(&s->v, pairs, nm, tiny, sizeof tiny) == BPE_GPU_EINVAL);
    CHECK(strlen(tiny) < sizeof tiny);
    /* the tables refuse what the check refuses (they see no merge list: a bad part is not theirs to find) */
    if (!strstr(msg, "part")) CHECK(bpe_vocab_tables(&s->v, NULL, 0, NULL, 0, &nf, &ni) == BPE_GPU_EINVAL);
}

int main(void)
{
    char msg[400];
    /* valid sets: merges and specials, zero merges, zero specials, neither */
    const size_t shapes[][2] = {{300, 2}, {0, 2}, {300, 0}, {0, 0}, {1, 1}};
    for (size_t k = 0; k < sizeof shapes / sizeof shapes[0]; k++) {
        struct voc s = make_voc(shapes[k][0], shapes[k][1], 1000, 100000);
        CHECK(bpe_vocab_check(&s.v, s.pairs, s.v.n_merges, msg, sizeof msg) == 0 && msg[0] == '\0');
        CHECK(bpe_vocab_check(&s.v, NULL, s.v.n_merges, NULL, 0) == 0);
        check_tables(&s);
        free_voc(&s);
    }
    /* the identity numbering */
    {
        struct voc s = make_voc(40, 3, 256, 256 + 40);
        for (uint32_t b = 0; b < 256; b++) s.byte_id[b] = b;
        for (uint32_t r = 0; r < 40; r++) s.merge_id[r] = 256 + r;
        for (uint32_t j = 0; j < 3; j++) s.special_id[j] = 256 + 40 + j;
        CHECK(bpe_vocab_check(&s.v, s.pairs, 40, msg, sizeof msg) == 0);
        check_tables(&s);
        free_voc(&s);
    }
    /* the largest allowed id, and the one past it */
    {
        struct voc s = make_voc(5, 2, 1000, 100000);
        s.special_id[1] = BPE_VOCAB_ID_LIMIT - 1;
        CHECK(bpe_vocab_check(&s.v, s.pairs, 5, msg, sizeof msg) == 0);
        check_tables(&s); /* (an inverse table of 2^24 entries) */
        s.special_id[1] = BPE_VOCAB_ID_LIMIT;
        expect_refusal(&s, s.pairs, 5, "special 1");
        s.special_id[1] = 0xFFFFFFFFu;
        expect_refusal(&s, s.pairs, 5, "2^24");
        s.special_id[1] = 100005;
        s.merge_id[4] = BPE_VOCAB_ID_LIMIT;
        expect_refusal(&s, s.pairs, 5, "merge 4");
        s.merge_id[4] = 1008;
        s.byte_id[0x41] = BPE_VOCAB_ID_LIMIT + 7;
        expect_refusal(&s, s.pairs, 5, "byte 0x41");
        free_voc(&s);
    }
    /* duplicates: inside one array and across each pair of arrays */
    {
        struct voc s = make_voc(6, 2, 1000, 100000);
        s.byte_id[9] = s.byte_id[8];
        expect_refusal(&s, s.pairs, 6, "byte 0x08 and byte 0x09");
        s.byte_id[9] = (9 * 7 + 3) % 256;
        s.merge_id[3] = s.byte_id[0x21];
        expect_refusal(&s, s.pairs, 6, "byte 0x21 and merge 3");
        s.merge_id[3] = s.merge_id[1];
        expect_refusal(&s, s.pairs, 6, "merge 1 and merge 3");
        s.merge_id[3] = 1006;
        s.special_id[0] = s.merge_id[5];
        expect_refusal(&s, s.pairs, 6, "merge 5 and special 0");
        s.special_id[0] = s.byte_id[0];
        expect_refusal(&s, s.pairs, 6, "byte 0x00 and special 0");
        s.special_id[0] = s.special_id[1];
        expect_refusal(&s, s.pairs, 6, "special 0 and special 1");
        free_voc(&s);
    }
    /* a merge that names its own or a later id */
    {
        struct voc s = make_voc(6, 0, 1000, 0);
        s.pairs[2 * 2] = 256 + 2;
        expect_refusal(&s, s.pairs, 6, "merge 2");
        s.pairs[2 * 2] = 2;
        s.pairs[2 * 4 + 1] = 256 + 5;
        expect_refusal(&s, s.pairs, 6, "second part");
        CHECK(bpe_vocab_check(&s.v, NULL, 6, msg, sizeof msg) == 0); /* (without a list there is nothing to name) */
        free_voc(&s);
    }
    /* counts that disagree, too many specials, missing arrays, no vocabulary */
    {
        struct voc s = make_voc(6, 2, 1000, 100000);
        CHECK(bpe_vocab_check(&s.v, s.pairs, 5, msg, sizeof msg) == BPE_GPU_EINVAL && strstr(msg, "6 merges"));
        CHECK(bpe_vocab_check(&s.v, s.pairs, 7, msg, sizeof msg) == BPE_GPU_EINVAL);
        s.v.n_specials = BPE_GPU_SPECIAL_MAX_COUNT + 1; /* (refused before any entry is read) */
        CHECK(bpe_vocab_check(&s.v, s.pairs, 6, msg, sizeof msg) == BPE_GPU_EINVAL && strstr(msg, "specials"));
        s.v.n_specials = 2;
        s.v.special_id = NULL;
        CHECK(bpe_vocab_check(&s.v, s.pairs, 6, msg, sizeof msg) == BPE_GPU_EINVAL && strstr(msg, "missing"));
        s.v.special_id = s.special_id;
        s.v.byte_id = NULL;
        CHECK(bpe_vocab_check(&s.v, s.pairs, 6, msg, sizeof msg) == BPE_GPU_EINVAL);
        CHECK(bpe_vocab_check(NULL, NULL, 0, msg, sizeof msg) == BPE_GPU_EINVAL);
        size_t nf, ni;
        CHECK(bpe_vocab_tables(NULL, NULL, 0, NULL, 0, &nf, &ni) == BPE_GPU_EINVAL);
        s.v.byte_id = s.byte_id;
        CHECK(bpe_vocab_tables(&s.v, NULL, 0, NULL, 0, NULL, &ni) == BPE_GPU_EINVAL);
        free_voc(&s);
    }
    printf("asan_vocab: ok\n");
    return 0;
}

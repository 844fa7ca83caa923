/* Stand-alone sanitizer check of the special tokens' host code (src/bpe_special.c:
 * bpe_specials_check and bpe_split_offsets_host_special, over bpe_split_offsets_host of
 * src/bpe_split_preset.c): built with -fsanitize=address,undefined.  The code under test
 * calls no engine function; the three stubs below only satisfy what
 * bpe_split_preset.c's other entry points reference.  Every buffer handed over is
 * malloc'd to exactly the size the call may touch, so a byte read past the text, past a
 * special or past `cap` entries is reported.  Test infrastructure only; `make
 * asan-special`, run by tests/test_asan_special.py.  Exits 0 and prints "asan_special: ok". */
#include "../../include/bpe_ex.h"
#include "../../llmtokenizer_amd/src/bpe_internal.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

int bpe_gpu_split_preset(bpe_gpu_ctx *c, int preset, size_t *ndocs) { (void)c, (void)preset, (void)ndocs; return BPE_GPU_ENODEV; }
uint32_t *encode_split_with(const uint8_t *bytes, size_t n, bpe_split_fn split, const void *rule, dyn_arr_t *pair_arr,
                            int device, size_t *len, uint64_t **id_off, uint64_t **byte_off, size_t *ndocs)
{
    (void)bytes, (void)n, (void)split, (void)rule, (void)pair_arr, (void)device, (void)len, (void)id_off, (void)byte_off, (void)ndocs;
    return NULL;
}
dyn_arr_t *train_split_with(const uint8_t *bytes, size_t n, bpe_split_fn split, const void *rule, long max_merges, int device)
{
    (void)bytes, (void)n, (void)split, (void)rule, (void)max_merges, (void)device;
    return NULL;
}

#define CHECK(x)                                                         \
    do {                                                                 \
        if (!(x)) {                                                      \
            fprintf(stderr, "asan_special: %s:%d: %s\n", __FILE__, __LINE__, #x); \
            exit(1);                                                     \
        }                                                                \
    } while (0)

/* a set in exactly sized heap buffers */
struct set {
    bpe_gpu_specials sp;
    uint8_t *bytes;
    uint32_t *len;
};

static struct set make_set(const char *const *items, size_t count)
{
    struct set s;
    size_t total = 0;
    for (size_t i = 0; i < count; i++) total += strlen(items[i]);
    s.bytes = malloc(total ? total : 1);
    s.len = malloc((count ? count : 1) * sizeof(uint32_t));
    CHECK(s.bytes && s.len);
    size_t o = 0;
    for (size_t i = 0; i < count; i++) {
        s.len[i] = (uint32_t)strlen(items[i]);
        memcpy(s.bytes + o, items[i], s.len[i]);
        o += s.len[i];
    }
    s.sp.bytes = total ? s.bytes : NULL;
    s.sp.len = count ? s.len : NULL;
    s.sp.count = count;
    if (!total) s.sp.bytes = s.bytes;
    return s;
}

static void free_set(struct set *s)
{
    free(s->bytes);
    free(s->len);
}

static int check_set(const char *const *items, size_t count, const char *want)
{
    struct set s = make_set(items, count);
    char *msg = malloc(200);
    CHECK(msg);
    const int rc = bpe_specials_check(&s.sp, msg, 200);
    if (want) CHECK(rc == BPE_GPU_EINVAL && strstr(msg, want));
    else CHECK(rc == 0 && msg[0] == '\0');
    /* a message buffer too small for the text, and none */
    char *tiny = malloc(8);
    CHECK(tiny);
    CHECK(bpe_specials_check(&s.sp, tiny, 8) == rc && strlen(tiny) < 8);
    CHECK(bpe_specials_check(&s.sp, NULL, 0) == rc);
    free(tiny);
    free(msg);
    free_set(&s);
    return rc;
}

/* the split of `text` (exactly sized) by `preset` or the tables; compares the two-phase protocol and every cap */
static void split(const char *text, int preset, const uint8_t *cls, const uint16_t *brk, const struct set *s,
                  const uint64_t *want, size_t want_count, const uint64_t *want_piece, size_t want_m)
{
    const size_t n = strlen(text);
    uint8_t *b = malloc(n ? n : 1);
    CHECK(b);
    memcpy(b, text, n);
    size_t count = 0, m = 0;
    CHECK(bpe_split_offsets_host_special(preset, cls, brk, b, n, &s->sp, NULL, 0, &count, NULL, NULL, 0, &m) == 0);
    CHECK(count == want_count && m == want_m);
    for (size_t cap = 0; cap <= count + 1; cap++) {
        uint64_t *out = malloc((cap ? cap : 1) * sizeof *out);
        uint64_t *piece = malloc((m ? m : 1) * sizeof *piece);
        uint32_t *index = malloc((m ? m : 1) * sizeof *index);
        CHECK(out && piece && index);
        size_t c2 = 0, m2 = 0;
        const size_t mcap = cap < m ? cap : m;
        CHECK(bpe_split_offsets_host_special(preset, cls, brk, b, n, &s->sp, out, cap, &c2, piece, index, mcap, &m2) == 0);
        CHECK(c2 == count && m2 == m);
        for (size_t i = 0; i < cap && i < count; i++) CHECK(out[i] == want[i]);
        for (size_t i = 0; i < mcap; i++) CHECK(piece[i] == want_piece[i] && index[i] < s->sp.count);
        free(out);
        free(piece);
        free(index);
    }
    free(b);
}

int main(void)
{
    static const char *const gpt2[] = {"<|endoftext|>"};
    static const char *const chat[] = {"<|endoftext|>", "<|im_start|>", "<|im_end|>"};
    static const char *const dup[] = {"<a>", "<b>", "<a>"};
    static const char *const sub[] = {"<|b|>", "b|"};
    static const char *const aa[] = {"aa"};
    static const char *const cross[] = {"<a>", "><"};
    static const char *const empty[] = {"<a>", ""};
    CHECK(check_set(gpt2, 1, NULL) == 0);
    CHECK(check_set(chat, 3, NULL) == 0);
    CHECK(check_set(NULL, 0, NULL) == 0);
    check_set(dup, 3, "twice");
    check_set(sub, 2, "substring");
    check_set(aa, 1, "suffix");
    check_set(cross, 2, "suffix");
    check_set(empty, 2, "0 bytes");
    CHECK(bpe_specials_check(NULL, NULL, 0) == 0);
    { /* 65 bytes, 64 bytes, 257 specials, a NUL */
        char big[66];
        memset(big, 'y', 65);
        big[0] = '<';
        big[65] = '\0';
        const char *const one[] = {big};
        check_set(one, 1, "65 bytes");
        big[64] = '\0';
        CHECK(check_set(one, 1, NULL) == 0);
        char names[257][8];
        const char *many[257];
        for (int i = 0; i < 257; i++) {
            snprintf(names[i], sizeof names[i], "<%d>", i);
            many[i] = names[i];
        }
        CHECK(check_set(many, 256, NULL) == 0);
        check_set(many, 257, "at most 256");
        struct set s = make_set(gpt2, 1);
        s.bytes[3] = 0;
        CHECK(bpe_specials_check(&s.sp, NULL, 0) == BPE_GPU_EINVAL);
        free_set(&s);
    }

    struct set s = make_set(chat, 3);
    { /* the three examples of bpe_gpu.h, BPE_SPLIT_GPT2 */
        const uint64_t w1[] = {0, 1, 3, 16}, p1[] = {2};
        split("a  <|endoftext|>", BPE_SPLIT_GPT2, NULL, NULL, &s, w1, 4, p1, 1);
        const uint64_t w2[] = {0, 13, 15}, p2[] = {0};
        split("<|endoftext|>'s", BPE_SPLIT_GPT2, NULL, NULL, &s, w2, 3, p2, 1);
        const uint64_t w3[] = {0, 1, 14, 16}, p3[] = {1};
        split("x<|endoftext|> y", BPE_SPLIT_GPT2, NULL, NULL, &s, w3, 4, p3, 1);
    }
    { /* adjacent matches, a match at each end, a text that ends in a prefix of a special, the empty text */
        const uint64_t w1[] = {0, 10, 23, 35, 36}, p1[] = {0, 1, 2};
        split("<|im_end|><|endoftext|><|im_start|>x", BPE_SPLIT_WORDS, NULL, NULL, &s, w1, 5, p1, 3);
        const uint64_t w2[] = {0, 1, 11, 12, 14, 16, 17, 19}, p2[] = {1};
        split("a<|im_end|>b<|im_en", BPE_SPLIT_WORDS, NULL, NULL, &s, w2, 8, p2, 1);
        const uint64_t w3[] = {0, 2, 15, 16}, p3[] = {1};
        split("a\n<|endoftext|>b", BPE_SPLIT_LINES, NULL, NULL, &s, w3, 4, p3, 1);
        const uint64_t w4[] = {0};
        split("", BPE_SPLIT_GPT2, NULL, NULL, &s, w4, 1, w4, 0);
    }
    { /* tables: every byte its own piece, and none but byte 0 */
        uint8_t *cls = calloc(256, 1);
        uint16_t *brk = calloc(16, sizeof *brk);
        CHECK(cls && brk);
        const uint64_t w1[] = {0, 2, 12, 14}, p1[] = {1};
        split("ab<|im_end|>cd", -1, cls, brk, &s, w1, 4, p1, 1);
        brk[0] = 1;
        const uint64_t w2[] = {0, 1, 2, 12, 13, 14};
        const uint64_t p2[] = {2};
        split("ab<|im_end|>cd", -1, cls, brk, &s, w2, 6, p2, 1);
        cls[7] = 16; /* a class above 15 */
        size_t count = 0;
        uint8_t x = 'x';
        CHECK(bpe_split_offsets_host_special(-1, cls, brk, &x, 1, &s.sp, NULL, 0, &count, NULL, NULL, 0, NULL) == BPE_GPU_EINVAL);
        CHECK(bpe_split_offsets_host_special(-1, NULL, NULL, &x, 1, &s.sp, NULL, 0, &count, NULL, NULL, 0, NULL) == BPE_GPU_EINVAL);
        CHECK(bpe_split_offsets_host_special(7, NULL, NULL, &x, 1, &s.sp, NULL, 0, &count, NULL, NULL, 0, NULL) == BPE_GPU_EINVAL);
        CHECK(bpe_split_offsets_host_special(BPE_SPLIT_WORDS, NULL, NULL, &x, 1, NULL, NULL, 0, &count, NULL, NULL, 0, NULL) == 0);
        CHECK(count == 2);
        free(cls);
        free(brk);
    }
    free_set(&s);
    { /* a refused set stops the split */
        struct set bad = make_set(aa, 1);
        size_t count = 0;
        uint8_t x = 'a';
        CHECK(bpe_split_offsets_host_special(BPE_SPLIT_WORDS, NULL, NULL, &x, 1, &bad.sp, NULL, 0, &count, NULL, NULL, 0, NULL) ==
              BPE_GPU_EINVAL);
        free_set(&bad);
    }
    printf("asan_special: ok\n");
    return 0;
}

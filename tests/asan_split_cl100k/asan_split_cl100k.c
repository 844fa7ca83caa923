/* Stand-alone sanitizer check of BPE_SPLIT_CL100K's host code (src/bpe_split_preset.c: the rule through
 * bpe_split_offsets_host; src/bpe_special.c: the preset through bpe_split_offsets_host_special): built with
 * -fsanitize=address,undefined.  The code under test calls no engine function; the three stubs below only
 * satisfy what bpe_split_preset.c's other entry points reference.  Every text is malloc'd to exactly its
 * length and every offset buffer to exactly its cap, so a byte read past the text (the letters of a
 * contraction the end cuts, a sequence the end cuts, the look-ahead through a white-space run) or an offset
 * written past cap is reported.  Test infrastructure only; `make asan-split-cl100k`, run by
 * tests/test_asan_split_cl100k.py.  Exits 0 and prints "asan_split_cl100k: ok". */
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
            fprintf(stderr, "asan_split_cl100k: %s:%d: %s\n", __FILE__, __LINE__, #x); \
            exit(1);                                                     \
        }                                                                \
    } while (0)

/* the pieces' lengths of text[0 .. n) as a string of digits, through the two-phase protocol and every cap */
static void lengths(const char *text, size_t n, const bpe_gpu_specials *sp, char *res, size_t res_cap)
{
    uint8_t *b = malloc(n ? n : 1);
    CHECK(b);
    memcpy(b, text, n);
    size_t cnt = 0;
    if (sp) CHECK(bpe_split_offsets_host_special(BPE_SPLIT_CL100K, NULL, NULL, b, n, sp, NULL, 0, &cnt, NULL, NULL, 0, NULL) == 0);
    else CHECK(bpe_split_offsets_host(BPE_SPLIT_CL100K, n ? b : NULL, n, NULL, 0, &cnt) == 0);
    CHECK(cnt >= 1 && cnt <= n + 1 && cnt <= res_cap);
    uint64_t *full = NULL;
    for (size_t cap = 0; cap <= cnt; cap++) { /* a cap smaller than the count: the count is whole, nothing is written past cap */
        uint64_t *out = malloc((cap ? cap : 1) * sizeof *out);
        CHECK(out);
        size_t again = 0;
        if (sp) CHECK(bpe_split_offsets_host_special(BPE_SPLIT_CL100K, NULL, NULL, b, n, sp, out, cap, &again, NULL, NULL, 0, NULL) == 0);
        else CHECK(bpe_split_offsets_host(BPE_SPLIT_CL100K, b, n, out, cap, &again) == 0);
        CHECK(again == cnt);
        if (cap == cnt) full = out;
        else free(out);
    }
    CHECK(full[0] == 0 && full[cnt - 1] == n);
    for (size_t d = 0; d + 1 < cnt; d++) {
        CHECK(full[d + 1] > full[d] && full[d + 1] - full[d] <= 40);
        res[d] = (char)('0' + (full[d + 1] - full[d]));
    }
    res[cnt - 1] = '\0';
    free(full);
    free(b);
}

static void lengths_are(const char *text, const char *want)
{
    char got[64];
    lengths(text, strlen(text), NULL, got, sizeof got);
    if (strcmp(got, want)) {
        fprintf(stderr, "asan_split_cl100k: \"%s\": pieces %s, expected %s\n", text, got, want);
        exit(1);
    }
}

int main(void)
{
    /* ---- the rule's named examples */
    lengths_are("don't", "32");
    lengths_are("DON'T", "32");
    lengths_are("'there", "24");
    lengths_are("'hello", "6");
    lengths_are(" 's", "21");
    lengths_are("12345", "32");
    lengths_are(" 123", "13");
    lengths_are("!\n\n  x", "312");
    lengths_are("x \n \ny", "141");
    lengths_are("a  b", "112");
    lengths_are("\"hi\"", "31");
    lengths_are("'\xc5\xbf", "3");                                  /* 'ſ: a contraction of three bytes */
    lengths_are("a'\xc5\xbf" "b", "131");
    lengths_are("\xd9\xa3\xd9\xa3\xd9\xa3\xd9\xa3\xc2\xbd", "64");  /* four arabic threes and one half: the run counts characters */
    lengths_are("", "");
    /* ---- texts that end in ', 'r, a truncated sequence, a digit and a space, after every kind of character */
    static const char *const heads[] = {"", "a", "1", " ", "\n", "!", "a ", "!\n\n", "\n ", "12", "123", "\xc3\xa9", "a'"};
    static const char *const tails[] = {"'", "'r", "'R", "'l", "'\xc5", "'s", "'re", "\xc3", "\xe4\xb8", "\xe3\x80", "\xf0\x9f\x98",
                                        "\xd9", "7", "77", " ", "  ", " \n", "\n "};
    for (size_t hd = 0; hd < sizeof heads / sizeof *heads; hd++)
        for (size_t t = 0; t < sizeof tails / sizeof *tails; t++) {
            char text[32], got[40];
            const size_t hl = strlen(heads[hd]), tl = strlen(tails[t]);
            memcpy(text, heads[hd], hl);
            memcpy(text + hl, tails[t], tl);
            lengths(text, hl + tl, NULL, got, sizeof got);
        }
    lengths_are("a'r", "12");   /* no contraction: the apostrophe is the letter's prefix */
    lengths_are("a're", "13");
    lengths_are("a'\xc5", "12");   /* the cut sequence is one byte of class P after the apostrophe */
    /* ---- through the special tokens' definition: a match breaks the run of numbers, the newlines after P, the look-ahead */
    {
        static const uint8_t spb[] = "<|endoftext|>\xac|x|";
        static const uint32_t spl[] = {13, 4};
        const bpe_gpu_specials sp = {spb, spl, 2};
        char got[40];
        const char *t1 = "1234<|endoftext|>5678";
        lengths(t1, strlen(t1), &sp, got, sizeof got);
        CHECK(!strcmp(got, "31=31")); /* ('=' is '0' + 13: the special) */
        const char *t2 = "!\n<|endoftext|>\n  \nx";
        lengths(t2, strlen(t2), &sp, got, sizeof got);
        CHECK(!strcmp(got, "2=41"));
        const char *t3 = "x\n  <|endoftext|> \ny";
        lengths(t3, strlen(t3), &sp, got, sizeof got);
        CHECK(!strcmp(got, "112=21"));
        const char *t4 = "a \xe2\x82\xac|x|'s";
        lengths(t4, strlen(t4), &sp, got, sizeof got);
        CHECK(!strcmp(got, "1342")); /* a | space E2 82 (the match cuts the sequence) | the special | 's */
        size_t cnt = 0;
        const uint8_t x = 'x';
        CHECK(bpe_split_offsets_host_special(BPE_SPLIT_CL100K, NULL, NULL, &x, 1, NULL, NULL, 0, &cnt, NULL, NULL, 0, NULL) == 0 && cnt == 2);
        CHECK(bpe_split_offsets_host(5, &x, 1, NULL, 0, &cnt) == BPE_GPU_EINVAL);
        CHECK(bpe_split_offsets_host(7, &x, 1, NULL, 0, &cnt) == BPE_GPU_EINVAL);
        CHECK(bpe_split_offsets_host(BPE_SPLIT_CL100K, NULL, 3, NULL, 0, &cnt) == BPE_GPU_EINVAL);
    }
    printf("asan_split_cl100k: ok\n");
    return 0;
}

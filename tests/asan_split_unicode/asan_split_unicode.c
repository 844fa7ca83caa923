/* Stand-alone sanitizer check of BPE_SPLIT_GPT2_UNICODE's host code (src/bpe_split_preset.c:
 * bpe_unicode_class, bpe_unicode_info, the preset through bpe_split_offsets_host; src/bpe_special.c:
 * the preset through bpe_split_offsets_host_special): built with -fsanitize=address,undefined.  The
 * code under test calls no engine function; the three stubs below only satisfy what
 * bpe_split_preset.c's other entry points reference.  Every text is malloc'd to exactly its length and
 * every offset buffer to exactly its cap, so a byte read past the text (a sequence the end cuts, the
 * look-ahead at end(i)) or an offset written past cap is reported.  Test infrastructure only; `make
 * asan-split-unicode`, run by tests/test_asan_split_unicode.py.  Exits 0 and prints
 * "asan_split_unicode: ok". */
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
            fprintf(stderr, "asan_split_unicode: %s:%d: %s\n", __FILE__, __LINE__, #x); \
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
    if (sp) CHECK(bpe_split_offsets_host_special(BPE_SPLIT_GPT2_UNICODE, NULL, NULL, b, n, sp, NULL, 0, &cnt, NULL, NULL, 0, NULL) == 0);
    else CHECK(bpe_split_offsets_host(BPE_SPLIT_GPT2_UNICODE, n ? b : NULL, n, NULL, 0, &cnt) == 0);
    CHECK(cnt >= 1 && cnt <= n + 1 && cnt <= res_cap);
    uint64_t *full = NULL;
    for (size_t cap = 0; cap <= cnt; cap++) { /* a cap smaller than the count: the count is whole, nothing is written past cap */
        uint64_t *out = malloc((cap ? cap : 1) * sizeof *out);
        CHECK(out);
        size_t again = 0;
        if (sp) CHECK(bpe_split_offsets_host_special(BPE_SPLIT_GPT2_UNICODE, NULL, NULL, b, n, sp, out, cap, &again, NULL, NULL, 0, NULL) == 0);
        else CHECK(bpe_split_offsets_host(BPE_SPLIT_GPT2_UNICODE, b, n, out, cap, &again) == 0);
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
        fprintf(stderr, "asan_split_unicode: \"%s\": pieces %s, expected %s\n", text, got, want);
        exit(1);
    }
}

int main(void)
{
    /* ---- the classes */
    CHECK(bpe_unicode_class(0) == 0 && bpe_unicode_class(0x10FFFF) == 0 && bpe_unicode_class(0x110000) == 0);
    CHECK(bpe_unicode_class(UINT32_MAX) == 0 && bpe_unicode_class(0xD800) == 0 && bpe_unicode_class(0x1C) == 0);
    CHECK(bpe_unicode_class('A') == 1 && bpe_unicode_class(0xE9) == 1 && bpe_unicode_class(0x4E2D) == 1 && bpe_unicode_class(0x10400) == 1);
    CHECK(bpe_unicode_class('7') == 2 && bpe_unicode_class(0x663) == 2 && bpe_unicode_class(0xBD) == 2 && bpe_unicode_class(0x1D7D8) == 2);
    CHECK(bpe_unicode_class(0x20) == 3 && bpe_unicode_class('\n') == 4 && bpe_unicode_class(0xA0) == 4 && bpe_unicode_class(0x3000) == 4);
    CHECK(bpe_unicode_class(0x2014) == 0 && bpe_unicode_class(0x1F600) == 0 && bpe_unicode_class(0x301) == 0);
    uint64_t h = 0xCBF29CE484222325ull, digest = 0; /* the digest over all code points: every table entry is read */
    for (uint32_t cp = 0; cp < 0x110000; cp++) h = (h ^ (uint64_t)bpe_unicode_class(cp)) * 0x100000001B3ull;
    const char *source = NULL;
    CHECK(bpe_unicode_info(&source, &digest) == 0 && digest == h && source && !strncmp(source, "regex ", 6));
    CHECK(bpe_unicode_info(NULL, NULL) == 0 && bpe_unicode_info(&source, NULL) == 0 && bpe_unicode_info(NULL, &digest) == 0);

    /* ---- the rule: letters, numbers, white space and punctuation beyond ASCII */
    lengths_are("a\xe2\x80\x94" "b \xe2\x82\xac" "5", "13141");          /* a | em dash | b | space euro | 5 */
    lengths_are("x\xd9\xa3\xc2\xbdy", "141");                           /* x | arabic three, one half | y */
    lengths_are("e\xcc\x81's", "131");                                  /* e | combining acute, apostrophe | s */
    lengths_are("\xc3\xa9's", "22");                                    /* e-acute | 's */
    lengths_are("a\xe3\x80\x80\xe3\x80\x80" "b\xe2\x80\xa8", "13313");  /* the last white space before text splits off */
    lengths_are("a\xc2\xa0 b", "122");
    lengths_are("a\x1c b", "112");
    lengths_are("\xf0\x90\x90\x80\xf0\x9d\x9f\x98", "44");
    lengths_are("", "");
    /* ill-formed bytes are characters of their own, class P: an overlong form, a surrogate, above U+10FFFF, FF */
    lengths_are("a\xc0\x80" "b", "121");
    lengths_are("a\xed\xa0\x80" "b", "131");
    lengths_are("a\xf4\x90\x80\x80\xff" "b", "151");
    /* ---- a sequence cut by n at every length: the bytes left are ill-formed, and nothing past n is read */
    static const char *const seqs[] = {"\xc3\xa9", "\xe4\xb8\xad", "\xe3\x80\x80", "\xf0\x90\x90\x80", "\xf0\x9f\x98\x80"};
    static const char *const heads[] = {"", "a", " ", "a ", "a'", "\xc3\xa9", "a\n\n"};
    for (size_t s = 0; s < sizeof seqs / sizeof *seqs; s++)
        for (size_t hd = 0; hd < sizeof heads / sizeof *heads; hd++)
            for (size_t k = 1; k <= strlen(seqs[s]); k++) {
                char text[16], got[32];
                const size_t hl = strlen(heads[hd]);
                memcpy(text, heads[hd], hl);
                memcpy(text + hl, seqs[s], k);
                lengths(text, hl + k, NULL, got, sizeof got);
                if (k < strlen(seqs[s]) && hl == 1 && text[0] == 'a') CHECK(got[0] == '1' && (size_t)(got[1] - '0') == k && !got[2]);
            }
    /* ---- through the special tokens' definition: a match cuts a sequence */
    {
        static const uint8_t spb[] = "<|endoftext|>\xac|x|";
        static const uint32_t spl[] = {13, 4};
        const bpe_gpu_specials sp = {spb, spl, 2};
        char got[32];
        const char *t1 = "a \xe2\x82\xac|x| b";
        lengths(t1, strlen(t1), &sp, got, sizeof got);
        CHECK(!strcmp(got, "1342")); /* a | space E2 82 (ill-formed: class P) | the special | space b */
        const char *t2 = "\xc3\xa9<|endoftext|>'s \xe4\xb8";
        lengths(t2, strlen(t2), &sp, got, sizeof got);
        CHECK(!strcmp(got, "2=23")); /* ('=' is '0' + 13: the special; 's begins its segment; the cut sequence is two bytes of class P) */
        size_t cnt = 0;
        const uint8_t x = 'x';
        CHECK(bpe_split_offsets_host_special(BPE_SPLIT_GPT2_UNICODE, NULL, NULL, &x, 1, NULL, NULL, 0, &cnt, NULL, NULL, 0, NULL) == 0 && cnt == 2);
        CHECK(bpe_split_offsets_host(5, &x, 1, NULL, 0, &cnt) == BPE_GPU_EINVAL);
        CHECK(bpe_split_offsets_host(BPE_SPLIT_GPT2_UNICODE, NULL, 3, NULL, 0, &cnt) == BPE_GPU_EINVAL);
    }
    printf("asan_split_unicode: ok\n");
    return 0;
}

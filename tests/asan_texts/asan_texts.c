/* Stand-alone sanitizer check of the text batches' host code (src/bpe_texts.c: bpe_texts_check and
 * bpe_texts_gap, bpe_texts_gap_range): built with -fsanitize=address,undefined.  The code under test calls no engine function.
 * Every buffer handed over is malloc'd to exactly the size the call may touch, so an offset read past
 * text_off[T], a byte read past the texts or written past n + T is reported.  Test infrastructure only;
 * `make asan-texts`, run by tests/test_asan_texts.py.  Exits 0 and prints "asan_texts: ok". */
#include "../../include/bpe_ex.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define CHECK(x)                                                         \
    do {                                                                 \
        if (!(x)) {                                                      \
            fprintf(stderr, "asan_texts: %s:%d: %s\n", __FILE__, __LINE__, #x); \
            exit(1);                                                     \
        }                                                                \
    } while (0)

/* T texts of the lengths len[0 .. T): the check accepts them and the gapped bytes are each text and a NUL */
static void accept(const size_t *len, size_t T)
{
    size_t n = 0;
    for (size_t k = 0; k < T; k++) n += len[k];
    uint64_t *off = malloc((T + 1) * sizeof *off);
    uint8_t *bytes = n ? malloc(n) : NULL, *out = n + T ? malloc(n + T) : NULL;
    CHECK(off && (!n || bytes) && (!(n + T) || out));
    off[0] = 0;
    for (size_t k = 0; k < T; k++) off[k + 1] = off[k] + len[k];
    for (size_t i = 0; i < n; i++) bytes[i] = (uint8_t)(i % 7 ? 1 + i % 250 : 0); /* NULs inside the texts too */
    char msg[400];
    CHECK(bpe_texts_check(off, T, n, msg, sizeof msg) == 0 && msg[0] == '\0');
    CHECK(bpe_texts_check(off, T, n, NULL, 0) == 0);
    if (n + T) memset(out, 0xAA, n + T);
    CHECK(bpe_texts_gap(bytes, n, off, T, out, n + T) == 0);
    size_t at = 0;
    for (size_t k = 0; k < T; k++) {
        CHECK(len[k] == 0 || memcmp(out + at, bytes + off[k], len[k]) == 0);
        at += len[k];
        CHECK(out[at++] == 0);
    }
    CHECK(at == n + T);
    if (n + T) CHECK(bpe_texts_gap(bytes, n, off, T, out, n + T - 1) == BPE_GPU_EINVAL); /* a byte too little room */
    /* every stretch that begins or ends at a gap or a byte beside one (all of them for a small batch), each
       into a buffer of exactly its size */
    for (size_t lo = 0; lo <= n + T; lo += (n + T > 64 ? 37 : 1))
        for (size_t hi = lo; hi <= n + T; hi += (n + T > 64 ? 41 : 1)) {
            uint8_t *part = hi > lo ? malloc(hi - lo) : NULL;
            CHECK(hi == lo || part);
            CHECK(bpe_texts_gap_range(bytes, n, off, T, lo, hi, part) == 0);
            CHECK(hi == lo || memcmp(part, out + lo, hi - lo) == 0);
            free(part);
        }
    CHECK(bpe_texts_gap_range(bytes, n, off, T, 1, 0, out) == BPE_GPU_EINVAL);
    CHECK(bpe_texts_gap_range(bytes, n, off, T, 0, n + T + 1, out) == BPE_GPU_EINVAL);
    free(off);
    free(bytes);
    free(out);
}

/* the offsets off[0 .. T] over n bytes are refused and the message holds `word` */
static void refuse(const uint64_t *src, size_t T, size_t n, const char *word)
{
    uint64_t *off = malloc((T + 1) * sizeof *off);
    char *msg = malloc(400), *tiny = malloc(8);
    CHECK(off && msg && tiny);
    memcpy(off, src, (T + 1) * sizeof *off);
    CHECK(bpe_texts_check(off, T, n, msg, 400) == BPE_GPU_EINVAL);
    CHECK(strncmp(msg, "texts: ", 7) == 0 && strstr(msg, word));
    CHECK(bpe_texts_check(off, T, n, tiny, 8) == BPE_GPU_EINVAL && strlen(tiny) == 7); /* cut to its room */
    CHECK(bpe_texts_check(off, T, n, NULL, 0) == BPE_GPU_EINVAL);
    uint8_t *out = malloc(n + T + 1);
    CHECK(out);
    if (n <= 64) { /* (the refusals over huge n name no bytes) */
        uint8_t *bytes = malloc(n + 1);
        CHECK(bytes);
        memset(bytes, 'x', n + 1);
        CHECK(bpe_texts_gap(bytes, n, off, T, out, n + T) == BPE_GPU_EINVAL);
        free(bytes);
    }
    free(out);
    free(off);
    free(msg);
    free(tiny);
}

int main(void)
{
    accept(NULL, 0); /* T = 0 */
    const size_t empty[5] = {0, 0, 0, 0, 0};
    accept(empty, 1);
    accept(empty, 5); /* all texts empty */
    const size_t one[1] = {13};
    accept(one, 1); /* one text */
    const size_t mixed[9] = {0, 3, 0, 0, 1, 64, 0, 7, 0};
    accept(mixed, 9);
    size_t *many = malloc(1000 * sizeof *many);
    CHECK(many);
    for (size_t k = 0; k < 1000; k++) many[k] = k % 4;
    accept(many, 1000);
    free(many);

    const uint64_t first[2] = {1, 5};
    refuse(first, 1, 5, "offset 0 is 1");
    const uint64_t falls[4] = {0, 4, 3, 9};
    refuse(falls, 3, 9, "offset 2 (3) is below offset 1 (4)");
    const uint64_t falls_last[4] = {0, 4, 4, 2};
    refuse(falls_last, 3, 2, "offset 3 (2) is below offset 2 (4)");
    const uint64_t shorter[3] = {0, 4, 8};
    refuse(shorter, 2, 9, "offset 2, the last, is 8");
    const uint64_t longer[3] = {0, 4, 10};
    refuse(longer, 2, 9, "offset 2, the last, is 10");
    const uint64_t none[1] = {0};
    refuse(none, 0, 3, "offset 0, the last, is 0");
    CHECK(bpe_texts_check(NULL, 0, 0, NULL, 0) == BPE_GPU_EINVAL);
    /* the position limit, reached by the bytes, by the gaps and by both (the offsets are not read then) */
    char msg[400];
    CHECK(bpe_texts_check(none, 1, (size_t)BPE_TEXTS_MAX_POSITIONS, msg, sizeof msg) == BPE_GPU_EINVAL && strstr(msg, "1 gap bytes"));
    CHECK(bpe_texts_check(none, (size_t)BPE_TEXTS_MAX_POSITIONS + 1, 0, msg, sizeof msg) == BPE_GPU_EINVAL);
    CHECK(bpe_texts_check(none, (size_t)-1, (size_t)-1, msg, sizeof msg) == BPE_GPU_EINVAL);
    const uint64_t edge[2] = {0, BPE_TEXTS_MAX_POSITIONS - 1};
    CHECK(bpe_texts_check(edge, 1, (size_t)BPE_TEXTS_MAX_POSITIONS - 1, msg, sizeof msg) == 0);
    printf("asan_texts: ok\n");
    return 0;
}

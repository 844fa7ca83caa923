/* Stand-alone sanitizer check of the packed streams' host code (src/bpe_stream.c: bpe_stream_check and
 * bpe_pack_stream_host): built with -fsanitize=address,undefined.  The code under test calls no engine function.
 * Every buffer handed over is malloc'd to exactly the size the call may touch (rows_cap == R exactly), so an offset
 * read past text_off[T], an id read past the ids or a cell written past the rows is reported.  The rows are held to
 * a second, cell-by-cell statement of the contract.  Test infrastructure only; `make asan-stream`, run by
 * tests/test_asan_stream.py.  Exits 0 and prints "asan_stream: ok". */
#include "../../include/bpe_ex.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define CHECK(x)                                                          \
    do {                                                                  \
        if (!(x)) {                                                       \
            fprintf(stderr, "asan_stream: %s:%d: %s\n", __FILE__, __LINE__, #x); \
            exit(1);                                                      \
        }                                                                 \
    } while (0)

/* T texts of the lengths len[0 .. T) under every BOS / EOS / drop_last combination and a few row lengths */
static void accept(const size_t *len, size_t T)
{
    size_t n = 0;
    for (size_t k = 0; k < T; k++) n += len[k];
    uint64_t *off = malloc((T + 1) * sizeof *off);
    uint32_t *ids = n ? malloc(n * sizeof *ids) : NULL;
    CHECK(off && (!n || ids));
    off[0] = 0;
    for (size_t k = 0; k < T; k++) off[k + 1] = off[k] + len[k];
    for (size_t i = 0; i < n; i++) ids[i] = (uint32_t)(1000 + i % 5000);
    const uint32_t Ls[5] = {1, 3, 4, 7, 64};
    for (size_t li = 0; li < 5; li++)
        for (uint32_t flags = 0; flags < 8; flags++) {
            const bpe_gpu_stream s = {Ls[li], flags, 0xFFFFFFF0u, 0xFFFFFFF1u, 0xFFFFFFFFu};
            const uint64_t b = flags & BPE_STREAM_BOS ? 1 : 0, e = flags & BPE_STREAM_EOS ? 1 : 0, L = Ls[li];
            const uint64_t N = n + T * (b + e), R = flags & BPE_STREAM_DROP_LAST ? N / L : (N + L - 1) / L;
            size_t nr = 99;
            uint64_t ns = 99;
            CHECK(bpe_pack_stream_host(ids, n, off, T, &s, NULL, NULL, NULL, 0, &nr, &ns) == 0); /* the query */
            CHECK(nr == R && ns == N);
            CHECK(bpe_pack_stream_host(ids, n, off, T, &s, NULL, NULL, NULL, 0, NULL, NULL) == 0);
            const size_t cells = (size_t)(R * L);
            uint32_t *rows = malloc(cells ? cells * 4 : 1), *seg = malloc(cells ? cells * 4 : 1), *pos = malloc(cells ? cells * 4 : 1);
            CHECK(rows && seg && pos);
            CHECK(bpe_pack_stream_host(ids, n, off, T, &s, rows, seg, pos, (size_t)R, &nr, &ns) == 0); /* rows_cap == R */
            CHECK(nr == R && ns == N);
            /* cell by cell: the text of cell c is found by walking the texts' starts */
            size_t k = 0;
            uint64_t start = 0; /* of text k */
            for (uint64_t c = 0; c < cells; c++) {
                if (c >= N) {
                    CHECK(rows[c] == s.pad_id && seg[c] == BPE_STREAM_NO_TEXT && pos[c] == 0);
                    continue;
                }
                while (c >= start + b + len[k] + e) start += b + len[k++] + e;
                const uint64_t o = c - start, row0 = c / L * L;
                const uint32_t want = b && o == 0 ? s.bos_id : o - b < len[k] ? ids[off[k] + o - b] : s.eos_id;
                CHECK(rows[c] == want && seg[c] == k && pos[c] == c - (start > row0 ? start : row0));
            }
            /* the optional outputs left out, one by one */
            uint32_t *rows2 = malloc(cells ? cells * 4 : 1);
            CHECK(rows2);
            CHECK(bpe_pack_stream_host(ids, n, off, T, &s, rows2, NULL, pos, (size_t)R, NULL, NULL) == 0);
            CHECK(!cells || memcmp(rows, rows2, cells * 4) == 0);
            CHECK(bpe_pack_stream_host(ids, n, off, T, &s, rows2, seg, NULL, (size_t)R, NULL, NULL) == 0);
            CHECK(bpe_pack_stream_host(ids, n, off, T, &s, rows2, NULL, NULL, (size_t)R, NULL, NULL) == 0);
            CHECK(!cells || memcmp(rows, rows2, cells * 4) == 0);
            if (R) /* a row too little room */
                CHECK(bpe_pack_stream_host(ids, n, off, T, &s, rows2, NULL, NULL, (size_t)R - 1, NULL, NULL) == BPE_GPU_EINVAL);
            free(rows);
            free(seg);
            free(pos);
            free(rows2);
        }
    free(off);
    free(ids);
}

/* the description is refused with `code` and the message holds `word` */
static void refuse(uint32_t seq_len, uint32_t flags, int code, const char *word)
{
    bpe_gpu_stream *s = malloc(sizeof *s);
    char *msg = malloc(400), *tiny = malloc(9);
    CHECK(s && msg && tiny);
    *s = (bpe_gpu_stream){seq_len, flags, 1, 2, 3};
    CHECK(bpe_stream_check(s, msg, 400) == code);
    CHECK(strncmp(msg, "stream: ", 8) == 0 && strstr(msg, word));
    CHECK(bpe_stream_check(s, tiny, 9) == code && strlen(tiny) == 8); /* cut to its room */
    CHECK(bpe_stream_check(s, NULL, 0) == code);
    const uint64_t off[2] = {0, 1};
    const uint32_t id[1] = {5};
    uint32_t cell[1] = {77};
    size_t nr = 99;
    CHECK(bpe_pack_stream_host(id, 1, off, 1, s, cell, NULL, NULL, 1, &nr, NULL) == code && cell[0] == 77 && nr == 99);
    free(s);
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
    accept(many, 1000); /* a thousand texts */
    for (size_t k = 0; k < 1000; k++) many[k] = (k * 7) % 23;
    accept(many, 1000);
    free(many);

    refuse(0, 0, BPE_GPU_EINVAL, "seq_len is 0");
    refuse(0, 8, BPE_GPU_EINVAL, "seq_len is 0");
    refuse(16, 8, BPE_GPU_EINVAL, "flags 0x8");
    refuse(16, 0x80000007u, BPE_GPU_EINVAL, "flags 0x80000007");
    refuse(BPE_STREAM_SEQ_MAX + 1, 3, BPE_GPU_ERANGE, "above 2^24");
    refuse(0xFFFFFFFFu, 0, BPE_GPU_ERANGE, "above 2^24");
    CHECK(bpe_stream_check(NULL, NULL, 0) == BPE_GPU_EINVAL);
    char msg[400];
    CHECK(bpe_stream_check(NULL, msg, sizeof msg) == BPE_GPU_EINVAL && strstr(msg, "no description"));
    const bpe_gpu_stream edge = {BPE_STREAM_SEQ_MAX, 7, 0, 0, 0};
    CHECK(bpe_stream_check(&edge, msg, sizeof msg) == 0 && msg[0] == '\0');
    /* offsets that do not describe the ids */
    const bpe_gpu_stream s = {4, 3, 1, 2, 3};
    const uint32_t ids[4] = {9, 8, 7, 6};
    uint32_t rows[12];
    const uint64_t first[3] = {1, 2, 4}, falls[3] = {0, 5, 4}, shorter[3] = {0, 2, 3}, longer[3] = {0, 2, 5};
    CHECK(bpe_pack_stream_host(ids, 4, first, 2, &s, rows, NULL, NULL, 3, NULL, NULL) == BPE_GPU_EINVAL);
    CHECK(bpe_pack_stream_host(ids, 4, falls, 2, &s, rows, NULL, NULL, 3, NULL, NULL) == BPE_GPU_EINVAL);
    CHECK(bpe_pack_stream_host(ids, 4, shorter, 2, &s, rows, NULL, NULL, 3, NULL, NULL) == BPE_GPU_EINVAL);
    CHECK(bpe_pack_stream_host(ids, 4, longer, 2, &s, rows, NULL, NULL, 3, NULL, NULL) == BPE_GPU_EINVAL);
    CHECK(bpe_pack_stream_host(ids, 4, NULL, 2, &s, rows, NULL, NULL, 3, NULL, NULL) == BPE_GPU_EINVAL);
    CHECK(bpe_pack_stream_host(NULL, 4, shorter, 2, &s, rows, NULL, NULL, 3, NULL, NULL) == BPE_GPU_EINVAL);
    printf("asan_stream: ok\n");
    return 0;
}

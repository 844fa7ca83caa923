/* Stand-alone sanitizer check of rows back to texts' host code (src/bpe_rows.c: bpe_rows_check and
 * bpe_unpack_rows_host): built with -fsanitize=address,undefined.  The code under test calls no engine function.
 * Every buffer handed over is malloc'd to exactly the size the call may touch (the rows end with the last row's last
 * cell, not with its stride; ids_cap == n exactly), so a cell read past a row, a window or the grid and an id written
 * past the ids is reported.  The results are held to a second, cell-by-cell statement of the contract.  Test
 * infrastructure only; `make asan-rows`, run by tests/test_asan_rows.py.  Exits 0 and prints "asan_rows: ok". */
#include "../../include/bpe_ex.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define CHECK(x)                                                        \
    do {                                                                \
        if (!(x)) {                                                     \
            fprintf(stderr, "asan_rows: %s:%d: %s\n", __FILE__, __LINE__, #x); \
            exit(1);                                                    \
        }                                                               \
    } while (0)

static uint64_t rng_state = 88172645463325252ull;
static uint32_t rnd(uint32_t below)
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return below ? (uint32_t)((rng_state >> 11) % below) : 0;
}

static int64_t cell_at(const void *rows, int cb, size_t i)
{
    return cb == 4 ? (int64_t)((const uint32_t *)rows)[i] : ((const int64_t *)rows)[i];
}

static int in_list(const uint32_t *list, uint32_t n, int64_t v)
{
    for (uint32_t j = 0; j < n; j++)
        if ((int64_t)list[j] == v) return 1;
    return 0;
}

/* B rows of L cells of cb bytes, row_stride cells apart, under every flag combination, with and without lens */
static void accept(size_t B, uint32_t L, size_t stride, int cb)
{
    /* the grid ends with the last row's last cell */
    const size_t cells = B ? (B - 1) * stride + L : 0;
    void *rows = cells ? malloc(cells * (size_t)cb) : NULL;
    uint32_t *lens = B ? malloc(B * sizeof *lens) : NULL;
    CHECK((!cells || rows) && (!B || lens));
    const uint32_t pad = 2, skip[5] = {9, 4, 9, 250, 6};
    for (size_t i = 0; i < cells; i++) {
        const uint32_t v = rnd(4) ? rnd(12) : pad;
        if (cb == 4) ((uint32_t *)rows)[i] = v;
        else ((int64_t *)rows)[i] = v;
    }
    for (size_t k = 0; k < B; k++) lens[k] = rnd(L + 1);
    if (B) lens[B - 1] = L; /* the last row's last cell is read */
    for (uint32_t flags = 0; flags < 4; flags++)
        for (uint32_t n_stop = 0; n_stop <= 8; n_stop += 4)
            for (int with_lens = 0; with_lens < 2; with_lens++) {
                bpe_gpu_rows d = {flags, pad, n_stop, {7, 3, 2, 100, 101, 102, 103, 11}, 5, skip};
                const uint32_t *ln = with_lens ? lens : NULL;
                size_t n = 99;
                char msg[400];
                CHECK(bpe_unpack_rows_host(rows, cb, B, L, stride, ln, &d, NULL, 0, &n, NULL, NULL, msg, sizeof msg) == 0); /* the query */
                CHECK(bpe_unpack_rows_host(rows, cb, B, L, stride, ln, &d, NULL, 0, NULL, NULL, NULL, NULL, 0) == 0);
                uint32_t *ids = malloc(n ? n * 4 : 1), *bounds = malloc(B ? B * 8 : 1);
                uint64_t *off = malloc((B + 1) * 8);
                CHECK(ids && bounds && off);
                size_t n2 = 0;
                CHECK(bpe_unpack_rows_host(rows, cb, B, L, stride, ln, &d, n ? ids : NULL, n, &n2, off, B ? bounds : NULL, msg,
                                           sizeof msg) == 0); /* ids_cap == n */
                CHECK(n2 == n && off[0] == 0 && off[B] == n);
                /* cell by cell */
                size_t at = 0;
                for (size_t k = 0; k < B; k++) {
                    const uint32_t win = ln ? ln[k] : L;
                    uint32_t a = 0;
                    if (flags & BPE_ROWS_PAD)
                        while (a < win && cell_at(rows, cb, k * stride + a) == pad) a++;
                    uint32_t z = a;
                    for (; z < win; z++) {
                        const int64_t v = cell_at(rows, cb, k * stride + z);
                        if (in_list(d.stop, n_stop, v) || ((flags & BPE_ROWS_PAD) && v == pad)) break;
                    }
                    CHECK(bounds[2 * k] == a && bounds[2 * k + 1] == z && off[k] == at);
                    for (uint32_t c = a; c < z; c++) {
                        const int64_t v = cell_at(rows, cb, k * stride + c);
                        if ((flags & BPE_ROWS_SKIP) && in_list(skip, 5, v)) continue;
                        CHECK(at < n && ids[at] == (uint32_t)v);
                        at++;
                    }
                }
                CHECK(at == n);
                if (n) { /* an id too little room: refused, nothing written */
                    memset(ids, 0x5A, n * 4);
                    off[0] = 77;
                    CHECK(bpe_unpack_rows_host(rows, cb, B, L, stride, ln, &d, ids, n - 1, &n2, off, bounds, msg, sizeof msg) ==
                          BPE_GPU_EINVAL);
                    CHECK(strstr(msg, "ids_cap") && ids[0] == 0x5A5A5A5Au && off[0] == 77);
                }
                free(ids);
                free(bounds);
                free(off);
            }
    free(rows);
    free(lens);
}

/* the description is refused with `code` and the message holds `word` */
static void refuse(bpe_gpu_rows d, int code, const char *word)
{
    bpe_gpu_rows *p = malloc(sizeof *p);
    char *msg = malloc(400), *tiny = malloc(7);
    CHECK(p && msg && tiny);
    *p = d;
    CHECK(bpe_rows_check(p, msg, 400) == code);
    CHECK(strncmp(msg, "rows: ", 6) == 0 && strstr(msg, word));
    CHECK(bpe_rows_check(p, tiny, 7) == code && strlen(tiny) == 6); /* cut to its room */
    CHECK(bpe_rows_check(p, NULL, 0) == code);
    const uint32_t cell[1] = {5};
    uint32_t id[1] = {77};
    size_t n = 99;
    CHECK(bpe_unpack_rows_host(cell, 4, 1, 1, 1, NULL, p, id, 1, &n, NULL, NULL, msg, 400) == code && id[0] == 77 && n == 99);
    free(p);
    free(msg);
    free(tiny);
}

int main(void)
{
    for (int cb = 4; cb <= 8; cb += 4) {
        accept(0, 0, 0, cb);   /* B == 0 and L == 0 */
        accept(0, 5, 5, cb);   /* B == 0 */
        accept(6, 0, 0, cb);   /* L == 0 */
        accept(6, 0, 3, cb);   /* L == 0 in rows that are not */
        accept(1, 1, 1, cb);
        accept(9, 7, 7, cb);
        accept(9, 7, 12, cb);  /* row_stride > L */
        accept(40, 65, 65, cb);
        accept(40, 65, 100, cb);
    }

    const uint32_t skip[1] = {1};
    refuse((bpe_gpu_rows){4, 0, 0, {0}, 0, NULL}, BPE_GPU_EINVAL, "flags 0x4");
    refuse((bpe_gpu_rows){0x80000001u, 0, 0, {0}, 0, NULL}, BPE_GPU_EINVAL, "flags 0x80000001");
    refuse((bpe_gpu_rows){1, 0, 9, {0}, 0, NULL}, BPE_GPU_EINVAL, "n_stop 9 above 8");
    refuse((bpe_gpu_rows){2, 0, 0, {0}, 257, skip}, BPE_GPU_EINVAL, "n_skip 257 above 256");
    refuse((bpe_gpu_rows){2, 0, 0, {0}, 1, NULL}, BPE_GPU_EINVAL, "skip is NULL");
    char msg[400];
    CHECK(bpe_rows_check(NULL, NULL, 0) == BPE_GPU_EINVAL);
    CHECK(bpe_rows_check(NULL, msg, sizeof msg) == BPE_GPU_EINVAL && strstr(msg, "no description"));
    const bpe_gpu_rows skip_unread = {1, 0, 8, {0}, 1000, NULL}; /* without BPE_ROWS_SKIP the list is not looked at */
    CHECK(bpe_rows_check(&skip_unread, msg, sizeof msg) == 0 && msg[0] == '\0');

    /* the call's own refusals */
    const bpe_gpu_rows d = {1, 0, 1, {9}, 0, NULL};
    int64_t *rows = malloc(6 * sizeof *rows);
    uint32_t *lens = malloc(2 * sizeof *lens), ids[6] = {77, 77, 77, 77, 77, 77};
    CHECK(rows && lens);
    const int64_t init[6] = {0, 4, 9, -100, 5, 6};
    memcpy(rows, init, sizeof init);
    size_t n = 99;
    CHECK(bpe_unpack_rows_host(rows, 2, 2, 3, 3, NULL, &d, ids, 6, &n, NULL, NULL, msg, sizeof msg) == BPE_GPU_EINVAL && strstr(msg, "cell_bytes 2"));
    CHECK(bpe_unpack_rows_host(rows, 8, 2, 3, 2, NULL, &d, ids, 6, &n, NULL, NULL, msg, sizeof msg) == BPE_GPU_EINVAL && strstr(msg, "row_stride 2 below L 3"));
    CHECK(bpe_unpack_rows_host(rows, 8, 0, BPE_ROWS_LEN_MAX + 1, BPE_ROWS_LEN_MAX + 1, NULL, &d, ids, 6, &n, NULL, NULL, msg, sizeof msg) == BPE_GPU_ERANGE && strstr(msg, "above 2^24"));
    CHECK(bpe_unpack_rows_host(NULL, 8, 2, 3, 3, NULL, &d, ids, 6, &n, NULL, NULL, msg, sizeof msg) == BPE_GPU_EINVAL && strstr(msg, "rows is NULL"));
    lens[0] = 3, lens[1] = 4;
    CHECK(bpe_unpack_rows_host(rows, 8, 2, 3, 3, lens, &d, ids, 6, &n, NULL, NULL, msg, sizeof msg) == BPE_GPU_EINVAL && strstr(msg, "lens[1] is 4, above the row length 3"));
    lens[0] = 5;
    CHECK(bpe_unpack_rows_host(rows, 8, 2, 3, 3, lens, &d, ids, 6, &n, NULL, NULL, NULL, 0) == BPE_GPU_EINVAL);
    CHECK(bpe_unpack_rows_host(rows, 8, 2, 3, 3, lens, &d, ids, 6, &n, NULL, NULL, msg, sizeof msg) == BPE_GPU_EINVAL && strstr(msg, "lens[0] is 5"));
    /* -100 in row 1's text */
    CHECK(bpe_unpack_rows_host(rows, 8, 2, 3, 3, NULL, &d, ids, 6, &n, NULL, NULL, msg, sizeof msg) == BPE_GPU_EDATA && strstr(msg, "row 1 keeps a cell"));
    CHECK(n == 99 && ids[0] == 77);
    lens[0] = 3, lens[1] = 0; /* ... and outside its window */
    CHECK(bpe_unpack_rows_host(rows, 8, 2, 3, 3, lens, &d, ids, 6, &n, NULL, NULL, msg, sizeof msg) == 0 && n == 1 && ids[0] == 4 && msg[0] == '\0');
    rows[3] = 9; /* behind a stop at the row's first cell */
    rows[4] = (int64_t)1 << 40;
    CHECK(bpe_unpack_rows_host(rows, 8, 2, 3, 3, NULL, &d, ids, 6, &n, NULL, NULL, msg, sizeof msg) == 0 && n == 1);
    free(rows);
    free(lens);
    printf("asan_rows: ok\n");
    return 0;
}

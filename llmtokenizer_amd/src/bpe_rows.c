/*
 * bpe_rows.c -- rows back to texts on the host, in plain C and without a GPU
 * (bpe_ex.h; the contract: bpe_gpu.h, "Rows back to texts"): bpe_rows_check (the
 * flags and the counts of a bpe_gpu_rows; the message names the field) and
 * bpe_unpack_rows_host (every row's start, end and kept ids, row by row and cell
 * by cell: the definition the device is held to).  bpe_gpu_unpack_rows checks
 * with the first.
 */
#include "../../include/bpe_ex.h"

#include <stdio.h>
#include <string.h>

static int refuse(int code, char *msg, size_t cap, const char *text)
{
    if (msg && cap) snprintf(msg, cap, "rows: %s", text);
    return code;
}

int bpe_rows_check(const bpe_gpu_rows *d, char *msg, size_t cap)
{
    char text[200];
    if (msg && cap) msg[0] = '\0';
    if (!d) return refuse(BPE_GPU_EINVAL, msg, cap, "no description given");
    if (d->flags & ~(uint32_t)BPE_ROWS_FLAGS) {
        snprintf(text, sizeof text, "flags 0x%x hold a bit that is neither BPE_ROWS_PAD nor BPE_ROWS_SKIP", (unsigned)d->flags);
        return refuse(BPE_GPU_EINVAL, msg, cap, text);
    }
    if (d->n_stop > BPE_ROWS_STOP_MAX) {
        snprintf(text, sizeof text, "n_stop %u above %d", (unsigned)d->n_stop, BPE_ROWS_STOP_MAX);
        return refuse(BPE_GPU_EINVAL, msg, cap, text);
    }
    if (d->flags & BPE_ROWS_SKIP) {
        if (d->n_skip > BPE_ROWS_SKIP_MAX) {
            snprintf(text, sizeof text, "n_skip %u above %d", (unsigned)d->n_skip, BPE_ROWS_SKIP_MAX);
            return refuse(BPE_GPU_EINVAL, msg, cap, text);
        }
        if (d->n_skip && !d->skip) {
            snprintf(text, sizeof text, "skip is NULL with n_skip %u", (unsigned)d->n_skip);
            return refuse(BPE_GPU_EINVAL, msg, cap, text);
        }
    }
    return 0;
}

/* cell c of a row: its value, and whether that is an id */
static int cell_id(const void *row, int cell_bytes, size_t c, uint32_t *id)
{
    if (cell_bytes == 4) {
        *id = ((const uint32_t *)row)[c];
        return 1;
    }
    const int64_t v = ((const int64_t *)row)[c];
    *id = (uint32_t)v;
    return v >= 0 && v <= (int64_t)0xFFFFFFFFll;
}

static int is_stop(const bpe_gpu_rows *d, uint32_t id)
{
    if ((d->flags & BPE_ROWS_PAD) && id == d->pad_id) return 1;
    for (uint32_t j = 0; j < d->n_stop; j++)
        if (d->stop[j] == id) return 1;
    return 0;
}

static int is_skipped(const bpe_gpu_rows *d, uint32_t id)
{
    if (!(d->flags & BPE_ROWS_SKIP)) return 0;
    for (uint32_t j = 0; j < d->n_skip; j++)
        if (d->skip[j] == id) return 1;
    return 0;
}

/* one row of the window [0, win): (a, z), the kept count, and with out the kept ids; 1 for a kept cell that is no id */
static int unpack_row(const void *row, int cell_bytes, uint32_t win, const bpe_gpu_rows *d, uint32_t *a_out,
                      uint32_t *z_out, uint64_t *cnt, uint32_t *out)
{
    uint32_t a = 0, id;
    if (d->flags & BPE_ROWS_PAD)
        while (a < win && cell_id(row, cell_bytes, a, &id) && id == d->pad_id) a++;
    uint32_t z = a;
    while (z < win && !(cell_id(row, cell_bytes, z, &id) && is_stop(d, id))) z++;
    uint64_t k = 0;
    for (uint32_t c = a; c < z; c++) {
        const int ok = cell_id(row, cell_bytes, c, &id);
        if (ok && is_skipped(d, id)) continue;
        if (!ok) return 1;
        if (out) out[k] = id;
        k++;
    }
    *a_out = a;
    *z_out = z;
    *cnt = k;
    return 0;
}

int bpe_unpack_rows_host(const void *rows, int cell_bytes, size_t B, uint32_t L, size_t row_stride, const uint32_t *lens,
                         const bpe_gpu_rows *d, uint32_t *ids, size_t ids_cap, size_t *n, uint64_t *text_off,
                         uint32_t *bounds, char *msg, size_t cap)
{
    char text[200];
    int r;
    if ((r = bpe_rows_check(d, msg, cap))) return r;
    if (cell_bytes != 4 && cell_bytes != 8) {
        snprintf(text, sizeof text, "cell_bytes %d is neither 4 nor 8", cell_bytes);
        return refuse(BPE_GPU_EINVAL, msg, cap, text);
    }
    if (L > BPE_ROWS_LEN_MAX) {
        snprintf(text, sizeof text, "L %u above 2^24", (unsigned)L);
        return refuse(BPE_GPU_ERANGE, msg, cap, text);
    }
    if (row_stride < L) {
        snprintf(text, sizeof text, "row_stride %zu below L %u", row_stride, (unsigned)L);
        return refuse(BPE_GPU_EINVAL, msg, cap, text);
    }
    if (!rows && B && L) return refuse(BPE_GPU_EINVAL, msg, cap, "rows is NULL");
    if (lens)
        for (size_t k = 0; k < B; k++)
            if (lens[k] > L) {
                snprintf(text, sizeof text, "lens[%zu] is %u, above the row length %u", k, (unsigned)lens[k], (unsigned)L);
                return refuse(BPE_GPU_EINVAL, msg, cap, text);
            }
    /* first the count and the cells' check, and only then the writes */
    uint64_t total = 0, cnt;
    uint32_t a, z;
    for (size_t k = 0; k < B; k++) {
        const void *row = rows ? (const char *)rows + k * row_stride * (size_t)cell_bytes : NULL; /* (NULL: no cells) */
        if (unpack_row(row, cell_bytes, lens ? lens[k] : L, d, &a, &z, &cnt, NULL)) {
            snprintf(text, sizeof text, "row %zu keeps a cell outside 0 .. 2^32 - 1", k);
            return refuse(BPE_GPU_EDATA, msg, cap, text);
        }
        total += cnt;
    }
    if (ids && ids_cap < total) {
        snprintf(text, sizeof text, "ids_cap %zu is below the %llu kept ids", ids_cap, (unsigned long long)total);
        return refuse(BPE_GPU_EINVAL, msg, cap, text);
    }
    if (n) *n = (size_t)total;
    total = 0;
    for (size_t k = 0; k < B && (ids || text_off || bounds); k++) {
        const void *row = rows ? (const char *)rows + k * row_stride * (size_t)cell_bytes : NULL; /* (NULL: no cells) */
        (void)unpack_row(row, cell_bytes, lens ? lens[k] : L, d, &a, &z, &cnt, ids ? ids + total : NULL);
        if (text_off) text_off[k] = total;
        if (bounds) bounds[2 * k] = a, bounds[2 * k + 1] = z;
        total += cnt;
    }
    if (text_off) text_off[B] = total;
    return 0;
}

/*
 * bpe_whole.c -- whole-text rows on the host, in plain C and without a GPU
 * (bpe_ex.h; the contract: bpe_gpu.h, "Whole-text rows"): bpe_whole_check (the
 * row length and the flags of a bpe_gpu_whole; the message names the field) and
 * bpe_pack_whole_host (the texts placed in order, a cursor moving from text to
 * text, and their cells written text by text and cell by cell: the definition
 * the device is held to).  bpe_gpu_pack_whole checks with the first.
 */
#include "../../include/bpe_ex.h"

#include <stdio.h>

static int refuse(int code, char *msg, size_t cap, const char *text)
{
    if (msg && cap) snprintf(msg, cap, "whole: %s", text);
    return code;
}

int bpe_whole_check(const bpe_gpu_whole *s, char *msg, size_t cap)
{
    char text[200];
    if (msg && cap) msg[0] = '\0';
    if (!s) return refuse(BPE_GPU_EINVAL, msg, cap, "no description given");
    if (s->seq_len == 0) return refuse(BPE_GPU_EINVAL, msg, cap, "seq_len is 0");
    if (s->flags & ~(uint32_t)BPE_WHOLE_FLAGS) {
        snprintf(text, sizeof text, "flags 0x%x hold a bit that is neither BPE_WHOLE_BOS nor BPE_WHOLE_EOS",
                 (unsigned)s->flags);
        return refuse(BPE_GPU_EINVAL, msg, cap, text);
    }
    if (s->seq_len > BPE_STREAM_SEQ_MAX) {
        snprintf(text, sizeof text, "seq_len %u above 2^24", (unsigned)s->seq_len);
        return refuse(BPE_GPU_ERANGE, msg, cap, text);
    }
    return 0;
}

/* One walk of the cursor over the texts.  rows == NULL: the placement alone (text_row / text_col unless NULL, the
 * rows and the long texts counted); else the texts' cells too.  Returns R. */
static uint64_t walk(const uint32_t *ids, const uint64_t *text_off, size_t T, const bpe_gpu_whole *s, uint32_t *rows,
                     uint32_t *seg, uint32_t *pos, uint32_t *text_row, uint32_t *text_col, uint64_t *n_long)
{
    const uint64_t b = (s->flags & BPE_WHOLE_BOS) != 0, e = (s->flags & BPE_WHOLE_EOS) != 0, L = s->seq_len;
    uint64_t row = 0, col = 0, longs = 0;
    for (size_t k = 0; k < T; k++) {
        const uint64_t len = text_off[k + 1] - text_off[k], wk = b + len + e;
        if (wk > L) { /* a long text: rows of its own */
            if (col) row++, col = 0;
            longs++;
        } else if (col + wk > L) { /* does not fit any more: the next row */
            row++, col = 0;
        }
        if (text_row) text_row[k] = (uint32_t)row;
        if (text_col) text_col[k] = (uint32_t)col;
        if (rows) {
            const uint64_t start = row * L + col;
            for (uint64_t o = 0; o < wk; o++) {
                const uint64_t c = start + o, row0 = c - c % L;
                rows[c] = b && o == 0 ? s->bos_id : o - b < len ? ids[text_off[k] + o - b] : s->eos_id;
                if (seg) seg[c] = (uint32_t)k;
                if (pos) pos[c] = (uint32_t)(c - (start > row0 ? start : row0));
            }
        }
        if (wk > L) { /* behind its last row */
            row += wk / L + (wk % L != 0);
        } else {
            col += wk;
            if (col == L) row++, col = 0; /* (an exact fit: the row is full) */
        }
    }
    if (n_long) *n_long = longs;
    return row + (col != 0);
}

int bpe_pack_whole_host(const uint32_t *ids, size_t n, const uint64_t *text_off, size_t T, const bpe_gpu_whole *s,
                        uint32_t *rows, uint32_t *seg, uint32_t *pos, uint32_t *text_row, uint32_t *text_col,
                        size_t rows_cap, size_t *n_rows, uint64_t *n_cells, uint64_t *n_long)
{
    int r;
    if ((r = bpe_whole_check(s, NULL, 0))) return r;
    if (!text_off || (!ids && n) || text_off[0] != 0 || text_off[T] != n) return BPE_GPU_EINVAL;
    for (size_t k = 0; k < T; k++)
        if (text_off[k + 1] < text_off[k]) return BPE_GPU_EINVAL;
    const uint64_t w = ((s->flags & BPE_WHOLE_BOS) != 0) + ((s->flags & BPE_WHOLE_EOS) != 0);
    /* the placement first: R decides whether anything may be written */
    const uint64_t R = walk(ids, text_off, T, s, NULL, NULL, NULL, NULL, NULL, n_long);
    if (n_rows) *n_rows = (size_t)R;
    if (n_cells) *n_cells = (uint64_t)n + (uint64_t)T * w;
    if (R > 0xFFFFFFFFull) return BPE_GPU_ERANGE;
    if (!rows) return 0; /* the query */
    if (rows_cap < R) return BPE_GPU_EINVAL;
    const uint64_t cells = R * (uint64_t)s->seq_len;
    for (uint64_t c = 0; c < cells; c++) { /* every cell a pad cell, until a text takes it */
        rows[c] = s->pad_id;
        if (seg) seg[c] = BPE_STREAM_NO_TEXT;
        if (pos) pos[c] = 0;
    }
    walk(ids, text_off, T, s, rows, seg, pos, text_row, text_col, NULL);
    return 0;
}

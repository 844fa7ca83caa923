/*
 * bpe_stream.c -- packed streams on the host, in plain C and without a GPU
 * (bpe_ex.h; the contract: bpe_gpu.h, "Packed streams"): bpe_stream_check (the
 * row length and the flags of a bpe_gpu_stream; the message names the field) and
 * bpe_pack_stream_host (the texts' ids joined with their BOS / EOS and cut into
 * rows, with every cell's text and position, text by text and cell by cell: the
 * definition the device is held to).  bpe_gpu_pack_stream checks with the first.
 */
#include "../../include/bpe_ex.h"

#include <stdio.h>

static int refuse(int code, char *msg, size_t cap, const char *text)
{
    if (msg && cap) snprintf(msg, cap, "stream: %s", text);
    return code;
}

int bpe_stream_check(const bpe_gpu_stream *s, char *msg, size_t cap)
{
    char text[200];
    if (msg && cap) msg[0] = '\0';
    if (!s) return refuse(BPE_GPU_EINVAL, msg, cap, "no description given");
    if (s->seq_len == 0) return refuse(BPE_GPU_EINVAL, msg, cap, "seq_len is 0");
    if (s->flags & ~(uint32_t)BPE_STREAM_FLAGS) {
        snprintf(text, sizeof text, "flags 0x%x hold a bit that is none of BPE_STREAM_BOS, _EOS and _DROP_LAST",
                 (unsigned)s->flags);
        return refuse(BPE_GPU_EINVAL, msg, cap, text);
    }
    if (s->seq_len > BPE_STREAM_SEQ_MAX) {
        snprintf(text, sizeof text, "seq_len %u above 2^24", (unsigned)s->seq_len);
        return refuse(BPE_GPU_ERANGE, msg, cap, text);
    }
    return 0;
}

int bpe_pack_stream_host(const uint32_t *ids, size_t n, const uint64_t *text_off, size_t T, const bpe_gpu_stream *s,
                         uint32_t *rows, uint32_t *seg, uint32_t *pos, size_t rows_cap, size_t *n_rows,
                         uint64_t *n_stream)
{
    int r;
    if ((r = bpe_stream_check(s, NULL, 0))) return r;
    if (!text_off || (!ids && n) || text_off[0] != 0 || text_off[T] != n) return BPE_GPU_EINVAL;
    for (size_t k = 0; k < T; k++)
        if (text_off[k + 1] < text_off[k]) return BPE_GPU_EINVAL;
    const int b = (s->flags & BPE_STREAM_BOS) != 0, e = (s->flags & BPE_STREAM_EOS) != 0;
    const uint64_t L = s->seq_len, N = (uint64_t)n + (uint64_t)T * (uint64_t)(b + e);
    const uint64_t R = (s->flags & BPE_STREAM_DROP_LAST) ? N / L : N / L + (N % L != 0);
    if (n_rows) *n_rows = (size_t)R;
    if (n_stream) *n_stream = N;
    if (!rows) return 0; /* the query */
    if (rows_cap < R) return BPE_GPU_EINVAL;
    const uint64_t cells = R * L;
    uint64_t c = 0; /* the next cell of the stream */
    for (size_t k = 0; k < T && c < cells; k++) {
        const uint64_t start = c, len = text_off[k + 1] - text_off[k], end = start + (uint64_t)b + len + (uint64_t)e;
        for (; c < end && c < cells; c++) {
            const uint64_t o = c - start, row0 = c - c % L;
            rows[c] = b && o == 0 ? s->bos_id : o - (uint64_t)b < len ? ids[text_off[k] + o - (uint64_t)b] : s->eos_id;
            if (seg) seg[c] = (uint32_t)k;
            if (pos) pos[c] = (uint32_t)(c - (start > row0 ? start : row0));
        }
    }
    for (; c < cells; c++) { /* behind the stream: the last row's pad */
        rows[c] = s->pad_id;
        if (seg) seg[c] = BPE_STREAM_NO_TEXT;
        if (pos) pos[c] = 0;
    }
    return 0;
}

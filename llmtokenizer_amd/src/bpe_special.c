/*
 * bpe_special.c -- special tokens of bpe_ex.h on the host, in plain C and without a
 * GPU: bpe_specials_check (the limits and the overlap-free condition of bpe_gpu.h,
 * naming the pair that breaks it) and bpe_split_offsets_host_special (the split
 * with specials as it is defined there: the matches found byte by byte, every
 * segment between two matches split as a text of its own).  This is the written
 * definition bpe_gpu_split_special is held to; it shares no code and no table
 * with the device path.  The entry points that drive the engine are in
 * bpe_special_gpu.c.
 */
#include "../../include/bpe_ex.h"
#include "bpe_split_presets.h"

#include <stdio.h>
#include <string.h>

/* "<|endoftext|>" as printable text for a message (at most 24 bytes of it) */
static void show(const uint8_t *s, uint32_t len, char *out, size_t cap)
{
    size_t k = 0;
    for (uint32_t i = 0; i < len && i < 24 && k + 5 < cap; i++) {
        if (s[i] >= 0x20 && s[i] < 0x7f && s[i] != '"' && s[i] != '\\') out[k++] = (char)s[i];
        else k += (size_t)snprintf(out + k, cap - k, "\\x%02x", s[i]);
    }
    if (len > 24 && k + 4 < cap) k += (size_t)snprintf(out + k, cap - k, "...");
    out[k < cap ? k : cap - 1] = '\0';
}

static int refuse(char *msg, size_t cap, const char *why, size_t i, const uint8_t *a, uint32_t la, size_t j,
                  const uint8_t *b, uint32_t lb)
{
    char sa[128], sb[128];
    show(a, la, sa, sizeof sa);
    if (b) show(b, lb, sb, sizeof sb);
    if (msg && cap) {
        if (b) snprintf(msg, cap, "specials: %s: special %zu \"%s\" and special %zu \"%s\"", why, i, sa, j, sb);
        else snprintf(msg, cap, "specials: %s: special %zu \"%s\"", why, i, sa);
    }
    return BPE_GPU_EINVAL;
}

static int contains(const uint8_t *hay, uint32_t lh, const uint8_t *needle, uint32_t ln)
{
    for (uint32_t o = 0; o + ln <= lh; o++)
        if (!memcmp(hay + o, needle, ln)) return 1;
    return 0;
}

int bpe_specials_check(const bpe_gpu_specials *sp, char *msg, size_t msg_cap)
{
    if (msg && msg_cap) msg[0] = '\0';
    if (!sp) return 0;
    if (sp->count > BPE_GPU_SPECIAL_MAX_COUNT) {
        if (msg && msg_cap) snprintf(msg, msg_cap, "specials: %zu of them, at most %d", sp->count, BPE_GPU_SPECIAL_MAX_COUNT);
        return BPE_GPU_EINVAL;
    }
    if (sp->count && (!sp->bytes || !sp->len)) {
        if (msg && msg_cap) snprintf(msg, msg_cap, "specials: no bytes or no lengths");
        return BPE_GPU_EINVAL;
    }
    size_t off[BPE_GPU_SPECIAL_MAX_COUNT + 1];
    off[0] = 0;
    for (size_t i = 0; i < sp->count; i++) {
        if (sp->len[i] < 1 || sp->len[i] > BPE_GPU_SPECIAL_MAX_LEN) {
            if (msg && msg_cap)
                snprintf(msg, msg_cap, "specials: special %zu is %u bytes long, 1..%d are allowed", i, sp->len[i],
                         BPE_GPU_SPECIAL_MAX_LEN);
            return BPE_GPU_EINVAL;
        }
        off[i + 1] = off[i] + sp->len[i];
    }
    for (size_t i = 0; i < sp->count; i++)
        if (memchr(sp->bytes + off[i], 0, sp->len[i]))
            return refuse(msg, msg_cap, "a NUL byte", i, sp->bytes + off[i], sp->len[i], 0, NULL, 0);
    for (size_t i = 0; i < sp->count; i++) {
        const uint8_t *a = sp->bytes + off[i];
        const uint32_t la = sp->len[i];
        for (size_t j = 0; j < sp->count; j++) {
            const uint8_t *b = sp->bytes + off[j];
            const uint32_t lb = sp->len[j];
            if (i != j && contains(b, lb, a, la))
                return refuse(msg, msg_cap, la == lb ? "the same special twice" : "one is a substring of the other", i, a,
                              la, j, b, lb);
            /* a proper suffix of a (k bytes) that b begins with; k == lb would make b a substring of a */
            for (uint32_t k = 1; k < la && k < lb; k++)
                if (!memcmp(a + la - k, b, k))
                    return refuse(msg, msg_cap, "a suffix of the first is a prefix of the second", i, a, la, j, b, lb);
        }
    }
    return 0;
}

/* one segment [s, e) split as a text of its own: its starts appended at *k (written below cap) */
static int segment(int preset, const uint8_t *cls, const uint16_t *brk, const uint8_t *bytes, size_t s, size_t e,
                   uint64_t *out, size_t cap, size_t *k)
{
    if (s == e) return 0;
    if (preset < 0) {
        for (size_t i = s; i < e; i++) {
            if (i > s && !((brk[cls[bytes[i - 1]] & 15] >> (cls[bytes[i]] & 15)) & 1)) continue;
            if (out && *k < cap) out[*k] = i;
            ++*k;
        }
        return 0;
    }
    size_t cnt = 0;
    const size_t room = out && *k < cap ? cap - *k : 0;
    const int rc = bpe_split_offsets_host(preset, bytes + s, e - s, room ? out + *k : NULL, room, &cnt);
    if (rc) return rc;
    const size_t pieces = cnt - 1; /* (the entry after them, e - s, is overwritten by what follows) */
    for (size_t i = 0; i < pieces && i < room; i++) out[*k + i] += s;
    *k += pieces;
    return 0;
}

int bpe_split_offsets_host_special(int preset, const uint8_t *cls, const uint16_t *brk, const uint8_t *bytes, size_t n,
                                   const bpe_gpu_specials *sp, uint64_t *out, size_t cap, size_t *count,
                                   uint64_t *sp_piece, uint32_t *sp_index, size_t sp_cap, size_t *sp_count)
{
    if ((!bytes && n) || !count) return BPE_GPU_EINVAL;
    if (preset < 0) {
        if (!cls || !brk) return BPE_GPU_EINVAL;
        for (int b = 0; b < 256; b++)
            if (cls[b] > 15) return BPE_GPU_EINVAL;
    } else if (!split_preset_find(preset)) {
        return BPE_GPU_EINVAL;
    }
    int rc = bpe_specials_check(sp, NULL, 0);
    if (rc) return rc;
    const size_t S = sp ? sp->count : 0;
    size_t off[BPE_GPU_SPECIAL_MAX_COUNT + 1];
    off[0] = 0;
    for (size_t j = 0; j < S; j++) off[j + 1] = off[j] + sp->len[j];
    size_t k = 0, m = 0, seg = 0, i = 0;
    while (i < n) {
        size_t hit = S;
        for (size_t j = 0; j < S && hit == S; j++) /* (the set is overlap-free: at most one special matches at i) */
            if (sp->len[j] <= n - i && !memcmp(bytes + i, sp->bytes + off[j], sp->len[j])) hit = j;
        if (hit == S) {
            i++;
            continue;
        }
        if ((rc = segment(preset, cls, brk, bytes, seg, i, out, cap, &k))) return rc;
        if (sp_piece && m < sp_cap) sp_piece[m] = k;
        if (sp_index && m < sp_cap) sp_index[m] = (uint32_t)hit;
        m++;
        if (out && k < cap) out[k] = i;
        k++;
        i += sp->len[hit];
        seg = i;
    }
    if ((rc = segment(preset, cls, brk, bytes, seg, n, out, cap, &k))) return rc;
    if (out && k < cap) out[k] = n;
    *count = k + 1;
    if (sp_count) *sp_count = m;
    return 0;
}

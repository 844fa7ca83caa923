/*
 * bpe_split_preset.c -- the preset split rules of bpe_ex.h: the rules in plain C
 * (bpe_split_offsets_host: the written definition the device kernels are held
 * to, no GPU; BPE_SPLIT_CL100K among them), and bpe_encode_split_preset / bpe_train_split_preset over
 * bpe_gpu_split_preset, on the bodies bpe_encode_split and bpe_train_split run.
 */
#include "bpe_internal.h"
#include "bpe_split_presets.h"
#include "../csrc/unicode_classes.h"

enum { C_P = 0, C_L = 1, C_N = 2, C_S = 3, C_W = 4 }; /* the classes of BPE_SPLIT_WORDS and BPE_SPLIT_GPT2 */

static int class_of(uint8_t b)
{
    return (b >= 'A' && b <= 'Z') || (b >= 'a' && b <= 'z') || b >= 0x80 ? C_L
           : b >= '0' && b <= '9'                                        ? C_N
           : b == ' '                                                    ? C_S
           : b >= '\t' && b <= '\r'                                      ? C_W
                                                                         : C_P;
}

/* BPE_SPLIT_GPT2: the length (2 or 3) of a contraction piece that starts at byte j < n, or 0 */
static int clen(const uint8_t *b, size_t n, size_t j)
{
    if (b[j] != '\'' || j + 1 >= n) return 0;
    if (j) {
        const int p = class_of(b[j - 1]);
        if (p != C_L && p != C_N && p != C_W) return 0; /* a space or punctuation takes the apostrophe along */
    }
    const uint8_t x = b[j + 1];
    if (x == 's' || x == 't' || x == 'm' || x == 'd') return 2;
    if (j + 2 >= n) return 0;
    const uint8_t y = b[j + 2];
    return ((x == 'r' || x == 'v') && y == 'e') || (x == 'l' && y == 'l') ? 3 : 0;
}

/* does a piece start at byte i, 0 < i < n? */
static int starts_gpt2(const uint8_t *b, size_t n, size_t i)
{
    const int c = class_of(b[i]), p = class_of(b[i - 1]);
    const int cw = c == C_S || c == C_W, pw = p == C_S || p == C_W;
    if (cw) {
        if (!pw) return 1;
        if (i + 1 >= n) return 0; /* a run that reaches the end of the text stays whole */
        const int x = class_of(b[i + 1]);
        return x != C_S && x != C_W; /* the last white-space byte before text splits off */
    }
    if (pw) return p == C_W; /* a space belongs to what follows it */
    if (clen(b, n, i - 1) >= 2 || (i >= 2 && clen(b, n, i - 2) == 3)) return 0;
    if ((i >= 2 && clen(b, n, i - 2) == 2) || (i >= 3 && clen(b, n, i - 3) == 3)) return 1;
    return c != p;
}

/* ---- BPE_SPLIT_GPT2_UNICODE: the same rule over the characters of the text decoded as UTF-8 */

int bpe_unicode_class(uint32_t cp)
{
    if (cp == 0x20) return C_S;
    if (cp > 0x10FFFF) return C_P;
    const uint32_t t = (BPE_UC_STAGE2[16u * BPE_UC_STAGE1[cp >> 8] + ((cp >> 4) & 15u)] >> (2u * (cp & 15u))) & 3u;
    return t == 3 ? C_W : (int)t;
}

int bpe_unicode_info(const char **source, uint64_t *digest)
{
    if (source) *source = BPE_UC_SOURCE;
    if (digest) *digest = BPE_UC_DIGEST;
    return 0;
}

/* the length (1..4) of the well-formed UTF-8 sequence (Unicode Table 3-7) that b[i ..] begins inside the
 * text, *cp its code point; 0 when there is none: an overlong form, a surrogate, a value above U+10FFFF,
 * a sequence the end of the text cuts, a byte that leads nothing */
static int u8_seq(const uint8_t *b, size_t n, size_t i, uint32_t *cp)
{
    const uint32_t b0 = b[i];
    if (b0 < 0x80) {
        *cp = b0;
        return 1;
    }
    const int len = b0 >= 0xC2 && b0 <= 0xDF ? 2 : b0 >= 0xE0 && b0 <= 0xEF ? 3 : b0 >= 0xF0 && b0 <= 0xF4 ? 4 : 0;
    if (!len || n - i < (size_t)len) return 0;
    uint32_t v = b0 & (0x7Fu >> len);
    for (int k = 1; k < len; k++) {
        if ((b[i + k] & 0xC0) != 0x80) return 0;
        v = (v << 6) | (b[i + k] & 0x3Fu);
    }
    if ((len == 3 && (v < 0x800 || (v >= 0xD800 && v <= 0xDFFF))) || (len == 4 && (v < 0x10000 || v > 0x10FFFF))) return 0;
    *cp = v;
    return len;
}

/* the character byte i < n belongs to: its class, *start its first byte and *end the offset just past it.
 * A byte in no well-formed sequence is a character of its own with class P. */
static int char_at(const uint8_t *b, size_t n, size_t i, size_t *start, size_t *end)
{
    uint32_t cp = 0;
    for (size_t d = 0; d <= 3 && d <= i; d++) { /* (a lead byte never lies inside another sequence: at most one d fits) */
        const int len = u8_seq(b, n, i - d, &cp);
        if ((size_t)len > d) {
            if (start) *start = i - d;
            if (end) *end = i - d + (size_t)len;
            return bpe_unicode_class(cp);
        }
        if (d == 0 && (b[i] & 0xC0) != 0x80) break; /* no continuation byte: nothing before it holds it */
    }
    if (start) *start = i;
    if (end) *end = i + 1;
    return C_P;
}

/* clen with the class of the character before the apostrophe (the contractions themselves are ASCII) */
static int clen_u(const uint8_t *b, size_t n, size_t j)
{
    if (b[j] != '\'' || j + 1 >= n) return 0;
    if (j) {
        const int p = char_at(b, n, j - 1, NULL, NULL);
        if (p != C_L && p != C_N && p != C_W) return 0;
    }
    const uint8_t x = b[j + 1];
    if (x == 's' || x == 't' || x == 'm' || x == 'd') return 2;
    if (j + 2 >= n) return 0;
    const uint8_t y = b[j + 2];
    return ((x == 'r' || x == 'v') && y == 'e') || (x == 'l' && y == 'l') ? 3 : 0;
}

/* does a piece start at byte i, 0 < i < n? */
static int starts_gpt2u(const uint8_t *b, size_t n, size_t i)
{
    size_t st, en;
    const int c = char_at(b, n, i, &st, &en);
    if (st != i) return 0; /* a continuation byte */
    const int p = char_at(b, n, i - 1, NULL, NULL);
    const int cw = c == C_S || c == C_W, pw = p == C_S || p == C_W;
    if (cw) {
        if (!pw) return 1;
        if (en >= n) return 0;
        const int x = char_at(b, n, en, NULL, NULL); /* (the character that begins at end(i)) */
        return x != C_S && x != C_W;
    }
    if (pw) return p == C_W;
    if (clen_u(b, n, i - 1) >= 2 || (i >= 2 && clen_u(b, n, i - 2) == 3)) return 0;
    if ((i >= 2 && clen_u(b, n, i - 2) == 2) || (i >= 3 && clen_u(b, n, i - 3) == 3)) return 1;
    return c != p;
}

/* ---- BPE_SPLIT_CL100K: the rule of bpe_gpu.h, one pass from the left over the characters of the text */

enum { C_R = 5 }; /* \r and \n, split off from C_W for this rule */

/* the character that begins at byte i < n (i is no byte inside a well-formed sequence): its class with R,
 * *end the offset just past it, *fold the letter a contraction reads there (A-Z folded, U+017F an s) or 0 */
static int cl_char(const uint8_t *b, size_t n, size_t i, size_t *end, int *fold)
{
    uint32_t cp = 0;
    const int len = u8_seq(b, n, i, &cp);
    *end = i + (len ? (size_t)len : 1);
    *fold = 0;
    if (!len) return C_P; /* a byte in no well-formed sequence */
    if (cp == '\r' || cp == '\n') return C_R;
    if (cp >= 'A' && cp <= 'Z') *fold = (int)cp + ('a' - 'A');
    else if (cp >= 'a' && cp <= 'z') *fold = (int)cp;
    else if (cp == 0x17F) *fold = 's';
    return bpe_unicode_class(cp);
}

/* the characters (2 or 3) of the contraction whose apostrophe is at byte j, or 0; the class before it is the caller's */
static int cl_clen(const uint8_t *b, size_t n, size_t j)
{
    size_t e1, e2;
    int x = 0, y = 0;
    if (j + 1 >= n) return 0;
    (void)cl_char(b, n, j + 1, &e1, &x);
    if (x == 's' || x == 't' || x == 'm' || x == 'd') return 2;
    if (e1 >= n) return 0;
    (void)cl_char(b, n, e1, &e2, &y);
    return ((x == 'r' || x == 'v') && y == 'e') || (x == 'l' && y == 'l') ? 3 : 0;
}

static int is_ws(int c) { return c == C_S || c == C_W || c == C_R; }

/* the starts of text b[0 .. n) under BPE_SPLIT_CL100K, in order: out[k] written below cap, *k their number */
static void starts_cl100k(const uint8_t *b, size_t n, uint64_t *out, size_t cap, size_t *k)
{
    int p = C_R, pp = C_R;  /* the classes of the two characters before this one: before the text all reads as R */
    size_t nrun = 0;        /* numbers in the run that ends just before this character, mod 3 */
    int armed = 0;          /* every character since the last P is R (chain A) */
    int inside = 0;         /* characters of a contraction still to come */
    int after = 0;          /* the character before this one ended a contraction */
    size_t q = 0, last_r = 0; /* the white-space run this character is in ends at byte q; has_r: its last R is at byte last_r */
    int has_r = 0;
    size_t end;
    for (size_t i = 0; i < n; i = end) {
        int fold;
        const int c = cl_char(b, n, i, &end, &fold);
        int s;
        if (is_ws(c) && (i == 0 || !is_ws(p))) { /* a run begins: look ahead through it once */
            has_r = 0;
            for (q = i; q < n;) {
                size_t e;
                int f;
                const int x = cl_char(b, n, q, &e, &f);
                if (!is_ws(x)) break;
                if (x == C_R) has_r = 1, last_r = q;
                q = e;
            }
        }
        if (c == C_N) {
            s = nrun == 0; /* (0 after a character that is no number) */
        } else if (is_ws(c)) {
            if (!is_ws(p)) s = !(p == C_P && c == C_R);
            else if (c == C_R) s = 0;
            else s = (end == q && q < n) || (p == C_R && !(has_r && last_r >= i)) || (p == C_R && armed);
        } else if (c == C_L) {
            if (inside) s = 0;
            else if (after) s = 1;
            else if (p == C_L) s = 0;
            else if (p == C_N || p == C_R) s = 1;
            else if (p == C_S || p == C_W) s = 0;
            else s = pp == C_P || pp == C_S;
        } else {
            s = p == C_L || p == C_N || p == C_R || p == C_W;
        }
        if (i == 0) s = 1;
        if (s) {
            if (out && *k < cap) out[*k] = i;
            ++*k;
        }
        /* the state the next character reads */
        after = 0;
        if (inside) after = --inside == 0;
        else if (c == C_P && b[i] == '\'' && p != C_P && p != C_S) inside = cl_clen(b, n, i) ? cl_clen(b, n, i) - 1 : 0;
        nrun = c == C_N ? (nrun + 1) % 3 : 0;
        armed = c == C_P ? 1 : c == C_R ? armed : 0;
        pp = p;
        p = c;
    }
}

static int starts_words(const uint8_t *b, size_t i)
{
    const int c = class_of(b[i]), p = class_of(b[i - 1]);
    return p == C_S ? c == C_W : c != p;
}

int bpe_split_offsets_host(int preset, const uint8_t *bytes, size_t n, uint64_t *out, size_t cap, size_t *count)
{
    if ((!bytes && n) || !count) return BPE_GPU_EINVAL;
    if (!split_preset_find(preset)) return BPE_GPU_EINVAL;
    size_t k = 0;
    if (preset == BPE_SPLIT_CL100K) {
        starts_cl100k(bytes, n, out, cap, &k);
        if (out && k < cap) out[k] = n;
        *count = k + 1;
        return 0;
    }
    for (size_t i = 0; i < n; i++) {
        const int s = i == 0                     ? 1
                      : preset == BPE_SPLIT_GPT2_UNICODE ? starts_gpt2u(bytes, n, i)
                      : preset == BPE_SPLIT_GPT2 ? starts_gpt2(bytes, n, i)
                      : preset == BPE_SPLIT_WORDS ? starts_words(bytes, i)
                                                  : bytes[i - 1] == '\n';
        if (!s) continue;
        if (out && k < cap) out[k] = i;
        k++;
    }
    if (out && k < cap) out[k] = n;
    *count = k + 1;
    return 0;
}

static int split_preset(bpe_gpu_ctx *ctx, const void *rule, size_t *pieces)
{
    return bpe_gpu_split_preset(ctx, *(const int *)rule, pieces);
}

uint32_t *bpe_encode_split_preset(const uint8_t *bytes, size_t n, int preset, dyn_arr_t *pair_arr, int device,
                                  size_t *len, uint64_t **id_off, uint64_t **byte_off, size_t *ndocs)
{
    return encode_split_with(bytes, n, split_preset, &preset, pair_arr, device, len, id_off, byte_off, ndocs);
}

dyn_arr_t *bpe_train_split_preset(const uint8_t *bytes, size_t n, int preset, long max_merges, int device)
{
    return train_split_with(bytes, n, split_preset, &preset, max_merges, device);
}

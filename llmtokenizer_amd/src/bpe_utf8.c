/*
 * bpe_utf8.c -- BPE_TEXT_REPLACE and BPE_TEXT_HOLD (bpe_gpu.h, "Decoded text") in plain C: one pass from the left
 * over the rule of bpe_utf8_rule.h, text by text and byte by byte.  This is the definition the device
 * (csrc/utf8.hip) is held to.  No GPU.
 */
#include "../../include/bpe_ex.h"
#include "bpe_utf8_rule.h"

int bpe_utf8_repair_host(const uint8_t *in, size_t n, const uint64_t *byte_off, size_t T, int errors, uint8_t *out,
                         size_t cap, size_t *out_len, uint64_t *byte_off_out, uint32_t *held) {
    if ((!in && n) || !out_len || (!byte_off && T)) return BPE_GPU_EINVAL;
    if (errors != U8_RAW && errors != U8_REPLACE && errors != U8_HOLD) return BPE_GPU_EINVAL;
    if (byte_off) {
        if (byte_off[0] != 0 || byte_off[T] != n) return BPE_GPU_EINVAL;
        for (size_t k = 0; k < T; k++)
            if (byte_off[k] > byte_off[k + 1]) return BPE_GPU_EINVAL;
    }
    const size_t texts = byte_off ? T : 1;
    for (int pass = 0; pass < 2; pass++) {  /* 0: the length alone; 1: the bytes, offsets and held counts */
        size_t len = 0;
        for (size_t k = 0; k < texts; k++) {
            const uint64_t lo = byte_off ? byte_off[k] : 0, hi = byte_off ? byte_off[k + 1] : n;
            if (pass && byte_off && byte_off_out) byte_off_out[k] = len;
            if (pass && held) held[k] = errors == U8_HOLD ? u8_held(in, lo, hi) : 0;
            for (uint64_t i = lo; i < hi; i++) {
                if (errors == U8_RAW) {
                    if (pass) out[len] = in[i];
                    len++;
                } else {
                    len += u8_byte(in, i, lo, hi, errors, pass ? out + len : NULL);
                }
            }
        }
        if (pass && byte_off && byte_off_out) byte_off_out[T] = len;
        *out_len = len;
        if (!out) return 0;
        if (cap < len) return BPE_GPU_EINVAL;
    }
    return 0;
}

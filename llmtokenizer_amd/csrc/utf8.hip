// utf8.hip -- BPE_TEXT_REPLACE / BPE_TEXT_HOLD on the decoders' output while it lies in HBM (bpe_gpu.h, "Decoded
// text"); included by engine.hip after normalize.hip, whose geometry (NF_PER, NF_T, NF_TILE, NF_GRID, NF_STAGE), sink
// and block scan it shares.  What one byte becomes is src/bpe_utf8_rule.h, compiled for the device; this file is how
// the text is cut up and how the bytes move.
//
// Worth.  Every byte is worth the output bytes u8_byte gives it: 1 for ASCII, the whole sequence for the lead of a
// complete one, 3 for the lead of a cut one and for a byte in no sequence, 0 for a covered continuation byte and a
// held tail.  It depends on b[i - 3 .. i + 3] and the text's bounds, so a lane's worth is its 16 bytes' and no
// lane waits for another.  An ASCII byte is worth 1 whatever stands beside it: the fast path is the lane's own
// word test alone (no ballot over the neighbours, no edge words), and such a lane is worth 16 and copies its words.
//
// Text bounds.  Only a byte >= 0x80 asks which text it lies in, and it asks by a binary search of byte_off (u8_text;
// the next such byte of the lane asks again only past that text's end).  A mask of start bits would cost a kernel,
// n / 8 bytes to clear and a load in every lane; the search costs ASCII nothing.
//   k_u8_measure  pass 1: the worth of every lane through the block scan: cnt[t] the tile's, pre[chunk] the worth of
//                 the tile's chunks before this 16-byte chunk.
//   (rocprim::exclusive_scan over cnt: the tiles' output offsets, 64 bits: 3 n may pass 2^32)
//   k_u8_write    pass 2: the same walk from off[t] + pre[chunk] (read back, not scanned again).  A tile's output is
//                 put together in LDS at the destination's alignment (byte o of the output at index o - (off[t] & ~15))
//                 and leaves in aligned 16-byte stores, single bytes only in the two partial groups at its ends.  An
//                 ASCII lane stores its four words at the shifted index when that is a multiple of 4.  A tile worth
//                 more than NF_STAGE bytes (it more than doubled) writes single bytes to memory instead.
//   k_u8_texts    a thread per text boundary: byte_off_out[k] = off[tile] + pre[chunk] + the worth of the at most 15
//                 bytes of the chunk before the boundary; held[k] from the text's last 3 bytes.
// Every read of b lies below n but the lanes' 16-byte loads, which end below n rounded up to 16 (the decoder's
// buffer has that room); every write lies below out_n.

#define U8_FN __device__ inline
#include "../src/bpe_utf8_rule.h"

namespace bpeamd {

struct U8Args {
    const uint8_t *b;      // the decoded bytes
    uint64_t n;
    const uint64_t *boff;  // T + 1 offsets from 0 to n, not falling (nullptr: one text)
    uint64_t T;
    int errors;            // U8_REPLACE or U8_HOLD
};

// the text [*lo, *hi) that holds byte i < n: the last k with boff[k] <= i (empty texts before it end at or below i)
__device__ inline void u8_text(const U8Args &A, uint64_t i, uint64_t *lo, uint64_t *hi) {
    uint64_t a = 0, z = A.boff ? A.T : 0;  // boff[a] <= i < boff[z]
    while (z - a > 1) {
        const uint64_t mid = (a + z) >> 1;
        if (A.boff[mid] <= i) a = mid; else z = mid;
    }
    *lo = A.boff ? A.boff[a] : 0;
    *hi = A.boff ? A.boff[a + 1] : A.n;
}

// the worth of the bytes [s, e) (e <= n, at most 16 of them), each judged in its own text; WRITE: and their bytes
template <bool WRITE>
__device__ inline uint32_t u8_walk(const U8Args &A, uint64_t s, uint64_t e, NfSink &sink) {
    uint32_t len = 0;
    uint64_t lo = 0, hi = 0;  // the text of the last byte that asked (none yet)
    for (uint64_t i = s; i < e; i++) {
        uint8_t u[4];
        if (A.b[i] >= 0x80 && i >= hi) u8_text(A, i, &lo, &hi);
        const uint32_t k = u8_byte(A.b, i, lo, hi, A.errors, WRITE ? u : nullptr);
        if (WRITE)
            for (uint32_t j = 0; j < k; j++) sink.put(u[j]);
        len += k;
    }
    return len;
}

// must the lane judge its bytes one by one?  (a partial chunk does: what lies past n in q is not the text's)
__device__ inline bool u8_slow(const uint4 &q, uint32_t valid) {
    return valid < NF_PER ? valid != 0 : ((q.x | q.y | q.z | q.w) & 0x80808080u) != 0;
}

__global__ __launch_bounds__(NF_T) void k_u8_measure(const U8Args A, unsigned long long *__restrict__ cnt,
                                                     uint32_t *__restrict__ pre) {
    __shared__ uint32_t s_w[4];
    const uint64_t ntiles = (A.n + NF_TILE - 1) / NF_TILE;
    NfSink none{};
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const uint64_t s = t * NF_TILE + (uint64_t)threadIdx.x * NF_PER;
        const uint32_t valid = s < A.n ? (uint32_t)(A.n - s < NF_PER ? A.n - s : NF_PER) : 0;
        uint4 q = make_uint4(0, 0, 0, 0);
        if (valid) q = *(const uint4 *)(A.b + s);
        uint32_t len = valid;
        if (u8_slow(q, valid)) len = u8_walk<false>(A, s, s + valid, none);
        uint32_t total;
        pre[t * NF_T + threadIdx.x] = nf_block_scan(len, s_w, &total);
        if (threadIdx.x == 0) cnt[t] = total;
    }
}

__global__ __launch_bounds__(NF_T) void k_u8_write(const U8Args A, const unsigned long long *__restrict__ off,
                                                   const uint32_t *__restrict__ pre, uint8_t *__restrict__ dst,
                                                   uint64_t out_n) {
    __shared__ uint4 s_out4[(NF_STAGE + 32) / 16];
    uint8_t *s_out = (uint8_t *)s_out4;
    const uint64_t ntiles = (A.n + NF_TILE - 1) / NF_TILE;
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const uint64_t s = t * NF_TILE + (uint64_t)threadIdx.x * NF_PER;
        const uint64_t o = off[t], total = off[t + 1] - o, base = o & ~15ull;
        const uint32_t valid = s < A.n ? (uint32_t)(A.n - s < NF_PER ? A.n - s : NF_PER) : 0;
        uint4 q = make_uint4(0, 0, 0, 0);
        if (valid) q = *(const uint4 *)(A.b + s);
        const bool direct = total > NF_STAGE;  // (the same in every lane)
        NfSink sink{};
        sink.lds = direct ? nullptr : s_out;
        sink.dst = dst;
        sink.pos = o + pre[t * NF_T + threadIdx.x];
        sink.base = base;
        sink.out_n = out_n;
        sink.cap = NF_STAGE + 16;
        if (u8_slow(q, valid)) {
            (void)u8_walk<true>(A, s, s + valid, sink);
        } else if (valid) {  // 16 ASCII bytes
            const uint64_t i = sink.pos - base;
            if (!direct && (i & 3u) == 0 && i + NF_PER <= sink.cap) {
                uint32_t *p = (uint32_t *)(s_out + i);
                p[0] = q.x, p[1] = q.y, p[2] = q.z, p[3] = q.w;
            } else {
                const uint32_t wd[4] = {q.x, q.y, q.z, q.w};
                for (uint32_t k = 0; k < NF_PER; k++) sink.put((uint8_t)(wd[k >> 2] >> (8u * (k & 3u))));
            }
        }
        __syncthreads();
        if (!direct) {
            const uint64_t end = o + total;  // (<= out_n: the scan's last entry)
            for (uint64_t g = threadIdx.x; base + 16 * g < end; g += NF_T) {
                const uint64_t gp = base + 16 * g;
                if (gp >= o && gp + 16 <= end && gp + 16 <= out_n) {
                    *(uint4 *)(dst + gp) = s_out4[g];
                } else {
                    for (uint64_t p = gp > o ? gp : o; p < gp + 16 && p < end && p < out_n; p++) dst[p] = s_out[p - base];
                }
            }
        }
        __syncthreads();  // (s_out is free again)
    }
}

// Boundary k of T + 1 (one text without offsets: its held count alone).  bout and held may each be nullptr.
__global__ void k_u8_texts(const U8Args A, const unsigned long long *__restrict__ off, const uint32_t *__restrict__ pre,
                           uint64_t *__restrict__ bout, uint32_t *__restrict__ held) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (!A.boff) {
        if (k == 0 && held) held[0] = A.errors == U8_HOLD ? u8_held(A.b, 0, A.n) : 0;
        return;
    }
    if (k > A.T) return;
    const uint64_t p = A.boff[k];
    if (bout) {
        uint64_t v = off[p / NF_TILE];  // (p == n on a tile's edge: the scan's last entry, the total)
        if (p % NF_TILE) {              // (else no chunk of the tile lies before p, and pre may end before p / 16)
            NfSink none{};
            v += pre[p / NF_PER] + u8_walk<false>(A, p & ~(uint64_t)(NF_PER - 1), p, none);
        }
        bout[k] = v;
    }
    if (held && k < A.T) held[k] = A.errors == U8_HOLD ? u8_held(A.b, p, A.boff[k + 1]) : 0;
}

}  // namespace bpeamd

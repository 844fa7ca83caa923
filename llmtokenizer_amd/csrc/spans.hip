// spans.hip -- token spans (bpe_gpu.h, "Token spans"); included by engine.hip after texts.hip.
//
// bpe_gpu_token_spans: the host builds the byte length of every id (src/bpe_spans.c), then
//   k_span_chk     every resident id is compared with the table's length before it is an index (as vm_lookup
//                  does); an id at or past it, or of length 0 (a vocabulary's hole), ORs bit 0 of *err.
//   (rocprim)      start[i] = the exclusive sum of lens[ids[i]] over all resident ids, start[len] the total: a
//                  scan over a transform iterator (SpanLen, which compares again: the scan reads no bad index).
//   k_span_texts   a text batch: a thread per text, start[text_off[k]] must be boff[k] (bit 1 of *err).  With it
//                  every text's lengths sum to its bytes, so a token's end is the next token's start at a text's
//                  end too.
//   k_span_lead    char unit: over the resident bytes (a text batch's gap bytes included), 16 bytes per lane; the
//                  four lanes of a 64-byte word put their 16 bits together with two shuffles, the first writes the
//                  word's 64-bit mask of non-continuation bytes and its count.  A scan of the counts follows, and
//                  lead(p) = pref[p >> 6] + popcll(mask[p >> 6] & ((1 << (p & 63)) - 1)): two gathers per query,
//                  12 bytes of side data per 64 bytes of text.  A gap byte is 0x00 and counts; a text's spans take
//                  lead(the text's first resident position) off, which cancels the gaps before it.
//   k_spans        a thread per id: out[i] = (s, e) relative to token i's text, one 8-byte store per lane.  The
//                  text comes from text_off: one search per wave for its first id, every lane then walks forward
//                  at most SPN_WALK texts (a wave's 64 ids lie in one or two texts as a rule) and searches for
//                  itself only past that.  Without a text batch there is no search.
// bpe_gpu_pack_spans:
//   k_pack_spans   out[row][col] = a span of text `row` or (0, 0): k_pack_rows' (bx, by) shape and cut; <true>: two
//                  cells per lane and one 16-byte store, when row_len is even and out is 16-byte aligned.
// No LDS, no atomics but the error bits, no scratch.

namespace bpeamd {

constexpr uint32_t SPN_T = 256;        // threads per workgroup of k_span_chk, k_spans and k_span_lead
constexpr uint32_t SPN_GRID = 2048;    // workgroups at most of k_span_chk and k_spans (more ids: grid strides)
constexpr uint32_t SPN_LGRID = 1024;   // workgroups at most of k_span_lead
constexpr uint32_t SPN_LBYTES = 16;    // bytes a lane of k_span_lead loads per step
constexpr uint32_t SPN_WALK = 4;       // texts a lane of k_spans walks past its wave's first before it searches

__global__ __launch_bounds__(SPN_T) void k_span_chk(const uint32_t *__restrict__ ids, uint64_t len,
                                                    const uint32_t *__restrict__ lens, uint32_t n_lens,
                                                    uint32_t *__restrict__ err) {
    bool bad = false;
    for (uint64_t i = (uint64_t)blockIdx.x * SPN_T + threadIdx.x; i < len; i += (uint64_t)gridDim.x * SPN_T) {
        const uint32_t x = ids[i];
        const uint32_t l = x < n_lens ? lens[x] : 0u;
        bad |= l == 0u;
    }
    if (bad) atomicOr(err, 1u);
}

// the length of id i for the scan (0 past the ids and for an id k_span_chk reports)
struct SpanLen {
    const uint32_t *ids, *lens;
    uint64_t len;
    uint32_t n_lens;
    __host__ __device__ uint64_t operator()(uint64_t i) const {
        if (i >= len) return 0;
        const uint32_t x = ids[i];
        return x < n_lens ? lens[x] : 0;
    }
};

__global__ __launch_bounds__(SPN_T) void k_span_texts(const uint64_t *__restrict__ start, const uint64_t *__restrict__ text_off,
                                                      const uint64_t *__restrict__ boff, uint64_t T, uint64_t len,
                                                      uint32_t *__restrict__ err) {
    for (uint64_t k = (uint64_t)blockIdx.x * SPN_T + threadIdx.x; k <= T; k += (uint64_t)gridDim.x * SPN_T) {
        const uint64_t i = text_off[k];
        if (i > len || start[i] != boff[k]) atomicOr(err, 2u);  // (i is compared before it is an index)
    }
}

// bits 0..3: which of the word's four bytes are no continuation bytes ((b & 0xC0) != 0x80)
__device__ inline uint32_t span_lead4(uint32_t x) {
    const uint32_t cont = x & ~(x << 1) & 0x80808080u;          // bit 7 of a byte: set and bit 6 clear
    const uint32_t y = ((cont ^ 0x80808080u) >> 7);             // bits 0, 8, 16, 24
    return ((y * 0x00204081u) >> 21) & 0xFu;                    // (the products' bits are pairwise distinct: no carry)
}

// bytes: the resident bytes, 16-byte aligned and readable up to 64 nwords (alloc_bytes keeps 64 bytes past n0)
__global__ __launch_bounds__(SPN_T) void k_span_lead(const uint8_t *__restrict__ bytes, uint64_t nwords,
                                                     unsigned long long *__restrict__ mask, uint32_t *__restrict__ cnt) {
    const uint4 *v = (const uint4 *)bytes;
    // g: the 16-byte group; its word g >> 2 is the same for the four lanes of a quad, so they leave together
    for (uint64_t g = (uint64_t)blockIdx.x * SPN_T + threadIdx.x; (g >> 2) < nwords; g += (uint64_t)gridDim.x * SPN_T) {
        const uint4 x = v[g];
        const uint32_t m16 = span_lead4(x.x) | (span_lead4(x.y) << 4) | (span_lead4(x.z) << 8) | (span_lead4(x.w) << 12);
        uint32_t m32 = m16 << (16u * (threadIdx.x & 1u));
        m32 |= (uint32_t)__shfl_xor((int)m32, 1);
        const uint32_t other = (uint32_t)__shfl_xor((int)m32, 2);
        if ((threadIdx.x & 3u) == 0) {
            const unsigned long long m = (unsigned long long)m32 | ((unsigned long long)other << 32);
            mask[g >> 2] = m;
            cnt[g >> 2] = (uint32_t)__popcll(m);
        }
    }
}

// non-continuation bytes among the resident bytes [0, p)
__device__ inline uint32_t span_lead(const unsigned long long *__restrict__ mask, const uint32_t *__restrict__ pref, uint64_t p) {
    const unsigned long long below = (1ull << (p & 63u)) - 1ull;
    return pref[p >> 6] + (uint32_t)__popcll(mask[p >> 6] & below);
}

// text_off / boff null: one text, the resident bytes.  mask null: the byte unit.
__global__ __launch_bounds__(SPN_T) void k_spans(const uint64_t *__restrict__ start, uint64_t len,
                                                 const uint64_t *__restrict__ text_off, const uint64_t *__restrict__ boff,
                                                 uint64_t T, const unsigned long long *__restrict__ mask,
                                                 const uint32_t *__restrict__ pref, uint2 *__restrict__ out) {
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t i = (uint64_t)blockIdx.x * SPN_T + threadIdx.x; i < len; i += (uint64_t)gridDim.x * SPN_T) {
        uint64_t k = 0, tb = 0;  // the token's text and that text's first byte in the plain join
        if (text_off) {
            // the text of the wave's first id: the last k with text_off[k] <= i0 (i0 < len = text_off[T], so k < T)
            const uint64_t i0 = i - lane;
            k = sx_lower(text_off, T + 1, i0 + 1, 0) - 1;
            uint32_t steps = 0;
            while (steps < SPN_WALK && text_off[k + 1] <= i) {  // (k + 1 <= T while i < text_off[T])
                k++;
                steps++;
            }
            if (text_off[k + 1] <= i) k = sx_lower(text_off, T + 1, i + 1, 0) - 1;
            tb = boff[k];
        }
        const uint64_t bs = start[i] - tb, be = start[i + 1] - tb;
        uint2 o;
        if (mask) {
            const uint64_t r0 = tb + k;  // the text's first resident position (a gap byte after every text before it)
            const uint32_t base = span_lead(mask, pref, r0);
            const uint32_t ls = span_lead(mask, pref, r0 + bs + 1) - base;
            o.x = (ls > 1u ? ls : 1u) - 1u;
            o.y = span_lead(mask, pref, r0 + be) - base;
        } else {
            o.x = (uint32_t)bs;
            o.y = (uint32_t)be;
        }
        out[i] = o;
    }
}

template <bool VEC>
__global__ __launch_bounds__(PK_T) void k_pack_spans(const uint2 *__restrict__ spans, const uint64_t *__restrict__ text_off,
                                                     uint64_t T, uint32_t row_len, uint32_t side, uint2 *__restrict__ out) {
    constexpr uint32_t PER = VEC ? 2 : 1;
    const uint64_t col = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * PER;
    if (col >= row_len) return;  // (VEC: row_len is even, so col + 1 < row_len)
    for (uint64_t row = (uint64_t)blockIdx.y * blockDim.y + threadIdx.y; row < T; row += (uint64_t)gridDim.y * blockDim.y) {
        const uint64_t a = text_off[row], b = text_off[row + 1], len = b - a;
        const uint32_t keep = len < row_len ? (uint32_t)len : row_len;
        const uint64_t src = (side && len > row_len ? b - row_len : a) + col;
        uint2 *dst = out + row * row_len + col;
        // (the cells as scalars: a select between two uint2 objects went through scratch memory)
        uint32_t px = 0, py = 0, qx = 0, qy = 0;
        if (col < keep) {
            const uint2 p = spans[src];
            px = p.x;
            py = p.y;
        }
        if (VEC) {
            if (col + 1 < keep) {
                const uint2 q = spans[src + 1];
                qx = q.x;
                qy = q.y;
            }
            *(uint4 *)dst = make_uint4(px, py, qx, qy);
        } else {
            *dst = make_uint2(px, py);
        }
    }
}

}  // namespace bpeamd

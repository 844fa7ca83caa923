// split.hip -- pieces of the resident bytes by a two-table rule or by a preset with a marking kernel of its own; included by engine.hip; its host side is pieces.hip.
//
// A rule is cls[256] (a class 0..15 per byte value) and brk[16]: a piece
// starts at byte i > 0 when bit cls[b[i]] of brk[cls[b[i - 1]]] is set, and at
// byte 0.  The offsets are the piece starts in order followed by n: exactly
// the doc_off[] of encode_docs.hip, left in HBM for it.
//
//   k_split_table  the rule folded into a 65,536-bit start table indexed by
//                  (cur << 8) | prev: two adjacent bytes as the little-endian
//                  halfword they are in memory (8 KiB, built once per split);
//   k_split_mark   one pass over the bytes: a thread takes 16 bytes (one
//                  16-byte load), looks its 16 halfwords up in the block's
//                  LDS copy of the table and stores the 16-bit start mask and,
//                  per wave (1,024 bytes), the number of starts.  The byte
//                  before a thread's first one comes from the lane below;
//                  lane 0 of a wave loads it;
//   k_split_mark_gpt2  the same pass for BPE_SPLIT_GPT2, which no two tables
//                  express: a start is a function of b[i - 4 .. i + 1] and n,
//                  evaluated four bytes at a time with word arithmetic, no
//                  table and no LDS; writes exactly what k_split_mark writes;
//   k_split_mark_gpt2u  the same pass for BPE_SPLIT_GPT2_UNICODE: a start is a function
//                  of b[i - 7 .. i + 7] and n; a wave whose windows are all ASCII runs
//                  k_split_mark_gpt2's body, any other decodes UTF-8 and looks the
//                  classes up in the two-stage table of unicode_classes.h (12.5 KiB,
//                  read through the cache);
//   k_cl_summary, k_split_mark_cl100k  the same pass for BPE_SPLIT_CL100K, whose starts also depend on runs
//                  of any length: a summary pass, a scan of its per-wave-tile effects and the marking
//                  pass that takes their result in (described where they are, below);
//   (rocprim::exclusive_scan of the wave counts, split_run in pieces.hip)
//   k_split_emit   reads the masks again (n / 8 bytes, not the bytes): a wave
//                  ranks its starts, stages their positions in LDS and writes
//                  them as consecutive 8-byte offsets at its scanned base.
//
// No workgroup waits for another one: the order comes from the scan between
// the two launches.

#define BPE_UC_STORAGE __device__ const
#include "unicode_classes.h"  // BPE_UC_STAGE1 / BPE_UC_STAGE2 in device memory

namespace bpeamd {

constexpr uint32_t SP_T = 256;            // threads per workgroup
constexpr uint32_t SP_PER = 16;           // bytes per thread and step
constexpr uint32_t SP_TILE = SP_T * SP_PER;  // bytes per workgroup and step (BPE_GPU_SPLIT_TILE)
constexpr uint32_t SP_WTILE = 64 * SP_PER;   // bytes per wave and step: the unit of the counts
constexpr uint32_t SP_GRID = 2048;        // workgroups at most (BPE_GPU_SPLIT_GRID); the tiles beyond are strided
constexpr uint32_t SP_TBL = 65536 / 32;   // words of the start table
static_assert(SP_TILE == BPE_GPU_SPLIT_TILE && SP_GRID == BPE_GPU_SPLIT_GRID, "bpe_gpu.h names the split's geometry");

struct SplitRule {
    uint8_t cls[256];
    uint16_t brk[16];
};

// word j of the table: cur = j >> 3, prev = 32 * (j & 7) + bit
__global__ __launch_bounds__(SP_T) void k_split_table(const SplitRule R, uint32_t *__restrict__ tbl) {
    const uint32_t j = blockIdx.x * SP_T + threadIdx.x;
    if (j >= SP_TBL) return;
    const uint32_t c = R.cls[j >> 3] & 15u;
    uint32_t w = 0;
    for (uint32_t k = 0; k < 32; k++) w |= (((uint32_t)R.brk[R.cls[32 * (j & 7) + k] & 15u] >> c) & 1u) << k;
    tbl[j] = w;
}

// the table's bit for the halfword in idx's low 16 bits (the bits above are ignored)
__device__ inline uint32_t sp_bit(const uint32_t *tbl, uint32_t idx) {
    const uint32_t w = *(const uint32_t *)((const char *)tbl + ((idx >> 3) & 0x1FFCu));  // tbl[idx >> 5]
    return __builtin_amdgcn_ubfe(w, idx & 31u, 1u);
}

// mask[t]: bit k = a piece starts at byte 16 t + k; wcnt[v]: starts in bytes [1024 v, 1024 v + 1024).
// Both arrays cover whole tiles (ntiles * SP_T masks, ntiles * SP_T / 64 counts): 0 past n.
__global__ __launch_bounds__(SP_T) void k_split_mark(const uint8_t *__restrict__ bytes, uint64_t n,
                                                     const uint32_t *__restrict__ tbl_g, uint64_t ntiles,
                                                     uint16_t *__restrict__ mask, uint32_t *__restrict__ wcnt) {
    __shared__ __align__(16) uint32_t tbl[SP_TBL];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    for (uint32_t k = tid; k < SP_TBL / 4; k += SP_T) ((uint4 *)tbl)[k] = ((const uint4 *)tbl_g)[k];
    __syncthreads();
    // (the buffer has 64 bytes of zeroed slack past n: a load that begins below n stays inside it)
    auto load16 = [&](uint64_t tile) {
        const uint64_t o = (tile * SP_T + tid) * SP_PER;
        return tile < ntiles && o < n ? *(const uint4 *)(bytes + o) : make_uint4(0, 0, 0, 0);
    };
    uint4 q = load16(blockIdx.x);
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t t = tile * SP_T + tid, o = t * SP_PER;
        const uint4 qn = load16(tile + gridDim.x);  // the next step's bytes are on their way during this one's lookups
        uint32_t pw = __shfl_up(q.w, 1);  // the word that ends with the byte before this thread's first
        if (lane == 0) pw = o && o < n ? (uint32_t)bytes[o - 1] << 24 : 0u;
        const uint32_t x[4] = {q.x, q.y, q.z, q.w};
        uint32_t m = 0;
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) {
            m |= sp_bit(tbl, __builtin_amdgcn_alignbit(x[j], pw, 24)) << (4 * j);
            m |= sp_bit(tbl, x[j]) << (4 * j + 1);
            m |= sp_bit(tbl, x[j] >> 8) << (4 * j + 2);
            m |= sp_bit(tbl, x[j] >> 16) << (4 * j + 3);
            pw = x[j];
        }
        if (o == 0) m |= 1u;  // byte 0 starts a piece
        m = o >= n ? 0u : n - o >= SP_PER ? m : m & ((1u << (uint32_t)(n - o)) - 1u);
        mask[t] = (uint16_t)m;
        uint32_t c = (uint32_t)__builtin_popcount(m);
        for (int d = 32; d; d >>= 1) c += __shfl_xor(c, d);
        if (lane == 0) wcnt[t >> 6] = c;
        q = qn;
    }
}

// ---- BPE_SPLIT_GPT2 (bpe_gpu.h): the starts as a function of b[i - 4 .. i + 1] and n, no table.
//
// A thread's 21-byte window is six words: w[0] = b[o - 4 .. o - 1], w[1..4] its 16 bytes, byte 0 of
// w[5] = b[o + 16].  Every predicate of the rule is kept as one flag per byte in bit 7 of that byte
// (the bits below are junk and stay below: only bitwise operations and shifts by whole bytes follow),
// so four bytes are classified per instruction and "the flag of the byte k before / after" is one
// v_alignbit across two words.  Bytes at and past n read as spaces: white space that is no text for
// the look-ahead, and no contraction letter.  The bytes before byte 0 read as newlines: class W, after
// which a contraction may start.

// bit 7 of every byte of x whose low seven bits are >= c (1 <= c <= 0x80; the bytes of x are <= 0x7f)
__device__ inline uint32_t sg_ge(uint32_t x, uint32_t c) { return x + (0x80u - c) * 0x01010101u; }
// bit 7 of every byte of x in [lo, hi]
__device__ inline uint32_t sg_in(uint32_t x, uint32_t lo, uint32_t hi) { return sg_ge(x, lo) ^ sg_ge(x, hi + 1u); }
// flags moved up by k bytes (byte i gets the flag of byte i - k) and down by k: `lo` / `hi` are the neighbouring words
__device__ inline uint32_t sg_up(uint32_t w, uint32_t lo, uint32_t k) { return __builtin_amdgcn_alignbit(w, lo, 32u - 8u * k); }
__device__ inline uint32_t sg_dn(uint32_t w, uint32_t hi, uint32_t k) { return __builtin_amdgcn_alignbit(hi, w, 8u * k); }

// a thread's 16 bytes of a tile with every byte at or past n replaced by a space (all spaces past the tiles)
// (the buffer has 64 bytes of slack past n: a load that begins below n stays inside it)
__device__ inline uint4 sg_load16(const uint8_t *__restrict__ bytes, uint64_t n, uint64_t ntiles, uint64_t tile) {
    constexpr uint32_t SPACES = 0x20202020u;
    const uint64_t o = (tile * SP_T + threadIdx.x) * SP_PER;
    if (tile >= ntiles || o >= n) return make_uint4(SPACES, SPACES, SPACES, SPACES);
    uint4 v = *(const uint4 *)(bytes + o);
    if (n - o < SP_PER) {  // the text ends inside these 16 bytes
        const uint32_t r = (uint32_t)(n - o);
        uint32_t x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) {
            const uint32_t keep = r <= 4 * j ? 0u : r - 4 * j >= 4 ? ~0u : (1u << (8 * (r - 4 * j))) - 1u;
            x[j] = (x[j] & keep) | (SPACES & ~keep);
        }
        v = make_uint4(x[0], x[1], x[2], x[3]);
    }
    return v;
}

// the 16 start bits of a thread's bytes from its six words (before byte 0 and the end of the text are applied)
__device__ inline uint32_t sg_mark16(const uint32_t *w) {
    constexpr uint32_t SPACES = 0x20202020u, B7 = 0x80808080u;
    {
        // per word: L letters, N digits, ws white space, S the space, ap the apostrophe; m1 one of s t m d,
        // rv one of r v, e, l (the letters of the contractions)
        uint32_t L[6], N[6], ws[6], S[6], ap[6], m1[6], rv[6], e[6], l[6];
#pragma unroll
        for (uint32_t j = 0; j < 6; j++) {
            const uint32_t hi = w[j] & B7;
            const uint32_t x = (w[j] & ~B7) | (hi - (hi >> 7));  // a byte >= 0x80 becomes 0x7f: in none of the ranges below
            S[j] = sg_in(x, ' ', ' ');
            ws[j] = S[j] | sg_in(x, '\t', '\r');
            L[j] = w[j] | sg_in(x | SPACES, 'a', 'z');  // (x | 0x20 folds A-Z onto a-z and nothing else into it)
            N[j] = sg_in(x, '0', '9');
            ap[j] = sg_in(x, '\'', '\'');
            m1[j] = sg_in(x, 'd', 'd') | sg_in(x, 'm', 'm') | sg_in(x, 's', 't');
            rv[j] = sg_in(x, 'r', 'r') | sg_in(x, 'v', 'v');
            e[j] = sg_in(x, 'e', 'e');
            l[j] = sg_in(x, 'l', 'l');
        }
        // c2 / c3: a contraction of 2 / 3 bytes starts here (words 0..4; byte 0 of word 0 is not used)
        uint32_t c2[5], c3[5];
#pragma unroll
        for (uint32_t j = 0; j < 5; j++) {
            const uint32_t ok = L[j] | N[j] | (ws[j] & ~S[j]);  // after this byte a contraction may start
            const uint32_t okp = j ? L[j - 1] | N[j - 1] | (ws[j - 1] & ~S[j - 1]) : 0u;
            const uint32_t a = ap[j] & sg_up(ok, okp, 1);
            c2[j] = a & sg_dn(m1[j], m1[j + 1], 1);
            c3[j] = a & ((sg_dn(rv[j], rv[j + 1], 1) & sg_dn(e[j], e[j + 1], 2)) |
                         (sg_dn(l[j], l[j + 1], 1) & sg_dn(l[j], l[j + 1], 2)));
        }
        uint32_t m = 0;
#pragma unroll
        for (uint32_t j = 1; j < 5; j++) {
            const uint32_t ws1 = sg_up(ws[j], ws[j - 1], 1), S1 = sg_up(S[j], S[j - 1], 1);
            const uint32_t wsn = sg_dn(ws[j], ws[j + 1], 1);
            const uint32_t diff = (L[j] ^ sg_up(L[j], L[j - 1], 1)) | (N[j] ^ sg_up(N[j], N[j - 1], 1));
            const uint32_t inside = sg_up(c2[j] | c3[j], c2[j - 1] | c3[j - 1], 1) | sg_up(c3[j], c3[j - 1], 2);
            const uint32_t after = sg_up(c2[j], c2[j - 1], 2) | sg_up(c3[j], c3[j - 1], 3);
            const uint32_t text = (ws1 & ~S1) | ((after | diff) & ~(ws1 | inside));  // b[i] is not white space
            const uint32_t st = ((ws[j] & ~(ws1 & wsn)) | (~ws[j] & text)) & B7;
            // bits 7, 15, 23, 31 -> 0, 1, 2, 3
            m |= (((st >> 7) | (st >> 14) | (st >> 21) | (st >> 28)) & 15u) << (4 * (j - 1));
        }
        return m;
    }
}

// what k_split_mark writes (the same tiles, grid striding, masks and counts), for the rule above
__global__ __launch_bounds__(SP_T) void k_split_mark_gpt2(const uint8_t *__restrict__ bytes, uint64_t n, uint64_t ntiles,
                                                          uint16_t *__restrict__ mask, uint32_t *__restrict__ wcnt) {
    constexpr uint32_t SPACES = 0x20202020u;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    uint4 q = sg_load16(bytes, n, ntiles, blockIdx.x);
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t t = tile * SP_T + tid, o = t * SP_PER;
        const uint4 qn = sg_load16(bytes, n, ntiles, tile + gridDim.x);
        uint32_t w[6] = {__shfl_up(q.w, 1), q.x, q.y, q.z, q.w, __shfl_down(q.x, 1)};
        if (lane == 0) w[0] = o && o < n ? *(const uint32_t *)(bytes + o - 4) : 0x0A0A0A0Au;  // (o is a multiple of 16)
        if (lane == 63) w[5] = o + SP_PER < n ? (uint32_t)bytes[o + SP_PER] : SPACES;
        uint32_t m = sg_mark16(w);
        if (o == 0) m |= 1u;  // byte 0 starts a piece
        m = o >= n ? 0u : n - o >= SP_PER ? m : m & ((1u << (uint32_t)(n - o)) - 1u);
        mask[t] = (uint16_t)m;
        uint32_t c = (uint32_t)__builtin_popcount(m);
        for (int d = 32; d; d >>= 1) c += __shfl_xor(c, d);
        if (lane == 0) wcnt[t >> 6] = c;
        q = qn;
    }
}

// ---- BPE_SPLIT_GPT2_UNICODE (bpe_gpu.h): the same rule over the characters of the text decoded as UTF-8; a start
// is a function of b[i - 7 .. i + 7] and n.
//
// A thread's window is eight words, w[0..7] = b[o - 8 .. o + 23]: window byte q is b[o - 8 + q].  Here every
// predicate is one 32-bit mask over the window, bit q for byte q, so "the byte k before / after" is a shift and
// the rule is evaluated for all of a thread's bytes (q = 8 .. 23) at once.  The ASCII predicates are classified
// four bytes at a time as above and gathered into the masks.  Every window byte 1 .. 27 is then decoded as the
// lead of a UTF-8 sequence from the four bytes that begin there (well-formedness at q is a function of those
// alone): a well-formed lead gives its class, looked up in the two-stage table of unicode_classes.h, to all
// bytes of its sequence and marks the others as continuation bytes; a byte >= 0x80 in no sequence stays in no
// mask: class P.  A sequence that begins at q = 0 is not seen, which misreads q <= 3 at most, and bit q of the
// result reads class bits from q - 4 on.  No branch and no loop depends on the text: a byte that leads
// nothing looks up code point 0.

// bits 7, 15, 23, 31 of x -> bits 0..3
__device__ inline uint32_t su_nib(uint32_t x) {
    x &= 0x80808080u;
    return ((x >> 7) | (x >> 14) | (x >> 21) | (x >> 28)) & 15u;
}

// bit q: a piece starts at window byte q (valid for q = 8 .. 23; byte 0 of the text and its end are the caller's)
__device__ inline uint32_t su_starts(const uint32_t *w) {
    constexpr uint32_t SPACES = 0x20202020u, B7 = 0x80808080u;
    // L letters, N numbers, ws white space, S the space, ap the apostrophe; m1 one of s t m d, rv one of r v, e, l
    uint32_t L = 0, N = 0, ws = 0, S = 0, ap = 0, m1 = 0, rv = 0, e = 0, l = 0;
#pragma unroll
    for (uint32_t j = 0; j < 8; j++) {
        const uint32_t hi = w[j] & B7;
        const uint32_t x = (w[j] & ~B7) | (hi - (hi >> 7));  // a byte >= 0x80 becomes 0x7f: in none of the ranges below
        const uint32_t s = sg_in(x, ' ', ' ');
        S |= su_nib(s) << (4 * j);
        ws |= su_nib(s | sg_in(x, '\t', '\r')) << (4 * j);
        L |= su_nib(sg_in(x | SPACES, 'a', 'z')) << (4 * j);
        N |= su_nib(sg_in(x, '0', '9')) << (4 * j);
        ap |= su_nib(sg_in(x, '\'', '\'')) << (4 * j);
        m1 |= su_nib(sg_in(x, 'd', 'd') | sg_in(x, 'm', 'm') | sg_in(x, 's', 't')) << (4 * j);
        rv |= su_nib(sg_in(x, 'r', 'r') | sg_in(x, 'v', 'v')) << (4 * j);
        e |= su_nib(sg_in(x, 'e', 'e')) << (4 * j);
        l |= su_nib(sg_in(x, 'l', 'l')) << (4 * j);
    }
    // cont: continuation bytes of well-formed sequences; w2 / w3: leads of white space of two / three bytes
    uint32_t cont = 0, w2 = 0, w3 = 0;
#pragma unroll
    for (uint32_t q = 1; q <= 27; q++) {
        const uint32_t v = q & 3u ? __builtin_amdgcn_alignbit(w[(q >> 2) + 1], w[q >> 2], 8u * (q & 3u)) : w[q >> 2];
        const uint32_t b0 = v & 0xFFu, b1 = (v >> 8) & 0x3Fu, b2 = (v >> 16) & 0x3Fu, b3 = (v >> 24) & 0x3Fu;
        const uint32_t cp2 = ((b0 & 0x1Fu) << 6) | b1, cp3 = ((b0 & 0x0Fu) << 12) | (b1 << 6) | b2;
        const uint32_t cp4 = ((b0 & 0x07u) << 18) | (b1 << 12) | (b2 << 6) | b3;
        // Unicode Table 3-7: E0 A0..BF is cp3 >= 0x800, ED 80..9F is no surrogate, F0 90..BF is cp4 >= 0x10000,
        // F4 80..8F and no lead above F4 is cp4 <= 0x10FFFF
        const bool ok2 = b0 >= 0xC2u && b0 <= 0xDFu && (v & 0xC000u) == 0x8000u;
        const bool ok3 = (b0 & 0xF0u) == 0xE0u && (v & 0xC0C000u) == 0x808000u && cp3 >= 0x800u && (cp3 & 0xF800u) != 0xD800u;
        const bool ok4 = (b0 & 0xF8u) == 0xF0u && (v & 0xC0C0C000u) == 0x80808000u && cp4 >= 0x10000u && cp4 <= 0x10FFFFu;
        const uint32_t len = ok2 ? 2u : ok3 ? 3u : ok4 ? 4u : 0u;
        const uint32_t cp = ok2 ? cp2 : ok3 ? cp3 : ok4 ? cp4 : 0u;
        const uint32_t t = (BPE_UC_STAGE2[16u * BPE_UC_STAGE1[cp >> 8] + ((cp >> 4) & 15u)] >> (2u * (cp & 15u))) & 3u;
        const uint32_t rng = ((1u << len) - 1u) << q;  // the bytes of the sequence (none when nothing is led here)
        L |= t == 1u ? rng : 0u;
        N |= t == 2u ? rng : 0u;
        ws |= t == 3u ? rng : 0u;
        cont |= rng & (rng - 1u);
        w2 |= t == 3u && len == 2u ? 1u << q : 0u;
        w3 |= t == 3u && len == 3u ? 1u << q : 0u;
        if (q % 9u == 0u) __builtin_amdgcn_sched_barrier(0);  // nine lookups in flight at a time: the registers of 27 are not there
    }
    const uint32_t ws1 = ws << 1, S1 = S << 1;
    // the class at end(i) is white space (no white space has four bytes)
    const uint32_t wsn = ((ws >> 1) & ~(w2 | w3)) | ((ws >> 2) & w2) | ((ws >> 3) & w3);
    const uint32_t a = ap & ((L | N | (ws & ~S)) << 1);  // an apostrophe a contraction may start at
    const uint32_t c2 = a & (m1 >> 1), c3 = a & (((rv >> 1) & (e >> 2)) | ((l >> 1) & (l >> 2)));
    const uint32_t inside = ((c2 | c3) << 1) | (c3 << 2), after = (c2 << 2) | (c3 << 3);
    const uint32_t diff = (L ^ (L << 1)) | (N ^ (N << 1));
    const uint32_t text = (ws1 & ~S1) | ((after | diff) & ~(ws1 | inside));  // b[i] is not white space
    return ((ws & ~(ws1 & wsn)) | (~ws & text)) & ~cont;
}

// what k_split_mark writes, for BPE_SPLIT_GPT2_UNICODE.  The two words before a thread's 16 bytes come from the
// lane below and the two after them from the lane above; lanes 0 and 63 load theirs, only below n.  Bytes at and
// past n read as spaces and the bytes before byte 0 as newlines before anything is decoded, so a sequence the
// end cuts is ill-formed.  A wave none of whose windows holds a byte >= 0x80 runs k_split_mark_gpt2's body.
__global__ __launch_bounds__(SP_T) void k_split_mark_gpt2u(const uint8_t *__restrict__ bytes, uint64_t n, uint64_t ntiles,
                                                           uint16_t *__restrict__ mask, uint32_t *__restrict__ wcnt) {
    constexpr uint32_t SPACES = 0x20202020u, B7 = 0x80808080u;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    uint4 q = sg_load16(bytes, n, ntiles, blockIdx.x);
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t t = tile * SP_T + tid, o = t * SP_PER;
        const uint4 qn = sg_load16(bytes, n, ntiles, tile + gridDim.x);
        uint32_t w[8] = {__shfl_up(q.z, 1), __shfl_up(q.w, 1), q.x, q.y, q.z, q.w, __shfl_down(q.x, 1), __shfl_down(q.y, 1)};
        if (lane == 0) {  // (o is a multiple of 16: b[o - 8 .. o - 1] lie below n when o does)
            const uint2 v = o && o < n ? *(const uint2 *)(bytes + o - 8) : make_uint2(0x0A0A0A0Au, 0x0A0A0A0Au);
            w[0] = v.x;
            w[1] = v.y;
        }
        if (lane == 63) {
            uint2 v = make_uint2(SPACES, SPACES);
            if (o + SP_PER < n) {  // (a load that begins below n stays inside the slack)
                v = *(const uint2 *)(bytes + o + SP_PER);
                const uint64_t r = n - (o + SP_PER);  // bytes of text in it
                if (r < 8) {
                    const uint32_t r4 = (uint32_t)r & 3u, keep = (1u << (8u * r4)) - 1u;  // (r4 == 0: keep nothing)
                    if (r < 4) v = make_uint2((v.x & keep) | (SPACES & ~keep), SPACES);
                    else v.y = (v.y & keep) | (SPACES & ~keep);
                }
            }
            w[6] = v.x;
            w[7] = v.y;
        }
        const bool high = ((w[0] | w[1] | w[2] | w[3] | w[4] | w[5] | w[6] | w[7]) & B7) != 0u;
        uint32_t m;
        if (__ballot(high) == 0ull) m = sg_mark16(w + 1);  // (what lies past byte 0 of its last word decides none of these 16 bits)
        else m = (su_starts(w) >> 8) & 0xFFFFu;
        if (o == 0) m |= 1u;  // byte 0 starts a piece
        m = o >= n ? 0u : n - o >= SP_PER ? m : m & ((1u << (uint32_t)(n - o)) - 1u);
        mask[t] = (uint16_t)m;
        uint32_t c = (uint32_t)__builtin_popcount(m);
        for (int d = 32; d; d >>= 1) c += __shfl_xor(c, d);
        if (lane == 0) wcnt[t >> 6] = c;
        q = qn;
    }
}

// ---- BPE_SPLIT_CL100K (bpe_gpu.h): the cl100k / Llama-3 pattern over the characters of the text decoded as
// UTF-8.  All of the rule but three conditions is a function of b[i - 8 .. i + 7] and n and is evaluated over the
// window of k_split_mark_gpt2u, one 32-bit mask per predicate.  The three are chains through runs of any length:
//   N  a number starts a piece when the numbers of its run before it are a multiple of 3;
//   A  white space after a run of R starts a piece when that run began right after a P;
//   B  white space after an R starts a piece when no R follows in its white-space run (this one reads ahead).
// Each is a scan of the characters with a state of two or three values, and what a stretch of text does to the
// state is either "decides it" (the stretch holds a character that resets the chain; then the value after it) or
// "passes it on" (plus, for N, a count mod 3).  Such effects compose associatively, so:
//   k_cl_summary        one pass over the bytes: the effect of every wave tile (1,024 bytes) on N and A read from
//                       the left, and on B read from the right (stored in reverse order);
//   (rocprim::exclusive_scan of both arrays with ClCompose: the state on entry to every wave tile)
//   k_split_mark_cl100k the marking pass: the same effects per thread, a scan of them across the wave's lanes from
//                       the tile's entry state, 16 steps over the thread's own characters, and the rule.
// A character belongs to the thread that holds its lead byte; continuation bytes pass every chain on.  No loop's
// trip count depends on the text and no workgroup waits for another one.
//
// With specials the bytes of the matches (the cover bitmap of special.hip, found before this pass) read as
// newlines before anything is decoded, and a match byte decides every chain to its reset value: a segment
// begins after it and ends before it.  k_sp_patch then sets the matches' own bits.

// an effect: bits 0-1 the N count mod 3, bit 2 N decided, bit 3 the A (or B) value, bit 4 A (or B) decided
constexpr uint32_t CL_NK = 3u, CL_ND = 4u, CL_AV = 8u, CL_AD = 16u;
constexpr uint32_t CL_RESET = CL_ND | CL_AD;  // both chains decided to 0: the ends of the text

// the effect of a stretch followed by the effect b of the next one (for B: the stretch to the right first)
struct ClCompose {
    __host__ __device__ inline uint32_t operator()(uint32_t a, uint32_t b) const {
        const uint32_t nk = (b & CL_ND) ? (b & (CL_NK | CL_ND)) : ((a & CL_ND) | (((a & CL_NK) + (b & CL_NK)) % 3u));
        const uint32_t av = (b & CL_AD) ? (b & (CL_AV | CL_AD)) : (a & (CL_AV | CL_AD));
        return nk | av;
    }
};

// the predicates of a thread's window as masks (bit q for window byte q, b[o - 8 + q]); every byte of a
// well-formed sequence carries its character's class, a byte in no sequence is in no class mask: P
struct ClMasks {
    uint32_t R, S, ws, L, N, cont;  // \r \n; the space; White_Space; letters; numbers; continuation bytes
    uint32_t w2, w3;                // leads of white space of two / three bytes
    uint32_t ap, m1, rv, e, l, ls;  // the apostrophe; s t m d; r v; e; l (A-Z folded); the lead of U+017F
};

// w[0..7] = b[o - 8 .. o + 23] after the substitutions (past n, before 0, match bytes); decode: some byte is >= 0x80.
// OWN: only the bits of the thread's own bytes (8 .. 23) are asked for (the effects on the chains): words 2 .. 5
// and the sequences that reach into them.  Otherwise an all-ASCII window needs words 1 .. 6 (the rule reads
// b[i - 4 .. i + 2] then), a window with sequences all eight.
template <bool OWN>
__device__ inline void cl_classify(const uint32_t *w, bool decode, ClMasks &m) {
    constexpr uint32_t SPACES = 0x20202020u, B7 = 0x80808080u;
    m = ClMasks{};
#pragma unroll
    for (uint32_t jj = 0; jj < 8; jj++) {
        const uint32_t j = jj < 6 ? jj + 1 : jj == 6 ? 0 : 7;  // words 1 .. 6, then 0 and 7
        if (OWN && (j < 2 || j > 5)) continue;
        if (!OWN && jj >= 6 && !decode) continue;  // (wave-uniform)
        const uint32_t hi = w[j] & B7;
        const uint32_t x = (w[j] & ~B7) | (hi - (hi >> 7));  // a byte >= 0x80 becomes 0x7f: in none of the ranges below
        const uint32_t f = x | SPACES;                       // A-Z onto a-z and nothing else into it
        const uint32_t s = sg_in(x, ' ', ' '), r = sg_in(x, '\n', '\n') | sg_in(x, '\r', '\r');
        m.S |= su_nib(s) << (4 * j);
        m.R |= su_nib(r) << (4 * j);
        m.ws |= su_nib(s | sg_in(x, '\t', '\r')) << (4 * j);
        m.L |= su_nib(sg_in(f, 'a', 'z')) << (4 * j);
        m.N |= su_nib(sg_in(x, '0', '9')) << (4 * j);
        m.ap |= su_nib(sg_in(x, '\'', '\'')) << (4 * j);
        m.m1 |= su_nib(sg_in(f, 'd', 'd') | sg_in(f, 'm', 'm') | sg_in(f, 's', 't')) << (4 * j);
        m.rv |= su_nib(sg_in(f, 'r', 'r') | sg_in(f, 'v', 'v')) << (4 * j);
        m.e |= su_nib(sg_in(f, 'e', 'e')) << (4 * j);
        m.l |= su_nib(sg_in(f, 'l', 'l')) << (4 * j);
    }
    if (!decode) return;  // (wave-uniform)
    // every window byte 0 .. 27 as the lead of a sequence, as su_starts does; byte 0 too: the class of the
    // character before the one before i is read, eight bytes back at most
#pragma unroll
    for (uint32_t q = OWN ? 5 : 0; q <= (OWN ? 23 : 27); q++) {
        const uint32_t v = q & 3u ? __builtin_amdgcn_alignbit(w[(q >> 2) + 1], w[q >> 2], 8u * (q & 3u)) : w[q >> 2];
        const uint32_t b0 = v & 0xFFu, b1 = (v >> 8) & 0x3Fu, b2 = (v >> 16) & 0x3Fu, b3 = (v >> 24) & 0x3Fu;
        const uint32_t cp2 = ((b0 & 0x1Fu) << 6) | b1, cp3 = ((b0 & 0x0Fu) << 12) | (b1 << 6) | b2;
        const uint32_t cp4 = ((b0 & 0x07u) << 18) | (b1 << 12) | (b2 << 6) | b3;
        const bool ok2 = b0 >= 0xC2u && b0 <= 0xDFu && (v & 0xC000u) == 0x8000u;
        const bool ok3 = (b0 & 0xF0u) == 0xE0u && (v & 0xC0C000u) == 0x808000u && cp3 >= 0x800u && (cp3 & 0xF800u) != 0xD800u;
        const bool ok4 = (b0 & 0xF8u) == 0xF0u && (v & 0xC0C0C000u) == 0x80808000u && cp4 >= 0x10000u && cp4 <= 0x10FFFFu;
        const uint32_t len = ok2 ? 2u : ok3 ? 3u : ok4 ? 4u : 0u;
        const uint32_t cp = ok2 ? cp2 : ok3 ? cp3 : ok4 ? cp4 : 0u;
        const uint32_t t = (BPE_UC_STAGE2[16u * BPE_UC_STAGE1[cp >> 8] + ((cp >> 4) & 15u)] >> (2u * (cp & 15u))) & 3u;
        const uint32_t rng = ((1u << len) - 1u) << q;  // the bytes of the sequence (none when nothing is led here)
        m.L |= t == 1u ? rng : 0u;
        m.N |= t == 2u ? rng : 0u;
        m.ws |= t == 3u ? rng : 0u;
        m.cont |= rng & (rng - 1u);
        m.w2 |= t == 3u && len == 2u ? 1u << q : 0u;
        m.w3 |= t == 3u && len == 3u ? 1u << q : 0u;
        m.ls |= ok2 && cp2 == 0x17Fu ? 1u << q : 0u;
        if (q % 9u == 8u) __builtin_amdgcn_sched_barrier(0);  // nine lookups in flight at a time
    }
}

// a thread's window and the cover bits of its bytes: w as k_split_mark_gpt2u builds it (the two words before a
// thread's 16 bytes from the lane below, the two after from the lane above; lanes 0 and 63 load theirs, only
// below n; past n spaces, before byte 0 newlines), then every match byte a newline.  cv: bit q = window byte q
// is a match byte (0 without a bitmap).  cover holds 128 words per tile.
__device__ inline void cl_window(const uint8_t *__restrict__ bytes, uint64_t n, uint64_t ntiles, const uint32_t *__restrict__ cover,
                                 const uint4 q, uint64_t o, uint32_t lane, uint32_t *w, uint32_t &cv) {
    constexpr uint32_t SPACES = 0x20202020u;
    w[0] = __shfl_up(q.z, 1), w[1] = __shfl_up(q.w, 1), w[2] = q.x, w[3] = q.y, w[4] = q.z, w[5] = q.w;
    w[6] = __shfl_down(q.x, 1), w[7] = __shfl_down(q.y, 1);
    if (lane == 0) {  // (o is a multiple of 16: b[o - 8 .. o - 1] lie below n when o does)
        const uint2 v = o && o < n ? *(const uint2 *)(bytes + o - 8) : make_uint2(0x0A0A0A0Au, 0x0A0A0A0Au);
        w[0] = v.x;
        w[1] = v.y;
    }
    if (lane == 63) {
        uint2 v = make_uint2(SPACES, SPACES);
        if (o + SP_PER < n) {  // (a load that begins below n stays inside the slack)
            v = *(const uint2 *)(bytes + o + SP_PER);
            const uint64_t r = n - (o + SP_PER);  // bytes of text in it
            if (r < 8) {
                const uint32_t r4 = (uint32_t)r & 3u, keep = (1u << (8u * r4)) - 1u;  // (r4 == 0: keep nothing)
                if (r < 4) v = make_uint2((v.x & keep) | (SPACES & ~keep), SPACES);
                else v.y = (v.y & keep) | (SPACES & ~keep);
            }
        }
        w[6] = v.x;
        w[7] = v.y;
    }
    cv = 0;
    if (cover && o < n) {  // bits o - 8 .. o + 23 of the bitmap: two words, the second only inside the tiles
        const uint64_t words = ntiles * (SP_TILE / 32);
        if (o == 0) {
            cv = cover[0] << 8;
        } else {
            const uint64_t k = (o - 8) >> 5;
            const uint32_t sh = (uint32_t)(o - 8) & 31u;  // 8 or 24
            cv = (cover[k] >> sh) | ((k + 1 < words ? cover[k + 1] : 0u) << (32u - sh));
        }
        if (cv) {
#pragma unroll
            for (uint32_t j = 0; j < 8; j++) {
                const uint32_t bm = ((((cv >> (4 * j)) & 15u) * 0x00204081u) & 0x01010101u) * 0xFFu;  // bit k of the nibble -> byte k
                w[j] = (w[j] & ~bm) | (0x0A0A0A0Au & bm);
            }
        }
    }
}

// The effects of a thread's own 16 bytes (window bits 8 .. 23): fwd on N and A read from the left, bwd on B read
// from the right.  A lead that is no number decides N to 0; a P decides A to 1, any other lead but R to 0; an R
// decides B to 1, a lead that is no white space to 0; a match byte decides all three to 0.
__device__ inline void cl_effects(const ClMasks &m, uint32_t cv, uint32_t &fwd, uint32_t &bwd) {
    const uint32_t lead = (~m.cont >> 8) & 0xFFFFu, cvo = (cv >> 8) & 0xFFFFu;
    const uint32_t N = (m.N >> 8) & lead & ~cvo, R = (m.R >> 8) & lead & ~cvo, ws = (m.ws >> 8) & lead;
    const uint32_t P = lead & ~((m.ws | m.L | m.N) >> 8) & ~cvo;
    const uint32_t nstop = lead & ~N;  // (a match byte is a lead and no number)
    const uint32_t above = nstop ? ~((2u << (31u - (uint32_t)__builtin_clz(nstop))) - 1u) : ~0u;
    fwd = (nstop ? CL_ND : 0u) | ((uint32_t)__builtin_popcount(N & above) % 3u);
    const uint32_t astop = lead & ~R;
    if (astop) fwd |= CL_AD | ((P >> (31u - (uint32_t)__builtin_clz(astop))) & 1u ? CL_AV : 0u);
    const uint32_t bstop = (lead & ~ws) | R | cvo;
    bwd = bstop ? CL_AD | ((R >> (uint32_t)__builtin_ctz(bstop)) & 1u ? CL_AV : 0u) : 0u;
}

// the effects of every lane's bytes composed with those of the lanes before it (fwd) and after it (bwd)
__device__ inline void cl_wave_scan(uint32_t lane, uint32_t &fwd, uint32_t &bwd) {
    const ClCompose op;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t yf = __shfl_up(fwd, d), yb = __shfl_down(bwd, d);
        if (lane >= d) fwd = op(yf, fwd);
        if (lane + d < 64) bwd = op(yb, bwd);
    }
}

// sum_f[v]: the effect of wave tile v on N and A; sum_b[nwt - 1 - v]: its effect on B (nwt = 4 ntiles wave tiles).
// sum_b == sum_f + nwt + 1: the word between the two arrays is the reset that begins the second scan.
__global__ __launch_bounds__(SP_T) void k_cl_summary(const uint8_t *__restrict__ bytes, uint64_t n, uint64_t ntiles,
                                                     const uint32_t *__restrict__ cover, uint32_t *__restrict__ sum_f,
                                                     uint32_t *__restrict__ sum_b) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint64_t nwt = ntiles * (SP_T / 64);
    if (blockIdx.x == 0 && tid == 0) sum_f[nwt] = CL_RESET;
    uint4 q = sg_load16(bytes, n, ntiles, blockIdx.x);
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t t = tile * SP_T + tid, o = t * SP_PER;
        const uint4 qn = sg_load16(bytes, n, ntiles, tile + gridDim.x);
        uint32_t w[8], cv, fwd, bwd;
        cl_window(bytes, n, ntiles, cover, q, o, lane, w, cv);
        const bool high = ((w[0] | w[1] | w[2] | w[3] | w[4] | w[5] | w[6] | w[7]) & 0x80808080u) != 0u;
        ClMasks m;
        cl_classify<true>(w, __ballot(high) != 0ull, m);
        cl_effects(m, cv, fwd, bwd);
        cl_wave_scan(lane, fwd, bwd);
        if (lane == 63) sum_f[t >> 6] = fwd;
        if (lane == 0) sum_b[nwt - 1 - (t >> 6)] = bwd;
        q = qn;
    }
}

// what k_split_mark writes, for BPE_SPLIT_CL100K.  in_f[v]: N and A on entry to wave tile v from the left;
// in_b[nwt - 1 - v]: B on entry to it from the right (both decided: the scans begin with CL_RESET).
__global__ __launch_bounds__(SP_T) void k_split_mark_cl100k(const uint8_t *__restrict__ bytes, uint64_t n, uint64_t ntiles,
                                                            const uint32_t *__restrict__ cover, const uint32_t *__restrict__ in_f,
                                                            const uint32_t *__restrict__ in_b, uint16_t *__restrict__ mask,
                                                            uint32_t *__restrict__ wcnt) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint64_t nwt = ntiles * (SP_T / 64);
    const ClCompose op;
    uint4 q = sg_load16(bytes, n, ntiles, blockIdx.x);
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t t = tile * SP_T + tid, o = t * SP_PER;
        const uint4 qn = sg_load16(bytes, n, ntiles, tile + gridDim.x);
        const uint32_t cf = in_f[t >> 6], cb = in_b[nwt - 1 - (t >> 6)];
        uint32_t w[8], cv, fwd, bwd;
        cl_window(bytes, n, ntiles, cover, q, o, lane, w, cv);
        const bool high = ((w[0] | w[1] | w[2] | w[3] | w[4] | w[5] | w[6] | w[7]) & 0x80808080u) != 0u;
        ClMasks k;
        cl_classify<false>(w, __ballot(high) != 0ull, k);
        cl_effects(k, cv, fwd, bwd);
        if (lane == 0) fwd = op(cf, fwd);
        if (lane == 63) bwd = op(cb, bwd);
        cl_wave_scan(lane, fwd, bwd);
        uint32_t ef = __shfl_up(fwd, 1), eb = __shfl_down(bwd, 1);  // the state before this thread's bytes and after them
        if (lane == 0) ef = cf;
        if (lane == 63) eb = cb;
        // the chains over the thread's own characters: nst a number whose run holds a multiple of 3 before it,
        // arm A before this byte, fol an R at or after this byte in its white-space run
        const uint32_t lead = (~k.cont >> 8) & 0xFFFFu, cvo = (cv >> 8) & 0xFFFFu;
        const uint32_t oN = (k.N >> 8) & ~cvo, oR = (k.R >> 8) & ~cvo, oWs = k.ws >> 8, oP = ~((k.ws | k.L | k.N) >> 8) & ~cvo;
        uint32_t d = ef & CL_NK, a = (ef >> 3) & 1u, f = (eb >> 3) & 1u, nst = 0, arm = 0, fol = 0;
#pragma unroll
        for (uint32_t b = 0; b < 16; b++) {
            const uint32_t bit = 1u << b;
            if (!(lead & bit)) continue;
            arm |= a ? bit : 0u;
            if (oN & bit) {
                nst |= d == 0u ? bit : 0u;
                d = d == 2u ? 0u : d + 1u;
                a = 0u;
            } else {
                d = 0u;
                a = oP & bit ? 1u : oR & bit ? a : 0u;
            }
        }
#pragma unroll
        for (int b = 15; b >= 0; b--) {
            const uint32_t bit = 1u << b;
            if (!(lead & bit)) continue;
            f = oR & bit ? 1u : (cvo & bit) || !(oWs & bit) ? 0u : f;
            fol |= f ? bit : 0u;
        }
        // the rule (bpe_gpu.h), every predicate a mask over the window: X << 1 is X of the byte before
        const uint32_t R = k.R, S = k.S, ws = k.ws, L = k.L, N = k.N, P = ~(ws | L | N), cont = k.cont;
        const uint32_t ws1 = ws << 1, R1 = R << 1, P1 = P << 1;
        const uint32_t wsn = ((ws >> 1) & ~(k.w2 | k.w3)) | ((ws >> 2) & k.w2) | ((ws >> 3) & k.w3);  // white space at end(i)
        const uint32_t ap = k.ap & ((L | N | (ws & ~S)) << 1);  // an apostrophe a contraction may start at
        const uint32_t c2 = ap & (k.m1 >> 1);
        const uint32_t c3 = ap & (((k.rv >> 1) & (k.e >> 2)) | ((k.l >> 1) & (k.l >> 2)) | (k.ls >> 1));  // ('ſ is three bytes)
        const uint32_t inside = ((c2 | c3) << 1) | (c3 << 2), after = (c2 << 2) | (c3 << 3);
        uint32_t ps = ~cont & ((P | S) << 1);  // the character before this one is P or S, on every byte of this one
        ps |= (ps << 1) & cont;
        ps |= (ps << 1) & cont;
        ps |= (ps << 1) & cont;
        const uint32_t st_l = ~inside & (after | (~(L << 1) & ((N << 1) | R1 | (P1 & (ps << 1)))));
        const uint32_t st_ws = (ws & ~ws1 & ~(P1 & R)) | (ws & ~R & ws1 & (~wsn | (R1 & ~(fol << 8)) | (R1 & (arm << 8))));
        const uint32_t st_p = P & ((L << 1) | (N << 1) | (ws1 & ~(S << 1)));
        uint32_t m = (((N & (nst << 8)) | st_ws | (L & st_l) | st_p) & ~cont) >> 8 & 0xFFFFu;
        if (o == 0) m |= 1u;  // byte 0 starts a piece
        m = o >= n ? 0u : n - o >= SP_PER ? m : m & ((1u << (uint32_t)(n - o)) - 1u);
        mask[t] = (uint16_t)m;
        uint32_t c = (uint32_t)__builtin_popcount(m);
        for (int dd = 32; dd; dd >>= 1) c += __shfl_xor(c, dd);
        if (lane == 0) wcnt[t >> 6] = c;
        q = qn;
    }
}

// out[woff[v] + r] = the position of the r-th start of wave tile v; out[woff[nwt]] = n
__global__ __launch_bounds__(SP_T) void k_split_emit(const uint16_t *__restrict__ mask,
                                                     const unsigned long long *__restrict__ woff, uint64_t ntiles,
                                                     uint64_t n, uint64_t *__restrict__ out) {
    __shared__ uint16_t pos[SP_T / 64][SP_WTILE];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {  // (block-uniform trips: the barriers)
        const uint64_t v = tile * (SP_T / 64) + wv;
        const uint32_t m = mask[v * 64 + lane];
        const uint32_t c = (uint32_t)__builtin_popcount(m);
        uint32_t inc = c;
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t y = __shfl_up(inc, d);
            if ((int)lane >= d) inc += y;
        }
        const uint32_t total = __shfl(inc, 63);
        uint32_t k = inc - c;
        for (uint32_t mm = m; mm; mm &= mm - 1) pos[wv][k++] = (uint16_t)(lane * SP_PER + (uint32_t)__builtin_ctz(mm));
        __syncthreads();
        const unsigned long long base = woff[v];
        for (uint32_t r = lane; r < total; r += 64) out[base + r] = v * SP_WTILE + pos[wv][r];
        __syncthreads();
    }
    if (blockIdx.x == 0 && tid == 0) out[woff[ntiles * (SP_T / 64)]] = n;
}

}  // namespace bpeamd

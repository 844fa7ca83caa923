// split.hip -- pieces of the resident bytes by a two-table rule or by BPE_SPLIT_GPT2; included by engine.hip.
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
//   (rocprim::exclusive_scan of the wave counts, engine.hip)
//   k_split_emit   reads the masks again (n / 8 bytes, not the bytes): a wave
//                  ranks its starts, stages their positions in LDS and writes
//                  them as consecutive 8-byte offsets at its scanned base.
//
// No workgroup waits for another one: the order comes from the scan between
// the two launches.

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

// what k_split_mark writes (the same tiles, grid striding, masks and counts), for the rule above
__global__ __launch_bounds__(SP_T) void k_split_mark_gpt2(const uint8_t *__restrict__ bytes, uint64_t n, uint64_t ntiles,
                                                          uint16_t *__restrict__ mask, uint32_t *__restrict__ wcnt) {
    constexpr uint32_t SPACES = 0x20202020u, B7 = 0x80808080u;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    // (the buffer has 64 bytes of slack past n: a load that begins below n stays inside it)
    auto load16 = [&](uint64_t tile) {
        const uint64_t o = (tile * SP_T + tid) * SP_PER;
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
    };
    uint4 q = load16(blockIdx.x);
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t t = tile * SP_T + tid, o = t * SP_PER;
        const uint4 qn = load16(tile + gridDim.x);
        uint32_t w[6] = {__shfl_up(q.w, 1), q.x, q.y, q.z, q.w, __shfl_down(q.x, 1)};
        if (lane == 0) w[0] = o && o < n ? *(const uint32_t *)(bytes + o - 4) : 0x0A0A0A0Au;  // (o is a multiple of 16)
        if (lane == 63) w[5] = o + SP_PER < n ? (uint32_t)bytes[o + SP_PER] : SPACES;
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
        if (o == 0) m |= 1u;  // byte 0 starts a piece
        m = o >= n ? 0u : n - o >= SP_PER ? m : m & ((1u << (uint32_t)(n - o)) - 1u);
        mask[t] = (uint16_t)m;
        uint32_t c = (uint32_t)__builtin_popcount(m);
        for (int d = 32; d; d >>= 1) c += __shfl_xor(c, d);
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

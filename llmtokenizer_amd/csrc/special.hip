// special.hip -- special tokens (bpe_gpu.h, "Special tokens"); included by engine.hip after split.hip and
// train_split.hip.  All of it runs beside the existing kernels, between or after their launches.
//
// The split (bpe_gpu_split_special), after the rule's own marking kernel and before the count scan:
//   k_sp_find     one pass over the bytes, 16 per thread like k_split_mark.  A byte whose value begins
//                 no special (a 256-bit set) is done.  A candidate is resolved against the specials held
//                 in LDS in lexicographic order: the set is prefix-free, so at most one special matches
//                 and the order of the text against any other special tells on which side it lies: a
//                 binary search of at most 9 steps of at most 64 byte compares.  Bytes at and past n are
//                 never compared: a text that ends in a proper prefix of a special has no match there.
//                 A match sets its bytes in the cover bitmap (atomicOr: idempotent, so the pass may run
//                 twice) and appends (start << 8 | j) to the match list through one atomicAdd per wave;
//                 past the list's capacity it only counts, and the host runs the pass again with room.
//   k_sp_patch    a thread per match [s, e): the start mask gets bit s, loses the bits of (s, e) and gets
//                 bit e (e < n).  For BPE_SPLIT_GPT2 the positions s - 1 and e + 1 .. e + 3 outside any
//                 match are decided again by the scalar form of the rule below over the window the
//                 definition substitutes; a byte right after a match byte begins a segment and is a
//                 start whatever the rule says.  For BPE_SPLIT_GPT2_UNICODE the positions are s - 7 .. s - 1
//                 and e + 1 .. e + 6 and the rule is split.hip's su_starts over b[i - 7 .. i + 7].  Two matches may touch one mask word and may decide the same
//                 position: every write is an atomicOr or atomicAnd of bits whose value is a function
//                 of the bytes and the (complete) cover bitmap alone, so the order does not matter.
//                 For BPE_SPLIT_CL100K nothing is decided again: k_sp_find runs before that rule's marking
//                 kernels, which read the cover bitmap themselves (split.hip), and the patch sets s and e alone.
//   k_sp_recount  the per-1,024-byte counts again from the masks: the scan and k_split_emit run as they are.
//   (rocprim::radix_sort_keys of the match list by start)
//   k_sp_pieces   start -> piece index, a binary search of the emitted offsets; the list stays resident.
// The encode post-pass (bpe_gpu_encode_split), after encode_docs_run has left ids and id offsets:
//   k_sp_idlen    per match the first id of its piece and the ids it loses (all but one);
//   (rocprim::exclusive_scan of those)
//   k_sp_ids      every old id finds the last match at or before it by a binary search of the matches'
//                 first ids and moves down by what was removed before it; a special's first id becomes
//                 256 + n_merges + j, its other ids vanish;
//   k_sp_idoff    every id offset moves down by what the special pieces before its piece lost.
// Training: k_sp_drop marks the piece-table records whose piece is a special piece (key 0xFFFFFFFF: they
// sort past the others and the entry count shrinks by their number).  Decoding: k_sp_dec_expand is
// k_dec_expand with the ids at and above 256 + n_merges copied from the specials' bytes.
//
// No loop has a trip count the text decides (16, 9, 64, 33 and a handful of mask words bound them) and
// no workgroup waits for another one.

namespace bpeamd {

constexpr uint32_t SX_MAX = 256;  // specials at most (BPE_GPU_SPECIAL_MAX_COUNT)
constexpr uint32_t SX_LEN = 64;   // bytes of a special at most (BPE_GPU_SPECIAL_MAX_LEN)
constexpr uint32_t SX_T = 256;    // threads per workgroup of the per-match and per-id kernels
constexpr uint32_t SX_GRID = 2048;
constexpr uint32_t SX_BREAK = 255;  // the index of a text break in the match list (BPE_GPU_TEXT_BREAK; texts.hip): no special's
static_assert(SX_MAX == BPE_GPU_SPECIAL_MAX_COUNT && SX_LEN == BPE_GPU_SPECIAL_MAX_LEN, "bpe_gpu.h names the limits");
static_assert(SX_LEN == TS_DEDUP_MAX, "a special is one deduplicated entry of the piece table");
static_assert(SX_BREAK == BPE_GPU_TEXT_BREAK && SX_BREAK == SX_MAX - 1, "bpe_gpu.h names the reserved index");

// the set as the device sees it (one upload)
struct SpSet {
    uint8_t txt[SX_MAX * SX_LEN];  // sorted lexicographically, each padded to SX_LEN
    uint8_t len[SX_MAX];           // ... their lengths - 1
    uint8_t idx[SX_MAX];           // ... their indices in the caller's list
    uint8_t lenj[SX_MAX];          // length - 1 by the caller's index
    uint32_t first[8];             // the byte values a special begins with
    uint32_t S;
};

__device__ inline uint32_t sx_covered(const uint32_t *cover, uint64_t p) { return (cover[p >> 5] >> (p & 31u)) & 1u; }

// the special that begins at byte p < n (its sorted index), or SX_MAX
__device__ inline uint32_t sx_resolve(const uint8_t *__restrict__ bytes, uint64_t n, uint64_t p, const uint8_t *txt,
                                      const uint8_t *len, uint32_t S) {
    const uint32_t avail = n - p < SX_LEN ? (uint32_t)(n - p) : SX_LEN;
    uint32_t lo = 0, hi = S;
    for (uint32_t step = 0; step < 9; step++) {
        if (lo >= hi) break;
        const uint32_t mid = (lo + hi) >> 1, L = (uint32_t)len[mid] + 1u, m = L < avail ? L : avail;
        const uint8_t *s = txt + mid * SX_LEN;
        int cmp = 0;  // the text against special mid, over the bytes both have
        for (uint32_t i = 0; i < SX_LEN; i++) {
            if (i >= m) break;
            const uint32_t tb = bytes[p + i], sb = s[i];
            if (tb != sb) {
                cmp = tb < sb ? -1 : 1;
                break;
            }
        }
        if (cmp == 0) {
            if (L <= avail) return mid;
            cmp = -1;  // the text ends inside the special: no special matches here, either side will do
        }
        if (cmp < 0) hi = mid;
        else lo = mid + 1;
    }
    return SX_MAX;
}

// ctl[0]: matches found (all of them, also those past cap)
__global__ __launch_bounds__(SP_T) void k_sp_find(const uint8_t *__restrict__ bytes, uint64_t n, uint64_t ntiles,
                                                  const SpSet *__restrict__ set, uint32_t *__restrict__ cover,
                                                  unsigned long long *__restrict__ list, uint32_t cap,
                                                  uint32_t *__restrict__ ctl) {
    __shared__ __align__(16) uint8_t txt[SX_MAX * SX_LEN];
    __shared__ uint8_t len[SX_MAX], idx[SX_MAX];
    __shared__ uint32_t first[8];
    const uint32_t tid = threadIdx.x, S = set->S;
    for (uint32_t k = tid; k < S * (SX_LEN / 16); k += SP_T) ((uint4 *)txt)[k] = ((const uint4 *)set->txt)[k];
    if (tid < S) {
        len[tid] = set->len[tid];
        idx[tid] = set->idx[tid];
    }
    if (tid < 8) first[tid] = set->first[tid];
    __syncthreads();
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {  // (block-uniform trips; every lane runs the body)
        const uint64_t o = (tile * SP_T + tid) * SP_PER;
        // (the buffer has 64 bytes of slack past n: a load that begins below n stays inside it; what it
        // brings from there is masked by p < n below)
        const uint4 q = o < n ? *(const uint4 *)(bytes + o) : make_uint4(0, 0, 0, 0);
        const uint32_t x[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (uint32_t k = 0; k < SP_PER; k++) {
            const uint32_t b = (x[k >> 2] >> (8 * (k & 3))) & 0xFFu;
            const uint64_t p = o + k;
            uint32_t hit = SX_MAX;
            if (p < n && ((first[b >> 5] >> (b & 31u)) & 1u)) hit = sx_resolve(bytes, n, p, txt, len, S);
            const bool found = hit != SX_MAX;
            const uint32_t at = ts_wave_take(found, &ctl[0]);
            if (found) {
                const uint64_t e = p + len[hit] + 1u;  // e <= n
                for (uint64_t w = p >> 5; w <= (e - 1) >> 5; w++) {  // (at most 3 words)
                    const uint64_t a = w << 5;
                    const uint32_t lo = p > a ? (uint32_t)(p - a) : 0u, hi = e - a < 32 ? (uint32_t)(e - a) : 32u;
                    atomicOr(&cover[w], (hi == 32 ? ~0u : (1u << hi) - 1u) & ~((1u << lo) - 1u));
                }
                if (at < cap) list[at] = ((unsigned long long)p << 8) | idx[hit];
            }
        }
    }
}

// ---- BPE_SPLIT_GPT2 for one position: the rule of bpe_gpu.h, byte by byte, over w[0..5] = b[i - 4 .. i + 1]
// as the definition substitutes them (0 < i; the caller has put newlines and the space in)

enum { SXC_P = 0, SXC_L = 1, SXC_N = 2, SXC_S = 3, SXC_W = 4 };

__device__ inline uint32_t sx_cls(uint32_t b) {
    return (b >= 'A' && b <= 'Z') || (b >= 'a' && b <= 'z') || b >= 0x80 ? SXC_L
           : b >= '0' && b <= '9'                                        ? SXC_N
           : b == ' '                                                    ? SXC_S
           : b >= '\t' && b <= '\r'                                      ? SXC_W
                                                                         : SXC_P;
}

// the length of a contraction at window index j (1..3), or 0
__device__ inline uint32_t sx_clen(const uint32_t *w, uint32_t j) {
    if (w[j] != '\'') return 0;
    const uint32_t p = sx_cls(w[j - 1]);
    if (p != SXC_L && p != SXC_N && p != SXC_W) return 0;
    const uint32_t x = w[j + 1], y = w[j + 2];
    if (x == 's' || x == 't' || x == 'm' || x == 'd') return 2;
    return ((x == 'r' || x == 'v') && y == 'e') || (x == 'l' && y == 'l') ? 3 : 0;
}

__device__ inline uint32_t sx_gpt2_start(const uint32_t *w) {
    const uint32_t c = sx_cls(w[4]), p = sx_cls(w[3]), x = sx_cls(w[5]);
    const bool cw = c == SXC_S || c == SXC_W, pw = p == SXC_S || p == SXC_W, xw = x == SXC_S || x == SXC_W;
    if (cw) return !pw || !xw;
    if (pw) return p == SXC_W;
    if (sx_clen(w, 3) >= 2 || sx_clen(w, 2) == 3) return 0;
    if (sx_clen(w, 2) == 2 || sx_clen(w, 1) == 3) return 1;
    return c != p;
}

// ---- BPE_SPLIT_GPT2_UNICODE for one position i (0 < i < n, neither i nor i - 1 a match byte): the rule of
// split.hip's su_starts, one evaluation for the marking kernel and the patch, over b[i - 7 .. i + 7] as the
// definition substitutes them before decoding.  Looking back, everything at or before the nearest match byte or
// the start of the text reads as a newline; looking ahead, everything from the nearest match byte or n on reads
// as a space (the segment ends there).  i is window byte 8; the window bytes the rule does not read are spaces.
__device__ inline uint32_t sx_gpt2u_start(const uint8_t *__restrict__ bytes, uint64_t n, const uint32_t *__restrict__ cover,
                                          uint64_t i) {
    uint32_t w[8] = {0x20202020u, 0x20202020u, (uint32_t)bytes[i] | 0x20202000u, 0x20202020u,
                     0x20202020u, 0x20202020u, 0x20202020u, 0x20202020u};
    bool cut = false;
#pragma unroll
    for (uint32_t d = 1; d <= 7; d++) {
        cut = cut || i < d || sx_covered(cover, i - d);
        const uint32_t b = cut ? (uint32_t)'\n' : (uint32_t)bytes[i - d], q = 8u - d, sh = 8u * (q & 3u);
        w[q >> 2] = (w[q >> 2] & ~(0xFFu << sh)) | (b << sh);
    }
    cut = false;
#pragma unroll
    for (uint32_t d = 1; d <= 7; d++) {
        cut = cut || i + d >= n || sx_covered(cover, i + d);
        const uint32_t b = cut ? (uint32_t)' ' : (uint32_t)bytes[i + d], q = 8u + d, sh = 8u * (q & 3u);
        w[q >> 2] = (w[q >> 2] & ~(0xFFu << sh)) | (b << sh);
    }
    return (su_starts(w) >> 8) & 1u;
}

__global__ __launch_bounds__(SX_T) void k_sp_patch(const uint8_t *__restrict__ bytes, uint64_t n,
                                                   const unsigned long long *__restrict__ list, uint32_t M,
                                                   const SpSet *__restrict__ set, const uint32_t *__restrict__ cover,
                                                   uint32_t *mask32, int gpt2) {
    for (uint64_t m = (uint64_t)blockIdx.x * SX_T + threadIdx.x; m < M; m += (uint64_t)gridDim.x * SX_T) {
        const uint64_t s = list[m] >> 8, e = s + set->lenj[list[m] & 0xFFu] + 1u;
        for (uint64_t w = s >> 5; w <= (e - 1) >> 5; w++) {  // the bits of (s, e) go (at most 3 words)
            const uint64_t a = w << 5;
            const uint32_t lo = s + 1 > a ? (uint32_t)(s + 1 - a) : 0u, hi = e - a < 32 ? (uint32_t)(e - a) : 32u;
            if (lo < hi) atomicAnd(&mask32[w], ~((hi == 32 ? ~0u : (1u << hi) - 1u) & ~((1u << lo) - 1u)));
        }
        atomicOr(&mask32[s >> 5], 1u << (s & 31u));
        if (e < n) atomicOr(&mask32[e >> 5], 1u << (e & 31u));
        if (!gpt2) continue;
        if (gpt2 == 2) {  // BPE_SPLIT_GPT2_UNICODE: s - 7 .. s - 1 and e + 1 .. e + 6 (e itself is set above)
#pragma unroll 1
            for (uint32_t k = 0; k < 13; k++) {
                if (k < 7 && s + k < 7) continue;
                const uint64_t i = k < 7 ? s + k - 7 : e + (uint64_t)(k - 6);
                if (i >= n || sx_covered(cover, i)) continue;
                const uint32_t v = i && !sx_covered(cover, i - 1) ? sx_gpt2u_start(bytes, n, cover, i) : 1u;
                if (v) atomicOr(&mask32[i >> 5], 1u << (i & 31u));
                else atomicAnd(&mask32[i >> 5], ~(1u << (i & 31u)));
            }
            continue;
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (k == 0 && s == 0) continue;
            const uint64_t i = k == 0 ? s - 1 : e + (uint64_t)k;
            if (i >= n || sx_covered(cover, i)) continue;
            uint32_t v = 1;  // (byte 0 and the byte after a match start a piece: a segment begins there)
            if (i && !sx_covered(cover, i - 1)) {
                uint32_t w[6];
                bool cut = false;  // a match byte, or the start of the text, lies at or after this one
#pragma unroll
                for (uint32_t d = 1; d <= 4; d++) {
                    cut = cut || i < d || sx_covered(cover, i - d);
                    w[4 - d] = cut ? (uint32_t)'\n' : (uint32_t)bytes[i - d];
                }
                w[4] = bytes[i];
                w[5] = i + 1 < n && !sx_covered(cover, i + 1) ? (uint32_t)bytes[i + 1] : (uint32_t)' ';
                v = sx_gpt2_start(w);
            }
            if (v) atomicOr(&mask32[i >> 5], 1u << (i & 31u));
            else atomicAnd(&mask32[i >> 5], ~(1u << (i & 31u)));
        }
    }
}

// wcnt[v] = the starts in bytes [1024 v, 1024 v + 1024), as the marking kernels leave them
__global__ __launch_bounds__(SP_T) void k_sp_recount(const uint16_t *__restrict__ mask, uint64_t ntiles,
                                                     uint32_t *__restrict__ wcnt) {
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t t = tile * SP_T + threadIdx.x;
        uint32_t c = (uint32_t)__builtin_popcount((uint32_t)mask[t]);
        for (int d = 32; d; d >>= 1) c += __shfl_xor(c, d);
        if ((threadIdx.x & 63u) == 0) wcnt[t >> 6] = c;
    }
}

// the largest k in [0, count] with a[k'] < v for every k' < k (a ascending; 33 steps reach count = 2^32)
template <typename T>
__device__ inline uint64_t sx_lower(const T *__restrict__ a, uint64_t count, uint64_t v, uint32_t shift) {
    uint64_t lo = 0, hi = count;
    for (uint32_t step = 0; step < 33; step++) {
        if (lo >= hi) break;
        const uint64_t mid = lo + (hi - lo) / 2;
        if ((uint64_t)(a[mid] >> shift) < v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// list[m] = (start << 8 | j), sorted -> (piece << 8 | j): off[piece] == start
__global__ __launch_bounds__(SX_T) void k_sp_pieces(const unsigned long long *__restrict__ list, uint32_t M,
                                                    const uint64_t *__restrict__ off, uint64_t P,
                                                    unsigned long long *__restrict__ out, uint32_t *__restrict__ bad) {
    for (uint64_t m = (uint64_t)blockIdx.x * SX_T + threadIdx.x; m < M; m += (uint64_t)gridDim.x * SX_T) {
        const uint64_t s = list[m] >> 8, p = sx_lower(off, P, s, 0);
        if (p >= P || off[p] != s) *bad = 1u;  // (cannot happen: the patch made s a start)
        out[m] = ((unsigned long long)p << 8) | (list[m] & 0xFFull);
    }
}

// ---------------------------------------------------------------- the encode post-pass

// ist[m] = the first id of match m's piece, rem[m] = the ids it loses; rem[M] = 0 (the scan's total).
// breaks: the list of a text batch, where an entry with the index SX_BREAK is a break piece, which keeps no id
__global__ __launch_bounds__(SX_T) void k_sp_idlen(const unsigned long long *__restrict__ pieces, uint32_t M,
                                                   const uint64_t *__restrict__ id_off, uint64_t *__restrict__ ist,
                                                   uint64_t *__restrict__ rem, int breaks) {
    for (uint64_t m = (uint64_t)blockIdx.x * SX_T + threadIdx.x; m <= M; m += (uint64_t)gridDim.x * SX_T) {
        if (m == M) {
            rem[m] = 0;
            continue;
        }
        const uint64_t p = pieces[m] >> 8, a = id_off[p], b = id_off[p + 1];
        ist[m] = a;
        if (breaks && (pieces[m] & 0xFFull) == SX_BREAK) rem[m] = b - a;
        else rem[m] = b > a ? b - a - 1 : 0;
    }
}

// rsum: the exclusive scan of rem ([M + 1]); out[] receives len - rsum[M] ids
__global__ __launch_bounds__(SX_T) void k_sp_ids(const uint32_t *__restrict__ ids, uint64_t len,
                                                 const unsigned long long *__restrict__ pieces, uint32_t M,
                                                 const uint64_t *__restrict__ ist, const uint64_t *__restrict__ rsum,
                                                 uint32_t base, uint32_t *__restrict__ out, int breaks) {
    for (uint64_t q = (uint64_t)blockIdx.x * SX_T + threadIdx.x; q < len; q += (uint64_t)gridDim.x * SX_T) {
        const uint64_t k = sx_lower(ist, M, q + 1, 0);  // matches whose piece begins at or before id q
        if (k == 0) {
            out[q] = ids[q];
            continue;
        }
        const uint64_t m = k - 1, a = ist[m], r0 = rsum[m], r1 = rsum[k];
        if (breaks && (pieces[m] & 0xFFull) == SX_BREAK) {
            if (q >= a + (r1 - r0)) out[q - r1] = ids[q];  // past the break piece, none of whose ids stays
            continue;
        }
        if (q > a + (r1 - r0)) out[q - r1] = ids[q];  // past the special piece
        else if (q == a) out[a - r0] = base + (uint32_t)(pieces[m] & 0xFFull);
    }
}

__global__ __launch_bounds__(SX_T) void k_sp_idoff(const uint64_t *__restrict__ id_off, uint64_t ndocs,
                                                   const unsigned long long *__restrict__ pieces, uint32_t M,
                                                   const uint64_t *__restrict__ rsum, uint64_t *__restrict__ out) {
    for (uint64_t d = (uint64_t)blockIdx.x * SX_T + threadIdx.x; d <= ndocs; d += (uint64_t)gridDim.x * SX_T)
        out[d] = id_off[d] - rsum[sx_lower(pieces, M, d, 8)];  // (the special pieces before piece d)
}

// ---------------------------------------------------------------- training

// key[e]: the piece of record e; a special piece's record gets the key 0xFFFFFFFF and is counted in *dropped
__global__ __launch_bounds__(SX_T) void k_sp_drop(uint32_t *__restrict__ key, uint64_t E,
                                                  const unsigned long long *__restrict__ pieces, uint32_t M,
                                                  uint32_t *__restrict__ dropped) {
    for (uint64_t base = (uint64_t)blockIdx.x * SX_T; base < E; base += (uint64_t)gridDim.x * SX_T) {  // (block-uniform trips)
        const uint64_t e = base + threadIdx.x;
        bool is = false;
        if (e < E) {
            const uint64_t p = key[e], k = sx_lower(pieces, M, p, 8);
            is = k < M && (pieces[k] >> 8) == p;
            if (is) key[e] = 0xFFFFFFFFu;
        }
        (void)ts_wave_take(is, dropped);
    }
}

// ---------------------------------------------------------------- decoding

// k_dec_expand with the ids V .. V + S - 1 copied from the specials: special j is sp[soff[j] .. soff[j + 1])
__global__ void k_sp_dec_expand(const uint32_t *__restrict__ ids, uint64_t len, const uint32_t *__restrict__ pairs,
                                const uint64_t *__restrict__ elen, const uint64_t *__restrict__ off, uint32_t V,
                                const uint8_t *__restrict__ sp, const uint32_t *__restrict__ soff,
                                uint8_t *__restrict__ out) {
    for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q < len; q += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t o = off[q];
        if (ids[q] >= V) {
            const uint32_t a = soff[ids[q] - V], L = soff[ids[q] - V + 1] - a;
            for (uint32_t i = 0; i < SX_LEN; i++) {
                if (i >= L) break;
                out[o + i] = sp[a + i];
            }
            continue;
        }
        uint32_t stack[48];
        int top = 0;
        stack[top++] = ids[q];
        while (top > 0) {
            const uint32_t x = stack[--top];
            if (dec_leaf(x, pairs)) {
                if ((uint8_t)x) out[o++] = (uint8_t)x;
                continue;
            }
            if (top + 2 <= 48) {
                stack[top++] = pairs[2 * (x - 256) + 1];
                stack[top++] = pairs[2 * (x - 256)];
                continue;
            }
            // deep chain: emit x byte by byte with a descent per byte
            for (uint64_t k = 0; k < elen[x]; k++) {
                uint32_t y = x;
                uint64_t kk = k;
                while (!dec_leaf(y, pairs)) {
                    const uint32_t ya = pairs[2 * (y - 256)], yb = pairs[2 * (y - 256) + 1];
                    if (kk < elen[ya]) y = ya;
                    else { kk -= elen[ya]; y = yb; }
                }
                out[o++] = (uint8_t)y;
            }
        }
    }
}

}  // namespace bpeamd

// split_o200k.hip -- the marking pass of BPE_SPLIT_O200K (bpe_gpu.h); included by engine.hip after split.hip, whose
// window, loads and ASCII predicates it uses.  It writes exactly what k_split_mark writes; its host side is
// mark_o200k of pieces.hip.
//
// The rule is an automaton (src/bpe_o200k_rule.h): a character is a symbol, a kind and up to three flags, and a
// piece start is a function of the symbol and of one of eight states that the characters before it leave.  Every
// chain of the pattern that no window bounds is a path through those states: the case phases of a letter run,
// the contractions that hang on each other, the M run behind punctuation, the tail of \r \n /, the numbers in
// threes.  Two flags read ahead without bound instead (only U up to the end of the letter run; an R later in the
// white-space run); they are a second automaton of four states read from the right.
//
// What a stretch of text does to either automaton is a map from states to states, eight bytes, byte s the state
// after the stretch when s was the state before it.  Maps compose by looking one up in the other, which is two
// v_perm_b32, and composition of maps is associative whatever the maps are, so:
//   k_o2_summary       one pass over the bytes: the map of every wave tile (1,024 bytes) read from the left and,
//                      stored in reverse order behind a reset, read from the right;
//   (one rocprim::exclusive_scan of that array with O2Compose: the state on entry to every wave tile)
//   k_split_mark_o200k the marking pass: the same maps per thread, a scan of them across the wave's lanes from the
//                      tile's entry states, 16 steps from the right over the thread's own bytes for the two flags
//                      and 16 from the left through the automaton, which gives the start bits.
// The 128 symbols' maps (bit 7 of byte s: the symbol starts a piece in state s) are folded from o2_step on the
// host, passed by value and staged in LDS, 1 KiB; a thread's 16 symbols are four words built from the predicate
// masks of its window.  A character belongs to the thread that holds its lead byte; the other bytes of a sequence
// are a symbol of their own that changes nothing.  No loop's trip count depends on the text, no workgroup waits
// for another one, and there are no atomics.
//
// With specials the bytes of the matches (the cover bitmap of special.hip, found before this pass) read as
// newlines before anything is decoded and are the symbol O2_X, which sends every state to the fresh one and, from
// the right, to the end of a text: a segment begins after it and ends before it.  k_sp_patch then sets the
// matches' own bits.  The gap bytes of a text batch are in the same bitmap.

#define BPE_UCC_STORAGE __device__ const
#include "unicode_case_classes.h"  // BPE_UCC_STAGE1 / BPE_UCC_STAGE2 in device memory
#define O2_FN __host__ __device__ static inline
#include "../src/bpe_o200k_rule.h"

namespace bpeamd {

constexpr uint64_t O2_LOW3 = 0x0707070707070707ull;  // the state of every byte of a map, without the start bits
constexpr uint64_t O2_IDENT = 0x0706050403020100ull;
constexpr uint64_t O2_TO_FRESH = 0ull;                     // the map of the text before byte 0 (every state to O2_FRESH)
constexpr uint64_t O2_TO_END = 0x0101010101010101ull * O2_BACK_END;  // ... and, from the right, of what lies past its end

struct O2Table {
    uint64_t e[O2_SYMBOLS];  // byte s: o2_step(s, symbol), bit 7 its start
};

static O2Table o2_table() {
    O2Table T;
    for (int sym = 0; sym < O2_SYMBOLS; sym++) {
        uint64_t v = 0;
        for (int s = 0; s < O2_STATES; s++) {
            int start = 0;
            const int to = (sym & 15) < O2_KINDS ? o2_step(s, sym, &start) : s;
            v |= (uint64_t)(to | (start << 7)) << (8 * s);
        }
        T.e[sym] = v;
    }
    return T;
}

// the map of a stretch (a) followed by the map b of the next one (from the right: the stretch to the right first);
// both without start bits
struct O2Compose {
    __host__ __device__ inline uint64_t operator()(uint64_t a, uint64_t b) const {
#if defined(__HIP_DEVICE_COMPILE__)
        const uint32_t bl = (uint32_t)b, bh = (uint32_t)(b >> 32);  // selector bytes 0 .. 3 take from bl, 4 .. 7 from bh
        return ((uint64_t)__builtin_amdgcn_perm(bh, bl, (uint32_t)(a >> 32)) << 32) | __builtin_amdgcn_perm(bh, bl, (uint32_t)a);
#else
        uint64_t r = 0;
        for (int s = 0; s < 8; s++) r |= ((b >> (8 * ((a >> (8 * s)) & 7u))) & 0xFFull) << (8 * s);
        return r;
#endif
    }
};

// the predicates of a thread's window as masks (bit q for window byte q, b[o - 8 + q]); every byte of a
// well-formed sequence carries its character's class, a byte >= 0x80 in no sequence is in no class mask
struct O2Masks {
    uint32_t U, l, B, M, N, ws, R, S, cont;  // case classes; numbers; White_Space; \r \n; the space; continuation bytes
    uint32_t n2, n3, n4;                     // leads of sequences of two / three / four bytes
    uint32_t ap, sl, m1, rv, e, ll, ls;      // ' and /; s t m d; r v; e; l (A-Z folded); the lead of U+017F
};

// w[0..7] = b[o - 8 .. o + 23] after the substitutions (cl_window); decode: some byte of the wave's windows is >= 0x80
__device__ inline void o2_classify(const uint32_t *w, bool decode, O2Masks &m) {
    constexpr uint32_t SPACES = 0x20202020u, B7 = 0x80808080u;
    m = O2Masks{};
#pragma unroll
    for (uint32_t j = 1; j < 8; j++) {  // (the rule reads b[i - 4 ..]: word 0 only through the sequences below)
        const uint32_t hi = w[j] & B7;
        const uint32_t x = (w[j] & ~B7) | (hi - (hi >> 7));  // a byte >= 0x80 becomes 0x7f: in none of the ranges below
        const uint32_t f = x | SPACES;                       // A-Z onto a-z and nothing else into it
        const uint32_t s = sg_in(x, ' ', ' ');
        m.S |= su_nib(s) << (4 * j);
        m.R |= su_nib(sg_in(x, '\n', '\n') | sg_in(x, '\r', '\r')) << (4 * j);
        m.ws |= su_nib(s | sg_in(x, '\t', '\r')) << (4 * j);
        m.U |= su_nib(sg_in(x, 'A', 'Z')) << (4 * j);
        m.l |= su_nib(sg_in(x, 'a', 'z')) << (4 * j);
        m.N |= su_nib(sg_in(x, '0', '9')) << (4 * j);
        m.ap |= su_nib(sg_in(x, '\'', '\'')) << (4 * j);
        m.sl |= su_nib(sg_in(x, '/', '/')) << (4 * j);
        m.m1 |= su_nib(sg_in(f, 'd', 'd') | sg_in(f, 'm', 'm') | sg_in(f, 's', 't')) << (4 * j);
        m.rv |= su_nib(sg_in(f, 'r', 'r') | sg_in(f, 'v', 'v')) << (4 * j);
        m.e |= su_nib(sg_in(f, 'e', 'e')) << (4 * j);
        m.ll |= su_nib(sg_in(f, 'l', 'l')) << (4 * j);
    }
    if (!decode) return;  // (wave-uniform)
    // window bytes 4 .. 27 as the lead of a sequence, as su_starts does: the character before byte 8 begins at
    // byte 4 or later, the one after byte 23 at byte 27 or earlier
#pragma unroll
    for (uint32_t q = 4; q <= 27; q++) {
        const uint32_t v = q & 3u ? __builtin_amdgcn_alignbit(w[(q >> 2) + 1], w[q >> 2], 8u * (q & 3u)) : w[q >> 2];
        const uint32_t b0 = v & 0xFFu, b1 = (v >> 8) & 0x3Fu, b2 = (v >> 16) & 0x3Fu, b3 = (v >> 24) & 0x3Fu;
        const uint32_t cp2 = ((b0 & 0x1Fu) << 6) | b1, cp3 = ((b0 & 0x0Fu) << 12) | (b1 << 6) | b2;
        const uint32_t cp4 = ((b0 & 0x07u) << 18) | (b1 << 12) | (b2 << 6) | b3;
        const bool ok2 = b0 >= 0xC2u && b0 <= 0xDFu && (v & 0xC000u) == 0x8000u;
        const bool ok3 = (b0 & 0xF0u) == 0xE0u && (v & 0xC0C000u) == 0x808000u && cp3 >= 0x800u && (cp3 & 0xF800u) != 0xD800u;
        const bool ok4 = (b0 & 0xF8u) == 0xF0u && (v & 0xC0C0C000u) == 0x80808000u && cp4 >= 0x10000u && cp4 <= 0x10FFFFu;
        const uint32_t len = ok2 ? 2u : ok3 ? 3u : ok4 ? 4u : 0u;
        const uint32_t cp = ok2 ? cp2 : ok3 ? cp3 : ok4 ? cp4 : 0u;
        const uint32_t t = (BPE_UCC_STAGE2[32u * BPE_UCC_STAGE1[cp >> 8] + ((cp >> 3) & 31u)] >> (4u * (cp & 7u))) & 15u;
        const uint32_t rng = ((1u << len) - 1u) << q;  // the bytes of the sequence (none when nothing is led here)
        m.U |= t == 1u ? rng : 0u;
        m.l |= t == 2u ? rng : 0u;
        m.B |= t == 3u ? rng : 0u;
        m.M |= t == 4u ? rng : 0u;
        m.N |= t == 5u ? rng : 0u;
        m.ws |= t == 6u ? rng : 0u;
        m.cont |= rng & (rng - 1u);
        m.n2 |= ok2 ? 1u << q : 0u;
        m.n3 |= ok3 ? 1u << q : 0u;
        m.n4 |= ok4 ? 1u << q : 0u;
        m.ls |= ok2 && cp2 == 0x17Fu ? 1u << q : 0u;
        if (q % 8u == 3u) __builtin_amdgcn_sched_barrier(0);  // eight lookups in flight at a time
    }
}

// bits 0 .. 3 of x -> bit 0 of bytes 0 .. 3
__device__ inline uint32_t o2_spread(uint32_t x) { return ((x & 15u) * 0x00204081u) & 0x01010101u; }

// A thread's 16 symbols as four words, a byte each, from its masks (without the two flags that read ahead, which
// only decide starts), and the 16-bit masks of its own bytes that the chains from the right read: own.x U,
// own.y l B M, own.z W, own.w R (leads only; a match byte is in none of them).
__device__ inline void o2_symbols(const O2Masks &m, uint32_t cv, uint32_t *sym, uint4 &own) {
    const uint32_t lead = ~m.cont, let = m.U | m.l | m.B | m.M, one = ~(m.n2 | m.n3 | m.n4);
    const uint32_t lets = let >> 1, wss = m.ws >> 1;  // the class at end(i): the next character's
    const uint32_t nlet = (lets & one) | ((lets >> 1) & m.n2) | ((lets >> 2) & m.n3) | ((lets >> 3) & m.n4);
    const uint32_t wsn = (wss & one) | ((wss >> 1) & m.n2) | ((wss >> 2) & m.n3) | ((wss >> 3) & m.n4);
    const uint32_t ws1 = m.ws << 1, R1 = m.R << 1;
    const uint32_t kW = m.ws & ~m.R & lead, kR = m.R & ~cv, pish = lead & ~(let | m.N | m.ws);
    const uint32_t cend = ((m.ap << 1) & (m.m1 | m.ls)) | ((m.ap << 2) & (((m.rv << 1) & m.e) | ((m.ll << 1) & m.ll)));
    const uint32_t contr = ((m.m1 | m.ls) >> 1) | ((m.rv >> 1) & (m.e >> 2)) | ((m.ll >> 1) & (m.ll >> 2));
    const uint32_t f0 = (let & lead & cend) | (kW & (~ws1 | ~wsn)) | (kR & ~ws1) | (pish & nlet);
    const uint32_t f1 = (let & lead & (ws1 & ~R1)) | (kW & R1) | (pish & (m.S << 1));
    const uint32_t f2 = m.ap & contr;
    const uint32_t kU = m.U & lead, kl = m.l & lead, kB = m.B & lead, kM = m.M & lead, kN = m.N & lead;
    // the kind's four bits (bpe_o200k_rule.h: U 1, l 2, B 3, M 4, N 5, W 6, R 7, SL 8, AP 9, X 10, CONT 11)
    const uint32_t k0 = kU | kB | kN | kR | m.ap | m.cont, k1 = kl | kB | kW | kR | cv | m.cont;
    const uint32_t k2 = kM | kN | kW | kR, k3 = m.sl | m.ap | cv | m.cont;
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) {
        const uint32_t sh = 8u + 4u * j;
        sym[j] = o2_spread(k0 >> sh) | (o2_spread(k1 >> sh) << 1) | (o2_spread(k2 >> sh) << 2) | (o2_spread(k3 >> sh) << 3) |
                 (o2_spread(f0 >> sh) << 4) | (o2_spread(f1 >> sh) << 5) | (o2_spread(f2 >> sh) << 6);
    }
    own = make_uint4((kU >> 8) & 0xFFFFu, ((kl | kB | kM) >> 8) & 0xFFFFu, (kW >> 8) & 0xFFFFu, (kR >> 8) & 0xFFFFu);
}

// symbol k of a thread's 16
__device__ inline uint32_t o2_sym(const uint32_t *sym, uint32_t k) { return (sym[k >> 2] >> (8u * (k & 3u))) & 0x7Fu; }

// The maps of a thread's own 16 bytes: fwd the automaton's, bwd the map of the chains read from the right (states
// 0 .. 3: bit 0 AU, bit 1 FOL; o2_back).  From the right the character nearest the left decides: the lowest lead
// that is no U decides AU (1 unless it is a letter or M), the lowest that is no W decides FOL (1 when it is an R).
__device__ inline void o2_effects(const uint64_t *tbl, const uint32_t *sym, const uint4 own, uint32_t lead, uint64_t &fwd, uint64_t &bwd) {
    const O2Compose op;
    fwd = O2_IDENT;
#pragma unroll
    for (uint32_t k = 0; k < 16; k++) fwd = op(fwd, tbl[o2_sym(sym, k)] & O2_LOW3);
    const uint32_t astop = lead & ~own.x, fstop = lead & ~own.z;
    const uint32_t au = astop ? ((own.y >> (uint32_t)__builtin_ctz(astop)) & 1u ? 0u : 0x01010101u) : 0x01000100u;
    const uint32_t fol = fstop ? ((own.w >> (uint32_t)__builtin_ctz(fstop)) & 1u ? 0x02020202u : 0u) : 0x02020000u;
    bwd = (O2_IDENT & 0xFFFFFFFF00000000ull) | au | fol;
}

// the maps of every lane's bytes composed with those of the lanes before it (fwd) and after it (bwd)
__device__ inline void o2_wave_scan(uint32_t lane, uint64_t &fwd, uint64_t &bwd) {
    const O2Compose op;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint64_t yf = __shfl_up((unsigned long long)fwd, d), yb = __shfl_down((unsigned long long)bwd, d);
        if (lane >= d) fwd = op(yf, fwd);
        if (lane + d < 64) bwd = op(yb, bwd);
    }
}

__device__ inline void o2_stage(const O2Table &T, uint64_t *tbl) {
    if (threadIdx.x < O2_SYMBOLS) tbl[threadIdx.x] = T.e[threadIdx.x];
    __syncthreads();
}

// sum[v]: the map of wave tile v; sum[nwt]: the reset; sum[2 nwt - v]: its map from the right (nwt = 4 ntiles)
__global__ __launch_bounds__(SP_T) void k_o2_summary(const uint8_t *__restrict__ bytes, uint64_t n, uint64_t ntiles,
                                                     const uint32_t *__restrict__ cover, const O2Table T, uint64_t *__restrict__ sum) {
    __shared__ uint64_t tbl[O2_SYMBOLS];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint64_t nwt = ntiles * (SP_T / 64);
    o2_stage(T, tbl);
    if (blockIdx.x == 0 && tid == 0) sum[nwt] = O2_TO_END;
    uint4 q = sg_load16(bytes, n, ntiles, blockIdx.x);
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t t = tile * SP_T + tid, o = t * SP_PER;
        const uint4 qn = sg_load16(bytes, n, ntiles, tile + gridDim.x);
        uint32_t w[8], cv, sym[4];
        uint64_t fwd, bwd;
        uint4 own;
        cl_window(bytes, n, ntiles, cover, q, o, lane, w, cv);
        const bool high = ((w[0] | w[1] | w[2] | w[3] | w[4] | w[5] | w[6] | w[7]) & 0x80808080u) != 0u;
        O2Masks m;
        o2_classify(w, __ballot(high) != 0ull, m);
        o2_symbols(m, cv, sym, own);
        o2_effects(tbl, sym, own, (~m.cont >> 8) & 0xFFFFu, fwd, bwd);
        o2_wave_scan(lane, fwd, bwd);
        if (lane == 63) sum[t >> 6] = fwd;
        if (lane == 0) sum[2 * nwt - (t >> 6)] = bwd;
        q = qn;
    }
}

// what k_split_mark writes, for BPE_SPLIT_O200K.  in[v]: the map of all text before wave tile v; in[2 nwt - v]: of
// all text after it, from the right (both send every state to one: the scan begins with O2_TO_FRESH and passes
// the reset).
__global__ __launch_bounds__(SP_T) void k_split_mark_o200k(const uint8_t *__restrict__ bytes, uint64_t n, uint64_t ntiles,
                                                           const uint32_t *__restrict__ cover, const O2Table T,
                                                           const uint64_t *__restrict__ in, uint16_t *__restrict__ mask,
                                                           uint32_t *__restrict__ wcnt) {
    __shared__ uint64_t tbl[O2_SYMBOLS];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint64_t nwt = ntiles * (SP_T / 64);
    const O2Compose op;
    o2_stage(T, tbl);
    uint4 q = sg_load16(bytes, n, ntiles, blockIdx.x);
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t t = tile * SP_T + tid, o = t * SP_PER;
        const uint4 qn = sg_load16(bytes, n, ntiles, tile + gridDim.x);
        const uint64_t cf = in[t >> 6], cb = in[2 * nwt - (t >> 6)];
        uint32_t w[8], cv, sym[4];
        uint64_t fwd, bwd;
        uint4 own;
        cl_window(bytes, n, ntiles, cover, q, o, lane, w, cv);
        const bool high = ((w[0] | w[1] | w[2] | w[3] | w[4] | w[5] | w[6] | w[7]) & 0x80808080u) != 0u;
        O2Masks k;
        o2_classify(w, __ballot(high) != 0ull, k);
        o2_symbols(k, cv, sym, own);
        const uint32_t lead = (~k.cont >> 8) & 0xFFFFu;
        o2_effects(tbl, sym, own, lead, fwd, bwd);
        if (lane == 0) fwd = op(cf, fwd);
        if (lane == 63) bwd = op(cb, bwd);
        o2_wave_scan(lane, fwd, bwd);
        uint64_t ef = __shfl_up((unsigned long long)fwd, 1), eb = __shfl_down((unsigned long long)bwd, 1);
        if (lane == 0) ef = cf;
        if (lane == 63) eb = cb;
        // from the right over the thread's own bytes: au / fol, the two chains as they stand to the right of each lead
        uint32_t a = (uint32_t)eb & 1u, f = ((uint32_t)eb >> 1) & 1u, au = 0, fol = 0;
#pragma unroll
        for (int b = 15; b >= 0; b--) {
            const uint32_t bit = 1u << b;
            if (!(lead & bit)) continue;
            au |= a ? bit : 0u;
            fol |= f ? bit : 0u;
            a = own.x & bit ? a : own.y & bit ? 0u : 1u;
            f = own.w & bit ? 1u : own.z & bit ? f : 0u;
        }
        // the two flags that read ahead: a U behind B or M with only U up to the end of its letter run (F2), a W
        // behind an R with no R left in its white-space run (F0)
        const uint32_t x2 = own.x & (((k.B | k.M) << 1) >> 8) & au, x0 = own.z & ((k.R << 1) >> 8) & ~fol;
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) sym[j] |= (o2_spread(x2 >> (4 * j)) << 6) | (o2_spread(x0 >> (4 * j)) << 4);
        // from the left through the automaton
        uint32_t st = (uint32_t)ef & 7u, m = 0;
#pragma unroll
        for (uint32_t b = 0; b < 16; b++) {
            const uint32_t v = (uint32_t)(tbl[o2_sym(sym, b)] >> (8u * st)) & 0xFFu;
            m |= (v >> 7) << b;
            st = v & 7u;
        }
        if (o == 0) m |= 1u;  // byte 0 starts a piece
        m = o >= n ? 0u : n - o >= SP_PER ? m : m & ((1u << (uint32_t)(n - o)) - 1u);
        mask[t] = (uint16_t)m;
        uint32_t c = (uint32_t)__builtin_popcount(m);
        for (int dd = 32; dd; dd >>= 1) c += __shfl_xor(c, dd);
        if (lane == 0) wcnt[t >> 6] = c;
        q = qn;
    }
}

}  // namespace bpeamd

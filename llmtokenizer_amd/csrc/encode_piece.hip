// encode_piece.hip -- piece-local replay over a BATCH OF DOCUMENTS (pieces); included by engine.hip.
//
// The window encoders (encode_win.hip, encode_docs.hip) replay the merge list
// layer by layer, so their cost follows the list and their 16-bit LDS layout
// bounds it (EW_MAX_MERGES, EW_MAX_BATCHES).  This encoder's cost follows the
// PIECE: a piece of k bytes needs at most k - 1 merges whatever the list holds,
// and pieces are independent.  Inside one piece the oracle's replay (merges in
// rank order, every occurrence left to right) equals
//   1. take the smallest rank among the piece's adjacent pairs,
//   2. merge all its occurrences left to right (an a == a run pairs greedily
//      from its first token),
//   3. look the changed pairs up, and repeat
// because a merge of rank r creates only pairs holding its new id 256 + r, and
// every record that uses that id has a rank above r (a record naming an id at
// or above its own never matches and is not in the table; of a repeated pair
// only the first record can match): the ranks a piece applies only rise, and
// no lower rank can appear later.  Ids are the list's own: no layers, no role
// masks, no relabeling.
//
// Work split: ONE WAVE owns a tile and needs no other wave, so the round loop
// has no workgroup barrier (ep_sync orders the wave's own LDS traffic).  Tile w
// owns the pieces that START in bytes [w * EP_C, (w + 1) * EP_C) and loads
// from the first such start to the end of the last such piece: every piece of
// at most EP_PIECE_MAX = EP_W - EP_C bytes fits.  A longer piece can only be
// the last one its tile owns (EP_PIECE_MAX >= EP_C: it ends beyond the core);
// the tile leaves it out and counts it, and the host sends it through the
// per-document fallback (engine.hip); given a list (EncPieceArgs::lng) the
// tile also appends the piece to it, for k_enc_long (encode_long.hip), and
// only what that kernel leaves goes to the fallback.  The tile's first piece comes from a
// lane-parallel search of the resident offsets, 64 probes per round trip.
//
// LDS per position: the id (u32) and the cached rank of the pair starting
// there (u32; EP_NONE, EP_LOOK = look it up again).  Token starts (sb) and
// piece starts (pb) are bitmaps; next / previous token are ctz / clz scans
// (ew_next / ew_prev).  A pair never reaches across a piece start.  The
// positions in use are dealt to the lanes in equal contiguous ranges (at most
// 32 each), so a tile of short pieces keeps every lane busy.
//
// The piece's minimum is an LDS atomicMin on a per-piece slot.  The slot costs
// no LDS of its own: it is rk[] of the piece's LAST position, which never
// holds a rank (a token starting there has no right neighbour in the piece,
// and nothing marks it: a merge marks its own left token and the token before
// it, both of which have a right neighbour).
//
// A round (all pieces of the tile advance together, each at its own rank):
//   A   every token start offers its rank to its piece's slot; no offer in the
//       whole wave (__any) ends the tile
//   B1  positions whose rank equals the slot are chosen; in an a == a run only
//       the run's first token (tok / sb are only read here)
//   B2  chosen positions merge: the left token takes the new id and EP_LOOK,
//       the right token's start bit goes, the token before gets EP_LOOK; an
//       a == a owner walks its run to its end or the piece's
//   C   slots are reset, marked pairs looked up (byte pairs: a direct table;
//       others: an open-addressing table in HBM, key and rank in one 8-byte load)
// The rounds of a tile are the largest merge count of its pieces.
//
// Output: the tile's ids, compacted, go to stage[] at the tile's first byte
// (tiles own disjoint byte ranges and a piece has no more ids than bytes);
// cnt[d] = ids of piece d.  The host scans cnt into the id offsets and
// k_ep_gather moves every tile's ids to their place.

namespace bpeamd {

constexpr uint32_t EP_T = 64;                      // one wave per tile
constexpr uint32_t EP_W = 2048;                    // LDS positions of a tile
constexpr uint32_t EP_C = 1024;                    // core: the tile owns the pieces starting in it
constexpr uint32_t EP_PIECE_MAX = EP_W - EP_C;     // bytes of the longest piece a tile takes
constexpr uint32_t EP_ID_BITS = 21;
constexpr uint32_t EP_MAX_IDS = 1u << EP_ID_BITS;  // ids (256 + merges) the packed table slot holds
constexpr uint32_t EP_LOOK = 0xFFFFFFFEu;          // rk: pair changed, look its rank up
constexpr uint32_t EP_NONE = 0xFFFFFFFFu;          //     no merge
static_assert(EP_W == EW_W, "ew_next / ew_prev scan EW_W / 32 bitmap words");
static_assert(EP_W / 32 == EP_T, "one bitmap word per lane in the output's prefix counts");
static_assert(EP_W <= 32 * EP_T, "a lane's range fits one 32-bit mask");
static_assert(EP_PIECE_MAX >= EP_C, "a piece too long for its tile is the last one the tile owns");

// control words (ctl); the last three are k_enc_long's (encode_long.hip): pieces it took, pieces beyond its limit,
// the largest round count of a piece
enum { EPC_LONG, EPC_ROUNDS, EPC_ERROR, EPC_LTAKEN, EPC_LOVER, EPC_LROUNDS, EPC_WORDS };

struct EncPieceArgs {
    const uint8_t *bytes;            // [n] (+ 64 bytes of slack)
    uint64_t n;
    const uint64_t *doc_off;         // [ndocs + 1] piece starts, doc_off[ndocs] == n
    uint32_t ndocs;
    uint32_t hmask;
    const uint32_t *bp;              // [65536] byte pair -> rank (EP_NONE: none)
    const unsigned long long *ht;    // a << 42 | b << 21 | rank + 1 (0: empty)
    uint32_t *stage;                 // [n] tile w's ids from its first owned byte on
    uint32_t *cnt;                   // [ndocs + 1] ids per piece (zeroed: empty, long and unowned pieces stay 0)
    uint32_t *tfirst, *tcnt;         // [tiles] the tile's first piece, its ids ([2 * tiles] with lng: a long piece each)
    uint32_t *ctl;                   // [EPC_WORDS] long pieces, largest round count, internal error
    uint32_t *lng;                   // [tiles] the long pieces left out, in any order (nullptr: only counted)
    uint32_t tiles;
    uint64_t thr, seed;              // dropout (encode_drop.hip): a pair is dropped iff its draw < thr; the rounds' seed
};

// the wave's own LDS stores and atomics are done before its next LDS loads
__device__ inline void ep_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// rank of the pair (x, y); EP_NONE when the list has no such merge
__device__ inline uint32_t ep_rank(const EncPieceArgs &A, uint32_t x, uint32_t y) {
    if ((x | y) < 256) return A.bp[(x << 8) | y];
    const uint64_t key = ((uint64_t)x << EP_ID_BITS) | y;
    uint32_t s = (uint32_t)mix64(key) & A.hmask;
    for (uint32_t k = 0; k <= A.hmask; k++) {  // (at most 1/4 full: an empty slot ends it long before)
        const unsigned long long e = A.ht[s];  // key and rank in ONE 8-byte load
        if (e == 0) return EP_NONE;
        if ((e >> EP_ID_BITS) == key) return (uint32_t)(e & (EP_MAX_IDS - 1)) - 1u;
        s = (s + 1) & A.hmask;
    }
    return EP_NONE;
}

// First d in [lo, hi] with off[d] >= x, given off[hi] >= x, by the whole wave:
// 64 probes per round trip, the span falls to under 1/63 of itself each time
// (6 rounds for 2^32 entries; the loop's bound is 8).
__device__ inline uint32_t ep_lower(const uint64_t *off, uint64_t lo, uint64_t hi, uint64_t x, uint32_t lane) {
    for (uint32_t it = 0; it < 8 && lo < hi; it++) {
        const uint64_t step = (hi - lo) / 63 + 1;  // (lane 63 probes hi)
        const uint64_t q = min(hi, lo + lane * step);
        const uint32_t f = (uint32_t)__builtin_ctzll(__ballot(off[q] >= x) | (1ull << 63));
        if (f == 0) break;
        hi = min(hi, lo + f * step);
        lo = lo + (f - 1) * step + 1;
    }
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)lo);
}

// bits [at, at + 32) of a bitmap (the arrays carry two words of padding)
__device__ inline uint32_t ep_bits(const uint32_t *bm, uint32_t at) {
    const uint64_t v = (uint64_t)bm[at >> 5] | ((uint64_t)bm[(at >> 5) + 1] << 32);
    return (uint32_t)(v >> (at & 31));
}

__global__ __launch_bounds__(EP_T) void k_enc_piece(EncPieceArgs A) {
    __shared__ __align__(16) uint32_t tok[EP_W];
    __shared__ __align__(16) uint32_t rk[EP_W];
    __shared__ uint32_t sb[EP_W / 32 + 2];  // token starts
    __shared__ uint32_t pb[EP_W / 32 + 2];  // piece starts; after the rounds: tokens before each word of sb
    const uint32_t lane = threadIdx.x;
    const uint64_t w = blockIdx.x;
    const uint64_t s0 = w * EP_C, s1 = min(A.n, s0 + EP_C);
    // the pieces starting in the core: [i0, i1)
    const uint32_t i0 = ep_lower(A.doc_off, 0, A.ndocs, s0, lane);
    const uint32_t i1 = ep_lower(A.doc_off, i0, A.ndocs, s1, lane);
    if (lane == 0) {
        A.tfirst[w] = i0;
        A.tcnt[w] = 0;
    }
    if (i0 == i1) return;  // no piece starts here
    const uint64_t L = A.doc_off[i0];
    uint64_t R = A.doc_off[i1];
    const bool lng = R - A.doc_off[i1 - 1] > EP_PIECE_MAX;  // only the last piece can be
    if (lng) {
        R = A.doc_off[i1 - 1];
        if (lane == 0) {
            const uint32_t s = atomicAdd(&A.ctl[EPC_LONG], 1u);  // (at most one a tile: s < tiles)
            if (A.lng) A.lng[s] = i1 - 1;
        }
    }
    if (R - L > EP_W) {  // (offsets that do not rise)
        if (lane == 0) atomicOr(&A.ctl[EPC_ERROR], 1u);
        return;
    }
    const uint32_t W = (uint32_t)(R - L);
    if (W == 0) return;
    // 16-byte loads from L rounded down, the bytes before L discarded (the buffer has 64 bytes of slack)
    {
        const uint32_t sh = (uint32_t)(L & 15u);
        const uint8_t *base = A.bytes + (L - sh);
        for (uint32_t t = lane; 16 * t < W + sh; t += EP_T) {
            typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
            const u32x4 v = __builtin_nontemporal_load((const u32x4 *)(base + 16 * (uint64_t)t));
            const uint32_t x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (uint32_t j = 0; j < 16; j++) {
                const uint32_t p = 16 * t + j - sh;  // (wraps for the bytes before L)
                if (p < W) tok[p] = (x[j >> 2] >> (8 * (j & 3))) & 0xFFu;
            }
        }
    }
    {
        const uint32_t b0 = lane * 32;
        sb[lane] = b0 + 32 <= W ? 0xFFFFFFFFu : b0 >= W ? 0u : (1u << (W - b0)) - 1u;
        pb[lane] = 0;
        if (lane < 2) sb[EP_W / 32 + lane] = pb[EP_W / 32 + lane] = 0;
    }
    ep_sync();
    for (uint64_t d = (uint64_t)i0 + lane; d < i1; d += EP_T) {  // (any number of them: empty pieces share a bit)
        const uint64_t p = A.doc_off[d] - L;
        if (p < W) atomicOr(&pb[p >> 5], 1u << (p & 31));
    }
    ep_sync();
    // this lane's positions [lo, hi), and the first piece start at or after hi
    const uint32_t per = (W + EP_T - 1) / EP_T;
    const uint32_t lo = min(W, lane * per), hi = min(W, lo + per);
    const uint32_t mask = hi - lo >= 32 ? 0xFFFFFFFFu : (1u << (hi - lo)) - 1u;
    const uint32_t pm = ep_bits(pb, lo) & mask;
    const uint32_t endhi = hi >= W ? W : min(W, ew_from(pb, hi));
    // the end of the piece that holds position lo + k
    auto pend = [&](uint32_t k) {
        const uint32_t above = (pm >> k) >> 1;
        return above ? lo + k + 1 + (uint32_t)__builtin_ctz(above) : endhi;
    };
    for (uint32_t p = lo; p < hi; p++)  // byte-pair ranks; none across a piece start
        rk[p] = p + 1 < W && !ew_is_start(pb, p + 1) ? A.bp[(tok[p] << 8) | tok[p + 1]] : EP_NONE;
    ep_sync();
    uint32_t rounds = 0;
    for (;;) {
        // A: the pieces' minima
        const uint32_t tm = ep_bits(sb, lo) & mask;
        bool any = false;
        for (uint32_t m = tm; m; m &= m - 1) {
            const uint32_t k = (uint32_t)__builtin_ctz(m), p = lo + k, pe = pend(k);
            if (p + 1 == pe) continue;  // (the slot itself)
            const uint32_t r = rk[p];
            if (r < EP_LOOK) {
                atomicMin(&rk[pe - 1], r);
                any = true;
            }
        }
        if (!__any(any)) break;
        if (++rounds > EP_W) {  // (a piece of k bytes merges at most k - 1 times)
            if (lane == 0) atomicOr(&A.ctl[EPC_ERROR], 2u);
            return;
        }
        ep_sync();
        // B1: who merges
        uint32_t mine = 0;
        for (uint32_t m = tm; m; m &= m - 1) {
            const uint32_t k = (uint32_t)__builtin_ctz(m), p = lo + k, pe = pend(k);
            if (p + 1 == pe) continue;
            const uint32_t r = rk[p];
            if (r >= EP_LOOK || r != rk[pe - 1]) continue;
            const uint32_t x = tok[p];
            // in an a == a run, its first token only (position 0 starts a piece)
            if (tok[ew_next(sb, p)] == x && !ew_is_start(pb, p) && tok[ew_prev(sb, p)] == x) continue;
            mine |= 1u << k;
        }
        ep_sync();
        // B2: merge
        for (uint32_t m = mine; m; m &= m - 1) {
            const uint32_t k = (uint32_t)__builtin_ctz(m), p = lo + k, pe = pend(k);
            const uint32_t x = tok[p], z = 256u + rk[p];
            if (!ew_is_start(pb, p)) rk[ew_prev(sb, p)] = EP_LOOK;  // its right neighbour changes
            uint32_t cur = p, q = ew_next(sb, p);  // the pair's right token (in p's piece: the pair has a rank)
            const bool run = tok[q] == x;
            for (uint32_t it = 0; it < EP_W / 2; it++) {  // (a pair per turn)
                tok[cur] = z;
                atomicAnd(&sb[q >> 5], ~(1u << (q & 31)));
                rk[cur] = EP_LOOK;
                if (!run) break;
                cur = ew_next(sb, cur);
                if (cur >= pe || tok[cur] != x) break;  // the run ends after a pair (or with its piece)
                q = ew_next(sb, cur);
                if (q >= pe || tok[q] != x) break;  // odd token out: its pair is as it was
            }
        }
        ep_sync();
        // C: reset the slots that lie in this lane's range, look the marked pairs up
        {
            uint32_t em = ep_bits(pb, lo + 1) & mask;
            if (hi == W && hi > lo) em |= 1u << (hi - lo - 1);
            for (; em; em &= em - 1) rk[lo + (uint32_t)__builtin_ctz(em)] = EP_NONE;
        }
        for (uint32_t m = ep_bits(sb, lo) & mask; m; m &= m - 1) {
            const uint32_t k = (uint32_t)__builtin_ctz(m), p = lo + k;
            if (rk[p] != EP_LOOK) continue;
            const uint32_t q = ew_next(sb, p);
            rk[p] = q < pend(k) ? ep_rank(A, tok[p], tok[q]) : EP_NONE;
        }
        ep_sync();
    }
    ep_sync();
    // tokens before each word of sb (into pb, which is done with), and the tile's total
    uint32_t total;
    {
        const uint32_t mc = (uint32_t)__builtin_popcount(sb[lane]);
        uint32_t inc = mc;
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t y = __shfl_up(inc, o);
            if ((int)lane >= o) inc += y;
        }
        pb[lane] = inc - mc;
        total = __shfl(inc, 63);
    }
    ep_sync();
    auto before = [&](uint32_t p) {  // tokens starting before position p
        return p >= W ? total : pb[p >> 5] + (uint32_t)__builtin_popcount(sb[p >> 5] & ((1u << (p & 31)) - 1u));
    };
    {
        uint32_t at = before(lo);  // compacted into rk, which is done with
        for (uint32_t m = ep_bits(sb, lo) & mask; m; m &= m - 1) rk[at++] = tok[lo + (uint32_t)__builtin_ctz(m)];
    }
    for (uint64_t d = (uint64_t)i0 + lane; d < i1 - (lng ? 1u : 0u); d += EP_T)
        A.cnt[d] = before((uint32_t)(A.doc_off[d + 1] - L)) - before((uint32_t)(A.doc_off[d] - L));
    ep_sync();
    for (uint32_t i = lane; i < total; i += EP_T) A.stage[L + i] = rk[i];
    if (lane == 0) {
        A.tcnt[w] = total;
        atomicMax(&A.ctl[EPC_ROUNDS], rounds);
    }
}

// The ids of tile w (staged at its first owned byte) to out + id_off[its first
// piece]: one wave per tile, the few ids before out's next 16-byte boundary
// one per lane, the rest four per lane as one 16-byte store, as k_ew_gather.
constexpr uint32_t EPG_T = 256;
__global__ __launch_bounds__(EPG_T) void k_ep_gather(const uint32_t *__restrict__ stage, const uint64_t *__restrict__ doc_off,
                                                     const uint64_t *__restrict__ id_off, const uint32_t *__restrict__ tfirst,
                                                     const uint32_t *__restrict__ tcnt, uint64_t tiles,
                                                     uint32_t *__restrict__ out) {
    const uint64_t w = (uint64_t)blockIdx.x * (EPG_T / 64) + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    if (w >= tiles) return;
    const uint32_t n = tcnt[w];
    if (!n) return;
    const uint32_t d = tfirst[w];
    const uint32_t *src = stage + doc_off[d];
    const uint64_t o = id_off[d];
    uint32_t *dst = out + o;
    const uint32_t h = min(n, (uint32_t)((4 - (o & 3)) & 3));  // ids before the boundary
    if (lane < h) dst[lane] = src[lane];
    const uint32_t nq = (n - h) / 4;
    for (uint32_t q = lane; q < nq; q += 64) {
        const uint32_t i = h + 4 * q;
        *reinterpret_cast<uint4 *>(dst + i) = make_uint4(src[i], src[i + 1], src[i + 2], src[i + 3]);
    }
    for (uint32_t i = h + 4 * nq + lane; i < n; i += 64) dst[i] = src[i];
}

}  // namespace bpeamd

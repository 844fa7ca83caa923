// encode_drop.hip -- the piece-local replay under BPE-dropout (Provilkov et al. 2020); included by engine.hip.
//
// The contract (bpe_gpu.h, "Dropout"): every piece is replayed on its own in
// rounds t = 0, 1, 2, ...  In round t every adjacent pair of live tokens that
// has a rank is a candidate, and each candidate is dropped or kept by a
// stateless draw on (seed, t, g), g the resident byte offset of the first byte
// of the pair's left token (ed_kept below).  A round with no kept candidate
// finishes the piece for good; otherwise the smallest rank among the KEPT
// candidates wins and all its kept occurrences merge left to right, an
// occurrence whose left token was just merged away being skipped.  Dropped
// winners stay and are drawn anew in round t + 1.
//
// encode_piece.hip and encode_long.hip rest on "the ranks a piece applies only
// rise".  A dropped pair of a low rank may be kept a round later, so here the
// winning ranks go up and down and nothing may be pruned by rank: these are
// kernels of their own.  What they keep: the geometry (one wave per tile of
// EP_W positions and EP_C core bytes; one workgroup of EL_T threads per listed
// long piece), the tables and ep_rank (a pair's rank does not depend on the
// draws, so a cached rank stays valid until a neighbour merges), EncPieceArgs,
// the ctl words and the (stage, cnt, tfirst, tcnt) output that ep_run scans and
// k_ep_gather places.  All pieces of a tile, and every long piece, start at
// round 0, so the round counter of the wave or workgroup IS the piece's t and
// the round's key k_t is uniform.
//
// k_enc_piece_drop, a round:
//   A   a lane draws once for every ranked token start of its range and keeps
//       the result as a 32-bit mask; only kept pairs are offered to the piece's
//       atomicMin slot (rk[] of the piece's last position, as in k_enc_piece).
//       A piece that is closed (below) offers nothing.  No offer in the whole
//       wave ends the tile: every piece is then finished.
//   B1  a ranked pair whose piece's slot is still EP_NONE had no kept candidate
//       in its piece: the slot takes EP_DONE, which closes the piece (phase A
//       skips it, phase C's reset respects it).  Chosen are the kept positions
//       whose rank equals the slot; of an a == a run only its first token,
//       and that one whether its own pair is kept or not.
//   B2  a chosen a != b pair merges.  An a == a owner walks its run: at each
//       position it takes the draw again (it is stateless), merges and steps
//       two tokens when the pair is kept, else steps one; the token before a
//       merged pair gets EP_LOOK.  The walk ends with the run or the piece
//       and is bounded by EP_W.
//   C   k_enc_piece's: slots reset (but for EP_DONE), marked pairs looked up.
// A round that is not the last merges at least one pair in some piece, so the
// rounds stay within EP_W; an overrun sets EPC_ERROR.
//
// k_enc_long_drop keeps its tokens compact, as k_enc_long does, and compaction
// loses a token's byte offset, which the draw needs.  A third array of u16
// would bring the workgroup to 164,032 B of LDS, 192 B beyond gfx950's 160 KiB,
// so the 14 offset bits ride in the spare bits of the two arrays there are:
//   tok[i] = id (21 bits) | (offset & 0x7FF) << 21
//   rk[i]  = kk << 3 | offset >> 11,   kk = rank << 1 | (a != b), ED_KLOOK, ED_KNONE
// LDS stays k_enc_long's 131,264 B and the limit EL_PIECE_MAX.  The rounds:
//   P1  as k_enc_long, then every own pair is drawn; the minimum runs over the
//       kept candidates only.  None kept (or none ranked) ends the piece.
//   P2  cm = (kk == key) & kept, for the own range and the two neighbours
//       (drawn from their own offsets); the stretch logic is k_enc_long's, now
//       over stretches of consecutive KEPT winners.
//   P3  k_enc_long's; a merged pair keeps its left token's offset.

namespace bpeamd {

constexpr uint32_t EP_DONE = 0xFFFFFFFDu;  // a piece's slot: the piece is finished (a round of it kept no candidate)
constexpr uint32_t ED_OFF_LO = 11;                            // offset bits in tok, above the id
constexpr uint32_t ED_OFF_HI = 3;                             //             in rk, below kk
constexpr uint32_t ED_KNONE = 0xFFFFFFFFu >> ED_OFF_HI;       // kk: no merge
constexpr uint32_t ED_KLOOK = ED_KNONE - 1;                   //     pair changed, look its rank up
static_assert(EP_ID_BITS + ED_OFF_LO <= 32, "id and low offset bits share a word");
static_assert((1u << (ED_OFF_LO + ED_OFF_HI)) >= EL_W, "the packed offset reaches every position of a long piece");
static_assert(((EP_MAX_IDS << 1) | 1u) < ED_KLOOK, "a rank key stays below the two marks");

// k_t: the key of round t
__device__ inline uint32_t ed_round_key(uint64_t seed, uint32_t t) {
    return (uint32_t)mix64(seed + 0x9E3779B97F4A7C15ull * ((uint64_t)t + 1));
}

// the draw of the pair whose left token starts at resident byte g, in the round of key kt: true = kept
__device__ inline bool ed_kept(uint32_t g, uint32_t kt, uint64_t thr) {
    uint32_t x = g ^ kt;
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return (uint64_t)x >= thr;
}

__global__ __launch_bounds__(EP_T) void k_enc_piece_drop(EncPieceArgs A) {
    __shared__ __align__(16) uint32_t tok[EP_W];
    __shared__ __align__(16) uint32_t rk[EP_W];
    __shared__ uint32_t sb[EP_W / 32 + 2];  // token starts
    __shared__ uint32_t pb[EP_W / 32 + 2];  // piece starts; after the rounds: tokens before each word of sb
    const uint32_t lane = threadIdx.x;
    const uint64_t w = blockIdx.x;
    const uint64_t s0 = w * EP_C, s1 = min(A.n, s0 + EP_C);
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
    for (uint64_t d = (uint64_t)i0 + lane; d < i1; d += EP_T) {
        const uint64_t p = A.doc_off[d] - L;
        if (p < W) atomicOr(&pb[p >> 5], 1u << (p & 31));
    }
    ep_sync();
    const uint32_t per = (W + EP_T - 1) / EP_T;
    const uint32_t lo = min(W, lane * per), hi = min(W, lo + per);
    const uint32_t mask = hi - lo >= 32 ? 0xFFFFFFFFu : (1u << (hi - lo)) - 1u;
    const uint32_t pm = ep_bits(pb, lo) & mask;
    const uint32_t endhi = hi >= W ? W : min(W, ew_from(pb, hi));
    auto pend = [&](uint32_t k) {
        const uint32_t above = (pm >> k) >> 1;
        return above ? lo + k + 1 + (uint32_t)__builtin_ctz(above) : endhi;
    };
    for (uint32_t p = lo; p < hi; p++)
        rk[p] = p + 1 < W && !ew_is_start(pb, p + 1) ? A.bp[(tok[p] << 8) | tok[p + 1]] : EP_NONE;
    ep_sync();
    const uint32_t g0 = (uint32_t)L;  // g of position p: g0 + p (a batch holds at most 2^32 - 2 bytes)
    uint32_t rounds = 0;
    for (;;) {
        const uint32_t kt = ed_round_key(A.seed, rounds);
        // A: draw; the pieces' minima over the kept pairs
        const uint32_t tm = ep_bits(sb, lo) & mask;
        uint32_t kept = 0;
        for (uint32_t m = tm; m; m &= m - 1) {
            const uint32_t k = (uint32_t)__builtin_ctz(m), p = lo + k, pe = pend(k);
            if (p + 1 == pe) continue;  // (the slot itself)
            const uint32_t r = rk[p];
            if (r >= EP_LOOK || rk[pe - 1] == EP_DONE) continue;  // (EP_DONE is never the target of an atomicMin)
            if (!ed_kept(g0 + p, kt, A.thr)) continue;
            atomicMin(&rk[pe - 1], r);
            kept |= 1u << k;
        }
        if (!__any(kept != 0)) break;  // no open piece kept a candidate: all are finished
        if (++rounds > EP_W) {         // (every round but a piece's last merges a pair of it)
            if (lane == 0) atomicOr(&A.ctl[EPC_ERROR], 2u);
            return;
        }
        ep_sync();
        // B1: close the pieces that kept nothing; who merges
        uint32_t mine = 0;
        for (uint32_t m = tm; m; m &= m - 1) {
            const uint32_t k = (uint32_t)__builtin_ctz(m), p = lo + k, pe = pend(k);
            if (p + 1 == pe) continue;
            const uint32_t r = rk[p];
            if (r >= EP_LOOK) continue;
            const uint32_t slot = rk[pe - 1];
            if (slot == EP_NONE) rk[pe - 1] = EP_DONE;  // ranked pairs and no offer (every writer stores the same)
            if (r != slot) continue;                    // (EP_NONE and EP_DONE equal no rank)
            const uint32_t x = tok[p];
            if (tok[ew_next(sb, p)] == x) {  // an a == a run: its first token, kept or not (position 0 starts a piece)
                if (!ew_is_start(pb, p) && tok[ew_prev(sb, p)] == x) continue;
            } else if (!((kept >> k) & 1u)) {
                continue;
            }
            mine |= 1u << k;
        }
        ep_sync();
        // B2: merge
        for (uint32_t m = mine; m; m &= m - 1) {
            const uint32_t k = (uint32_t)__builtin_ctz(m), p = lo + k, pe = pend(k);
            const uint32_t x = tok[p], z = 256u + rk[p];
            uint32_t prev = ew_is_start(pb, p) ? EP_NONE : ew_prev(sb, p);
            uint32_t cur = p, q = ew_next(sb, p);  // the pair's right token (in p's piece: the pair has a rank)
            if (tok[q] != x) {
                if (prev != EP_NONE) rk[prev] = EP_LOOK;  // its right neighbour changes
                tok[p] = z;
                atomicAnd(&sb[q >> 5], ~(1u << (q & 31)));
                rk[p] = EP_LOOK;
                continue;
            }
            for (uint32_t it = 0; it < EP_W; it++) {  // (a token or two per turn)
                if (!ed_kept(g0 + cur, kt, A.thr)) {  // dropped: the pair stays, the walk goes on from its right token
                    prev = cur;
                    cur = q;
                } else {
                    const uint32_t nx = ew_next(sb, q);
                    tok[cur] = z;
                    atomicAnd(&sb[q >> 5], ~(1u << (q & 31)));
                    rk[cur] = EP_LOOK;
                    if (prev != EP_NONE) rk[prev] = EP_LOOK;
                    prev = cur;
                    cur = nx;
                    if (cur >= pe || tok[cur] != x) break;  // the run ends after a pair (or with its piece)
                }
                q = ew_next(sb, cur);
                if (q >= pe || tok[q] != x) break;  // the run's last token: its pair is as it was
            }
        }
        ep_sync();
        // C: reset the open slots that lie in this lane's range, look the marked pairs up
        {
            uint32_t em = ep_bits(pb, lo + 1) & mask;
            if (hi == W && hi > lo) em |= 1u << (hi - lo - 1);
            for (; em; em &= em - 1) {
                const uint32_t s = lo + (uint32_t)__builtin_ctz(em);
                if (rk[s] != EP_DONE) rk[s] = EP_NONE;
            }
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
    // the output, as k_enc_piece leaves it
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

constexpr uint32_t ED_ID_MASK = EP_MAX_IDS - 1;
constexpr uint32_t ED_LO_MASK = (1u << ED_OFF_LO) - 1;
constexpr uint32_t ED_HI_MASK = (1u << ED_OFF_HI) - 1;

// the byte offset in its piece that the words (tok, rk) of a token carry
__device__ inline uint32_t ed_off(uint32_t t, uint32_t r) { return (t >> EP_ID_BITS) | ((r & ED_HI_MASK) << ED_OFF_LO); }

__global__ __launch_bounds__(EL_T) void k_enc_long_drop(EncPieceArgs A) {
    __shared__ uint32_t tok[EL_W];
    __shared__ uint32_t rk[EL_W];
    __shared__ uint32_t wmin[EL_WAVES];
    __shared__ uint32_t wsum[EL_WAVES];
    __shared__ int32_t whead[EL_WAVES];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t nl = min(A.ctl[EPC_LONG], A.tiles);  // (k_enc_piece_drop is done: the same for every workgroup and thread)
    for (uint32_t s = blockIdx.x; s < nl; s += gridDim.x) {
        const uint32_t d = A.lng[s];
        const uint64_t L = A.doc_off[d], len = A.doc_off[d + 1] - L;
        if (tid == 0) A.tfirst[A.tiles + s] = d;
        if (len > EL_PIECE_MAX) {  // (the whole workgroup skips it; the host encodes it without dropout)
            if (tid == 0) atomicAdd(&A.ctl[EPC_LOVER], 1u);
            continue;
        }
        for (uint32_t p = tid; p < (uint32_t)len; p += EL_T) {
            tok[p] = (uint32_t)A.bytes[L + p] | ((p & ED_LO_MASK) << EP_ID_BITS);
            rk[p] = (ED_KLOOK << ED_OFF_HI) | (p >> ED_OFF_LO);
        }
        __syncthreads();
        const uint32_t g0 = (uint32_t)L;
        uint32_t n = (uint32_t)len, rounds = 0;
        bool bad = false;
        for (;;) {
            const uint32_t kt = ed_round_key(A.seed, rounds);
            const uint32_t per = (n + EL_T - 1) / EL_T;
            const uint32_t lo = min(n, tid * per), hi = min(n, lo + per), mine = hi - lo;
            // P1: look up, load, draw, the minimum of the kept
            for (uint32_t p = lo; p < hi; p++) {
                const uint32_t r = rk[p];
                if ((r >> ED_OFF_HI) != ED_KLOOK) continue;
                uint32_t kk = ED_KNONE;
                if (p + 1 < n) {
                    const uint32_t x = tok[p] & ED_ID_MASK, y = tok[p + 1] & ED_ID_MASK;
                    kk = min(el_key(ep_rank(A, x, y), x, y), ED_KNONE);  // (EP_NONE -> ED_KNONE)
                }
                rk[p] = (kk << ED_OFF_HI) | (r & ED_HI_MASK);
            }
            uint32_t t_[EL_PER], r_[EL_PER], mn = ED_KNONE, kept = 0;
#pragma unroll
            for (uint32_t k = 0; k < EL_PER; k++) {
                const bool in = k < mine;
                t_[k] = in ? tok[lo + k] : 0u;
                r_[k] = in ? rk[lo + k] : 0xFFFFFFFFu;
                const uint32_t kk = r_[k] >> ED_OFF_HI;
                if (kk < ED_KLOOK && ed_kept(g0 + ed_off(t_[k], r_[k]), kt, A.thr)) {
                    kept |= 1u << k;
                    mn = min(mn, kk);
                }
            }
            for (int o = 32; o; o >>= 1) mn = min(mn, (uint32_t)__shfl_xor((int)mn, o));
            if (lane == 0) wmin[wave] = mn;
            __syncthreads();  // 1
            uint32_t key = wmin[lane & 15];
            for (int o = 8; o; o >>= 1) key = min(key, (uint32_t)__shfl_xor((int)key, o));
            key = (uint32_t)__builtin_amdgcn_readfirstlane((int)key);
            if (key >= ED_KLOOK) break;  // no kept candidate: the piece is finished
            if (++rounds > EL_W) {       // (every round but the last merges a pair)
                bad = true;
                break;
            }
            // P2: who merges: the kept winners
            uint32_t cm = 0;
#pragma unroll
            for (uint32_t k = 0; k < EL_PER; k++) cm |= (r_[k] >> ED_OFF_HI) == key ? 1u << k : 0u;
            cm &= kept;
            bool cprev = false, cnext = false;
            if (mine && lo > 0) {
                const uint32_t r = rk[lo - 1];
                cprev = (r >> ED_OFF_HI) == key && ed_kept(g0 + ed_off(tok[lo - 1], r), kt, A.thr);
            }
            if (mine && hi < n) {
                const uint32_t r = rk[hi];
                cnext = (r >> ED_OFF_HI) == key && ed_kept(g0 + ed_off(tok[hi], r), kt, A.thr);
            }
            uint32_t ch = cm;
            bool chprev = cprev;
            if (!(key & 1u)) {  // an a == a pair: in a stretch of kept winners, those at an even distance from its head
                const uint32_t hm = cm & ~((cm << 1) | (cprev ? 1u : 0u));
                int32_t inc = hm ? (int32_t)(lo + 31u - (uint32_t)__builtin_clz(hm)) : -1;
                for (int o = 1; o < 64; o <<= 1) {
                    const int32_t y = __shfl_up(inc, o);
                    if ((int)lane >= o) inc = max(inc, y);
                }
                if (lane == 63) whead[wave] = inc;
                int32_t carry = __shfl_up(inc, 1);  // the last head before this thread's range
                if (lane == 0) carry = -1;
                __syncthreads();  // 2
                int32_t wv = (lane & 15) < wave ? whead[lane & 15] : -1;
                for (int o = 8; o; o >>= 1) wv = max(wv, __shfl_xor(wv, o));
                carry = max(carry, wv);
                ch = 0;
                int32_t cur = carry;
                for (uint32_t m = cm; m; m &= m - 1) {
                    const uint32_t k = (uint32_t)__builtin_ctz(m);
                    if ((hm >> k) & 1u) cur = (int32_t)(lo + k);
                    if (!((lo + k - (uint32_t)cur) & 1u)) ch |= 1u << k;
                }
                chprev = cprev && !((lo - 1u - (uint32_t)carry) & 1u);  // (cprev: a head lies at or before lo - 1)
            }
            // P3: close the gaps
            const uint32_t keep = ((1u << mine) - 1u) & ~((ch << 1) | (chprev ? 1u : 0u));
            const uint32_t look = ch | (cm >> 1) | (cnext ? 1u << ((mine - 1u) & 31u) : 0u);  // merged, or the right neighbour merges
            const uint32_t kc = (uint32_t)__builtin_popcount(keep);
            uint32_t at = kc;
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t y = (uint32_t)__shfl_up((int)at, o);
                if ((int)lane >= o) at += y;
            }
            if (lane == 63) wsum[wave] = at;
            at -= kc;
            __syncthreads();  // 3
            uint32_t tot = wsum[lane & 15], bef = (lane & 15) < wave ? tot : 0u;
            for (int o = 8; o; o >>= 1) {
                tot += (uint32_t)__shfl_xor((int)tot, o);
                bef += (uint32_t)__shfl_xor((int)bef, o);
            }
            at += bef;
            const uint32_t z = 256u + (key >> 1);
#pragma unroll
            for (uint32_t k = 0; k < EL_PER; k++) {
                if (!((keep >> k) & 1u)) continue;
                tok[at] = (ch >> k) & 1u ? (t_[k] & ~ED_ID_MASK) | z : t_[k];  // (the left token's offset stays)
                rk[at] = (look >> k) & 1u ? (ED_KLOOK << ED_OFF_HI) | (r_[k] & ED_HI_MASK) : r_[k];
                at++;
            }
            n = (uint32_t)__builtin_amdgcn_readfirstlane((int)tot);
            __syncthreads();  // 4
        }
        if (bad) {
            if (tid == 0) atomicOr(&A.ctl[EPC_ERROR], 4u);
        } else {
            for (uint32_t i = tid; i < n; i += EL_T) A.stage[L + i] = tok[i] & ED_ID_MASK;
            if (tid == 0) {
                A.cnt[d] = n;
                A.tcnt[A.tiles + s] = n;
                atomicAdd(&A.ctl[EPC_LTAKEN], 1u);
                atomicMax(&A.ctl[EPC_LROUNDS], rounds);
            }
        }
        __syncthreads();  // tok[] is read above and loaded anew by the next piece
    }
}

}  // namespace bpeamd

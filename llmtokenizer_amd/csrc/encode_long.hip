// encode_long.hip -- the piece-local replay for ONE LONG PIECE per workgroup; included by engine.hip.
//
// k_enc_piece (encode_piece.hip) leaves out a piece of more than EP_PIECE_MAX
// bytes.  Under BPE_ENC_PIECE_LONG it also appends the piece's index to a list,
// and k_enc_long, launched behind it on the same stream, replays every listed
// piece of at most EL_PIECE_MAX bytes: one workgroup of EL_T threads per piece,
// the whole piece resident in LDS.  A longer one is counted and left to the
// per-document fallback (engine.hip).
//
// The replay is encode_piece.hip's: take the smallest rank among the piece's
// adjacent pairs, merge all its occurrences left to right, look the changed
// pairs up, repeat; the same tables (ep_table), the same ep_rank, and the same
// argument (a merge of rank r creates only pairs of rank above r).  What
// differs, with one piece per workgroup:
//   - The winning rank is ONE value: a wave minimum, sixteen LDS words and a
//     barrier, not a slot per piece.
//   - The tokens are kept COMPACT: tok[0, n) are the piece's n live tokens and
//     rk[i] belongs to the pair (tok[i], tok[i + 1]).  Every round closes the
//     gaps its merges left (a workgroup prefix count of the tokens that stay),
//     so there are no start bitmaps, a token's neighbours are i - 1 and i + 1,
//     a token's ordinal is its index, the n live tokens are dealt anew to the
//     threads in equal contiguous ranges each round (late rounds of few tokens
//     stay balanced), and at the end tok[] is the output.
//   - rk holds rank << 1 | (a != b), so the round's minimum also tells every
//     thread whether the winning pair is an a == a pair: a uniform branch.
//   - a == a runs have no walking lane.  The positions whose rank is the
//     winner form stretches of consecutive positions (the pairs inside a run
//     of a); the pairs taken are those at an even distance from their
//     stretch's first position.  The first position of the stretch that holds
//     position i is the largest stretch head at or before i: a max-scan of
//     the heads over the workgroup (in a wave by shuffles, across waves
//     through sixteen LDS words).  When a != b no two winners are adjacent
//     and all of them merge; the scan and its barrier are skipped.
//
// A round of n live tokens, thread t owning [lo, hi) of [0, n):
//   P1  pairs marked EP_LOOK in the own range are looked up (ep_rank) and
//       written back; the own tokens and ranks go to registers (EL_PER each);
//       the minimum: wave, wmin[], BARRIER 1, all waves read the 16 words.
//       No rank left ends the piece.
//   P2  winners of the own range and of its two neighbours (rk[lo - 1], rk[hi]);
//       for an a == a winner the stretch heads' max-scan (BARRIER 2, these
//       rounds only) decides which winners merge
//   P3  the tokens that stay (all but the right token of a merged pair) are
//       counted, prefix-summed over the workgroup (wsum[], BARRIER 3: every
//       read of the old arrays is done) and written to their new places from
//       the registers: a merged pair's left token as 256 + rank with EP_LOOK,
//       the token before a merged pair with EP_LOOK; BARRIER 4.
// Three barriers a round, four in a round of an a == a pair.  No loop depends
// on the piece's or a run's length beyond the thread's own share (at most
// EL_PER positions); the rounds are at most the piece's bytes (bounded by
// EL_W: an overrun sets EPC_ERROR), a probe chain by the table (ep_rank).
//
// Output, in the form k_enc_piece leaves: the piece's ids at stage[] from the
// piece's first byte, cnt[d] their number, and one more (tfirst, tcnt) entry
// behind the tiles' (entry tiles + s for list slot s; unused entries keep
// tcnt 0), so that the scan of cnt and k_ep_gather place them.  The ranges of
// stage[] stay disjoint: a tile stages at most as many ids as it loaded bytes,
// from its first owned piece's first byte, and it loads up to the START of
// the long piece it leaves out; no piece starts inside another, so no tile
// stages into [doc_off[d], doc_off[d + 1]) of a long piece d, and two long
// pieces do not overlap.

namespace bpeamd {

constexpr uint32_t EL_T = 1024;              // threads of the workgroup (16 waves)
constexpr uint32_t EL_WAVES = EL_T / 64;
constexpr uint32_t EL_W = 16384;             // LDS positions
constexpr uint32_t EL_PER = EL_W / EL_T;     // positions a thread owns at most
constexpr uint32_t EL_PIECE_MAX = EL_W;      // bytes of the longest piece the kernel takes
constexpr uint32_t EL_GRID = 256;            // workgroups at most (one fits a CU: 128 KiB of LDS); they stride the list
static_assert(EL_WAVES == 16, "the cross-wave steps read one word per (lane & 15)");
static_assert(EL_PER <= 31, "a thread's range fits one 32-bit mask with a bit to spare");
static_assert(EL_PIECE_MAX > EP_PIECE_MAX, "the list holds pieces the tiles left out");

// rk's value for the pair (x, y) of rank r: the rank, then whether the two differ
__device__ inline uint32_t el_key(uint32_t r, uint32_t x, uint32_t y) { return r == EP_NONE ? EP_NONE : (r << 1) | (x != y ? 1u : 0u); }

__global__ __launch_bounds__(EL_T) void k_enc_long(EncPieceArgs A) {
    __shared__ uint32_t tok[EL_W];
    __shared__ uint32_t rk[EL_W];
    __shared__ uint32_t wmin[EL_WAVES];
    __shared__ uint32_t wsum[EL_WAVES];
    __shared__ int32_t whead[EL_WAVES];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t nl = min(A.ctl[EPC_LONG], A.tiles);  // (k_enc_piece is done: the same for every workgroup and thread)
    for (uint32_t s = blockIdx.x; s < nl; s += gridDim.x) {
        const uint32_t d = A.lng[s];
        const uint64_t L = A.doc_off[d], len = A.doc_off[d + 1] - L;
        if (tid == 0) A.tfirst[A.tiles + s] = d;
        if (len > EL_PIECE_MAX) {  // (the whole workgroup skips it)
            if (tid == 0) atomicAdd(&A.ctl[EPC_LOVER], 1u);
            continue;
        }
        for (uint32_t p = tid; p < (uint32_t)len; p += EL_T) {
            tok[p] = A.bytes[L + p];
            rk[p] = EP_LOOK;
        }
        __syncthreads();
        uint32_t n = (uint32_t)len, rounds = 0;
        bool bad = false;
        for (;;) {
            const uint32_t per = (n + EL_T - 1) / EL_T;
            const uint32_t lo = min(n, tid * per), hi = min(n, lo + per), mine = hi - lo;
            // P1: look up, load, the minimum
            for (uint32_t p = lo; p < hi; p++) {
                if (rk[p] != EP_LOOK) continue;
                const uint32_t x = tok[p], y = p + 1 < n ? tok[p + 1] : 0u;
                rk[p] = p + 1 < n ? el_key(ep_rank(A, x, y), x, y) : EP_NONE;
            }
            uint32_t t_[EL_PER], r_[EL_PER], mn = EP_NONE;
#pragma unroll
            for (uint32_t k = 0; k < EL_PER; k++) {
                const bool in = k < mine;
                t_[k] = in ? tok[lo + k] : 0u;
                r_[k] = in ? rk[lo + k] : EP_NONE;
                mn = min(mn, r_[k]);
            }
            for (int o = 32; o; o >>= 1) mn = min(mn, (uint32_t)__shfl_xor((int)mn, o));
            if (lane == 0) wmin[wave] = mn;
            __syncthreads();  // 1
            uint32_t key = wmin[lane & 15];
            for (int o = 8; o; o >>= 1) key = min(key, (uint32_t)__shfl_xor((int)key, o));
            key = (uint32_t)__builtin_amdgcn_readfirstlane((int)key);
            if (key >= EP_LOOK) break;  // no pair has a rank: done
            if (++rounds > EL_W) {      // (a piece of k bytes merges at most k - 1 times)
                bad = true;
                break;
            }
            // P2: who merges
            uint32_t cm = 0;
#pragma unroll
            for (uint32_t k = 0; k < EL_PER; k++) cm |= r_[k] == key ? 1u << k : 0u;
            const bool cprev = mine && lo > 0 && rk[lo - 1] == key;
            const bool cnext = mine && hi < n && rk[hi] == key;
            uint32_t ch = cm;
            bool chprev = cprev;
            if (!(key & 1u)) {  // an a == a pair: in a stretch of winners, those at an even distance from its head
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
                tok[at] = (ch >> k) & 1u ? z : t_[k];
                rk[at] = (look >> k) & 1u ? EP_LOOK : r_[k];
                at++;
            }
            n = (uint32_t)__builtin_amdgcn_readfirstlane((int)tot);
            __syncthreads();  // 4
        }
        if (bad) {
            if (tid == 0) atomicOr(&A.ctl[EPC_ERROR], 4u);
        } else {
            for (uint32_t i = tid; i < n; i += EL_T) A.stage[L + i] = tok[i];
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

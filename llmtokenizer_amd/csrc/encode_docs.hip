// encode_docs.hip -- window-local encoder over a BATCH OF DOCUMENTS; included by engine.hip.
//
// The bytes are the documents concatenated, doc d = bytes[off[d], off[d + 1]);
// no merge crosses a document start.  The machinery is encode_win.hip's (its
// plan image, rank cache, start bitmap, certain range [Lu, Ru), u16 staging
// and k_ew_gather); the differences are the boundaries:
//   * windows tile the concatenated stream in cores as there, but a window is
//     CLIPPED at the last document start <= its core's first byte and at the
//     first one >= its core's end (ed_geom).  A clipped side has no halo and
//     needs none: the neighbour there is known to be absent, so the window
//     starts out certain on that side (lunk / runk false);
//   * document starts inside the window are a second bitmap (db).  A pair
//     whose right token starts a document has no rank, ever (the byte-pair
//     ranks and ed_relook), so no merge and no a == a run crosses one: the run
//     pre-pass keeps a token that starts a document (its run begins there) and
//     the run walk stops in front of one;
//   * an edge of the certain range that sits on a document start has a known
//     (absent) neighbour: the edge token is certain whatever its id, so Lu
//     never moves past a document start and Ru never has to back off one.
// With these, a token is certain under exactly the rules of encode_win.hip:
// every argument there is about pairs of adjacent tokens, and a document start
// only removes pairs.
//
// Per document starting in the core the kernel stores the number of core
// tokens before it; k_ed_offsets adds the window's offset from the count scan
// (id_off[d]).  A window whose core came out uncertain is recorded in wfail[]:
// the host encodes the documents touching it one by one (engine.hip).

namespace bpeamd {

static_assert(EW_W / 32 == 64, "k_enc_docs scans the start bitmap's words with one wave");

struct EncDocArgs {
    EncWinArgs w;             // bytes, n, core, halo, nwin, the plan's tables, stage, cnt, ticket;
                              // lh / rh / lav / rav / lmore / rmore unused; *fail counts the failed windows
    const uint64_t *doc_off;  // [ndocs + 1] document starts (doc_off[ndocs] == n)
    const uint32_t *wfirst;   // [nwin + 1] first document with doc_off >= min(n, w * core) (k_ed_first)
    uint32_t *rel;            // [ndocs + 1] core tokens before the document's start, in its window
    uint32_t *wfail;          // [nwin] the window's core was not certain
};

// first index d in [0, ndocs] with off[d] >= x (ndocs + 1: none)
__host__ __device__ inline uint64_t ed_lower(const uint64_t *off, uint64_t ndocs, uint64_t x) {
    uint64_t lo = 0, hi = ndocs + 1;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (off[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// Window w = bytes [L, R) around the core [s0, s1): clipped at the last
// document start <= s0 and the first one >= s1 (off[ndocs] == n counts as
// one).  i0 / i1 = ed_lower of s0 / s1.  lunk / runk: the byte before L / at R
// belongs to the same document (the neighbour there exists and is unknown).
struct EdGeom {
    uint64_t L, R;
    uint32_t lunk, runk;
};
__host__ __device__ inline EdGeom ed_geom(const uint64_t *off, uint64_t n, uint32_t core, uint32_t halo, uint64_t w,
                                          uint64_t i0, uint64_t i1) {
    const uint64_t s0 = w * core, s1 = n < s0 + core ? n : s0 + core;
    const uint64_t dl = off[i0] == s0 ? s0 : off[i0 - 1];  // (off[0] == 0 <= s0: i0 >= 1 here)
    const uint64_t dr = off[i1];                            // (off[ndocs] == n >= s1)
    const uint64_t hl = s0 > halo ? s0 - halo : 0, hr = s1 + halo;
    EdGeom G;
    G.L = hl > dl ? hl : dl;
    G.R = hr < dr ? hr : dr;
    G.lunk = G.L != dl;  // (no document starts in (dl, s0])
    G.runk = G.R != dr;
    return G;
}

// the first document of every window (and of the end): one binary search per
// window here instead of one per workgroup in k_enc_docs
__global__ void k_ed_first(const uint64_t *__restrict__ off, uint64_t ndocs, uint64_t n, uint32_t core, uint64_t nwin,
                           uint32_t *__restrict__ wfirst) {
    const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w > nwin) return;
    const uint64_t s = w * core;
    wfirst[w] = (uint32_t)ed_lower(off, ndocs, s < n ? s : n);
}

// id_off[d] = ids before document d: its window's offset plus the core tokens
// before it there; a document starting at n (trailing empty ones, and d == ndocs) gets the total
__global__ void k_ed_offsets(const uint64_t *__restrict__ off, uint64_t ndocs, uint64_t n, uint32_t core,
                             const unsigned long long *__restrict__ win_off, uint64_t nwin,
                             const uint32_t *__restrict__ rel, uint64_t *__restrict__ id_off) {
    const uint64_t d = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (d > ndocs) return;
    const uint64_t o = off[d];
    id_off[d] = o >= n ? win_off[nwin] : win_off[o / core] + rel[d];
}

// out[d] = src[idx[d]] (bpe_gpu_decode_docs: byte offsets from the ids' prefix sum)
__global__ void k_ed_pick(const uint64_t *__restrict__ src, const uint64_t *__restrict__ idx, uint64_t count,
                          uint64_t *__restrict__ out) {
    const uint64_t d = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (d < count) out[d] = src[idx[d]];
}

__device__ inline bool ed_doc(const uint32_t *db, uint32_t p) { return (db[p >> 5] >> (p & 31)) & 1u; }

// bits [lo, hi) of the bitmap word that starts at position w32
__device__ inline uint32_t ed_span(uint32_t w32, uint32_t lo, uint32_t hi) {
    uint32_t m = ~0u;
    if (lo > w32) m &= lo - w32 >= 32 ? 0u : ~0u << (lo - w32);
    if (hi < w32 + 32) m &= hi <= w32 ? 0u : (1u << (hi - w32)) - 1u;
    return m;
}

// ew_relook with the boundary rule: no rank when the right token starts a document
__device__ inline void ed_relook(const EncWinArgs &A, const uint16_t *tok, uint16_t *rk, const uint32_t *sb,
                                 const uint32_t *db, uint32_t p, uint32_t W) {
    uint32_t r = ~0u;
    if (ew_is_start(sb, p)) {
        const uint32_t q = ew_next(sb, p);
        if (q < W && !ed_doc(db, q)) r = ew_info(A, tok[p], tok[q]);
    }
    rk[p] = (uint16_t)r;
}

__global__ __launch_bounds__(EW_T) __attribute__((amdgpu_waves_per_eu(EW_WAVES, 8))) void k_enc_docs(EncDocArgs D) {
    const EncWinArgs &A = D.w;
    __shared__ __align__(16) uint16_t tok[EW_W];
    __shared__ __align__(16) uint16_t rk[EW_W];
    __shared__ uint32_t sb[EW_W / 32];
    __shared__ uint32_t db[EW_W / 32];  // document starts (position 0 too when L is one)
    __shared__ __align__(16) uint16_t s_pend[EW_PENDCAP];
    __shared__ uint32_t s_win, s_Lu, s_Ru, s_runend, s_npend;
    __shared__ uint32_t s_lid, s_rid, s_lm[8], s_rm[8], s_lact, s_ract, s_tpos;
    __shared__ uint32_t s_wcnt[EW_T / 64];
    static_assert(EW_PENDCAP * 2 >= EW_W / 32 * 4, "s_pend holds the bitmap words' prefix counts after the batches");
    const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const uint32_t p0 = tid * EW_PER;
    uint16_t *myrk = rk + p0;
    uint32_t *tok32 = (uint32_t *)tok;
    for (uint32_t k = tid; k < EW_W / 32; k += EW_T) db[k] = 0;  // (each window clears it again when done)
    for (;;) {
        if (tid == 0) s_win = atomicAdd(A.ticket, 1u);
        __syncthreads();
        const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_win);
        if (w >= A.nwin) return;
        unsigned long long tp0 = EW_PROF_ON ? wall_clock64() : 0, nhas = 0, tpa = 0, tpb = 0, tq = 0;
        // geometry: block-uniform, from the pre-pass's first documents (three loads of doc_off)
        const uint64_t s0 = (uint64_t)w * A.core, s1 = min(A.n, s0 + A.core);
        const uint32_t i0 = D.wfirst[w], i1 = D.wfirst[w + 1];  // documents starting in the core: [i0, i1)
        const EdGeom G = ed_geom(D.doc_off, A.n, A.core, A.halo, w, i0, i1);
        const uint32_t L = (uint32_t)G.L, W = (uint32_t)(G.R - G.L);
        const bool lunk = G.lunk != 0, runk = G.runk != 0;
        // 16-byte loads from L rounded down, the front discarded (a clipped
        // window's L is rarely aligned; the buffer has 64 bytes of slack)
        {
            const uint32_t sh = L & 15u, ks = sh >> 2, bs = 8 * (sh & 3u);
            const uint8_t *base = A.bytes + (L - sh);
            for (uint32_t t = tid; t * 16 < W; t += EW_T) {
                typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
                const u32x4 q = __builtin_nontemporal_load((const u32x4 *)(base + 16 * (uint64_t)t));
                uint32_t x[4] = {q.x, q.y, q.z, q.w};
                if (sh) {
                    const u32x4 q2 = __builtin_nontemporal_load((const u32x4 *)(base + 16 * (uint64_t)t + 16));
                    const uint32_t z[8] = {q.x, q.y, q.z, q.w, q2.x, q2.y, q2.z, q2.w};
                    uint32_t a[5];
#pragma unroll
                    for (uint32_t j = 0; j < 5; j++) a[j] = ks == 0 ? z[j] : ks == 1 ? z[j + 1] : ks == 2 ? z[j + 2] : z[j + 3];
#pragma unroll
                    for (uint32_t j = 0; j < 4; j++) x[j] = (uint32_t)((((uint64_t)a[j + 1] << 32) | a[j]) >> bs);
                }
#pragma unroll
                for (uint32_t j = 0; j < 4; j++) {
                    tok32[8 * t + 2 * j] = (x[j] & 0xFFu) | ((x[j] << 8) & 0xFF0000u);
                    tok32[8 * t + 2 * j + 1] = ((x[j] >> 16) & 0xFFu) | ((x[j] >> 8) & 0xFF0000u);
                }
            }
        }
        for (uint32_t k = tid; k < EW_W / 32; k += EW_T) {
            const uint32_t lo = k * 32;
            sb[k] = lo + 32 <= W ? 0xFFFFFFFFu : lo >= W ? 0u : (1u << (W - lo)) - 1u;
        }
        // the documents starting in the core (any number of them: 1-byte and empty ones)
        for (uint64_t d = (uint64_t)i0 + tid; d < i1; d += EW_T) {
            const uint32_t p = (uint32_t)(D.doc_off[d] - G.L);
            if (p < EW_W) atomicOr(&db[p >> 5], 1u << (p & 31));
        }
        if (tid == 0) {
            s_Lu = 0;
            s_Ru = W;
            s_runend = 0;
            s_npend = 0;
            s_lid = s_rid = EW_NOPOS;
        }
        __syncthreads();
        // byte-pair ranks: independent lookups, 8 at a time; none for a pair
        // whose right byte starts a document (dmk bit k: position p0 + k + 1 does)
        {
            const uint32_t wd = p0 >> 5;
            const uint64_t v = (uint64_t)db[wd] | ((uint64_t)(wd + 1 < EW_W / 32 ? db[wd + 1] : 0u) << 32);
            const uint32_t dmk = (uint32_t)(v >> ((p0 & 31) + 1)) & 0xFFFFu;
#pragma unroll
            for (uint32_t h = 0; h < EW_PER; h += 8) {
                uint32_t r[8];
#pragma unroll
                for (uint32_t k = 0; k < 8; k++) {
                    const uint32_t p = p0 + h + k;
                    r[k] = p + 1 < W && !((dmk >> (h + k)) & 1u) ? A.bp[((uint32_t)tok[p] << 8) | tok[p + 1]] : ~0u;
                }
                *(uint4 *)(myrk + h) = make_uint4((r[0] & 0xFFFFu) | (r[1] << 16), (r[2] & 0xFFFFu) | (r[3] << 16),
                                                  (r[4] & 0xFFFFu) | (r[5] << 16), (r[6] & 0xFFFFu) | (r[7] << 16));
            }
        }
        // Edge snapshot as in k_enc_win; an edge on a document start is not
        // active: its neighbour on that side is known to be absent.
        auto snapshot = [&](uint32_t Lu, uint32_t Ru) {
            s_lact = Lu < Ru && (lunk || Lu > 0) && !ed_doc(db, Lu);
            if (s_lact && tok[Lu] != s_lid) {
                s_lid = tok[Lu];
                ew_mask(A, s_lid, 1, s_lm);
            }
            s_ract = 0;
            if (Ru > Lu && (Ru < W ? !ed_doc(db, Ru) : runk)) {
                const uint32_t tp = ew_prev(sb, Ru);
                if (tp != EW_NOPOS) {
                    s_ract = 1;
                    s_tpos = tp;
                    if (tok[tp] != s_rid) {
                        s_rid = tok[tp];
                        ew_mask(A, s_rid, 0, s_rm);
                    }
                }
            }
        };
        if (tid == EW_EDGE_T) snapshot(0, W);  // (tok and db are complete: the init barrier)
        unsigned long long tp1 = EW_PROF_ON ? wall_clock64() : 0;
        for (uint32_t b = 0; b < A.nb; b++) {
            const uint32_t r0 = A.bstart[b], r1 = A.bstart[b + 1];
            uint4 va = ((const uint4 *)myrk)[0], vc = ((const uint4 *)myrk)[1];
            uint32_t mine = ew_in(va, vc, r0, r1);
            const bool has = __syncthreads_or(mine != 0);
            const uint32_t Lu = s_Lu, Ru = s_Ru;
            bool lmove = false, rmove = false;
            if (tid == EW_EDGE_T) {
                lmove = s_lact && ((s_lm[b >> 5] >> (b & 31)) & 1u);
                rmove = s_ract && ((s_rm[b >> 5] >> (b & 31)) & 1u);
            }
            if (!has) {
                if (tid == EW_EDGE_T && (lmove || rmove)) {  // (no thread writes tok / sb in this batch)
                    const uint32_t lu = lmove ? ew_next(sb, Lu) : Lu, ru = rmove ? s_tpos : Ru;
                    s_Lu = lu;
                    s_Ru = ru;
                    snapshot(lu, ru);
                }
                continue;  // the next batch's barrier orders these stores
            }
            nhas++;
            if (EW_PROF_ON) tq = wall_clock64();
            if (A.beq[b]) {  // (block-uniform: the barrier inside is reached by every thread or none)
                // a == a runs: a run's tokens after its first drop out of the
                // scan; a token that starts a document is a run's first
                for (uint32_t m = mine; m; m &= m - 1) {
                    const uint32_t k = (uint32_t)__builtin_ctz(m), p = p0 + k;
                    const uint32_t x = tok[p];
                    if (tok[ew_next(sb, p)] != x) continue;
                    const uint32_t lp = ew_prev(sb, p);
                    if (lp != EW_NOPOS && tok[lp] == x && !ed_doc(db, p)) {
                        myrk[k] = EW_NONE;
                        mine &= ~(1u << k);
                    }
                }
                __syncthreads();
            }
            for (uint32_t m = mine; m; m &= m - 1) {
                const uint32_t p = p0 + (uint32_t)__builtin_ctz(m);
                const uint32_t x = tok[p];
                const uint16_t z = (uint16_t)(256u + rk[p]);
                const uint32_t lp = ew_prev(sb, p);
                if (lp != EW_NOPOS) ew_pend(rk, s_pend, &s_npend, lp);  // its right neighbour changes
                uint32_t cur = p, q = ew_next(sb, p);  // the pair's right token (in p's document: the pair has a rank)
                const bool run = tok[q] == x;
                for (;;) {
                    tok[cur] = z;
                    atomicAnd(&sb[q >> 5], ~(1u << (q & 31)));
                    rk[q] = EW_NONE;
                    ew_pend(rk, s_pend, &s_npend, cur);
                    if (!run) break;
                    cur = ew_next(sb, cur);
                    if (cur >= W || tok[cur] != x || ed_doc(db, cur)) break;  // the run ends after a pair (or with its document)
                    q = ew_next(sb, cur);
                    if (q >= W || tok[q] != x || ed_doc(db, q)) {  // odd token out
                        cur = q;
                        break;
                    }
                }
                // a run whose first token has an unknown left neighbour is uncertain to its end
                if (run && (p < Lu || (p == Lu && (lunk || Lu > 0) && !ed_doc(db, p)))) atomicMax(&s_runend, min(cur, W));
            }
            __syncthreads();
            if (EW_PROF_ON) {
                const unsigned long long t = wall_clock64();
                tpa += t - tq;
                tq = t;
            }
            const uint32_t np = s_npend;
            if (np <= EW_PENDCAP) {
                for (uint32_t i = tid; i < np; i += EW_T) ed_relook(A, tok, rk, sb, db, s_pend[i], W);
            } else {
                va = ((const uint4 *)myrk)[0];
                vc = ((const uint4 *)myrk)[1];
                for (uint32_t m = ew_in(va, vc, EW_PEND, EW_PEND + 1); m; m &= m - 1)
                    ed_relook(A, tok, rk, sb, db, p0 + (uint32_t)__builtin_ctz(m), W);
                if (EW_PROF_ON && tid == 0) atomicAdd(&A.prof[6], 1ull);
            }
            if (tid == EW_EDGE_T) {  // (phase B: no thread writes tok / sb)
                const uint32_t lu = max(lmove ? ew_next(sb, Lu) : Lu, s_runend), ru = rmove ? s_tpos : Ru;
                s_Lu = lu;
                s_Ru = ru;
                snapshot(lu, ru);
            }
            __syncthreads();
            if (EW_PROF_ON) tpb += wall_clock64() - tq;
            if (tid == 0) s_npend = 0;  // read by every thread above; the next batch's first barrier orders it
        }
        __syncthreads();
        unsigned long long tp2 = EW_PROF_ON ? wall_clock64() : 0;
        // db is done with; s_pend becomes the core-token counts before each word of sb (wave 0)
        for (uint32_t k = tid; k < EW_W / 32; k += EW_T) db[k] = 0;
        const uint32_t c0 = (uint32_t)(s0 - G.L), c1 = (uint32_t)(s1 - G.L);
        uint32_t *pref = (uint32_t *)s_pend;
        if (tid < 64) {
            const uint32_t mc = (uint32_t)__builtin_popcount(sb[tid] & ed_span(tid * 32, c0, c1));
            uint32_t inc = mc;
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t y = __shfl_up(inc, o);
                if ((int)lane >= o) inc += y;
            }
            pref[tid] = inc - mc;
        }
        // stage the tokens that start in the core, as k_enc_win does
        const uint32_t per = (c1 - c0 + EW_T - 1) / EW_T;
        const uint32_t lo = min(c1, c0 + tid * per), hi = min(c1, lo + per);
        uint32_t cnt = 0;
        for (uint32_t p = lo; p < hi; p++) cnt += ew_is_start(sb, p);
        if (tid == 0) {
            const uint32_t Lu = s_Lu, Ru = s_Ru;
            const uint32_t f = ew_from(sb, c0), g = ew_from(sb, max(Ru, c0));
            if ((f < c1 && f < Lu) || g < c1) {
                D.wfail[w] = 1u;
                atomicAdd(A.fail, 1u);
            }
        }
        uint32_t incl = cnt;
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t y = __shfl_up(incl, o);
            if ((int)lane >= o) incl += y;
        }
        if (lane == 63) s_wcnt[wv] = incl;
        __syncthreads();
        uint32_t before = 0, agg = 0;
        for (uint32_t k = 0; k < EW_T / 64; k++) {
            before += k < wv ? s_wcnt[k] : 0u;
            agg += s_wcnt[k];
        }
        // core tokens before every document that starts in the core (a
        // document start is a token start: nothing merges across it)
        for (uint64_t d = (uint64_t)i0 + tid; d < i1; d += EW_T) {
            const uint32_t p = (uint32_t)(D.doc_off[d] - G.L);
            if (p < EW_W) {
                const uint32_t wd = p >> 5;
                const uint32_t m = sb[wd] & ed_span(wd * 32, c0, p);
                D.rel[d] = pref[wd] + (uint32_t)__builtin_popcount(m);
            }
        }
        uint16_t *cmp = rk + before + incl - cnt;
        for (uint32_t p = lo; p < hi; p++)
            if (ew_is_start(sb, p)) *cmp++ = tok[p];
        __syncthreads();
        uint4 *dst = (uint4 *)(A.stage + (uint64_t)w * A.core);  // (core * 2 bytes is a multiple of 16)
        for (uint32_t k = tid; k * 8 < agg; k += EW_T) dst[k] = ((const uint4 *)rk)[k];
        if (tid == 0) A.cnt[w] = agg;
        if (EW_PROF_ON && tid == 0) {
            const unsigned long long tp3 = wall_clock64();
            atomicAdd(&A.prof[0], tp1 - tp0);
            atomicAdd(&A.prof[1], tp2 - tp1);
            atomicAdd(&A.prof[2], tp3 - tp2);
            atomicAdd(&A.prof[4], nhas);
            atomicAdd(&A.prof[3], tpa);
            atomicAdd(&A.prof[7], tpb);
            atomicAdd(&A.prof[5], 1ull);
        }
        __syncthreads();
    }
}

}  // namespace bpeamd

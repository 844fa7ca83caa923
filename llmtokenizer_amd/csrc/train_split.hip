// train_split.hip -- training on the pieces of the last split; included by engine.hip; its host side is pieces.hip.
//
// The corpus is the multiset of pieces (split.hip's offsets over the resident
// bytes): a pair is counted only inside one piece and a merge is applied inside
// each piece, left to right.  Two stages, both beside the batch engine:
//
// Stage A, the piece table.  Equal pieces become one weighted entry.
//   k_ts_insert    a thread per piece: pieces of at most TS_DEDUP_MAX bytes are
//                  hashed and looked up in an open-addressing table in HBM whose
//                  slot is one 64-bit word (hash tag << 32) | piece index.  An
//                  empty slot is claimed with one CAS; a slot with the same tag
//                  is confirmed by comparing the bytes of its piece, then
//                  lowered to the smaller index with a 64-bit atomicMin.  A slot
//                  word is complete the moment it exists, so no lane waits for
//                  another one, and a probe chain ends after TS_PROBE slots
//                  (the host then grows the table and runs the stage again).
//                  The per-slot counts go through a per-block LDS table first.
//   k_ts_collect_* the occupied slots and the pieces above TS_DEDUP_MAX (an
//                  entry each, count 1) as (piece index, count) records;
//   (rocprim::radix_sort_pairs by piece index = by start; exclusive_scan of the lengths)
//   k_ts_entries   start and length of every entry;
//   k_ts_gather    a thread per OUTPUT token finds its entry by a binary search
//                  of the scanned lengths: one huge entry costs what many small do.
//
// Stage B, a weighted recount per merge over the entries' tokens (tok[], and
// ent[]: the entry of every token, which is both the boundary and the weight).
//   k_tb_count     adds the entry's weight for every adjacent in-entry pair into
//                  a pair table in HBM (64-bit key CAS, bounded probes), through
//                  a 128 KiB LDS table per workgroup that takes the contention;
//   k_tb_argmax*   the pair with (count desc, a asc, b asc);
//   k_tb_heads     a == a merges: where a run of `a` begins (an entry start is
//                  one), turned into every token's run start by an inclusive
//                  max-scan (rocprim), so no lane walks a run;
//   k_tb_flag      which tokens a merge drops; (exclusive_scan) k_tb_scatter
//                  writes the survivors into the other buffer.
//
// No loop has a trip count that a piece length, a run length or a probe chain
// decides: they are bounded by TS_DEDUP_MAX, TS_PROBE, TB_PROBE, TB_LPROBE and 32
// (the binary search).

namespace bpeamd {

constexpr uint32_t TS_T = 256;           // threads per workgroup, every kernel of this file
constexpr uint32_t TS_DEDUP_MAX = 64;    // longest piece that is hashed (bpe_gpu_train_split_info)
constexpr uint32_t TS_PROBE = 128;       // slots a piece probes before the table counts as full
constexpr uint32_t TB_PROBE = 128;       // ... a pair in the pair table
constexpr uint32_t TS_LSLOTS = 2048;     // slots of a workgroup's LDS count table (24 KiB)
constexpr uint32_t TB_LPROBE = 8;        // LDS probes before a count goes to HBM directly
constexpr uint32_t TB_CT = 1024;         // threads of a workgroup of the count pass
constexpr uint32_t TB_LSLOTS = 16384;    // slots of its LDS pair table (128 KiB)
constexpr uint32_t TS_GRID = 2048;       // workgroups at most; the rest is strided
constexpr unsigned long long TS_EMPTY = ~0ull;

// ctl words (device, read by the host after each stage)
enum { TSC_FULL = 0, TSC_LONG = 1, TSC_CLAIMED = 2, TSC_APPEND = 3, TSC_PFULL = 4, TSC_CNT = 5, TSC_A = 6, TSC_B = 7 };

__device__ inline uint64_t ts_mix64(uint64_t x) {
    x ^= x >> 33;
    x *= 0xff51afd7ed558ccdull;
    x ^= x >> 33;
    x *= 0xc4ceb9fe1a85ec53ull;
    x ^= x >> 33;
    return x;
}

// one atomicAdd per wave of the number of lanes with `pred`; the lane's index in the sum (pred lanes only).
// Every lane of the wave must call it.
__device__ inline uint32_t ts_wave_take(bool pred, uint32_t *ctr) {
    const unsigned long long m = __ballot(pred);
    if (!m) return 0;
    const uint32_t lane = threadIdx.x & 63u, leader = (uint32_t)__builtin_ctzll(m);
    uint32_t base = 0;
    if (lane == leader) base = atomicAdd(ctr, (uint32_t)__popcll(m));
    base = __shfl(base, (int)leader);
    return base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
}

// the workgroup's LDS count table: add w under `key`; false when TB_LPROBE slots from h held other keys
__device__ inline bool ts_lds_add(unsigned long long *lk, uint32_t *lc, unsigned long long key, uint32_t h, uint32_t w) {
#pragma unroll
    for (uint32_t p = 0; p < TB_LPROBE; p++) {
        const uint32_t i = (h + p) & (TS_LSLOTS - 1);
        unsigned long long cur = __hip_atomic_load(&lk[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (cur == TS_EMPTY) {
            cur = atomicCAS(&lk[i], TS_EMPTY, key);
            if (cur == TS_EMPTY) cur = key;
        }
        if (cur == key) {
            atomicAdd(&lc[i], w);
            return true;
        }
    }
    return false;
}

__device__ inline void ts_lds_clear(unsigned long long *lk, uint32_t *lc) {
    for (uint32_t i = threadIdx.x; i < TS_LSLOTS; i += TS_T) {
        lk[i] = TS_EMPTY;
        lc[i] = 0;
    }
    __syncthreads();
}

// ---------------------------------------------------------------- stage A

__global__ __launch_bounds__(TS_T) void k_ts_insert(const uint8_t *__restrict__ bytes, const uint64_t *__restrict__ off,
                                                    uint64_t P, unsigned long long *slot, uint32_t *scnt, uint64_t smask,
                                                    uint32_t *ctl) {
    __shared__ unsigned long long lk[TS_LSLOTS];
    __shared__ uint32_t lc[TS_LSLOTS];
    ts_lds_clear(lk, lc);
    for (uint64_t base = (uint64_t)blockIdx.x * TS_T; base < P; base += (uint64_t)gridDim.x * TS_T) {  // (block-uniform trips)
        const uint64_t p = base + threadIdx.x;
        bool is_long = false, claimed = false;
        if (p < P) {
            const uint64_t s = off[p], len = off[p + 1] - s;
            if (len > TS_DEDUP_MAX) {
                is_long = true;
            } else {
                const uint8_t *b = bytes + s;
                uint64_t h = 0xcbf29ce484222325ull ^ len;
                for (uint32_t i = 0; i < TS_DEDUP_MAX; i++) {
                    if (i >= len) break;
                    h = (h ^ b[i]) * 0x100000001b3ull;
                }
                h = ts_mix64(h);
                const unsigned long long tag = h >> 32, mine = (tag << 32) | p;
                uint64_t i = h & smask;
                bool done = false;
                for (uint32_t k = 0; k < TS_PROBE; k++) {
                    unsigned long long w = __hip_atomic_load(&slot[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (w == TS_EMPTY) {
                        w = atomicCAS(&slot[i], TS_EMPTY, mine);
                        if (w == TS_EMPTY) {
                            claimed = true;
                            w = mine;
                        }
                    }
                    bool same = w == mine;
                    if (!same && (w >> 32) == tag) {  // the slot's piece (any piece of its class: all hold equal bytes)
                        const uint64_t q = w & 0xFFFFFFFFull, qs = off[q];
                        if (off[q + 1] - qs == len) {
                            const uint8_t *r = bytes + qs;
                            same = true;
                            for (uint32_t j = 0; j < TS_DEDUP_MAX; j++) {
                                if (j >= len) break;
                                if (r[j] != b[j]) {
                                    same = false;
                                    break;
                                }
                            }
                        }
                        if (same && mine < w) atomicMin(&slot[i], mine);
                    }
                    if (same) {
                        if (!ts_lds_add(lk, lc, i, (uint32_t)(h >> 40), 1u)) atomicAdd(&scnt[i], 1u);
                        done = true;
                        break;
                    }
                    i = (i + 1) & smask;
                }
                if (!done) ctl[TSC_FULL] = 1u;
            }
        }
        (void)ts_wave_take(is_long, &ctl[TSC_LONG]);
        (void)ts_wave_take(claimed, &ctl[TSC_CLAIMED]);
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < TS_LSLOTS; i += TS_T)
        if (lc[i]) atomicAdd(&scnt[lk[i]], lc[i]);
}

// (piece index, count) of every occupied slot, appended at ctl[TSC_APPEND]; E = the records' capacity
__global__ __launch_bounds__(TS_T) void k_ts_collect_slots(const unsigned long long *__restrict__ slot,
                                                           const uint32_t *__restrict__ scnt, uint64_t S, uint32_t *ctl,
                                                           uint32_t *__restrict__ key, uint32_t *__restrict__ val, uint64_t E) {
    for (uint64_t base = (uint64_t)blockIdx.x * TS_T; base < S; base += (uint64_t)gridDim.x * TS_T) {
        const uint64_t i = base + threadIdx.x;
        const unsigned long long w = i < S ? slot[i] : TS_EMPTY;
        const bool has = w != TS_EMPTY;
        const uint32_t at = ts_wave_take(has, &ctl[TSC_APPEND]);
        if (has && at < E) {
            key[at] = (uint32_t)w;
            val[at] = scnt[i];
        }
    }
}

__global__ __launch_bounds__(TS_T) void k_ts_collect_long(const uint64_t *__restrict__ off, uint64_t P, uint32_t *ctl,
                                                          uint32_t *__restrict__ key, uint32_t *__restrict__ val, uint64_t E) {
    for (uint64_t base = (uint64_t)blockIdx.x * TS_T; base < P; base += (uint64_t)gridDim.x * TS_T) {
        const uint64_t p = base + threadIdx.x;
        const bool has = p < P && off[p + 1] - off[p] > TS_DEDUP_MAX;
        const uint32_t at = ts_wave_take(has, &ctl[TSC_APPEND]);
        if (has && at < E) {
            key[at] = (uint32_t)p;
            val[at] = 1u;
        }
    }
}

// est[e], elen[e] of the sorted entries; elen[E] = 0 (the scan's last element is the total)
__global__ __launch_bounds__(TS_T) void k_ts_entries(const uint64_t *__restrict__ off, const uint32_t *__restrict__ epi,
                                                     uint64_t E, uint64_t *__restrict__ est, uint32_t *__restrict__ elen) {
    const uint64_t e = (uint64_t)blockIdx.x * TS_T + threadIdx.x;
    if (e < E) {
        const uint64_t s = off[epi[e]];
        est[e] = s;
        elen[e] = (uint32_t)(off[(uint64_t)epi[e] + 1] - s);
    } else if (e == E) {
        elen[e] = 0;
    }
}

// tok[t] = the byte at offset t - eoff[e] of entry e, ent[t] = e, where eoff[e] <= t < eoff[e + 1]
__global__ __launch_bounds__(TS_T) void k_ts_gather(const uint8_t *__restrict__ bytes, const uint64_t *__restrict__ est,
                                                    const uint32_t *__restrict__ eoff, uint32_t E, uint32_t T,
                                                    uint32_t *__restrict__ tok, uint32_t *__restrict__ ent) {
    for (uint64_t t = (uint64_t)blockIdx.x * TS_T + threadIdx.x; t < T; t += (uint64_t)gridDim.x * TS_T) {
        uint32_t lo = 0, hi = E;  // eoff[lo] <= t < eoff[hi]  (eoff[0] == 0, eoff[E] == T; no entry is empty)
        for (uint32_t k = 0; k < 32; k++) {
            if (hi - lo <= 1) break;
            const uint32_t mid = lo + (hi - lo) / 2;
            if (eoff[mid] <= t) lo = mid;
            else hi = mid;
        }
        tok[t] = bytes[est[lo] + (t - eoff[lo])];
        ent[t] = lo;
    }
}

// ---------------------------------------------------------------- stage B

__device__ inline void tb_global_add(unsigned long long *pk, uint32_t *pc, uint64_t pmask, unsigned long long key, uint32_t w,
                                     uint32_t *ctl) {
    uint64_t i = ts_mix64(key) & pmask;
    for (uint32_t k = 0; k < TB_PROBE; k++) {
        unsigned long long cur = __hip_atomic_load(&pk[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == TS_EMPTY) {
            cur = atomicCAS(&pk[i], TS_EMPTY, key);
            if (cur == TS_EMPTY) cur = key;
        }
        if (cur == key) {
            atomicAdd(&pc[i], w);
            return;
        }
        i = (i + 1) & pmask;
    }
    ctl[TSC_PFULL] = 1u;
}

// The count pass has a workgroup of its own shape: 1,024 threads and a 128 KiB LDS table (one workgroup per
// CU, 16 waves) of 32-bit keys a << 16 | b, so that the ~10^4 distinct pairs of random bytes still meet in
// LDS; a pair with an id of 65,535 or more goes to HBM directly.
__global__ __launch_bounds__(TB_CT) void k_tb_count(const uint32_t *__restrict__ tok, const uint32_t *__restrict__ ent,
                                                    const uint32_t *__restrict__ ecnt, uint32_t T, unsigned long long *pk,
                                                    uint32_t *pc, uint64_t pmask, uint32_t *ctl) {
    __shared__ uint32_t lk[TB_LSLOTS];
    __shared__ uint32_t lc[TB_LSLOTS];
    for (uint32_t i = threadIdx.x; i < TB_LSLOTS; i += TB_CT) {
        lk[i] = ~0u;
        lc[i] = 0;
    }
    __syncthreads();
    for (uint64_t t = (uint64_t)blockIdx.x * TB_CT + threadIdx.x; t + 1 < T; t += (uint64_t)gridDim.x * TB_CT) {
        const uint32_t e = ent[t];
        if (e != ent[t + 1]) continue;
        const uint32_t a = tok[t], b = tok[t + 1], w = ecnt[e];
        bool placed = false;
        if ((a | b) < 0xFFFFu) {
            const uint32_t key = (a << 16) | b, h = (key * 0x9E3779B1u) >> 18;
#pragma unroll
            for (uint32_t p = 0; p < TB_LPROBE; p++) {
                const uint32_t i = (h + p) & (TB_LSLOTS - 1);
                uint32_t cur = __hip_atomic_load(&lk[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                if (cur == ~0u) {
                    cur = atomicCAS(&lk[i], ~0u, key);
                    if (cur == ~0u) cur = key;
                }
                if (cur == key) {
                    atomicAdd(&lc[i], w);
                    placed = true;
                    break;
                }
            }
        }
        if (!placed) tb_global_add(pk, pc, pmask, ((unsigned long long)a << 32) | b, w, ctl);
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < TB_LSLOTS; i += TB_CT)
        if (lc[i]) tb_global_add(pk, pc, pmask, ((unsigned long long)(lk[i] >> 16) << 32) | (lk[i] & 0xFFFFu), lc[i], ctl);
}

// (c1, k1) ahead of (c2, k2): the larger count, then the smaller a, then the smaller b (key = a << 32 | b)
__device__ inline bool tb_ahead(uint32_t c1, unsigned long long k1, uint32_t c2, unsigned long long k2) {
    return c1 > c2 || (c1 == c2 && k1 < k2);
}

// the workgroup's best of the threads' (c, k) in thread 0
__device__ inline void tb_block_best(uint32_t &c, unsigned long long &k) {
    __shared__ uint32_t sc[TS_T / 64];
    __shared__ unsigned long long sk[TS_T / 64];
    for (int d = 32; d; d >>= 1) {
        const uint32_t c2 = __shfl_xor(c, d);
        const unsigned long long k2 = __shfl_xor(k, d);
        if (tb_ahead(c2, k2, c, k)) {
            c = c2;
            k = k2;
        }
    }
    if ((threadIdx.x & 63u) == 0) {
        sc[threadIdx.x >> 6] = c;
        sk[threadIdx.x >> 6] = k;
    }
    __syncthreads();
    if (threadIdx.x == 0)
        for (uint32_t v = 1; v < TS_T / 64; v++)
            if (tb_ahead(sc[v], sk[v], c, k)) {
                c = sc[v];
                k = sk[v];
            }
}

// part[2 b], part[2 b + 1] = workgroup b's best count and key (count 0: none)
__global__ __launch_bounds__(TS_T) void k_tb_argmax(const unsigned long long *__restrict__ pk, const uint32_t *__restrict__ pc,
                                                    uint64_t S, unsigned long long *__restrict__ part) {
    uint32_t c = 0;
    unsigned long long k = TS_EMPTY;
    for (uint64_t i = (uint64_t)blockIdx.x * TS_T + threadIdx.x; i < S; i += (uint64_t)gridDim.x * TS_T) {
        const uint32_t ci = pc[i];
        if (ci && tb_ahead(ci, pk[i], c, k)) {
            c = ci;
            k = pk[i];
        }
    }
    tb_block_best(c, k);
    if (threadIdx.x == 0) {
        part[2 * blockIdx.x] = c;
        part[2 * blockIdx.x + 1] = k;
    }
}

__global__ __launch_bounds__(TS_T) void k_tb_argmax2(const unsigned long long *__restrict__ part, uint32_t nb, uint32_t *ctl) {
    uint32_t c = 0;
    unsigned long long k = TS_EMPTY;
    for (uint32_t i = threadIdx.x; i < nb; i += TS_T) {
        const uint32_t ci = (uint32_t)part[2 * i];
        if (ci && tb_ahead(ci, part[2 * i + 1], c, k)) {
            c = ci;
            k = part[2 * i + 1];
        }
    }
    tb_block_best(c, k);
    if (threadIdx.x == 0) {
        ctl[TSC_CNT] = c;
        ctl[TSC_A] = (uint32_t)(k >> 32);
        ctl[TSC_B] = (uint32_t)k;
    }
}

// v[t] = t where a run of `a` begins or no run is (an entry start, another token), else 0:
// the inclusive max-scan of v is every token's run start
__global__ __launch_bounds__(TS_T) void k_tb_heads(const uint32_t *__restrict__ tok, const uint32_t *__restrict__ ent,
                                                   uint32_t T, uint32_t a, uint32_t *__restrict__ v) {
    for (uint64_t t = (uint64_t)blockIdx.x * TS_T + threadIdx.x; t < T; t += (uint64_t)gridDim.x * TS_T) {
        const bool inside = t > 0 && tok[t] == a && tok[t - 1] == a && ent[t - 1] == ent[t];
        v[t] = inside ? 0u : (uint32_t)t;
    }
}

// keep[t] = 0 for the second token of every merged pair, else 1; keep[T] = 0.
// a != b: pairs cannot overlap.  a == b (rs != nullptr): pairs sit at even offsets from the run start,
// so a token at an odd offset is the second one of the pair before it.
__global__ __launch_bounds__(TS_T) void k_tb_flag(const uint32_t *__restrict__ tok, const uint32_t *__restrict__ ent,
                                                  const uint32_t *__restrict__ rs, uint32_t T, uint32_t a, uint32_t b,
                                                  uint32_t *__restrict__ keep) {
    for (uint64_t t = (uint64_t)blockIdx.x * TS_T + threadIdx.x; t <= T; t += (uint64_t)gridDim.x * TS_T) {
        bool drop = false;
        if (t < T && tok[t] == b) {
            if (rs) drop = (((uint32_t)t - rs[t]) & 1u) != 0;
            else drop = t > 0 && tok[t - 1] == a && ent[t - 1] == ent[t];
        }
        keep[t] = t < T && !drop ? 1u : 0u;
    }
}

// the kept tokens at their scanned positions; one whose successor was dropped becomes z
__global__ __launch_bounds__(TS_T) void k_tb_scatter(const uint32_t *__restrict__ tok, const uint32_t *__restrict__ ent,
                                                     const uint32_t *__restrict__ keep, const uint32_t *__restrict__ pos,
                                                     uint32_t T, uint32_t z, uint32_t *__restrict__ tok2,
                                                     uint32_t *__restrict__ ent2) {
    for (uint64_t t = (uint64_t)blockIdx.x * TS_T + threadIdx.x; t < T; t += (uint64_t)gridDim.x * TS_T) {
        if (!keep[t]) continue;
        const bool merged = t + 1 < T && !keep[t + 1];
        const uint32_t o = pos[t];
        tok2[o] = merged ? z : tok[t];
        ent2[o] = ent[t];
    }
}

}  // namespace bpeamd

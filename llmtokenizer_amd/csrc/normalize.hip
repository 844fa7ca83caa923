// normalize.hip -- BPE_NORM_NFC on the resident bytes (bpe_gpu.h, "Normalization"); included by engine.hip after
// rows.hip.  The steps on one character or one buffer are those of src/bpe_nfc_rule.h, compiled for the device
// over the tables of unicode_nfc.h in device memory; this file is how the text is cut up and how the bytes move.
//
// Segments.  A character whose work flag is clear is a boundary; a segment is a boundary (or the text's first
// character) and every flagged character behind it.  A segment with a flagged character is dirty.  A byte of a
// clean segment is worth one output byte to the lane that holds it; a dirty segment is worth its normalized length
// to the lane that holds its first byte, and its bytes are worth nothing where they lie.  So a tile with no dirty
// segment is worth its own size and is copied as it is.
//
// A lane takes NF_PER = 16 bytes (one aligned 16-byte load), a wave NF_WAVE, a workgroup NF_TILE, tiles past the
// grid in grid strides.  Every flagged code point is >= U+0300, a lead byte >= 0xCC: a lane in whose window
// [s - 3, s + 20) no such byte lies (its own word test, its two neighbours' by ballot, the wave's two edges by one
// word each) counts and copies its 16 bytes with no table load.  Any other lane walks the characters of its chunk
// (nf_lane): the record of each, and for the owner of a dirty segment nf_segment: decompose into the lane's NF_LANE
// entries of LDS, order, compose, and measure or encode.  Every loop there is bounded by 16 bytes or NF_LANE entries.
//   k_nf_measure  pass 1: the worth of every tile (cnt), a flag when any segment is dirty, and the queue of the
//                 segments that outgrow NF_LANE entries (their worth comes from k_nf_long_run, added to cnt).
//   (rocprim::exclusive_scan over cnt: the tiles' output offsets)
//   k_nf_write    pass 2: the same walk from the tile's offset.  A tile's output is put together in LDS at the
//                 destination's alignment (byte o of the output at index o - (tile offset & ~15)) and leaves in
//                 aligned 16-byte stores, single bytes only in the two partial groups at its ends.  A clean tile is
//                 its source words stored at the shifted index (whole words when the shift is a multiple of 4).  A
//                 tile worth more than NF_STAGE bytes, or one that holds a queued segment, writes single bytes to
//                 memory instead.  In a text batch the lane that holds a NUL looks it up among the gaps (a binary
//                 search of boff; only a NUL pays it) and writes the gap's new position: no second pass over the
//                 text, and no lane waits for another.
//   k_nf_long_len / _run / _write  the fallback, a segment per workgroup, one lane working: slow and exact for any
//                 length.  The entries are decomposed into a workspace the host sized from k_nf_long_len's counts,
//                 ordered by a counting sort on ccc (stable; 5,000 marks in reverse order are 5,000 moves, not
//                 12 million), composed in place and encoded to where pass 2 said the segment begins.
// The pair list is searched where it lies (941 keys: ten probes of an L2-resident array).  Staging its 11 KiB in
// LDS for a tile of 4 KiB with one dirty segment would triple what that workgroup reads.

#define BPE_NFC_STORAGE __device__ const
#define NFC_FN __device__ inline
#include "../src/bpe_nfc_rule.h"

namespace bpeamd {

constexpr uint32_t NF_PER = 16;                      // bytes per lane
constexpr uint32_t NF_T = 256;                       // threads per workgroup
constexpr uint32_t NF_WAVE = 64 * NF_PER;            // bytes per wave tile
constexpr uint32_t NF_TILE = BPE_GPU_SPLIT_TILE;     // bytes per workgroup step (the split kernels' tile)
constexpr uint32_t NF_GRID = 2048;                   // workgroups at most
constexpr uint32_t NF_LANE = 32;                     // entries (decomposed code points) of a segment a lane takes
constexpr uint32_t NF_SEG_STRIDE = NF_LANE + 1;      // words between two lanes' buffers (odd: no bank in common)
constexpr uint32_t NF_STAGE = 2 * NF_TILE;           // output bytes of a tile that are staged in LDS
static_assert(NF_TILE == NF_T * NF_PER, "a lane per 16 bytes");

enum { NFC_DIRTY = 0, NFC_QCOUNT, NFC_ERR, NFC_WORDS };  // control words

struct NfLong {  // a queued segment
    unsigned long long start, end, ncp, ws, outlen, ncomp, outpos, pad;
};

struct NfArgs {
    const uint8_t *b;
    uint64_t n;
    uint32_t *ctl;
    unsigned long long *queue;  // pass 1: the starts of the queued segments
    uint32_t qcap;
    NfLong *ent;                // pass 2: the queued segments, sorted by start
    uint32_t nent;
    const uint64_t *boff;       // a text batch's offsets (nullptr: none) and where the new ones go
    uint64_t *boff_new;
    uint64_t T;
};

// where pass 2 puts a byte: LDS (index pos - base, below cap) or memory (below out_n)
struct NfSink {
    uint8_t *lds;
    uint8_t *dst;
    uint64_t pos, base, out_n;
    uint32_t cap;
    __device__ inline void put(uint8_t v) {
        if (lds) {
            const uint64_t i = pos - base;
            if (i < cap) lds[i] = v;
        } else if (pos < out_n) {
            dst[pos] = v;
        }
        pos++;
    }
};

__device__ inline bool nf_has_cc(uint32_t w) {  // a byte >= 0xCC in w
    return (((w & 0x7F7F7F7Fu) + 0x34343434u) & w & 0x80808080u) != 0;
}
__device__ inline bool nf_has_zero(uint32_t w) { return ((w - 0x01010101u) & ~w & 0x80808080u) != 0; }

// the queued segment that starts at c, or nent
__device__ inline uint32_t nf_find_long(const NfArgs &A, uint64_t c) {
    uint32_t lo = 0, hi = A.nent;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (A.ent[mid].start < c) lo = mid + 1; else hi = mid;
    }
    return lo < A.nent && A.ent[lo].start == c ? lo : A.nent;
}

// the NUL at resident position p now lies at output position o: if it is gap k, boff_new[k + 1] = o - k
__device__ inline void nf_gap(const NfArgs &A, uint64_t p, uint64_t o) {
    uint64_t lo = 0, hi = A.T;  // gap k is at boff[k + 1] + k, ascending in k
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (A.boff[mid + 1] + mid < p) lo = mid + 1; else hi = mid;
    }
    if (lo < A.T && A.boff[lo + 1] + lo == p) A.boff_new[lo + 1] = o - lo;
}

// MODE 0: pass 1, measure (an outgrown segment is queued and worth 0 here); 1: pass 2, measure (its worth is the
// fallback's); 2: pass 2, write (its bytes are the fallback's: its output position is noted and stepped over).
// The segment begins at c with the character (e, l); buf: the lane's NF_LANE entries.  Returns its worth.
template <int MODE>
__device__ inline uint32_t nf_segment(const NfArgs &A, uint64_t c, uint32_t e, uint32_t l, uint32_t *buf, NfSink &sink,
                                      bool &has_long) {
    uint32_t cnt = 0, d[4];
    bool fits = true;
    for (uint64_t p = c;;) {  // (at most NF_LANE + 1 turns: every turn adds an entry)
        const uint32_t k = nfc_decompose(e, nfc_record(e), d);
        if (cnt + k > NF_LANE) { fits = false; break; }
        for (uint32_t i = 0; i < k; i++) buf[cnt + i] = d[i];
        cnt += k;
        p += l;
        if (p >= A.n) break;
        l = nfc_decode(A.b, A.n, p, &e);
        if (!NFC_WORK(nfc_record(e))) break;
    }
    if (!fits) {
        has_long = true;
        if (MODE == 0) {
            const uint32_t i = atomicAdd(&A.ctl[NFC_QCOUNT], 1u);
            if (i < A.qcap) A.queue[i] = c;
            return 0;
        }
        const uint32_t i = nf_find_long(A, c);
        if (i == A.nent) { A.ctl[NFC_ERR] = 1u; return 0; }
        const uint32_t len = (uint32_t)A.ent[i].outlen;
        if (MODE == 2) { A.ent[i].outpos = sink.pos; sink.pos += len; }
        return len;
    }
    nfc_reorder(buf, cnt);
    cnt = (uint32_t)nfc_compose(buf, cnt);
    uint32_t len = 0;
    for (uint32_t i = 0; i < cnt; i++) {
        if (MODE == 2) {
            uint8_t u[4];
            const uint32_t k = nfc_encode(buf[i], u);
            for (uint32_t j = 0; j < k; j++) sink.put(u[j]);
            len += k;
        } else {
            len += nfc_utf8_len(buf[i]);
        }
    }
    return len;
}

// the worth of the chunk [s, s + 16) clipped to n, character by character
template <int MODE>
__device__ inline uint32_t nf_lane(const NfArgs &A, uint64_t s, uint32_t *buf, NfSink &sink, bool &has_long) {
    const uint64_t end = s + NF_PER < A.n ? s + NF_PER : A.n;
    uint32_t len = 0, e, e2 = 0, l2 = 0;
    uint64_t c = nfc_char_start(A.b, A.n, s);
    uint32_t l = nfc_decode(A.b, A.n, c, &e);
    bool w = NFC_WORK(nfc_record(e)), w2 = false;
    while (c < end) {  // (at most 16 turns)
        const uint64_t q = c + l;
        w2 = false;
        if (q < A.n) {
            l2 = nfc_decode(A.b, A.n, q, &e2);
            w2 = NFC_WORK(nfc_record(e2));
        }
        if (MODE == 2 && A.boff && e == 0 && c >= s) nf_gap(A, c, sink.pos);  // (a NUL is the first of its segment)
        if (!w && !w2) {  // a clean character: the bytes of it that lie in this chunk
            const uint64_t lo = c > s ? c : s, hi = q < end ? q : end;
            if (MODE == 2)
                for (uint64_t p = lo; p < hi; p++) sink.put(A.b[p]);
            len += (uint32_t)(hi - lo);
        } else if ((!w || c == 0) && c >= s) {  // the first character of a dirty segment, its lead byte here
            if (MODE == 0) A.ctl[NFC_DIRTY] = 1u;
            len += nf_segment<MODE>(A, c, e, l, buf, sink, has_long);
        }
        c = q, e = e2, l = l2, w = w2;
    }
    return len;
}

// Does a byte >= 0xCC lie in the lane's window [s - 3, s + 20)?  q: the lane's 16 bytes (zeros at and past n).
__device__ inline bool nf_near(const NfArgs &A, uint64_t s, const uint4 &q) {
    const bool hi = nf_has_cc(q.x) | nf_has_cc(q.y) | nf_has_cc(q.z) | nf_has_cc(q.w);
    const unsigned long long m = __ballot(hi);
    const uint32_t lane = threadIdx.x & 63u;
    bool near = ((m >> lane) & 1ull) | (lane ? (m >> (lane - 1)) & 1ull : 0ull) | (lane < 63 ? (m >> (lane + 1)) & 1ull : 0ull);
    // (the words before and behind the wave tile; the bytes hold 64 zeros past n, and s is a multiple of 16)
    if (lane == 0 && s && s < A.n) near |= nf_has_cc(*(const uint32_t *)(A.b + s - 4));
    if (lane == 63 && s + NF_PER < A.n) near |= nf_has_cc(*(const uint32_t *)(A.b + s + NF_PER));
    return near;
}

// exclusive scan of x over the workgroup's NF_T lanes; *total = the sum.  sw: 4 words of LDS.
__device__ inline uint32_t nf_block_scan(uint32_t x, uint32_t *sw, uint32_t *total) {
    uint32_t incl = x;
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    for (uint32_t o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(incl, o);
        if (lane >= o) incl += y;
    }
    __syncthreads();  // (sw may still be read from the turn before)
    if (lane == 63) sw[wv] = incl;
    __syncthreads();
    uint32_t before = 0, all = 0;
    for (uint32_t k = 0; k < NF_T / 64; k++) {
        if (k < wv) before += sw[k];
        all += sw[k];
    }
    *total = all;
    return before + incl - x;
}

__global__ __launch_bounds__(NF_T) void k_nf_measure(const NfArgs A, unsigned long long *__restrict__ cnt) {
    __shared__ uint32_t s_seg[NF_T * NF_SEG_STRIDE];
    __shared__ uint32_t s_w[4];
    const uint64_t ntiles = (A.n + NF_TILE - 1) / NF_TILE;
    NfSink none{};
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const uint64_t s = t * NF_TILE + (uint64_t)threadIdx.x * NF_PER;
        uint4 q = make_uint4(0, 0, 0, 0);
        if (s < A.n) q = *(const uint4 *)(A.b + s);
        uint32_t len = s < A.n ? (uint32_t)(A.n - s < NF_PER ? A.n - s : NF_PER) : 0;
        bool has_long = false;
        if (nf_near(A, s, q) && s < A.n) len = nf_lane<0>(A, s, s_seg + threadIdx.x * NF_SEG_STRIDE, none, has_long);
        uint32_t total;
        (void)nf_block_scan(len, s_w, &total);
        if (threadIdx.x == 0) cnt[t] = total;
    }
}

__global__ __launch_bounds__(NF_T) void k_nf_write(const NfArgs A, const unsigned long long *__restrict__ off,
                                                   uint8_t *__restrict__ dst, uint64_t out_n) {
    __shared__ uint32_t s_seg[NF_T * NF_SEG_STRIDE];
    __shared__ uint4 s_out4[(NF_STAGE + 32) / 16];
    __shared__ uint32_t s_w[4];
    uint8_t *s_out = (uint8_t *)s_out4;
    const uint64_t ntiles = (A.n + NF_TILE - 1) / NF_TILE;
    if (blockIdx.x == 0 && threadIdx.x == 0 && A.boff) A.boff_new[0] = 0;
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const uint64_t s = t * NF_TILE + (uint64_t)threadIdx.x * NF_PER;
        const uint64_t o = off[t], total = off[t + 1] - o, base = o & ~15ull;
        uint4 q = make_uint4(0, 0, 0, 0);
        if (s < A.n) q = *(const uint4 *)(A.b + s);
        const uint32_t valid = s < A.n ? (uint32_t)(A.n - s < NF_PER ? A.n - s : NF_PER) : 0;
        const bool near = nf_near(A, s, q) && s < A.n;
        uint32_t *buf = s_seg + threadIdx.x * NF_SEG_STRIDE;
        NfSink sink{};
        bool has_long = false;
        uint32_t len = valid;
        if (near) len = nf_lane<1>(A, s, buf, sink, has_long);
        uint32_t sum;
        const uint32_t mine = nf_block_scan(len, s_w, &sum);
        const bool direct = __syncthreads_or(has_long) || total > NF_STAGE;  // (also: s_out is free again)
        sink.lds = direct ? nullptr : s_out;
        sink.dst = dst;
        sink.pos = o + mine;
        sink.base = base;
        sink.out_n = out_n;
        sink.cap = NF_STAGE + 16;
        if (near) {
            (void)nf_lane<2>(A, s, buf, sink, has_long);
        } else if (valid) {
            if (A.boff && (nf_has_zero(q.x) | nf_has_zero(q.y) | nf_has_zero(q.z) | nf_has_zero(q.w))) {
                const uint32_t wd[4] = {q.x, q.y, q.z, q.w};
                for (uint32_t k = 0; k < valid; k++)
                    if (((wd[k >> 2] >> (8u * (k & 3u))) & 0xFFu) == 0) nf_gap(A, s + k, sink.pos + k);
            }
            const uint64_t i = sink.pos - base;
            if (!direct && valid == NF_PER && (i & 3u) == 0 && i + NF_PER <= sink.cap) {
                uint32_t *p = (uint32_t *)(s_out + i);
                p[0] = q.x, p[1] = q.y, p[2] = q.z, p[3] = q.w;
            } else {
                const uint32_t wd[4] = {q.x, q.y, q.z, q.w};
                for (uint32_t k = 0; k < valid; k++) sink.put((uint8_t)(wd[k >> 2] >> (8u * (k & 3u))));
            }
        }
        __syncthreads();
        if (!direct) {
            const uint64_t end = o + total;  // (<= out_n: the scan's last entry)
            for (uint64_t g = threadIdx.x; base + 16 * g < end; g += NF_T) {
                const uint64_t gp = base + 16 * g;
                if (gp >= o && gp + 16 <= end && gp + 16 <= out_n) {
                    *(uint4 *)(dst + gp) = s_out4[g];
                } else {
                    for (uint64_t p = gp > o ? gp : o; p < gp + 16 && p < end && p < out_n; p++) dst[p] = s_out[p - base];
                }
            }
        }
        __syncthreads();
    }
}

// ---- the fallback: a thread per queued segment finds its end and counts its entries ...
__global__ void k_nf_long_len(const NfArgs A, NfLong *__restrict__ ent, uint32_t nq) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq) return;
    uint64_t p = A.queue[i], ncp = 0;
    uint32_t e, d[4];
    NfLong L{};
    L.start = p;
    do {
        const uint32_t l = nfc_decode(A.b, A.n, p, &e);
        if (p != L.start && !NFC_WORK(nfc_record(e))) break;
        ncp += nfc_decompose(e, nfc_record(e), d);
        p += l;
    } while (p < A.n);
    L.end = p;
    L.ncp = ncp;
    ent[i] = L;
}

// ... then a workgroup per segment, lane 0 working: decompose into ws[L.ws ..), order into the second half and
// back, compose, measure; the worth goes to the segment's tile
__global__ __launch_bounds__(64) void k_nf_long_run(const NfArgs A, NfLong *__restrict__ ent, uint32_t *__restrict__ ws,
                                                    unsigned long long *__restrict__ cnt) {
    __shared__ uint32_t s_h[256];
    if (threadIdx.x) return;
    NfLong &L = ent[blockIdx.x];
    uint32_t *a = ws + L.ws, *b2 = a + L.ncp, e, d[4];
    uint64_t m = 0;
    for (uint64_t p = L.start; p < L.end;) {
        p += nfc_decode(A.b, A.n, p, &e);
        const uint32_t k = nfc_decompose(e, nfc_record(e), d);
        for (uint32_t i = 0; i < k && m < L.ncp; i++) a[m++] = d[i];
    }
    for (uint64_t i = 0; i < m;) {  // every maximal run [i, j) of entries with ccc != 0
        if (!NFC_CCC(a[i])) { i++; continue; }
        uint64_t j = i;
        while (j < m && NFC_CCC(a[j])) j++;
        if (j - i < 16) {
            nfc_reorder(a + i, (size_t)(j - i));
        } else {  // counting sort on ccc: stable
            for (uint32_t k = 0; k < 256; k++) s_h[k] = 0;
            for (uint64_t k = i; k < j; k++) s_h[NFC_CCC(a[k]) & 255u]++;
            uint32_t acc = 0;
            for (uint32_t k = 0; k < 256; k++) { const uint32_t v = s_h[k]; s_h[k] = acc; acc += v; }
            for (uint64_t k = i; k < j; k++) b2[i + s_h[NFC_CCC(a[k]) & 255u]++] = a[k];
            for (uint64_t k = i; k < j; k++) a[k] = b2[k];
        }
        i = j;
    }
    m = nfc_compose(a, (size_t)m);
    uint64_t len = 0;
    for (uint64_t i = 0; i < m; i++) len += nfc_utf8_len(a[i]);
    L.ncomp = m;
    L.outlen = len;
    atomicAdd(&cnt[L.start / NF_TILE], (unsigned long long)len);
}

// ... and, after pass 2 noted where each begins, its bytes
__global__ __launch_bounds__(64) void k_nf_long_write(const NfLong *__restrict__ ent, const uint32_t *__restrict__ ws,
                                                      uint8_t *__restrict__ dst, uint64_t out_n) {
    if (threadIdx.x) return;
    const NfLong &L = ent[blockIdx.x];
    if (L.outpos + L.outlen > out_n) return;
    uint8_t *p = dst + L.outpos;
    for (uint64_t i = 0; i < L.ncomp; i++) p += nfc_encode(ws[L.ws + i], p);
}

}  // namespace bpeamd

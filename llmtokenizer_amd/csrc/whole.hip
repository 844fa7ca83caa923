// whole.hip -- whole-text rows (bpe_gpu.h, "Whole-text rows"); included by engine.hip after stream.hip.
//
// bpe_gpu_pack_whole, the placement.  S[k] = text_off[k] + k * w is where text k would start in the stream (a prefix
// sum already: no scan), S[T] the cells of all texts.  A text that opens a row decides which text opens the next:
//   k_whole_next    a lane per text k: next[k], the opener of the row behind the row(s) that k opens.  With the bound
//                   B = S[k] + L for a text that fits a row and B = S[k + 1] for a long one (rows of its own), it is
//                   the first j > k with S[j + 1] > B: the first text that does not fit any more, or, behind a long
//                   text, the first that has a cell at all.  A text without a cell is never a next[].  One bounded
//                   binary search (33 steps; with w > 0 a row holds at most L texts, which bounds it further);
//                   next[T] = T.  mark[k] = 1 for the first text with a cell (S[k] == 0 < S[k + 1]), else 0.
//   k_whole_double  the row openers are the orbit of that text under next[].  Round i: every marked k marks jump[k],
//                   and jump'[k] = jump[jump[k]].  Before round i, jump = next^(2^i) and the members of the orbit less
//                   than 2^i steps from its start are marked; after it, those less than 2^(i + 1) steps.  A lane that
//                   sees a mark set in the same round marks a member of the orbit early, which harms nothing.  jump'
//                   is a second buffer: written in place, jump[jump[k]] could read a pointer doubled already, reach
//                   2^i + 2^(i + 1) steps and leave the members between unmarked for good.  ceil(log2(T + 1)) rounds
//                   reach the whole orbit; the host fixes their number from T and reads nothing back between them.
//   (rocprim)       an exclusive scan of WhCount{rows k opens if marked, 1 if long} gives every opener its first row
//                   and, at T, R and n_long; an inclusive max-scan of (marked ? k : 0) gives every text its opener
//                   (k_tb_heads' idiom).  Both read mark[] and text_off through a transform iterator.
//   k_whole_place   cell[k], the cell text k's first cell takes (row * L + col, rising with k): the opener's first row
//                   times L, plus S[k] - S[opener] inside a row, or the rows of a long opener for the cell-less
//                   texts behind it.  Stays with the ids for the fill.
//   k_whole_rowcol  text_row / text_col from cell[], when the caller asks for the placement.
//
// The fill.
//   k_fill_whole    k_pack_stream's shape: consecutive cells per workgroup, TILE per step; <true> four
//                   cells per lane and one 16-byte store per output array (L a multiple of 4, outputs 16-byte
//                   aligned), <false> one cell.  The text of a cell is the last k with cell[k] <= c: one search per
//                   wave for its first cell, then every lane walks forward at most WH_WALK texts and searches for
//                   itself only past that.  A cell at or past the end of its text's cells is a pad cell.  A body cell
//                   reads ids[a + o - b]: consecutive across the lanes inside a text.  No LDS, no atomics.

namespace bpeamd {

constexpr uint32_t WH_T = 256;         // threads per workgroup of every kernel here
constexpr uint32_t WH_GRID = 1024;     // workgroups of the placement kernels at most (more texts: several per lane)
constexpr uint32_t WH_FILL_GRID = 2048;  // workgroups of k_fill_whole at most (more cells: several steps per workgroup)
constexpr uint32_t WH_VEC = 4;         // cells a lane of k_fill_whole<true> takes per step
constexpr uint32_t WH_WALK = 4;        // texts a lane walks forward before it searches for itself

struct WhCount {
    uint64_t rows, longs;
};
struct WhPlus {
    __host__ __device__ WhCount operator()(const WhCount &x, const WhCount &y) const {
        return WhCount{x.rows + y.rows, x.longs + y.longs};
    }
};

// the scans' inputs, read where they lie (k == T: nothing)
struct WhCountOf {
    const uint8_t *mark;
    const uint64_t *text_off;
    uint64_t T, w, L;
    __device__ WhCount operator()(uint64_t k) const {
        if (k >= T) return WhCount{0, 0};
        const uint64_t wk = text_off[k + 1] - text_off[k] + w;
        const uint64_t rows = wk > L ? (wk + L - 1) / L : 1;
        return WhCount{mark[k] ? rows : 0, wk > L ? 1ull : 0ull};
    }
};
struct WhOpenerOf {
    const uint8_t *mark;
    uint64_t T;
    __device__ uint32_t operator()(uint64_t k) const { return k < T && mark[k] ? (uint32_t)k : 0u; }
};

// jump0 / jump1: T + 1 entries each (both get the sentinel), mark: T
__global__ __launch_bounds__(WH_T) void k_whole_next(const uint64_t *__restrict__ text_off, uint64_t T, uint64_t w, uint64_t L,
                                                     uint32_t *__restrict__ jump0, uint32_t *__restrict__ jump1,
                                                     uint8_t *__restrict__ mark) {
    const uint64_t stride = (uint64_t)gridDim.x * WH_T;
    for (uint64_t k = (uint64_t)blockIdx.x * WH_T + threadIdx.x; k <= T; k += stride) {
        if (k == T) {
            jump0[T] = (uint32_t)T;
            jump1[T] = (uint32_t)T;
            continue;
        }
        const uint64_t s0 = text_off[k] + k * w, s1 = text_off[k + 1] + (k + 1) * w;
        const uint64_t bound = s1 - s0 > L ? s1 : s0 + L;
        // S[lo + 1] <= bound < S[hi + 1], with S[T + 1] = infinity
        uint64_t lo = k, hi = T;
        if (w && T - k > L + 1) hi = k + L + 1;  // (every text has a cell: L + 1 of them exceed a row)
        for (uint32_t step = 0; step < 33; step++) {
            if (hi - lo <= 1) break;
            const uint64_t mid = lo + (hi - lo) / 2;  // (k < mid < T)
            if (text_off[mid + 1] + (mid + 1) * w <= bound) lo = mid;
            else hi = mid;
        }
        jump0[k] = (uint32_t)hi;
        mark[k] = s0 == 0 && s1 > 0;
    }
}

__global__ __launch_bounds__(WH_T) void k_whole_double(uint8_t *mark, const uint32_t *__restrict__ jin,
                                                       uint32_t *__restrict__ jout, uint64_t T) {
    const uint64_t stride = (uint64_t)gridDim.x * WH_T;
    for (uint64_t k = (uint64_t)blockIdx.x * WH_T + threadIdx.x; k < T; k += stride) {
        const uint32_t j = jin[k];  // (j <= T)
        if (j < T && mark[k]) mark[j] = 1;
        jout[k] = jin[j];
    }
}

// first[k]: the scanned WhCount (T + 1 entries), opener[k]: the max-scan (T entries); cell: T entries
__global__ __launch_bounds__(WH_T) void k_whole_place(const uint64_t *__restrict__ text_off, uint64_t T, uint64_t w, uint64_t L,
                                                      const uint8_t *__restrict__ mark, const WhCount *__restrict__ first,
                                                      const uint32_t *__restrict__ opener, uint64_t *__restrict__ cell) {
    const uint64_t stride = (uint64_t)gridDim.x * WH_T;
    for (uint64_t k = (uint64_t)blockIdx.x * WH_T + threadIdx.x; k < T; k += stride) {
        const uint64_t o = opener[k];  // (o <= k)
        uint64_t p = 0;                // (no opener at or before k: no text up to k has a cell)
        if (mark[o]) {
            const uint64_t so = text_off[o] + o * w, wo = text_off[o + 1] + (o + 1) * w - so;
            p = first[o].rows * L;
            if (wo <= L) p += text_off[k] + k * w - so;     // in the opener's row, or just behind it when that is full
            else if (k > o) p += (wo + L - 1) / L * L;      // a text without a cell behind a long text's rows
        }
        cell[k] = p;
    }
}

__global__ __launch_bounds__(WH_T) void k_whole_rowcol(const uint64_t *__restrict__ cell, uint64_t T, uint64_t L,
                                                       uint32_t *__restrict__ text_row, uint32_t *__restrict__ text_col) {
    const uint64_t stride = (uint64_t)gridDim.x * WH_T;
    for (uint64_t k = (uint64_t)blockIdx.x * WH_T + threadIdx.x; k < T; k += stride) {
        const uint64_t p = cell[k];
        if (text_row) text_row[k] = (uint32_t)(p / L);
        if (text_col) text_col[k] = (uint32_t)(p % L);
    }
}

// the last k with cell[k] <= c (T >= 1 and cell[0] == 0 <= c).  33 steps reach T = 2^32.
__device__ inline uint64_t wh_find(const uint64_t *__restrict__ cell, uint64_t T, uint64_t c) {
    uint64_t lo = 0, hi = T;  // cell[lo] <= c < cell[hi], cell[T] = infinity
    for (uint32_t step = 0; step < 33; step++) {
        if (hi - lo <= 1) break;
        const uint64_t mid = lo + (hi - lo) / 2;  // (0 < mid < T)
        if (cell[mid] <= c) lo = mid;
        else hi = mid;
    }
    return lo;
}

// what a lane knows of its text k: p = cell[k], pn = cell[k + 1] (infinity for the last text), a = text_off[k],
// z = text_off[k + 1]
struct WhText {
    uint64_t k, p, pn, a, z;
};
__device__ inline void wh_load(const uint64_t *__restrict__ cell, const uint64_t *__restrict__ text_off, uint64_t T, uint64_t k,
                               WhText &t) {
    t.k = k;
    t.p = cell[k];
    t.pn = k + 1 < T ? cell[k + 1] : ~0ull;
    t.a = text_off[k];
    t.z = text_off[k + 1];
}
// cell[t.k] <= c: moved on to the last such k
__device__ inline void wh_forward(const uint64_t *__restrict__ cell, const uint64_t *__restrict__ text_off, uint64_t T, uint64_t c,
                                  WhText &t) {
    uint32_t steps = 0;
    while (steps < WH_WALK && t.pn <= c) {  // (pn <= c means k + 1 < T)
        t.k++;
        t.p = t.pn;
        t.pn = t.k + 1 < T ? cell[t.k + 1] : ~0ull;
        t.a = t.z;
        t.z = text_off[t.k + 1];
        steps++;
    }
    if (t.pn <= c) wh_load(cell, text_off, T, wh_find(cell, T, c), t);
}

// cells = R * L (> 0, so T >= 1); workgroup g takes the cells [g * steps * TILE, (g + 1) * steps * TILE), TILE of them
// per step; b: a BOS opens a text (w - b: an EOS closes it); seg, pos: may be null
template <bool VEC>
__global__ __launch_bounds__(WH_T) void k_fill_whole(const uint32_t *__restrict__ ids, uint64_t n,
                                                     const uint64_t *__restrict__ text_off,
                                                     const uint64_t *__restrict__ cell, uint64_t T, uint64_t cells,
                                                     uint64_t steps, uint32_t L, uint32_t w, uint32_t b, uint32_t bos,
                                                     uint32_t eos, uint32_t pad, uint32_t *__restrict__ rows,
                                                     uint32_t *__restrict__ seg, uint32_t *__restrict__ pos) {
    constexpr uint32_t PER = VEC ? WH_VEC : 1;
    constexpr uint32_t TILE = WH_T * PER;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t first = (uint64_t)blockIdx.x * steps * TILE;
    const uint64_t last = first + steps * TILE < cells ? first + steps * TILE : cells;
    const uint32_t tile_col = TILE % L;
    uint64_t c = first + (uint64_t)threadIdx.x * PER;
    if (c >= last) return;             // (VEC: L and c are multiples of 4, so col + 3 < L and c + 3 < cells)
    uint32_t col = (uint32_t)(c % L);
    // the text of the wave's first cell, once: from step to step a lane's k only moves forward
    WhText t;
    wh_load(cell, text_off, T, wh_find(cell, T, c - (uint64_t)lane * PER), t);
    for (; c < last; c += TILE) {
        uint32_t v[PER], sg[PER], ps[PER];
#pragma unroll
        for (uint32_t j = 0; j < PER; j++) {
            const uint64_t cj = c + j;
            wh_forward(cell, text_off, T, cj, t);
            const uint64_t o = cj - t.p, row0 = cj - (col + j);
            const uint64_t i = t.a + o - b;  // (only read when o >= b)
            v[j] = pad;
            sg[j] = 0xFFFFFFFFu;
            ps[j] = 0;
            if (o < t.z - t.a + w) {  // one of the text's cells
                if (b && o == 0) v[j] = bos;
                else if (i >= t.z) v[j] = eos;  // (past the body there is an EOS)
                else if (i < n) v[j] = ids[i];
                sg[j] = (uint32_t)t.k;
                ps[j] = (uint32_t)(cj - (t.p > row0 ? t.p : row0));
            }
        }
        if constexpr (VEC) {
            *(uint4 *)(rows + c) = make_uint4(v[0], v[1], v[2], v[3]);
            if (seg) *(uint4 *)(seg + c) = make_uint4(sg[0], sg[1], sg[2], sg[3]);
            if (pos) *(uint4 *)(pos + c) = make_uint4(ps[0], ps[1], ps[2], ps[3]);
        } else {
            rows[c] = v[0];
            if (seg) seg[c] = sg[0];
            if (pos) pos[c] = ps[0];
        }
        col += tile_col;
        if (col >= L) col -= L;
    }
}

}  // namespace bpeamd

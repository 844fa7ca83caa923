// stream.hip -- packed streams (bpe_gpu.h, "Packed streams"); included by engine.hip after spans.hip.
//
// bpe_gpu_pack_stream:
//   k_pack_stream  a lane per cell c of the R * L cells: rows[c], seg[c] and pos[c] of the stream that joins the texts'
//                  ids with their BOS / EOS.  Text k starts at S[k] = text_off[k] + k * w (text_off is a prefix sum
//                  already: no scan), and the text of cell c is the last k with S[k] <= c, which is the text that owns
//                  the cell among equal S (empty texts with w == 0) too.  A workgroup takes consecutive cells, TILE
//                  (256 lanes' cells) per step and `steps` steps: one step while the cells fit STR_GRID workgroups,
//                  more past that.  The search is k_spans': one per wave for its first cell, once; every lane then
//                  walks forward at most STR_WALK texts (a wave's 256 cells lie in one or two texts as a rule) and
//                  searches for itself only past that, and so it goes on from one cell of a lane to the next and from
//                  one step to the next, a tile further on.  (A grid-stride loop, a search per wave and step, spent
//                  its time in the searches' dependent loads: DESIGN 7.8.)  A body cell reads ids[c - k * w - b]:
//                  consecutive across the lanes inside a text.  <true>: four consecutive cells per lane and one
//                  16-byte store per output array, when L is a multiple of 4 (a lane's four cells then lie in one row)
//                  and every output is 16-byte aligned; <false>: one cell per lane.  The column of a cell comes from
//                  one division per lane, then moves with the tile's remainder.  No LDS, no atomics, no scratch; no
//                  loop runs by a text's length or by the number of texts.

namespace bpeamd {

constexpr uint32_t STR_T = 256;      // threads per workgroup of k_pack_stream
constexpr uint32_t STR_GRID = 2048;  // workgroups at most (more cells: several steps per workgroup)
constexpr uint32_t STR_VEC = 4;      // cells a lane of k_pack_stream<true> takes per step
constexpr uint32_t STR_WALK = 4;     // texts a lane walks forward before it searches for itself

// the last k with S[k] <= c, for c < S[T] (so k < T; S[0] == 0 <= c).  33 steps reach T = 2^32.
__device__ inline uint64_t str_find(const uint64_t *__restrict__ text_off, uint64_t T, uint64_t w, uint64_t c) {
    uint64_t lo = 0, hi = T;  // S[lo] <= c < S[hi]
    for (uint32_t step = 0; step < 33; step++) {
        if (hi - lo <= 1) break;
        const uint64_t mid = lo + (hi - lo) / 2;  // (0 < mid < T)
        if (text_off[mid] + mid * w <= c) lo = mid;
        else hi = mid;
    }
    return lo;
}

// k with S[k] <= c < S[T], a = text_off[k], z = text_off[k + 1]: moved on to the last such k
__device__ inline void str_forward(const uint64_t *__restrict__ text_off, uint64_t T, uint64_t w, uint64_t c, uint64_t &k,
                                   uint64_t &a, uint64_t &z) {
    uint32_t steps = 0;
    // (S[k + 1] <= c < S[T] means k + 1 < T; it is compared all the same, before k + 2 is an index)
    while (steps < STR_WALK && k + 1 < T && z + (k + 1) * w <= c) {
        k++;
        a = z;
        z = text_off[k + 1];
        steps++;
    }
    if (k + 1 < T && z + (k + 1) * w <= c) {
        k = str_find(text_off, T, w, c);
        a = text_off[k];
        z = text_off[k + 1];
    }
}

// cells = R * L, N = n + T * w the stream's cells; workgroup g takes the cells [g * steps * TILE, (g + 1) * steps * TILE),
// TILE of them per step; b: a BOS opens a text (w - b: an EOS closes it); seg, pos: may be null
template <bool VEC>
__global__ __launch_bounds__(STR_T) void k_pack_stream(const uint32_t *__restrict__ ids, uint64_t n,
                                                       const uint64_t *__restrict__ text_off, uint64_t T, uint64_t N,
                                                       uint64_t cells, uint64_t steps, uint32_t L, uint32_t w, uint32_t b,
                                                       uint32_t bos, uint32_t eos, uint32_t pad, uint32_t *__restrict__ rows,
                                                       uint32_t *__restrict__ seg, uint32_t *__restrict__ pos) {
    constexpr uint32_t PER = VEC ? STR_VEC : 1;
    constexpr uint32_t TILE = STR_T * PER;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t first = (uint64_t)blockIdx.x * steps * TILE;
    const uint64_t last = first + steps * TILE < cells ? first + steps * TILE : cells;
    const uint32_t tile_col = TILE % L;
    uint64_t c = first + (uint64_t)threadIdx.x * PER;
    uint32_t col = (uint32_t)(c % L);  // (VEC: L and c are multiples of 4, so col + 3 < L and c + 3 < cells)
    // the text of the wave's first cell, once: from step to step a lane's k only moves forward
    uint64_t k = 0, a = 0, z = 0;
    if (c < N) {  // (the wave's first cell is then in the stream too; a lane past the stream stays past it)
        k = str_find(text_off, T, w, c - (uint64_t)lane * PER);
        a = text_off[k];
        z = text_off[k + 1];
    }
    for (; c < last; c += TILE) {
        uint32_t v[PER], sg[PER], ps[PER];
#pragma unroll
        for (uint32_t j = 0; j < PER; j++) {
            const uint64_t cj = c + j;
            v[j] = pad;
            sg[j] = 0xFFFFFFFFu;
            ps[j] = 0;
            if (cj < N) {
                str_forward(text_off, T, w, cj, k, a, z);
                const uint64_t s = a + k * w, o = cj - s, row0 = cj - (col + j);
                const uint64_t i = a + o - b;  // (only read when o >= b)
                if (b && o == 0) v[j] = bos;
                else if (i >= z) v[j] = eos;  // (o < z - a + w: past the body there is an EOS)
                else if (i < n) v[j] = ids[i];
                sg[j] = (uint32_t)k;
                ps[j] = (uint32_t)(cj - (s > row0 ? s : row0));
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

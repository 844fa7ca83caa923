// texts.hip -- text batches (bpe_gpu.h, "Text batches"); included by engine.hip after vocab.hip.
//
// A context loaded by bpe_gpu_load_texts holds every text followed by one gap byte; boff[0 .. T] are the texts'
// byte offsets in the plain join, so gap k is resident position boff[k + 1] + k.  The split (pieces.hip):
//   k_text_breaks  a thread per gap: what k_sp_find does for a match.  The gap's bit goes into the cover bitmap
//                  (atomicOr: a word may hold a special's bits too) and (position << 8 | SX_BREAK) into the match
//                  list behind the specials' matches, at index k: no counter, the host sized the list for them.
//                  k_sp_patch, the recount, the sort and k_sp_pieces then run as they are (a break reads as a
//                  one-byte match: SpSet::lenj[SX_BREAK] is 0, a text batch takes at most 255 specials).
//   k_text_pieces  a thread per gap: its piece index, a binary search of the emitted offsets.
//   k_text_compact the offsets without the break pieces, each moved down by the gaps before it (the plain join's
//                  coordinates); bpe_gpu_encode_split runs it again over the id offsets, nothing subtracted.
// The encode post-pass (special.hip) removes every id of a break piece; then
//   k_text_off     text_off[k] = the id offset at which break k - 1's ids vanished, text_off[0] = 0.
// Rows (bpe_gpu_pack_texts):
//   k_pack_rows    out[row][col] = an id of text `row` or the pad.  A workgroup is PK_T threads shaped (bx, by),
//                  bx a power of two: x runs along a row and y over rows, so row and column come from the thread
//                  and block indices with no division, a wave's lanes are consecutive in a row (both the read of
//                  the ids and the write of the row coalesce) and short rows still fill a workgroup.  <true>: four
//                  columns per lane and one 16-byte store, when row_len is a multiple of 4 and out is 16-byte
//                  aligned (the ids are read one by one: a text starts at any id); <false>: one column per lane.
//                  Rows past gridDim.y * by are walked in grid strides.  No atomics, no LDS, no scratch; no loop
//                  runs by a text's length.

namespace bpeamd {

constexpr uint32_t PK_T = 256;             // threads per workgroup of k_pack_rows
constexpr uint32_t PK_BLOCKS = 1u << 20;   // workgroups at most (more rows are walked in grid strides)
constexpr uint32_t PK_ROW_MAX = 1u << 24;  // row_len at most

__global__ __launch_bounds__(SX_T) void k_text_breaks(const uint64_t *__restrict__ boff, uint64_t T,
                                                      uint32_t *__restrict__ cover, unsigned long long *__restrict__ list) {
    for (uint64_t k = (uint64_t)blockIdx.x * SX_T + threadIdx.x; k < T; k += (uint64_t)gridDim.x * SX_T) {
        const uint64_t g = boff[k + 1] + k;
        atomicOr(&cover[g >> 5], 1u << (g & 31u));
        list[k] = ((unsigned long long)g << 8) | SX_BREAK;
    }
}

// bpiece[k] = the piece that is gap k: off[bpiece[k]] == boff[k + 1] + k (else *bad; the patch made it a start)
__global__ __launch_bounds__(SX_T) void k_text_pieces(const uint64_t *__restrict__ boff, uint64_t T,
                                                      const uint64_t *__restrict__ off, uint64_t P,
                                                      uint64_t *__restrict__ bpiece, uint32_t *__restrict__ bad) {
    for (uint64_t k = (uint64_t)blockIdx.x * SX_T + threadIdx.x; k < T; k += (uint64_t)gridDim.x * SX_T) {
        const uint64_t g = boff[k + 1] + k, p = sx_lower(off, P, g, 0);
        if (p >= P || off[p] != g || off[p + 1] != g + 1) *bad = 1u;
        bpiece[k] = p;
    }
}

// out[p - (breaks before p)] = in[p] - (sub ? breaks before p : 0) for every p in [0, P] that is no break piece
__global__ __launch_bounds__(SX_T) void k_text_compact(const uint64_t *__restrict__ in, uint64_t P,
                                                       const uint64_t *__restrict__ bpiece, uint64_t T, int sub,
                                                       uint64_t *__restrict__ out) {
    for (uint64_t p = (uint64_t)blockIdx.x * SX_T + threadIdx.x; p <= P; p += (uint64_t)gridDim.x * SX_T) {
        const uint64_t nb = sx_lower(bpiece, T, p, 0);
        if (nb < T && bpiece[nb] == p) continue;
        out[p - nb] = in[p] - (sub ? nb : 0);
    }
}

// id_off: the id offsets with the break pieces still in them, a break piece empty
__global__ __launch_bounds__(SX_T) void k_text_off(const uint64_t *__restrict__ id_off, const uint64_t *__restrict__ bpiece,
                                                   uint64_t T, uint64_t *__restrict__ text_off) {
    for (uint64_t k = (uint64_t)blockIdx.x * SX_T + threadIdx.x; k <= T; k += (uint64_t)gridDim.x * SX_T)
        text_off[k] = k ? id_off[bpiece[k - 1]] : 0;
}

template <bool VEC>
__global__ __launch_bounds__(PK_T) void k_pack_rows(const uint32_t *__restrict__ ids, const uint64_t *__restrict__ text_off,
                                                    uint64_t T, uint32_t row_len, uint32_t pad, uint32_t side,
                                                    uint32_t *__restrict__ out, uint32_t *__restrict__ lens) {
    constexpr uint32_t PER = VEC ? 4 : 1;
    const uint64_t col = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * PER;
    if (col >= row_len) return;  // (VEC: row_len is a multiple of 4, so col + 3 < row_len)
    for (uint64_t row = (uint64_t)blockIdx.y * blockDim.y + threadIdx.y; row < T; row += (uint64_t)gridDim.y * blockDim.y) {
        const uint64_t a = text_off[row], b = text_off[row + 1], len = b - a;
        const uint32_t keep = len < row_len ? (uint32_t)len : row_len;
        const uint64_t src = (side && len > row_len ? b - row_len : a) + col;
        if (col == 0 && lens) lens[row] = keep;
        uint32_t *dst = out + row * row_len + col;
        if (VEC) {
            uint4 v;
            v.x = col + 0 < keep ? ids[src + 0] : pad;
            v.y = col + 1 < keep ? ids[src + 1] : pad;
            v.z = col + 2 < keep ? ids[src + 2] : pad;
            v.w = col + 3 < keep ? ids[src + 3] : pad;
            *(uint4 *)dst = v;
        } else {
            *dst = col < keep ? ids[src] : pad;
        }
    }
}

}  // namespace bpeamd

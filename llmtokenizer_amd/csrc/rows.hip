// rows.hip -- rows back to texts (bpe_gpu.h, "Rows back to texts"); included by engine.hip after stream.hip.
//
// bpe_gpu_unpack_rows:
//   k_rows_bounds  a wave per row, ROWS_PER_WG rows per workgroup, in a grid-stride over the rows under ROWS_GRID
//                  workgroups: (a, z) of the row, the start and the end of its text, and cnt, the cells it keeps.  The
//                  wave reads its row in consecutive steps of 64 cells, a cell per lane (<CELL, false>), or of 256, four
//                  per lane in one 16-byte load (4-byte cells) or two (8-byte cells) (<CELL, true>: when the first cell
//                  and the rows' stride in bytes are 16-byte aligned and L is a multiple of 4, so that a lane's four
//                  cells lie in one row and in one aligned vector).  First the leading pads: a ballot of "is no pad" per
//                  cell of a lane, the first set bit is the start, and the loop leaves at the step that holds it.  Then,
//                  from that step on, a ballot of "ends the text" (a stop id, a pad, the window's end) and one of "is
//                  kept" (in [a, window), no stop, not in the skip list); the first set bit of the former is the end, the
//                  kept count the popcount of the latter below it, and the loop leaves there.  A wave owns a row, its row
//                  index and its window are made scalar (readfirstlane), so every trip count is wave-uniform and no
//                  ballot sits under divergent control flow.  The loads of the next step go out before this step's cells
//                  are judged (one step ahead, held in registers): a wave has one row and its steps depend on each
//                  other, so without that it would wait out a memory latency per step with nothing in flight.  The stop
//                  list (at most 8 ids) and the pad come by value in the kernel's arguments; the sorted skip list (at
//                  most 256 ids, filled up to a power of two with its largest) is copied to LDS once per workgroup and
//                  searched in log2 of that many steps, at most 8; without one no LDS is touched.  Two error words, each the lowest offending row by an atomic min: a window
//                  above L (the row is then not read), a kept 8-byte cell that is no id.
//   rocprim::exclusive_scan of cnt: text_off.
//   k_rows_gather  the same shape over [a, z) of every row: ids[text_off[k] + rank] = the kept cell.  Without a skip list
//                  rank = c - a, a plain coalesced copy with no ballot in it; with one the rank of a lane's cell is
//                  base + the kept cells of the step in front of it (popcounts of the keep ballots below the lane), and
//                  base moves on by the step's kept count.
//   No loop runs by anything but L; no atomics but the two error words; no scratch.

namespace bpeamd {

constexpr uint32_t ROWS_T = 256;                // threads per workgroup of k_rows_bounds / k_rows_gather
constexpr uint32_t ROWS_PER_WG = ROWS_T / 64;   // rows (waves) per workgroup
constexpr uint32_t ROWS_GRID = 2048;            // workgroups at most (more rows: a wave goes on to further rows)
constexpr uint32_t ROWS_VEC = 4;                // cells a lane of the vector variants takes per step
constexpr uint32_t ROWS_SKIP_MAX = 256;         // ids of the skip list at most (BPE_ROWS_SKIP_MAX)
constexpr unsigned long long ROWS_NO_ROW = ~0ull;  // an error word that names no row

// what the kernels need of a bpe_gpu_rows, by value
struct RowsDesc {
    uint32_t pad_on, pad, n_stop, stop[8];
    uint32_t skip_steps;  // 0: no skip list; else the list holds 1 << (skip_steps - 1) ids
};

// PER cells of lane `lane` from c0 on: v[j] = cell c0 + lane * PER + j of the row, read when it lies below `lim`
// (VEC: lim is L, a multiple of 4, and the lane's four cells are read together or not at all)
template <typename CELL, bool VEC>
__device__ inline void rows_load(const CELL *__restrict__ row, uint32_t c, uint32_t lim, CELL *v) {
    if constexpr (!VEC) {
        v[0] = c < lim ? row[c] : (CELL)0;
    } else if constexpr (sizeof(CELL) == 4) {
        uint4 q = make_uint4(0, 0, 0, 0);
        if (c < lim) q = *(const uint4 *)(row + c);
        v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
    } else {
        ulonglong2 q0 = make_ulonglong2(0, 0), q1 = q0;
        if (c < lim) {
            q0 = *(const ulonglong2 *)(row + c);
            q1 = *(const ulonglong2 *)(row + c + 2);
        }
        v[0] = (CELL)q0.x, v[1] = (CELL)q0.y, v[2] = (CELL)q1.x, v[3] = (CELL)q1.y;
    }
}

// the cells of the step from c0 on, asked for while the step before it is judged: read only when the step begins
// below `end` (wave-uniform), so that no load goes out for a step the loop will not make
template <typename CELL, bool VEC>
__device__ inline void rows_next(const CELL *__restrict__ row, uint32_t c0, uint32_t end, uint32_t lane, uint32_t L, CELL *v) {
    constexpr uint32_t PER = VEC ? ROWS_VEC : 1;
    rows_load<CELL, VEC>(row, c0 + lane * PER, c0 < end ? L : 0, v);
}

// is the cell an id (an 8-byte cell: a signed value in 0 .. 2^32 - 1)?
template <typename CELL>
__device__ inline bool rows_is_id(CELL v) {
    if constexpr (sizeof(CELL) == 4) return true;
    else return (unsigned long long)v <= 0xFFFFFFFFull;
}

template <typename CELL>
__device__ inline bool rows_is_pad(const RowsDesc &d, CELL v) {
    return d.pad_on && rows_is_id(v) && (uint32_t)v == d.pad;
}

template <typename CELL>
__device__ inline bool rows_is_stop(const RowsDesc &d, CELL v) {
    if (!rows_is_id(v)) return false;
    const uint32_t id = (uint32_t)v;
    bool hit = d.pad_on && id == d.pad;
#pragma unroll
    for (uint32_t j = 0; j < 8; j++) hit |= j < d.n_stop && id == d.stop[j];
    return hit;
}

// is the id in the sorted list of 1 << (steps - 1) ids in LDS?  steps - 1 halvings, at most 8
__device__ inline bool rows_in_skip(const uint32_t *s_skip, uint32_t steps, uint32_t id) {
    uint32_t pos = 0;
    for (uint32_t half = (1u << (steps - 1)) >> 1; half; half >>= 1)
        if (s_skip[pos + half - 1] < id) pos += half;
    return s_skip[pos] == id;
}

// the lanes below lane n of a wave (n in 0 .. 64)
__device__ inline unsigned long long rows_below(uint32_t n) { return n >= 64 ? ~0ull : (1ull << n) - 1; }

// the first cell in lane-major order (cell lane * PER + j is bit `lane` of m[j]) with its bit set, or 64 * PER
template <uint32_t PER>
__device__ inline uint32_t rows_first(const unsigned long long *m) {
    unsigned long long any = 0;
#pragma unroll
    for (uint32_t j = 0; j < PER; j++) any |= m[j];
    if (!any) return 64 * PER;
    const uint32_t lane = (uint32_t)__ffsll((long long)any) - 1;
    uint32_t j = 0;
#pragma unroll
    for (uint32_t t = PER; t-- > 0;)
        if ((m[t] >> lane) & 1ull) j = t;
    return lane * PER + j;
}

// the set bits of m[.] whose cell lies below cell e (e in 0 .. 64 * PER)
template <uint32_t PER>
__device__ inline uint32_t rows_count_below(const unsigned long long *m, uint32_t e) {
    uint32_t n = 0;
#pragma unroll
    for (uint32_t j = 0; j < PER; j++)  // (cell lane * PER + j < e: lane < ceil((e - j) / PER))
        n += (uint32_t)__popcll(m[j] & rows_below(e > j ? (e - j + PER - 1) / PER : 0));
    return n;
}

__device__ inline void rows_skip_to_lds(uint32_t *s_skip, const uint32_t *__restrict__ skip, uint32_t steps) {
    if (steps) {  // (uniform over the workgroup: a kernel argument)
        if (threadIdx.x < (1u << (steps - 1))) s_skip[threadIdx.x] = skip[threadIdx.x];
        __syncthreads();
    }
}

// rows: the first cell of row 0; stride: cells from row to row; lens: the windows or null; skip: the sorted list (read
// when d.skip_steps); bounds[2 k], bounds[2 k + 1] = (a, z), cnt[k] = the kept cells; err[0], err[1]: the lowest row
// with a window above L / with a kept cell that is no id (set to ROWS_NO_ROW before the launch)
template <typename CELL, bool VEC>
__global__ __launch_bounds__(ROWS_T) void k_rows_bounds(const CELL *__restrict__ rows, uint64_t B, uint32_t L, uint64_t stride,
                                                        const uint32_t *__restrict__ lens, RowsDesc d,
                                                        const uint32_t *__restrict__ skip, uint32_t *__restrict__ bounds,
                                                        uint64_t *__restrict__ cnt, unsigned long long *__restrict__ err) {
    constexpr uint32_t PER = VEC ? ROWS_VEC : 1, STEP = 64 * PER;
    __shared__ uint32_t s_skip[ROWS_SKIP_MAX];
    rows_skip_to_lds(s_skip, skip, d.skip_steps);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (uint64_t k = (uint64_t)blockIdx.x * ROWS_PER_WG + wave; k < B; k += (uint64_t)gridDim.x * ROWS_PER_WG) {
        const uint32_t win = lens ? __builtin_amdgcn_readfirstlane(lens[k]) : L;
        if (win > L) {  // (the row is not read: the call fails)
            if (lane == 0) {
                atomicMin(err, (unsigned long long)k);
                bounds[2 * k] = bounds[2 * k + 1] = 0;
                cnt[k] = 0;
            }
            continue;
        }
        const CELL *row = rows + k * stride;
        // the start: the first window cell that is no pad
        uint32_t a = 0;
        if (d.pad_on) {
            a = win;
            for (uint32_t c0 = 0; c0 < win; c0 += STEP) {
                CELL v[PER];
                unsigned long long m[PER];
                rows_load<CELL, VEC>(row, c0 + lane * PER, L, v);
#pragma unroll
                for (uint32_t j = 0; j < PER; j++) m[j] = __ballot(c0 + lane * PER + j >= win || !rows_is_pad(d, v[j]));
                const uint32_t f = rows_first<PER>(m);
                if (f < STEP) {
                    a = c0 + f < win ? c0 + f : win;
                    break;
                }
            }
        }
        // the end: the first cell from a on that is a stop or a pad; the kept cells in front of it
        uint32_t z = win, kept = 0;
        bool bad = false;
        CELL v[PER], nx[PER];
        uint32_t c0 = a - a % STEP;
        rows_load<CELL, VEC>(row, c0 + lane * PER, L, v);
        for (; c0 < win; c0 += STEP) {
            unsigned long long ends[PER], keep[PER], noid[PER];
            rows_next<CELL, VEC>(row, c0 + STEP, win, lane, L, nx);
#pragma unroll
            for (uint32_t j = 0; j < PER; j++) {
                const uint32_t c = c0 + lane * PER + j;
                const bool in = c >= a && c < win, stop = rows_is_stop(d, v[j]);
                const bool skipped = d.skip_steps && rows_is_id(v[j]) && rows_in_skip(s_skip, d.skip_steps, (uint32_t)v[j]);
                ends[j] = __ballot(c >= win || (in && stop));
                keep[j] = __ballot(in && !stop && !skipped);
                noid[j] = __ballot(in && !rows_is_id(v[j]));
            }
            const uint32_t e = rows_first<PER>(ends);  // (STEP: the text goes on into the next step)
            kept += rows_count_below<PER>(keep, e);
            bad |= rows_count_below<PER>(noid, e) != 0;
            if (e < STEP) {
                z = c0 + e;
                break;
            }
#pragma unroll
            for (uint32_t j = 0; j < PER; j++) v[j] = nx[j];
        }
        if (lane == 0) {
            if (bad) atomicMin(err + 1, (unsigned long long)k);
            bounds[2 * k] = a;
            bounds[2 * k + 1] = z;
            cnt[k] = kept;
        }
    }
}

// ids[text_off[k] ..) = the kept cells of [a, z) of row k, for the bounds and the offsets k_rows_bounds and the scan left
template <typename CELL, bool VEC>
__global__ __launch_bounds__(ROWS_T) void k_rows_gather(const CELL *__restrict__ rows, uint64_t B, uint32_t L, uint64_t stride,
                                                        RowsDesc d, const uint32_t *__restrict__ skip,
                                                        const uint32_t *__restrict__ bounds,
                                                        const uint64_t *__restrict__ text_off, uint32_t *__restrict__ ids) {
    constexpr uint32_t PER = VEC ? ROWS_VEC : 1, STEP = 64 * PER;
    __shared__ uint32_t s_skip[ROWS_SKIP_MAX];
    rows_skip_to_lds(s_skip, skip, d.skip_steps);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (uint64_t k = (uint64_t)blockIdx.x * ROWS_PER_WG + wave; k < B; k += (uint64_t)gridDim.x * ROWS_PER_WG) {
        const uint32_t a = __builtin_amdgcn_readfirstlane(bounds[2 * k]), z = __builtin_amdgcn_readfirstlane(bounds[2 * k + 1]);
        const CELL *row = rows + k * stride;
        uint32_t *out = ids + text_off[k];
        CELL v[PER], nx[PER];
        uint32_t c0 = a - a % STEP;
        rows_load<CELL, VEC>(row, c0 + lane * PER, L, v);
        if (!d.skip_steps) {  // every cell of [a, z) is kept: a copy
            for (; c0 < z; c0 += STEP) {
                rows_next<CELL, VEC>(row, c0 + STEP, z, lane, L, nx);
#pragma unroll
                for (uint32_t j = 0; j < PER; j++) {
                    const uint32_t c = c0 + lane * PER + j;
                    if (c >= a && c < z) out[c - a] = (uint32_t)v[j];
                    v[j] = nx[j];
                }
            }
            continue;
        }
        uint32_t base = 0;  // the kept cells of the steps before this one
        for (; c0 < z; c0 += STEP) {
            unsigned long long keep[PER];
            bool mine[PER];
            rows_next<CELL, VEC>(row, c0 + STEP, z, lane, L, nx);
#pragma unroll
            for (uint32_t j = 0; j < PER; j++) {
                const uint32_t c = c0 + lane * PER + j;
                mine[j] = c >= a && c < z && !(rows_is_id(v[j]) && rows_in_skip(s_skip, d.skip_steps, (uint32_t)v[j]));
                keep[j] = __ballot(mine[j]);
            }
            uint32_t rank = base;  // of the lane's first cell: the kept cells of the lanes below
#pragma unroll
            for (uint32_t j = 0; j < PER; j++) rank += (uint32_t)__popcll(keep[j] & rows_below(lane));
#pragma unroll
            for (uint32_t j = 0; j < PER; j++) {
                if (mine[j]) out[rank++] = (uint32_t)v[j];
                base += (uint32_t)__popcll(keep[j]);
                v[j] = nx[j];
            }
        }
    }
}

}  // namespace bpeamd

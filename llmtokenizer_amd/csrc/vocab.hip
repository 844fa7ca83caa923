// vocab.hip -- vocabulary ids (bpe_gpu.h, "Vocabularies"); included by engine.hip after special.hip.
//
//   k_ids_map    ids[i] = fwd[ids[i]] in place over the resident ids of an encode (bpe_gpu_map_ids): internal
//                ids become the vocabulary's.  fwd has 256 + n_merges + n_specials entries.
//   k_ids_unmap  ids[i] = inv[ids[i]] over ids the caller supplied (decode_run, before k_dec_check): vocabulary
//                ids become internal ones.  inv has (largest vocabulary id + 1) entries, 0xFFFFFFFF for a hole.
//
// Both are one body.  An id is compared with the table's length before it is used as an index, always: an id at
// or past it (and, in the inverse table, a hole) ORs bit 0 of *err and its slot gets 0, so nothing downstream
// indexes with it.  Neither table holds 0xFFFFFFFF for a valid entry (vocabulary ids are below 2^24, internal
// ids below 256 + 2^24 + 256), which is what lets the forward lookup share the hole test.
//
// Memory: 16 bytes (four ids) per lane and access, a grid-strided loop over the 16-byte-aligned middle of the
// array; the at most three ids before it and the at most three after it are moved one by one by the first six
// threads of workgroup 0.  The table is read from global memory (4 bytes per lookup, L2-resident: 1 MB at 256 k
// tokens) -- no LDS, no atomics but the error bit, no scratch.  The trip counts are block-uniform up to the last
// partial step, nothing waits for another workgroup.

namespace bpeamd {

constexpr uint32_t VM_T = 256;      // threads per workgroup
constexpr uint32_t VM_PER = 4;      // ids one thread moves per step (one 16-byte access)
constexpr uint32_t VM_GRID = 2048;  // workgroups at most (longer arrays are walked in grid strides)
constexpr uint32_t VM_HOLE = 0xFFFFFFFFu;

// tab[id] or 0; *bad is set for id >= n (compared first: id is no index then) or a hole
__device__ inline uint32_t vm_lookup(uint32_t id, const uint32_t *__restrict__ tab, uint32_t n, bool *bad) {
    const uint32_t v = id < n ? tab[id] : VM_HOLE;
    if (v == VM_HOLE) {
        *bad = true;
        return 0u;
    }
    return v;
}

__device__ inline void vm_apply(uint32_t *ids, uint64_t len, const uint32_t *__restrict__ tab, uint32_t n,
                                uint32_t *__restrict__ err) {
    // ids is 4-byte aligned: head = the ids before the first 16-byte boundary (0..3, at most len)
    const uint64_t to16 = (uint64_t)((16u - (uint32_t)((uintptr_t)ids & 15u)) & 15u) >> 2;
    const uint64_t head = to16 < len ? to16 : len;
    const uint64_t nvec = (len - head) / VM_PER;
    uint4 *v = (uint4 *)(ids + head);
    bool bad = false;
    for (uint64_t q = (uint64_t)blockIdx.x * VM_T + threadIdx.x; q < nvec; q += (uint64_t)gridDim.x * VM_T) {
        uint4 x = v[q];
        x.x = vm_lookup(x.x, tab, n, &bad);
        x.y = vm_lookup(x.y, tab, n, &bad);
        x.z = vm_lookup(x.z, tab, n, &bad);
        x.w = vm_lookup(x.w, tab, n, &bad);
        v[q] = x;
    }
    if (blockIdx.x == 0 && threadIdx.x < 6) {  // the scalar head (threads 0..2) and tail (3..5)
        const uint32_t t = threadIdx.x;
        const uint64_t i = t < 3 ? t : head + nvec * VM_PER + (t - 3);
        if (t < 3 ? i < head : i < len) ids[i] = vm_lookup(ids[i], tab, n, &bad);
    }
    if (bad) atomicOr(err, 1u);
}

__global__ __launch_bounds__(VM_T) void k_ids_map(uint32_t *ids, uint64_t len, const uint32_t *__restrict__ fwd,
                                                  uint32_t nfwd, uint32_t *__restrict__ err) {
    vm_apply(ids, len, fwd, nfwd, err);
}

__global__ __launch_bounds__(VM_T) void k_ids_unmap(uint32_t *ids, uint64_t len, const uint32_t *__restrict__ inv,
                                                    uint32_t ninv, uint32_t *__restrict__ err) {
    vm_apply(ids, len, inv, ninv, err);
}

}  // namespace bpeamd

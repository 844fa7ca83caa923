// pieces.hip -- the host side of the pieces path; included by engine.hip.  The calls of bpe_gpu.h that cut the
// resident bytes into pieces (kernels: split.hip, special.hip), train on the pieces (train_split.hip) and encode
// them as documents (encode_docs_run of engine.hip, then special.hip's post-pass).
#include "../src/bpe_split_presets.h"

extern "C" {

// a grow-only device array of 8-byte entries (d_split, d_sp_pieces): room for `need`, `least` at the smallest
static int grow_array(bpe_gpu_ctx *c, void **p, size_t *cap, size_t need, size_t least, const char *what) {
    if (*cap >= need) return 0;
    HIPCHK(hipStreamSynchronize(c->st));
    if (*p) (void)hipFree(*p);
    *p = nullptr;
    *cap = 0;
    hipError_t e = hipMalloc(p, std::max(need, least) * 8);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(BPE_GPU_ENOMEM, what, e);
    }
    *cap = std::max(need, least);
    return 0;
}

// ------------------------------------------------ pieces of the resident bytes (split.hip)

// What marks the starts: the tables of bpe_gpu_split, or the kernel of a preset that has none.
enum MarkKind { MARK_TABLE, MARK_GPT2, MARK_GPT2_UNICODE, MARK_CL100K };
struct Marker {
    MarkKind kind = MARK_TABLE;
    SplitRule tables;  // kind == MARK_TABLE
    bool specials_first() const { return kind == MARK_CL100K; }  // found before marking: the kernel reads their cover
    // what k_sp_patch decides again around a match: 1 BPE_SPLIT_GPT2's rule, 2 BPE_SPLIT_GPT2_UNICODE's, 0 nothing
    int patch_mode() const { return kind == MARK_GPT2 ? 1 : kind == MARK_GPT2_UNICODE ? 2 : 0; }
};

// the marker of a preset (preset >= 0) or of the tables cls / brk (preset < 0)
static int marker_of(int preset, const uint8_t *cls, const uint16_t *brk, Marker *m) {
    uint8_t pc[256];
    uint16_t pb[16];
    switch (preset) {
    case BPE_SPLIT_GPT2: m->kind = MARK_GPT2; return 0;
    case BPE_SPLIT_GPT2_UNICODE: m->kind = MARK_GPT2_UNICODE; return 0;
    case BPE_SPLIT_CL100K: m->kind = MARK_CL100K; return 0;
    default:  // a table preset (bpe_gpu_split_rule refuses every other number), or the caller's tables
        if (preset >= 0 && bpe_gpu_split_rule(preset, pc, pb)) return BPE_GPU_EINVAL;
        if (preset >= 0) cls = pc, brk = pb;
    }
    m->kind = MARK_TABLE;
    for (int b = 0; b < 256; b++)
        if ((m->tables.cls[b] = cls[b]) > 15) return fail(BPE_GPU_EINVAL, "split: a class above 15");
    memcpy(m->tables.brk, brk, sizeof m->tables.brk);
    return 0;
}

// workgroups of the per-match / per-id kernels of special.hip (they stride)
static uint32_t sx_grid(uint64_t items) {
    return (uint32_t)std::min<uint64_t>(std::max<uint64_t>((items + SX_T - 1) / SX_T, 1), SX_GRID);
}

// what the special passes leave on the device for the passes after them (DS_SP_SET, _COVER, _LIST, _SORTED, _CTL)
struct SpFound {
    SpSet *set = nullptr;
    uint32_t *cover = nullptr;             // a bit per byte of the whole tiles
    unsigned long long *list = nullptr;    // the matches, M of them
    unsigned long long *sorted = nullptr;  // ... by start, once sp_patch ran
    uint32_t *ctl = nullptr;               // control words
    uint32_t M = 0;
};

// The special passes of a split (special.hip).  sp_find: the matches; it runs after the marking kernel, or before
// it for a marker whose kernel reads the cover bitmap (Marker::specials_first).  sp_patch, between the marking
// kernel and the count scan when there are matches: patch, recount and sort.
// T, boff: the gaps of a text batch (texts.hip), which join the list behind the matches as breaks; T == 0: none
static int sp_find(bpe_gpu_ctx *c, const SpSet *sp, uint64_t n, uint64_t ntiles, uint32_t grid, SpFound *F, uint64_t *info,
                   uint64_t T = 0, const uint64_t *boff = nullptr) {
    int r;
    const size_t cov_bytes = ntiles * SP_T * 2;  // a bit per byte of the whole tiles
    if ((r = dscratch(c, DS_SP_SET, sizeof(SpSet), &F->set)) || (r = dscratch(c, DS_SP_COVER, cov_bytes, &F->cover)) ||
        (r = dscratch(c, DS_SP_CTL, 64, &F->ctl)))
        return r;
    HIPCHK(hipMemcpyAsync(F->set, sp, sizeof(SpSet), hipMemcpyHostToDevice, c->st));
    HIPCHK(hipMemsetAsync(F->cover, 0, cov_bytes, c->st));
    // room for a match every 256 bytes; a text with more runs the pass again with the room it counted
    uint64_t cap = n / 256 + 1024;
    for (int pass = 1;; pass++) {
        if ((r = dscratch(c, DS_SP_LIST, (cap + T) * 8, &F->list))) return r;
        HIPCHK(hipMemsetAsync(F->ctl, 0, 64, c->st));
        if (!sp->S) break;  // (a text batch without specials: the list holds its breaks alone)
        k_sp_find<<<grid, SP_T, 0, c->st>>>(c->h.bytes, n, ntiles, F->set, F->cover, F->list,
                                            (uint32_t)std::min<uint64_t>(cap, 0xFFFFFFFFull), F->ctl);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(&F->M, F->ctl, 4, hipMemcpyDeviceToHost, c->st));
        HIPCHK(hipStreamSynchronize(c->st));
        info[2] = (uint64_t)pass;
        if (F->M <= cap) break;
        if (pass == 2) return fail(BPE_GPU_EINTERNAL, "split_special: the second find pass counted more matches than the first");
        cap = F->M;
    }
    info[1] = F->M;
    info[3] = cap;
    if (T) {
        k_text_breaks<<<sx_grid(T), SX_T, 0, c->st>>>(boff, T, F->cover, F->list + F->M);
        HIPCHK(hipGetLastError());
        F->M += (uint32_t)T;  // (matches and gaps are distinct bytes: M + T <= n)
    }
    return 0;
}

static int sp_patch(bpe_gpu_ctx *c, SpFound *F, int mode, uint64_t n, uint64_t ntiles, uint32_t grid, uint16_t *mask, uint32_t *wcnt) {
    int r;
    if (!F->M) return 0;
    k_sp_patch<<<sx_grid(F->M), SX_T, 0, c->st>>>(c->h.bytes, n, F->list, F->M, F->set, F->cover, (uint32_t *)mask, mode);
    HIPCHK(hipGetLastError());
    k_sp_recount<<<grid, SP_T, 0, c->st>>>(mask, ntiles, wcnt);
    HIPCHK(hipGetLastError());
    if ((r = dscratch(c, DS_SP_SORTED, (size_t)F->M * 8, &F->sorted))) return r;
    return ROCPRIM_RUN(c, DS_SP_TMP, rocprim::radix_sort_keys(tmp, tb, F->list, F->sorted, F->M, 8, 40, c->st));
}

// BPE_SPLIT_CL100K's marks: the effects of the wave tiles on the three chains, their scan, and the marks
// (split.hip).  One scan serves both directions: sum_f[nwt], a reset (the summary kernel writes it), sum_b[nwt]
// (the tiles in reverse order).  cover: the specials' bitmap, or nullptr
static int mark_cl100k(bpe_gpu_ctx *c, const uint32_t *cover, uint64_t n, uint64_t ntiles, uint64_t nwt, uint32_t grid,
                uint16_t *mask, uint32_t *wcnt) {
    int r;
    uint32_t *sum;
    const size_t cnt = 2 * nwt + 1;
    if ((r = dscratch(c, DS_CL_CHAINS, 2 * cnt * 4, &sum))) return r;
    uint32_t *in = sum + cnt;
    k_cl_summary<<<grid, SP_T, 0, c->st>>>(c->h.bytes, n, ntiles, cover, sum, sum + nwt + 1);
    HIPCHK(hipGetLastError());
    if ((r = ROCPRIM_RUN(c, DS_CL_TMP, rocprim::exclusive_scan(tmp, tb, sum, in, CL_RESET, cnt, ClCompose(), c->st)))) return r;
    k_split_mark_cl100k<<<grid, SP_T, 0, c->st>>>(c->h.bytes, n, ntiles, cover, in, in + nwt + 1, mask, wcnt);
    return 0;
}

// The body of bpe_gpu_split, bpe_gpu_split_preset and bpe_gpu_split_special (preset >= 0, or the tables): all but the
// marking launches is one code, so the offsets and their lifetime are the same whichever kernel marked the starts.
// sp: the specials of bpe_gpu_split_special (nullptr: none, and nothing but the launches below runs)
static int split_run(bpe_gpu_ctx *c, int preset, const uint8_t *cls, const uint16_t *brk, size_t *ndocs, const SpSet *sp) {
    Marker m;
    int r = marker_of(preset, cls, brk, &m);
    if (r) return r;
    HIPCHK(hipSetDevice(c->dev));
    c->split_ready = false;
    c->ts_ready = false;  // bpe_gpu_train_split's results describe the offsets replaced here
    c->sp_S = 0;          // ... and so do the specials and their pieces
    c->sp_M = 0;
    // a text batch: its gaps are breaks, found like matches whether or not there are specials
    const uint64_t T = c->tx_on ? c->tx_T : 0;
    const uint64_t *boff = (const uint64_t *)c->dscr[DS_TX_BOFF];
    std::vector<SpSet> none;
    if (T && !sp) {
        none.resize(1);
        memset(&none[0], 0, sizeof(SpSet));
        sp = &none[0];
    }
    if (T && sp->S > SX_BREAK)
        return fail(BPE_GPU_EINVAL, "split: a text batch takes at most 255 specials (index 255 is BPE_GPU_TEXT_BREAK)");
    uint64_t sp_info[4] = {sp ? sp->S : 0u, 0, 0, 0};
    SpFound F;
    const uint64_t n = c->n0, ntiles = (n + SP_TILE - 1) / SP_TILE, nwt = ntiles * (SP_T / 64);
    const uint32_t grid = (uint32_t)std::min<uint64_t>(ntiles, SP_GRID);
    unsigned long long total = 0, *woff = nullptr;
    uint16_t *mask = nullptr;
    if (n) {
        uint32_t *tbl = nullptr;
        // counts [nwt + 1] (the last one 0) and their scan [nwt + 1] in one slot
        if ((m.kind == MARK_TABLE && (r = dscratch(c, DS_SPLIT_TABLE, SP_TBL * 4, &tbl))) ||
            (r = dscratch(c, DS_SPLIT_MASK, ntiles * SP_T * 2, &mask)) ||
            (r = dscratch(c, DS_SPLIT_COUNTS, (nwt + 1) * 8 + ((nwt + 1) * 4 + 7) / 8 * 8, &woff)))
            return r;
        uint32_t *wcnt = (uint32_t *)(woff + nwt + 1);
        HIPCHK(hipMemsetAsync(wcnt + nwt, 0, 4, c->st));
        if (sp && m.specials_first() && (r = sp_find(c, sp, n, ntiles, grid, &F, sp_info, T, boff))) return r;
        switch (m.kind) {
        case MARK_TABLE:
            k_split_table<<<SP_TBL / SP_T, SP_T, 0, c->st>>>(m.tables, tbl);
            HIPCHK(hipGetLastError());
            k_split_mark<<<grid, SP_T, 0, c->st>>>(c->h.bytes, n, tbl, ntiles, mask, wcnt);
            break;
        case MARK_GPT2:
            k_split_mark_gpt2<<<grid, SP_T, 0, c->st>>>(c->h.bytes, n, ntiles, mask, wcnt);
            break;
        case MARK_GPT2_UNICODE:
            k_split_mark_gpt2u<<<grid, SP_T, 0, c->st>>>(c->h.bytes, n, ntiles, mask, wcnt);
            break;
        case MARK_CL100K:
            if ((r = mark_cl100k(c, F.cover, n, ntiles, nwt, grid, mask, wcnt))) return r;
            break;
        }
        HIPCHK(hipGetLastError());
        if (sp && !m.specials_first() && (r = sp_find(c, sp, n, ntiles, grid, &F, sp_info, T, boff))) return r;
        if (sp && (r = sp_patch(c, &F, m.patch_mode(), n, ntiles, grid, mask, wcnt))) return r;
        r = ROCPRIM_RUN(c, DS_SPLIT_TMP, rocprim::exclusive_scan(tmp, tb, wcnt, woff, 0ull, nwt + 1, rocprim::plus<unsigned long long>(), c->st));
        if (r) return r;
        HIPCHK(hipMemcpyAsync(&total, woff + nwt, 8, hipMemcpyDeviceToHost, c->st));
        HIPCHK(hipStreamSynchronize(c->st));
        if (total == 0 || total > n) return fail(BPE_GPU_EINTERNAL, "split: piece count out of range");
    }
    if ((r = grow_array(c, (void **)&c->d_split, &c->split_cap, total + 1, 32, "split: hipMalloc of the offsets"))) return r;
    if (n) {
        k_split_emit<<<grid, SP_T, 0, c->st>>>(mask, woff, ntiles, n, c->d_split);
        HIPCHK(hipGetLastError());
    } else {
        HIPCHK(hipMemsetAsync(c->d_split, 0, 8, c->st));
    }
    if (F.M) {  // the matches' starts as piece indices: the list that stays
        if ((r = grow_array(c, (void **)&c->d_sp_pieces, &c->sp_cap, F.M, 1, "split_special: hipMalloc of the special pieces"))) return r;
        uint32_t bad = 0;
        k_sp_pieces<<<sx_grid(F.M), SX_T, 0, c->st>>>(F.sorted, F.M, c->d_split, total, c->d_sp_pieces, F.ctl + 1);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(&bad, F.ctl + 1, 4, hipMemcpyDeviceToHost, c->st));
        HIPCHK(hipStreamSynchronize(c->st));
        if (bad) return fail(BPE_GPU_EINTERNAL, "split_special: a match does not start a piece");
    }
    if (c->tx_on) {  // every gap's piece, and the offsets as the caller sees them: no break piece, the plain join's bytes
        if (total < T) return fail(BPE_GPU_EINTERNAL, "split: fewer pieces than text breaks");
        uint64_t *bpiece, *plain;
        uint32_t *bad, hbad = 0;
        if ((r = dscratch(c, DS_TX_PIECE, T * 8, &bpiece)) || (r = dscratch(c, DS_TX_SPLIT, (total - T + 1) * 8, &plain)) ||
            (r = dscratch(c, DS_SP_CTL, 64, &bad)))
            return r;
        HIPCHK(hipMemsetAsync(bad + 2, 0, 4, c->st));
        if (T) k_text_pieces<<<sx_grid(T), SX_T, 0, c->st>>>(boff, T, c->d_split, total, bpiece, bad + 2);
        HIPCHK(hipGetLastError());
        k_text_compact<<<sx_grid(total + 1), SX_T, 0, c->st>>>(c->d_split, total, bpiece, T, 1, plain);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(&hbad, bad + 2, 4, hipMemcpyDeviceToHost, c->st));
        HIPCHK(hipStreamSynchronize(c->st));
        if (hbad) return fail(BPE_GPU_EINTERNAL, "split: a text break is no piece of its own");
    }
    HIPCHK(hipStreamSynchronize(c->st));
    c->sp_S = sp ? sp->S : 0u;
    c->sp_M = F.M;
    memcpy(c->sp_info, sp_info, sizeof sp_info);
    c->split_n = total;
    c->split_ready = true;
    *ndocs = (size_t)(total - T);
    return 0;
}

int bpe_gpu_split_rule(int preset, uint8_t *cls, uint16_t *brk) {
    if (!cls || !brk) return fail(BPE_GPU_EINVAL, "split_rule: bad argument");
    memset(cls, 0, 256);
    memset(brk, 0, 16 * sizeof(uint16_t));
    const split_preset *p = split_preset_find(preset);
    if (!p) return fail(BPE_GPU_EINVAL, "split_rule: no such preset");
    if (!p->has_tables) {
        char msg[128];
        snprintf(msg, sizeof msg, "split_rule: %s has no tables (bpe_gpu_split_preset)", p->name);
        return fail(BPE_GPU_EINVAL, msg);
    }
    if (preset == BPE_SPLIT_LINES) {
        cls['\n'] = 1;
        brk[1] = 0x3;
        return 0;
    }
    for (int b = 0; b < 256; b++)  // BPE_SPLIT_WORDS
        cls[b] = (b >= 'A' && b <= 'Z') || (b >= 'a' && b <= 'z') || b >= 0x80 ? 1
                 : b >= '0' && b <= '9'                                        ? 2
                 : b == ' '                                                    ? 3
                 : b >= '\t' && b <= '\r'                                      ? 4
                                                                               : 0;
    for (int q = 0; q < 5; q++) brk[q] = (uint16_t)(0x1F & ~(1 << q));
    brk[3] = 1 << 4;
    return 0;
}

int bpe_gpu_split_info(uint64_t *out4) {
    if (!out4) return BPE_GPU_EINVAL;
    out4[0] = SP_TILE;
    out4[1] = (uint64_t)SP_TILE * SP_GRID;
    out4[2] = out4[3] = 0;
    return 0;
}

int bpe_gpu_split(bpe_gpu_ctx *c, const uint8_t *cls, const uint16_t *brk, size_t *ndocs) {
    if (!c || !cls || !brk || !ndocs) return BPE_GPU_EINVAL;
    if (!c->loaded) return fail(BPE_GPU_ESTATE, "split before load");
    return split_run(c, -1, cls, brk, ndocs, nullptr);
}

int bpe_gpu_split_preset(bpe_gpu_ctx *c, int preset, size_t *ndocs) {
    if (!c || !ndocs) return BPE_GPU_EINVAL;
    if (!split_preset_find(preset)) return fail(BPE_GPU_EINVAL, "split_preset: no such preset");
    if (!c->loaded) return fail(BPE_GPU_ESTATE, "split before load");
    return split_run(c, preset, nullptr, nullptr, ndocs, nullptr);
}

int bpe_gpu_split_special(bpe_gpu_ctx *c, int preset, const uint8_t *cls, const uint16_t *brk,
                          const bpe_gpu_specials *specials, size_t *ndocs) {
    if (!c || !ndocs) return BPE_GPU_EINVAL;
    if (preset < 0 && (!cls || !brk)) return fail(BPE_GPU_EINVAL, "split_special: no preset and no tables");
    if (preset >= 0 && !split_preset_find(preset)) return fail(BPE_GPU_EINVAL, "split_special: no such preset");
    char msg[400];
    if (bpe_specials_check(specials, msg, sizeof msg)) return fail(BPE_GPU_EINVAL, msg);
    if (!c->loaded) return fail(BPE_GPU_ESTATE, "split before load");
    const size_t S = specials ? specials->count : 0;
    if (S == 0) return split_run(c, preset, cls, brk, ndocs, nullptr);
    // the set as the device reads it: in lexicographic order (no special is a prefix of another, so the first
    // difference decides), with the first-byte set
    std::vector<SpSet> hs(1);
    SpSet &H = hs[0];
    memset(&H, 0, sizeof H);
    std::vector<size_t> off(S + 1, 0);
    for (size_t j = 0; j < S; j++) off[j + 1] = off[j] + specials->len[j];
    std::vector<uint32_t> order(S);
    for (size_t j = 0; j < S; j++) order[j] = (uint32_t)j;
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
        const int d = memcmp(specials->bytes + off[a], specials->bytes + off[b], std::min(specials->len[a], specials->len[b]));
        return d ? d < 0 : specials->len[a] < specials->len[b];
    });
    for (size_t k = 0; k < S; k++) {
        const uint32_t j = order[k], L = specials->len[j];
        memcpy(H.txt + k * SX_LEN, specials->bytes + off[j], L);
        H.len[k] = (uint8_t)(L - 1);
        H.idx[k] = (uint8_t)j;
        H.lenj[j] = (uint8_t)(L - 1);
        const uint8_t b = specials->bytes[off[j]];
        H.first[b >> 5] |= 1u << (b & 31);
    }
    H.S = (uint32_t)S;
    return split_run(c, preset, cls, brk, ndocs, &H);
}

int bpe_gpu_split_special_info(bpe_gpu_ctx *c, uint64_t *out4) {
    if (!c || !out4) return BPE_GPU_EINVAL;
    if (!c->loaded || !c->split_ready) return fail(BPE_GPU_ESTATE, "no split: split first");
    memset(out4, 0, 4 * sizeof(uint64_t));
    if (c->sp_S) memcpy(out4, c->sp_info, sizeof c->sp_info);  // (a text batch's breaks are not counted: sp_find)
    return 0;
}

int bpe_gpu_fetch_special_pieces(bpe_gpu_ctx *c, uint64_t *piece, uint32_t *index, size_t cap, size_t *count) {
    if (!c || !count) return BPE_GPU_EINVAL;
    if (!c->loaded || !c->split_ready) return fail(BPE_GPU_ESTATE, "no special pieces: split first");
    HIPCHK(hipSetDevice(c->dev));
    const uint64_t T = c->tx_on ? c->tx_T : 0;
    const uint64_t M = c->sp_S ? c->sp_M : 0;  // (of a text batch: the breaks among them)
    *count = (size_t)(M ? M - T : 0);
    const size_t k = std::min<size_t>(cap, *count);
    if (!k || (!piece && !index)) return 0;
    // a text batch: the list holds the break pieces too, which are skipped, and the pieces are numbered without them
    std::vector<unsigned long long> h(T ? (size_t)M : k);
    const int r = d2h_staged(c, h.data(), c->d_sp_pieces, h.size() * 8);
    if (r) return r;
    size_t breaks = 0, at = 0;
    for (size_t m = 0; m < h.size() && at < k; m++) {
        if (T && (h[m] & 0xFFull) == SX_BREAK) {
            breaks++;
            continue;
        }
        if (piece) piece[at] = (h[m] >> 8) - breaks;
        if (index) index[at] = (uint32_t)(h[m] & 0xFFull);
        at++;
    }
    return 0;
}

int bpe_gpu_fetch_split_offsets(bpe_gpu_ctx *c, uint64_t *out, size_t cap, size_t *count) {
    if (!c || !count) return BPE_GPU_EINVAL;
    if (!c->loaded || !c->split_ready) return fail(BPE_GPU_ESTATE, "no split offsets: split first");
    HIPCHK(hipSetDevice(c->dev));
    const uint64_t T = c->tx_on ? c->tx_T : 0;  // a text batch: the offsets without the break pieces (DS_TX_SPLIT)
    *count = c->split_n - T + 1;
    const size_t k = out ? std::min<size_t>(cap, *count) : 0;
    if (k) return d2h_staged(c, out, c->tx_on ? (const uint64_t *)c->dscr[DS_TX_SPLIT] : c->d_split, k * 8);
    return 0;
}

static int encode_split_specials(bpe_gpu_ctx *c, uint64_t M, size_t n_merges, bool tx);
static int encode_split_texts(bpe_gpu_ctx *c);

int bpe_gpu_encode_split(bpe_gpu_ctx *c, const uint32_t *pairs, size_t n_merges) {
    if (!c || (!pairs && n_merges)) return BPE_GPU_EINVAL;
    if (!c->loaded) return fail(BPE_GPU_ESTATE, "encode before load");
    if (!c->split_ready) return fail(BPE_GPU_ESTATE, "encode_split: no split of the loaded bytes");
    if (n_merges > 0xFFFFFEFFull) return fail(BPE_GPU_ERANGE, "merge list too long");
    const bool tx = c->tx_on;
    const uint64_t M = c->sp_S || tx ? c->sp_M : 0;
    if (M && n_merges + 256 + c->sp_S > 0xFFFFFFFFull) return fail(BPE_GPU_ERANGE, "merge list too long for the specials' ids");
    int r = encode_docs_run(c, nullptr, c->split_n, pairs, n_merges, now_ms());
    if (r || (!M && !tx)) return r;
    if (tx) c->docs_ready = false;  // (until the texts' offsets below are written)
    if (M && (r = encode_split_specials(c, M, n_merges, tx))) return r;
    return tx ? encode_split_texts(c) : 0;
}

// The post-pass of bpe_gpu_encode_split over the M special pieces (special.hip): whichever path left ids_out / d_idoff,
// every special piece keeps one id, 256 + n_merges + j, and the ids and offsets after it move down.  tx: a text batch,
// whose break pieces are among the M and keep no id.
static int encode_split_specials(bpe_gpu_ctx *c, uint64_t M, size_t n_merges, bool tx) {
    int r;
    const double t0 = now_ms();
    const uint64_t len = c->ids_len, ndocs = c->split_n;
    uint64_t *ist, *rem, *rsum;
    if ((r = dscratch(c, DS_SP_FIRST_ID, M * 8, &ist)) || (r = dscratch(c, DS_SP_REMOVED, (M + 1) * 8, &rem)) ||
        (r = dscratch(c, DS_SP_REMOVED_SCAN, (M + 1) * 8, &rsum)))
        return r;
    k_sp_idlen<<<sx_grid(M + 1), SX_T, 0, c->st>>>(c->d_sp_pieces, (uint32_t)M, c->d_idoff, ist, rem, tx);
    HIPCHK(hipGetLastError());
    r = ROCPRIM_RUN(c, DS_SP_TMP, rocprim::exclusive_scan(tmp, tb, rem, rsum, (uint64_t)0, M + 1, rocprim::plus<uint64_t>(), c->st));
    if (r) return r;
    uint64_t removed = 0;
    HIPCHK(hipMemcpyAsync(&removed, rsum + M, 8, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    if (removed > len || len - removed < M - (tx ? c->tx_T : 0)) return fail(BPE_GPU_EINTERNAL, "encode_split: the special pieces hold more ids than there are");
    uint32_t *ids2;
    uint64_t *idoff2;
    if ((r = dalloc(c, &ids2, len - removed, false)) || (r = dalloc(c, &idoff2, ndocs + 1, false))) return r;
    k_sp_ids<<<sx_grid(len), SX_T, 0, c->st>>>(c->h.ids_out, len, c->d_sp_pieces, (uint32_t)M, ist, rsum,
                                              (uint32_t)(256 + n_merges), ids2, tx);
    HIPCHK(hipGetLastError());
    k_sp_idoff<<<sx_grid(ndocs + 1), SX_T, 0, c->st>>>(c->d_idoff, ndocs, c->d_sp_pieces, (uint32_t)M, rsum, idoff2);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->st));
    c->h.ids_out = ids2;
    c->d_idoff = idoff2;
    c->ids_len = len - removed;
    const double ms = now_ms() - t0;
    c->stats.n_out = c->ids_len;
    c->stats.occurrences = c->n0 - std::min<uint64_t>(c->n0, c->ids_len);
    c->stats.ms_train += ms;
    c->stats.ms_total += ms;
    return 0;
}

// ... and of a text batch after it (texts.hip): text_off from where the break pieces' ids vanished, and the id offsets
// without the break pieces
static int encode_split_texts(bpe_gpu_ctx *c) {
    const double t0 = now_ms();
    const uint64_t T = c->tx_T, P = c->split_n;
    const uint64_t *bpiece = (const uint64_t *)c->dscr[DS_TX_PIECE];
    uint64_t *toff, *idoff3;
    int r;
    if ((r = dscratch(c, DS_TX_IDOFF, (T + 1) * 8, &toff)) || (r = dalloc(c, &idoff3, P - T + 1, false))) return r;
    k_text_off<<<sx_grid(T + 1), SX_T, 0, c->st>>>(c->d_idoff, bpiece, T, toff);
    HIPCHK(hipGetLastError());
    k_text_compact<<<sx_grid(P + 1), SX_T, 0, c->st>>>(c->d_idoff, P, bpiece, T, 0, idoff3);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->st));
    c->d_idoff = idoff3;
    c->docs_n = P - T;
    c->docs_info[0] = P - T;
    c->docs_ready = true;
    const double ms = now_ms() - t0;
    c->stats.ms_train += ms;
    c->stats.ms_total += ms;
    return 0;
}

// ------------------------------------------------ training on the pieces (train_split.hip)

// workgroups for `items` elements at `per` of them per thread, TS_GRID at most (the kernels stride)
static uint32_t ts_grid(uint64_t items, uint32_t per = 1) {
    const uint64_t chunk = (uint64_t)TS_T * per;
    return (uint32_t)std::min<uint64_t>(std::max<uint64_t>((items + chunk - 1) / chunk, 1), TS_GRID);
}

// the control words on the host (one synchronisation)
static int ts_read_ctl(bpe_gpu_ctx *c, const uint32_t *ctl, uint32_t *hc) {
    HIPCHK(hipMemcpyAsync(hc, ctl, 16 * 4, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    return 0;
}

// what ts_piece_table leaves for stage B: E entries of T bytes in start order (DS_TS_ESTART, _EOFF, _ECNT), its counters
struct TsTable {
    const uint64_t *start = nullptr;  // [E] the entries' first bytes
    const uint32_t *off = nullptr;    // [E + 1] their scanned lengths
    const uint32_t *count = nullptr;  // [E] pieces per entry
    uint64_t E = 0, T = 0, nlong = 0, slots = 0;
};

// Stage A: the pieces as weighted entries in start order.
static int ts_piece_table(bpe_gpu_ctx *c, uint32_t *ctl, TsTable *out) {
    const uint64_t P = c->split_n;
    const uint64_t *off = c->d_split;
    uint32_t hc[16], *pcnt;
    int r;
    // the table starts small (text has few distinct pieces) and grows fourfold when a probe chain runs out;
    // at 2 P slots or more a chain of TS_PROBE is a defect of the hash, not load
    const uint64_t smax = std::max<uint64_t>(pow2_at_least(2 * P), 1024) * 16;
    const int knob = getenv_int("BPE_TS_SLOTS", 0);
    uint64_t S = knob > 0 ? pow2_at_least(std::max(knob, 64)) : std::min<uint64_t>(std::max<uint64_t>(pow2_at_least(2 * P), 1024), 1u << 22);
    unsigned long long *pslot;
    for (;;) {
        if ((r = dscratch(c, DS_TS_SLOTS, S * 8, &pslot)) || (r = dscratch(c, DS_TS_SLOT_CNT, S * 4, &pcnt))) return r;
        HIPCHK(hipMemsetAsync(pslot, 0xFF, S * 8, c->st));
        HIPCHK(hipMemsetAsync(pcnt, 0, S * 4, c->st));
        HIPCHK(hipMemsetAsync(ctl, 0, 16 * 4, c->st));
        k_ts_insert<<<ts_grid(P, 8), TS_T, 0, c->st>>>(c->h.bytes, off, P, pslot, pcnt, S - 1, ctl);
        HIPCHK(hipGetLastError());
        if ((r = ts_read_ctl(c, ctl, hc))) return r;
        if (!hc[TSC_FULL]) break;
        if (S >= smax) return fail(BPE_GPU_EINTERNAL, "train_split: the piece table is full at its largest size");
        S *= 4;
    }
    uint64_t ne = (uint64_t)hc[TSC_LONG] + hc[TSC_CLAIMED];
    if (ne == 0 || ne > P) return fail(BPE_GPU_EINTERNAL, "train_split: entry count out of range");
    uint32_t *k0, *v0, *k1, *v1, *elen, *eoff;
    uint64_t *est;
    void *tmp;
    if ((r = dscratch(c, DS_TS_KEY0, ne * 4, &k0)) || (r = dscratch(c, DS_TS_VAL0, ne * 4, &v0)) ||
        (r = dscratch(c, DS_TS_KEY1, ne * 4, &k1)) || (r = dscratch(c, DS_TS_ECNT, ne * 4, &v1)) ||
        (r = dscratch(c, DS_TS_ESTART, ne * 8, &est)) || (r = dscratch(c, DS_TS_ELEN, (ne + 1) * 4, &elen)) ||
        (r = dscratch(c, DS_TS_EOFF, (ne + 1) * 4, &eoff)))
        return r;
    k_ts_collect_slots<<<ts_grid(S), TS_T, 0, c->st>>>(pslot, pcnt, S, ctl, k0, v0, ne);
    HIPCHK(hipGetLastError());
    if (hc[TSC_LONG]) {
        k_ts_collect_long<<<ts_grid(P), TS_T, 0, c->st>>>(off, P, ctl, k0, v0, ne);
        HIPCHK(hipGetLastError());
    }
    const uint64_t nlong = hc[TSC_LONG];
    // After a split with specials their pieces are no part of the corpus: each special is at most one record
    // (it fits TS_DEDUP_MAX), whose key k_sp_drop sets to 0xFFFFFFFF, so that it sorts past the entries.
    const uint64_t nrec = ne;
    if (c->sp_S && c->sp_M) {
        k_sp_drop<<<sx_grid(nrec), SX_T, 0, c->st>>>(k0, nrec, c->d_sp_pieces, (uint32_t)c->sp_M, ctl + 8);
        HIPCHK(hipGetLastError());
        if ((r = ts_read_ctl(c, ctl, hc))) return r;
        if (hc[8] > c->sp_S || hc[8] > nrec) return fail(BPE_GPU_EINTERNAL, "train_split: more special records than specials");
        ne = nrec - hc[8];
    }
    // one temporary, sized for the larger of the sort and the scan
    size_t tb = 0, tb2 = 0;
    HIPCHK(rocprim::radix_sort_pairs(nullptr, tb, k0, k1, v0, v1, nrec, 0, 32, c->st));
    HIPCHK(rocprim::exclusive_scan(nullptr, tb2, elen, eoff, 0u, ne + 1, rocprim::plus<uint32_t>(), c->st));
    if ((r = dscratch(c, DS_TS_TMP, tb = std::max(tb, tb2), &tmp))) return r;
    HIPCHK(rocprim::radix_sort_pairs(tmp, tb, k0, k1, v0, v1, nrec, 0, 32, c->st));
    k_ts_entries<<<(uint32_t)((ne + TS_T) / TS_T), TS_T, 0, c->st>>>(off, k1, ne, est, elen);
    HIPCHK(hipGetLastError());
    HIPCHK(rocprim::exclusive_scan(tmp, tb, elen, eoff, 0u, ne + 1, rocprim::plus<uint32_t>(), c->st));
    uint32_t total = 0;
    HIPCHK(hipMemcpyAsync(&total, eoff + ne, 4, hipMemcpyDeviceToHost, c->st));
    if ((r = ts_read_ctl(c, ctl, hc))) return r;
    if (hc[TSC_APPEND] != nrec) return fail(BPE_GPU_EINTERNAL, "train_split: entry records do not match their count");
    if (total < ne || total > c->n0) return fail(BPE_GPU_EINTERNAL, "train_split: entry bytes out of range");
    *out = TsTable{est, eoff, v1, ne, total, nlong, S};
    return 0;
}

int bpe_gpu_train_split(bpe_gpu_ctx *c, long max_merges, size_t *n_merges) {
    if (!c || !n_merges) return BPE_GPU_EINVAL;
    if (!c->loaded) return fail(BPE_GPU_ESTATE, "train_split before load");
    if (c->tx_on) return fail(BPE_GPU_ESTATE, "train_split: the context holds a text batch (bpe_gpu_load_texts): training on text batches is not offered");
    if (!c->split_ready) return fail(BPE_GPU_ESTATE, "train_split: no split of the loaded bytes");
    HIPCHK(hipSetDevice(c->dev));
    c->ts_ready = false;
    c->ts_merges.clear();
    const bool own_cap = max_merges < 0 || (uint64_t)max_merges > engine_merge_cap();  // else the caller's
    const uint64_t cap = own_cap ? engine_merge_cap() : (uint64_t)max_merges;
    int r;
    uint32_t *ctl, hc[16];
    if ((r = dscratch(c, DS_TS_CTL, 16 * 4, &ctl))) return r;
    TsTable tab;
    if (c->split_n && (r = ts_piece_table(c, ctl, &tab))) return r;
    const uint64_t E = tab.E;
    uint64_t T = tab.T, stop = 0;
    // Stage B: tok / ent ping-pong, keep and its scan, run heads and their scan (DS_TS_TOK0 .. DS_TS_RUNS)
    uint32_t *tok[2] = {}, *ent[2] = {}, *keep = nullptr, *pos = nullptr, *hv = nullptr, *rs = nullptr;
    void *tmp = nullptr;
    size_t tb = 0, t1 = 0, t2 = 0;
    if (T) {
        uint32_t **q[8] = {&tok[0], &tok[1], &ent[0], &ent[1], &keep, &pos, &hv, &rs};
        for (int k = 0; k < 8; k++)
            if ((r = dscratch(c, (DScr)(DS_TS_TOK0 + k), (T + 1) * 4, q[k]))) return r;
        // one temporary for the loop below, sized once for the larger of its two scans
        HIPCHK(rocprim::exclusive_scan(nullptr, t1, keep, pos, 0u, T + 1, rocprim::plus<uint32_t>(), c->st));
        HIPCHK(rocprim::inclusive_scan(nullptr, t2, hv, rs, T, rocprim::maximum<uint32_t>(), c->st));
        if ((r = dscratch(c, DS_TS_TMP, tb = std::max(t1, t2), &tmp))) return r;
        k_ts_gather<<<ts_grid(T), TS_T, 0, c->st>>>(c->h.bytes, tab.start, tab.off, (uint32_t)E, (uint32_t)T, tok[0], ent[0]);
        HIPCHK(hipGetLastError());
    }
    // the pair table starts at 2 T slots or 2^20 and grows like the piece table
    const uint64_t pmax = std::max<uint64_t>(pow2_at_least(2 * T), 1024) * 16;
    uint64_t Sp = std::min<uint64_t>(std::max<uint64_t>(pow2_at_least(2 * T), 1024), 1u << 20);
    unsigned long long *part;
    if ((r = dscratch(c, DS_TS_ARGMAX, (size_t)TS_GRID * 16, &part))) return r;
    int cur = 0;
    for (uint64_t m = 0;; m++) {
        uint32_t best = 0, a = 0, b = 0;
        if (T >= 2) {
            for (;;) {
                unsigned long long *pk;
                uint32_t *pc;
                if ((r = dscratch(c, DS_TS_PAIR_KEYS, Sp * 8, &pk)) || (r = dscratch(c, DS_TS_PAIR_CNT, Sp * 4, &pc))) return r;
                HIPCHK(hipMemsetAsync(pk, 0xFF, Sp * 8, c->st));
                HIPCHK(hipMemsetAsync(pc, 0, Sp * 4, c->st));
                HIPCHK(hipMemsetAsync(ctl, 0, 16 * 4, c->st));
                k_tb_count<<<ts_grid(T, 16), TB_CT, 0, c->st>>>(tok[cur], ent[cur], tab.count, (uint32_t)T, pk, pc, Sp - 1, ctl);
                HIPCHK(hipGetLastError());
                const uint32_t nb = ts_grid(Sp, 4);
                k_tb_argmax<<<nb, TS_T, 0, c->st>>>(pk, pc, Sp, part);
                HIPCHK(hipGetLastError());
                k_tb_argmax2<<<1, TS_T, 0, c->st>>>(part, nb, ctl);
                HIPCHK(hipGetLastError());
                if ((r = ts_read_ctl(c, ctl, hc))) return r;
                if (!hc[TSC_PFULL]) break;
                if (Sp >= pmax) return fail(BPE_GPU_EINTERNAL, "train_split: the pair table is full at its largest size");
                Sp *= 4;
            }
            best = hc[TSC_CNT], a = hc[TSC_A], b = hc[TSC_B];
        }
        if (best <= 1) {  // the reference's rule first: no pair left, or none seen twice
            stop = 1;
            break;
        }
        if (m == cap) {
            stop = own_cap ? 3 : 2;
            break;
        }
        const uint32_t z = 256u + (uint32_t)m, g = ts_grid(T, 4);
        const uint32_t *runs = nullptr;
        if (a == b) {
            k_tb_heads<<<g, TS_T, 0, c->st>>>(tok[cur], ent[cur], (uint32_t)T, a, hv);
            HIPCHK(hipGetLastError());
            HIPCHK(rocprim::inclusive_scan(tmp, tb, hv, rs, T, rocprim::maximum<uint32_t>(), c->st));
            runs = rs;
        }
        k_tb_flag<<<g, TS_T, 0, c->st>>>(tok[cur], ent[cur], runs, (uint32_t)T, a, b, keep);
        HIPCHK(hipGetLastError());
        HIPCHK(rocprim::exclusive_scan(tmp, tb, keep, pos, 0u, T + 1, rocprim::plus<uint32_t>(), c->st));
        k_tb_scatter<<<g, TS_T, 0, c->st>>>(tok[cur], ent[cur], keep, pos, (uint32_t)T, z, tok[cur ^ 1], ent[cur ^ 1]);
        HIPCHK(hipGetLastError());
        uint32_t newT = 0;
        HIPCHK(hipMemcpyAsync(&newT, pos + T, 4, hipMemcpyDeviceToHost, c->st));
        HIPCHK(hipStreamSynchronize(c->st));
        if (newT >= T || newT < E) return fail(BPE_GPU_EINTERNAL, "train_split: a merge removed no token or too many");
        T = newT;
        cur ^= 1;
        c->ts_merges.push_back(a);
        c->ts_merges.push_back(b);
    }
    if (stop == 3)
        fprintf(stderr,
                "bpe: training stopped at the engine's merge cap (%llu merges) before the reference's stop rule "
                "(max count <= 1); pass a merge cap to choose the length\n",
                (unsigned long long)cap);
    const uint64_t info[8] = {c->split_n, E, tab.T, tab.nlong, c->ts_merges.size() / 2, stop, TS_DEDUP_MAX, tab.slots};
    memcpy(c->ts_info, info, sizeof info);
    c->ts_ready = true;
    *n_merges = c->ts_merges.size() / 2;
    return 0;
}

int bpe_gpu_fetch_split_merges(bpe_gpu_ctx *c, uint32_t *out, size_t cap, size_t *count) {
    if (!c || !count) return BPE_GPU_EINVAL;
    if (!c->loaded || !c->split_ready || !c->ts_ready) return fail(BPE_GPU_ESTATE, "no split merges: train_split first");
    const size_t k = c->ts_merges.size() / 2;
    *count = k;
    if (out) memcpy(out, c->ts_merges.data(), std::min(cap, k) * 8);
    return 0;
}

int bpe_gpu_train_split_info(bpe_gpu_ctx *c, uint64_t *out8) {
    if (!c || !out8) return BPE_GPU_EINVAL;
    if (!c->loaded || !c->split_ready || !c->ts_ready) return fail(BPE_GPU_ESTATE, "no split training: train_split first");
    memcpy(out8, c->ts_info, sizeof c->ts_info);
    return 0;
}

// a call of its own, after bpe_gpu_train_split: it reads the slots ts_piece_table filled, which stay while ts_ready
int bpe_gpu_fetch_piece_table(bpe_gpu_ctx *c, uint64_t *start, uint32_t *len, uint32_t *count, size_t cap, size_t *entries) {
    if (!c || !entries) return BPE_GPU_EINVAL;
    if (!c->loaded || !c->split_ready || !c->ts_ready) return fail(BPE_GPU_ESTATE, "no piece table: train_split first");
    HIPCHK(hipSetDevice(c->dev));
    *entries = (size_t)c->ts_info[1];
    const size_t k = std::min<size_t>(cap, *entries);
    int r;
    if (k && start && (r = d2h_staged(c, start, c->dscr[DS_TS_ESTART], k * 8))) return r;
    if (k && len && (r = d2h_staged(c, len, c->dscr[DS_TS_ELEN], k * 4))) return r;
    if (k && count && (r = d2h_staged(c, count, c->dscr[DS_TS_ECNT], k * 4))) return r;
    return 0;
}

}  // extern "C"

// hgx_front_lines.hpp -- the line table of an alignment stream, made on the device: (offset, length, task) of the records that the
// regions keep, in QNAME order inside a task.  BAM records (chain walk, region filter) and SAM text (newline scan, line fields) each
// have their front half; the kept list (kept_list), the name order (name_order) and the table itself (k_name_lines) are one
// implementation, told where a format keeps its names by a small source type (BamNames, SamNames).
// Part of hgx_front.hip's translation unit: included there alone, inside its unnamed namespace, behind the scan (fe_scan), Lap and
// ctl_read.
#pragma once

// ---- BAM records straight from the inflated stream (round 4): chain walk, region filter, name sort as kernels -----------------
// What hgx_bam.cpp does on the host's threads when the records are not left to the device: the records of a BAM form a chain (each
// block_size leads to the next), so the stream is cut into ranges; every range but the first GUESSES a record start (a header that
// is plausible and leads to three more plausible headers) and walks from there past its end; the guesses are then CHECKED -- a
// range's walk must end exactly where the next one's begins -- and anything that does not link up declines the call.
// (The walk and link kernels live in hgx_bam_walk.hpp: read extraction walks its chunks with them too.)
// region filter (hgx_bam.cpp: reference span from the CIGAR, overlap with every region of the list) + the checks the host makes on a
// record.  keep[i] = the record's region MASK (bit g: region g of its task's list keeps it; one region or none: 0 / 1) -- the header
// and the CIGAR are read once, whatever the number of regions.
__global__ void __launch_bounds__(256) k_bam_filter(const unsigned char *__restrict__ text, const uint32_t *__restrict__ rec_off, const uint32_t *__restrict__ rec_len,
                                                    const uint16_t *__restrict__ rec_task, uint32_t n_rec, const BamSeg *__restrict__ segs,
                                                    const uint8_t *__restrict__ ref_action, const BamSpan *__restrict__ spans, uint32_t *__restrict__ keep, BamCtl *ctl) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rec) return;
    const unsigned char *r = text + rec_off[i];
    const uint32_t bs = rec_len[i], l_rn = r[8];
    const BamSeg G = segs[rec_task[i]];
    uint32_t k = 1;
    if (G.filtered) {
        const int32_t rid = bam_i32(r), pos = bam_i32(r + 4);
        if (rid < 0 || rid >= G.n_ref) k = 0;
        else {
            const uint32_t n_cig = bam_u16(r + 12), flag = bam_u16(r + 14);
            long long reflen = 0;
            if (!(flag & 4) && 32 + (size_t)l_rn + 4 * (size_t)n_cig <= bs) {
                const unsigned char *c = r + 32 + l_rn;
                for (uint32_t x = 0; x < n_cig; ++x) {
                    const uint32_t v = bam_u32(c + 4 * x), op = v & 15;
                    if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) reflen += v >> 4;
                }
            }
            const long long end0 = (long long)pos + (reflen > 0 ? reflen : 1) - 1;
            const uint8_t act = ref_action[G.act_off + (uint32_t)rid];
            k = act == 1 ? 1u : (act == 2 ? ((end0 >= G.left0 && (long long)pos <= G.right0) ? 1u : 0u) : 0u);
            for (uint32_t g = 1; g < G.n_regions; ++g) {
                const uint8_t a = ref_action[G.act_off + g * (uint32_t)G.n_ref + (uint32_t)rid];
                const BamSpan S = spans[G.span_off + g - 1];
                if (a == 1 || (a == 2 && end0 >= S.left0 && (long long)pos <= S.right0)) k |= 1u << g;
            }
        }
    }
    if (k && (l_rn == 0 || 32 + (size_t)l_rn > bs || r[32 + l_rn - 1] != 0)) { bam_decline(ctl, HGX_FE_DECLINE_RECORD); k = 0; }   // "malformed BAM record": the host's to report
    keep[i] = k;
    if (k) atomicMax(&ctl->max_klen, l_rn - 1);
}
// one region (or none): the kept list from the scan of the 0 / 1 masks
__global__ void k_keep_compact(const uint32_t *__restrict__ keep, const uint32_t *__restrict__ pos, uint32_t n_rec, uint32_t *__restrict__ idx, BamCtl *ctl) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rec) return;
    if (keep[i]) idx[pos[i]] = i;
    if (i == n_rec - 1) ctl->n_kept = pos[i] + keep[i];
}
// ---- a region list: the stable multi-way partition of region masks (k_bam_filter, k_sam_line_info; the panel set's k_set_route) ---
// One lane per record, PART_TILE records per workgroup.  part_wave_counts: per-slot counts of one wavefront's masks by ballot +
// popcount (lane l leaves with slot l's count: no atomics).  k_part_counts stores a tile's counts slot-major, [n_slots][n_tiles], so
// that ONE k_fe_scan gives every slot's list its start and every tile its place inside it; k_part_scatter adds the wavefronts
// before (LDS) and the lanes before (prefix popcount of the ballot).  No atomic decides a position: the lists are slot after slot,
// input order inside a slot, a record once per slot that keeps it.
constexpr int PART_TILE = 1024;
__device__ __forceinline__ uint32_t part_wave_counts(unsigned long long m, int n_slots, int lane) {
    uint32_t mine = 0;
    for (int l = 0; l < n_slots; ++l) {
        const unsigned long long b = __ballot((int)((m >> l) & 1ull));
        if (lane == l) mine = (uint32_t)__builtin_popcountll(b);
    }
    return mine;
}
template <class M>
__global__ void __launch_bounds__(PART_TILE) k_part_counts(const M *__restrict__ mask, uint32_t n_rec, int n_slots, uint32_t n_tiles,
                                                           uint32_t *__restrict__ cnt /* [n_slots][n_tiles] */) {
    __shared__ uint32_t s_cnt[PART_TILE / 64][64];
    const uint32_t i = blockIdx.x * PART_TILE + threadIdx.x;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const unsigned long long m = i < n_rec ? (unsigned long long)mask[i] : 0ull;
    s_cnt[wv][lane] = part_wave_counts(m, n_slots, lane);
    __syncthreads();
    if ((int)threadIdx.x < n_slots) {
        uint32_t sum = 0;
        for (int w = 0; w < PART_TILE / 64; ++w) sum += s_cnt[w][threadIdx.x];
        cnt[(size_t)threadIdx.x * n_tiles + blockIdx.x] = sum;
    }
}
template <class M>
__global__ void __launch_bounds__(PART_TILE) k_part_scatter(const M *__restrict__ mask, uint32_t n_rec, int n_slots, uint32_t n_tiles,
                                                            const uint32_t *__restrict__ base /* [n_slots][n_tiles] */, uint32_t *__restrict__ idx) {
    __shared__ uint32_t s_cnt[PART_TILE / 64][64];
    __shared__ uint32_t s_base[PART_TILE / 64][64];
    const uint32_t i = blockIdx.x * PART_TILE + threadIdx.x;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const unsigned long long m = i < n_rec ? (unsigned long long)mask[i] : 0ull;
    s_cnt[wv][lane] = part_wave_counts(m, n_slots, lane);
    __syncthreads();
    {
        uint32_t before = 0;
        for (int w = 0; w < wv; ++w) before += s_cnt[w][lane];
        s_base[wv][lane] = before;
    }
    __syncthreads();
    const unsigned long long lanes_before = (1ull << lane) - 1ull;
    for (int l = 0; l < n_slots; ++l) {
        const bool mine = (m >> l) & 1ull;
        const unsigned long long b = __ballot((int)mine);
        if (mine) idx[base[(size_t)l * n_tiles + blockIdx.x] + s_base[wv][l] + (uint32_t)__builtin_popcountll(b & lanes_before)] = i;
    }
}
// QNAME order as hgx_bam.cpp's line_less: bytes, a name that is a prefix of another first
__device__ __forceinline__ int bam_name_cmp(const unsigned char *a, uint32_t la, const unsigned char *b, uint32_t lb) {
    const uint32_t m = la < lb ? la : lb;
    for (uint32_t k = 0; k < m; ++k) if (a[k] != b[k]) return a[k] < b[k] ? -1 : 1;
    return la < lb ? -1 : (la > lb ? 1 : 0);
}
// bytes [8 c, 8 c + 8) of a name, big endian, zero beyond its end (one 8-byte load: it reaches at most 7 bytes beyond the name, into the
// record's next fields or the buffer's padding)
__device__ __forceinline__ unsigned long long name_chunk(const unsigned char *name, uint32_t klen, uint32_t c) {
    if (8 * c >= klen) return 0ull;
    unsigned long long w;
    __builtin_memcpy(&w, name + 8 * c, 8);
    unsigned long long v = __builtin_bswap64(w);
    const uint32_t have = klen - 8 * c;
    if (have < 8) v &= ~0ull << (8 * (8 - have));
    return v;
}
// The name sort on the bits that VARY (round 5, late).  An LSD radix sort over 8-byte chunks of the names costs ~25 library
// launches per chunk; read names differ in a few dozen bit positions (the digits of a counter).  The order check that runs anyway
// also ORs together, per chunk, the XOR of every two neighbouring names -- exactly the bit positions in which not all names
// agree -- and the sort keys are those bits alone, most significant first, packed into 64-bit words (one word, one sort over
// ~30 bits, for the usual names).  Dropping positions in which all keys agree changes no comparison.
#define NAME_DIFF_CHUNKS 32
struct NameDiff { unsigned long long m[NAME_DIFF_CHUNKS]; };
__device__ __forceinline__ void name_diff_add(const unsigned char *a, uint32_t la, const unsigned char *b, uint32_t lb, bool valid, unsigned long long *diff) {
    const uint32_t l = la > lb ? la : lb;
    const uint32_t nc_mine = valid ? (l + 7) / 8 : 0u;
    uint32_t nc = nc_mine;                                                  // chunks this wavefront walks: the longest pair's
#pragma unroll
    for (int d = 32; d; d >>= 1) nc = max(nc, (uint32_t)__shfl_xor((int)nc, d, 64));
    if (nc > NAME_DIFF_CHUNKS) nc = NAME_DIFF_CHUNKS;                       // (longer names: the caller sorts chunk by chunk)
    for (uint32_t c = 0; c < nc; ++c) {
        unsigned long long x = c < nc_mine ? name_chunk(a, la, c) ^ name_chunk(b, lb, c) : 0ull;
#pragma unroll
        for (int d = 32; d; d >>= 1) x |= (unsigned long long)__shfl_xor((long long)x, d, 64);
        if ((threadIdx.x & 63) == 0 && x) atomicOr(&diff[c], x);
    }
}
// word `word` (0 = least significant) of the packed key: the varying bits of all chunks, most significant first
__device__ __forceinline__ unsigned long long name_packed_word(const unsigned char *name, uint32_t klen, const NameDiff &D, int n_chunks, int n_bits, int word) {
    unsigned long long out = 0;
    int p = n_bits;                                                         // bits still to place (the next goes to position p - 1)
    for (int c = 0; c < n_chunks && p > 64 * word; ++c) {
        unsigned long long m = D.m[c];
        if (!m) continue;
        const unsigned long long v = name_chunk(name, klen, (uint32_t)c);
        while (m) {
            const int b = 63 - __builtin_clzll(m);
            m &= ~(1ull << b);
            --p;
            if ((p >> 6) == word) out |= ((v >> b) & 1ull) << (p & 63);
        }
    }
    return out;
}
// Where the names of a stream's entries lie -- all the name-order stage knows of a format.  Entry r (a BAM record, a kept SAM line):
// its offset in the text, its name, the name's length, its task.
struct BamNames {                            // records of the walked table: the name behind the 32 fixed bytes, l_read_name counts its NUL
    const unsigned char *text; const uint32_t *rec_off; const uint16_t *rec_task;
    static constexpr bool has_tasks = true;
    static constexpr const char *lap_sort = "BAM name sort", *lap_check = "BAM name order check";
    __device__ __forceinline__ uint32_t off(uint32_t r) const { return rec_off[r]; }
    __device__ __forceinline__ const unsigned char *name(uint32_t r) const { return text + rec_off[r] + 32; }
    __device__ __forceinline__ uint32_t klen(uint32_t r) const { return (uint32_t)text[rec_off[r] + 8] - 1; }
    __device__ __forceinline__ uint32_t task(uint32_t r) const { return rec_task[r]; }
};
struct SamNames {                            // kept lines of SAM text: the name is the line's first field; one task
    const unsigned char *text; const uint32_t *k_off, *k_klen;
    static constexpr bool has_tasks = false;
    static constexpr const char *lap_sort = "SAM name sort", *lap_check = "SAM name order check";
    __device__ __forceinline__ uint32_t off(uint32_t r) const { return k_off[r]; }
    __device__ __forceinline__ const unsigned char *name(uint32_t r) const { return text + k_off[r]; }
    __device__ __forceinline__ uint32_t klen(uint32_t r) const { return k_klen[r]; }
    __device__ __forceinline__ uint32_t task(uint32_t) const { return 0u; }
};
// is the list idx[0 .. n) in name order inside every task?  (and, with `diff`, which bits of the names vary)
template <class S>
__global__ void __launch_bounds__(256) k_name_sorted(S src, const uint32_t *__restrict__ idx, uint32_t n, BamCtl *ctl, unsigned long long *__restrict__ diff) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = i > 0 && i < n;
    const uint32_t ra = idx[valid ? i - 1 : 0], rb = idx[valid ? i : 0];
    const unsigned char *a = src.name(ra), *b = src.name(rb);
    const uint32_t la = src.klen(ra), lb = src.klen(rb);
    if (diff) name_diff_add(a, la, b, lb, valid, diff);                    // (names of more than one 8-byte chunk: the sort will want it)
    if (!valid) return;
    if (S::has_tasks) {
        // (one region per task: the entries are in task order before the sort, only names inside a task matter; a region-major list of
        // several tasks is not -- the sort's task key brings the tasks together again)
        const uint32_t ta = src.task(ra), tb = src.task(rb);
        if (ta != tb) { if (ta > tb) ctl->unsorted = 1; return; }
    }
    if (bam_name_cmp(b, lb, a, la) < 0) ctl->unsorted = 1;
}
template <class S>
__global__ void __launch_bounds__(256) k_name_key_packed(S src, const uint32_t *__restrict__ idx, uint32_t n, NameDiff D, int n_chunks, int n_bits, int word,
                                                         unsigned long long *__restrict__ key) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t r = idx[i];
    key[i] = name_packed_word(src.name(r), src.klen(r), D, n_chunks, n_bits, word);
}
// bytes [8 c, 8 c + 8) of every name, big endian, zero beyond its end: LSD radix passes over these give the byte order above
template <class S>
__global__ void __launch_bounds__(256) k_name_key(S src, const uint32_t *__restrict__ idx, uint32_t n, uint32_t chunk, unsigned long long *__restrict__ key) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t r = idx[i];
    key[i] = name_chunk(src.name(r), src.klen(r), chunk);
}
// the line table of the ordered list (`off_base`: the text is a part of a larger one that starts off_base bytes into it)
template <class S>
__global__ void k_name_lines(S src, const uint32_t *__restrict__ len, const uint32_t *__restrict__ idx, uint32_t n, uint32_t off_base, FeLine *__restrict__ lines) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { const uint32_t r = idx[i]; lines[i] = FeLine{off_base + src.off(r), len[r], src.task(r)}; }
}
__global__ void k_bam_task_key(const uint16_t *__restrict__ rec_task, const uint32_t *__restrict__ idx, uint32_t n, unsigned long long *__restrict__ key) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) key[i] = rec_task[idx[i]];
}

// The record table of unwalked BAM streams (resident at d_text: one per task, at `bases`): the chains walked in ranges, linked, and
// (offset, length, task) of every record written in (task, file order).  The first half of bam_lines_dev, and what an
// hgx_alignment_set keeps beside its inflated streams.
struct BamTable {
    DevBuf b_seg, b_act, b_span, b_ctl, b_off, b_len, b_task;
    int n_seg = 0;
    int max_regions = 0;                 // the longest region list among the tasks (0: nothing is filtered)
    uint32_t n_rec = 0;
};
int bam_table_dev(const unsigned char *text, const std::vector<const hgx_bam_deferred *> &defs, const std::vector<size_t> &bases, const std::vector<size_t> &sizes,
                  hipStream_t st, BamTable &T, int *declined, Lap &lap) {
    *declined = 0;
    const int n_seg = (int)defs.size();
    if (n_seg < 1 || n_seg > 65535) { *declined = HGX_FE_DECLINE_SIZE; return HGX_OK; }
    std::vector<BamSeg> segs((size_t)n_seg);
    std::vector<uint8_t> acts;
    std::vector<BamSpan> spans;
    size_t total_body = 0;
    for (int t = 0; t < n_seg; ++t) {
        if (defs[t]->n_regions() > HGX_MAX_REGIONS) { *declined = HGX_FE_DECLINE_SIZE; return HGX_OK; }
        if (defs[t]->body0 > sizes[t] || bases[t] + sizes[t] >= (1ull << 32) - 64) { *declined = HGX_FE_DECLINE_SIZE; return HGX_OK; }
        total_body += sizes[t] - defs[t]->body0;
    }
    // ranges: ~16 KB of records each, at most 8192 for a lone stream, shared out by size among many
    // Ranges of ~8 KB (about twenty records).  Measured at 1 M records (tools/walk_ranges.sh): the first walk takes 0.41 / 0.34 /
    // 0.32 / 0.32 / 0.35 ms with ranges of 48 / 16 / 8 / 4 / 2 KB -- most of it the scan for each range's first record, the walk
    // itself (the second pass: 0.04 ms) is a short chain of dependent loads per range.
    const size_t W_all = std::max<size_t>((size_t)n_seg, std::min<size_t>(((size_t)1 << 20) + (size_t)n_seg, total_body / 8192 + 1));
    uint32_t w_at = 0;
    for (int t = 0; t < n_seg; ++t) {
        const hgx_bam_deferred &d = *defs[t];
        BamSeg &G = segs[t];
        G.base = (uint32_t)bases[t]; G.n = (uint32_t)sizes[t]; G.body0 = (uint32_t)d.body0;
        G.n_ref = (int32_t)d.ref_action.size();
        G.act_off = (uint32_t)acts.size();
        acts.insert(acts.end(), d.ref_action.begin(), d.ref_action.end());
        G.filtered = d.filtered ? 1u : 0u; G.left0 = (long long)d.left0; G.right0 = (long long)d.right0;
        G.n_regions = (uint32_t)d.n_regions(); G.span_off = (uint32_t)spans.size();
        for (int g = 1; g < d.n_regions(); ++g) {                               // (region-major rows: act_off + g * n_ref)
            acts.insert(acts.end(), d.action_of(g).begin(), d.action_of(g).end());
            spans.push_back(BamSpan{(long long)d.left_of(g), (long long)d.right_of(g)});
        }
        T.max_regions = std::max(T.max_regions, d.n_regions());
        const size_t body = sizes[t] - d.body0;
        G.first_range = w_at;
        G.n_ranges = (uint32_t)std::max<size_t>(1, total_body ? (W_all * body + total_body - 1) / total_body : 1);
        w_at += G.n_ranges;
    }
    const int W = (int)w_at;
    DevBuf b_rng, b_base, b_cnt, b_tmpw;
    Drain drain{st};
    ALLOC(T.b_seg, (size_t)n_seg * sizeof(BamSeg));
    ALLOC(b_rng, (size_t)W * sizeof(BamRange));
    ALLOC(b_base, (size_t)W * 4);
    ALLOC(b_cnt, (size_t)W * 4);
    ALLOC(T.b_ctl, sizeof(BamCtl));
    ALLOC(T.b_act, std::max<size_t>(acts.size(), 16));
    ALLOC(T.b_span, std::max<size_t>(spans.size(), 1) * sizeof(BamSpan));
    if (!spans.empty()) HIPCHK(hipMemcpyAsync(T.b_span.p, spans.data(), spans.size() * sizeof(BamSpan), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(T.b_ctl.p, 0, sizeof(BamCtl), st));
    HIPCHK(hipMemcpyAsync(T.b_seg.p, segs.data(), (size_t)n_seg * sizeof(BamSeg), hipMemcpyHostToDevice, st));
    if (!acts.empty()) HIPCHK(hipMemcpyAsync(T.b_act.p, acts.data(), acts.size(), hipMemcpyHostToDevice, st));
    BamCtl *ctl = T.b_ctl.as<BamCtl>();
    const BamSeg *d_seg = T.b_seg.as<BamSeg>();
    k_bam_walk<0><<<nblk(W, 64), 64, 0, st>>>(text, d_seg, n_seg, W, b_rng.as<BamRange>(), nullptr, nullptr, nullptr, nullptr);
    k_bam_link<<<nblk(W, 256), 256, 0, st>>>(b_rng.as<BamRange>(), d_seg, n_seg, W, b_cnt.as<uint32_t>(), ctl);
    {
        ALLOC(b_tmpw, fe_scan_scratch_bytes(W));
        HIPCHK(hipMemsetAsync(b_tmpw.p, 0, fe_scan_scratch_bytes(W), st));
        FeScanArgs sa{};
        sa.n_ch = 1;
        sa.ch[0] = FeScanCh{b_cnt.p, b_base.as<uint32_t>(), 0, FSC_U32};
        sa.totals = ctl->tot;                                                  // (the records of all ranges)
        const int rcs = fe_scan(sa, W, b_tmpw.p, st);
        if (rcs) return rcs;
    }
    BamCtl h;
    { const int rc_r = ctl_read(&h, ctl, st); if (rc_r) return rc_r; }
    lap("BAM record walk (ranges)");
    if (h.decline) { *declined = h.decline; return HGX_OK; }
    const uint32_t n_rec = h.tot[0];
    if (n_rec >= (1u << 30)) { *declined = HGX_FE_DECLINE_SIZE; return HGX_OK; }
    T.n_seg = n_seg;
    T.n_rec = n_rec;
    if (n_rec == 0) return HGX_OK;
    ALLOC(T.b_off, (size_t)n_rec * 4); ALLOC(T.b_len, (size_t)n_rec * 4); ALLOC(T.b_task, (size_t)n_rec * 2 + 16);
    k_bam_walk<1><<<nblk(W, 64), 64, 0, st>>>(text, d_seg, n_seg, W, b_rng.as<BamRange>(), b_base.as<uint32_t>(), T.b_off.as<uint32_t>(), T.b_len.as<uint32_t>(),
                                             T.b_task.as<uint16_t>());
    HIPCHK(hipGetLastError());
    return HGX_OK;
}

// The name-order stage, one for both formats (S: BamNames / SamNames): the n entries `idx` names (task after task, or region after
// region over all tasks) brought into QNAME order inside every task -- stable: list order among equal names.  The order check runs
// first and collects the varying bits of the names on its way; a list in order (an aligner writes its records grouped by read
// already) is left as it is.  `idx` is only read (an hgx_alignment_set's lists serve many calls): the sort ping-pongs in buffers of
// `B`, and *ordered is `idx` itself or one of them -- the caller keeps `B` until its last kernel over *ordered has run.  `ctl` is a
// control block whose `unsorted` is still zero.  With `unsorted_out`, a list out of order is reported and not sorted.
struct NameOrder { DevBuf b_diff, b_idx_a, b_idx_b, b_key, b_key2, b_tmp; };
template <class S>
int name_order(const S &src, const uint32_t *idx, uint32_t n, uint32_t max_klen, int n_seg, BamCtl *ctl, hipStream_t st, Lap &lap, NameOrder &B,
               const uint32_t **ordered, int *unsorted_out = nullptr) {
    *ordered = idx;
    if (n < 2) return HGX_OK;
    ALLOC(B.b_diff, sizeof(NameDiff));
    HIPCHK(hipMemsetAsync(B.b_diff.p, 0, sizeof(NameDiff), st));
    // names of one 8-byte chunk are sorted as they are (one sort either way); longer ones on their varying bits
    const int n_chunks = (int)(max_klen + 7) / 8;
    const bool packed = n_chunks >= 2 && n_chunks <= NAME_DIFF_CHUNKS && !hgx_switch_has("front", "name_chunks");
    k_name_sorted<S><<<nblk(n, 256), 256, 0, st>>>(src, idx, n, ctl, packed ? B.b_diff.as<unsigned long long>() : (unsigned long long *)nullptr);
    NameDiff nd;
    BamCtl h;
    { const int rc_d = hgx_d2h(&nd, B.b_diff.p, sizeof(NameDiff), st); if (rc_d) { (void)hgx_sync(st); return rc_d; } }
    { const int rc_r = ctl_read(&h, ctl, st); if (rc_r) return rc_r; }
    if (h.unsorted && unsorted_out) { *unsorted_out = 1; return HGX_OK; }
    if (h.unsorted) {
        size_t tmp_bytes = 0;
        (void)hipcub::DeviceRadixSort::SortPairs((void *)nullptr, tmp_bytes, (unsigned long long *)nullptr, (unsigned long long *)nullptr, (uint32_t *)nullptr,
                                                 (uint32_t *)nullptr, (int)n, 0, 64, st);
        ALLOC(B.b_tmp, std::max<size_t>(tmp_bytes, 256));
        ALLOC(B.b_idx_a, (size_t)n * 4); ALLOC(B.b_idx_b, (size_t)n * 4); ALLOC(B.b_key, (size_t)n * 8); ALLOC(B.b_key2, (size_t)n * 8);
        unsigned long long *key = B.b_key.as<unsigned long long>(), *key_alt = B.b_key2.as<unsigned long long>();
        uint32_t *nxt = B.b_idx_a.as<uint32_t>();
        // one stable pass over the low `bits` bits of `key`, from the list at hand into the other buffer
        auto sort_pass = [&](int bits) -> int {
            size_t b = tmp_bytes;
            HIPCHK(hipcub::DeviceRadixSort::SortPairs(B.b_tmp.p, b, key, key_alt, idx, nxt, (int)n, 0, bits, st));
            idx = nxt;
            nxt = nxt == B.b_idx_a.as<uint32_t>() ? B.b_idx_b.as<uint32_t>() : B.b_idx_a.as<uint32_t>();
            return HGX_OK;
        };
        int n_bits = 0;
        for (int c = 0; c < std::min(n_chunks, NAME_DIFF_CHUNKS); ++c) n_bits += __builtin_popcountll(nd.m[c]);
        if (packed) {
            // the varying bits alone, 64 to a word, least significant word first; every pass stable
            for (int word = 0; word < (n_bits + 63) / 64; ++word) {
                k_name_key_packed<S><<<nblk(n, 256), 256, 0, st>>>(src, idx, n, nd, n_chunks, n_bits, word, key);
                const int rc_p = sort_pass(std::min(64, n_bits - 64 * word));
                if (rc_p) return rc_p;
            }
        } else
        for (int chunk = n_chunks - 1; chunk >= 0; --chunk) {      // (names beyond 256 bytes; test switch front=name_chunks) eight bytes at a time, least significant first
            k_name_key<S><<<nblk(n, 256), 256, 0, st>>>(src, idx, n, (uint32_t)chunk, key);
            const int rc_p = sort_pass(64);
            if (rc_p) return rc_p;
        }
        if constexpr (S::has_tasks) if (n_seg > 1) {                               // ... and the tasks apart again, names in order inside
            k_bam_task_key<<<nblk(n, 256), 256, 0, st>>>(src.rec_task, idx, n, key);
            const int rc_p = sort_pass(16);
            if (rc_p) return rc_p;
        }
    }
    lap(h.unsorted ? S::lap_sort : S::lap_check);
    *ordered = idx;
    return HGX_OK;
}

// ... and its second half, on an index list: the n_kept records `idx` names (task after task, file order inside a task) brought into
// QNAME order inside every task (name_order) and written as the line table.  `idx` is only read; `ctl` is a zeroed control block of
// the caller's.
int bam_lines_of(const unsigned char *text, const uint32_t *rec_off, const uint32_t *rec_len, const uint16_t *rec_task, int n_seg, const uint32_t *idx,
                 uint32_t n_kept, uint32_t max_klen, BamCtl *ctl, hipStream_t st, DevBuf &b_lines, Lap &lap) {
    NameOrder order;
    Drain drain{st};     // (the last kernels read this function's buffers)
    const BamNames src{text, rec_off, rec_task};
    { const int rc_o = name_order(src, idx, n_kept, max_klen, n_seg, ctl, st, lap, order, &idx); if (rc_o) return rc_o; }
    if (n_kept) k_name_lines<BamNames><<<nblk(n_kept, 256), 256, 0, st>>>(src, rec_len, idx, n_kept, 0u, b_lines.as<LineRef>());
    HIPCHK(hipGetLastError());
    return HGX_OK;
}

// The kept list of a region mask: mask[i] bit g = region g keeps entry i (one region or none: 0 / 1).  Leaves in K.b_idx the entries
// kept, region after region, input order inside a region, an entry once per region that keeps it (one region: a scan and a
// compaction; a list: the stable partition k_part_*), and their number in ctl->n_kept.  n > 0.
struct KeptList { DevBuf b_pos, b_cnt, b_tmp, b_idx; };
int kept_list(const uint32_t *mask, uint32_t n, int n_reg, BamCtl *ctl, hipStream_t st, KeptList &K) {
    const uint32_t n_tiles = (n + PART_TILE - 1) / PART_TILE;
    const size_t n_scan = n_reg > 1 ? (size_t)n_reg * n_tiles : (size_t)n;
    ALLOC(K.b_pos, n_scan * 4);
    ALLOC(K.b_idx, (size_t)n * (size_t)std::max(n_reg, 1) * 4);
    ALLOC(K.b_tmp, std::max<size_t>(fe_scan_scratch_bytes((long)n_scan), 256));
    HIPCHK(hipMemsetAsync(K.b_tmp.p, 0, fe_scan_scratch_bytes((long)n_scan), st));
    FeScanArgs sa{};
    sa.n_ch = 1;
    sa.ch[0] = FeScanCh{mask, K.b_pos.as<uint32_t>(), 0, FSC_U32};
    if (n_reg > 1) {
        ALLOC(K.b_cnt, n_scan * 4);
        k_part_counts<uint32_t><<<n_tiles, PART_TILE, 0, st>>>(mask, n, n_reg, n_tiles, K.b_cnt.as<uint32_t>());
        sa.ch[0].in = K.b_cnt.p;
        sa.totals = &ctl->n_kept;
    }
    const int rcs = fe_scan(sa, (long)n_scan, K.b_tmp.p, st);
    if (rcs) return rcs;
    if (n_reg > 1) k_part_scatter<uint32_t><<<n_tiles, PART_TILE, 0, st>>>(mask, n, n_reg, n_tiles, K.b_pos.as<uint32_t>(), K.b_idx.as<uint32_t>());
    else k_keep_compact<<<nblk(n, 256), 256, 0, st>>>(mask, K.b_pos.as<uint32_t>(), n, K.b_idx.as<uint32_t>(), ctl);
    return HGX_OK;
}

// the line table of unwalked BAM streams, made on the device: (offset, length, task) of the records the tasks' regions keep, task
// after task, in QNAME order inside a task (stable: file order among equal names) -- what hgx_bam.cpp's walk + filter + sort_lines
// give per file
int bam_lines_dev(const char *d_text, const std::vector<const hgx_bam_deferred *> &defs, const std::vector<size_t> &bases, const std::vector<size_t> &sizes,
                  hipStream_t st, DevBuf &b_lines, uint32_t *n_lines, int *declined) {
    *declined = 0;
    *n_lines = 0;
    Lap lap(st);
    const unsigned char *text = (const unsigned char *)d_text;
    BamTable T;
    DevBuf b_keep;
    KeptList K;
    Drain drain{st};
    { const int rc_t = bam_table_dev(text, defs, bases, sizes, st, T, declined, lap); if (rc_t || *declined) return rc_t; }
    const uint32_t n_rec = T.n_rec;
    const int n_seg = T.n_seg;
    BamCtl *ctl = T.b_ctl.as<BamCtl>();
    // a region list: the kept list may be longer than the record table (a record once per region that keeps it)
    const int n_reg = T.max_regions;
    if (n_reg > 1 && (unsigned long long)n_rec * (unsigned long long)n_reg >= (1ull << 30)) { *declined = HGX_FE_DECLINE_SIZE; return HGX_OK; }
    if (n_rec == 0) { ALLOC(b_lines, sizeof(LineRef)); return HGX_OK; }
    ALLOC(b_keep, (size_t)n_rec * 4);
    k_bam_filter<<<nblk(n_rec, 256), 256, 0, st>>>(text, T.b_off.as<uint32_t>(), T.b_len.as<uint32_t>(), T.b_task.as<uint16_t>(), n_rec, T.b_seg.as<BamSeg>(),
                                                   T.b_act.as<uint8_t>(), T.b_span.as<BamSpan>(), b_keep.as<uint32_t>(), ctl);
    // (a region list: region after region over all tasks, file order inside; bam_lines_of's name sort and its stable task key make of
    // it, per task, what the host reader's lists + sort give)
    { const int rc_k = kept_list(b_keep.as<uint32_t>(), n_rec, n_reg, ctl, st, K); if (rc_k) return rc_k; }
    BamCtl h;
    { const int rc_r = ctl_read(&h, ctl, st); if (rc_r) return rc_r; }
    lap("BAM records + region filter");
    if (h.decline) { *declined = h.decline; return HGX_OK; }
    const uint32_t n_kept = h.n_kept;
    ALLOC(b_lines, std::max<size_t>(n_kept, 1) * sizeof(LineRef));
    const int rc_l = bam_lines_of(text, T.b_off.as<uint32_t>(), T.b_len.as<uint32_t>(), T.b_task.as<uint16_t>(), n_seg, K.b_idx.as<uint32_t>(), n_kept, h.max_klen, ctl, st,
                                  b_lines, lap);
    if (rc_l) return rc_l;
    *n_lines = n_kept;
    return HGX_OK;
}

// ---- the line table of SAM TEXT on the device (round 5) --------------------------------------------------------------
// What hgx_bam.cpp's readers do per line on the host's threads (0.2-0.3 CPU-seconds per 1 M-read call: memchr for the newlines,
// six fields of every line for the region test, the QNAME order check): here the text that went up is scanned where it lies.
//   k_sam_nl<0/1>    newlines per 4 KB tile (a wavefront reads 1 KB per step, 16 bytes per lane, a SWAR zero-byte test per dword),
//                    a scan of the tile counts, then the same walk again writing every line's start
//   k_sam_line_info  a lane per line: '\r' stripped, blank and '@' lines dropped, the region test of `samtools view` on RNAME, POS and
//                    the CIGAR's reference span against every region of the list (hgx_bam_deferred; a region MASK), QNAME length
//   scan + k_sam_compact (one region), or kept_list + k_sam_gather (a region list): the kept lines' offset, length, name length,
//   name_order<SamNames> (QNAME order check; the sort where the text is not in name order, as for BAM), k_name_lines -> FeLine
struct SamRegion { int whole_len, name_len; long long left0, right0; char whole[96], name[96]; };
struct SamRegions { int filtered, n; SamRegion r[HGX_MAX_REGIONS]; };       // (uploaded: the list is beyond what a launch's arguments should carry)
#include "hgx_nl_tiles.hpp"            // SAM_TILE, sam_nl_mask, k_sam_nl<0/1>: shared with the aligner's read table (hgx_reads.hip)
__device__ __forceinline__ bool sam_bytes_eq(const unsigned char *a, const char *b, int n) {
    for (int i = 0; i < n; ++i) if (a[i] != (unsigned char)b[i]) return false;
    return true;
}
__global__ void __launch_bounds__(256) k_sam_line_info(const unsigned char *__restrict__ text, size_t n, const uint32_t *__restrict__ starts, uint32_t n_all,
                                                       const SamRegions *__restrict__ Rp, uint32_t *__restrict__ keep, uint32_t *__restrict__ l_len, uint32_t *__restrict__ l_klen,
                                                       BamCtl *ctl) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_all) return;
    const uint32_t off = starts[i];
    uint32_t end = i + 1 < n_all ? starts[i + 1] - 1u : (uint32_t)n;             // the newline's place (or the text's end: a last line without one)
    if (end < off) end = off;
    if (end > off && text[end - 1] == '\r') --end;
    const uint32_t len = end - off;
    uint32_t k = 0, klen = 0;                                                    // k: the line's region mask (nothing filtered: 0 / 1)
    const int r_filtered = Rp->filtered, r_n = Rp->n;
    if (len && text[off] != '@') {
        // QNAME and, for the region test, FLAG / RNAME / POS / CIGAR (hgx_bam.cpp take_line)
        const unsigned char *p = text + off;
        uint32_t tab[6];
        int nf = 0;
        const int want = r_filtered ? 6 : 1;
        // the first `want` tabs, eight bytes per look (an exact zero-byte test of word ^ tabs gives their places)
        for (uint32_t q = 0; q < len && nf < want;) {
            if (q + 8 <= len) {
                unsigned long long w;
                __builtin_memcpy(&w, p + q, 8);
                const unsigned long long x = w ^ 0x0909090909090909ULL;
                unsigned long long m = ~(((x & 0x7F7F7F7F7F7F7F7FULL) + 0x7F7F7F7F7F7F7F7FULL) | x) & 0x8080808080808080ULL;
                while (m && nf < want) { tab[nf++] = q + (uint32_t)(__builtin_ctzll(m) >> 3); m &= m - 1; }
                q += 8;
            } else {
                if (p[q] == '\t') tab[nf++] = q;
                ++q;
            }
        }
        klen = nf ? tab[0] : len;
        if (!r_filtered) k = 1;
        else if (nf == 6) {
            long long flag = 0, pos = 0;
            bool fneg = false, pneg = false;
            {   // strtol(.., 10): optional blanks and sign, digits (what follows is ignored)
                uint32_t q = tab[0] + 1;
                while (q < tab[1] && (p[q] == ' ' || (p[q] >= 9 && p[q] <= 13))) ++q;
                if (q < tab[1] && (p[q] == '+' || p[q] == '-')) { fneg = p[q] == '-'; ++q; }
                for (; q < tab[1] && p[q] >= '0' && p[q] <= '9'; ++q) if (flag < (1ll << 40)) flag = flag * 10 + (p[q] - '0');
                if (fneg) flag = -flag;
                q = tab[2] + 1;
                while (q < tab[3] && (p[q] == ' ' || (p[q] >= 9 && p[q] <= 13))) ++q;
                if (q < tab[3] && (p[q] == '+' || p[q] == '-')) { pneg = p[q] == '-'; ++q; }
                for (; q < tab[3] && p[q] >= '0' && p[q] <= '9'; ++q) if (pos < (1ll << 40)) pos = pos * 10 + (p[q] - '0');
                if (pneg) pos = -pos;
            }
            const long long pos0 = pos - 1;
            long long reflen = 0;
            if (!(flag & 4)) {
                long long num = 0;
                for (uint32_t q = tab[4] + 1; q < tab[5]; ++q) {
                    const unsigned char c = p[q];
                    if (c >= '0' && c <= '9') { num = num * 10 + (c - '0'); continue; }
                    if (c == 'M' || c == 'D' || c == 'N' || c == '=' || c == 'X') reflen += num;
                    num = 0;
                }
            }
            const long long end0 = pos0 + (reflen > 0 ? reflen : 1) - 1;
            const unsigned char *rn = p + tab[1] + 1;
            const int rl = (int)(tab[2] - tab[1] - 1);
            for (int g = 0; g < r_n; ++g) {
                const SamRegion &R = Rp->r[g];
                if (rl == R.whole_len && sam_bytes_eq(rn, R.whole, rl)) k |= 1u << g;
                else if (R.name_len > 0 && rl == R.name_len && sam_bytes_eq(rn, R.name, rl)) k |= ((end0 >= R.left0 && pos0 <= R.right0) ? 1u : 0u) << g;
            }
        }
    }
    keep[i] = k;
    l_len[i] = len;
    l_klen[i] = klen;
    if (k) atomicMax(&ctl->max_klen, klen);
}
// the kept lines side by side (k_off / k_len / k_klen; idx = the list name_order starts from: 0, 1, 2, ...).  One region: fused with the
// compaction (kept_list + k_sam_gather would be one launch more per part of a text: 0.015 ms on a 0.17 ms lap) ...
__global__ void k_sam_compact(const uint32_t *__restrict__ keep, const uint32_t *__restrict__ pos, const uint32_t *__restrict__ starts, const uint32_t *__restrict__ l_len,
                              const uint32_t *__restrict__ l_klen, uint32_t n_all, uint32_t *__restrict__ k_off, uint32_t *__restrict__ k_len,
                              uint32_t *__restrict__ k_klen, uint32_t *__restrict__ idx, BamCtl *ctl) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_all) return;
    if (keep[i]) { const uint32_t q = pos[i]; k_off[q] = starts[i]; k_len[q] = l_len[i]; k_klen[q] = l_klen[i]; idx[q] = q; }
    if (i == n_all - 1) ctl->n_kept = pos[i] + keep[i];
}
// ... a region list: behind kept_list (src[q] = the line at place q of the region-after-region list)
__global__ void k_sam_gather(const uint32_t *__restrict__ src, uint32_t n_kept, const uint32_t *__restrict__ starts, const uint32_t *__restrict__ l_len,
                             const uint32_t *__restrict__ l_klen, uint32_t *__restrict__ k_off, uint32_t *__restrict__ k_len, uint32_t *__restrict__ k_klen,
                             uint32_t *__restrict__ idx) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n_kept) return;
    const uint32_t i = src[q];
    k_off[q] = starts[i]; k_len[q] = l_len[i]; k_klen[q] = l_klen[i]; idx[q] = q;
}

// `off_base`: d_text is a PART of a larger text that starts off_base bytes into it (the lines' offsets count from the whole text's
// first byte).  `unsorted_out` != NULL: a text that is not in name order is not sorted here -- *unsorted_out = 1, no lines.
int sam_lines_dev(const char *d_text, size_t n_bytes, const hgx_bam_deferred &def, hipStream_t st, DevBuf &b_lines, uint32_t *n_lines, int *declined,
                  uint32_t off_base = 0, int *unsorted_out = nullptr) {
    *declined = 0;
    *n_lines = 0;
    if (unsorted_out) *unsorted_out = 0;
    Lap lap(st);
    const unsigned char *text = (const unsigned char *)d_text;
    if (n_bytes >= (1ull << 32) - 64) { *declined = HGX_FE_DECLINE_SIZE; return HGX_OK; }
    SamRegions RS;
    memset(&RS, 0, sizeof(RS));
    RS.filtered = def.filtered ? 1 : 0;
    RS.n = def.n_regions();
    if (RS.n > HGX_MAX_REGIONS) { *declined = HGX_FE_DECLINE_SIZE; return HGX_OK; }
    for (int g = 0; g < RS.n; ++g) {
        SamRegion &R = RS.r[g];
        const std::string &whole = def.whole_of(g), &name = def.name_of(g);
        if (whole.size() >= sizeof(R.whole) || name.size() >= sizeof(R.name)) { *declined = HGX_FE_DECLINE_SIZE; return HGX_OK; }
        R.whole_len = (int)whole.size(); memcpy(R.whole, whole.data(), whole.size());
        R.name_len = (int)name.size(); memcpy(R.name, name.data(), name.size());
        R.left0 = (long long)def.left_of(g); R.right0 = (long long)def.right_of(g);
    }
    const int n_reg = RS.n;
    const uint32_t n_tiles = (uint32_t)((n_bytes + SAM_TILE - 1) / SAM_TILE);
    DevBuf b_cnt, b_base, b_ctl, b_starts, b_keep, b_pos, b_tmp, b_len, b_klen, b_koff, b_k_len, b_k_klen, b_idx, b_reg;
    KeptList K;
    NameOrder order;
    Drain drain{st};     // (the uploads below read this frame's RS)
    ALLOC(b_reg, sizeof(SamRegions));
    HIPCHK(hipMemcpyAsync(b_reg.p, &RS, sizeof(SamRegions), hipMemcpyHostToDevice, st));
    const size_t sc_t = fe_scan_scratch_bytes(std::max<uint32_t>(n_tiles, 1));
    ALLOC(b_cnt, std::max<size_t>(n_tiles, 1) * 4);
    ALLOC(b_base, std::max<size_t>(n_tiles, 1) * 4);
    ALLOC(b_ctl, 256 + sc_t);
    HIPCHK(hipMemsetAsync(b_ctl.p, 0, 256 + sc_t, st));
    BamCtl *ctl = b_ctl.as<BamCtl>();
    BamCtl h;
    memset(&h, 0, sizeof(h));
    if (n_tiles) {
        k_sam_nl<0><<<nblk(n_tiles, 4), 256, 0, st>>>(text, n_bytes, n_tiles, b_cnt.as<uint32_t>(), nullptr, nullptr);
        FeScanArgs sa{};
        sa.n_ch = 1;
        sa.ch[0] = FeScanCh{b_cnt.p, b_base.as<uint32_t>(), 0, FSC_U32};
        sa.totals = ctl->tot;
        const int rcs = fe_scan(sa, (long)n_tiles, (char *)b_ctl.p + 256, st);
        if (rcs) return rcs;
        { const int rc_r = ctl_read(&h, ctl, st); if (rc_r) return rc_r; }
    }
    // lines = newlines (+ a last line without one); one more entry than lines for "the next line's start"
    const uint32_t n_nl = h.tot[0];
    ALLOC(b_starts, ((size_t)n_nl + 2) * 4);
    HIPCHK(hipMemsetAsync(b_starts.p, 0, 4, st));                            // the first line starts at 0
    if (n_tiles) k_sam_nl<1><<<nblk(n_tiles, 4), 256, 0, st>>>(text, n_bytes, n_tiles, nullptr, b_base.as<uint32_t>(), b_starts.as<uint32_t>());
    // (a text that ends with its last newline has no line behind it; k_sam_line_info drops the empty one)
    const uint32_t n_all = n_nl + 1;
    lap("SAM newline scan");
    if (n_all >= (1u << 30)) { *declined = HGX_FE_DECLINE_SIZE; return HGX_OK; }
    // a region list: the kept list may be longer than the line table (a line once per region that keeps it)
    if (n_reg > 1 && (unsigned long long)n_all * (unsigned long long)n_reg >= (1ull << 30)) { *declined = HGX_FE_DECLINE_SIZE; return HGX_OK; }
    const size_t n_out = (size_t)n_all * (size_t)std::max(n_reg, 1);
    ALLOC(b_keep, (size_t)n_all * 4); ALLOC(b_len, (size_t)n_all * 4); ALLOC(b_klen, (size_t)n_all * 4);
    ALLOC(b_koff, n_out * 4); ALLOC(b_k_len, n_out * 4); ALLOC(b_k_klen, n_out * 4); ALLOC(b_idx, n_out * 4);
    k_sam_line_info<<<nblk(n_all, 256), 256, 0, st>>>(text, n_bytes, b_starts.as<uint32_t>(), n_all, b_reg.as<SamRegions>(), b_keep.as<uint32_t>(), b_len.as<uint32_t>(),
                                                      b_klen.as<uint32_t>(), ctl);
    if (n_reg > 1) {
        // region after region, file order inside; the name sort below is stable over it
        { const int rc_k = kept_list(b_keep.as<uint32_t>(), n_all, n_reg, ctl, st, K); if (rc_k) return rc_k; }
        { const int rc_r = ctl_read(&h, ctl, st); if (rc_r) return rc_r; }
        if (h.n_kept) k_sam_gather<<<nblk(h.n_kept, 256), 256, 0, st>>>(K.b_idx.as<uint32_t>(), h.n_kept, b_starts.as<uint32_t>(), b_len.as<uint32_t>(), b_klen.as<uint32_t>(),
                                                                       b_koff.as<uint32_t>(), b_k_len.as<uint32_t>(), b_k_klen.as<uint32_t>(), b_idx.as<uint32_t>());
    } else {
        ALLOC(b_pos, (size_t)n_all * 4);
        ALLOC(b_tmp, std::max<size_t>(fe_scan_scratch_bytes((long)n_all), 256));
        HIPCHK(hipMemsetAsync(b_tmp.p, 0, fe_scan_scratch_bytes((long)n_all), st));
        FeScanArgs sa{};
        sa.n_ch = 1;
        sa.ch[0] = FeScanCh{b_keep.p, b_pos.as<uint32_t>(), 0, FSC_U32};
        const int rcs = fe_scan(sa, (long)n_all, b_tmp.p, st);
        if (rcs) return rcs;
        k_sam_compact<<<nblk(n_all, 256), 256, 0, st>>>(b_keep.as<uint32_t>(), b_pos.as<uint32_t>(), b_starts.as<uint32_t>(), b_len.as<uint32_t>(), b_klen.as<uint32_t>(),
                                                        n_all, b_koff.as<uint32_t>(), b_k_len.as<uint32_t>(), b_k_klen.as<uint32_t>(), b_idx.as<uint32_t>(), ctl);
        { const int rc_r = ctl_read(&h, ctl, st); if (rc_r) return rc_r; }
    }
    lap("SAM lines + region filter");
    const uint32_t n_kept = h.n_kept;
    // QNAME is at most 254 characters (SAM specification 1.4; a BAM's l_read_name caps it at 255 with the NUL): a longer "name" is a
    // malformed or tab-less line -- its length would become the number of 8-byte sort passes below (a 1 MB line: ~130 000 of them)
    // before the record stage declined it anyway.  The host stages take the call and word the error.
    if (h.max_klen > 254) { *declined = HGX_FE_DECLINE_RECORD; return HGX_OK; }
    ALLOC(b_lines, std::max<size_t>(n_kept, 1) * sizeof(LineRef));
    const SamNames src{text, b_koff.as<uint32_t>(), b_k_klen.as<uint32_t>()};
    const uint32_t *idx = b_idx.as<uint32_t>();
    { const int rc_o = name_order(src, idx, n_kept, h.max_klen, 1, ctl, st, lap, order, &idx, unsorted_out); if (rc_o) return rc_o; }
    if (unsorted_out && *unsorted_out) return HGX_OK;
    if (n_kept) k_name_lines<SamNames><<<nblk(n_kept, 256), 256, 0, st>>>(src, b_k_len.as<uint32_t>(), idx, n_kept, off_base, b_lines.as<LineRef>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));                                           // (idx may live in a buffer of `order`)
    *n_lines = n_kept;
    return HGX_OK;
}

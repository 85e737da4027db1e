// hgx_align_linear.hip -- the kernels of the "hgx" aligner on a linear index (gfx950, wave64).  The candidate test,
// the key and the record text are the core's (hgx_align_linear_core.hpp), the same code the host route runs; this unit is the index
// in HBM, the grids and the chunks.  A unit of its own: the graph aligner's code object (hgx_align.hip) stays as it was.
//
// The reads are taken in SPANS of up to SPAN_READS; a span is cut into CHUNKS on the host from its candidate counts, so that the
// device memory of a chunk is bounded by a budget that does not grow with the allele count (a 7 000-allele family has ~20 000
// candidates per read: chunks get shorter, not larger).  Stages:
//   per span
//     k_alnl_pack     a lane per (read, strand): the oriented read as three bit planes of 4 words (96 B)
//     k_alnl_count    a lane per (read, strand, seed): the seed's code, its bucket in the seed table by bisection: size and begin
//     (host)          the counts copied down; chunks cut at pair boundaries: candidates <= budget, records <= record budget.  A read
//                     (pair) whose candidates alone pass the budget declines the call (HGX_ALNL_DECLINE_BUDGET)
//   per chunk -- count, scan, fill; no atomic decides a position, nothing passes between workgroups of these kernels
//     (scan)          the chunk's seed counts -> every seed's first candidate
//     k_alnl_verify   a lane per candidate: its seed by bisection of the scanned counts, the bucket entry, XOR + popcount over the bit
//                     planes (the HOT kernel), the earlier seeds' exact-match test; flag 0 / 1 and the 64-bit key
//     (scan)          the flags -> every hit's place
//     k_alnl_fill     a lane per candidate: the hits' keys, compacted
//     (hipcub)        one radix sort of the keys (read | NM | allele | pos0 | strand): read order, and the rule's order within a read
//     k_alnl_bounds   a lane per hit: where its read's hits begin and end (each word has one writer)
//     k_alnl_emit     a lane per hit, twice: the record's size (0 from rank k on), (scan,) the record at its offset
// Loop bounds: the read length (<= 256), the seeds per read (<= 5), the plane words (<= 4), log2 of the seed table's keys and of the
// chunk's seeds for the two bisections.  Every index is below a count the host sized the buffer with: a candidate below the scanned
// total, a hit below the flags' total, a record's bytes = the size the same code counted.
#include <hipcub/hipcub.hpp>

#include "hgx_common.hpp"
#include "hgx_align_linear.hpp"
#include "hgx_reads.hpp"

namespace {
typedef hgx_alnl_planes<HGX_ALNL_DEV_WORDS> DevPlanes;
typedef hgx_dev_reads DevReads;
constexpr long SPAN_READS = 65536;                 // reads whose seeds are counted at once (even: mates stay together; < 2^HGX_ALNL_READ_BITS)
constexpr long CAND_BUDGET = 1L << 24;             // candidates of one chunk: 16 B each in flag / key / place, 16 B per hit in the sort
constexpr long REC_BUDGET = 1L << 20;              // records of one chunk: with HGX_ALNL_LINE_MAX their text stays below 2^32 bytes
static_assert(SPAN_READS <= (1L << HGX_ALNL_READ_BITS), "a chunk's reads fit the key");
static_assert((unsigned long long)REC_BUDGET * HGX_ALNL_LINE_MAX < (1ull << 32), "a chunk's text fits 32-bit offsets");

// slots per strand and per read: a read has 2 * (max_edits + 1) seeds at most; per read a multiple of 4, so that every chunk's counts
// start at a multiple of 16 bytes (the scan loads them four at a time)
__host__ __device__ inline int slots_per_strand(int max_edits) { return (max_edits + 2) & ~1; }

__global__ void __launch_bounds__(256)
k_alnl_pack(DevReads rd, long first, long n, DevPlanes *planes) {
    const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= 2 * n) return;
    const long i = first + (gid >> 1);
    const hgx_aln_read R{rd.text + rd.seq_off[i], rd.len[i], (int)(gid & 1)};
    DevPlanes p;
    hgx_alnl_pack(R, p);
    planes[gid] = p;
}

__global__ void __launch_bounds__(256)
k_alnl_count(hgx_alnl_view V, DevReads rd, long first, long n, int max_edits, int sps, const DevPlanes *planes, uint32_t *cnt, uint32_t *begin) {
    const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= 2 * n * sps) return;
    const int j = (int)(gid % sps);
    const long rs = gid / sps;                     // (read, strand)
    uint32_t b0 = 0, b1 = 0, code;
    if (j < hgx_alnl_n_seeds(rd.len[first + (rs >> 1)], max_edits)) {
        const DevPlanes &p = planes[rs];
        if (hgx_alnl_code(p.lo, p.hi, p.mask, (long)j * HGX_ALNL_K, &code)) hgx_alnl_bucket(V, code, &b0, &b1);
    }
    cnt[gid] = b1 - b0;
    begin[gid] = b0;
}

// the candidates [0, n_cand) of the chunk's seeds [0, n_slots): coff = the scanned counts, begin = the buckets' first entries
__global__ void __launch_bounds__(256)
k_alnl_verify(hgx_alnl_view V, DevReads rd, long first, int sps, int max_edits, const DevPlanes *planes, const uint32_t *coff, const uint32_t *begin,
              uint32_t n_slots, uint32_t n_cand, uint32_t *flag, unsigned long long *key) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_cand) return;
    uint32_t lo = 0, hi = n_slots;                 // the first seed whose candidates start behind c; the one in front of it holds c
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (coff[mid] <= c) lo = mid + 1;
        else hi = mid;
    }
    const uint32_t s = lo - 1, e = begin[s] + (c - coff[s]);
    const uint32_t rs = s / (uint32_t)sps, i = rs >> 1;
    const int j = (int)(s % (uint32_t)sps), strand = (int)(rs & 1);
    const DevPlanes &rp = planes[rs];                 // (read through the pointer: a copy would sit in the lane's private memory)
    const int32_t a = V.kal[e];
    int32_t pos0 = 0;
    int nm = 0;
    const bool hit = hgx_alnl_candidate(V, rp, rd.len[first + i], j, a, V.kpos[e], max_edits, &pos0, &nm);
    flag[c] = hit ? 1u : 0u;
    key[c] = hit ? hgx_alnl_key(i, nm, a, pos0, strand) : 0ull;
}

__global__ void __launch_bounds__(256)
k_alnl_fill(uint32_t n_cand, const uint32_t *flag, const uint32_t *dst, const unsigned long long *key, unsigned long long *hits) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < n_cand && flag[c]) hits[dst[c]] = key[c];
}

// hits sorted: those of read r stand at [lo[r], hi[r]); both zeroed beforehand, so a read without a hit has none
__global__ void __launch_bounds__(256)
k_alnl_bounds(uint32_t n_hits, const unsigned long long *hits, uint32_t *lo, uint32_t *hi) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_hits) return;
    const uint32_t r = hgx_alnl_key_read(hits[j]);
    if (j == 0 || hgx_alnl_key_read(hits[j - 1]) != r) lo[r] = j;
    if (j + 1 == n_hits || hgx_alnl_key_read(hits[j + 1]) != r) hi[r] = j + 1;
}

// out == nullptr: sizes[j] = the bytes of hit j's record (0 from rank k on; a record past HGX_ALNL_LINE_MAX raises *decline);
// else the record at out + off[j]
__global__ void __launch_bounds__(64)
k_alnl_emit(hgx_alnl_view V, DevReads rd, long first, int k, uint32_t n_hits, const unsigned long long *hits, const uint32_t *lo, const uint32_t *hi,
            uint32_t *sizes, const uint32_t *off, char *out, int *decline) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_hits) return;
    const unsigned long long key = hits[j];
    const uint32_t r = hgx_alnl_key_read(key);
    const int rank = (int)(j - lo[r]), nh = (int)(hi[r] - lo[r]);
    if (rank >= k) {
        if (!out) sizes[j] = 0;
        return;
    }
    const long i = first + r;
    const bool mate_wrote = rd.paired && hi[r ^ 1u] > lo[r ^ 1u];
    hgx_aln_out o{out ? out + off[j] : nullptr, 0};
    hgx_alnl_line(V, rd.text + rd.name_off[i], rd.name_len[i], rd.text + rd.seq_off[i], rd.qual_off[i] < 0 ? nullptr : rd.text + rd.qual_off[i],
                  rd.len[i], key, rank, nh < k ? nh : k, nh, rd.paired ? (int)(r & 1) : -1, mate_wrote, o);
    if (!out) {
        sizes[j] = o.n > HGX_ALNL_LINE_MAX ? 0u : (uint32_t)o.n;
        if (o.n > HGX_ALNL_LINE_MAX) *decline = HGX_ALNL_DECLINE_LINE;       // (every writer stores the same word)
    }
}

template <class T> size_t put(std::vector<char> &blk, const std::vector<T> &v) {
    const size_t off = (blk.size() + 15) & ~(size_t)15;
    blk.resize(off + std::max<size_t>(v.size() * sizeof(T), 16));
    if (!v.empty()) memcpy(blk.data() + off, v.data(), v.size() * sizeof(T));
    return off;
}

// the index in HBM, made once per index and device: text, planes and seed table in one block
int ensure_device_index(hgx_align_linear_index *ix) {
    std::lock_guard<std::mutex> g(ix->mu);
    int dev = 0;
    HIPCHK(hipGetDevice(&dev));
    if (ix->dev_ready == dev) return HGX_OK;
    if (ix->d_block) { (void)hipFree(ix->d_block); ix->d_block = nullptr; ix->dev_ready = -1; }
    std::vector<char> blk;
    const size_t o_tx = put(blk, ix->text), o_of = put(blk, ix->off), o_lo = put(blk, ix->lo), o_hi = put(blk, ix->hi), o_mk = put(blk, ix->mask),
                 o_ky = put(blk, ix->keys), o_ko = put(blk, ix->koff), o_ka = put(blk, ix->kal), o_kp = put(blk, ix->kpos),
                 o_no = put(blk, ix->name_off), o_nl = put(blk, ix->name_len), o_pl = put(blk, ix->pool);
    HIPCHK(hipMalloc(&ix->d_block, blk.size()));
    HIPCHK(hipMemcpy(ix->d_block, blk.data(), blk.size(), hipMemcpyHostToDevice));
    const char *b = (const char *)ix->d_block;
    hgx_alnl_view &V = ix->dv;
    V = ix->hv;
    V.text = b + o_tx; V.off = (const int32_t *)(b + o_of);
    V.lo = (const uint64_t *)(b + o_lo); V.hi = (const uint64_t *)(b + o_hi); V.mask = (const uint64_t *)(b + o_mk);
    V.keys = (const uint32_t *)(b + o_ky); V.koff = (const uint32_t *)(b + o_ko);
    V.kal = (const int32_t *)(b + o_ka); V.kpos = (const int32_t *)(b + o_kp);
    V.name_off = (const int32_t *)(b + o_no); V.name_len = (const int32_t *)(b + o_nl); V.pool = b + o_pl;
    ix->dev_ready = dev;
    return HGX_OK;
}

// the budgets of this call: the constants above, or what the test switch align_linear_budget=C[,R[,N]] says (candidates and records
// of a chunk, reads of a span): small values put a chunk cut between any two reads of a test
void budgets_of(long *cand, long *rec, long *span) {
    *cand = CAND_BUDGET; *rec = REC_BUDGET; *span = SPAN_READS;
    const char *sw = hgx_test_switch("align_linear_budget");
    if (!sw) return;
    long v[3] = {0, 0, 0};
    int n = 0;
    for (const char *p = sw; n < 3; ++n) {
        v[n] = atol(p);
        p = strchr(p, ',');
        if (!p) { ++n; break; }
        ++p;
    }
    if (n > 0 && v[0] > 0) *cand = std::min(v[0], CAND_BUDGET);
    if (n > 1 && v[1] > 0) *rec = std::min(v[1], REC_BUDGET);
    if (n > 2 && v[2] > 0) *span = std::min(std::max(2L, v[2] & ~1L), SPAN_READS);
}

// a pool block that only grows: the chunks of one call reuse it (a chunk ends synchronised, so none is in use when it is replaced)
struct GrowBuf {
    DevBuf b;
    size_t cap = 0;
    int need(size_t bytes) {
        if (bytes <= cap) return 0;
        if (b.p) { hgx_pool_free(b.p); b.p = nullptr; cap = 0; }
        if (b.alloc(bytes + bytes / 4)) return -1;
        cap = bytes + bytes / 4;
        return 0;
    }
    template <class T> T *as() { return (T *)b.p; }
};
#define NEED(buf, bytes)                                               \
    do {                                                               \
        if ((buf).need(bytes)) {                                       \
            hgx_set_error("device allocation of %zu bytes failed", (size_t)(bytes));   \
            return HGX_ENOMEM;                                         \
        }                                                              \
    } while (0)

int chunks(hgx_align_linear_index *ix, const DevReads &rd, long n, int max_edits, int k, std::string &body, hgx_alnl_counts *counts, int *decline) {
    const size_t body0 = body.size();
    const hgx_alnl_counts counts0 = *counts;
    auto declined = [&](int dec) {                // what earlier chunks appended is taken back
        body.resize(body0);
        *counts = counts0;
        *decline = dec;
        return HGX_OK;
    };
    long cand_budget, rec_budget, span_reads;
    budgets_of(&cand_budget, &rec_budget, &span_reads);
    hipStream_t st = nullptr;
    const int sps = slots_per_strand(max_edits), spr = 2 * sps, step = rd.paired ? 2 : 1;
    const long smax = std::min(n, span_reads);
    DevBuf d_planes, d_cnt, d_begin, d_coff, d_misc, d_lo, d_hi;
    GrowBuf d_flag, d_key, d_dst, d_hits, d_sorted, d_tmp, d_sizes, d_off, d_out, d_scan;      // the chunks': sized by the largest so far
    Drain drain{st};                              // (whatever way this returns, the stream has run dry before the buffers above go back)
    ALLOC(d_planes, (size_t)smax * 2 * sizeof(DevPlanes));
    ALLOC(d_cnt, (size_t)smax * spr * 4); ALLOC(d_begin, (size_t)smax * spr * 4); ALLOC(d_coff, (size_t)smax * spr * 4);
    ALLOC(d_lo, (size_t)smax * 4); ALLOC(d_hi, (size_t)smax * 4);
    ALLOC(d_misc, 16);                            // [0] a scan's total, [1] the decline word
    std::vector<uint32_t> h_cnt((size_t)smax * spr), h_lo(smax), h_hi(smax);
    for (long s0 = 0; s0 < n; s0 += span_reads) {
        const long ns = std::min(span_reads, n - s0);
        k_alnl_pack<<<nblk(2 * ns, 256), 256, 0, st>>>(rd, s0, ns, d_planes.as<DevPlanes>());
        k_alnl_count<<<nblk(ns * spr, 256), 256, 0, st>>>(ix->dv, rd, s0, ns, max_edits, sps, d_planes.as<DevPlanes>(), d_cnt.as<uint32_t>(),
                                                          d_begin.as<uint32_t>());
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(h_cnt.data(), d_cnt.p, (size_t)ns * spr * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        for (long c0 = 0; c0 < ns;) {
            // the chunk [c0, c1): whole reads (pairs) while candidates and records stay within the budgets
            long c1 = c0, cand = 0, rec = 0;
            while (c1 < ns) {
                long ucand = 0, urec = 0;
                for (long i = c1; i < std::min(c1 + step, ns); ++i) {
                    long rc_ = 0;
                    for (int s = 0; s < spr; ++s) rc_ += h_cnt[(size_t)i * spr + s];
                    ucand += rc_;
                    urec += std::min<long>(rc_, k);
                }
                if (ucand > cand_budget || urec > rec_budget) return declined(HGX_ALNL_DECLINE_BUDGET);
                if (c1 > c0 && (cand + ucand > cand_budget || rec + urec > rec_budget)) break;
                cand += ucand; rec += urec; c1 = std::min(c1 + step, ns);
            }
            const long first = s0 + c0, nc = c1 - c0;
            const uint32_t n_slots = (uint32_t)(nc * spr), n_cand = (uint32_t)cand;
            counts->candidates += cand;
            c0 = c1;
            if (!n_cand) continue;
            const DevPlanes *planes = d_planes.as<DevPlanes>() + (first - s0) * 2;
            const uint32_t *cnt = d_cnt.as<uint32_t>() + (first - s0) * spr, *begin = d_begin.as<uint32_t>() + (first - s0) * spr;
            NEED(d_scan, hgx_scan_u32_scratch_bytes(std::max<long>(n_cand, n_slots)) + 16);      // (hits <= candidates: it serves all three scans)
            NEED(d_flag, (size_t)n_cand * 4); NEED(d_dst, (size_t)n_cand * 4); NEED(d_key, (size_t)n_cand * 8);
            TRY(hgx_scan_u32_dev(cnt, d_coff.as<uint32_t>(), n_slots, d_scan.b.p, d_misc.as<uint32_t>(), st));
            k_alnl_verify<<<nblk(n_cand, 256), 256, 0, st>>>(ix->dv, rd, first, sps, max_edits, planes, d_coff.as<uint32_t>(), begin, n_slots, n_cand,
                                                             d_flag.as<uint32_t>(), d_key.as<unsigned long long>());
            HIPCHK(hipGetLastError());
            TRY(hgx_scan_u32_dev(d_flag.as<uint32_t>(), d_dst.as<uint32_t>(), n_cand, d_scan.b.p, d_misc.as<uint32_t>(), st));
            uint32_t n_hits = 0;
            HIPCHK(hipMemcpyAsync(&n_hits, d_misc.p, 4, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            if (n_hits > n_cand) { hgx_set_error("hgx_align_linear_reads: %u hits of %u candidates", n_hits, n_cand); return HGX_EHIP; }
            if (!n_hits) continue;
            NEED(d_hits, (size_t)n_hits * 8); NEED(d_sorted, (size_t)n_hits * 8);
            k_alnl_fill<<<nblk(n_cand, 256), 256, 0, st>>>(n_cand, d_flag.as<uint32_t>(), d_dst.as<uint32_t>(), d_key.as<unsigned long long>(),
                                                           d_hits.as<unsigned long long>());
            HIPCHK(hipGetLastError());
            int end_bit = 64 - HGX_ALNL_READ_BITS;                          // the key's bits below the read field, and the chunk's reads above them
            while (end_bit < 64 && ((nc - 1) >> (end_bit - (64 - HGX_ALNL_READ_BITS)))) ++end_bit;
            size_t tmp_bytes = 0;
            (void)hipcub::DeviceRadixSort::SortKeys((void *)nullptr, tmp_bytes, (unsigned long long *)nullptr, (unsigned long long *)nullptr, (int)n_hits,
                                                    0, end_bit, st);
            NEED(d_tmp, std::max<size_t>(tmp_bytes, 256));
            HIPCHK(hipcub::DeviceRadixSort::SortKeys(d_tmp.b.p, tmp_bytes, d_hits.as<unsigned long long>(), d_sorted.as<unsigned long long>(), (int)n_hits,
                                                     0, end_bit, st));
            HIPCHK(hipMemsetAsync(d_lo.p, 0, (size_t)nc * 4, st));
            HIPCHK(hipMemsetAsync(d_hi.p, 0, (size_t)nc * 4, st));
            HIPCHK(hipMemsetAsync(d_misc.p, 0, 16, st));
            k_alnl_bounds<<<nblk(n_hits, 256), 256, 0, st>>>(n_hits, d_sorted.as<unsigned long long>(), d_lo.as<uint32_t>(), d_hi.as<uint32_t>());
            HIPCHK(hipGetLastError());
            NEED(d_sizes, (size_t)n_hits * 4); NEED(d_off, (size_t)n_hits * 4);
            k_alnl_emit<<<nblk(n_hits, 64), 64, 0, st>>>(ix->dv, rd, first, k, n_hits, d_sorted.as<unsigned long long>(), d_lo.as<uint32_t>(),
                                                         d_hi.as<uint32_t>(), d_sizes.as<uint32_t>(), nullptr, nullptr, d_misc.as<int>() + 1);
            HIPCHK(hipGetLastError());
            TRY(hgx_scan_u32_dev(d_sizes.as<uint32_t>(), d_off.as<uint32_t>(), n_hits, d_scan.b.p, d_misc.as<uint32_t>(), st));
            uint32_t back[2] = {0, 0};                // the text's bytes, the decline word
            HIPCHK(hipMemcpyAsync(back, d_misc.p, 8, hipMemcpyDeviceToHost, st));
            HIPCHK(hipMemcpyAsync(h_lo.data(), d_lo.p, (size_t)nc * 4, hipMemcpyDeviceToHost, st));
            HIPCHK(hipMemcpyAsync(h_hi.data(), d_hi.p, (size_t)nc * 4, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            if (back[1]) return declined((int)back[1]);
            for (long i = 0; i < nc; ++i) {
                const long nh = (long)h_hi[i] - (long)h_lo[i];
                counts->aligned += nh > 0;
                counts->records += std::min<long>(nh, k);
            }
            const uint32_t total = back[0];
            if (!total) continue;
            NEED(d_out, (size_t)total);
            k_alnl_emit<<<nblk(n_hits, 64), 64, 0, st>>>(ix->dv, rd, first, k, n_hits, d_sorted.as<unsigned long long>(), d_lo.as<uint32_t>(),
                                                         d_hi.as<uint32_t>(), nullptr, d_off.as<uint32_t>(), d_out.as<char>(), nullptr);
            HIPCHK(hipGetLastError());
            const size_t at = body.size();
            body.resize(at + total);
            HIPCHK(hipMemcpyAsync(&body[at], d_out.b.p, total, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
        }
    }
    return HGX_OK;
}
}      // namespace

void hgx_alnl_device_free(hgx_align_linear_index *ix) {
    if (ix->d_block) (void)hipFree(ix->d_block);
    ix->d_block = nullptr;
    ix->dev_ready = -1;
}

// the upload half: the loader's table and text copied up, then the chunks over them
int hgx_alnl_device(hgx_align_linear_index *ix, const hgx_aln_reads &reads, int max_edits, int k, std::string &body, hgx_alnl_counts *counts,
                    int *decline) {
    *decline = 0;
    const long n = (long)reads.n();
    int max_len = 0;
    for (long i = 0; i < n; ++i) max_len = std::max(max_len, (int)reads.len[i]);
    if (max_len > HGX_ALNL_DEV_MAX_READ) { *decline = HGX_ALNL_DECLINE_READ_LEN; return HGX_OK; }
    TRY(ensure_device_index(ix));
    DevBuf d_text, d_no, d_so, d_qo, d_nl, d_len;
    ALLOC(d_text, reads.text.size() + 16);
    ALLOC(d_no, n * 8); ALLOC(d_so, n * 8); ALLOC(d_qo, n * 8); ALLOC(d_nl, n * 4); ALLOC(d_len, n * 4);
    HIPCHK(hipMemcpy(d_text.p, reads.text.data(), reads.text.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_no.p, reads.name_off.data(), n * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_so.p, reads.seq_off.data(), n * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_qo.p, reads.qual_off.data(), n * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_nl.p, reads.name_len.data(), n * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_len.p, reads.len.data(), n * 4, hipMemcpyHostToDevice));
    const DevReads rd{d_text.as<char>(), d_no.as<int64_t>(), d_so.as<int64_t>(), d_qo.as<int64_t>(), d_nl.as<int32_t>(), d_len.as<int32_t>(),
                      reads.paired};
    return chunks(ix, rd, n, max_edits, k, body, counts, decline);
}

// the body: the chunks of a read table that lies in HBM
int hgx_alnl_device_body(hgx_align_linear_index *ix, const hgx_dev_reads &rd, long n, int max_len, int max_edits, int k, std::string &body,
                         hgx_alnl_counts *counts, int *decline) {
    *decline = 0;
    if (max_len > HGX_ALNL_DEV_MAX_READ) { *decline = HGX_ALNL_DECLINE_READ_LEN; return HGX_OK; }
    TRY(ensure_device_index(ix));
    return chunks(ix, rd, n, max_edits, k, body, counts, decline);
}

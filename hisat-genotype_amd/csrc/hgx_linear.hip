// hgx_linear.hip -- linear-index typing on the device (typing_core.py:1597-1649; include/hgx.h "linear-index typing").
//
// The reference reads `samtools view <file> [region]` in file order; a class is the set of alleles a read aligned to with its
// best AS so far (HISAT2 / Bowtie2 against an index of allele sequences, -k 10: common:1003-1016).  Kernels, in order:
//   k_lin_records   one thread per line: columns as str.split() cuts them, FLAG, RNAME -> allele id (name_lookup of
//                   hgx_records.hpp: device hash of the locus' names, exact byte compare), the filters of core:1618-1623, AS
//                   (last cols[11:] column starting "AS"), the read-id hash; anything the host route has to word (unknown
//                   in-gene name, no integer AS, a short line) declines
//   scan + k_lin_compact     the kept records, in order (k_scan_u32)
//   k_rec_heads     a record opens a group where its read id differs from the previous kept record's (hash, then bytes)
//   scan + k_rec_gstart      group extents (both kernels shared with the extract route: hgx_records.hpp)
//   k_lin_groups    one thread per group: the segmented exclusive prefix max of AS (accept flags), the accepted ids in name
//                   order without repeats, the bowtie2 size rule, the class key, and Gene_counts of the group's trigger (the
//                   NEXT group's first kept RNAME, core:1600-1604) with its first-seen group for the dict order
//   k_lin_insert / k_lin_verify   class dedup: open addressing on the 64-bit key, first group wins (atomicMin = first seen),
//                   an exact compare of every group with its class's first group (a mismatch = a key collision: host route)
//   scan + k_lin_class + scan + k_lin_gather   class ids in first-seen order, counts, and the name ids of DISTINCT classes only
// Bytes: the text once by k_lin_records (plus 16 B of line table per line); the compacted stream (~40 B per kept record) a few
// times; per group ~32 B.
#include <algorithm>
#include <memory>
#include <vector>

#include "hgx_common.hpp"
#include "hgx_internal.hpp"
#include "hgx_linear.hpp"
#include "hgx_records.hpp"

__device__ static inline bool lin_sp(char c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r' || c == '\v' || c == '\f'; }

__device__ static inline bool lin_int(const char *p, long n, int64_t &v) {
    long i = 0;
    bool neg = false;
    if (i < n && (p[i] == '+' || p[i] == '-')) neg = p[i++] == '-';
    if (i >= n) return false;
    int64_t x = 0;
    for (; i < n; ++i) {
        if (p[i] < '0' || p[i] > '9') return false;
        x = x * 10 + (p[i] - '0');
        if (x > ((int64_t)1 << 40)) return false;
    }
    v = neg ? -x : x;
    return true;
}

__global__ void k_lin_records(const char *__restrict__ text, const uint64_t *__restrict__ ls, const uint64_t *__restrict__ le, long N,
                              const char *__restrict__ gene, int gene_len, const hgx_name_view names, uint32_t *__restrict__ keep,
                              int32_t *__restrict__ aid, int32_t *__restrict__ as_out, uint64_t *__restrict__ qh,
                              uint64_t *__restrict__ qoff, uint32_t *__restrict__ qlen, uint32_t *__restrict__ decline) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    keep[i] = 0;
    const uint64_t e = le[i];
    uint64_t pos = ls[i];
    int col = 0;
    uint64_t q0 = 0, r0 = 0, f0 = 0, a0 = 0;
    uint32_t qn = 0, rn = 0, fn = 0, an = 0;
    while (pos < e) {
        while (pos < e && lin_sp(text[pos])) ++pos;
        if (pos >= e) break;
        const uint64_t b = pos;
        while (pos < e && !lin_sp(text[pos])) ++pos;
        const uint32_t n = (uint32_t)(pos - b);
        if (col == 0) { q0 = b; qn = n; }
        else if (col == 1) { f0 = b; fn = n; }
        else if (col == 2) { r0 = b; rn = n; }
        else if (col >= 11 && n >= 2 && text[b] == 'A' && text[b + 1] == 'S') { a0 = b; an = n; }
        ++col;
    }
    int64_t flag;
    if (col < 3 || !lin_int(text + f0, fn, flag)) { atomicOr(decline, 1u << HGX_LIN_DECLINE_RECORD); return; }
    if (flag & 0x4) return;
    const char *r = text + r0;
    if ((int)rn < gene_len) return;
    for (int k = 0; k < gene_len; ++k)
        if (r[k] != gene[k]) return;
    for (uint32_t k = 0; k + 8 <= rn; ++k) {
        if (r[k] == 'B' && r[k + 1] == 'A' && r[k + 2] == 'C' && r[k + 3] == 'K' && r[k + 4] == 'B' && r[k + 5] == 'O' &&
            r[k + 6] == 'N' && r[k + 7] == 'E')
            return;
    }
    int64_t asv;
    if (an == 0 || !lin_int(text + a0 + min(an, 5u), (long)an - (long)min(an, 5u), asv) || asv > INT32_MAX || asv < INT32_MIN) {
        atomicOr(decline, 1u << HGX_LIN_DECLINE_AS);
        return;
    }
    const int32_t id = name_lookup(names, r, rn);
    if (id < 0) { atomicOr(decline, 1u << HGX_LIN_DECLINE_UNKNOWN_NAME); return; }
    keep[i] = 1;
    aid[i] = id;
    as_out[i] = (int32_t)asv;
    qh[i] = fnv1a(text + q0, qn);
    qoff[i] = q0;
    qlen[i] = qn;
}

// The same for BAM records (SAM/BAM specification 4.2): rs[i] = offset of refID, rl[i] = block_size.  RNAME through the per-refID
// table (tab[n_ref] = "*"), FLAG, QNAME, and AS from the aux data as samtools view prints it: the last tag named AS; an integer
// type (cCsSiI) gives the value, any other type (f, Z, A, H, B) or no AS declines to the host route, which words int()'s error or
// the assertion.  A tag whose printed text would hold whitespace (Z / H with a blank, A = ' ') would shift the columns the
// reference splits on: the record declines too, as does a record whose aux data do not fit its block.
__device__ static inline uint32_t lin_u32(const char *p) {
    const unsigned char *q = (const unsigned char *)p;
    return (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) | ((uint32_t)q[3] << 24);
}

__global__ void k_lin_bam_records(const char *__restrict__ raw, const uint64_t *__restrict__ rs, const uint64_t *__restrict__ rl, long N,
                                  const int32_t *__restrict__ tab, int32_t n_ref, uint32_t *__restrict__ keep, int32_t *__restrict__ aid,
                                  int32_t *__restrict__ as_out, uint64_t *__restrict__ qh, uint64_t *__restrict__ qoff,
                                  uint32_t *__restrict__ qlen, uint32_t *__restrict__ decline) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    keep[i] = 0;
    const char *r = raw + rs[i];
    const uint64_t bs = rl[i];
    if (bs < 32) { atomicOr(decline, 1u << HGX_LIN_DECLINE_RECORD); return; }
    const int32_t ref = (int32_t)lin_u32(r);
    const uint32_t l_rn = (uint8_t)r[8];
    const uint32_t n_cig = (uint8_t)r[12] | ((uint32_t)(uint8_t)r[13] << 8);
    const uint32_t flag = (uint8_t)r[14] | ((uint32_t)(uint8_t)r[15] << 8);
    const uint32_t l_seq = lin_u32(r + 16);
    if (flag & 0x4) return;
    const int32_t id = tab[(ref >= 0 && ref < n_ref) ? ref : n_ref];
    if (id == -1) return;
    if (id < 0) { atomicOr(decline, 1u << HGX_LIN_DECLINE_UNKNOWN_NAME); return; }
    uint64_t p = 32 + (uint64_t)l_rn + 4ull * n_cig + ((uint64_t)l_seq + 1) / 2 + (uint64_t)l_seq;
    if (l_rn == 0 || p > bs) { atomicOr(decline, 1u << HGX_LIN_DECLINE_RECORD); return; }
    int as_state = 0;                                        // 0 none, 1 integer, 2 other type
    int64_t asv = 0;
    bool bad = false;
    while (p < bs && !bad) {
        if (p + 3 > bs) { bad = true; break; }
        const char t0 = r[p], t1 = r[p + 1], ty = r[p + 2];
        p += 3;
        int64_t v = 0;
        bool integer = true;
        switch (ty) {
            case 'c': if (p + 1 > bs) { bad = true; break; } v = (int8_t)r[p]; p += 1; break;
            case 'C': if (p + 1 > bs) { bad = true; break; } v = (uint8_t)r[p]; p += 1; break;
            case 's': if (p + 2 > bs) { bad = true; break; } v = (int16_t)((uint8_t)r[p] | ((uint16_t)(uint8_t)r[p + 1] << 8)); p += 2; break;
            case 'S': if (p + 2 > bs) { bad = true; break; } v = (uint16_t)((uint8_t)r[p] | ((uint16_t)(uint8_t)r[p + 1] << 8)); p += 2; break;
            case 'i': if (p + 4 > bs) { bad = true; break; } v = (int32_t)lin_u32(r + p); p += 4; break;
            case 'I': if (p + 4 > bs) { bad = true; break; } v = (int64_t)lin_u32(r + p); p += 4; break;
            case 'A': if (p + 1 > bs) { bad = true; break; } integer = false; if (lin_sp(r[p])) bad = true; p += 1; break;
            case 'f': if (p + 4 > bs) { bad = true; break; } integer = false; p += 4; break;
            case 'Z': case 'H': {
                integer = false;
                while (p < bs && r[p] != 0) { if (lin_sp(r[p])) bad = true; ++p; }
                if (p >= bs) bad = true;
                ++p;
                break;
            }
            case 'B': {
                integer = false;
                if (p + 5 > bs) { bad = true; break; }
                const char sub = r[p];
                const uint64_t cnt = lin_u32(r + p + 1);
                const uint64_t w = (sub == 'c' || sub == 'C') ? 1 : (sub == 's' || sub == 'S') ? 2 : (sub == 'i' || sub == 'I' || sub == 'f') ? 4 : 0;
                if (!w) { bad = true; break; }
                p += 5 + w * cnt;
                if (p > bs) bad = true;
                break;
            }
            default: bad = true;
        }
        if (!bad && t0 == 'A' && t1 == 'S') { as_state = integer ? 1 : 2; asv = v; }
    }
    if (bad) { atomicOr(decline, 1u << HGX_LIN_DECLINE_RECORD); return; }
    // (a type-I value above INT32_MAX is no int32 AS: declined, as the text kernel declines the same printed number)
    if (as_state != 1 || asv > INT32_MAX) { atomicOr(decline, 1u << HGX_LIN_DECLINE_AS); return; }
    keep[i] = 1;
    aid[i] = id;
    as_out[i] = (int32_t)asv;
    qh[i] = fnv1a(r + 32, l_rn - 1);
    qoff[i] = rs[i] + 32;
    qlen[i] = l_rn - 1;
}

__global__ void k_lin_compact(const uint32_t *__restrict__ keep, const uint32_t *__restrict__ pos, long N,
                              const int32_t *__restrict__ aid, const int32_t *__restrict__ as_in, const uint64_t *__restrict__ qh,
                              const uint64_t *__restrict__ qoff, const uint32_t *__restrict__ qlen,
                              int32_t *__restrict__ c_aid, int32_t *__restrict__ c_as, uint64_t *__restrict__ c_qh,
                              uint64_t *__restrict__ c_qoff, uint32_t *__restrict__ c_qlen) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N || !keep[i]) return;
    const uint32_t j = pos[i];
    c_aid[j] = aid[i];
    c_as[j] = as_in[i];
    c_qh[j] = qh[i];
    c_qoff[j] = qoff[i];
    c_qlen[j] = qlen[i];
}

__global__ void k_lin_groups(const uint32_t *__restrict__ gstart, long G, const int32_t *__restrict__ aid, const int32_t *__restrict__ as_in,
                             const int32_t *__restrict__ rank, int aligner, int32_t last_trigger, int collide,
                             int32_t *__restrict__ acc, uint32_t *__restrict__ glen, uint64_t *__restrict__ ghash,
                             uint32_t *__restrict__ counted, unsigned long long *__restrict__ cnt, uint32_t *__restrict__ firstg) {
    const long g = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G) return;
    const uint32_t s = gstart[g], e = gstart[g + 1];
    // accept flags (AS >= the max AS of the group's records before it; the first record always joins), and each accepted id
    // straight into a name-ordered list without repeats (the class key is '-'.join(sorted(set))): binary search, then insert --
    // repeats of an id cost a search, not a place in the list
    int32_t mx = as_in[s];
    uint32_t nd = 0;
    for (uint32_t j = s; j < e; ++j) {
        const int32_t a = as_in[j];
        if (j != s && a < mx) continue;
        mx = max(mx, a);
        const int32_t v = aid[j], rv = rank[v];
        uint32_t lo = 0, hi = nd;
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (rank[acc[s + mid]] < rv) lo = mid + 1; else hi = mid;
        }
        if (lo < nd && acc[s + lo] == v) continue;
        for (uint32_t y = nd; y > lo; --y) acc[s + y] = acc[s + y - 1];
        acc[s + lo] = v;
        ++nd;
    }
    const bool last = g == G - 1;
    const bool c = aligner == 0 || (aligner == 1 && nd < 10) || last;
    uint64_t h = 1469598103934665603ull ^ nd;
    for (uint32_t x = 0; x < nd; ++x) h = (h ^ (uint32_t)acc[s + x]) * 1099511628211ull;
    if (collide) h &= 7ull;                     // test switch linear_collide: every class on a handful of keys
    if (h == HGX_EMPTY_KEY) h = 0;
    glen[g] = nd;
    ghash[g] = h;
    counted[g] = c ? 1u : 0u;
    if (!c) return;
    const int32_t t = last ? last_trigger : aid[gstart[g + 1]];
    if (t >= 0) {
        atomicAdd(&cnt[t], 1ull);
        atomicMin(&firstg[t], (uint32_t)g);
    }
}

__global__ void k_lin_insert(const uint64_t *__restrict__ ghash, const uint32_t *__restrict__ counted, long G,
                             unsigned long long *__restrict__ tkey, uint32_t *__restrict__ tfirst, uint32_t tmask, uint32_t *__restrict__ gslot) {
    const long g = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G || !counted[g]) return;
    const unsigned long long h = ghash[g];
    for (uint32_t s = (uint32_t)(h ^ (h >> 32)) & tmask;; s = (s + 1) & tmask) {
        const unsigned long long prev = atomicCAS(&tkey[s], (unsigned long long)HGX_EMPTY_KEY, h);
        if (prev == HGX_EMPTY_KEY || prev == h) {
            atomicMin(&tfirst[s], (uint32_t)g);
            gslot[g] = s;
            return;
        }
    }
}

__global__ void k_lin_verify(const uint32_t *__restrict__ gstart, const int32_t *__restrict__ acc, const uint32_t *__restrict__ glen,
                             const uint32_t *__restrict__ counted, const uint32_t *__restrict__ gslot, const uint32_t *__restrict__ tfirst,
                             long G, uint32_t *__restrict__ first, uint32_t *__restrict__ decline) {
    const long g = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G) return;
    if (!counted[g]) { first[g] = 0; return; }
    const uint32_t rep = tfirst[gslot[g]];
    first[g] = rep == (uint32_t)g ? 1u : 0u;
    if (rep == (uint32_t)g) return;
    bool same = glen[rep] == glen[g];
    const int32_t *a = acc + gstart[g], *b = acc + gstart[rep];
    for (uint32_t x = 0; same && x < glen[g]; ++x) same = a[x] == b[x];
    if (!same) atomicOr(decline, 1u << HGX_LIN_DECLINE_COLLISION);
}

__global__ void k_lin_class(const uint32_t *__restrict__ counted, const uint32_t *__restrict__ first, const uint32_t *__restrict__ gslot,
                            const uint32_t *__restrict__ tfirst, const uint32_t *__restrict__ cid, const uint32_t *__restrict__ glen,
                            const uint32_t *__restrict__ gstart, long G, unsigned long long *__restrict__ ccount,
                            uint32_t *__restrict__ clen, uint32_t *__restrict__ csrc) {
    const long g = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G || !counted[g]) return;
    const uint32_t c = cid[tfirst[gslot[g]]];
    atomicAdd(&ccount[c], 1ull);
    if (first[g]) { clen[c] = glen[g]; csrc[c] = gstart[g]; }
}

__global__ void k_lin_gather(const uint32_t *__restrict__ clen, const uint32_t *__restrict__ csrc, const uint32_t *__restrict__ coff,
                             long C, const int32_t *__restrict__ acc, int32_t *__restrict__ out) {
    const long c = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    for (uint32_t x = 0; x < clen[c]; ++x) out[coff[c] + x] = acc[csrc[c] + x];
}

// the device copies of a locus' names, freed on the device that holds them
static void lin_free_names(hgx_linear_locus &ll) {
    free_on_device(ll.dev, {ll.d_names.pool, ll.d_names.off, ll.d_names.slot, ll.d_rank});
    ll.d_names = hgx_name_view();
    ll.d_rank = nullptr;
}

static int lin_upload_names(hgx_linear_locus &ll) {
    int dev = 0;
    HIPCHK(hipGetDevice(&dev));
    if (ll.d_names.slot && ll.dev == dev) return HGX_OK;
    lin_free_names(ll);
    ll.dev = dev;
    const bool ok = name_table_upload(ll.d_names, ll.name) && upload_array(ll.d_rank, ll.rank.data(), ll.rank.size() * 4);
    if (!ok) {
        const hipError_t e = hipGetLastError();
        lin_free_names(ll);
        hgx_set_error("linear route: upload of the locus' names failed: %s", hipGetErrorString(e));
        return HGX_EHIP;
    }
    return HGX_OK;
}

// The records one linear call reads: SAM text lines, or BAM records (offset of refID, block_size) in the inflated stream --
// in file order, region-filtered as samtools view does.  Opened once (hgx_linear_input_open) it serves every locus of a
// typing() call: read, inflated and walked once, uploaded on the first device use.
struct hgx_linear_input {
    hgx_align_lines al;                      // owns the host bytes of a file
    std::string path, regions;
    bool has_regions = false;
    const char *base = nullptr;              // host bytes the offsets point into
    size_t n_bytes = 0;
    bool binary = false;
    std::vector<std::string> refs;
    std::vector<uint64_t> ls, le;            // text: [start, end) of a line; BAM: record start (at refID), block_size
    void *d_raw = nullptr, *d_ls = nullptr, *d_le = nullptr;
    int dev = -1;
    long long last_up = 0;                  // bytes the last call uploaded (0: already resident)
    bool host_text = false;                  // BAM decoded to text for the host route (made on the first decline)
    std::vector<char> text;
    std::vector<uint64_t> t_ls, t_le;
    ~hgx_linear_input() { release_dev(); }
    void release_dev() {
        free_on_device(dev, {d_raw, d_ls, d_le});
        d_raw = d_ls = d_le = nullptr;
    }
};

static int lin_upload_input(hgx_linear_input &in, hipStream_t st) {
    int dev = 0;
    HIPCHK(hipGetDevice(&dev));
    in.last_up = 0;
    if (in.d_raw && in.dev == dev) return HGX_OK;
    in.release_dev();
    in.dev = dev;
    const size_t N = in.ls.size();
    bool ok = hipMalloc(&in.d_raw, std::max<size_t>(in.n_bytes, 1)) == hipSuccess && hipMalloc(&in.d_ls, std::max<size_t>(N, 1) * 8) == hipSuccess &&
              hipMalloc(&in.d_le, std::max<size_t>(N, 1) * 8) == hipSuccess;
    ok = ok && (!in.n_bytes || hipMemcpyAsync(in.d_raw, in.base, in.n_bytes, hipMemcpyHostToDevice, st) == hipSuccess) &&
         (!N || (hipMemcpyAsync(in.d_ls, in.ls.data(), N * 8, hipMemcpyHostToDevice, st) == hipSuccess &&
                 hipMemcpyAsync(in.d_le, in.le.data(), N * 8, hipMemcpyHostToDevice, st) == hipSuccess)) &&
         hipStreamSynchronize(st) == hipSuccess;
    if (!ok) {
        const hipError_t e = hipGetLastError();
        in.release_dev();
        hgx_set_error("linear route: upload of the records failed: %s", hipGetErrorString(e));
        return HGX_EHIP;
    }
    in.last_up = (long long)(in.n_bytes + 16 * N);
    return HGX_OK;
}

static inline uint32_t lin_rd32(const char *p) { uint32_t v; memcpy(&v, p, 4); return v; }

// RNAME of the last record the loop reads (the loop's last `allele`, core:1600-1604)
static std::string lin_last_rname(const hgx_linear_input &in) {
    const size_t N = in.ls.size();
    if (!N) return std::string();
    if (!in.binary) return hgx_linear_rname(in.base + in.ls[N - 1], in.le[N - 1] - in.ls[N - 1]);
    const int32_t ref = (int32_t)lin_rd32(in.base + in.ls[N - 1]);
    return ref >= 0 && ref < (int32_t)in.refs.size() ? in.refs[ref] : std::string("*");
}

// the device route; *declined != 0: nothing in `out` is to be used, the host route takes the records
static int lin_device(hgx_linear &out, hgx_linear_locus &ll, hgx_linear_input &in, const hgx_linear_opts &o, hipStream_t st, int *declined) {
    *declined = 0;
    RCHK(lin_upload_names(ll));
    const long N = (long)in.ls.size();
    const int A = (int)ll.name.size();
    const std::string gene = o.gene ? o.gene : "";
    out.extra.clear();
    out.count_id.clear(); out.count_val.clear();
    out.cls_off.assign(1, 0); out.cls_ids.clear(); out.cls_count.clear();      // no kept record: no class
    if (N == 0) return HGX_OK;
    RCHK(lin_upload_input(in, st));
    int32_t last_trigger = hgx_linear_name_id(out, ll, lin_last_rname(in));
    if (last_trigger >= A) last_trigger = -1;              // a name outside the locus: counted on the host below
    DevBufs m("linear route");
    char *d_gene;
    const char *d_text = (const char *)in.d_raw;
    uint64_t *d_qh, *d_qoff, *c_qh, *c_qoff, *d_ghash;
    uint32_t *d_keep, *d_pos, *d_qlen, *c_qlen, *d_dec, *d_tot;
    int32_t *d_aid, *d_as, *c_aid, *c_as;
    char *d_scan;
    RCHK(m.get(d_gene, gene.size() + 1));
    RCHK(m.get(d_keep, N)); RCHK(m.get(d_pos, N)); RCHK(m.get(d_aid, N)); RCHK(m.get(d_as, N));
    RCHK(m.get(d_qh, N)); RCHK(m.get(d_qoff, N)); RCHK(m.get(d_qlen, N));
    RCHK(m.get(d_dec, 1)); RCHK(m.get(d_tot, 4));
    RCHK(m.get(d_scan, hgx_scan_u32_scratch_bytes(N)));     // one scan scratch for the four scans (each is <= N long)
    if (!gene.empty()) HIPCHK(hipMemcpyAsync(d_gene, gene.data(), gene.size(), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(d_dec, 0, 4, st));
    if (in.binary) {
        // per refID: the allele id, filtered (-1: not the gene, or BACKBONE), or unknown in-gene name (-2); the last entry is "*"
        const size_t R = in.refs.size();
        std::vector<int32_t> tab(R + 1);
        for (size_t r = 0; r <= R; ++r) {
            const std::string &nm = r < R ? in.refs[r] : std::string("*");
            if (nm.compare(0, gene.size(), gene) != 0 || nm.size() < gene.size() || nm.find("BACKBONE") != std::string::npos) tab[r] = -1;
            else { auto it = ll.id.find(nm); tab[r] = it != ll.id.end() ? it->second : -2; }
        }
        int32_t *d_tab;
        RCHK(m.get(d_tab, R + 1));
        HIPCHK(hipMemcpyAsync(d_tab, tab.data(), (R + 1) * 4, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_lin_bam_records, dim3(nblk(N, 256)), dim3(256), 0, st, d_text, (const uint64_t *)in.d_ls, (const uint64_t *)in.d_le,
                           N, d_tab, (int32_t)R, d_keep, d_aid, d_as, d_qh, d_qoff, d_qlen, d_dec);
    } else {
        hipLaunchKernelGGL(k_lin_records, dim3(nblk(N, 256)), dim3(256), 0, st, d_text, (const uint64_t *)in.d_ls, (const uint64_t *)in.d_le,
                           N, d_gene, (int)gene.size(), ll.d_names, d_keep, d_aid, d_as, d_qh, d_qoff, d_qlen, d_dec);
    }
    HIPCHK(hipGetLastError());
    RCHK(hgx_scan_u32_dev(d_keep, d_pos, N, d_scan, d_tot, st));
    uint32_t h_dec = 0, M = 0;
    HIPCHK(hipMemcpyAsync(&h_dec, d_dec, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&M, d_tot, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (h_dec) { *declined = first_decline(h_dec); return HGX_OK; }
    out.n_kept = M;
    if (M == 0) return HGX_OK;
    RCHK(m.get(c_aid, M)); RCHK(m.get(c_as, M)); RCHK(m.get(c_qh, M)); RCHK(m.get(c_qoff, M)); RCHK(m.get(c_qlen, M));
    hipLaunchKernelGGL(k_lin_compact, dim3(nblk(N, 256)), dim3(256), 0, st, d_keep, d_pos, N, d_aid, d_as, d_qh, d_qoff, d_qlen,
                       c_aid, c_as, c_qh, c_qoff, c_qlen);
    HIPCHK(hipGetLastError());
    // group heads and extents (the N-sized scratch is reused: keep -> head, pos -> gid)
    uint32_t *d_head = d_keep, *d_gid = d_pos;
    hipLaunchKernelGGL(k_rec_heads<uint64_t>, dim3(nblk(M, 256)), dim3(256), 0, st, d_text, c_qh, c_qoff, c_qlen, (long)M, d_head);
    HIPCHK(hipGetLastError());
    RCHK(hgx_scan_u32_dev(d_head, d_gid, M, d_scan, d_tot + 1, st));
    uint32_t G = 0;
    HIPCHK(hipMemcpyAsync(&G, d_tot + 1, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    out.n_groups = G;
    uint32_t *d_gstart, *d_glen, *d_counted, *d_firstg, *d_gslot, *d_first, *d_cid, *d_tfirst;
    int32_t *d_acc;
    unsigned long long *d_cnt, *d_tkey;
    uint32_t ts = 16;
    while (ts < 2 * G + 16) ts <<= 1;
    RCHK(m.get(d_gstart, (size_t)G + 1)); RCHK(m.get(d_acc, M)); RCHK(m.get(d_glen, G)); RCHK(m.get(d_ghash, G));
    RCHK(m.get(d_counted, G)); RCHK(m.get(d_cnt, A)); RCHK(m.get(d_firstg, A)); RCHK(m.get(d_gslot, G));
    RCHK(m.get(d_first, G)); RCHK(m.get(d_cid, G)); RCHK(m.get(d_tkey, ts)); RCHK(m.get(d_tfirst, ts));
    hipLaunchKernelGGL(k_rec_gstart, dim3(nblk(M, 256)), dim3(256), 0, st, d_head, d_gid, (long)M, d_gstart);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(d_gstart + G, &M, 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(d_cnt, 0, (size_t)std::max(A, 1) * 8, st));
    HIPCHK(hipMemsetAsync(d_firstg, 0xFF, (size_t)std::max(A, 1) * 4, st));
    HIPCHK(hipMemsetAsync(d_tkey, 0xFF, (size_t)ts * 8, st));
    HIPCHK(hipMemsetAsync(d_tfirst, 0xFF, (size_t)ts * 4, st));
    const int collide = hgx_test_switch("linear_collide") != nullptr;
    hipLaunchKernelGGL(k_lin_groups, dim3(nblk(G, 256)), dim3(256), 0, st, d_gstart, (long)G, c_aid, c_as, ll.d_rank,
                       (int)o.aligner, last_trigger, collide, d_acc, d_glen, d_ghash, d_counted, d_cnt, d_firstg);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_lin_insert, dim3(nblk(G, 256)), dim3(256), 0, st, d_ghash, d_counted, (long)G, d_tkey, d_tfirst, ts - 1, d_gslot);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_lin_verify, dim3(nblk(G, 256)), dim3(256), 0, st, d_gstart, d_acc, d_glen, d_counted, d_gslot, d_tfirst,
                       (long)G, d_first, d_dec);
    HIPCHK(hipGetLastError());
    RCHK(hgx_scan_u32_dev(d_first, d_cid, G, d_scan, d_tot + 2, st));
    uint32_t C = 0;
    HIPCHK(hipMemcpyAsync(&h_dec, d_dec, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&C, d_tot + 2, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (h_dec) {
        *declined = HGX_LIN_DECLINE_COLLISION;
        return HGX_OK;
    }
    unsigned long long *d_ccount;
    uint32_t *d_clen, *d_csrc, *d_coff;
    RCHK(m.get(d_ccount, C)); RCHK(m.get(d_clen, C)); RCHK(m.get(d_csrc, C)); RCHK(m.get(d_coff, C));
    HIPCHK(hipMemsetAsync(d_ccount, 0, (size_t)std::max<uint32_t>(C, 1) * 8, st));
    hipLaunchKernelGGL(k_lin_class, dim3(nblk(G, 256)), dim3(256), 0, st, d_counted, d_first, d_gslot, d_tfirst, d_cid, d_glen, d_gstart,
                       (long)G, d_ccount, d_clen, d_csrc);
    HIPCHK(hipGetLastError());
    uint32_t n_ids = 0;
    if (C) {
        RCHK(hgx_scan_u32_dev(d_clen, d_coff, C, d_scan, d_tot + 3, st));
        HIPCHK(hipMemcpyAsync(&n_ids, d_tot + 3, 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    int32_t *d_ids;
    RCHK(m.get(d_ids, n_ids));
    if (C) {
        hipLaunchKernelGGL(k_lin_gather, dim3(nblk(C, 256)), dim3(256), 0, st, d_clen, d_csrc, d_coff, (long)C, d_acc, d_ids);
        HIPCHK(hipGetLastError());
    }
    std::vector<unsigned long long> cnt(A), ccount(C);
    std::vector<uint32_t> firstg(A), coff(C);
    out.cls_ids.resize(n_ids);
    if (A) {
        HIPCHK(hipMemcpyAsync(cnt.data(), d_cnt, (size_t)A * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(firstg.data(), d_firstg, (size_t)A * 4, hipMemcpyDeviceToHost, st));
    }
    if (C) {
        HIPCHK(hipMemcpyAsync(ccount.data(), d_ccount, (size_t)C * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(coff.data(), d_coff, (size_t)C * 4, hipMemcpyDeviceToHost, st));
    }
    if (n_ids) HIPCHK(hipMemcpyAsync(out.cls_ids.data(), d_ids, (size_t)n_ids * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    // Gene_counts in insertion order: by the first group that counted on the allele (one group counts on one trigger)
    std::vector<int32_t> order;
    for (int a = 0; a < A; ++a)
        if (cnt[a]) order.push_back(a);
    std::sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return firstg[x] < firstg[y]; });
    out.count_id.assign(order.begin(), order.end());
    out.count_val.clear();
    for (int32_t a : order) out.count_val.push_back((int64_t)cnt[a]);
    if (G > 0 && last_trigger < 0) {                        // the last group's count on a name outside the locus (it is the last new key)
        out.count_id.push_back(hgx_linear_name_id(out, ll, lin_last_rname(in)));
        out.count_val.push_back(1);
    }
    out.cls_off.assign(C + 1, 0);
    out.cls_count.assign(C, 0);
    for (uint32_t c = 0; c < C; ++c) { out.cls_off[c] = (int32_t)coff[c]; out.cls_count[c] = (int64_t)ccount[c]; }
    out.cls_off[C] = (int32_t)n_ids;
    return HGX_OK;
}

// the host route's form of the records: text lines (a BAM is decoded to text once, on the first decline)
static int lin_host_text(hgx_linear_input &in, const char *&base, const uint64_t *&ls, const uint64_t *&le, size_t &n) {
    if (!in.binary) { base = in.base; ls = in.ls.data(); le = in.le.data(); n = in.ls.size(); return HGX_OK; }
    if (!in.host_text) {
        size_t tot;
        RCHK(bam_as_sam_text(in.path.c_str(), in.has_regions ? in.regions.c_str() : nullptr, SIZE_MAX, in.text, tot, &in.t_ls, &in.t_le));
        in.host_text = true;
    }
    base = in.text.data(); ls = in.t_ls.data(); le = in.t_le.data(); n = in.t_ls.size();
    return HGX_OK;
}

static int lin_type(hgx_linear **out, hgx_linear_locus *ll, hgx_linear_input &in, const hgx_linear_opts *o, void *stream) {
    std::unique_ptr<hgx_linear> r(new hgx_linear());
    const bool force = hgx_switch_has("front", "device");
    const bool host_only = hgx_switch_has("front", "host");
    int declined = host_only ? HGX_LIN_DECLINE_FORCED : (!force && (int64_t)in.ls.size() < HGX_LIN_MIN_RECORDS) ? HGX_LIN_DECLINE_SMALL : 0;
    if (!declined) {
        const int rc = lin_device(*r, *ll, in, *o, (hipStream_t)stream, &declined);
        if (rc) { hgx_front_set_last(0, 0, 0); return rc; }
    }
    if (declined) {
        const char *base;
        const uint64_t *ls, *le;
        size_t n;
        int rc = lin_host_text(in, base, ls, le, n);
        if (!rc) rc = hgx_linear_host(*r, *ll, base, ls, le, n, *o);
        hgx_front_set_last(0, declined, 0);
        if (rc) return rc;
        r->route = 0;
        r->decline = declined;
    } else {
        hgx_front_set_last(2, 0, in.last_up);
        r->route = 2;
    }
    *out = r.release();
    return HGX_OK;
}

extern "C" int hgx_linear_locus_create(hgx_linear_locus **out, const char *name_pool, size_t n_bytes, int32_t n_names) {
    ARGCHK(out && (name_pool || n_bytes == 0) && n_names >= 0);
    auto *ll = new hgx_linear_locus();
    size_t p = 0;
    for (int32_t a = 0; a < n_names; ++a) {
        const char *z = (const char *)memchr(name_pool + p, 0, n_bytes - p);
        if (!z) { delete ll; hgx_set_error("invalid argument: name pool holds fewer than %d names", n_names); return HGX_EINVAL; }
        const size_t len = (size_t)(z - (name_pool + p));
        ll->name.emplace_back(name_pool + p, len);
        ll->id.emplace(ll->name.back(), a);            // a repeated name keeps its first index, as a dict lookup would
        p += len + 1;
    }
    std::vector<int32_t> idx(n_names);
    for (int32_t a = 0; a < n_names; ++a) idx[a] = a;
    std::stable_sort(idx.begin(), idx.end(), [&](int32_t x, int32_t y) { return ll->name[x] < ll->name[y]; });
    ll->rank.assign(n_names, 0);
    for (int32_t k = 0; k < n_names; ++k) ll->rank[idx[k]] = k;
    *out = ll;
    return HGX_OK;
}

extern "C" int hgx_linear_locus_destroy(hgx_linear_locus *ll) {
    if (!ll) return HGX_OK;
    lin_free_names(*ll);
    delete ll;
    return HGX_OK;
}

extern "C" int hgx_linear_type_sam(hgx_linear **out, hgx_linear_locus *ll, const char *sam, size_t n_bytes, const hgx_linear_opts *opts,
                                   void *stream) {
    ARGCHK(out && ll && opts && (sam || n_bytes == 0));
    hgx_linear_input in;
    in.base = sam ? sam : "";
    in.n_bytes = n_bytes;
    hgx_linear_lines(in.base, n_bytes, in.ls, in.le);
    return lin_type(out, ll, in, opts, stream);
}

extern "C" int hgx_linear_input_open(hgx_linear_input **out, const char *path, const char *regions_or_null) {
    ARGCHK(out && path);
    *out = nullptr;
    std::unique_ptr<hgx_linear_input> in(new hgx_linear_input());
    in->path = path;
    in->has_regions = regions_or_null != nullptr;
    if (regions_or_null) in->regions = regions_or_null;
    in->al.file_order = true;
    RCHK(hgx_read_alignment_lines(path, regions_or_null, 0, in->al, /*keep_binary=*/true));
    in->base = in->al.raw;
    in->n_bytes = in->al.raw_bytes;
    in->binary = in->al.binary;
    in->refs = in->al.ref_names;
    const size_t N = in->al.lines.size();
    in->ls.resize(N);
    in->le.resize(N);
    for (size_t i = 0; i < N; ++i) {
        const hgx_line &l = in->al.lines[i];
        if (in->binary) { in->ls[i] = (uint64_t)(l.p - 32 - in->base); in->le[i] = l.len; }     // record start (refID), block_size
        else { in->ls[i] = (uint64_t)(l.p - in->base); in->le[i] = in->ls[i] + l.len; }
        if (!in->base || l.p < in->base || (uint64_t)(l.p - in->base) > in->n_bytes) {
            hgx_set_error("hgx_linear_input_open: a record outside the reader's buffer");
            return HGX_EINVAL;
        }
    }
    *out = in.release();
    return HGX_OK;
}

extern "C" int hgx_linear_input_dims(const hgx_linear_input *in, int64_t *n_records, int32_t *is_bam, size_t *n_bytes) {
    ARGCHK(in);
    if (n_records) *n_records = (int64_t)in->ls.size();
    if (is_bam) *is_bam = in->binary ? 1 : 0;
    if (n_bytes) *n_bytes = in->n_bytes;
    return HGX_OK;
}

extern "C" int hgx_linear_input_close(hgx_linear_input *in) {
    delete in;
    return HGX_OK;
}

extern "C" int hgx_linear_type_input(hgx_linear **out, hgx_linear_input *in, hgx_linear_locus *ll, const hgx_linear_opts *opts, void *stream) {
    ARGCHK(out && in && ll && opts);
    return lin_type(out, ll, *in, opts, stream);
}

extern "C" int hgx_linear_type_file(hgx_linear **out, hgx_linear_locus *ll, const char *path, const char *regions_or_null,
                                    const hgx_linear_opts *opts, void *stream) {
    ARGCHK(out && ll && path && opts);
    hgx_linear_input *in = nullptr;
    RCHK(hgx_linear_input_open(&in, path, regions_or_null));
    const int rc = lin_type(out, ll, *in, opts, stream);
    hgx_linear_input_close(in);
    return rc;
}

extern "C" int hgx_linear_dims(const hgx_linear *r, int32_t *n_counted, int32_t *n_classes, int64_t *n_class_ids, int32_t *n_extra,
                               size_t *extra_bytes, int64_t *n_groups) {
    ARGCHK(r);
    if (n_counted) *n_counted = (int32_t)r->count_id.size();
    if (n_classes) *n_classes = (int32_t)r->cls_count.size();
    if (n_class_ids) *n_class_ids = (int64_t)r->cls_ids.size();
    if (n_extra) *n_extra = (int32_t)r->extra.size();
    if (extra_bytes) {
        size_t b = 0;
        for (const auto &s : r->extra) b += s.size() + 1;
        *extra_bytes = b;
    }
    if (n_groups) *n_groups = r->n_groups;
    return HGX_OK;
}

extern "C" int hgx_linear_counts(const hgx_linear *r, int32_t *name_id, int64_t *count) {
    ARGCHK(r);
    for (size_t k = 0; k < r->count_id.size(); ++k) {
        if (name_id) name_id[k] = r->count_id[k];
        if (count) count[k] = r->count_val[k];
    }
    return HGX_OK;
}

extern "C" int hgx_linear_classes(const hgx_linear *r, int64_t *offsets, int32_t *name_ids, int64_t *count) {
    ARGCHK(r);
    const size_t C = r->cls_count.size();
    if (offsets)
        for (size_t c = 0; c <= C; ++c) offsets[c] = r->cls_off[c];
    if (name_ids && !r->cls_ids.empty()) memcpy(name_ids, r->cls_ids.data(), r->cls_ids.size() * 4);
    if (count)
        for (size_t c = 0; c < C; ++c) count[c] = r->cls_count[c];
    return HGX_OK;
}

extern "C" int hgx_linear_extra_names(const hgx_linear *r, char *pool) {
    ARGCHK(r && pool);
    for (const auto &s : r->extra) {
        memcpy(pool, s.data(), s.size());
        pool += s.size();
        *pool++ = 0;
    }
    return HGX_OK;
}

extern "C" int hgx_linear_destroy(hgx_linear *r) {
    delete r;
    return HGX_OK;
}

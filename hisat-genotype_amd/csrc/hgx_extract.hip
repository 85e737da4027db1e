// hgx_extract.hip -- read extraction from a genome-wide alignment stream on the device (typing_process.py:1630-1745;
// include/hgx.h "read extraction").
//
// The reference walks the aligner's SAM over the whole genotype genome and writes, per locus family, the read pairs with a hit
// in one of the family's regions.  The stream arrives in chunks cut on group boundaries (ext_feed); per chunk, in order:
//   k_ext_records   one thread per line: columns as str.split() cuts them, FLAG, POS - 1, RNAME -> chromosome (name_lookup of
//                   hgx_records.hpp: device hash of the region table's chromosome names, exact byte compare) -> the family of
//                   the first region of that chromosome holding the position, AS / XS / NH (cols[11:] by their first two
//                   characters, last one wins), the hash of the read name (up to '|' in simulation mode), and where QNAME, SEQ
//                   and QUAL lie; anything the host route has to word (a short line, a value int() refuses) declines
//   k_rec_heads     a record opens a group where its name differs from the previous record's (hash, then bytes)
//   scan + k_rec_gstart      group extents (k_scan_u32; both kernels shared with the linear route: hgx_records.hpp)
//   k_ext_groups    one thread per group: read1_first / read2_first carried in record order, the hit condition as Python parses
//                   it, the family bit set (<= 64 families), read 1 = the first left record, read 2 = the LAST right record
//   scan + k_ext_hits        the groups with a family, in order
//   per family met: k_ext_sizes + two scans (output bytes per mate), then
//   k_ext_emit      one wavefront per hit group and mate: SEQ and QUAL staged into LDS with 16-byte loads, the FASTQ / FASTA text
//                   (reverse complement, reversed quality) formed in LDS at the destination's alignment, written with dword stores
// Bytes per record: the line once (k_ext_records), 8 B of line table in, 64 B of fields out; per group 24 B; per written read
// its text twice (LDS in between).
#include <algorithm>
#include <cstdio>
#include <functional>
#include <memory>
#include <vector>

#include "hgx_common.hpp"
#include "hgx_internal.hpp"
#include "hgx_extract.hpp"
#include "hgx_reads.hpp"
#include "hgx_records.hpp"
#include "hgx_bam_walk.hpp"

__device__ static inline bool ext_sp(char c) { return c == ' ' || (c >= '\t' && c <= '\r') || (c >= 0x1c && c <= 0x1f); }

// a plain integer of 32 bits (sign, digits); anything else int() may still take (underscores) is the host route's
__device__ static inline bool ext_int(const char *p, uint32_t n, int64_t &v) {
    uint32_t i = 0;
    bool neg = false;
    if (i < n && (p[i] == '+' || p[i] == '-')) neg = p[i++] == '-';
    if (i >= n || n - i > 10) return false;
    int64_t x = 0;
    for (; i < n; ++i) {
        if (p[i] < '0' || p[i] > '9') return false;
        x = x * 10 + (p[i] - '0');
    }
    if (x > 0x7fffffffll) return false;
    v = neg ? -x : x;
    return true;
}

struct ExtRec {                         // per record, structure of arrays
    uint32_t *flag, *tags, *qoff, *qlen, *klen, *soff, *slen, *loff, *llen;
    int32_t *fam, *as, *xs, *nh;
    uint64_t *kh;
};
constexpr uint32_t EXT_HAS_AS = 1, EXT_HAS_XS = 2, EXT_HAS_NH = 4;

__global__ void k_ext_records(const char *__restrict__ text, const uint32_t *__restrict__ ls, const uint32_t *__restrict__ le, long N,
                              const hgx_name_view chroms, const uint32_t *__restrict__ creg, const int32_t *__restrict__ rfam,
                              const long long *__restrict__ rl, const long long *__restrict__ rr, int simulation, ExtRec R,
                              uint32_t *__restrict__ decline) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const uint32_t e = le[i];
    uint32_t pos = ls[i];
    int col = 0;
    uint32_t q0 = 0, qn = 0, f0 = 0, fn = 0, r0 = 0, rn = 0, p0o = 0, pn = 0, s0 = 0, sn = 0, l0 = 0, ln = 0;
    uint32_t tags = 0;
    int64_t v_as = 0, v_xs = 0, v_nh = 0;
    bool bad_value = false, bad_byte = false;
    while (pos < e) {
        while (pos < e && ext_sp(text[pos])) ++pos;
        if (pos >= e) break;
        const uint32_t b = pos;
        while (pos < e && !ext_sp(text[pos])) { bad_byte |= (text[pos] & 0x80) != 0; ++pos; }
        const uint32_t n = pos - b;
        switch (col) {
            case 0: q0 = b; qn = n; break;
            case 1: f0 = b; fn = n; break;
            case 2: r0 = b; rn = n; break;
            case 3: p0o = b; pn = n; break;
            case 9: s0 = b; sn = n; break;
            case 10: l0 = b; ln = n; break;
            default: break;
        }
        if (col >= 11 && n >= 2) {
            const char a = text[b], c = text[b + 1];
            const int t = (a == 'A' && c == 'S') ? 0 : (a == 'X' && c == 'S') ? 1 : (a == 'N' && c == 'H') ? 2 : -1;
            if (t >= 0) {
                int64_t v = 0;
                if (n <= 5 || !ext_int(text + b + 5, n - 5, v)) bad_value = true;
                if (t == 0) v_as = v; else if (t == 1) v_xs = v; else v_nh = v;
                tags |= 1u << t;
            }
        }
        ++col;
    }
    // (the group kernel reads every record of a group: a declined record still gets defined fields)
    R.flag[i] = 0x4; R.tags[i] = 0; R.fam[i] = -1; R.kh[i] = 0; R.qoff[i] = ls[i]; R.qlen[i] = 0; R.klen[i] = 0;
    R.soff[i] = R.loff[i] = ls[i]; R.slen[i] = R.llen[i] = 0; R.as[i] = R.xs[i] = R.nh[i] = 0;
    if (col < 11 || bad_byte) { atomicOr(decline, 1u << HGX_EXT_DECLINE_RECORD); return; }
    int64_t flag, p1;
    if (bad_value || !ext_int(text + f0, fn, flag) || !ext_int(text + p0o, pn, p1)) {
        atomicOr(decline, 1u << HGX_EXT_DECLINE_VALUE);
        return;
    }
    const long long p0 = p1 - 1;
    int32_t fam = -1;
    if (!(flag & 0x4)) {
        const int32_t c = name_lookup(chroms, text + r0, rn);
        if (c >= 0) {
            for (uint32_t x = creg[c]; x < creg[c + 1]; ++x)
                if (p0 >= rl[x] && p0 < rr[x]) { fam = rfam[x]; break; }
        }
    }
    const char *q = text + q0;
    uint32_t kn = qn;
    if (simulation) {
        for (uint32_t k = 0; k < qn; ++k)
            if (q[k] == '|') { kn = k; break; }
        if (kn == 0) atomicOr(decline, 1u << HGX_EXT_DECLINE_NAMES);
    }
    R.flag[i] = (uint32_t)(flag & 0xffff);
    R.tags[i] = tags;
    R.fam[i] = fam;
    R.as[i] = (int32_t)v_as; R.xs[i] = (int32_t)v_xs; R.nh[i] = (int32_t)v_nh;
    R.kh[i] = fnv1a(q, kn);
    R.qoff[i] = q0; R.qlen[i] = qn; R.klen[i] = kn;
    R.soff[i] = s0; R.slen[i] = sn;
    R.loff[i] = l0; R.llen[i] = ln;
}

// BAM: one lane per record of the inflated stream (rec_off: behind its block_size word, rec_len: block_size).  It fills the arrays
// k_ext_records fills, so everything behind it runs unchanged, and it declines whatever would make the line `samtools view`
// prints for the record (hgx_bam.cpp: bam_record_text, the contract) split otherwise than the BAM fields lie: a blank, a control
// blank or a byte >= 0x80 in QNAME, in a tag or in an A / Z / H value, a reference name of that kind (reftab -2), a quality whose
// + 33 leaves ASCII, a QNAME that starts a header line, damaged aux data.  reftab: per refID the chromosome's index in the region
// table or -1.  AS / XS / NH: every tag is walked by its type, the last occurrence wins, the integer types count.
__global__ void k_ext_bam_records(const unsigned char *__restrict__ text, const uint32_t *__restrict__ rec_off, const uint32_t *__restrict__ rec_len,
                                  long N, const int32_t *__restrict__ reftab, int n_ref, const uint32_t *__restrict__ creg,
                                  const int32_t *__restrict__ rfam, const long long *__restrict__ rl, const long long *__restrict__ rr, int simulation,
                                  ExtRec R, uint32_t *__restrict__ decline) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const uint32_t o = rec_off[i], bs = rec_len[i];
    const unsigned char *r = text + o;
    // (the group kernel reads every record of a group: a declined record still gets defined fields)
    R.flag[i] = 0x4; R.tags[i] = 0; R.fam[i] = -1; R.kh[i] = 0; R.qoff[i] = o + 32; R.qlen[i] = 0; R.klen[i] = 0;
    R.soff[i] = R.loff[i] = o + 32; R.slen[i] = R.llen[i] = 0; R.as[i] = R.xs[i] = R.nh[i] = 0;
    const int32_t rid = bam_i32(r), pos = bam_i32(r + 4), l_seq = bam_i32(r + 16), nrid = bam_i32(r + 20);
    const uint32_t l_rn = r[8], n_cig = bam_u16(r + 12), flag = bam_u16(r + 14);
    const size_t fixed = 32 + (size_t)l_rn + 4 * (size_t)n_cig + (l_seq > 0 ? (size_t)(l_seq + 1) / 2 + (size_t)l_seq : 0);
    if (l_rn == 0 || l_seq < 0 || fixed > bs) { atomicOr(decline, 1u << HGX_EXT_DECLINE_RECORD); return; }
    auto bad_text = [](uint32_t c) { return c >= 0x80u || ext_sp((char)c); };
    uint32_t dec = 0;
    const unsigned char *q = r + 32;
    const uint32_t qn = l_rn - 1;
    uint32_t kn = qn;
    for (uint32_t k = 0; k < qn; ++k) {
        const uint32_t c = q[k];
        if (bad_text(c) || c == 0) dec |= 1u << HGX_EXT_DECLINE_RECORD;
        if (simulation && c == '|' && kn == qn) kn = k;
    }
    if (qn && q[0] == '@') dec |= 1u << HGX_EXT_DECLINE_RECORD;
    if (kn == 0) dec |= 1u << HGX_EXT_DECLINE_NAMES;
    if (rid >= n_ref || (rid >= 0 && reftab[rid] == -2)) dec |= 1u << HGX_EXT_DECLINE_RECORD;
    if (nrid >= 0 && nrid < n_ref && nrid != rid && reftab[nrid] == -2) dec |= 1u << HGX_EXT_DECLINE_RECORD;
    const uint32_t so = 32 + l_rn + 4 * n_cig, lo = so + (uint32_t)(l_seq + 1) / 2;          // (within the record)
    const bool no_qual = l_seq == 0 || r[lo] == 0xff;
    if (!no_qual) {
        uint32_t top = 0;
        for (int32_t k = 0; k < l_seq; ++k) top = max(top, (uint32_t)r[lo + k]);
        if (top + 33 >= 0x80u) dec |= 1u << HGX_EXT_DECLINE_RECORD;
    }
    uint32_t tags = 0;
    int32_t v_as = 0, v_xs = 0, v_nh = 0;
    size_t a = fixed;
    while (a + 3 <= bs) {
        const uint32_t t0 = r[a], t1 = r[a + 1], ty = r[a + 2];
        a += 3;
        if (bad_text(t0) || bad_text(t1)) dec |= 1u << HGX_EXT_DECLINE_RECORD;
        const int which = (t0 == 'A' && t1 == 'S') ? 0 : (t0 == 'X' && t1 == 'S') ? 1 : (t0 == 'N' && t1 == 'H') ? 2 : -1;
        size_t sz = 0;
        bool broken = false, is_int = false;
        switch (ty) {
            case 'A': case 'c': case 'C': sz = 1; break;
            case 's': case 'S': sz = 2; break;
            case 'i': case 'I': case 'f': sz = 4; break;
            case 'Z': case 'H': {
                size_t e = a;
                while (e < bs && r[e] != 0) { if (bad_text(r[e])) dec |= 1u << HGX_EXT_DECLINE_RECORD; ++e; }
                broken = e >= bs;
                sz = e - a + 1;
            } break;
            case 'B': {
                if (a + 5 > bs) { broken = true; break; }
                const uint32_t st = r[a];
                const size_t w = (st == 'c' || st == 'C') ? 1 : (st == 's' || st == 'S') ? 2 : (st == 'i' || st == 'I' || st == 'f') ? 4 : 0;
                broken = w == 0;
                sz = 5 + w * (size_t)bam_u32(r + a + 1);
            } break;
            default: broken = true;
        }
        if (broken || a + sz > bs) { dec |= 1u << HGX_EXT_DECLINE_RECORD; a = bs; break; }
        long long v = 0;
        switch (ty) {
            case 'A': if (bad_text(r[a])) dec |= 1u << HGX_EXT_DECLINE_RECORD; break;
            case 'c': v = (int8_t)r[a]; is_int = true; break;
            case 'C': v = r[a]; is_int = true; break;
            case 's': v = (int16_t)bam_u16(r + a); is_int = true; break;
            case 'S': v = bam_u16(r + a); is_int = true; break;
            case 'i': v = bam_i32(r + a); is_int = true; break;
            case 'I': v = bam_u32(r + a); is_int = true; break;
            default: break;
        }
        if (which >= 0) {
            // (the text kernel takes a sign and up to 2^31 - 1: the same range here, so that both decline the same streams)
            if (!is_int || v > 0x7fffffffll || v < -0x7fffffffll) dec |= 1u << HGX_EXT_DECLINE_VALUE;
            else if (which == 0) v_as = (int32_t)v;
            else if (which == 1) v_xs = (int32_t)v;
            else v_nh = (int32_t)v;
            tags |= 1u << which;
        }
        a += sz;
    }
    if (a != bs) dec |= 1u << HGX_EXT_DECLINE_RECORD;
    if (dec) { atomicOr(decline, dec); return; }
    int32_t fam = -1;
    if (!(flag & 0x4) && rid >= 0) {
        const int32_t c = reftab[rid];
        if (c >= 0) {
            const long long p0 = pos;
            for (uint32_t x = creg[c]; x < creg[c + 1]; ++x)
                if (p0 >= rl[x] && p0 < rr[x]) { fam = rfam[x]; break; }
        }
    }
    R.flag[i] = flag;
    R.tags[i] = tags;
    R.fam[i] = fam;
    R.as[i] = v_as; R.xs[i] = v_xs; R.nh[i] = v_nh;
    R.kh[i] = fnv1a((const char *)q, kn);
    R.qoff[i] = o + 32; R.qlen[i] = qn; R.klen[i] = kn;
    R.soff[i] = o + so; R.slen[i] = l_seq ? (uint32_t)l_seq : 1u;
    R.loff[i] = o + lo; R.llen[i] = no_qual ? 1u : (uint32_t)l_seq;
}

// The loop body of process:1678-1713 for one group, in record order.
__global__ void k_ext_groups(const uint32_t *__restrict__ gstart, long G, ExtRec R, int aligner, int paired,
                             unsigned long long *__restrict__ gbits, uint32_t *__restrict__ r1, uint32_t *__restrict__ r2,
                             uint32_t *__restrict__ ghit, unsigned long long *__restrict__ fam_or, uint32_t *__restrict__ decline) {
    const long g = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G) return;
    const uint32_t s = gstart[g], e = gstart[g + 1];
    bool r1f = true, r2f = true;
    unsigned long long bits = 0;
    uint32_t i1 = ~0u, i2 = ~0u, dec = 0;
    for (uint32_t j = s; j < e; ++j) {
        const uint32_t flag = R.flag[j], tags = R.tags[j];
        const bool left = (flag & 0x40) || !paired;
        if (!(flag & 0x4)) {
            bool hit = aligner == 0 && (tags & EXT_HAS_NH) && R.nh[j] == 1;
            if (!hit) {
                if (left) {
                    if (aligner == 1) {
                        const bool a = tags & EXT_HAS_AS, x = tags & EXT_HAS_XS;
                        if (a != x) dec |= 1u << HGX_EXT_DECLINE_TYPE;
                        hit = a && x && R.as[j] > R.xs[j] && r1f;
                    }
                } else hit = r2f;
            }
            const int32_t f = R.fam[j];
            if (hit && f >= 0) bits |= 1ull << f;
        }
        if (left) {
            r1f = false;
            if (i1 == ~0u) i1 = j;
        } else {
            if (!(flag & 0x80)) dec |= 1u << HGX_EXT_DECLINE_MATE;
            r2f = false;
            i2 = j;
        }
    }
    if (bits && (i1 == ~0u || (paired && i2 == ~0u))) dec |= 1u << HGX_EXT_DECLINE_INDEX;
    if (dec) atomicOr(decline, dec);
    gbits[g] = bits;
    r1[g] = i1;
    r2[g] = i2;
    ghit[g] = bits ? 1u : 0u;
    if (bits) atomicOr(fam_or, bits);
}

__global__ void k_ext_hits(const uint32_t *__restrict__ ghit, const uint32_t *__restrict__ hpos, long G, uint32_t *__restrict__ hg) {
    const long g = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g < G && ghit[g]) hg[hpos[g]] = (uint32_t)g;
}

// bytes one read takes in its file: "@name\nSEQ\n+\nQUAL\n" or ">name\nSEQ\n"
__device__ static inline uint32_t ext_read_bytes(uint32_t name_n, uint32_t seq_n, uint32_t qual_n, int fastq) {
    return 1 + name_n + 1 + seq_n + 1 + (fastq ? 2 + qual_n + 1 : 0);
}

__global__ void k_ext_sizes(const uint32_t *__restrict__ hg, long H, const unsigned long long *__restrict__ gbits, int fam,
                            const uint32_t *__restrict__ gstart, const uint32_t *__restrict__ r1, const uint32_t *__restrict__ r2,
                            ExtRec R, int paired, int fastq, uint32_t *__restrict__ sz1, uint32_t *__restrict__ sz2,
                            unsigned long long *__restrict__ total, unsigned long long *__restrict__ count) {
    const long h = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (h >= H) return;
    const uint32_t g = hg[h];
    uint32_t a = 0, b = 0;
    if ((gbits[g] >> fam) & 1ull) {
        const uint32_t nn = R.qlen[gstart[g]];
        a = ext_read_bytes(nn, R.slen[r1[g]], R.llen[r1[g]], fastq);
        if (paired) b = ext_read_bytes(nn, R.slen[r2[g]], R.llen[r2[g]], fastq);
        atomicAdd(total, (unsigned long long)a + b);
        atomicAdd(count, 1ull);
    }
    sz1[h] = a;
    sz2[h] = b;
}

constexpr int EXT_SRC_MAX = 4096;        // SEQ .. QUAL of one record staged in LDS (bytes, 16-byte granules)
constexpr int EXT_IMG_MAX = 4608;        // the read's text in LDS

__device__ static inline char ext_comp(char c) { return c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : c; }

// One wavefront (= one block) per hit group and mate.  The record's SEQ and QUAL columns are neighbours in the line: their
// span is read with 16-byte loads from its 16-byte-aligned start into LDS, the text is formed byte by byte in LDS, shifted by the
// destination's offset within its dword, and leaves as whole dwords (the partial first and last dword as bytes: the neighbour
// read's text shares them).  A read whose span or text does not fit in LDS is copied byte by byte.
// BAM = true: `text` is the inflated stream; soff / loff are where the record's 4-bit bases and its binary qualities lie, slen /
// llen the lengths of the text `samtools view` prints for them (1 for the '*' of an empty SEQ, or of qualities that start with 0xff);
// l_seq is read from the record (qoff is its read_name: 32 bytes behind the record's start).  The staged span holds the packed
// bases and the qualities; a base comes through the 16-entry table, high nibble first.
__device__ static inline char ext_base(uint32_t code) {                 // "=ACMGRSVTWYHKDBN"[code], the table in two registers
    const unsigned long long w = code < 8 ? 0x565352474d43413dull : 0x4e42444b48595754ull;
    return (char)(w >> (8 * (code & 7)));
}
template <bool BAM>
__global__ void __launch_bounds__(64) k_ext_emit(const char *__restrict__ text, const uint32_t *__restrict__ hg, long H,
                                                 const unsigned long long *__restrict__ gbits, int fam,
                                                 const uint32_t *__restrict__ gstart, const uint32_t *__restrict__ r1,
                                                 const uint32_t *__restrict__ r2, ExtRec R, int fastq, const uint32_t *__restrict__ off1,
                                                 const uint32_t *__restrict__ off2, char *__restrict__ out1, char *__restrict__ out2) {
    __shared__ __attribute__((aligned(16))) char s_src[EXT_SRC_MAX];
    __shared__ __attribute__((aligned(16))) char s_img[EXT_IMG_MAX];
    const long h = blockIdx.x >> 1;
    const int mate = blockIdx.x & 1;
    const int lane = threadIdx.x;
    if (h >= H) return;
    const uint32_t g = hg[h];
    if (!((gbits[g] >> fam) & 1ull)) return;
    if (mate && !out2) return;
    const uint32_t rec = mate ? r2[g] : r1[g], first = gstart[g];
    const char *name = text + R.qoff[first];
    const uint32_t nn = R.qlen[first], sn = R.slen[rec], ln = R.llen[rec];
    const uint32_t so = R.soff[rec], lo = R.loff[rec];
    uint32_t l_seq = 0;                                                 // BAM: bases in the record (0: SEQ prints '*')
    if (BAM) __builtin_memcpy(&l_seq, text + R.qoff[rec] - 16, 4);
    const bool seq_star = BAM && l_seq == 0, qual_star = BAM && (l_seq == 0 || (uint8_t)text[lo] == 0xff);
    const bool rev = (R.flag[rec] & 0x10) != 0;
    char *dst = (mate ? out2 : out1) + (mate ? off2[h] : off1[h]);
    const uint32_t total = ext_read_bytes(nn, sn, ln, fastq);
    const uint32_t a0 = so & ~15u;
    const uint32_t span = (BAM ? (fastq ? lo + l_seq : lo) : (fastq ? lo + ln : so + sn)) - a0;
    const uint32_t pad = (uint32_t)((uintptr_t)dst & 3u);
    const bool staged = span <= (uint32_t)EXT_SRC_MAX && pad + total <= (uint32_t)EXT_IMG_MAX && (!fastq || lo >= so);
    // where the pieces start in the text
    const uint32_t p_seq = 1 + nn + 1, p_plus = p_seq + sn + 1, p_qual = p_plus + 2;
    if (staged) {
        for (uint32_t k = 16u * lane; k < span; k += 16u * 64)          // (the text buffer is padded: the last granule may read past the line)
            *reinterpret_cast<uint4 *>(s_src + k) = *reinterpret_cast<const uint4 *>(text + a0 + k);
        __syncthreads();
    }
    const char *seq = staged ? s_src + (so - a0) : text + so;
    const char *qual = staged ? s_src + (lo - a0) : text + lo;
    for (uint32_t k = lane; k < total; k += 64) {
        char c;
        if (k == 0) c = fastq ? '@' : '>';
        else if (k <= nn) c = name[k - 1];
        else if (k < p_seq) c = '\n';
        else if (k < p_seq + sn) {
            const uint32_t x = k - p_seq, y = rev ? sn - 1 - x : x;
            if (!BAM) c = seq[y];
            else if (seq_star) c = '*';
            else { const uint32_t b = (uint8_t)seq[y >> 1]; c = ext_base((y & 1) ? (b & 15u) : (b >> 4)); }
            if (rev) c = ext_comp(c);
        }
        else if (k < p_plus) c = '\n';
        else if (k == p_plus) c = '+';
        else if (k < p_qual) c = '\n';
        else if (k < p_qual + ln) {
            const uint32_t x = k - p_qual, y = rev ? ln - 1 - x : x;
            c = !BAM ? qual[y] : qual_star ? '*' : (char)(qual[y] + 33);
        }
        else c = '\n';
        if (staged) s_img[pad + k] = c; else dst[k] = c;
    }
    if (!staged) return;
    __syncthreads();
    const uint32_t end = pad + total;                                   // bytes of the image, from the dword boundary below dst
    uint32_t *dw = reinterpret_cast<uint32_t *>(dst - pad);
    const uint32_t w0 = pad ? 1u : 0u, w1 = end >> 2;                  // whole dwords [w0, w1)
    const uint32_t head_end = pad ? min(end, 4u) : 0u;                 // the bytes of a shared first dword
    if ((uint32_t)lane >= pad && (uint32_t)lane < head_end) dst[lane - pad] = s_img[lane];
    for (uint32_t w = w0 + lane; w < w1; w += 64) dw[w] = *reinterpret_cast<const uint32_t *>(s_img + 4u * w);
    const uint32_t tail0 = max(4u * w1, head_end);                     // the bytes behind the last whole dword
    if (tail0 + lane < end) dst[tail0 + lane - pad] = s_img[tail0 + lane];
}

static void ext_free_table(hgx_extract &h) {
    free_on_device(h.dev, {h.d_chrom.pool, h.d_chrom.off, h.d_chrom.slot, h.d_creg, h.d_rfam, h.d_rl, h.d_rr, h.d_reftab});
    h.d_reftab = nullptr;
    h.d_chrom = hgx_name_view();
    h.d_creg = nullptr; h.d_rfam = nullptr; h.d_rl = h.d_rr = nullptr;
}

static int ext_upload_table(hgx_extract &h) {
    int dev = 0;
    HIPCHK(hipGetDevice(&dev));
    if (h.d_chrom.slot && h.dev == dev) return HGX_OK;
    ext_free_table(h);
    const size_t NR = h.reg_fam.size();
    h.dev = dev;
    const bool ok = name_table_upload(h.d_chrom, h.chrom) && upload_array(h.d_creg, h.creg_off.data(), h.creg_off.size() * 4) &&
                    upload_array(h.d_rfam, h.reg_fam.data(), NR * 4) && upload_array(h.d_rl, h.reg_left.data(), NR * 8) &&
                    upload_array(h.d_rr, h.reg_right.data(), NR * 8);
    if (!ok) {
        const hipError_t e = hipGetLastError();
        ext_free_table(h);
        hgx_set_error("extract route: upload of the region table failed: %s", hipGetErrorString(e));
        return HGX_EHIP;
    }
    return HGX_OK;
}

// the per-record and per-chunk arrays both record kernels fill and the group kernels read
struct ExtWork {
    char *d_scan;
    uint32_t *d_head, *d_gid, *d_dec, *d_tot;
    unsigned long long *d_or;
    ExtRec R;
};
static int ext_work_alloc(DevBufs &m, ExtWork &w, long N, hipStream_t st) {
    ExtRec &R = w.R;
    RCHK(m.get(w.d_head, N + 4)); RCHK(m.get(w.d_gid, N + 4));
    RCHK(m.get(R.flag, N)); RCHK(m.get(R.tags, N)); RCHK(m.get(R.qoff, N)); RCHK(m.get(R.qlen, N)); RCHK(m.get(R.klen, N));
    RCHK(m.get(R.soff, N)); RCHK(m.get(R.slen, N)); RCHK(m.get(R.loff, N)); RCHK(m.get(R.llen, N));
    RCHK(m.get(R.fam, N)); RCHK(m.get(R.as, N)); RCHK(m.get(R.xs, N)); RCHK(m.get(R.nh, N)); RCHK(m.get(R.kh, N));
    RCHK(m.get(w.d_dec, 4)); RCHK(m.get(w.d_tot, 4 + 2 * 64)); RCHK(m.get(w.d_or, 2 + 64));
    RCHK(m.get(w.d_scan, hgx_scan_u32_scratch_bytes(N)));
    HIPCHK(hipMemsetAsync(w.d_dec, 0, 16, st));
    HIPCHK(hipMemsetAsync(w.d_or, 0, (2 + 64) * 8, st));
    return HGX_OK;
}

// keep mode (hgx_extract_keep.hpp holds the bookkeeping): host-route chunks' text becomes host segments in front of what follows
static void ext_keep_flush(hgx_extract &h) { hgx_keep_flush(h.out, h.segs); }
static void ext_keep_drop(hgx_extract &h, size_t k) { hgx_keep_drop(h.segs, k, [](void *p) { hgx_pool_free(p); }); }

// Behind either record kernel: groups, hits, sizes and the text of the chunk's N records (d_text: the SAM text, or, BAM, the
// inflated stream).  *declined != 0: nothing was appended.  keep_last (a BAM chunk that is not the stream's last): the last
// group may go on in the next chunk and stays out -- *n_proc = its first record = the records this call took, *g_first = the
// first record of the last group taken.  before_emit(n_proc, &code), if given, may still decline before anything is written.
template <bool BAM>
static int ext_groups_emit(hgx_extract &h, DevBufs &m, const char *d_text, ExtWork &w, long N, hipStream_t st, int *declined, bool keep_last,
                           const std::function<int(uint32_t, int *)> &before_emit, uint32_t *n_proc, uint32_t *g_first) {
    ExtRec &R = w.R;
    char *d_scan = w.d_scan;
    uint32_t *d_head = w.d_head, *d_gid = w.d_gid, *d_dec = w.d_dec, *d_tot = w.d_tot;
    unsigned long long *d_or = w.d_or;
    hipLaunchKernelGGL(k_rec_heads<uint32_t>, dim3(nblk(N, 256)), dim3(256), 0, st, d_text, R.kh, R.qoff, R.klen, N, d_head);
    HIPCHK(hipGetLastError());
    RCHK(hgx_scan_u32_dev(d_head, d_gid, N, d_scan, d_tot, st));
    uint32_t h_dec = 0, G = 0;
    HIPCHK(hipMemcpyAsync(&h_dec, d_dec, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&G, d_tot, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (h_dec) { *declined = first_decline(h_dec); return HGX_OK; }
    uint32_t *d_gstart, *d_r1, *d_r2, *d_ghit, *d_hpos;
    unsigned long long *d_gbits;
    RCHK(m.get(d_gstart, (size_t)G + 1)); RCHK(m.get(d_r1, G + 4)); RCHK(m.get(d_r2, G)); RCHK(m.get(d_ghit, G + 4)); RCHK(m.get(d_hpos, G + 4));
    RCHK(m.get(d_gbits, G));
    hipLaunchKernelGGL(k_rec_gstart, dim3(nblk(N, 256)), dim3(256), 0, st, d_head, d_gid, N, d_gstart);
    HIPCHK(hipGetLastError());
    const uint32_t n32 = (uint32_t)N;
    HIPCHK(hipMemcpyAsync(d_gstart + G, &n32, 4, hipMemcpyHostToDevice, st));
    if (keep_last) {
        // the last set head flag is the first record of the last group: that group waits for the next chunk
        if (G <= 1) { *n_proc = 0; *g_first = 0; return HGX_OK; }
        uint32_t tail[2] = {0, 0};                                       // first records of the last group taken and of the one kept
        HIPCHK(hipMemcpyAsync(tail, d_gstart + G - 2, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        *g_first = tail[0];
        *n_proc = tail[1];
        G -= 1;
    } else if (n_proc) {
        uint32_t first = 0;
        HIPCHK(hipMemcpyAsync(&first, d_gstart + G - 1, 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        *g_first = first;
        *n_proc = n32;
    }
    if (before_emit) {
        int code = 0;
        RCHK(before_emit(*n_proc, &code));
        if (code) { *declined = code; return HGX_OK; }
    }
    hipLaunchKernelGGL(k_ext_groups, dim3(nblk(G, 256)), dim3(256), 0, st, d_gstart, (long)G, R, h.aligner, h.paired, d_gbits, d_r1, d_r2,
                       d_ghit, d_or, d_dec);
    HIPCHK(hipGetLastError());
    RCHK(hgx_scan_u32_dev(d_ghit, d_hpos, G, d_scan, d_tot + 1, st));
    uint32_t H = 0;
    unsigned long long fam_or = 0;
    HIPCHK(hipMemcpyAsync(&h_dec, d_dec, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&H, d_tot + 1, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&fam_or, d_or, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (h_dec) { *declined = first_decline(h_dec); return HGX_OK; }
    if (H == 0) { h.n_groups += G; return HGX_OK; }
    std::vector<int> fams;
    for (int f = 0; f < h.n_fam; ++f)
        if ((fam_or >> f) & 1ull) fams.push_back(f);
    const size_t F = fams.size();
    uint32_t *d_hg, *d_sz, *d_off;
    const size_t Hp = ((size_t)H + 3) & ~(size_t)3;                     // k_scan_u32 reads and writes 16 bytes at a time: aligned rows
    RCHK(m.get(d_hg, H)); RCHK(m.get(d_sz, 2 * Hp)); RCHK(m.get(d_off, 2 * F * Hp));
    hipLaunchKernelGGL(k_ext_hits, dim3(nblk(G, 256)), dim3(256), 0, st, d_ghit, d_hpos, (long)G, d_hg);
    HIPCHK(hipGetLastError());
    for (size_t k = 0; k < F; ++k) {
        hipLaunchKernelGGL(k_ext_sizes, dim3(nblk(H, 256)), dim3(256), 0, st, d_hg, (long)H, d_gbits, fams[k], d_gstart, d_r1, d_r2, R,
                           h.paired, h.fastq, d_sz, d_sz + Hp, d_or + 1, d_or + 2 + k);
        HIPCHK(hipGetLastError());
        RCHK(hgx_scan_u32_dev(d_sz, d_off + (2 * k) * Hp, H, d_scan, d_tot + 4 + 2 * k, st));
        RCHK(hgx_scan_u32_dev(d_sz + Hp, d_off + (2 * k + 1) * Hp, H, d_scan, d_tot + 4 + 2 * k + 1, st));
    }
    std::vector<uint32_t> tot(2 * F);
    std::vector<unsigned long long> cnt(1 + F);                          // all bytes, then reads per family
    HIPCHK(hipMemcpyAsync(tot.data(), d_tot + 4, 2 * F * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(cnt.data(), d_or + 1, (1 + F) * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (cnt[0] >= (1ull << 31)) { *declined = HGX_EXT_DECLINE_SIZE; return HGX_OK; }
    // one output buffer, a 16-byte aligned part per family and mate
    std::vector<size_t> part(2 * F + 1, 0);
    for (size_t k = 0; k < 2 * F; ++k) part[k + 1] = part[k] + (((size_t)tot[k] + 15) & ~(size_t)15);
    char *d_out;
    RCHK(m.get(d_out, part[2 * F] + 16));
    for (size_t k = 0; k < F; ++k) {
        hipLaunchKernelGGL(k_ext_emit<BAM>, dim3(2 * H), dim3(64), 0, st, d_text, d_hg, (long)H, d_gbits, fams[k], d_gstart, d_r1, d_r2, R, h.fastq,
                           d_off + (2 * k) * Hp, d_off + (2 * k + 1) * Hp, d_out + part[2 * k], h.paired ? d_out + part[2 * k + 1] : (char *)nullptr);
        HIPCHK(hipGetLastError());
    }
    if (h.keep) {                                                        // the parts stay in HBM, each a segment of its family and mate
        ext_keep_flush(h);
        for (size_t k = 0; k < F; ++k)
            for (int mate = 0; mate < (h.paired ? 2 : 1); ++mate) {
                const size_t n = tot[2 * k + mate];
                if (!n) continue;
                hgx_keep_seg sg;
                sg.n = n;
                sg.d = hgx_pool_alloc(n);
                if (!sg.d) { hgx_set_error("device allocation of %zu bytes failed", n); return HGX_ENOMEM; }
                h.segs[2 * fams[k] + mate].push_back(sg);
                HIPCHK(hipMemcpyAsync(sg.d, d_out + part[2 * k + mate], n, hipMemcpyDeviceToDevice, st));
            }
        HIPCHK(hipStreamSynchronize(st));
        for (size_t k = 0; k < F; ++k) h.written[fams[k]] += (int64_t)cnt[1 + k];
        h.n_groups += G;
        return HGX_OK;
    }
    std::vector<char> host(part[2 * F] + 16);
    HIPCHK(hipMemcpyAsync(host.data(), d_out, part[2 * F], hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (size_t k = 0; k < F; ++k) {
        h.out[2 * fams[k]].append(host.data() + part[2 * k], tot[2 * k]);
        if (h.paired) h.out[2 * fams[k] + 1].append(host.data() + part[2 * k + 1], tot[2 * k + 1]);
        h.written[fams[k]] += (int64_t)cnt[1 + k];
    }
    h.n_groups += G;
    return HGX_OK;
}


// the device route for one chunk of text; *declined != 0: nothing was appended, the host route takes the chunk
static int ext_device(hgx_extract &h, const char *base, size_t n_bytes, const std::vector<uint32_t> &ls, const std::vector<uint32_t> &le,
                      hipStream_t st, int *declined) {
    *declined = 0;
    const long N = (long)ls.size();
    if (h.n_fam > 64) { *declined = HGX_EXT_DECLINE_FAMILIES; return HGX_OK; }
    RCHK(ext_upload_table(h));
    DevBufs m("extract route");
    char *d_text;
    uint32_t *d_ls, *d_le;
    ExtWork w;
    RCHK(m.get(d_text, n_bytes + 64));
    RCHK(m.get(d_ls, N)); RCHK(m.get(d_le, N));
    RCHK(ext_work_alloc(m, w, N, st));
    HIPCHK(hipMemcpyAsync(d_text, base, n_bytes, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(d_text + n_bytes, 0, 64, st));
    HIPCHK(hipMemcpyAsync(d_ls, ls.data(), (size_t)N * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_le, le.data(), (size_t)N * 4, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_ext_records, dim3(nblk(N, 256)), dim3(256), 0, st, d_text, d_ls, d_le, N, h.d_chrom, h.d_creg,
                       h.d_rfam, h.d_rl, h.d_rr, h.simulation, w.R, w.d_dec);
    HIPCHK(hipGetLastError());
    RCHK((ext_groups_emit<false>(h, m, d_text, w, N, st, declined, false, nullptr, nullptr, nullptr)));
    if (!*declined) h.up_bytes += (long long)n_bytes + 8ll * N;
    return HGX_OK;
}

// Index of the first record of the last group of lines [0, n), n > 0 (a name counts up to '|' in simulation mode).
static size_t ext_last_group(const hgx_extract &h, const char *base, const std::vector<uint32_t> &ls, const std::vector<uint32_t> &le, size_t n) {
    const char *nm, *pn;
    uint32_t nn, kn, pnn, pkn;
    size_t j = n - 1;
    hgx_extract_name(base + ls[j], le[j] - ls[j], nm, nn, kn);
    if (!h.simulation) kn = nn;
    while (j > 0) {
        hgx_extract_name(base + ls[j - 1], le[j - 1] - ls[j - 1], pn, pnn, pkn);
        if (!h.simulation) pkn = pnn;
        if (pkn != kn || memcmp(pn, nm, kn) != 0) break;
        --j;
    }
    return j;
}

// One chunk: lines [0, n) of `base`, all of whose groups are complete.
static int ext_chunk(hgx_extract &h, const char *base, size_t n_bytes, std::vector<uint32_t> &ls, std::vector<uint32_t> &le, size_t n,
                     hipStream_t st) {
    if (n == 0) return HGX_OK;
    ls.resize(n);
    le.resize(n);
    const bool force = hgx_switch_has("front", "device"), host_only = hgx_switch_has("front", "host");
    int declined = host_only ? HGX_EXT_DECLINE_FORCED : (!force && (int64_t)n < HGX_EXT_MIN_RECORDS) ? HGX_EXT_DECLINE_SMALL : 0;
    if (!declined && h.chk_line && !hgx_extract_chk(h, base, ls.data(), le.data(), n)) declined = HGX_EXT_DECLINE_NAMES;
    if (!declined) {
        const int rc = ext_device(h, base, std::min<size_t>(n_bytes, (size_t)le[n - 1] + 1), ls, le, st, &declined);
        if (rc) { hgx_front_set_last(0, 0, 0); return rc; }
    }
    if (declined) {
        ++h.chunks_host;
        h.last_decline = declined;
        hgx_front_set_last(0, declined, 0);
        return hgx_extract_host(h, base, ls.data(), le.data(), n);
    }
    // what the loop holds behind the chunk: the last group's first name; the chk_line test is over (hgx_extract_chk passed it)
    const size_t j = ext_last_group(h, base, ls, le, n);
    const char *nm;
    uint32_t nn, kn;
    hgx_extract_name(base + ls[j], le[j] - ls[j], nm, nn, kn);
    h.prev_name.assign(nm, nn);
    h.chk_line = false;
    h.n_records += (int64_t)n;
    ++h.chunks_dev;
    hgx_front_set_last(2, 0, (long long)n_bytes + 8ll * (long long)n);
    return HGX_OK;
}

constexpr size_t EXT_MAX_BUF = (size_t)1 << 30;          // offsets are 32 bits wide; a group larger than this is refused

// h.buf holds the carried tail and the new bytes: run every complete group, keep the rest.
static int ext_run(hgx_extract &h, bool last, hipStream_t st) {
    const char *base = h.buf.data();
    size_t nb = h.buf.size();
    if (!last) {                                         // complete lines only
        while (nb > 0 && base[nb - 1] != '\n') --nb;
    }
    std::vector<uint32_t> ls, le;
    hgx_extract_lines(base, nb, ls, le);
    size_t n = ls.size();
    size_t keep_from = nb;                               // first byte carried over
    if (!last && n > 0) {
        // the last group may go on in the next bytes: it is complete once a record with another name has been seen
        n = ext_last_group(h, base, ls, le, n);
        keep_from = ls[n];
    }
    int rc = HGX_OK;
    if (n > 0) rc = ext_chunk(h, base, keep_from, ls, le, n, st);
    if (rc == HGX_OK && !last) {
        if (keep_from > 0) h.buf.erase(h.buf.begin(), h.buf.begin() + (ptrdiff_t)keep_from);
    } else h.buf.clear();
    return rc;
}


// ---- a BAM stream (hgx_extract_feed_bam) ----------------------------------------------------------------------------------------
// Deflated bytes go up in chunks and are inflated there (hgx_inflate.hip) behind the carry; the records are walked (hgx_bam_walk.hpp,
// the open form) and decoded from their binary form (k_ext_bam_records); groups, hits and sizes are the text route's kernels, the
// text is formed from the 4-bit bases and the binary qualities (k_ext_emit<true>).  Per record the device reads: its deflated
// bytes once (inflate), 36 bytes of header per walk pass, the record once (k_ext_bam_records), and per written read its packed
// span once.  Nothing of the inflated stream travels to the host unless the chunk declines.
int hgx_bgzf_inflate_dev(const unsigned char *d_in, const hgx_bgzf_block *blocks, size_t n_blocks, unsigned char *d_out, hipStream_t st, int *bad,
                         void *staging);

static void ext_bam_drop_dev_carry(hgx_extract &h) {
    if (h.d_carry) hgx_pool_free(h.d_carry);
    h.d_carry = nullptr;
    h.carry_dev = false;
}

// The header: the leading blocks through zlib until the reference list is complete.  `next` = the first block not consumed.
static int ext_bam_header(hgx_extract &h, const std::vector<hgx_bgzf_block> &blocks, bool last, size_t &next) {
    next = 0;
    while (!h.have_hdr && next < blocks.size()) {
        const hgx_bgzf_block &b = blocks[next++];
        const size_t at = h.head.size();
        h.head.resize(at + b.out_len);
        if (!hgx_bam_inflate_block(h.comp.data(), b, h.head.data() + at)) {
            hgx_set_error("corrupt BGZF block (inflate / CRC32 / ISIZE mismatch)");
            return HGX_EPARSE;
        }
        size_t body0 = 0;
        const int st = hgx_bam_parse_header(h.head.data(), h.head.size(), h.refs, &body0);
        if (st < 0) { hgx_set_error("hgx_extract_feed_bam: the stream is no BAM (its inflated bytes do not start with BAM\\1)"); return HGX_EINVAL; }
        if (st == 0) continue;
        h.have_hdr = true;
        // per refID: the chromosome of the handle's region table, from the host map (no name lookup per record on the device)
        h.reftab.assign(h.refs.size(), -1);
        for (size_t k = 0; k < h.refs.size(); ++k) {
            const std::string &nm = h.refs[k];
            bool plain = !nm.empty();
            for (unsigned char c : nm) plain = plain && c < 0x80 && !(c == ' ' || (c >= '\t' && c <= '\r') || (c >= 0x1c && c <= 0x1f));
            const auto it = h.chrom_id.find(nm);
            h.reftab[k] = !plain ? -2 : it == h.chrom_id.end() ? -1 : it->second;
        }
        h.hcarry.assign(h.head.begin() + (ptrdiff_t)body0, h.head.end());           // the records behind the header in its block
        h.carry_n = h.hcarry.size();
        h.stream_pos = body0;
        h.head.clear();
        h.head.shrink_to_fit();
    }
    if (!h.have_hdr && last) { hgx_set_error(h.head.size() < 12 ? "truncated BAM header" : "truncated BAM reference list"); return HGX_EPARSE; }
    return HGX_OK;
}

// The host route of a BAM chunk: the carry and the chunk's blocks (inflated here) as one stream, its complete records printed by
// the reader's decoder, the text through hgx_extract_host.  Takes what the device declines and words every error.
static int ext_bam_host(hgx_extract &h, const std::vector<hgx_bgzf_block> &blocks, size_t b0, size_t total_out, bool last, int code) {
    if (h.carry_dev) {
        h.hcarry.resize(h.carry_n);
        if (h.carry_n) HIPCHK(hipMemcpy(h.hcarry.data(), (const char *)h.d_carry, h.carry_n, hipMemcpyDeviceToHost));
        ext_bam_drop_dev_carry(h);
    }
    bool counted = false;
    auto count = [&]() {                                         // the host route took (or refused) a chunk
        if (counted) return;
        counted = true;
        ++h.chunks_host;
        h.last_decline = code;
        hgx_front_set_last(0, code, 0);
    };
    std::vector<unsigned char> s;
    s.swap(h.hcarry);
    const size_t cn = s.size(), n = cn + total_out;
    s.resize(n);
    const size_t out0 = b0 < blocks.size() ? blocks[b0].out_off : 0;
    std::atomic<int> bad{0};
    hgx_par_ranges(hgx_default_threads(), blocks.size() - b0, [&](int, size_t b, size_t e) {
        for (size_t k = b0 + b; k < b0 + e; ++k)
            if (!hgx_bam_inflate_block(h.comp.data(), blocks[k], s.data() + cn + (blocks[k].out_off - out0))) bad = 1;
    });
    if (bad) { count(); hgx_set_error("corrupt BGZF block (inflate / CRC32 / ISIZE mismatch)"); return HGX_EPARSE; }
    struct Rec { size_t off; uint32_t len; };
    std::vector<Rec> recs;
    size_t q = 0;
    auto rd32 = [&](size_t p) { return (uint32_t)s[p] | ((uint32_t)s[p + 1] << 8) | ((uint32_t)s[p + 2] << 16) | ((uint32_t)s[p + 3] << 24); };
    while (q + 4 <= n) {
        const uint32_t bs = rd32(q);
        if (bs < 32) { count(); hgx_set_error("truncated BAM record at offset %zu", h.stream_pos + q); return HGX_EPARSE; }
        if (q + 4 + (size_t)bs > n) break;
        recs.push_back(Rec{q + 4, bs});
        q += 4 + (size_t)bs;
    }
    if (last && q != n) { count(); hgx_set_error("truncated BAM record at offset %zu", h.stream_pos + q); return HGX_EPARSE; }
    std::string txt;
    std::vector<uint32_t> ls, le;
    std::vector<size_t> rec_of;                                  // the record of every line (a QNAME that starts with '@' prints a header line: no record)
    for (size_t i = 0; i < recs.size(); ++i) {
        const size_t b = txt.size();
        if (!hgx_bam_record_line(s.data() + recs[i].off, recs[i].len, h.refs, txt)) { count(); hgx_set_error("malformed BAM record"); return HGX_EPARSE; }
        if (txt.size() > 0xFFFFFFF0ull) { hgx_set_error("BAM chunk too large"); return HGX_EPARSE; }
        if (txt.size() == b || txt[b] != '@') { ls.push_back((uint32_t)b); le.push_back((uint32_t)txt.size()); rec_of.push_back(i); }
        txt.push_back('\n');
    }
    size_t n_use = ls.size(), keep = q;
    if (!last && n_use > 0) {
        n_use = ext_last_group(h, txt.data(), ls, le, n_use);
        keep = recs[rec_of[n_use]].off - 4;
        // the stream's name test (process:1651-1659) looks at the second record before the first group is flushed: a first
        // chunk of one record waits for the next one
        if (h.chk_line && h.prev_name.empty() && n_use < 2) { n_use = 0; keep = 0; }
    }
    int rc = HGX_OK;
    if (n_use > 0) {
        count();
        rc = hgx_extract_host(h, txt.data(), ls.data(), le.data(), n_use);
    }
    if (rc) return rc;
    if (n - keep > EXT_MAX_BUF) { hgx_set_error("hgx_extract_feed_bam: one read's records span more than %zu bytes", EXT_MAX_BUF); return HGX_EINVAL; }
    h.hcarry.assign(s.begin() + (ptrdiff_t)keep, s.end());
    h.carry_n = h.hcarry.size();
    h.stream_pos += keep;
    return HGX_OK;
}

// The device route of a BAM chunk; *declined != 0: nothing was changed, the host route takes the chunk.
static int ext_bam_device(hgx_extract &h, const std::vector<hgx_bgzf_block> &blocks, size_t b0, size_t used,
                          size_t total_out, bool last, hipStream_t st, int *declined) {
    *declined = 0;
    if (h.n_fam > 64) { *declined = HGX_EXT_DECLINE_FAMILIES; return HGX_OK; }
    // the gate before anything touches the device: a record takes at least 36 bytes of the stream, so fewer bytes than 36 per
    // gate record cannot reach the gate (the exact count is known after the walk and gates again there)
    const bool force = hgx_switch_has("front", "device");
    if (!force && (h.carry_n + total_out) / 36 < (size_t)HGX_EXT_MIN_RECORDS) { *declined = HGX_EXT_DECLINE_SMALL; return HGX_OK; }
    for (size_t k = b0; k < blocks.size(); ++k)
        if (blocks[k].out_len > 65536) { *declined = HGX_EXT_DECLINE_INFLATE; return HGX_OK; }
    RCHK(ext_upload_table(h));
    if (!h.d_reftab && !upload_array(h.d_reftab, h.reftab.data(), h.reftab.size() * 4)) {
        hgx_set_error("extract route: upload of the reference table failed: %s", hipGetErrorString(hipGetLastError()));
        return HGX_EHIP;
    }
    const size_t cn = h.carry_n, n = cn + total_out;
    if (n == 0) return HGX_OK;
    // the stream lies behind `lead` bytes so that its inflated part starts on a 64-byte boundary and the aligned loads of the walk
    // and of the emit kernel may reach below its first byte; 1 KB of zeros behind it
    const size_t lead = 64 + ((64 - (cn & 63)) & 63), pad = 1024;
    if (lead + n + pad >= (1ull << 32)) { *declined = HGX_EXT_DECLINE_SIZE; return HGX_OK; }
    struct Hold { void *p; ~Hold() { if (p) hgx_pool_free(p); } } hold{hgx_pool_alloc(lead + n + pad)};
    if (!hold.p) { hgx_set_error("extract route: device allocation of %zu bytes failed", lead + n + pad); return HGX_ENOMEM; }
    char *d_text = (char *)hold.p;
    DevBufs m("extract route");
    long long up = 0;
    HIPCHK(hipMemsetAsync(d_text, 0, lead, st));
    HIPCHK(hipMemsetAsync(d_text + lead + n, 0, pad, st));
    if (cn) {
        if (h.carry_dev) HIPCHK(hipMemcpyAsync(d_text + lead, (const char *)h.d_carry, cn, hipMemcpyDeviceToDevice, st));
        else { HIPCHK(hipMemcpyAsync(d_text + lead, h.hcarry.data(), cn, hipMemcpyHostToDevice, st)); up += (long long)cn; }
    }
    if (b0 < blocks.size()) {
        const size_t c0 = blocks[b0].in_off, cb = used - c0, out0 = blocks[b0].out_off;     // (from the first block's deflate data on)
        std::vector<hgx_bgzf_block> rel(blocks.begin() + (ptrdiff_t)b0, blocks.end());
        for (hgx_bgzf_block &b : rel) { b.in_off -= c0; b.out_off -= out0; }
        unsigned char *d_comp;
        RCHK(m.get(d_comp, cb + 2048));
        HIPCHK(hipMemcpyAsync(d_comp, h.comp.data() + c0, cb, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemsetAsync(d_comp + cb, 0, 2048, st));
        int bad = 0;
        RCHK(hgx_bgzf_inflate_dev(d_comp, rel.data(), rel.size(), (unsigned char *)d_text + lead + cn, st, &bad, nullptr));
        if (bad) { *declined = HGX_EXT_DECLINE_INFLATE; return HGX_OK; }
        up += (long long)cb + 20ll * (long long)rel.size();
    }
    // the record chain, from the known chain position (the stream's first byte)
    const int W = (int)std::min<size_t>((size_t)1 << 20, n / 8192 + 1);
    BamSeg seg{};
    seg.base = (uint32_t)lead; seg.n = (uint32_t)n; seg.body0 = 0; seg.n_ref = (int32_t)h.refs.size(); seg.first_range = 0; seg.n_ranges = (uint32_t)W;
    BamSeg *d_seg;
    BamRange *d_rng;
    BamCtl *d_ctl;
    uint32_t *d_cnt, *d_base;
    char *d_wscan;
    RCHK(m.get(d_seg, 1)); RCHK(m.get(d_rng, W)); RCHK(m.get(d_ctl, 1)); RCHK(m.get(d_cnt, W + 4)); RCHK(m.get(d_base, W + 4));
    RCHK(m.get(d_wscan, hgx_scan_u32_scratch_bytes(W)));
    HIPCHK(hipMemsetAsync(d_ctl, 0, sizeof(BamCtl), st));
    HIPCHK(hipMemcpyAsync(d_seg, &seg, sizeof seg, hipMemcpyHostToDevice, st));
    const unsigned char *u_text = (const unsigned char *)d_text;
    hipLaunchKernelGGL((k_bam_walk<0, true>), dim3(nblk(W, 64)), dim3(64), 0, st, u_text, d_seg, 1, W, d_rng, (const uint32_t *)nullptr,
                       (uint32_t *)nullptr, (uint32_t *)nullptr, (uint16_t *)nullptr);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_bam_link_open, dim3(nblk(W, 256)), dim3(256), 0, st, u_text, d_rng, d_seg, 1, W, d_cnt, d_ctl);
    HIPCHK(hipGetLastError());
    RCHK(hgx_scan_u32_dev(d_cnt, d_base, W, d_wscan, d_ctl->tot, st));
    BamCtl ctl;
    HIPCHK(hipMemcpyAsync(&ctl, d_ctl, sizeof ctl, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (ctl.decline) { *declined = HGX_EXT_DECLINE_CHAIN; return HGX_OK; }
    const long N = (long)ctl.tot[0];
    const size_t end = ctl.end;                                          // the first incomplete record (offset in the stream)
    if (last && end != n) { hgx_set_error("truncated BAM record at offset %zu", h.stream_pos + end); return HGX_EPARSE; }
    if (N > 0 && !force && N < HGX_EXT_MIN_RECORDS) { *declined = HGX_EXT_DECLINE_SMALL; return HGX_OK; }
    uint32_t n_proc = 0, g_first = 0;
    uint32_t *d_off = nullptr;
    if (N > 0) {
        uint32_t *d_len;
        uint16_t *d_task;
        ExtWork w;
        RCHK(m.get(d_off, N)); RCHK(m.get(d_len, N)); RCHK(m.get(d_task, N + 8));
        RCHK(ext_work_alloc(m, w, N, st));
        hipLaunchKernelGGL((k_bam_walk<1, true>), dim3(nblk(W, 64)), dim3(64), 0, st, u_text, d_seg, 1, W, d_rng, (const uint32_t *)d_base, d_off, d_len, d_task);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(k_ext_bam_records, dim3(nblk(N, 256)), dim3(256), 0, st, u_text, d_off, d_len, N, h.d_reftab, (int)h.refs.size(), h.d_creg,
                           h.d_rfam, h.d_rl, h.d_rr, h.simulation, w.R, w.d_dec);
        HIPCHK(hipGetLastError());
        // a record's name, copied back (the first two for the stream's name test, one per chunk for prev_name)
        auto name_of = [&](uint32_t rec, std::string &name) -> int {
            uint32_t off = 0;
            unsigned char buf[32 + 256];
            HIPCHK(hipMemcpyAsync(&off, d_off + rec, 4, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            HIPCHK(hipMemcpyAsync(buf, d_text + off, sizeof buf, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            name.assign((const char *)buf + 32, buf[8] ? (size_t)buf[8] - 1 : 0);
            return HGX_OK;
        };
        auto chk = [&](uint32_t np, int *code) -> int {
            if (!h.chk_line || np == 0) return HGX_OK;
            std::string txt, nm;
            std::vector<uint32_t> ls, le;
            for (uint32_t k = 0; k < 2 && k < (uint32_t)N; ++k) {
                RCHK(name_of(k, nm));
                ls.push_back((uint32_t)txt.size());
                txt += nm;
                le.push_back((uint32_t)txt.size());
                txt.push_back('\n');
            }
            if (!hgx_extract_chk(h, txt.data(), ls.data(), le.data(), (size_t)N)) *code = HGX_EXT_DECLINE_NAMES;
            return HGX_OK;
        };
        RCHK((ext_groups_emit<true>(h, m, d_text, w, N, st, declined, !last, chk, &n_proc, &g_first)));
        if (*declined) return HGX_OK;
        if (n_proc > 0) {
            RCHK(name_of(g_first, h.prev_name));
            h.chk_line = false;
            h.n_records += (int64_t)n_proc;
            ++h.chunks_dev;
        }
    }
    h.up_bytes += up;
    hgx_front_set_last(2, 0, up);                                        // (also a chunk that only grew the carry)
    // the carry: from the first record not taken on (with `last` the stream has ended on a record boundary: nothing)
    size_t keep = n;
    if (!last) {
        keep = end;
        if (n_proc < (uint32_t)N) {
            uint32_t off = 0;
            HIPCHK(hipMemcpyAsync(&off, d_off + n_proc, 4, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            keep = (size_t)off - 4 - lead;
        }
    }
    const size_t new_n = n - keep;
    if (new_n > EXT_MAX_BUF) { hgx_set_error("hgx_extract_feed_bam: one read's records span more than %zu bytes", EXT_MAX_BUF); return HGX_EINVAL; }
    void *nc = nullptr;
    if (new_n) {
        nc = hgx_pool_alloc(new_n + 64);
        if (!nc) { hgx_set_error("extract route: device allocation of %zu bytes failed", new_n + 64); return HGX_ENOMEM; }
        const hipError_t e = hipMemcpyAsync(nc, d_text + lead + keep, new_n, hipMemcpyDeviceToDevice, st);
        const hipError_t e2 = e == hipSuccess ? hipStreamSynchronize(st) : e;
        if (e2 != hipSuccess) { hgx_pool_free(nc); hgx_set_error("extract route: %s", hipGetErrorString(e2)); return HGX_EHIP; }
    }
    ext_bam_drop_dev_carry(h);
    h.hcarry.clear();
    h.d_carry = nc;
    h.carry_dev = nc != nullptr;
    h.carry_n = new_n;
    h.stream_pos += keep;
    return HGX_OK;
}

// h.comp holds the undigested bytes and the new ones: run every complete block, keep the rest.
static int ext_bam_run(hgx_extract &h, bool last, hipStream_t st) {
    // the complete blocks at the head of h.comp (in_off within h.comp, out_off from 0); a partial one waits for the next feed
    std::vector<hgx_bgzf_block> blocks;
    size_t used = 0, b0 = 0;
    RCHK(hgx_bgzf_scan_stream(h.comp.data(), h.comp.size(), last, h.comp_pos, blocks, nullptr, &used));
    if (!h.have_hdr) RCHK(ext_bam_header(h, blocks, last, b0));
    if (h.have_hdr && (b0 < blocks.size() || last)) {
        size_t total_out = 0;
        for (size_t k = b0; k < blocks.size(); ++k) total_out += blocks[k].out_len;
        int declined = hgx_switch_has("front", "host") ? HGX_EXT_DECLINE_FORCED : 0;
        if (!declined) {
            const int rc = ext_bam_device(h, blocks, b0, used, total_out, last, st, &declined);
            if (rc) { hgx_front_set_last(0, 0, 0); return rc; }
        }
        if (declined) RCHK(ext_bam_host(h, blocks, b0, total_out, last, declined));
    }
    h.comp.erase(h.comp.begin(), h.comp.begin() + (ptrdiff_t)used);
    h.comp_pos += used;
    return HGX_OK;
}

extern "C" int hgx_extract_open(hgx_extract **out, int32_t n_regions, const int32_t *family, const char *chrom_pool, size_t chrom_bytes,
                                const int64_t *left, const int64_t *right, int32_t n_families, const hgx_extract_opts *opts) {
    ARGCHK(out && opts && n_regions >= 0 && n_families >= 0 && (n_regions == 0 || (family && chrom_pool && left && right)));
    std::unique_ptr<hgx_extract> h(new hgx_extract());
    h->aligner = opts->aligner; h->paired = opts->paired != 0; h->simulation = opts->simulation != 0; h->fastq = opts->fastq != 0;
    h->n_fam = n_families;
    std::vector<int32_t> rc(n_regions);
    size_t p = 0;
    for (int32_t r = 0; r < n_regions; ++r) {
        const char *z = p < chrom_bytes ? (const char *)memchr(chrom_pool + p, 0, chrom_bytes - p) : nullptr;
        if (!z || family[r] < 0 || family[r] >= n_families) {
            hgx_set_error("invalid argument: region %d has no chromosome name or a family outside [0, %d)", r, n_families);
            return HGX_EINVAL;
        }
        const std::string c(chrom_pool + p, (size_t)(z - (chrom_pool + p)));
        p += c.size() + 1;
        auto it = h->chrom_id.find(c);
        if (it == h->chrom_id.end()) { it = h->chrom_id.emplace(c, (int32_t)h->chrom.size()).first; h->chrom.push_back(c); }
        rc[r] = it->second;
    }
    h->creg_off.assign(h->chrom.size() + 1, 0);
    for (int32_t r = 0; r < n_regions; ++r) ++h->creg_off[rc[r] + 1];
    for (size_t c = 0; c < h->chrom.size(); ++c) h->creg_off[c + 1] += h->creg_off[c];
    std::vector<uint32_t> at(h->creg_off.begin(), h->creg_off.end() - 1);
    h->reg_fam.resize(n_regions); h->reg_left.resize(n_regions); h->reg_right.resize(n_regions);
    for (int32_t r = 0; r < n_regions; ++r) {            // stable: .locus order inside a chromosome
        const uint32_t x = at[rc[r]]++;
        h->reg_fam[x] = family[r]; h->reg_left[x] = left[r]; h->reg_right[x] = right[r];
    }
    h->written.assign(n_families, 0);
    h->out.assign((size_t)2 * n_families, std::string());
    h->taken.assign((size_t)2 * n_families, std::string());
    *out = h.release();
    return HGX_OK;
}

extern "C" int hgx_extract_feed(hgx_extract *h, const char *bytes, size_t n_bytes, int32_t last, void *stream) {
    ARGCHK(h && (bytes || n_bytes == 0));
    if (h->error_kind) { hgx_set_error("hgx_extract_feed: the stream has already raised"); return HGX_EPARSE; }
    if (h->finished) { hgx_set_error("hgx_extract_feed: the stream was closed by an earlier last feed"); return HGX_EINVAL; }
    if (h->mode == 2) { hgx_set_error("hgx_extract_feed: the handle was fed BAM bytes (hgx_extract_feed_bam); a stream is text or BAM, not both"); return HGX_EINVAL; }
    h->mode = 1;
    const size_t piece = hgx_test_switch("extract_piece") ? (size_t)atol(hgx_test_switch("extract_piece")) : ((size_t)256 << 20);
    size_t p = 0;
    do {
        const size_t take = std::min(std::max<size_t>(piece, 1), n_bytes - p);
        if (h->buf.size() + take > EXT_MAX_BUF) {
            hgx_set_error("hgx_extract_feed: one read's records span more than %zu bytes", EXT_MAX_BUF);
            return HGX_EINVAL;
        }
        h->buf.insert(h->buf.end(), bytes + p, bytes + p + take);
        p += take;
        const bool fin = last && p == n_bytes;
        RCHK(ext_run(*h, fin, (hipStream_t)stream));
        if (fin) h->finished = true;
    } while (p < n_bytes);
    return HGX_OK;
}


constexpr size_t EXT_BAM_PIECE = (size_t)64 << 20;       // deflated bytes per chunk
static size_t ext_bam_piece() {
    const char *sw = hgx_test_switch("extract_bam_piece");
    return std::max<size_t>(sw ? (size_t)atol(sw) : EXT_BAM_PIECE, 1);
}

extern "C" int hgx_extract_feed_bam(hgx_extract *h, const void *bgzf, size_t n_bytes, int32_t last, void *stream) {
    ARGCHK(h && (bgzf || n_bytes == 0));
    if (h->error_kind) { hgx_set_error("hgx_extract_feed_bam: the stream has already raised"); return HGX_EPARSE; }
    if (h->finished) { hgx_set_error("hgx_extract_feed_bam: the stream was closed by an earlier last feed"); return HGX_EINVAL; }
    if (h->mode == 1) { hgx_set_error("hgx_extract_feed_bam: the handle was fed text (hgx_extract_feed); a stream is text or BAM, not both"); return HGX_EINVAL; }
    h->mode = 2;
    const size_t piece = ext_bam_piece();
    const unsigned char *bytes = (const unsigned char *)bgzf;
    size_t p = 0;
    do {
        const size_t take = std::min(piece, n_bytes - p);
        h->comp.insert(h->comp.end(), bytes + p, bytes + p + take);
        p += take;
        const bool fin = last && p == n_bytes;
        RCHK(ext_bam_run(*h, fin, (hipStream_t)stream));
        if (fin) h->finished = true;
    } while (p < n_bytes);
    return HGX_OK;
}

// true: the file's first BGZF block inflates to a BAM header's magic (a bgzipped SAM text, or anything else, goes the text way)
static bool ext_file_is_bam(FILE *f) {
    std::vector<unsigned char> d((size_t)1 << 16);
    rewind(f);
    const size_t n = fread(d.data(), 1, d.size(), f);
    if (n < 18 || d[0] != 0x1f || d[1] != 0x8b || d[2] != 8 || !(d[3] & 4)) return false;
    const size_t xlen = (size_t)d[10] | ((size_t)d[11] << 8);
    size_t blen = 0;
    for (size_t q = 12; q + 6 <= 12 + xlen && q + 6 <= n;) {
        const size_t slen = (size_t)d[q + 2] | ((size_t)d[q + 3] << 8);
        if (d[q] == 66 && d[q + 1] == 67 && slen == 2) blen = ((size_t)d[q + 4] | ((size_t)d[q + 5] << 8)) + 1;
        q += 4 + slen;
    }
    if (!blen || blen > n || blen < 12 + xlen + 8) return false;
    hgx_bgzf_block b;
    b.in_off = 12 + xlen; b.in_len = blen - 12 - xlen - 8; b.out_off = 0;
    b.crc = (uint32_t)d[blen - 8] | ((uint32_t)d[blen - 7] << 8) | ((uint32_t)d[blen - 6] << 16) | ((uint32_t)d[blen - 5] << 24);
    b.out_len = (uint32_t)d[blen - 4] | ((uint32_t)d[blen - 3] << 8) | ((uint32_t)d[blen - 2] << 16) | ((uint32_t)d[blen - 1] << 24);
    if (b.out_len < 4 || b.out_len > 65536) return false;
    std::vector<unsigned char> out(b.out_len);
    return hgx_bam_inflate_block(d.data(), b, out.data()) && memcmp(out.data(), "BAM\1", 4) == 0;
}

extern "C" int hgx_extract_file(hgx_extract *h, const char *path, void *stream) {
    ARGCHK(h && path);
    FILE *f = fopen(path, "rb");
    if (!f) { hgx_set_error("hgx_extract_file: cannot open %s", path); return HGX_EINVAL; }
    unsigned char magic[4] = {0, 0, 0, 0};
    const size_t got = fread(magic, 1, 4, f);
    if (got >= 2 && magic[0] == 0x1f && magic[1] == 0x8b && ext_file_is_bam(f)) {
        // BAM: the file's deflated bytes, block after block; the handle inflates them and reads the records in their binary form
        rewind(f);
        std::vector<unsigned char> blk(ext_bam_piece());
        int rc = HGX_OK;
        for (;;) {
            const size_t n = fread(blk.data(), 1, blk.size(), f);
            const bool fin = n < blk.size();
            rc = hgx_extract_feed_bam(h, blk.data(), n, fin ? 1 : 0, stream);
            if (rc || fin) break;
        }
        fclose(f);
        return rc;
    }
    if (got >= 2 && magic[0] == 0x1f && magic[1] == 0x8b) {
        // any other BGZF / gzip file (a bgzipped SAM text): the reader inflates it in one piece; its lines, in file order, are
        // the stream
        fclose(f);
        std::vector<char> text;
        size_t tot;
        RCHK(bam_as_sam_text(path, nullptr, EXT_MAX_BUF, text, tot));
        if (tot > EXT_MAX_BUF) {
            hgx_set_error("hgx_extract_file: %s holds %zu bytes of records; a compressed text is read in one piece of at most %zu (feed it as SAM text)",
                          path, tot, EXT_MAX_BUF);
            return HGX_EINVAL;
        }
        return hgx_extract_feed(h, text.data(), text.size(), 1, stream);
    }
    rewind(f);
    std::vector<char> blk((size_t)64 << 20);
    int rc = HGX_OK;
    for (;;) {
        const size_t n = fread(blk.data(), 1, blk.size(), f);
        const bool fin = n < blk.size();
        rc = hgx_extract_feed(h, blk.data(), n, fin ? 1 : 0, stream);
        if (rc || fin) break;
    }
    fclose(f);
    return rc;
}

extern "C" int hgx_extract_keep(hgx_extract *h, int32_t keep) {
    ARGCHK(h);
    if (h->mode != 0 || h->finished) { hgx_set_error("hgx_extract_keep: the handle has been fed already"); return HGX_EINVAL; }
    h->keep = keep != 0;
    h->segs.assign(h->keep ? h->out.size() : 0, std::vector<hgx_keep_seg>());
    return HGX_OK;
}

extern "C" int hgx_extract_take_reads(hgx_extract *h, int32_t family, hgx_reads **out) {
    ARGCHK(h && out && family >= 0 && family < h->n_fam);
    *out = nullptr;
    if (!h->keep) { hgx_set_error("hgx_extract_take_reads: the handle does not keep its text (hgx_extract_keep)"); return HGX_EINVAL; }
    hipStream_t st = nullptr;
    ext_keep_flush(*h);
    const int ni = h->paired ? 2 : 1;
    std::unique_ptr<hgx_reads> r(new hgx_reads);
    r->n_inputs = ni;
    hgx_keep_plan plan;
    int bad = 0;
    size_t bad_bytes = 0;
    if (!hgx_keep_layout(h->segs, family, ni, plan, &bad, &bad_bytes)) {
        hgx_set_error("hgx_extract_take_reads: %zu bytes or more of reads for one family and mate %d (take them more often: below 2 GB)",
                      bad_bytes, bad + 1);
        return HGX_EINVAL;
    }
    for (int i = 0; i < ni; ++i) { r->in_off[i] = plan.in_off[i]; r->in_bytes[i] = plan.in_bytes[i]; }
    r->text_bytes = plan.text_bytes;
    r->d_text = hgx_pool_alloc(plan.text_bytes + 64);        // (the object frees it, however this call ends)
    if (!r->d_text) { hgx_set_error("device allocation of %zu bytes failed", plan.text_bytes + 64); return HGX_ENOMEM; }
    char *d = (char *)r->d_text;
    hgx_keep_copy copy;
    copy.from_dev = [&](size_t at, const void *dev, size_t n) -> int { HIPCHK(hipMemcpyAsync(d + at, dev, n, hipMemcpyDeviceToDevice, st)); return HGX_OK; };
    copy.from_host = [&](size_t at, const char *host, size_t n) -> int { HIPCHK(hipMemcpyAsync(d + at, host, n, hipMemcpyHostToDevice, st)); return HGX_OK; };
    copy.zero = [&](size_t at, size_t n) -> int { HIPCHK(hipMemsetAsync(d + at, 0, n, st)); return HGX_OK; };
    RCHK(hgx_keep_join(h->segs, family, ni, plan, copy));
    HIPCHK(hipStreamSynchronize(st));
    // the table where the text lies; the gate does not apply (nothing is left to upload), front=host still sends it to the loader
    if (hgx_switch_has("front", "host")) r->decline = HGX_RD_DECLINE_SWITCH;
    else RCHK(hgx_reads_table_dev(r.get(), h->fastq, st));
    if (r->decline) {                                        // the text copied down once, the table by the host loader
        std::vector<std::string> text(ni);
        for (int i = 0; i < ni; ++i) {
            text[i].resize(r->in_bytes[i]);
            if (r->in_bytes[i]) RCHK(hgx_reads_text_to_host(r.get(), r->in_off[i], r->in_bytes[i], &text[i][0]));
        }
        hgx_reads_dev_free(r.get());
        RCHK(hgx_reads_host_table(r.get(), text, h->fastq, r->decline));
    }
    // the object is complete: only now are the family's segments given up (a failure above leaves them for another call)
    for (int i = 0; i < ni; ++i) ext_keep_drop(*h, (size_t)(2 * family + i));
    hgx_reads_set_last(r.get());
    *out = r.release();
    return HGX_OK;
}

extern "C" int hgx_extract_take(hgx_extract *h, int32_t family, int32_t mate, const char **text, size_t *n_bytes) {
    ARGCHK(h && text && n_bytes && family >= 0 && family < h->n_fam && (mate == 0 || mate == 1));
    if (h->keep) { hgx_set_error("hgx_extract_take: the handle keeps its text in HBM (hgx_extract_take_reads)"); return HGX_EINVAL; }
    std::string &t = h->taken[2 * family + mate];
    t.clear();
    t.swap(h->out[2 * family + mate]);
    *text = t.data();
    *n_bytes = t.size();
    return HGX_OK;
}

extern "C" int hgx_extract_stats(const hgx_extract *h, int64_t *records, int64_t *groups, int64_t *written, int32_t *route, int32_t *decline,
                                 int32_t *error_kind, int64_t *chunks_device, int64_t *chunks_host) {
    ARGCHK(h);
    if (records) *records = h->n_records;
    if (groups) *groups = h->n_groups;
    if (written) for (int f = 0; f < h->n_fam; ++f) written[f] = h->written[f];
    if (route) *route = (h->chunks_dev > 0 && h->chunks_host == 0) ? 2 : 0;
    if (decline) *decline = h->last_decline;
    if (error_kind) *error_kind = h->error_kind;
    if (chunks_device) *chunks_device = h->chunks_dev;
    if (chunks_host) *chunks_host = h->chunks_host;
    return HGX_OK;
}

extern "C" int hgx_extract_close(hgx_extract *h) {
    if (!h) return HGX_OK;
    ext_free_table(*h);
    ext_bam_drop_dev_carry(*h);
    for (size_t k = 0; k < h->segs.size(); ++k) ext_keep_drop(*h, k);
    delete h;
    return HGX_OK;
}

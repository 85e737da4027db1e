// hgx_align_linear_core.hpp -- the "hgx" aligner on a LINEAR index: what the kernels (hgx_align_linear.hip) and the
// host route (hgx_align_linear_host.cpp) both run.  The rule is stated in plain Python in tests/align_linear_ref.py.
//
// The index is the family's allele sequences, concatenated.  A read is aligned ungapped and end to end with at most max_edits
// mismatches; up to k hits per read are written, ordered by (NM, allele, pos0, strand).  Candidates come from the read's first
// min(max_edits + 1, L / 16) disjoint 16-mers through a seed table (16-mer code -> the (allele, position) pairs that hold it, a
// sorted CSR); a candidate is verified with XOR and popcount over three bit planes (low bit, high bit, non-ACGT mask) of 64 bases
// per word, and is TAKEN only from the first of the read's seeds that matches exactly at it, so no hit is found twice.
// Plain C++ (HGX_ALN_HD marks what the kernels call); no state, no atomics.
#pragma once
#include <stdint.h>

#include "hgx_align_core.hpp"          // HGX_ALN_HD, hgx_aln_read, hgx_aln_code2, hgx_aln_out

#if defined(__HIPCC__)
#define HGX_ALNL_UNROLL _Pragma("unroll")
#else
#define HGX_ALNL_UNROLL
#endif

#define HGX_ALNL_K 16
#define HGX_ALNL_MAX_EDITS 4           // hgx_align_linear_opts.max_edits
#define HGX_ALNL_MAX_K 1024            // hgx_align_linear_opts.k
#define HGX_ALNL_MAX_SEEDS (HGX_ALNL_MAX_EDITS + 1)
#define HGX_ALNL_HOST_WORDS (HGX_ALN_MAX_READ / 64)          // plane words of the longest read the host route takes (1 024 bases)
#define HGX_ALNL_DEV_MAX_READ HGX_ALN_DEV_MAX_READ           // the longest read the kernels take (256 bases)
#define HGX_ALNL_DEV_WORDS (HGX_ALNL_DEV_MAX_READ / 64)
#define HGX_ALNL_PLANE_PAD (HGX_ALNL_HOST_WORDS + 1)        // zero words behind the planes: a window's loads stay inside
// the 64-bit key (read | NM | allele | pos0 | strand): 20 + 3 + 20 + 20 + 1 bits
#define HGX_ALNL_READ_BITS 20          // reads of one chunk
#define HGX_ALNL_ALLELE_BITS 20        // alleles of an index (hgx_align_linear_index_create refuses more)
#define HGX_ALNL_POS_BITS 20           // bases of one allele (refused likewise)
#define HGX_ALNL_LINE_MAX 4000         // bytes of one record on the kernels' route (a longer one declines): 2^20 records stay below 2^32 bytes

// route = auto takes the kernels from reads x alleles >= this: the measured break-even (6 400 .. 13 000 on MI355X at 100, 1 000 and
// 7 000 alleles) rounded up to a power of two.  The host route costs 40 .. 90 ns per (read, allele), a call of the
// kernels' route ~0.5 ms before its first read
#define HGX_ALNL_GATE 16384

// why the kernels did not give the bytes (hgx_align_linear_last); the host route gave them then
#define HGX_ALNL_DECLINE_NONE 0
#define HGX_ALNL_DECLINE_GATE 1        // route = auto with reads x alleles < HGX_ALNL_GATE
#define HGX_ALNL_DECLINE_READ_LEN 2    // a read longer than HGX_ALNL_DEV_MAX_READ
#define HGX_ALNL_DECLINE_BUDGET 3      // the candidates of one read (one pair, for paired input) alone pass the chunk's budget
#define HGX_ALNL_DECLINE_LINE 4        // a record longer than HGX_ALNL_LINE_MAX bytes (a very long read name)
#define HGX_ALNL_DECLINE_SWITCH 7      // route = host, or the test switch front=host

struct hgx_alnl_view {
    const char *text;                  // the alleles' bases, upper case, concatenated in index order
    const int32_t *off;                // [n_alleles + 1] into text
    int32_t n_alleles;
    const uint64_t *lo, *hi, *mask;    // bit planes over `text` (bit i of word w = base 64 w + i) + HGX_ALNL_PLANE_PAD zero words
    const uint32_t *keys;              // the distinct 16-mer codes, ascending
    int32_t n_keys;
    const uint32_t *koff;              // [n_keys + 1]: a code's entries
    const int32_t *kal, *kpos;         // per entry: allele and position in it; ascending (allele, position) within a code
    const int32_t *name_off, *name_len;
    const char *pool;
};

// an oriented read as bit planes: W words of 64 bases, zero behind the read
template <int W> struct hgx_alnl_planes { uint64_t lo[W], hi[W], mask[W]; };

template <int W> HGX_ALN_HD inline void hgx_alnl_pack(const hgx_aln_read &R, hgx_alnl_planes<W> &p) {
    for (int w = 0; w < W; ++w) p.lo[w] = p.hi[w] = p.mask[w] = 0;
    for (int r = 0; r < R.L; ++r) {
        const int c = hgx_aln_code2(R.at(r));
        const uint64_t bit = 1ull << (r & 63);
        if (c < 0) p.mask[r >> 6] |= bit;
        else {
            if (c & 1) p.lo[r >> 6] |= bit;
            if (c & 2) p.hi[r >> 6] |= bit;
        }
    }
}

HGX_ALN_HD inline int hgx_alnl_n_seeds(int L, int max_edits) {
    const int n = L / HGX_ALNL_K;
    return n < max_edits + 1 ? n : max_edits + 1;
}
// the 16 bits at base `at` of a plane that starts at `p`
HGX_ALN_HD inline uint32_t hgx_alnl_bits16(const uint64_t *p, long at) {
    const long q = at >> 6;
    const int s = (int)(at & 63);
    uint64_t v = p[q] >> s;
    if (s > 48) v |= p[q + 1] << (64 - s);
    return (uint32_t)(v & 0xffffu);
}
// the code of the 16-mer at base `at` of (lo, hi, mask), false if it holds a base outside ACGT
HGX_ALN_HD inline bool hgx_alnl_code(const uint64_t *lo, const uint64_t *hi, const uint64_t *mask, long at, uint32_t *code) {
    if (hgx_alnl_bits16(mask, at)) return false;
    *code = (hgx_alnl_bits16(hi, at) << 16) | hgx_alnl_bits16(lo, at);
    return true;
}
// the entries [*b0, *b1) of `code` in the seed table (empty if it is not there); n_keys halvings
HGX_ALN_HD inline void hgx_alnl_bucket(const hgx_alnl_view &V, uint32_t code, uint32_t *b0, uint32_t *b1) {
    int32_t lo = 0, hi = V.n_keys;
    while (lo < hi) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (V.keys[mid] < code) lo = mid + 1;
        else hi = mid;
    }
    if (lo < V.n_keys && V.keys[lo] == code) { *b0 = V.koff[lo]; *b1 = V.koff[lo + 1]; }
    else *b0 = *b1 = 0;
}

// Hamming distance of the oriented read and the L bases at P of the text; mm[0 .. ceil(L / 64)) = the mismatching bases, a bit each.
// On the device the loop is unrolled over the W words, so that its indices are constants and mm[] stays in registers; it ends
// behind the read's last word on either route
template <int W> HGX_ALN_HD inline int hgx_alnl_mismatches(const hgx_alnl_view &V, long P, const hgx_alnl_planes<W> &rp, int L, uint64_t *mm) {
    const int nw = (L + 63) >> 6, s = (int)(P & 63);
    const long q = P >> 6;
    int nm = 0;
    HGX_ALNL_UNROLL
    for (int j = 0; j < W; ++j) {
        if (j >= nw) break;
        uint64_t alo = V.lo[q + j] >> s, ahi = V.hi[q + j] >> s, am = V.mask[q + j] >> s;
        if (s) {
            alo |= V.lo[q + j + 1] << (64 - s);
            ahi |= V.hi[q + j + 1] << (64 - s);
            am |= V.mask[q + j + 1] << (64 - s);
        }
        uint64_t x = (alo ^ rp.lo[j]) | (ahi ^ rp.hi[j]) | am | rp.mask[j];
        if (j == nw - 1 && (L & 63)) x &= (1ull << (L & 63)) - 1;
        mm[j] = x;
        nm += __builtin_popcountll(x);
    }
    return nm;
}

// the candidate "seed j of the read stands at position p of allele a": true if it is a hit AND no earlier seed of the read matches
// exactly at its place (that seed's bucket holds the same hit)
template <int W>
HGX_ALN_HD inline bool hgx_alnl_candidate(const hgx_alnl_view &V, const hgx_alnl_planes<W> &rp, int L, int j, int32_t a, int32_t p, int max_edits,
                                          int32_t *pos0_out, int *nm_out) {
    static_assert(W * 64 >= HGX_ALNL_MAX_SEEDS * HGX_ALNL_K, "the seeds lie in the planes");
    const int32_t pos0 = p - j * HGX_ALNL_K, len = V.off[a + 1] - V.off[a];
    if (pos0 < 0 || pos0 > len - L) return false;
    uint64_t mm[W];
    const int nm = hgx_alnl_mismatches<W>(V, (long)V.off[a] + pos0, rp, L, mm);
    if (nm > max_edits) return false;
    HGX_ALNL_UNROLL
    for (int e = 0; e < HGX_ALNL_MAX_SEEDS - 1; ++e) {          // (seed e < j lies inside the read: its word of mm[] is set)
        if (e >= j) break;
        if (((mm[(e * HGX_ALNL_K) >> 6] >> ((e * HGX_ALNL_K) & 63)) & 0xffffu) == 0) return false;
    }
    *pos0_out = pos0;
    *nm_out = nm;
    return true;
}

HGX_ALN_HD inline uint64_t hgx_alnl_key(uint32_t read, int nm, int32_t a, int32_t pos0, int strand) {
    return ((uint64_t)read << 44) | ((uint64_t)nm << 41) | ((uint64_t)(uint32_t)a << 21) | ((uint64_t)(uint32_t)pos0 << 1) | (uint64_t)strand;
}
HGX_ALN_HD inline uint32_t hgx_alnl_key_read(uint64_t k) { return (uint32_t)(k >> 44); }
HGX_ALN_HD inline int hgx_alnl_key_nm(uint64_t k) { return (int)((k >> 41) & 7); }
HGX_ALN_HD inline int32_t hgx_alnl_key_allele(uint64_t k) { return (int32_t)((k >> 21) & 0xfffff); }
HGX_ALN_HD inline int32_t hgx_alnl_key_pos0(uint64_t k) { return (int32_t)((k >> 1) & 0xfffff); }
HGX_ALN_HD inline int hgx_alnl_key_strand(uint64_t k) { return (int)(k & 1); }

// the record of the hit `key`, with its '\n': the read's record number `rank` of n_written, of a read with n_hits hits.  mate_no < 0:
// single-end input; else the mate's number and whether the OTHER mate wrote a record.  RNEXT *, PNEXT 0, TLEN 0 on purpose: the linear
// typing reads none of them and the mates are placed independently.  qual == nullptr (FASTA): 'I' x L, as hgx_aln_line writes it.
HGX_ALN_HD inline void hgx_alnl_line(const hgx_alnl_view &V, const char *name, int name_len, const char *seq, const char *qual, int L, uint64_t key,
                                     int rank, int n_written, int n_hits, int mate_no, bool mate_wrote, hgx_aln_out &out) {
    const int strand = hgx_alnl_key_strand(key), nm = hgx_alnl_key_nm(key);
    const int32_t a = hgx_alnl_key_allele(key), pos0 = hgx_alnl_key_pos0(key);
    const hgx_aln_read R{seq, L, strand};
    int flag = strand ? 0x10 : 0;
    if (mate_no >= 0) flag |= 0x1 | (mate_no == 0 ? 0x40 : 0x80) | (mate_wrote ? 0 : 0x8);
    if (rank) flag |= 0x100;
    out.str(name, name_len); out.ch('\t');
    out.num(flag); out.ch('\t');
    out.str(V.pool + V.name_off[a], V.name_len[a]); out.ch('\t');
    out.num(pos0 + 1); out.ch('\t');
    out.num(n_hits == 1 ? 60 : 1); out.ch('\t');
    out.num(L); out.str("M\t*\t0\t0\t", 8);
    for (int r = 0; r < L; ++r) out.ch(R.at(r));
    out.ch('\t');
    for (int r = 0; r < L; ++r) out.ch(qual ? qual[strand ? L - 1 - r : r] : 'I');
    out.str("\tAS:i:", 6); out.num(-6 * nm);
    out.str("\tNM:i:", 6); out.num(nm);
    out.str("\tMD:Z:", 6);
    const char *w = V.text + V.off[a] + pos0;
    int run = 0;
    for (int r = 0; r < L; ++r) {
        const char c = R.at(r);
        if (c == w[r] && hgx_aln_code2(c) >= 0) ++run;
        else { out.num(run); out.ch(w[r]); run = 0; }
    }
    out.num(run);
    out.str("\tNH:i:", 6); out.num(n_written);
    out.ch('\n');
}

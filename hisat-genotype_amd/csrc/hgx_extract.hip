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
#include <memory>
#include <vector>

#include "hgx_common.hpp"
#include "hgx_internal.hpp"
#include "hgx_extract.hpp"
#include "hgx_records.hpp"

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
    const bool rev = (R.flag[rec] & 0x10) != 0;
    char *dst = (mate ? out2 : out1) + (mate ? off2[h] : off1[h]);
    const uint32_t total = ext_read_bytes(nn, sn, ln, fastq);
    const uint32_t a0 = so & ~15u;
    const uint32_t span = (fastq ? lo + ln : so + sn) - a0;
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
        else if (k < p_seq + sn) { const uint32_t x = k - p_seq; c = rev ? ext_comp(seq[sn - 1 - x]) : seq[x]; }
        else if (k < p_plus) c = '\n';
        else if (k == p_plus) c = '+';
        else if (k < p_qual) c = '\n';
        else if (k < p_qual + ln) { const uint32_t x = k - p_qual; c = rev ? qual[ln - 1 - x] : qual[x]; }
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
    free_on_device(h.dev, {h.d_chrom.pool, h.d_chrom.off, h.d_chrom.slot, h.d_creg, h.d_rfam, h.d_rl, h.d_rr});
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

// the device route for one chunk; *declined != 0: nothing was appended, the host route takes the chunk
static int ext_device(hgx_extract &h, const char *base, size_t n_bytes, const std::vector<uint32_t> &ls, const std::vector<uint32_t> &le,
                      hipStream_t st, int *declined) {
    *declined = 0;
    const long N = (long)ls.size();
    if (h.n_fam > 64) { *declined = HGX_EXT_DECLINE_FAMILIES; return HGX_OK; }
    RCHK(ext_upload_table(h));
    DevBufs m("extract route");
    char *d_text, *d_scan;
    uint32_t *d_ls, *d_le, *d_head, *d_gid, *d_dec, *d_tot;
    unsigned long long *d_or;
    ExtRec R;
    RCHK(m.get(d_text, n_bytes + 64));
    RCHK(m.get(d_ls, N)); RCHK(m.get(d_le, N)); RCHK(m.get(d_head, N)); RCHK(m.get(d_gid, N));
    RCHK(m.get(R.flag, N)); RCHK(m.get(R.tags, N)); RCHK(m.get(R.qoff, N)); RCHK(m.get(R.qlen, N)); RCHK(m.get(R.klen, N));
    RCHK(m.get(R.soff, N)); RCHK(m.get(R.slen, N)); RCHK(m.get(R.loff, N)); RCHK(m.get(R.llen, N));
    RCHK(m.get(R.fam, N)); RCHK(m.get(R.as, N)); RCHK(m.get(R.xs, N)); RCHK(m.get(R.nh, N)); RCHK(m.get(R.kh, N));
    RCHK(m.get(d_dec, 4)); RCHK(m.get(d_tot, 4 + 2 * 64)); RCHK(m.get(d_or, 2 + 64));
    RCHK(m.get(d_scan, hgx_scan_u32_scratch_bytes(N)));
    HIPCHK(hipMemcpyAsync(d_text, base, n_bytes, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(d_text + n_bytes, 0, 64, st));
    HIPCHK(hipMemcpyAsync(d_ls, ls.data(), (size_t)N * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_le, le.data(), (size_t)N * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(d_dec, 0, 16, st));
    HIPCHK(hipMemsetAsync(d_or, 0, (2 + 64) * 8, st));
    hipLaunchKernelGGL(k_ext_records, dim3(nblk(N, 256)), dim3(256), 0, st, d_text, d_ls, d_le, N, h.d_chrom, h.d_creg,
                       h.d_rfam, h.d_rl, h.d_rr, h.simulation, R, d_dec);
    HIPCHK(hipGetLastError());
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
    RCHK(m.get(d_gstart, (size_t)G + 1)); RCHK(m.get(d_r1, G)); RCHK(m.get(d_r2, G)); RCHK(m.get(d_ghit, G)); RCHK(m.get(d_hpos, G));
    RCHK(m.get(d_gbits, G));
    hipLaunchKernelGGL(k_rec_gstart, dim3(nblk(N, 256)), dim3(256), 0, st, d_head, d_gid, N, d_gstart);
    HIPCHK(hipGetLastError());
    const uint32_t n32 = (uint32_t)N;
    HIPCHK(hipMemcpyAsync(d_gstart + G, &n32, 4, hipMemcpyHostToDevice, st));
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
    h.up_bytes += (long long)n_bytes + 8ll * N;
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
        hipLaunchKernelGGL(k_ext_emit, dim3(2 * H), dim3(64), 0, st, d_text, d_hg, (long)H, d_gbits, fams[k], d_gstart, d_r1, d_r2, R, h.fastq,
                           d_off + (2 * k) * Hp, d_off + (2 * k + 1) * Hp, d_out + part[2 * k], h.paired ? d_out + part[2 * k + 1] : (char *)nullptr);
        HIPCHK(hipGetLastError());
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

extern "C" int hgx_extract_file(hgx_extract *h, const char *path, void *stream) {
    ARGCHK(h && path);
    FILE *f = fopen(path, "rb");
    if (!f) { hgx_set_error("hgx_extract_file: cannot open %s", path); return HGX_EINVAL; }
    unsigned char magic[4] = {0, 0, 0, 0};
    const size_t got = fread(magic, 1, 4, f);
    if (got >= 2 && magic[0] == 0x1f && magic[1] == 0x8b) {
        // BAM (BGZF): the existing reader inflates and walks the file in one piece, records in file order, as the text
        // `samtools view` prints; that text is the stream
        fclose(f);
        std::vector<char> text;
        size_t tot;
        RCHK(bam_as_sam_text(path, nullptr, EXT_MAX_BUF, text, tot));
        if (tot > EXT_MAX_BUF) {
            hgx_set_error("hgx_extract_file: %s holds %zu bytes of records; a BAM is read in one piece of at most %zu (feed it as SAM text)",
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

extern "C" int hgx_extract_take(hgx_extract *h, int32_t family, int32_t mate, const char **text, size_t *n_bytes) {
    ARGCHK(h && text && n_bytes && family >= 0 && family < h->n_fam && (mate == 0 || mate == 1));
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
    delete h;
    return HGX_OK;
}

// hgx_bgzf.cpp -- the BGZF container (SAM/BAM specification v1, section 4.1) as the host sees it: the block table of a file or of a
// piece of one.  Host only: the reader (hgx_bam.cpp), the index (hgx_bai.cpp) and read extraction walk the container here; the
// kernels that inflate the blocks are hgx_inflate.hip.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "hgx_internal.hpp"

namespace {
inline size_t rd16(const unsigned char *p) { return (size_t)p[0] | ((size_t)p[1] << 8); }
inline uint32_t rd32(const unsigned char *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
}   // namespace

// One block header (hgx_internal.hpp): magic, XLEN, the BC subfield, the block length, and the payload's place, crc and size.  The BC
// subfield is read only where it lies inside the extra field (and inside the bytes present); the last one wins.
int hgx_bgzf_block_at(const unsigned char *data, size_t n, size_t off, hgx_bgzf_block *b, size_t *blen_out) {
    const unsigned char *h = data + off;
    const size_t have = n - off;
    if (blen_out) *blen_out = 0;
    if (h[0] != 0x1f || (have > 1 && h[1] != 0x8b) || (have > 2 && h[2] != 8) || (have > 3 && !(h[3] & 4))) return HGX_BGZF_NOT;
    if (have < 18) return HGX_BGZF_SHORT;
    const size_t ext_end = 12 + rd16(h + 10), seen = std::min(ext_end, have);
    size_t blen = 0;
    for (size_t p = 12; p + 4 <= seen;) {
        const size_t slen = rd16(h + p + 2);
        if (h[p] == 66 && h[p + 1] == 67 && slen == 2 && p + 6 <= seen) blen = rd16(h + p + 4) + 1;
        p += 4 + slen;
    }
    if (blen_out) *blen_out = blen;
    if (ext_end > have) return HGX_BGZF_CUT_HEADER;
    if (!blen) return HGX_BGZF_NO_BC;
    if (blen < ext_end + 8) return HGX_BGZF_BAD_LEN;
    if (blen > have) return HGX_BGZF_CUT_BLOCK;
    if (b) { b->in_off = off + ext_end; b->in_len = blen - ext_end - 8; b->crc = rd32(h + blen - 8); b->out_len = rd32(h + blen - 4); b->out_off = 0; }
    return HGX_BGZF_BLOCK;
}

// the BGZF blocks of `data` (host bytes; n bytes) as descriptors: HGX_OK, or the host reader's error for a malformed container.
// The stream form takes a piece of a file that arrives in chunks: `file_off` = where data[0] lies in the file (the errors' offsets),
// `last` = the file ends with these bytes; otherwise a block that is not complete yet is left for the next call and *used = the
// bytes the complete blocks take.
int hgx_bgzf_scan_stream(const unsigned char *data, size_t n, bool last, size_t file_off, std::vector<hgx_bgzf_block> &blocks, size_t *total_out,
                         size_t *used) {
    blocks.clear();
    size_t off = 0, total = 0;
    while (off < n) {
        hgx_bgzf_block b;
        size_t blen = 0;
        const int st = hgx_bgzf_block_at(data, n, off, &b, &blen);
        if (st != HGX_BGZF_BLOCK) {
            if (!last && (st == HGX_BGZF_SHORT || st == HGX_BGZF_CUT_HEADER || st == HGX_BGZF_CUT_BLOCK)) break;       // (the next call's)
            hgx_set_error(st == HGX_BGZF_CUT_HEADER ? "truncated BGZF header at offset %zu" : st == HGX_BGZF_NO_BC ? "BGZF block without BC subfield at offset %zu" :
                          st == HGX_BGZF_NOT || st == HGX_BGZF_SHORT ? "not a BGZF block at offset %zu" : "truncated BGZF block at offset %zu", file_off + off);
            return HGX_EPARSE;
        }
        b.out_off = total;
        total += b.out_len;
        blocks.push_back(b);
        off += blen;
    }
    if (total_out) *total_out = total;
    if (used) *used = off;
    return HGX_OK;
}
int hgx_bgzf_scan(const unsigned char *data, size_t n, std::vector<hgx_bgzf_block> &blocks, size_t *total_out) {
    return hgx_bgzf_scan_stream(data, n, true, 0, blocks, total_out, nullptr);
}

// The same on several host threads.  The blocks of a BGZF file form a chain (each BSIZE leads to the next header), and every hop of
// the walk is a cache miss in bytes another core has just written: 5 007 blocks of a 20 MB BAM took 0.55 ms on one thread -- in front
// of the device inflate's launch (tools/bam_gap_timeline.py).  Here the file is cut into ranges; every range but the first FINDS a
// block start (the gzip magic with a BC subfield whose BSIZE leads to three more such headers, or to the file's end) and walks from
// there to the first block boundary at or behind its end; the ranges must link up -- a walk ends exactly where the next one began --
// or the chain is walked by one thread after all (which also words the errors).  Same descriptors, same order.
int hgx_bgzf_scan_par(const unsigned char *data, size_t n, std::vector<hgx_bgzf_block> &blocks, size_t *total_out, int n_threads) {
    const int T = (int)std::min<size_t>({(size_t)std::max(1, n_threads), (size_t)16, n / (1u << 20)});
    if (T < 2) return hgx_bgzf_scan(data, n, blocks, total_out);
    // length of the block whose header starts at `off` (0 = not a block the serial walk would take), its payload's place
    auto block_at = [&](size_t off, hgx_bgzf_block *b) -> size_t {
        size_t blen = 0;
        return hgx_bgzf_block_at(data, n, off, b, &blen) == HGX_BGZF_BLOCK ? blen : 0;
    };
    std::vector<std::vector<hgx_bgzf_block>> part((size_t)T);
    std::vector<size_t> first((size_t)T, n), last((size_t)T, n), out_bytes((size_t)T, 0);
    std::vector<int> bad((size_t)T, 0);
    hgx_run_workers(T, [&](int r) {
        const size_t lo = n * (size_t)r / (size_t)T, hi = n * (size_t)(r + 1) / (size_t)T;
        size_t off = lo;
        if (r > 0) {
            off = n;
            for (size_t p = lo; p + 18 <= n && p < hi;) {
                const unsigned char *q = (const unsigned char *)memchr(data + p, 0x1f, hi - p);
                if (!q) break;
                p = (size_t)(q - data);
                size_t at = p;
                int hops = 0;
                for (; hops < 4 && at < n; ++hops) {
                    const size_t bl = block_at(at, nullptr);
                    if (!bl) break;
                    at += bl;
                }
                if (hops == 4 || (hops > 0 && at == n)) { off = p; break; }
                ++p;
            }
        }
        first[(size_t)r] = off;
        std::vector<hgx_bgzf_block> &mine = part[(size_t)r];
        mine.reserve((hi - lo) / 2048 + 16);
        size_t tot = 0;
        while (off < hi) {
            hgx_bgzf_block b;
            const size_t bl = block_at(off, &b);
            if (!bl) { bad[(size_t)r] = 1; break; }
            b.out_off = tot;
            tot += b.out_len;
            mine.push_back(b);
            off += bl;
        }
        last[(size_t)r] = off;
        out_bytes[(size_t)r] = tot;
    });
    bool linked = first[0] == 0;
    for (int r = 0; r < T && linked; ++r) linked = !bad[(size_t)r] && last[(size_t)r] == (r + 1 < T ? first[(size_t)r + 1] : n);
    if (!linked) return hgx_bgzf_scan(data, n, blocks, total_out);
    size_t n_blocks = 0, total = 0;
    for (auto &v : part) n_blocks += v.size();
    blocks.clear();
    blocks.reserve(n_blocks);
    for (int r = 0; r < T; ++r) {
        for (hgx_bgzf_block b : part[(size_t)r]) { b.out_off += total; blocks.push_back(b); }
        total += out_bytes[(size_t)r];
    }
    if (total_out) *total_out = total;
    return HGX_OK;
}

// test entry (hgx.h; host only, no GPU): the container walked by one thread and by `n_threads` -- *same = both gave the same verdict
// and, where they took the file, the same descriptors
extern "C" int hgx_bgzf_scan_compare(const void *bgzf, size_t n_bytes, int32_t n_threads, int64_t *n_blocks, int32_t *same) {
    HARGCHK(bgzf && n_blocks && same);
    std::vector<hgx_bgzf_block> a, b;
    size_t ta = 0, tb = 0;
    const int ra = hgx_bgzf_scan((const unsigned char *)bgzf, n_bytes, a, &ta);
    const int rb = hgx_bgzf_scan_par((const unsigned char *)bgzf, n_bytes, b, &tb, n_threads);
    *n_blocks = ra == HGX_OK ? (int64_t)a.size() : -1;
    bool eq = ra == rb;
    if (eq && ra == HGX_OK) {
        eq = ta == tb && a.size() == b.size();
        for (size_t k = 0; k < a.size() && eq; ++k)
            eq = a[k].in_off == b[k].in_off && a[k].in_len == b[k].in_len && a[k].out_off == b[k].out_off && a[k].out_len == b[k].out_len && a[k].crc == b[k].crc;
    }
    *same = eq ? 1 : 0;
    return HGX_OK;
}

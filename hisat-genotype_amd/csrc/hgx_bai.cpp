// hgx_bai.cpp -- the BAM index (SAM specification section 5.2, `.bai`): read, query, plan, write.  Host only.
//
// The reference reads a locus with `samtools index` + `samtools view file chr:left-right` (typing_core.py:433-444): samtools goes
// through the index and touches the few BGZF blocks that hold the region.  This unit is that index for libhgx:
//   * hgx_bai_parse / hgx_bai_load: every read bounds-checked against the file's length; anything wrong makes the index UNUSABLE,
//     which the reader treats as "no index" (it then reads the whole file as before), never as an error;
//   * hgx_bai_query: the chunks (pairs of virtual offsets) that may hold records overlapping [beg0, end0) on a reference;
//   * hgx_bai_plan: the union of the chunks of all regions of a call as a short list of segments to read;
//   * hgx_bam_index_build (exported): what `samtools index` does for a coordinate-sorted BAM, one streaming pass, bounded memory.
// tests/bai_ref.py states the same rules in plain Python; the tests compare the writer's bytes with it.
//
// A virtual offset is (file offset of a BGZF block << 16) | offset inside the block's payload.  A chunk's end is where the record
// after its last one begins, so chunk ends (and the ends of merged chunks) are record boundaries.
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "hgx_internal.hpp"

namespace {

inline uint32_t ld32(const unsigned char *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
inline uint64_t ld64(const unsigned char *p) { return (uint64_t)ld32(p) | ((uint64_t)ld32(p + 4) << 32); }

constexpr uint32_t BAI_PSEUDO_BIN = 37450;           // htslib's metadata bin: its "chunks" are counters, not offsets
constexpr int64_t BAI_MAX_POS = (int64_t)1 << 29;    // the binning scheme's reach

// [lo, hi) of the reference a bin covers (the specification's six levels: 1, 8, 64, 512, 4096, 32768 bins); false: no such bin
inline bool bin_span(uint32_t bin, int64_t &lo, int64_t &hi) {
    static const uint32_t first[7] = {0, 1, 9, 73, 585, 4681, 37449};
    for (int lv = 0; lv < 6; ++lv)
        if (bin < first[lv + 1]) {
            const int shift = 29 - 3 * lv;
            lo = (int64_t)(bin - first[lv]) << shift;
            hi = lo + ((int64_t)1 << shift);
            return true;
        }
    return false;
}

}   // namespace

bool hgx_bai_parse(const unsigned char *p, size_t n, hgx_bai_index &ix) {
    ix = hgx_bai_index();
    size_t q = 0;
    auto have = [&](uint64_t k) { return (uint64_t)(n - q) >= k; };
    if (!have(8) || memcmp(p, "BAI\1", 4) != 0) return false;
    const int32_t n_ref = (int32_t)ld32(p + 4);
    q = 8;
    if (n_ref < 0 || !have((uint64_t)n_ref * 8)) return false;          // (a reference takes at least its two counts)
    ix.refs.resize((size_t)n_ref);
    for (int32_t r = 0; r < n_ref; ++r) {
        hgx_bai_index::Ref &R = ix.refs[(size_t)r];
        if (!have(4)) return false;
        const int32_t n_bin = (int32_t)ld32(p + q);
        q += 4;
        if (n_bin < 0 || !have((uint64_t)n_bin * 8)) return false;
        R.bin0 = ix.bins.size();
        R.n_bin = (size_t)n_bin;
        for (int32_t b = 0; b < n_bin; ++b) {
            if (!have(8)) return false;
            hgx_bai_index::Bin B;
            B.bin = ld32(p + q);
            const int32_t n_chunk = (int32_t)ld32(p + q + 4);
            q += 8;
            if (n_chunk < 0 || !have((uint64_t)n_chunk * 16)) return false;
            B.chunk0 = ix.chunks.size();
            B.n_chunk = (uint32_t)n_chunk;
            for (int32_t c = 0; c < n_chunk; ++c, q += 16) {
                const hgx_bai_chunk ch{ld64(p + q), ld64(p + q + 8)};
                if (B.bin != BAI_PSEUDO_BIN && ch.beg > ch.end) return false;
                ix.chunks.push_back(ch);
            }
            ix.bins.push_back(B);
        }
        if (!have(4)) return false;
        const int32_t n_intv = (int32_t)ld32(p + q);
        q += 4;
        if (n_intv < 0 || !have((uint64_t)n_intv * 8)) return false;
        R.intv0 = ix.ioffset.size();
        R.n_intv = (size_t)n_intv;
        for (int32_t w = 0; w < n_intv; ++w, q += 8) ix.ioffset.push_back(ld64(p + q));
    }
    if (n - q >= 8) ix.n_no_coor = (int64_t)ld64(p + q);                // optional
    else if (n - q != 0) return false;                                   // (cut inside it)
    return true;
}

// <path>.bai, then <path minus .bam>.bai.  0 = usable, 1 = none beside the file, 2 = unusable
int hgx_bai_load(const char *bam_path, hgx_bai_index &ix) {
    std::string cand[2];
    cand[0] = std::string(bam_path) + ".bai";
    const size_t L = strlen(bam_path);
    if (L > 4 && strcmp(bam_path + L - 4, ".bam") == 0) cand[1] = std::string(bam_path, L - 4) + ".bai";
    for (const std::string &c : cand) {
        if (c.empty()) continue;
        const int fd = open(c.c_str(), O_RDONLY);
        if (fd < 0) continue;
        struct stat sb;
        if (fstat(fd, &sb) != 0 || sb.st_size < 0 || !S_ISREG(sb.st_mode)) { close(fd); return 2; }
        std::vector<unsigned char> bytes((size_t)sb.st_size);
        const bool got_all = hgx_pread_all(fd, bytes.data(), bytes.size(), 0);
        close(fd);
        if (!got_all) return 2;
        return hgx_bai_parse(bytes.data(), bytes.size(), ix) ? 0 : 2;
    }
    return 1;
}

// chunks that may hold records overlapping [beg0, end0) of reference `ref`, appended to `out`.  false: the positions are beyond what
// the binning scheme reaches (the index is unusable for this call).  The bins are the specification's reg2bins (a bin is taken
// when its span overlaps the region; the pseudo-bin has no span); a chunk that ends at or before the linear offset of the region's
// first 16 kb window holds no record that reaches the window.  The linear offset is a lower bound only: it may be 0, or carried
// over from an earlier window; a region that begins beyond the last window takes what the bins give.
bool hgx_bai_query(const hgx_bai_index &ix, int32_t ref, int64_t beg0, int64_t end0, std::vector<hgx_bai_chunk> &out) {
    if (beg0 < 0) beg0 = 0;
    if (beg0 >= BAI_MAX_POS || end0 > BAI_MAX_POS) return false;
    if (ref < 0 || (size_t)ref >= ix.refs.size() || end0 <= beg0) return true;
    const hgx_bai_index::Ref &R = ix.refs[(size_t)ref];
    const size_t w = (size_t)(beg0 >> 14);
    const uint64_t min_off = w < R.n_intv ? ix.ioffset[R.intv0 + w] : 0;
    for (size_t b = R.bin0; b < R.bin0 + R.n_bin; ++b) {
        const hgx_bai_index::Bin &B = ix.bins[b];
        int64_t lo, hi;
        if (!bin_span(B.bin, lo, hi) || hi <= beg0 || lo >= end0) continue;
        for (size_t c = B.chunk0; c < B.chunk0 + B.n_chunk; ++c)
            if (ix.chunks[c].end > min_off && ix.chunks[c].end > ix.chunks[c].beg) out.push_back(ix.chunks[c]);
    }
    return true;
}

// The union of `chunks` (any order; sorted in place) as segments in file order.  Two chunks become one segment when the next one
// begins at or before the current one's end, in the BGZF block where the current one ends, or no more than HGX_BAI_MERGE_GAP bytes of
// file behind that block's start (a few blocks read and filtered away cost less than another read and another chain to check).
// Chunk ends are record boundaries, so a segment begins and ends on a record boundary too.
void hgx_bai_plan(std::vector<hgx_bai_chunk> &chunks, std::vector<hgx_bai_chunk> &segments) {
    segments.clear();
    std::sort(chunks.begin(), chunks.end(), [](const hgx_bai_chunk &a, const hgx_bai_chunk &b) { return a.beg != b.beg ? a.beg < b.beg : a.end < b.end; });
    for (const hgx_bai_chunk &c : chunks) {
        if (!segments.empty() && (c.beg <= segments.back().end || (c.beg >> 16) <= (segments.back().end >> 16) + HGX_BAI_MERGE_GAP))
            segments.back().end = std::max(segments.back().end, c.end);
        else segments.push_back(c);
    }
}

// do the segments lie inside a file of `file_size` bytes?  (begin inside it, end at most at its end, an end inside a block only where a
// block can begin.)  The reader asks before it reads: an index that points elsewhere is stale.
bool hgx_bai_plan_fits(const std::vector<hgx_bai_chunk> &segments, uint64_t file_size) {
    for (const hgx_bai_chunk &s : segments) {
        const uint64_t fb = s.beg >> 16, fe = s.end >> 16;
        if (fb >= file_size || fe > file_size || fe < fb || ((s.end & 0xffff) && fe >= file_size)) return false;
    }
    return true;
}

#ifndef HGX_BAI_STANDALONE
// ---- writer ---------------------------------------------------------------------------------------------------------------
// One pass over the file in pieces of deflated bytes: the pieces' complete BGZF blocks are inflated (host), the record chain is
// followed through them, a record cut by a piece's end is carried into the next piece.  Memory: one piece, its inflated bytes and
// the index of ONE reference (a reference's part is written as soon as the next reference begins).  The rule, so that the bytes
// are defined (tests/bai_ref.py):
//   * a record's virtual offset names the first block whose payload reaches beyond the record's first byte; the end of the stream
//     is (file size << 16);
//   * placed = refID >= 0 and pos >= 0; bin = reg2bin(pos, pos + max(reference span of the CIGAR, 1)), span 0 with the unmapped flag;
//   * the chunks of a (reference, bin) are the maximal runs of consecutive records with that pair, each [first record's offset,
//     offset of the record behind the run), bins in ascending order, no pseudo-bin;
//   * ioffset[w] = the smallest offset of a record overlapping 16 kb window w, windows without one take the previous window's
//     value (0 in front of the first), n_intv = last overlapped window + 1;
//   * n_no_coor = the records that are not placed, written at the end.
namespace {

int bai_reg2bin(int64_t beg, int64_t end) {
    --end;
    if (beg >> 14 == end >> 14) return (int)(4681 + (beg >> 14));
    if (beg >> 17 == end >> 17) return (int)(585 + (beg >> 17));
    if (beg >> 20 == end >> 20) return (int)(73 + (beg >> 20));
    if (beg >> 23 == end >> 23) return (int)(9 + (beg >> 23));
    if (beg >> 26 == end >> 26) return (int)(1 + (beg >> 26));
    return 0;
}

struct Span { uint64_t stream_off; uint32_t out_len; uint64_t file_off; };      // a block's payload in the inflated stream

struct RefIndex {
    std::map<uint32_t, std::vector<hgx_bai_chunk>> bins;
    std::vector<uint64_t> ioffset;        // 0 = not set yet (no record starts at virtual offset 0: the header's magic is there)
    void clear() { bins.clear(); ioffset.clear(); }
};

void w32(std::vector<unsigned char> &o, uint32_t v) { for (int k = 0; k < 4; ++k) o.push_back((unsigned char)(v >> (8 * k))); }
void w64(std::vector<unsigned char> &o, uint64_t v) { for (int k = 0; k < 8; ++k) o.push_back((unsigned char)(v >> (8 * k))); }

void emit_ref(std::vector<unsigned char> &o, RefIndex &R) {
    w32(o, (uint32_t)R.bins.size());
    for (auto &kv : R.bins) {
        w32(o, kv.first);
        w32(o, (uint32_t)kv.second.size());
        for (const hgx_bai_chunk &c : kv.second) { w64(o, c.beg); w64(o, c.end); }
    }
    w32(o, (uint32_t)R.ioffset.size());
    uint64_t prev = 0;
    for (uint64_t v : R.ioffset) { if (v) prev = v; w64(o, prev); }
    R.clear();
}

}   // namespace

extern "C" int hgx_bam_index_build(const char *path, const char *out_path, int32_t n_threads) {
    HARGCHK(path);
    if (n_threads <= 0) n_threads = hgx_default_threads();
    n_threads = std::max(1, std::min(n_threads, 512));
    const std::string out_name = out_path && out_path[0] ? std::string(out_path) : std::string(path) + ".bai";
    const std::string tmp_name = out_name + ".tmp." + std::to_string((long)getpid());
    int fd = -1;
    FILE *fo = nullptr;
    auto fail = [&](int rc) {
        if (fd >= 0) close(fd);
        if (fo) { fclose(fo); unlink(tmp_name.c_str()); }
        return rc;
    };
    try {
        fd = open(path, O_RDONLY);
        if (fd < 0) { hgx_set_error("cannot open %s", path); return HGX_EINVAL; }
        struct stat sb;
        if (fstat(fd, &sb) != 0 || sb.st_size < 0) { hgx_set_error("cannot stat %s", path); return fail(HGX_EINVAL); }
        const size_t file_size = (size_t)sb.st_size;
        const char *piece_sw = hgx_test_switch("bai_piece");              // deflated bytes per piece (tests: small, so that every piece cuts a record)
        const size_t piece = piece_sw ? std::max<size_t>(1, (size_t)strtoull(piece_sw, nullptr, 10)) : ((size_t)16 << 20);
        fo = fopen(tmp_name.c_str(), "wb");
        if (!fo) { hgx_set_error("cannot create %s", tmp_name.c_str()); return fail(HGX_EINVAL); }
        std::vector<unsigned char> comp, text, o;      // deflated bytes not yet taken; inflated bytes not yet taken; output not yet written
        std::vector<Span> spans;                       // the blocks `text` lies in
        std::vector<hgx_bgzf_block> blocks;
        size_t file_pos = 0, comp_at = 0;              // next byte to read; file offset of comp[0]
        uint64_t text_at = 0;                          // stream offset of text[0]
        bool header_done = false;
        int32_t n_ref = 0;
        std::vector<int32_t> ref_len;
        RefIndex R;
        int32_t cur_ref = -1;                          // the reference whose index is being collected; refs below it are written
        int64_t last_pos = -1;
        bool open_run = false, seen_unplaced = false;
        uint32_t run_bin = 0;
        uint64_t run_beg = 0, n_no_coor = 0;
        auto flush_to = [&](int32_t ref) {             // the parts of the references below `ref`
            while (cur_ref < ref) {
                if (cur_ref >= 0) emit_ref(o, R);
                ++cur_ref;
            }
        };
        auto close_run = [&](uint64_t v) {
            if (open_run) R.bins[run_bin].push_back(hgx_bai_chunk{run_beg, v});
            open_run = false;
        };
        o.insert(o.end(), {'B', 'A', 'I', 1});
        while (true) {
            const bool last = file_pos >= file_size;
            if (!last) {
                const size_t want = std::min(piece, file_size - file_pos), at = comp.size();
                comp.resize(at + want);
                size_t got = 0;
                if (!hgx_pread_all(fd, comp.data() + at, want, file_pos, &got)) { hgx_set_error("short read on %s at offset %zu", path, file_pos + got); return fail(HGX_EINVAL); }
                file_pos += want;
            }
            const bool at_end = file_pos >= file_size;
            size_t used = 0, total = 0;
            if (comp.empty()) { if (at_end) break; continue; }
            const int rc = hgx_bgzf_scan_stream(comp.data(), comp.size(), at_end, comp_at, blocks, &total, &used);
            if (rc) return fail(rc);
            if (!blocks.empty()) {
                size_t hdr_at = 0;
                for (const hgx_bgzf_block &b : blocks) {                 // (ISIZE is the file's word: checked before it sizes a buffer)
                    if (b.out_len > 65536) { hgx_set_error("BGZF block at offset %zu claims %zu bytes of payload", comp_at + hdr_at, (size_t)b.out_len); return fail(HGX_EPARSE); }
                    hdr_at = b.in_off + b.in_len + 8;
                }
                const size_t t0 = text.size();
                text.resize(t0 + total);
                std::vector<int> bad((size_t)n_threads, 0);
                hgx_par_ranges(blocks.size() >= 64 ? n_threads : 1, blocks.size(), [&](int t, size_t b0, size_t b1) {
                    for (size_t k = b0; k < b1; ++k)
                        if (blocks[k].out_len > 65536 || !hgx_bam_inflate_block(comp.data(), blocks[k], text.data() + t0 + blocks[k].out_off)) { bad[(size_t)t] = (int)k + 1; return; }
                });
                for (int v : bad)
                    if (v) {
                        const hgx_bgzf_block &b = blocks[(size_t)v - 1];
                        hgx_set_error("corrupt BGZF block near offset %zu (inflate / CRC32 / ISIZE mismatch)", comp_at + b.in_off);
                        return fail(HGX_EPARSE);
                    }
                size_t hdr = 0;                                          // (a block's header begins where the block before it ended)
                for (const hgx_bgzf_block &b : blocks) {
                    if (b.out_len) spans.push_back(Span{text_at + t0 + b.out_off, (uint32_t)b.out_len, comp_at + hdr});
                    hdr = b.in_off + b.in_len + 8;
                }
            }
            comp.erase(comp.begin(), comp.begin() + (ptrdiff_t)used);
            comp_at += used;
            // ---- the records these bytes complete ------------------------------------------------------------------
            size_t q = 0, sp = 0;                                        // offset in `text`; the span q lies in
            if (!header_done) {
                const size_t n = text.size();
                bool need_more = false;
                if (n >= 4 && memcmp(text.data(), "BAM\1", 4) != 0) { hgx_set_error("%s is not a BAM file", path); return fail(HGX_EPARSE); }
                if (n < 12) need_more = true;
                size_t p = 0;
                if (!need_more) {
                    p = 8 + (size_t)ld32(&text[4]);
                    if (p + 4 > n) need_more = true;
                }
                if (!need_more) {
                    n_ref = (int32_t)ld32(&text[p]);
                    if (n_ref < 0) { hgx_set_error("malformed BAM header in %s", path); return fail(HGX_EPARSE); }
                    p += 4;
                    ref_len.clear();
                    for (int32_t i = 0; i < n_ref && !need_more; ++i) {
                        if (p + 4 > n) { need_more = true; break; }
                        const size_t l_name = ld32(&text[p]);
                        if (p + 4 + l_name + 4 > n) { need_more = true; break; }
                        ref_len.push_back((int32_t)ld32(&text[p + 4 + l_name]));
                        p += 4 + l_name + 4;
                    }
                }
                if (need_more) {
                    if (at_end) { hgx_set_error("truncated BAM header in %s", path); return fail(HGX_EPARSE); }
                    continue;
                }
                for (int32_t i = 0; i < n_ref; ++i)
                    if ((int64_t)ref_len[(size_t)i] > BAI_MAX_POS) {
                        hgx_set_error("reference %d of %s is longer than 2^29: a .bai cannot index it (header offset %zu)", i, path, p);
                        return fail(HGX_EINVAL);
                    }
                header_done = true;
                w32(o, (uint32_t)n_ref);
                q = p;
            }
            auto voffset = [&](uint64_t s) -> uint64_t {                 // s moves forward only
                while (sp < spans.size() && spans[sp].stream_off + spans[sp].out_len <= s) ++sp;
                if (sp == spans.size()) return (uint64_t)file_size << 16;
                return (spans[sp].file_off << 16) | (s - spans[sp].stream_off);
            };
            const size_t n = text.size();
            while (q + 4 <= n) {
                const uint32_t bs = ld32(&text[q]);
                if (bs < 32) { hgx_set_error("malformed BAM record at offset %llu of the inflated stream", (unsigned long long)(text_at + q)); return fail(HGX_EPARSE); }
                if (q + 4 + (size_t)bs > n) break;                       // cut by the piece's end: carried
                const unsigned char *r = &text[q + 4];
                const uint64_t v = voffset(text_at + q);
                const int32_t rid = (int32_t)ld32(r), pos = (int32_t)ld32(r + 4);
                if (rid >= n_ref) { hgx_set_error("record with reference %d of %d at virtual offset %llu", rid, n_ref, (unsigned long long)v); return fail(HGX_EPARSE); }
                if (rid < 0 || pos < 0) {
                    close_run(v);
                    seen_unplaced = true;
                    ++n_no_coor;
                } else {
                    if (seen_unplaced) { hgx_set_error("placed record behind an unplaced one at virtual offset %llu: not sorted by coordinate", (unsigned long long)v); return fail(HGX_EINVAL); }
                    if (rid < cur_ref || (rid == cur_ref && pos < last_pos)) {
                        hgx_set_error("records out of coordinate order at virtual offset %llu (reference %d, position %d)", (unsigned long long)v, rid, pos + 1);
                        return fail(HGX_EINVAL);
                    }
                    const int64_t end = (int64_t)pos + std::max<int64_t>(hgx_bam_cigar_reflen(r, bs), 1);
                    if (end > BAI_MAX_POS) { hgx_set_error("record beyond position 2^29 at virtual offset %llu: a .bai cannot index it", (unsigned long long)v); return fail(HGX_EINVAL); }
                    const uint32_t bin = (uint32_t)bai_reg2bin(pos, end);
                    if (rid != cur_ref) { close_run(v); flush_to(rid); last_pos = -1; }
                    if (!open_run || bin != run_bin) { close_run(v); open_run = true; run_bin = bin; run_beg = v; }
                    const size_t w1 = (size_t)((end - 1) >> 14);
                    if (R.ioffset.size() <= w1) R.ioffset.resize(w1 + 1, 0);
                    for (size_t w = (size_t)(pos >> 14); w <= w1; ++w) if (!R.ioffset[w]) R.ioffset[w] = v;
                    last_pos = pos;
                }
                q += 4 + (size_t)bs;
            }
            if (at_end && q != n) { hgx_set_error("truncated BAM record at offset %llu of the inflated stream", (unsigned long long)(text_at + q)); return fail(HGX_EPARSE); }
            // drop what was taken: the bytes and the spans in front of q
            {
                size_t keep = 0;
                while (keep < spans.size() && spans[keep].stream_off + spans[keep].out_len <= text_at + q) ++keep;
                spans.erase(spans.begin(), spans.begin() + (ptrdiff_t)keep);
                text.erase(text.begin(), text.begin() + (ptrdiff_t)q);
                text_at += q;
            }
            if (o.size() > (1u << 20) || at_end) {
                if (at_end) {
                    if (!header_done) { hgx_set_error("%s holds no BAM header", path); return fail(HGX_EPARSE); }
                    close_run((uint64_t)file_size << 16);
                    flush_to(n_ref);
                    w64(o, n_no_coor);
                }
                if (!o.empty() && fwrite(o.data(), 1, o.size(), fo) != o.size()) { hgx_set_error("short write on %s", tmp_name.c_str()); return fail(HGX_EINVAL); }
                o.clear();
            }
            if (at_end) break;
        }
        if (!header_done) { hgx_set_error("%s holds no BAM header", path); return fail(HGX_EPARSE); }
        close(fd);
        fd = -1;
        const bool ok = fclose(fo) == 0;
        fo = nullptr;
        if (!ok || rename(tmp_name.c_str(), out_name.c_str()) != 0) {
            unlink(tmp_name.c_str());
            hgx_set_error("cannot write %s", out_name.c_str());
            return HGX_EINVAL;
        }
        return HGX_OK;
    } catch (const std::exception &e) {
        hgx_set_error("hgx_bam_index_build: %s", e.what());
        return fail(HGX_ENOMEM);
    }
}
#endif   // HGX_BAI_STANDALONE

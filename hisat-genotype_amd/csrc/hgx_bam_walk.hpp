// hgx_bam_walk.hpp -- the record chain of an inflated BAM stream walked on the device, shared by the front end (hgx_front.hip:
// whole files of one or many tasks) and read extraction (hgx_extract.hip: one chunk of a stream of any length).
// The records of a BAM form a chain (each block_size leads to the next), so the stream is cut into ranges; every range but the
// first GUESSES a record start (a header that is plausible and leads to three more plausible headers) and walks from there past
// its end; the guesses are then CHECKED -- a range's walk must end exactly where the next one's begins -- and anything that does
// not link up declines the call.  OPEN (extraction): the stream may end inside a record; the walk stops in front of the first
// record that is not complete and the link kernel reports that offset (BamCtl::end) instead of asking for the stream's end.
#pragma once
#include <cstdint>

#include "hgx_internal.hpp"

namespace {
struct BamCtl { int32_t decline; uint32_t n_rec, n_kept, max_klen, unsorted; uint32_t tot[4]; uint32_t end; };      // tot: the scans' aggregates (records of the walk ranges); end: OPEN, the first incomplete record
__device__ __forceinline__ void bam_decline(BamCtl *c, int code) { atomicCAS(&c->decline, 0, code); }
__device__ __forceinline__ uint32_t bam_u32(const unsigned char *p) { uint32_t v; __builtin_memcpy(&v, p, 4); return v; }
__device__ __forceinline__ int32_t bam_i32(const unsigned char *p) { int32_t v; __builtin_memcpy(&v, p, 4); return v; }
__device__ __forceinline__ uint32_t bam_u16(const unsigned char *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
__device__ bool bam_plausible(const unsigned char *raw, size_t n, size_t o, int n_ref) {
    if (o + 36 > n) return false;
    const uint32_t bs = bam_u32(raw + o);
    if (bs < 32 || o + 4 + (size_t)bs > n) return false;
    const unsigned char *r = raw + o + 4;
    const int32_t rid = bam_i32(r), pos = bam_i32(r + 4), nrid = bam_i32(r + 20), npos = bam_i32(r + 24), l_seq = bam_i32(r + 16);
    const uint32_t l_rn = r[8], n_cig = bam_u16(r + 12);
    if (rid < -1 || rid >= n_ref || nrid < -1 || nrid >= n_ref) return false;
    if (pos < -1 || npos < -1 || l_seq < 0 || l_rn == 0) return false;
    if (32 + (size_t)l_rn + 4 * (size_t)n_cig + (size_t)(l_seq + 1) / 2 + (size_t)l_seq > bs) return false;
    if (r[32 + l_rn - 1] != 0) return false;
    for (uint32_t k = 0; k + 1 < l_rn; ++k) if (r[32 + k] < 33 || r[32 + k] > 126) return false;
    return true;
}
// the chain's cheaper test: the fields that tie a header to its block_size and the name's terminator -- every load independent of the
// others (the character loop of bam_plausible is a chain of dependent loads; it runs once, on the candidate whose chain held)
__device__ bool bam_header_fits(const unsigned char *raw, size_t n, size_t o, int n_ref) {
    if (o + 36 > n) return false;
    const uint32_t bs = bam_u32(raw + o);
    const unsigned char *r = raw + o + 4;
    const int32_t rid = bam_i32(r), l_seq = bam_i32(r + 16);
    const uint32_t l_rn = r[8], n_cig = bam_u16(r + 12);
    if (bs < 32 || o + 4 + (size_t)bs > n) return false;
    if (rid < -1 || rid >= n_ref || l_seq < 0 || l_rn == 0) return false;
    if (32 + (size_t)l_rn + 4 * (size_t)n_cig + (size_t)(l_seq + 1) / 2 + (size_t)l_seq > bs) return false;
    return r[32 + l_rn - 1] == 0;
}
// OPEN: the chain may also end at a record that runs past the stream's end (or whose block_size word does)
__device__ __forceinline__ bool bam_open_end(const unsigned char *raw, size_t n, size_t o) {
    if (o + 4 > n) return true;
    const uint32_t bs = bam_u32(raw + o);
    return bs >= 32 && bs < (1u << 24) && o + 4 + (size_t)bs > n;
}
struct BamRange { uint32_t first, stop, count, state; };     // (offsets inside the task's stream) state: 1 = walked, 2 = no record start in the range, 0 = a broken record
// a task's stream inside the device text (one task: the whole text), its header's verdicts and its share of the walk ranges
struct BamSeg {
    uint32_t base, n, body0;           // where the stream starts in the text, its bytes, its first record
    int32_t n_ref;
    uint32_t act_off;                  // its references' actions in the action table (0 drop, 1 keep, 2 keep where the span overlaps)
    uint32_t filtered;
    long long left0, right0;
    uint32_t first_range, n_ranges;
    // a region LIST (k_bam_filter): regions 1 .. n_regions - 1 -- region g's span at spans[span_off + g - 1], its references' actions at
    // act_off + g * n_ref (region 0: left0 / right0 and act_off, as for one region)
    uint32_t n_regions, span_off;
};
struct BamSpan { long long left0, right0; };
__device__ __forceinline__ int bam_seg_of(const BamSeg *__restrict__ segs, int n_seg, uint32_t range) {
    int lo = 0, hi = n_seg - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (segs[mid].first_range <= range) lo = mid; else hi = mid - 1; }
    return lo;
}
// PASS 0: find the range's first record and count; PASS 1: the same walk again, writing (offset after block_size, length, task)
template <int PASS, bool OPEN = false>
__global__ void __launch_bounds__(64) k_bam_walk(const unsigned char *__restrict__ text, const BamSeg *__restrict__ segs, int n_seg, int W,
                                                 BamRange *__restrict__ rng, const uint32_t *__restrict__ base, uint32_t *__restrict__ rec_off,
                                                 uint32_t *__restrict__ rec_len, uint16_t *__restrict__ rec_task) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= W) return;
    const int sg = bam_seg_of(segs, n_seg, (uint32_t)t);
    const BamSeg G = segs[sg];
    const unsigned char *raw = text + G.base;
    const size_t n = G.n, body0 = G.body0;
    const size_t k = (size_t)t - G.first_range, Wg = G.n_ranges;
    const size_t lo = body0 + (n - body0) * k / Wg, hi = body0 + (n - body0) * (k + 1) / Wg;
    size_t o = lo;
    if (PASS == 0) {
        if (k > 0) {
            // The scan for a record start, in two alternating loops so that the lanes of a wavefront stay together: (1) slide an
            // 8-byte window (block_size, refID) to the next offset whose block_size is in [32, 2^24) and whose refID names a
            // reference or none -- cheap, lanes leave it at different trip counts and WAIT for each other at its exit; (2) the
            // full header check and the chain of three more headers -- a dozen dependent loads from cold lines, which all lanes
            // now run at the same time.  (In one loop every lane met its candidate in a different iteration and the wavefront
            // ran the 64 chains one after the other: 0.6 of this kernel's 0.7 ms.)
            // The window is fed eight bytes at a time from 8-byte-aligned loads (the lanes of a wavefront scan 64 different
            // lines: a byte load per step made 8x the gathers), the next eight requested a round ahead.
            bool found = false;
            const size_t n8 = n & ~(size_t)7;                         // (the text buffer is padded by 64 bytes beyond the last stream)
            auto load8 = [&](size_t at) -> uint64_t {                 // bytes [at, at + 8) of the stream, `at` 8-aligned in the text
                uint64_t v = 0;
                if (at + 8 <= n8 + 8) v = *reinterpret_cast<const uint64_t *>(raw + at);
                return v;
            };
            // bring o to where (raw + o) is 8-aligned, byte by byte (at most seven candidates go through the full check directly)
            uint64_t lo8 = 0, hi8 = 0, nxt8 = 0;
            int fed = 0;                                              // bytes of hi8 not yet shifted into lo8
            {
                const size_t mis = (size_t)(reinterpret_cast<uintptr_t>(raw + o) & 7u);
                const size_t o_al = o - mis;                          // (>= 0: the stream's base is 64-aligned and o >= body0 > mis)
                lo8 = load8(o_al) >> (8 * mis);
                hi8 = load8(o_al + 8);
                if (mis) { lo8 |= hi8 << (64 - 8 * mis); hi8 >>= 8 * mis; }
                fed = 8 - (int)mis;
                nxt8 = load8(o_al + 16);
            }
            size_t next_at = o + 8 + (size_t)fed;                     // stream offset of the first byte of nxt8
            auto step = [&]() {                                       // the window moves on by one byte
                lo8 = (lo8 >> 8) | (hi8 << 56);
                hi8 >>= 8;
                if (--fed == 0) { hi8 = nxt8; fed = 8; next_at += 8; nxt8 = load8(next_at); }
                ++o;
            };
            while (!found && o < hi) {
                for (;;) {
                    const uint32_t bs0 = (uint32_t)lo8;
                    const int32_t rid0 = (int32_t)(lo8 >> 32);
                    if (o >= hi || (bs0 >= 32u && bs0 < (1u << 24) && rid0 >= -1 && rid0 < G.n_ref)) break;
                    step();
                }
                if (o >= hi) break;
                {
                    size_t q = o;
                    int good = 0;
                    while (good < 4 && q < n && bam_header_fits(raw, n, q, G.n_ref)) { q += 4 + (size_t)bam_u32(raw + q); ++good; }
                    found = good > 0 && (good == 4 || q == n || (OPEN && bam_open_end(raw, n, q))) && bam_plausible(raw, n, o, G.n_ref);
                }
                if (!found) step();
            }
            if (!found) { rng[t] = BamRange{(uint32_t)hi, (uint32_t)hi, 0u, 2u}; return; }
        }
    } else {
        if (rng[t].state != 1u) return;
        o = rng[t].first;
    }
    size_t q = o;
    uint32_t cnt = 0;
    bool ok = true;
    uint32_t at = PASS == 1 ? base[t] : 0u;
    while (q < hi && q < n) {
        if (q + 4 > n) { ok = OPEN; break; }
        const uint32_t bs = bam_u32(raw + q);
        if (bs < 32 || q + 4 + (size_t)bs > n) { ok = OPEN && bs >= 32; break; }
        if (PASS == 1) { rec_off[at] = (uint32_t)(G.base + q + 4); rec_len[at] = bs; rec_task[at] = (uint16_t)sg; ++at; }
        ++cnt;
        q += 4 + (size_t)bs;
    }
    if (PASS == 0) rng[t] = BamRange{(uint32_t)o, (uint32_t)q, cnt, ok ? 1u : 0u};
}
// the ranges of a task must link up: every walked range begins where the walked range before it stopped (ranges without a record
// start -- a record longer than a range -- are passed over), the first at the first record, the last ends with the stream
template <bool OPEN>
__device__ __forceinline__ void bam_link_range(const unsigned char *__restrict__ text, const BamRange *__restrict__ rng, const BamSeg *__restrict__ segs,
                                               int n_seg, int W, uint32_t *__restrict__ cnt, BamCtl *ctl) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= W) return;
    const BamRange r = rng[t];
    cnt[t] = r.state == 1u ? r.count : 0u;
    if (r.state == 2u) return;
    if (r.state != 1u) { bam_decline(ctl, HGX_FE_DECLINE_RECORD); return; }
    const BamSeg G = segs[bam_seg_of(segs, n_seg, (uint32_t)t)];
    const int r0 = (int)G.first_range, r1 = r0 + (int)G.n_ranges;
    int p = t - 1;
    while (p >= r0 && rng[p].state == 2u) --p;
    const uint32_t expect = p < r0 ? G.body0 : rng[p].stop;
    if (r.first != expect) { bam_decline(ctl, HGX_FE_DECLINE_RECORD); return; }
    int q = t + 1;
    while (q < r1 && rng[q].state == 2u) ++q;
    if (q != r1) return;
    if (!OPEN) {
        if (r.stop != G.n) bam_decline(ctl, HGX_FE_DECLINE_RECORD);
    } else {
        // the last walked range stopped in front of the first incomplete record: a complete one there means that a range behind
        // it found no record start although it held one
        if (!bam_open_end(text + G.base, G.n, r.stop) && r.stop != G.n) bam_decline(ctl, HGX_FE_DECLINE_RECORD);
        ctl->end = r.stop;
    }
}
__attribute__((unused)) __global__ void __launch_bounds__(256) k_bam_link(const BamRange *__restrict__ rng, const BamSeg *__restrict__ segs, int n_seg, int W,
                                                  uint32_t *__restrict__ cnt, BamCtl *ctl) {
    bam_link_range<false>(nullptr, rng, segs, n_seg, W, cnt, ctl);
}
__attribute__((unused)) __global__ void __launch_bounds__(256) k_bam_link_open(const unsigned char *__restrict__ text, const BamRange *__restrict__ rng,
                                                       const BamSeg *__restrict__ segs, int n_seg, int W, uint32_t *__restrict__ cnt, BamCtl *ctl) {
    bam_link_range<true>(text, rng, segs, n_seg, W, cnt, ctl);
}
}   // namespace

// hgx_align.hip -- the "hgx" aligner's kernels (gfx950, wave64).  The per-anchor search, the pick and the record
// text are the core's (hgx_align_core.hpp), the same code the host route runs; this unit is the index in HBM, the grids and the
// fixed-size scratch.  Stages of one chunk of reads:
//   k_aln_seed     a lane per (read, strand, seed offset): the 16-mer's code, the probe of the open-addressing table, one anchor
//                  slot per hit (HGX_ALN_DEV_ANCHORS per read; a read with more declines the call)
//   k_aln_extend   a lane per anchor slot: canon(a) by the core's depth-first search, scratch in the lane's private memory; a limit
//                  reached raises the decline code and writes nothing
//   k_aln_pick     a lane per read: the smallest canon(a) and NH
//   k_aln_pair_pick  (paired input with opts.pair = 1 only) a wavefront per pair: where a combination of the two mates' canon(a) is
//                  concordant, best[] and nh[] of both mates are rewritten from the smallest one (the core's pair order)
//   k_aln_emit     a lane per read, twice: record sizes, (exclusive scan,) then the SAM lines at their offsets; the pair's flags are
//                  read off the mate's pick
//   (opts.clip > 0 or hgx_align_more.gap > 0 only) the FALLBACK TIER between the picks and k_aln_emit, for the reads with anchors and
//                  no alignment: k_aln_tier_mark / _fill / _extend<T> / _pick<T>, below.  One tier, two instances: T = ClipTier or
//                  GapTier names the canon, the pick, the lane's scratch and what a read's extra word means; a call runs one of them,
//                  or (hgx_align_more.rescue_clip > 0) both as two passes with k_aln_tier_keep / k_aln_tier_choose around the second
// Every write is bounds-checked by construction: slots < HGX_ALN_DEV_ANCHORS, a record's bytes = the size the same code counted.
//
// opts.search != 0 adds a second tier, the search over STATES (hgx_align_states.hpp), for the reads of a chunk that are MARKED: in
// "states" a read that passes the anchor slots, or an anchor of which reaches the stack or step limit (k_aln_extend marks instead
// of raising the decline word); in "states_all" every read with an anchor (k_aln_extend does not run).  Per chunk with a mark:
//   k_aln_seed_marked   a lane per (marked read, strand, seed offset), twice: hits counted, (exclusive scan,) the anchors written
//                       at their offsets -- the read's FULL list, capped only in total (ST_ANCHOR_CAP: HGX_ALN_DECLINE_ANCHORS)
//   k_aln_task_info     a lane per (marked read, strand, locus): its anchors' count and the hull of their diagonals.  The host
//                       turns the non-empty ones into tasks: the window (wider than HGX_ALN_STATES_MAX_WINDOW: DECLINE_WINDOW),
//                       the offset of the task's two tables in the scratch, batches that fit ST_CELL_BUDGET cells
//   k_aln_states        a workgroup per task: lanes across the window's columns, rows in sequence (right row L - t and left row t
//                       in step t, one barrier per step); then every anchor's canon by two lookups, the task's best and placements
//   k_aln_states_pick   a lane per marked read: its tasks' bests combined (hgx_st_combine) into the read's first res slot,
//                       best[i], nh[i]; k_aln_pick leaves marked reads alone
// Tables live in HBM / L2 (16 B per cell): a row reads the rows within the longest known insertion + 1 of it, and the lists are
// read back from any row, so an LDS ring would not spare the table.  Every index into the scratch is bounded by
// the numbers the host sized it with: the task's window, read length and cell offset.
#include <hipcub/hipcub.hpp>

#include "hgx_common.hpp"
#include "hgx_align.hpp"
#include "hgx_reads.hpp"

namespace {
typedef hgx_aln_res<HGX_ALN_DEV_VARS> DevRes;
constexpr int CHUNK = 8192;           // reads per chunk (an even number: mates stay together)
constexpr long ST_ANCHOR_CAP = (long)CHUNK * HGX_ALN_DEV_ANCHORS;      // anchors of a chunk's marked reads, in total
constexpr size_t ST_CELL_BUDGET = (size_t)1 << 26;                     // table cells of the tasks in flight (1 GiB)

typedef hgx_dev_reads DevReads;          // (hgx_reads.hpp: the read table in HBM, uploaded here or made there by hgx_reads.hip)

// the device buffers of one chunk, made once per call (hgx_align_device) and handed to the tiers
struct Chunk {
    int32_t *cnt;                     // per read: anchors found
    int2 *anch;                       // per slot (read * HGX_ALN_DEV_ANCHORS + k)
    DevRes *res;                      // per slot: canon(a)
    int32_t *best, *nh;               // per read: the pick
    int32_t *mark;                    // per read: marked for the states tier (opts.search; else nullptr)
    // the fallback tier's (nullptr without one)
    uint32_t *slot_word, *read_word;  // the tier's extra word (clip counts / gap descriptor) per slot and of the read's pick
    uint32_t *nslot, *soff;           // per read: slots to extend, their first compacted index
    int32_t *compact;                 // per compacted index: the slot
    void *scan;                       // hgx_scan_u32_dev's scratch
    int *decline;                     // the chunk's decline word
    uint32_t *total;                  // a scan's total
    // both tiers (rescue_clip > 0; nullptr otherwise): read_word holds 2 * nc words of a chunk, the clip pass's and, nc words
    // behind them, the gap pass's
    uint32_t *nslot2;                 // per read: slots of the gap pass (0: the cost rule or the first mark kept it out)
    DevRes *kept;                     // per read: the clip pass's pick, kept while the gap pass reuses the read's slots of res[]
    int32_t *kept_nh, *cost;          // per read: its NH and cost(C) = clipL + clipR + NM (RESCUE_NONE: the clip pass left it unaligned)
};

__global__ void __launch_bounds__(256)
k_aln_seed(hgx_aln_view V, DevReads rd, long first, int nc, int n_off_max, int32_t *cnt, int2 *anch) {
    const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (long)nc * 2 * n_off_max) return;
    const int k = (int)(gid % n_off_max), strand = (int)((gid / n_off_max) & 1), i = (int)(gid / (2L * n_off_max));
    const int L = rd.len[first + i];
    if (k >= hgx_aln_n_offsets(L)) return;
    const hgx_aln_read R{rd.text + rd.seq_off[first + i], L, strand};
    const int o = hgx_aln_offset(L, k);
    uint32_t code;
    if (!hgx_aln_seed_code(R, o, &code)) return;
    for (uint32_t h = hgx_aln_hash(code) & V.hmask; V.hpos[h] >= 0; h = (h + 1) & V.hmask) {
        if (V.hkey[h] != code) continue;
        const int slot = atomicAdd(&cnt[i], 1);
        if (slot < HGX_ALN_DEV_ANCHORS) anch[(long)i * HGX_ALN_DEV_ANCHORS + slot] = make_int2(o | (strand << 16), V.hpos[h]);
    }
}

// MARK (search "states"): a read past the anchor slots, or an anchor at the stack or step limit, marks its read for the second tier
// instead of raising the decline word; decline[2] counts the reads marked.  MARK = false is the kernel as it was.
template <bool MARK> __global__ void __launch_bounds__(64)
k_aln_extend(hgx_aln_view V, DevReads rd, long first, int nc, int max_edits, const int32_t *cnt, const int2 *anch, DevRes *res,
             int *decline, int32_t *mark) {
    const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (long)nc * HGX_ALN_DEV_ANCHORS) return;
    const int i = (int)(gid / HGX_ALN_DEV_ANCHORS), slot = (int)(gid % HGX_ALN_DEV_ANCHORS);
    const int n = cnt[i];
    if (n > HGX_ALN_DEV_ANCHORS) {
        if (slot == 0) {
            if constexpr (MARK) { if (atomicExch(&mark[i], 1) == 0) atomicAdd(decline + 2, 1); }
            else atomicMax(decline, HGX_ALN_DECLINE_ANCHORS);
        }
        return;
    }
    if (slot >= n) return;
    hgx_aln_frame stk[HGX_ALN_DEV_STK];
    int32_t cur[HGX_ALN_DEV_VARS];
    hgx_aln_side<HGX_ALN_DEV_VARS> side;
    hgx_aln_no_memo memo;
    const int2 a = anch[gid];
    const hgx_aln_read R{rd.text + rd.seq_off[first + i], rd.len[first + i], a.x >> 16};
    const int rc = hgx_aln_canon<HGX_ALN_DEV_STK, HGX_ALN_DEV_VARS>(V, R, a.x & 0xffff, a.y, max_edits, HGX_ALN_DEV_STEPS, stk, cur, side,
                                                                   res[gid], memo);
    if (rc) {
        res[gid].ok = 0;
        if (MARK && (rc == HGX_ALN_DECLINE_STACK || rc == HGX_ALN_DECLINE_STEPS)) { if (atomicExch(&mark[i], 1) == 0) atomicAdd(decline + 2, 1); }
        else atomicMax(decline, rc);
    }
}

__global__ void __launch_bounds__(64)
k_aln_pick(int nc, const int32_t *cnt, const DevRes *res, int32_t *best, int32_t *nh, const int32_t *mark) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nc) return;
    if (mark && mark[i]) return;                   // k_aln_states_pick's
    const int n = cnt[i] < HGX_ALN_DEV_ANCHORS ? cnt[i] : HGX_ALN_DEV_ANCHORS;
    int h = 0;
    best[i] = hgx_aln_pick(res + (long)i * HGX_ALN_DEV_ANCHORS, n, &h);
    nh[i] = h;
}

// opts.pair = 1: the pair pick (hgx_align_core.hpp), one wavefront (= one workgroup) per pair over the two mates' slots.  LDS per
// pair: the 2 x 128 slot heads (8 KB), their in-use marks, starts and placements (0.75 KB), the 128 x 128-bit set of (placement, placement)
// (2 KB) -- 10.75 KB, so a CU's 160 KB hold 14 pairs.  Lanes run over mate 1's slots, each with a loop over mate 2's; the lists stay in
// global memory and are read only where two combinations tie in everything else.  Every index is a slot below HGX_ALN_DEV_ANCHORS.
// pairs[0 .. 2]: pairs searched, placed, changed.
__device__ inline int pp_cmp(const hgx_aln_head (*h)[HGX_ALN_DEV_ANCHORS], const DevRes *r1, const DevRes *r2, int x, int y) {
    return hgx_aln_pair_cmp(h[0][x >> 8], r1[x >> 8].vl, h[1][x & 255], r2[x & 255].vl, h[0][y >> 8], r1[y >> 8].vl, h[1][y & 255],
                            r2[y & 255].vl);
}

__global__ void __launch_bounds__(64)
k_aln_pair_pick(int nc, int max_fragment, const int32_t *cnt, const DevRes *res, int32_t *best, int32_t *nh, unsigned long long *pairs) {
    constexpr int N = HGX_ALN_DEV_ANCHORS;
    __shared__ hgx_aln_head s_h[2][N];
    __shared__ uint8_t s_used[2][N], s_start[2][N], s_place[2][N];
    __shared__ uint32_t s_set[N * N / 32];
    const int lane = threadIdx.x, i = 2 * blockIdx.x, j = i + 1;
    if (j >= nc || best[i] < 0 || best[j] < 0) return;                 // (the whole wavefront)
    const int n[2] = {cnt[i] < N ? cnt[i] : N, cnt[j] < N ? cnt[j] : N};
    const DevRes *r[2] = {res + (long)i * N, res + (long)j * N};
    for (int k = lane; k < 2 * N; k += 64) {
        const int m = k / N, e = k % N;
        hgx_aln_head h{0, 0, 0, 0, 0, 0, 0, 0};
        if (e < n[m]) {
            const int4 *p = (const int4 *)&r[m][e];                   // (a DevRes is 160 bytes: 16-byte aligned)
            const int4 lo = p[0], hi = p[1];
            h = hgx_aln_head{lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
        }
        s_h[m][e] = h;
        s_used[m][e] = 0;
    }
    for (int k = lane; k < N * N / 32; k += 64) s_set[k] = 0;
    __syncthreads();
    // the smallest sums over the concordant combinations, then the smallest combination among those that have them
    uint64_t sums = ~0ull;
    for (int a = lane; a < n[0]; a += 64) {
        const hgx_aln_head h1 = s_h[0][a];
        if (!h1.ok) continue;
        for (int b = 0; b < n[1]; ++b)
            if (hgx_aln_concordant(h1, s_h[1][b], max_fragment)) {
                const uint64_t s = hgx_aln_pair_sums(h1, s_h[1][b]);
                sums = s < sums ? s : sums;
            }
    }
    for (int d = 32; d; d >>= 1) {
        const uint64_t o = (uint64_t)__shfl_xor((long long)sums, d, 64);
        sums = o < sums ? o : sums;
    }
    if (lane == 0) atomicAdd(pairs, 1ull);
    if (sums == ~0ull) return;                                         // no concordant combination: the independent picks stand
    const int nm = hgx_aln_pair_sums_nm(sums);
    int win = -1;                                                      // slot of c1 << 8 | slot of c2
    for (int a = lane; a < n[0]; a += 64) {
        const hgx_aln_head h1 = s_h[0][a];
        if (!h1.ok) continue;
        for (int b = 0; b < n[1]; ++b) {
            if (!hgx_aln_concordant(h1, s_h[1][b], max_fragment) || h1.nm + s_h[1][b].nm != nm) continue;
            s_used[0][a] = 1;                                          // (several lanes may write the same 1 to mate 2's)
            s_used[1][b] = 1;
            if (hgx_aln_pair_sums(h1, s_h[1][b]) != sums) continue;
            const int x = (a << 8) | b;
            if (win < 0 || pp_cmp(s_h, r[0], r[1], x, win) < 0) win = x;
        }
    }
    for (int d = 32; d; d >>= 1) {
        const int o = __shfl_xor(win, d, 64);
        if (o < 0) continue;
        const int c = win < 0 ? -1 : pp_cmp(s_h, r[0], r[1], o, win);
        if (c < 0 || (c == 0 && o < win)) win = o;                     // (equal combinations: the same canon through two anchors)
    }
    __syncthreads();
    // placements of the candidates in use: which of them start one, then each one's start
    for (int k = lane; k < 2 * N; k += 64) {
        const int m = k / N, e = k % N;
        if (e >= n[m] || !s_used[m][e]) continue;
        const hgx_aln_head he = s_h[m][e];
        int start = 1;
        for (int x = 0; x < n[m] && start; ++x)
            if (s_used[m][x] && hgx_aln_covers(s_h[m][x], x, he, e)) start = 0;
        s_start[m][e] = (uint8_t)start;
    }
    __syncthreads();
    for (int k = lane; k < 2 * N; k += 64) {
        const int m = k / N, e = k % N;
        if (e >= n[m] || !s_used[m][e]) continue;
        const hgx_aln_head he = s_h[m][e];
        int p = e;                                                     // the last start at or before e on its locus and strand
        if (!s_start[m][e]) {
            p = -1;
            for (int x = 0; x < n[m]; ++x)
                if (s_used[m][x] && s_start[m][x] && s_h[m][x].locus == he.locus && s_h[m][x].strand == he.strand &&
                    hgx_aln_before(s_h[m][x], x, he, e) && (p < 0 || hgx_aln_before(s_h[m][p], p, s_h[m][x], x))) p = x;
        }
        s_place[m][e] = (uint8_t)(p < 0 ? e : p);                      // (p < 0 cannot be: the first in order is a start)
    }
    __syncthreads();
    for (int a = lane; a < n[0]; a += 64) {
        const hgx_aln_head h1 = s_h[0][a];
        if (!h1.ok || !s_used[0][a]) continue;
        for (int b = 0; b < n[1]; ++b)
            if (s_used[1][b] && h1.nm + s_h[1][b].nm == nm && hgx_aln_concordant(h1, s_h[1][b], max_fragment)) {
                const int bit = (int)s_place[0][a] * N + s_place[1][b];
                atomicOr(&s_set[bit >> 5], 1u << (bit & 31));
            }
    }
    __syncthreads();
    int count = 0;
    for (int k = lane; k < N * N / 32; k += 64) count += __popc(s_set[k]);
    for (int d = 32; d; d >>= 1) count += __shfl_xor(count, d, 64);
    if (lane == 0 && win >= 0) {                                       // (win < 0 cannot be: some combination has `sums`)
        const int a = win >> 8, b = win & 255;
        const DevRes &o1 = r[0][best[i]], &o2 = r[1][best[j]];
        const bool changed = hgx_aln_res_cmp(r[0][a], o1) != 0 || hgx_aln_res_cmp(r[1][b], o2) != 0 || nh[i] != count || nh[j] != count;
        best[i] = a; best[j] = b;
        nh[i] = count; nh[j] = count;
        atomicAdd(pairs + 1, 1ull);
        if (changed) atomicAdd(pairs + 2, 1ull);
    }
}

// out == nullptr: sizes[i] and flags[i] (1 aligned, 2 = mate 1 of a concordant pair); else the line at out + off[i].  word[i] = the
// read's extra word from the fallback tier (nullptr without one).  CLIP (opts.clip > 0): its clip counts for the S ops; GAP (gap > 0):
// its gap descriptor (0: none).  CLIP and GAP (both tiers): two word arrays, the clip counts in word[0 .. nc) and the gap descriptors
// in word[nc .. 2 nc); at most one of a read's two is non-zero.
template <bool CLIP, bool GAP = false> __global__ void __launch_bounds__(64)
k_aln_emit(hgx_aln_view V, DevReads rd, long first, int nc, int max_fragment, const DevRes *res, const int32_t *best, const int32_t *nh,
           uint32_t *sizes, int32_t *flags, const uint32_t *off, char *out, const uint32_t *word) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nc) return;
    if (best[i] < 0) {
        if (!out) { sizes[i] = 0; flags[i] = 0; }
        return;
    }
    const DevRes &a = res[(long)i * HGX_ALN_DEV_ANCHORS + best[i]];
    DevRes none;
    none.ok = 0;
    const DevRes *mate = nullptr;
    if (rd.paired) {
        const int j = i ^ 1;
        mate = best[j] >= 0 ? &res[(long)j * HGX_ALN_DEV_ANCHORS + best[j]] : &none;
    }
    const long r = first + i;
    hgx_aln_out w{out ? out + off[i] : nullptr, 0};
    const uint32_t cc = CLIP || GAP ? word[i] : 0;
    uint32_t gd = GAP ? cc : 0;
    if constexpr (CLIP && GAP) gd = word[(long)nc + i];
    hgx_aln_line<HGX_ALN_DEV_VARS, CLIP, GAP>(V, rd.text + rd.name_off[r], rd.name_len[r], rd.text + rd.seq_off[r],
                                              rd.qual_off[r] >= 0 ? rd.text + rd.qual_off[r] : nullptr, rd.len[r], a, nh[i], mate, i & 1,
                                              max_fragment, w, CLIP ? hgx_aln_clip_l(cc) : 0, CLIP ? hgx_aln_clip_r(cc) : 0, gd);
    if (!out) {
        sizes[i] = (uint32_t)w.n;
        flags[i] = 1 | ((rd.paired && !(i & 1) && hgx_aln_concordant(a, *mate, max_fragment)) ? 2 : 0);
    }
}

// ---- coordinate order (hgx_align_more.order = 1; the rule in plain Python: tests/align_resident_ref.py) ------------------------------
// The chunks' text stays in HBM, one buffer per chunk.  Behind a chunk's k_aln_emit passes:
//   k_aln_rec_keys      a lane per read: entry first + i of the call's record table -- key (index of RNAME << 32 | POS - 1, from the
//                       pick that k_aln_emit printed: hgx_aln_coord_key; REC_NONE for a read without a record), place (chunk << 32 |
//                       offset in the chunk's text), length (0 without a record) and the entry's own index
// and after the last chunk, over the n entries: one stable radix sort of (key, index) -- ties keep input order --,
//   k_aln_rec_lens      a lane per sorted entry: its length, for the exclusive scan that gives every line's offset in the ordered text
//   k_aln_gather_lines  a wavefront per sorted entry: the line's bytes from its chunk's text to its offset, lanes across the bytes
//                       (source and destination are unaligned and unrelated; lines are 150 - 900 bytes)
// No atomic decides a position and nothing passes between workgroups.  Every table index is below n, every source byte inside its
// chunk's text (offset + length <= the chunk's total, both from the scan that placed the line), every destination byte below the
// chunks' totals summed (the scan of the same lengths in another order).
// A read without a record has the key n_loci << 32, behind every record's: the sort runs over the bits that n_loci << 32 has.
__global__ void __launch_bounds__(256)
k_aln_rec_keys(hgx_aln_view V, long first, int nc, uint32_t chunk, const DevRes *res, const int32_t *best, const uint32_t *sizes,
               const uint32_t *off, unsigned long long *key, unsigned long long *place, uint32_t *len, uint32_t *idx) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nc) return;
    const long r = first + i;
    const bool has = best[i] >= 0;
    key[r] = has ? hgx_aln_coord_key(V, res[(long)i * HGX_ALN_DEV_ANCHORS + best[i]]) : (unsigned long long)V.n_loci << 32;
    place[r] = ((unsigned long long)chunk << 32) | (has ? off[i] : 0u);
    len[r] = has ? sizes[i] : 0u;
    idx[r] = (uint32_t)r;
}

__global__ void __launch_bounds__(256) k_aln_rec_lens(const uint32_t *sorted, uint32_t n, const uint32_t *len, uint32_t *out) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) out[j] = len[sorted[j]];
}

__global__ void __launch_bounds__(256)
k_aln_gather_lines(const uint32_t *sorted, uint32_t n, const unsigned long long *place, const uint32_t *len, const uint32_t *dst_off,
                   const char *const *chunk_text, char *out) {
    const uint32_t j = blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64;
    if (j >= n) return;                                                // (the whole wavefront)
    const uint32_t e = sorted[j], L = len[e];
    const unsigned long long p = place[e];
    const char *src = chunk_text[p >> 32] + (uint32_t)p;
    char *dst = out + dst_off[j];
    for (uint32_t b = threadIdx.x & 63; b < L; b += 64) dst[b] = src[b];
}

// ---- the fallback tier (opts.clip > 0: ClipTier, "soft clips"; hgx_align_more.gap > 0: GapTier, "novel gaps"; hgx_align_core.hpp) ----
// For a chunk that holds a read with anchors that k_aln_pick left unaligned: a dearer canon over the same anchor slots, the pick
// again, and one extra word per read for k_aln_emit.  Count, scan, fill -- no atomic decides a position:
//   k_aln_tier_mark       a lane per read: nslot[i] = its anchor slots if it has some and no alignment, else 0
//   (hgx_scan_u32_dev)    soff[i] = the read's first compacted slot, the total
//   k_aln_tier_fill       a lane per (read, slot): compact[soff[i] + slot] = the slot's index in res[]
//   k_aln_tier_extend<T>  a lane per compacted slot: T's canon into res[] and slot_word[]; a limit reached raises the decline word
//   k_aln_tier_pick<T>    a lane per read with nslot[i] > 0: T's pick and NH over its slots, best[], nh[], read_word[]
// A tier T names: canon() with the lane's private scratch as its own arrays (arrays, not one struct: as a struct the compiler lays
// the lane's memory out otherwise and the kernels' registers and occupancy move), pick() and bases() (what a read's word counts
// for, the third counter).  Every loop bound is the read length, the slot count, max_edits + 1,
// the longest gap, the options at a position or the step limit; every index is a slot below nc * HGX_ALN_DEV_ANCHORS or a compacted
// slot below the scan's total.
//
// ClipTier: the clip canon by the core's CLIP walks; the word = the clip counts.  Scratch: the per-e entries of both sides (2 x 5
// entries of 37 words), the stack of 32 frames of 6 words and the list of 32: 2 376 bytes per lane.
struct ClipTier {
    static constexpr int id = HGX_ALN_TIER_CLIP;
    static __device__ int canon(const hgx_aln_view &V, const hgx_aln_read &R, int o, int32_t b, int max_edits, int clip, DevRes &res, uint32_t *word) {
        hgx_aln_frame stk[HGX_ALN_DEV_STK];
        int32_t cur[HGX_ALN_DEV_VARS];
        hgx_aln_side<HGX_ALN_DEV_VARS> left[HGX_ALN_CLIP_EDITS + 1], right[HGX_ALN_CLIP_EDITS + 1];
        return hgx_aln_clip_canon<HGX_ALN_DEV_STK, HGX_ALN_DEV_VARS>(V, R, o, b, max_edits, clip, HGX_ALN_DEV_STEPS, stk, cur, left, right, res, word);
    }
    static __device__ int pick(const DevRes *res, int n, int *nh, const uint32_t *words) {
        return hgx_aln_pick<HGX_ALN_DEV_VARS, true>(res, n, nh, words);
    }
    static int bases(uint32_t word) { return hgx_aln_clip_total(word); }
};
// GapTier: the gap canon by the core's GAP walks; the word = the gap descriptor.  Scratch: the outer and the inner walks' stacks
// (2 x 32 frames of 6 words) and lists (2 x 32), three side entries of 37 words: 2 236 bytes per lane.  The step limit is one per
// side, shared by its inner walks.
struct GapTier {
    static constexpr int id = HGX_ALN_TIER_GAP;
    static __device__ int canon(const hgx_aln_view &V, const hgx_aln_read &R, int o, int32_t b, int max_edits, int gap, DevRes &res, uint32_t *word) {
        hgx_aln_frame stk[HGX_ALN_DEV_STK], stk2[HGX_ALN_DEV_STK];
        int32_t cur[HGX_ALN_DEV_VARS], cur2[HGX_ALN_DEV_VARS];
        hgx_aln_side<HGX_ALN_DEV_VARS> sides[3];
        return hgx_aln_gap_canon<HGX_ALN_DEV_STK, HGX_ALN_DEV_VARS>(V, R, o, b, max_edits, gap, HGX_ALN_DEV_STEPS, stk, cur, stk2, cur2, sides, res,
                                                                   word);
    }
    static __device__ int pick(const DevRes *res, int n, int *nh, const uint32_t *words) { return hgx_aln_gap_pick(res, n, nh, words); }
    static int bases(uint32_t word) { return hgx_aln_gap_len(word); }
};

__global__ void __launch_bounds__(256)
k_aln_tier_mark(int nc, const int32_t *cnt, const int32_t *best, uint32_t *nslot) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nc) return;
    nslot[i] = (best[i] < 0 && cnt[i] > 0 && cnt[i] <= HGX_ALN_DEV_ANCHORS) ? (uint32_t)cnt[i] : 0u;
}

__global__ void __launch_bounds__(256)
k_aln_tier_fill(int nc, const uint32_t *nslot, const uint32_t *soff, uint32_t total, int32_t *compact) {
    const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (long)nc * HGX_ALN_DEV_ANCHORS) return;
    const int i = (int)(gid / HGX_ALN_DEV_ANCHORS);
    const uint32_t slot = (uint32_t)(gid % HGX_ALN_DEV_ANCHORS);
    if (slot >= nslot[i] || soff[i] + slot >= total) return;
    compact[soff[i] + slot] = (int32_t)gid;
}

template <class T> __global__ void __launch_bounds__(64)
k_aln_tier_extend(hgx_aln_view V, DevReads rd, long first, uint32_t total, int max_edits, int budget, const int32_t *compact, const int2 *anch,
                  DevRes *res, uint32_t *slot_word, int *decline) {
    const long j = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= (long)total) return;
    const int32_t gid = compact[j];
    const int i = gid / HGX_ALN_DEV_ANCHORS;
    const int2 a = anch[gid];
    const hgx_aln_read R{rd.text + rd.seq_off[first + i], rd.len[first + i], a.x >> 16};
    uint32_t w = 0;
    const int rc = T::canon(V, R, a.x & 0xffff, a.y, max_edits, budget, res[gid], &w);
    slot_word[gid] = w;
    if (rc) {
        res[gid].ok = 0;
        atomicMax(decline, rc);
    }
}

template <class T> __global__ void __launch_bounds__(64)
k_aln_tier_pick(int nc, const uint32_t *nslot, const DevRes *res, const uint32_t *slot_word, int32_t *best, int32_t *nh, uint32_t *read_word) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nc || nslot[i] == 0) return;
    int h = 0;
    const int b = T::pick(res + (long)i * HGX_ALN_DEV_ANCHORS, (int)nslot[i], &h, slot_word + (long)i * HGX_ALN_DEV_ANCHORS);
    best[i] = b;
    nh[i] = h;
    read_word[i] = b >= 0 ? slot_word[(long)i * HGX_ALN_DEV_ANCHORS + b] : 0u;
}

// ---- both tiers in one call (hgx_align_more.rescue_clip > 0; the rule in plain Python: tests/align_rescue_ref.py) ----------------
// The clip pass runs first (the cheap one) over the reads k_aln_tier_mark marks, then, a lane per read:
//   k_aln_tier_keep     for a marked read: the clip pick's DevRes and NH into kept[] / kept_nh[] (the gap pass writes its canons into
//                       the same slots of res[]) and cost[i] = clipL + clipR + NM, RESCUE_NONE if the clip pass left it unaligned;
//                       for every read: nslot2[i], the gap pass's mark = the read's slots if it is marked and cost[i] >= 2 (a gap
//                       costs at least 1 and a tie goes to the clip), else 0
//   (the gap pass)      scan, fill, extend, pick over nslot2[] as they are, with the gap words behind the clip words
//   k_aln_tier_choose   for a read of the gap pass: the gap's pick stands iff it exists and its NM < cost[i] (the clip word is
//                       zeroed); else, if the clip pass aligned the read, kept[i] goes back into the read's slot 0 with best[],
//                       nh[] and the gap word zeroed; else the read stays unaligned
// Every index is a read below nc or the read's own slot 0 of res[].
constexpr int32_t RESCUE_NONE = INT32_MAX;

__global__ void __launch_bounds__(64)
k_aln_tier_keep(int nc, const uint32_t *nslot, const DevRes *res, const int32_t *best, const int32_t *nh, const uint32_t *clip_word, DevRes *kept,
                int32_t *kept_nh, int32_t *cost, uint32_t *nslot2) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nc) return;
    uint32_t n2 = 0;
    if (nslot[i] > 0) {
        int32_t c = RESCUE_NONE;
        if (best[i] >= 0) {
            const DevRes &a = res[(long)i * HGX_ALN_DEV_ANCHORS + best[i]];
            kept[i] = a;
            kept_nh[i] = nh[i];
            c = hgx_aln_clip_total(clip_word[i]) + a.nm;
        }
        cost[i] = c;
        if (c >= 2) n2 = nslot[i];
    }
    nslot2[i] = n2;
}

__global__ void __launch_bounds__(64)
k_aln_tier_choose(int nc, const uint32_t *nslot2, const DevRes *kept, const int32_t *kept_nh, const int32_t *cost, DevRes *res, int32_t *best,
                  int32_t *nh, uint32_t *clip_word, uint32_t *gap_word) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nc || nslot2[i] == 0) return;                 // (not in the gap pass: the clip pass's pick, or none, stands)
    const int32_t c = cost[i];
    if (best[i] >= 0 && res[(long)i * HGX_ALN_DEV_ANCHORS + best[i]].nm < c) clip_word[i] = 0;
    else if (c != RESCUE_NONE) {
        res[(long)i * HGX_ALN_DEV_ANCHORS] = kept[i];
        best[i] = 0;
        nh[i] = kept_nh[i];
        gap_word[i] = 0;
    }
}

// one pass of tier T over the reads `nslot` marks, into `read_word`: scan, fill, extend, pick.  *total = 0: no read is marked and
// nothing ran; *decline != 0: a limit was reached.
template <class T>
int tier_pass(hgx_align_index *ix, const DevReads &rd, int max_edits, int budget, long first, int nc, const Chunk &c, const uint32_t *nslot,
              uint32_t *read_word, hipStream_t st, uint32_t *total, int *decline) {
    const int rc = hgx_scan_u32_dev(nslot, c.soff, nc, c.scan, c.total, st);
    if (rc) return rc;
    *total = 0;
    HIPCHK(hipMemcpy(total, c.total, 4, hipMemcpyDeviceToHost));
    if (!*total) return HGX_OK;
    k_aln_tier_fill<<<nblk((long)nc * HGX_ALN_DEV_ANCHORS, 256), 256, 0, st>>>(nc, nslot, c.soff, *total, c.compact);
    k_aln_tier_extend<T><<<nblk(*total, 64), 64, 0, st>>>(ix->dv, rd, first, *total, max_edits, budget, c.compact, c.anch, c.res, c.slot_word,
                                                          c.decline);
    HIPCHK(hipGetLastError());
    int dec = 0;
    HIPCHK(hipMemcpy(&dec, c.decline, 4, hipMemcpyDeviceToHost));
    if (dec) { *decline = dec; return HGX_OK; }
    k_aln_tier_pick<T><<<nblk(nc, 64), 64, 0, st>>>(nc, nslot, c.res, c.slot_word, c.best, c.nh, read_word);
    HIPCHK(hipGetLastError());
    return HGX_OK;
}

// what a chunk's tiers counted: [tier][reads searched, reads the tier wrote, the bases their words stand for]
typedef int64_t TierCounts[HGX_ALN_N_TIERS][3];

template <class T> void tier_sum(int nc, const uint32_t *nslot, const uint32_t *word, TierCounts counts) {
    for (int i = 0; i < nc; ++i) {
        if (!nslot[i]) continue;
        counts[T::id][0] += 1;
        counts[T::id][1] += word[i] != 0;
        counts[T::id][2] += T::bases(word[i]);
    }
}

// the fallback tier of one chunk, behind k_aln_pick: *decline != 0: the call goes to the host route.  budgets[0 .. 1]: the clip
// tier's and the gap tier's.
template <class T>
int fallback_tier(hgx_align_index *ix, const DevReads &rd, int max_edits, const int *budgets, long first, int nc, const Chunk &c, hipStream_t st,
                  TierCounts counts, int *decline) {
    HIPCHK(hipMemsetAsync(c.read_word, 0, (size_t)nc * 4, st));
    k_aln_tier_mark<<<nblk(nc, 256), 256, 0, st>>>(nc, c.cnt, c.best, c.nslot);
    HIPCHK(hipGetLastError());
    uint32_t total = 0;
    const int rc = tier_pass<T>(ix, rd, max_edits, budgets[T::id == GapTier::id], first, nc, c, c.nslot, c.read_word, st, &total, decline);
    if (rc || !total || *decline) return rc;
    std::vector<uint32_t> nslot((size_t)nc), word((size_t)nc);
    HIPCHK(hipMemcpy(nslot.data(), c.nslot, (size_t)nc * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(word.data(), c.read_word, (size_t)nc * 4, hipMemcpyDeviceToHost));
    tier_sum<T>(nc, nslot.data(), word.data(), counts);
    return HGX_OK;
}

// both tiers of one chunk: the clip pass, the gap pass over the reads the cost rule leaves to it, the choice; the counters are
// summed from what is copied back after the choice
int rescue_tiers(hgx_align_index *ix, const DevReads &rd, int max_edits, const int *budgets, long first, int nc, const Chunk &c, hipStream_t st,
                 TierCounts counts, int *decline) {
    uint32_t *clip_word = c.read_word, *gap_word = c.read_word + nc;
    HIPCHK(hipMemsetAsync(c.read_word, 0, (size_t)nc * 8, st));
    k_aln_tier_mark<<<nblk(nc, 256), 256, 0, st>>>(nc, c.cnt, c.best, c.nslot);
    HIPCHK(hipGetLastError());
    uint32_t total = 0, total2 = 0;
    int rc = tier_pass<ClipTier>(ix, rd, max_edits, budgets[0], first, nc, c, c.nslot, clip_word, st, &total, decline);
    if (rc || !total || *decline) return rc;
    k_aln_tier_keep<<<nblk(nc, 64), 64, 0, st>>>(nc, c.nslot, c.res, c.best, c.nh, clip_word, c.kept, c.kept_nh, c.cost, c.nslot2);
    HIPCHK(hipGetLastError());
    rc = tier_pass<GapTier>(ix, rd, max_edits, budgets[1], first, nc, c, c.nslot2, gap_word, st, &total2, decline);
    if (rc || *decline) return rc;
    if (total2) {
        k_aln_tier_choose<<<nblk(nc, 64), 64, 0, st>>>(nc, c.nslot2, c.kept, c.kept_nh, c.cost, c.res, c.best, c.nh, clip_word, gap_word);
        HIPCHK(hipGetLastError());
    }
    std::vector<uint32_t> nslot((size_t)nc), nslot2((size_t)nc), word((size_t)nc * 2);
    HIPCHK(hipMemcpy(nslot.data(), c.nslot, (size_t)nc * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(nslot2.data(), c.nslot2, (size_t)nc * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(word.data(), c.read_word, (size_t)nc * 8, hipMemcpyDeviceToHost));
    tier_sum<ClipTier>(nc, nslot.data(), word.data(), counts);
    tier_sum<GapTier>(nc, nslot2.data(), word.data() + nc, counts);
    return HGX_OK;
}

// ---- the second tier: the search over states (hgx_align_states.hpp) ------------------------------------------------------------
struct StInfo { int32_t n, dmin, dmax, a0, a1; };                  // of one (marked read, strand, locus): anchors [a0, a1) are the (read, strand)'s
struct StTask {
    int32_t i, strand, locus, a0, a1, wlo, whi;                    // i: the read's index in the chunk
    uint64_t cell_off;                                             // of its right table in the batch's scratch; the left one follows
};

// search "states_all": every read with an anchor
__global__ void __launch_bounds__(256) k_aln_mark_all(int nc, const int32_t *cnt, int32_t *mark, int *misc) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nc || cnt[i] <= 0) return;
    mark[i] = 1;
    atomicAdd(misc + 2, 1);
}

// off == nullptr: n_hits[gid]; else the anchors at off[gid] + 0, 1, ... (below cap)
__global__ void __launch_bounds__(256)
k_aln_seed_marked(hgx_aln_view V, DevReads rd, long first, const int32_t *marked, int n_marked, int n_off_max, uint32_t *n_hits,
                  const uint32_t *off, hgx_st_anchor *anch, long cap) {
    const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (long)n_marked * 2 * n_off_max) return;
    const int k = (int)(gid % n_off_max), strand = (int)((gid / n_off_max) & 1), i = marked[gid / (2L * n_off_max)];
    const int L = rd.len[first + i];
    uint32_t n = 0;
    if (k < hgx_aln_n_offsets(L)) {
        const hgx_aln_read R{rd.text + rd.seq_off[first + i], L, strand};
        const int o = hgx_aln_offset(L, k);
        uint32_t code;
        if (hgx_aln_seed_code(R, o, &code))
            for (uint32_t h = hgx_aln_hash(code) & V.hmask; V.hpos[h] >= 0; h = (h + 1) & V.hmask) {
                if (V.hkey[h] != code) continue;
                if (off && (long)off[gid] + n < cap) anch[off[gid] + n] = hgx_st_anchor{o | (strand << 16), V.hpos[h]};
                ++n;
            }
    }
    if (!off) n_hits[gid] = n;
}

__global__ void __launch_bounds__(256)
k_aln_task_info(hgx_aln_view V, int n_marked, int n_off_max, const uint32_t *off, uint32_t total, const hgx_st_anchor *anch, StInfo *info) {
    const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (long)n_marked * 2 * V.n_loci) return;
    const int g = (int)(gid % V.n_loci);
    const long ms = gid / V.n_loci;                                // marked read * 2 + strand
    const uint32_t a0 = off[ms * n_off_max], a1 = ms + 1 < (long)n_marked * 2 ? off[(ms + 1) * n_off_max] : total;
    const int32_t lo = V.bb_off[g], hi = V.bb_off[g + 1];
    StInfo t{0, INT32_MAX, INT32_MIN, (int32_t)a0, (int32_t)a1};
    for (uint32_t a = a0; a < a1; ++a) {
        const hgx_st_anchor x = anch[a];
        if (x.y < lo || x.y >= hi) continue;
        const int32_t d = x.y - (x.x & 0xffff);
        ++t.n;
        t.dmin = d < t.dmin ? d : t.dmin;
        t.dmax = d > t.dmax ? d : t.dmax;
    }
    info[gid] = t;
}

__device__ inline unsigned long long st_key(const int4 c, int32_t lo) {      // (NM, indels, variants, pos0) of a stored cost, in order
    return ((unsigned long long)c.x << 54) | ((unsigned long long)(c.w >> 16) << 42) | ((unsigned long long)(c.w & 0xffff) << 30) |
           (unsigned long long)(c.y - lo);
}

// acost[a] = (NM or -1, pos0, end, indels << 16 | variants) of anchor a, written by the one task whose locus holds it
__global__ void __launch_bounds__(256)
k_aln_states(hgx_aln_view V, DevReads rd, long first, int max_edits, const StTask *tasks, const hgx_st_anchor *anch, int4 *acost,
             hgx_st_cell *scratch, DevRes *tres, int32_t *tnh, int *decline) {
    __shared__ unsigned long long s_key;
    __shared__ int s_flag, s_nh;
    const StTask tk = tasks[blockIdx.x];
    const int tid = threadIdx.x, L = rd.len[first + tk.i];
    hgx_st_task T;
    T.R = hgx_aln_read{rd.text + rd.seq_off[first + tk.i], L, tk.strand};
    T.lo = V.bb_off[tk.locus]; T.hi = V.bb_off[tk.locus + 1];
    T.wlo = tk.wlo; T.whi = tk.whi;
    T.stride = tk.whi - tk.wlo + 1;
    T.max_edits = max_edits < L ? max_edits : L;
    T.right = scratch + tk.cell_off;
    T.left = T.right + hgx_st_table_cells(L, tk.whi - tk.wlo);
    if (tid == 0) { s_key = ~0ull; s_flag = 0; s_nh = 0; }
    const int W = tk.whi - tk.wlo;
    for (int t = 0; t < L; ++t) {
        for (int col = tid; col <= W; col += blockDim.x) {
            hgx_st_right_cell(V, T, L - t, tk.wlo + col);
            if (col < W) hgx_st_left_cell(V, T, t, tk.wlo + col);
        }
        __threadfence_block();
        __syncthreads();
    }
    // every anchor's canon: two lookups
    for (int a = tk.a0 + tid; a < tk.a1; a += blockDim.x) {
        const hgx_st_anchor x = anch[a];
        if (x.y < T.lo || x.y >= T.hi) continue;
        hgx_st_cost c;
        const int rc = hgx_st_canon_cost(T, x.x & 0xffff, x.y, &c);
        int4 v = make_int4(-1, 0, 0, 0);
        if (rc == HGX_ST_POISONED) atomicMax(&s_flag, HGX_ALN_DECLINE_WINDOW);
        else if (rc) {
            v = make_int4(c.nm, c.pos0, c.end, (c.nind << 16) | c.nvar);
            atomicMin(&s_key, st_key(v, T.lo));
        }
        acost[a] = v;
    }
    __threadfence_block();
    __syncthreads();
    DevRes &res = tres[blockIdx.x];
    if (tid == 0) {
        res.ok = 0;
        int32_t tmp[HGX_ALN_DEV_VARS];
        for (int a = tk.a0; a < tk.a1 && !s_flag && s_key != ~0ull; ++a) {
            const hgx_st_anchor x = anch[a];
            if (x.y < T.lo || x.y >= T.hi) continue;
            const int4 c = acost[a];
            if (c.x < 0 || st_key(c, T.lo) != s_key) continue;
            const int nvar = c.w & 0xffff;
            if (nvar > HGX_ALN_DEV_VARS) { s_flag = HGX_ALN_DECLINE_VARS; break; }
            if (!res.ok) {
                hgx_st_canon_list(V, T, x.x & 0xffff, x.y, res.vl);
                res.ok = 1; res.nm = c.x; res.nind = c.w >> 16; res.nvar = nvar; res.locus = tk.locus; res.strand = tk.strand;
                res.pos0 = c.y; res.end = c.z;
            } else if (nvar > 0) {
                hgx_st_canon_list(V, T, x.x & 0xffff, x.y, tmp);
                int cmp = 0;
                for (int j = 0; cmp == 0 && j < nvar; ++j) cmp = tmp[j] != res.vl[j] ? (tmp[j] < res.vl[j] ? -1 : 1) : 0;
                if (cmp < 0) {
                    for (int j = 0; j < nvar; ++j) res.vl[j] = tmp[j];
                    res.end = c.z;
                }
            }
        }
        if (s_flag) { res.ok = 0; atomicMax(decline, s_flag); }
    }
    __syncthreads();
    if (s_flag || s_key == ~0ull) {
        if (tid == 0) tnh[blockIdx.x] = 0;
        return;
    }
    // placements of the anchors with the task's smallest NM: anchor a starts one iff no anchor before it in (pos0, a) order ends behind a's pos0
    const int nm = (int)(s_key >> 54);
    for (int a = tk.a0 + tid; a < tk.a1; a += blockDim.x) {
        const hgx_st_anchor x = anch[a];
        if (x.y < T.lo || x.y >= T.hi) continue;
        const int4 c = acost[a];
        if (c.x != nm) continue;
        int start = 1;
        for (int b = tk.a0; b < tk.a1 && start; ++b) {
            const hgx_st_anchor y = anch[b];
            if (b == a || y.y < T.lo || y.y >= T.hi) continue;
            const int4 d = acost[b];
            if (d.x != nm) continue;
            if ((d.y < c.y || (d.y == c.y && b < a)) && d.z > c.y) start = 0;
        }
        if (start) atomicAdd(&s_nh, 1);
    }
    __syncthreads();
    if (tid == 0) tnh[blockIdx.x] = s_nh;
}

// t_first[m] .. t_first[m + 1]: the tasks of marked read m
__global__ void __launch_bounds__(64)
k_aln_states_pick(int n_marked, const int32_t *marked, const int32_t *t_first, const DevRes *tres, const int32_t *tnh, DevRes *res,
                  int32_t *best, int32_t *nh) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= n_marked) return;
    const int i = marked[m], t0 = t_first[m], n = t_first[m + 1] - t0;
    int h = 0;
    const int b = hgx_st_combine(tres + t0, tnh + t0, n, &h);
    if (b >= 0) res[(long)i * HGX_ALN_DEV_ANCHORS] = tres[t0 + b];
    best[i] = b >= 0 ? 0 : -1;
    nh[i] = h;
}

// the second tier of one chunk: *decline != 0: the call goes to the host route
int states_tier(hgx_align_index *ix, const int32_t *h_len, const DevReads &rd, const hgx_align_opts *opts, long first, int nc,
                int n_off_max, const Chunk &c, hipStream_t st, int *decline) {
    const hgx_aln_view &V = ix->dv;
    std::vector<int32_t> mark(nc), marked;
    HIPCHK(hipMemcpy(mark.data(), c.mark, (size_t)nc * 4, hipMemcpyDeviceToHost));
    for (int i = 0; i < nc; ++i)
        if (mark[i]) marked.push_back(i);
    const int nm = (int)marked.size();
    if (!nm) return HGX_OK;
    const long n_lanes = (long)nm * 2 * n_off_max;
    DevBuf d_marked, d_hits, d_off, d_scan2, d_anch;
    ALLOC(d_marked, (size_t)nm * 4);
    ALLOC(d_hits, (size_t)n_lanes * 4); ALLOC(d_off, (size_t)n_lanes * 4);
    ALLOC(d_scan2, hgx_scan_u32_scratch_bytes(n_lanes) + 16);
    HIPCHK(hipMemcpy(d_marked.p, marked.data(), (size_t)nm * 4, hipMemcpyHostToDevice));
    k_aln_seed_marked<<<nblk(n_lanes, 256), 256, 0, st>>>(V, rd, first, d_marked.as<int32_t>(), nm, n_off_max, d_hits.as<uint32_t>(), nullptr,
                                                         nullptr, 0);
    HIPCHK(hipGetLastError());
    int rc = hgx_scan_u32_dev(d_hits.as<uint32_t>(), d_off.as<uint32_t>(), n_lanes, d_scan2.p, c.total, st);
    if (rc) return rc;
    uint32_t total = 0;
    HIPCHK(hipMemcpy(&total, c.total, 4, hipMemcpyDeviceToHost));
    if ((long)total > ST_ANCHOR_CAP) { *decline = HGX_ALN_DECLINE_ANCHORS; return HGX_OK; }
    ALLOC(d_anch, (size_t)std::max<uint32_t>(total, 1) * sizeof(hgx_st_anchor));
    k_aln_seed_marked<<<nblk(n_lanes, 256), 256, 0, st>>>(V, rd, first, d_marked.as<int32_t>(), nm, n_off_max, nullptr, d_off.as<uint32_t>(),
                                                         d_anch.as<hgx_st_anchor>(), (long)total);
    const long n_info = (long)nm * 2 * V.n_loci;
    DevBuf d_info;
    ALLOC(d_info, (size_t)n_info * sizeof(StInfo));
    k_aln_task_info<<<nblk(n_info, 256), 256, 0, st>>>(V, nm, n_off_max, d_off.as<uint32_t>(), total, d_anch.as<hgx_st_anchor>(),
                                                      d_info.as<StInfo>());
    HIPCHK(hipGetLastError());
    std::vector<StInfo> info((size_t)n_info);
    HIPCHK(hipMemcpy(info.data(), d_info.p, (size_t)n_info * sizeof(StInfo), hipMemcpyDeviceToHost));
    // the tasks, in (marked read, strand, locus) order; batches whose tables fit the budget
    std::vector<StTask> tasks;
    std::vector<int32_t> t_first(1, 0), batch_first(1, 0);
    size_t in_batch = 0, largest = 0;
    int64_t cells = 0;
    for (int m = 0; m < nm; ++m) {
        const int L = h_len[first + marked[m]];
        for (int sg = 0; sg < 2 * V.n_loci; ++sg) {
            const StInfo &t = info[(size_t)m * 2 * V.n_loci + sg];
            if (t.n <= 0) continue;
            const int g = sg % V.n_loci;
            const int32_t lo = ix->bb_off[g], hi = ix->bb_off[g + 1];
            StTask k{marked[m], sg / V.n_loci, g, t.a0, t.a1, 0, 0, 0};
            hgx_st_window(lo, hi, t.dmin, t.dmax, L, HGX_ALN_STATES_MARGIN, &k.wlo, &k.whi);
            if (k.whi - k.wlo > HGX_ALN_STATES_MAX_WINDOW || hi - lo >= (1 << 30)) { *decline = HGX_ALN_DECLINE_WINDOW; return HGX_OK; }
            const size_t need = 2 * hgx_st_table_cells(L, k.whi - k.wlo);
            if (in_batch && in_batch + need > ST_CELL_BUDGET) { batch_first.push_back((int32_t)tasks.size()); in_batch = 0; }
            k.cell_off = in_batch;
            in_batch += need;
            largest = std::max(largest, in_batch);
            cells += 2 * (int64_t)L * (k.whi - k.wlo);
            tasks.push_back(k);
        }
        t_first.push_back((int32_t)tasks.size());
    }
    batch_first.push_back((int32_t)tasks.size());
    const size_t nt = tasks.size();
    DevBuf d_tasks, d_tf, d_tres, d_tnh, d_acost, d_cells;
    ALLOC(d_tasks, std::max<size_t>(nt, 1) * sizeof(StTask));
    ALLOC(d_tf, t_first.size() * 4);
    ALLOC(d_tres, std::max<size_t>(nt, 1) * sizeof(DevRes));
    ALLOC(d_tnh, std::max<size_t>(nt, 1) * 4);
    ALLOC(d_acost, (size_t)std::max<uint32_t>(total, 1) * sizeof(int4));
    ALLOC(d_cells, std::max<size_t>(largest, 1) * sizeof(hgx_st_cell));
    HIPCHK(hipMemcpy(d_tasks.p, tasks.data(), nt * sizeof(StTask), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_tf.p, t_first.data(), t_first.size() * 4, hipMemcpyHostToDevice));
    for (size_t b = 0; b + 1 < batch_first.size(); ++b) {
        const int t0 = batch_first[b], n = batch_first[b + 1] - t0;
        if (n <= 0) continue;
        k_aln_states<<<n, 256, 0, st>>>(V, rd, first, opts->max_edits, d_tasks.as<StTask>() + t0, d_anch.as<hgx_st_anchor>(), d_acost.as<int4>(),
                                        d_cells.as<hgx_st_cell>(), d_tres.as<DevRes>() + t0, d_tnh.as<int32_t>() + t0, c.decline);
        HIPCHK(hipGetLastError());
    }
    k_aln_states_pick<<<nblk(nm, 64), 64, 0, st>>>(nm, d_marked.as<int32_t>(), d_tf.as<int32_t>(), d_tres.as<DevRes>(), d_tnh.as<int32_t>(), c.res,
                                                   c.best, c.nh);
    HIPCHK(hipGetLastError());
    int dec = 0;
    HIPCHK(hipMemcpy(&dec, c.decline, 4, hipMemcpyDeviceToHost));     // (also: the tier is finished before its buffers go back to the pool)
    if (dec) { *decline = dec; return HGX_OK; }
    hgx_align_states_count(nm, (int64_t)total, cells);
    return HGX_OK;
}

template <class T> size_t put(std::vector<char> &blk, const std::vector<T> &v) {
    const size_t off = (blk.size() + 15) & ~(size_t)15;
    blk.resize(off + std::max<size_t>(v.size() * sizeof(T), 16));
    if (!v.empty()) memcpy(blk.data() + off, v.data(), v.size() * sizeof(T));
    return off;
}

// the index in HBM, made once per index and device
int ensure_device_index(hgx_align_index *ix) {
    std::lock_guard<std::mutex> g(ix->mu);
    int dev = 0;
    HIPCHK(hipGetDevice(&dev));
    if (ix->dev_ready == dev) return HGX_OK;
    if (ix->d_block) { (void)hipFree(ix->d_block); ix->d_block = nullptr; ix->dev_ready = -1; }
    std::vector<char> blk;
    const size_t o_bb = put(blk, ix->bb), o_bo = put(blk, ix->bb_off), o_hk = put(blk, ix->hkey), o_hp = put(blk, ix->hpos),
                 o_vt = put(blk, ix->vtype), o_vp = put(blk, ix->vpos), o_vl = put(blk, ix->vlen), o_vd = put(blk, ix->vdata),
                 o_io = put(blk, ix->vid_off), o_il = put(blk, ix->vid_len), o_no = put(blk, ix->name_off), o_nl = put(blk, ix->name_len),
                 o_pl = put(blk, ix->pool), o_so = put(blk, ix->sgl_off), o_s = put(blk, ix->sgl), o_do = put(blk, ix->dls_off),
                 o_d = put(blk, ix->dls), o_eo = put(blk, ix->dle_off), o_e = put(blk, ix->dle), o_no2 = put(blk, ix->ins_off),
                 o_n = put(blk, ix->ins);
    HIPCHK(hipMalloc(&ix->d_block, blk.size()));
    HIPCHK(hipMemcpy(ix->d_block, blk.data(), blk.size(), hipMemcpyHostToDevice));
    const char *b = (const char *)ix->d_block;
    hgx_aln_view &V = ix->dv;
    V = ix->hv;
    V.bb = b + o_bb; V.bb_off = (const int32_t *)(b + o_bo); V.hkey = (const uint32_t *)(b + o_hk); V.hpos = (const int32_t *)(b + o_hp);
    V.vtype = (const uint8_t *)(b + o_vt); V.vpos = (const int32_t *)(b + o_vp); V.vlen = (const int32_t *)(b + o_vl);
    V.vdata = (const int32_t *)(b + o_vd); V.vid_off = (const int32_t *)(b + o_io); V.vid_len = (const int32_t *)(b + o_il);
    V.name_off = (const int32_t *)(b + o_no); V.name_len = (const int32_t *)(b + o_nl); V.pool = b + o_pl;
    V.sgl_off = (const int32_t *)(b + o_so); V.sgl = (const int32_t *)(b + o_s); V.dls_off = (const int32_t *)(b + o_do);
    V.dls = (const int32_t *)(b + o_d); V.dle_off = (const int32_t *)(b + o_eo); V.dle = (const int32_t *)(b + o_e);
    V.ins_off = (const int32_t *)(b + o_no2); V.ins = (const int32_t *)(b + o_n);
    ix->dev_ready = dev;
    return HGX_OK;
}

// coordinate order: the call's record table and the chunks' text, both in HBM until the last chunk has run
struct Ordered {
    DevBuf key, place, len, idx;               // per read (k_aln_rec_keys)
    std::vector<void *> text;                  // per chunk: its emitted text (nullptr: none)
    std::vector<uint32_t> bytes;               // ... and its size
    hipStream_t st = nullptr;
    ~Ordered() {                               // (whatever way the call returns: the kernels over these buffers have run)
        if (!text.empty()) (void)hipStreamSynchronize(st);
        for (void *p : text) if (p) hgx_pool_free(p);
    }
};

// the table sorted, the lines gathered: the ordered text, `header` in front of it and 64 zeroed bytes behind it with ord->keep (left
// in ord->d_text), else appended to `body`
int order_text(const hgx_align_index *ix, Ordered &O, long n, std::string &body, hgx_aln_ordered *ord, hipStream_t st) {
    size_t total = 0;
    for (uint32_t b : O.bytes) total += b;
    const size_t head = ord->keep ? ix->header.size() : 0;
    if (head + total >= ((size_t)1 << 32) - 64 || n >= (1L << 31)) {       // beyond the 32-bit offsets: input order, the caller sorts the lines
        for (size_t k = 0; k < O.text.size(); ++k) {
            if (!O.bytes[k]) continue;
            const size_t at = body.size();
            body.resize(at + O.bytes[k]);
            HIPCHK(hipMemcpy(&body[at], O.text[k], O.bytes[k], hipMemcpyDeviceToHost));
        }
        ord->unordered = true;
        return HGX_OK;
    }
    const uint32_t nn = (uint32_t)n;
    DevBuf d_ptrs, d_key2, d_sorted, d_tmp, d_slen, d_dst, d_scan, d_total, d_out;
    ALLOC(d_ptrs, O.text.size() * sizeof(void *));
    HIPCHK(hipMemcpy(d_ptrs.p, O.text.data(), O.text.size() * sizeof(void *), hipMemcpyHostToDevice));
    ALLOC(d_key2, (size_t)nn * 8); ALLOC(d_sorted, (size_t)nn * 4); ALLOC(d_slen, (size_t)nn * 4); ALLOC(d_dst, (size_t)nn * 4);
    ALLOC(d_scan, hgx_scan_u32_scratch_bytes(nn) + 16);
    ALLOC(d_total, 16);
    int end_bit = 33;                                                      // the bits of n_loci << 32, the largest key
    while (end_bit < 64 && ((unsigned long long)ix->hv.n_loci >> (end_bit - 32))) ++end_bit;
    size_t tmp_bytes = 0;
    (void)hipcub::DeviceRadixSort::SortPairs((void *)nullptr, tmp_bytes, (unsigned long long *)nullptr, (unsigned long long *)nullptr, (uint32_t *)nullptr,
                                             (uint32_t *)nullptr, (int)nn, 0, end_bit, st);
    ALLOC(d_tmp, std::max<size_t>(tmp_bytes, 256));
    HIPCHK(hipcub::DeviceRadixSort::SortPairs(d_tmp.p, tmp_bytes, O.key.as<unsigned long long>(), d_key2.as<unsigned long long>(), O.idx.as<uint32_t>(),
                                              d_sorted.as<uint32_t>(), (int)nn, 0, end_bit, st));
    k_aln_rec_lens<<<nblk(nn, 256), 256, 0, st>>>(d_sorted.as<uint32_t>(), nn, O.len.as<uint32_t>(), d_slen.as<uint32_t>());
    HIPCHK(hipGetLastError());
    TRY(hgx_scan_u32_dev(d_slen.as<uint32_t>(), d_dst.as<uint32_t>(), nn, d_scan.p, d_total.as<uint32_t>(), st));
    ALLOC(d_out, head + total + 64);
    HIPCHK(hipMemsetAsync(d_out.as<char>() + head + total, 0, 64, st));
    if (head) HIPCHK(hipMemcpyAsync(d_out.p, ix->header.data(), head, hipMemcpyHostToDevice, st));
    k_aln_gather_lines<<<nblk(nn, 4), 256, 0, st>>>(d_sorted.as<uint32_t>(), nn, O.place.as<unsigned long long>(), O.len.as<uint32_t>(),
                                                    d_dst.as<uint32_t>(), (const char *const *)d_ptrs.p, d_out.as<char>() + head);
    HIPCHK(hipGetLastError());
    uint32_t scanned = 0;
    HIPCHK(hipMemcpy(&scanned, d_total.p, 4, hipMemcpyDeviceToHost));        // (also: the gather has run before its buffers go back to the pool)
    HIPCHK(hipStreamSynchronize(st));
    if (scanned != total) { hgx_set_error("hgx_align_reads: the ordered text has %u bytes, the chunks' %zu", scanned, total); return HGX_EHIP; }
    if (ord->keep) {
        ord->d_text = d_out.p;
        ord->n_bytes = head + total;
        d_out.p = nullptr;
    } else if (total) {
        const size_t at = body.size();
        body.resize(at + total);
        HIPCHK(hipMemcpy(&body[at], d_out.p, total, hipMemcpyDeviceToHost));
    }
    return HGX_OK;
}
}      // namespace

void hgx_align_device_free(hgx_align_index *ix) {
    if (ix->d_block) (void)hipFree(ix->d_block);
    ix->d_block = nullptr;
    ix->dev_ready = -1;
}

static int align_chunks(hgx_align_index *ix, const hgx_dev_reads &rd, long n, int max_len, const int32_t *h_len, const hgx_align_opts *opts,
                        int gap, int rescue_clip, std::string &body, int64_t *aligned, int64_t *concordant, int *decline, hgx_aln_ordered *ord);

// the upload half: the loader's table and text copied up, then the chunks over them
int hgx_align_device(hgx_align_index *ix, const hgx_aln_reads &reads, const hgx_align_opts *opts, int gap, int rescue_clip, std::string &body,
                     int64_t *aligned, int64_t *concordant, int *decline, hgx_aln_ordered *ord) {
    *decline = 0;
    const long n = (long)reads.n();
    int max_len = 0;
    for (long i = 0; i < n; ++i) max_len = std::max(max_len, (int)reads.len[i]);
    if (max_len > HGX_ALN_DEV_MAX_READ) { *decline = HGX_ALN_DECLINE_READ_LEN; return HGX_OK; }
    int rc = ensure_device_index(ix);
    if (rc) return rc;
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
    return align_chunks(ix, rd, n, max_len, reads.len.data(), opts, gap, rescue_clip, body, aligned, concordant, decline, ord);
}

// the body: the chunks of a read table that lies in HBM.  h_len (the reads' lengths on the host) is read by the states tier alone:
// nullptr with opts->search == 0.
int hgx_align_device_body(hgx_align_index *ix, const hgx_dev_reads &rd, long n, int max_len, const int32_t *h_len, const hgx_align_opts *opts,
                          int gap, int rescue_clip, std::string &body, int64_t *aligned, int64_t *concordant, int *decline,
                          hgx_aln_ordered *ord) {
    *decline = 0;
    if (max_len > HGX_ALN_DEV_MAX_READ) { *decline = HGX_ALN_DECLINE_READ_LEN; return HGX_OK; }
    const int rc = ensure_device_index(ix);
    if (rc) return rc;
    return align_chunks(ix, rd, n, max_len, h_len, opts, gap, rescue_clip, body, aligned, concordant, decline, ord);
}

// the chunks themselves: the index is in HBM and no read is longer than the kernels take (either caller has seen to both)
static int align_chunks(hgx_align_index *ix, const hgx_dev_reads &rd, long n, int max_len, const int32_t *h_len, const hgx_align_opts *opts,
                        int gap, int rescue_clip, std::string &body, int64_t *aligned, int64_t *concordant, int *decline, hgx_aln_ordered *ord) {
    *decline = 0;
    const size_t body0 = body.size();
    const int64_t aligned0 = *aligned, concordant0 = *concordant;
    const int n_off_max = hgx_aln_n_offsets(max_len);
    int rc = HGX_OK;
    hipStream_t st = nullptr;
    const int cmax = (int)std::min<long>(n, CHUNK);
    DevBuf d_cnt, d_anch, d_res, d_best, d_nh, d_sizes, d_off, d_flags, d_scan, d_misc, d_mark;
    const int search = opts->search;
    if (search) ALLOC(d_mark, (size_t)cmax * 4);
    ALLOC(d_cnt, (size_t)cmax * 4);
    ALLOC(d_anch, (size_t)cmax * HGX_ALN_DEV_ANCHORS * sizeof(int2));
    ALLOC(d_res, (size_t)cmax * HGX_ALN_DEV_ANCHORS * sizeof(DevRes));
    ALLOC(d_best, (size_t)cmax * 4); ALLOC(d_nh, (size_t)cmax * 4); ALLOC(d_sizes, (size_t)cmax * 4); ALLOC(d_off, (size_t)cmax * 4);
    ALLOC(d_flags, (size_t)cmax * 4);
    ALLOC(d_scan, hgx_scan_u32_scratch_bytes(cmax) + 16);
    ALLOC(d_misc, 48);                       // [0] decline code, [1] total bytes, [2] reads marked for the second tier; pair mode: bytes 16 .. 40 = pairs searched, placed, changed
    // the call's fallback tier (one, or both with rescue_clip > 0: hgx_align_reads_x) and the k_aln_emit that reads its words, chosen
    // here once
    const int clip = opts->clip;
    const bool rescue = rescue_clip > 0 && gap > 0;
    const auto tier = rescue ? rescue_tiers : clip > 0 ? fallback_tier<ClipTier> : gap > 0 ? fallback_tier<GapTier> : nullptr;
    const auto emit = rescue ? k_aln_emit<true, true> : clip > 0 ? k_aln_emit<true> : gap > 0 ? k_aln_emit<false, true> : k_aln_emit<false>;
    const int budgets[2] = {rescue ? rescue_clip : clip, gap};
    DevBuf d_read_word, d_nslot, d_soff, d_slot_word, d_compact, d_nslot2, d_kept, d_kept_nh, d_cost;
    if (tier) {
        ALLOC(d_read_word, (size_t)cmax * (rescue ? 8 : 4)); ALLOC(d_nslot, (size_t)cmax * 4); ALLOC(d_soff, (size_t)cmax * 4);
        ALLOC(d_slot_word, (size_t)cmax * HGX_ALN_DEV_ANCHORS * 4); ALLOC(d_compact, (size_t)cmax * HGX_ALN_DEV_ANCHORS * 4);
    }
    if (rescue) {
        ALLOC(d_nslot2, (size_t)cmax * 4); ALLOC(d_kept, (size_t)cmax * sizeof(DevRes)); ALLOC(d_kept_nh, (size_t)cmax * 4);
        ALLOC(d_cost, (size_t)cmax * 4);
    }
    const Chunk c{d_cnt.as<int32_t>(), d_anch.as<int2>(), d_res.as<DevRes>(), d_best.as<int32_t>(), d_nh.as<int32_t>(),
                  search ? d_mark.as<int32_t>() : nullptr, d_slot_word.as<uint32_t>(), d_read_word.as<uint32_t>(), d_nslot.as<uint32_t>(),
                  d_soff.as<uint32_t>(), d_compact.as<int32_t>(), d_scan.p, d_misc.as<int>(), d_misc.as<uint32_t>() + 1,
                  d_nslot2.as<uint32_t>(), d_kept.as<DevRes>(), d_kept_nh.as<int32_t>(), d_cost.as<int32_t>()};
    auto launch_emit = [&](long first, int nc, uint32_t *sizes, int32_t *flags, const uint32_t *off, char *out) {      // either pass
        emit<<<nblk(nc, 64), 64, 0, st>>>(ix->dv, rd, first, nc, opts->max_fragment, c.res, c.best, c.nh, sizes, flags, off, out, c.read_word);
        return hipGetLastError();
    };
    auto declined = [&](int dec) {                // what earlier chunks appended is taken back
        body.resize(body0);
        *aligned = aligned0;
        *concordant = concordant0;
        *decline = dec;
        return HGX_OK;
    };
    TierCounts tier_counts = {};
    const bool pair_aware = rd.paired && opts->pair == 1;
    const size_t misc_bytes = pair_aware ? 40 : 16;
    int64_t pairs[3] = {0, 0, 0};
    std::vector<int32_t> flags(cmax);
    std::string text;
    Ordered O;                                 // (ord == nullptr: stays empty -- no buffer, no kernel)
    if (ord) {
        O.st = st;
        ALLOC(O.key, (size_t)n * 8); ALLOC(O.place, (size_t)n * 8); ALLOC(O.len, (size_t)n * 4); ALLOC(O.idx, (size_t)n * 4);
    }
    for (long first = 0; first < n; first += CHUNK) {
        const int nc = (int)std::min<long>(CHUNK, n - first);
        HIPCHK(hipMemsetAsync(d_cnt.p, 0, (size_t)nc * 4, st));
        HIPCHK(hipMemsetAsync(d_misc.p, 0, misc_bytes, st));
        if (search) HIPCHK(hipMemsetAsync(d_mark.p, 0, (size_t)nc * 4, st));
        const long n_seed = (long)nc * 2 * n_off_max;
        if (n_seed > 0)
            k_aln_seed<<<nblk(n_seed, 256), 256, 0, st>>>(ix->dv, rd, first, nc, n_off_max, d_cnt.as<int32_t>(), d_anch.as<int2>());
        if (search == 2) k_aln_mark_all<<<nblk(nc, 256), 256, 0, st>>>(nc, c.cnt, c.mark, c.decline);
        else if (search == 1)
            k_aln_extend<true><<<nblk((long)nc * HGX_ALN_DEV_ANCHORS, 64), 64, 0, st>>>(ix->dv, rd, first, nc, opts->max_edits, c.cnt, c.anch, c.res,
                                                                                         c.decline, c.mark);
        else
            k_aln_extend<false><<<nblk((long)nc * HGX_ALN_DEV_ANCHORS, 64), 64, 0, st>>>(ix->dv, rd, first, nc, opts->max_edits, c.cnt, c.anch, c.res,
                                                                                          c.decline, nullptr);
        HIPCHK(hipGetLastError());
        int misc[4] = {0, 0, 0, 0};
        HIPCHK(hipMemcpy(misc, d_misc.p, search ? 16 : 4, hipMemcpyDeviceToHost));
        int dec = misc[0];
        if (!dec && search && misc[2] > 0) {
            rc = states_tier(ix, h_len, rd, opts, first, nc, n_off_max, c, st, &dec);
            if (rc) return rc;
        }
        if (dec) return declined(dec);
        k_aln_pick<<<nblk(nc, 64), 64, 0, st>>>(nc, c.cnt, c.res, c.best, c.nh, c.mark);
        if (pair_aware)
            k_aln_pair_pick<<<nc / 2, 64, 0, st>>>(nc, opts->max_fragment, c.cnt, c.res, c.best, c.nh,
                                                   (unsigned long long *)(d_misc.as<char>() + 16));
        if (tier) {
            rc = tier(ix, rd, opts->max_edits, budgets, first, nc, c, st, tier_counts, &dec);
            if (rc) return rc;
            if (dec) return declined(dec);
        }
        HIPCHK(launch_emit(first, nc, d_sizes.as<uint32_t>(), d_flags.as<int32_t>(), nullptr, nullptr));
        rc = hgx_scan_u32_dev(d_sizes.as<uint32_t>(), d_off.as<uint32_t>(), nc, c.scan, c.total, st);
        if (rc) return rc;
        uint32_t back[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};                // total bytes; pair mode: the rest of d_misc with it
        HIPCHK(hipMemcpy(back, c.total, pair_aware ? 36 : 4, hipMemcpyDeviceToHost));
        const uint32_t total = back[0];
        for (int k = 0; k < 3; ++k) {
            uint64_t v;
            memcpy(&v, back + 3 + 2 * k, 8);
            pairs[k] += (int64_t)v;
        }
        HIPCHK(hipMemcpy(flags.data(), d_flags.p, (size_t)nc * 4, hipMemcpyDeviceToHost));
        for (int i = 0; i < nc; ++i) { *aligned += flags[i] & 1; *concordant += (flags[i] >> 1) & 1; }
        if (ord) {                                                     // coordinate order: the text stays, the chunk's records join the table
            void *d_keep = total ? hgx_pool_alloc(total) : nullptr;
            O.text.push_back(d_keep);
            O.bytes.push_back(total);
            if (total && !d_keep) { hgx_set_error("device allocation of %u bytes failed", total); return HGX_ENOMEM; }
            if (total) HIPCHK(launch_emit(first, nc, nullptr, nullptr, d_off.as<uint32_t>(), (char *)d_keep));
            k_aln_rec_keys<<<nblk(nc, 256), 256, 0, st>>>(ix->dv, first, nc, (uint32_t)(first / CHUNK), c.res, c.best, d_sizes.as<uint32_t>(),
                                                          d_off.as<uint32_t>(), O.key.as<unsigned long long>(), O.place.as<unsigned long long>(),
                                                          O.len.as<uint32_t>(), O.idx.as<uint32_t>());
            HIPCHK(hipGetLastError());
        } else if (total) {
            DevBuf d_out;
            ALLOC(d_out, (size_t)total);
            HIPCHK(launch_emit(first, nc, nullptr, nullptr, d_off.as<uint32_t>(), d_out.as<char>()));
            text.resize(total);
            HIPCHK(hipMemcpy(&text[0], d_out.p, total, hipMemcpyDeviceToHost));
            body += text;
        }
    }
    if (ord) {
        rc = order_text(ix, O, n, body, ord, st);
        if (rc) { (void)hipStreamSynchronize(st); return rc; }
    }
    HIPCHK(hipStreamSynchronize(st));
    if (pair_aware) hgx_align_pairs_count(pairs[0], pairs[1], pairs[2]);
    for (int t = 1; tier && t < HGX_ALN_N_TIERS; ++t) hgx_align_tier_count(t, tier_counts[t][0], tier_counts[t][1], tier_counts[t][2]);
    return HGX_OK;
}

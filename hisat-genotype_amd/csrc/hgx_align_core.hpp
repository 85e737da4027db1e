// hgx_align_core.hpp -- the "hgx" aligner's per-anchor and per-read logic, compiled into the kernels
// (hgx_align.hip) and into the host route (hgx_align_host.cpp).  The rules are stated in plain Python in tests/align_ref.py
// (pair-aware placement: tests/align_pair_ref.py; soft clips: tests/align_clip_ref.py; novel gaps: tests/align_gap_ref.py).
//
// An alignment of an oriented read at a locus = a start pos0 + an ordered list of known variants.  The walk of
// simulate._truth_record consumes the read with them: at state (r, p), r > 0, at most one known insertion and one known deletion
// that start at p are taken (the insertion first, so that both sit at their database position), then read base r sits on backbone
// base p -- a match, a known single (free; the first in Var_list order whose data is the base) or one unknown edit.
// The search is a depth-first enumeration of the indel choices left
// and right of a 16-base anchor, cut where a side's edits exceed the budget or its cost exceeds the best found; the first three
// components of the order are sums over the two sides, so each side is minimised on its own.  Scratch is of fixed size (MAXSTK
// pending choices, MAXV variants, max_steps read bases walked): reaching a limit returns a decline code before anything is written.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define HGX_ALN_HD __host__ __device__
#else
#define HGX_ALN_HD
#endif

#define HGX_ALN_K 16
#define HGX_ALN_STRIDE 4
#define HGX_ALN_MAX_READ 1024          // the longest read the core takes (either route)
#define HGX_ALN_DEV_MAX_READ 256       // the longest read the kernels take
#define HGX_ALN_DEV_ANCHORS 128        // anchor slots per read on the device (a 256-base read has 61 seed offsets: two placements fit)
#define HGX_ALN_DEV_STK 32             // pending indel choices per side on the device
#define HGX_ALN_DEV_VARS 32            // variants per alignment on the device
#define HGX_ALN_DEV_STEPS 200000       // read bases walked per side on the device

// decline codes (hgx_align_last)
#define HGX_ALN_DECLINE_NONE 0
#define HGX_ALN_DECLINE_GATE 1         // fewer reads than the gate
#define HGX_ALN_DECLINE_READ_LEN 2
#define HGX_ALN_DECLINE_ANCHORS 3
#define HGX_ALN_DECLINE_STACK 4
#define HGX_ALN_DECLINE_VARS 5
#define HGX_ALN_DECLINE_STEPS 6
#define HGX_ALN_DECLINE_SWITCH 7       // front=host

#define HGX_ALN_INS 0
#define HGX_ALN_SGL 1
#define HGX_ALN_DEL 2

// the index as flat arrays (host or device memory); positions are GLOBAL: locus g covers [bb_off[g], bb_off[g + 1]) of `bb`, and a
// variant's global index orders it as (locus, Var_list index)
struct hgx_aln_view {
    const char *bb;
    const int32_t *bb_off;
    int32_t n_loci, n_pos;
    const uint32_t *hkey;              // open-addressing table of the 16-mer codes: hpos < 0 = empty; equal codes sit in one probe run
    const int32_t *hpos;
    uint32_t hmask;
    const uint8_t *vtype;
    const int32_t *vpos, *vlen;        // vlen: deleted bases / inserted bases / 1
    const int32_t *vdata;              // single: the base; insertion: offset of its bases in `pool`
    const int32_t *vid_off, *vid_len;  // the variant's id in `pool`
    const int32_t *name_off, *name_len;   // per locus: its reference name in `pool`
    const char *pool;
    // per-position CSR tables [n_pos + 1]: singles at p, deletions starting at p, deletions ending at p (first base behind them), insertions at p
    const int32_t *sgl_off, *sgl, *dls_off, *dls, *dle_off, *dle, *ins_off, *ins;
};

struct hgx_aln_read {
    const char *seq;                   // upper case, as given
    int32_t L, strand;
    HGX_ALN_HD char at(int r) const {
        if (!strand) return seq[r];
        const char c = seq[L - 1 - r];
        return c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : c;
    }
};

HGX_ALN_HD inline int hgx_aln_code2(char c) { return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : -1; }
HGX_ALN_HD inline uint32_t hgx_aln_hash(uint32_t code) { return (code * 0x9E3779B1u) ^ (code >> 15); }
HGX_ALN_HD inline int hgx_aln_n_offsets(int L) {        // 0, 4, 8, ... <= L - 16, plus L - 16
    if (L < HGX_ALN_K) return 0;
    const int last = L - HGX_ALN_K;
    return last / HGX_ALN_STRIDE + 1 + (last % HGX_ALN_STRIDE != 0);
}
HGX_ALN_HD inline int hgx_aln_offset(int L, int k) {
    const int last = L - HGX_ALN_K;
    return k * HGX_ALN_STRIDE <= last ? k * HGX_ALN_STRIDE : last;
}
// the 16-mer code of the oriented read at offset o, false if it holds a non-ACGT base
HGX_ALN_HD inline bool hgx_aln_seed_code(const hgx_aln_read &R, int o, uint32_t *code) {
    uint32_t c = 0;
    for (int k = 0; k < HGX_ALN_K; ++k) {
        const int b = hgx_aln_code2(R.at(o + k));
        if (b < 0) return false;
        c = (c << 2) | (uint32_t)b;
    }
    *code = c;
    return true;
}
HGX_ALN_HD inline int hgx_aln_locus_of(const hgx_aln_view &V, int32_t P) {
    int g = 0;
    while (g + 1 < V.n_loci && V.bb_off[g + 1] <= P) ++g;
    return g;
}

// read base r on backbone base P: 0 = match, 1 = unknown edit, 2 = the known single *v
HGX_ALN_HD inline int hgx_aln_base(const hgx_aln_view &V, const hgx_aln_read &R, int r, int32_t P, int32_t *v) {
    const char c = R.at(r);
    if (c == V.bb[P]) return 0;
    if (hgx_aln_code2(c) >= 0)
        for (int32_t k = V.sgl_off[P]; k < V.sgl_off[P + 1]; ++k)
            if ((char)V.vdata[V.sgl[k]] == c) { *v = V.sgl[k]; return 2; }
    return 1;
}
// bases the insertion v consumes at read base r (cut by the read's right end), or -1 if they differ
HGX_ALN_HD inline int hgx_aln_ins_fits(const hgx_aln_view &V, const hgx_aln_read &R, int32_t v, int r) {
    const char *d = V.pool + V.vdata[v];
    int n = V.vlen[v];
    if (n > R.L - r) n = R.L - r;
    for (int k = 0; k < n; ++k)
        if (R.at(r + k) != d[k]) return -1;
    return n;
}

template <int MAXV> struct hgx_aln_side {
    int32_t found, nm, nind, nl, pos;          // pos: pos0 (left side) or the backbone end (right side), global
    int32_t vl[MAXV];                          // in walk order
};
template <int MAXV> struct hgx_aln_res {
    int32_t ok, nm, nind, nvar, locus, strand, pos0, end;      // pos0 / end global
    int32_t vl[MAXV];
};
struct hgx_aln_frame { int32_t r, P, nm, nind, nl, k; };

HGX_ALN_HD inline int hgx_aln_cmp3(int a0, int a1, int a2, int b0, int b1, int b2) {
    return a0 != b0 ? (a0 < b0 ? -1 : 1) : a1 != b1 ? (a1 < b1 ? -1 : 1) : a2 != b2 ? (a2 < b2 ? -1 : 1) : 0;
}
// the left side's best x and the right side's best y as one alignment of locus g
template <int MAXV>
HGX_ALN_HD inline int hgx_aln_join(const hgx_aln_side<MAXV> &x, const hgx_aln_side<MAXV> &y, int g, int strand, hgx_aln_res<MAXV> &res) {
    if (x.nl + y.nl > MAXV) return HGX_ALN_DECLINE_VARS;
    for (int i = 0; i < x.nl; ++i) res.vl[i] = x.vl[i];
    for (int i = 0; i < y.nl; ++i) res.vl[x.nl + i] = y.vl[i];
    res.nm = x.nm + y.nm; res.nind = x.nind + y.nind; res.nvar = x.nl + y.nl; res.pos0 = x.pos; res.end = y.pos;
    res.locus = g; res.strand = strand; res.ok = 1;
    return 0;
}

// ---- soft clips (opts.clip > 0; the rule in plain Python: tests/align_clip_ref.py) -------------------------------------------------
// The clip tier runs the same two walks with CLIP = true.  A side then has one more option at every state it ENTERS: stop there
// and clip what is left of the read (right: the L - r bases from r on; left: the r bases in front of "base r sits on Q").  What a
// side returns is one entry per e = 0 .. max_nm: the smallest (clip, indels, variants, [pos0,] list) among its ways with exactly e
// unknown mismatches (hgx_aln_clip_canon combines the two sides).  Along one way the stop with the fewest clipped bases for e is the
// last state entered with e mismatches, so a state's stop is offered only where the step from it does not simply go on: the
// mismatch e + 1 is taken, the backbone ends or the walk dies.  The cut by the best found and the memo are off (neither is lossless
// once a side keeps an entry per e); a stop that alone clips more than the budget is not offered, which loses nothing.
#define HGX_ALN_CLIP_EDITS 4           // clip > 0 takes max_edits up to this (the per-e entries are of fixed size)
#define HGX_ALN_CLIP_MAX 255
// A side's entries are hgx_aln_side[HGX_ALN_CLIP_EDITS + 1], indexed by e, whose `nm` word holds the CLIP count; the CLIP walks
// take the array through their `best` argument.
// a way of the walk (its list in cur[0 .. nl), backwards if `rev`) against the side's entry for its e (not the plain arms')
template <int MAXV>
HGX_ALN_HD inline void hgx_aln_clip_offer(hgx_aln_side<MAXV> &b, int clip, int nind, int nl, int32_t pos, bool use_pos, const int32_t *cur,
                                          bool rev) {
    int c = b.found ? hgx_aln_cmp3(clip, nind, nl, b.nm, b.nind, b.nl) : -1;
    if (c == 0 && use_pos && pos != b.pos) c = pos < b.pos ? -1 : 1;
    for (int i = 0; c == 0 && i < nl; ++i) {
        const int32_t a = rev ? cur[nl - 1 - i] : cur[i];
        c = a != b.vl[i] ? (a < b.vl[i] ? -1 : 1) : 0;
    }
    if (c < 0) {
        b.found = 1; b.nm = clip; b.nind = nind; b.nl = nl; b.pos = pos;
        for (int i = 0; i < nl; ++i) b.vl[i] = rev ? cur[nl - 1 - i] : cur[i];
    }
}

// ---- novel gaps (hgx_align_more.gap > 0; the rule in plain Python: tests/align_gap_ref.py) -----------------------------------------
// The gap tier runs the same two walks with GAP = 1.  Such a walk is the plain enumeration with one edit of the budget held back
// (a gap costs at least 1); it offers nothing at its own end.  On ENTRY to each state it runs, for every novel deletion and
// insertion of 1 .. n bases that the edits left allow, an inner PLAIN walk (GAP = 2: the plain walk that also reports its steps)
// from the state behind the gap, with a stack and a list of its own, and offers prefix + gap + the inner walk's best to the side's
// best.  The prefix is fixed while the inner walk runs and every component of the order is a sum or a concatenation, so the inner
// best gives the smallest way through that gap; costs only grow along a way, so the cut "partial cost (with the 1 held back)
// passes the best found" stays lossless, and so does giving an inner walk no more edits than the best found leaves.  The gap is
// not a pending frame of the depth-first stack (every state on a way would hold one).  The memo is off in the tier: an arrival
// that a plain search may drop can still be the prefix of the smallest way with a gap.  All inner walks of a side share the side's
// step limit.  The descriptor (read offset, kind, length) is the last component of the order; it packs into one word whose order
// as a number is the descriptor's.
#define HGX_ALN_GAP_MAX 16
HGX_ALN_HD inline uint32_t hgx_aln_gap_pack(int r, int kind, int len) { return ((uint32_t)r << 8) | ((uint32_t)kind << 7) | (uint32_t)len; }
HGX_ALN_HD inline int hgx_aln_gap_r(uint32_t gd) { return (int)(gd >> 8); }
HGX_ALN_HD inline int hgx_aln_gap_kind(uint32_t gd) { return (int)((gd >> 7) & 1); }      // 0 deletion, 1 insertion
HGX_ALN_HD inline int hgx_aln_gap_len(uint32_t gd) { return (int)(gd & 0x7f); }
template <int MAXV> struct hgx_aln_gap_ctx {
    hgx_aln_frame *stk;                        // the inner walks' scratch
    int32_t *cur;
    hgx_aln_side<MAXV> *inner;
    int n;                                     // the longest gap
    uint32_t gd;                               // the descriptor of the side's best
    long used;                                 // steps the inner walks took
};
// prefix (nm, nind, the list in `pre`: backwards if `rev`, then in front of the inner list) + an optional single + the inner best
// `in` against the side's best; returns true if it became the best
template <int MAXV>
HGX_ALN_HD inline bool hgx_aln_gap_offer(hgx_aln_side<MAXV> &b, uint32_t *bgd, int nm, int nind, const int32_t *pre, int npre, int32_t sv,
                                         const hgx_aln_side<MAXV> &in, bool rev, uint32_t gd) {
    const int nsv = sv >= 0, nl = npre + nsv + in.nl;
    auto at = [&](int i) -> int32_t {
        if (!rev) return i < npre ? pre[i] : in.vl[i - npre];
        return i < in.nl ? in.vl[i] : (nsv && i == in.nl) ? sv : pre[npre - 1 - (i - in.nl - nsv)];
    };
    int c = b.found ? hgx_aln_cmp3(nm + in.nm, nind + in.nind, nl, b.nm, b.nind, b.nl) : -1;
    if (c == 0 && rev && in.pos != b.pos) c = in.pos < b.pos ? -1 : 1;
    for (int i = 0; c == 0 && i < nl; ++i) c = at(i) != b.vl[i] ? (at(i) < b.vl[i] ? -1 : 1) : 0;
    if (c == 0 && gd != *bgd) c = gd < *bgd ? -1 : 1;
    if (c >= 0) return false;
    b.found = 1; b.nm = nm + in.nm; b.nind = nind + in.nind; b.nl = nl; b.pos = in.pos;
    for (int i = 0; i < nl; ++i) b.vl[i] = at(i);
    *bgd = gd;
    return true;
}

// MEMO: what a route remembers about the states a side's search has reached through a known indel.  dominated(side, r, P, cost, list)
// == true cuts the path: an earlier path reached the same state (side 0: (r, P) before its events; side 1: base r on P) with a
// smaller cost, or the same cost and a list that sorts first -- every way to finish from here is then a way to finish from there
// with a smaller total, so nothing the order could pick is lost.  Without a memo (the kernels: fixed scratch) the enumeration grows
// with the number of COMBINATIONS of known indels that lead to one state (a tandem repeat with many known unit deletions and
// insertions) and ends at max_steps; with one (the host route) a state is finished once per improvement of its arrival.
struct hgx_aln_no_memo {
    HGX_ALN_HD void reset() {}
    HGX_ALN_HD bool dominated(int, int, int32_t, int, int, int, const int32_t *) { return false; }
};

// every way to finish from state (r0, P0), r0 > 0, inside the locus [lo, hi): the smallest by (NM, indels, variants, list)
// GAP = 1 (max_nm counts the gap; `gx`): the smallest with ONE novel gap, by (NM, indels, variants, list, descriptor)
template <int MAXSTK, int MAXV, class MEMO, bool CLIP = false, int GAP = 0>
HGX_ALN_HD int hgx_aln_right(const hgx_aln_view &V, const hgx_aln_read &R, int32_t hi, int r0, int32_t P0, int max_nm, long max_steps,
                             hgx_aln_frame *stk, int32_t *cur, hgx_aln_side<MAXV> &best, MEMO &memo, int clip = 0,
                             hgx_aln_gap_ctx<MAXV> *gx = nullptr) {
    int sp = 0;
    long steps = 0;
    if (!CLIP) best.found = 0;
    if constexpr (GAP == 1) {
        gx->gd = 0;
        gx->used = 0;
        if (max_nm < 1) return 0;
    }
    const int walk_nm = GAP == 1 ? max_nm - 1 : max_nm;
    int r = r0, nm = 0, nind = 0, nl = 0, k = 0;
    int32_t P = P0;
    for (;;) {
        bool dead = false, done = false;
        int32_t end = P;
        const int r_in = r, nm_in = nm, nind_in = nind, nl_in = nl;      // (CLIP: the state entered, for its stop)
        if (r == R.L) done = true;
        else if (P >= hi) dead = true;
        else {
            if (++steps > max_steps) return HGX_ALN_DECLINE_STEPS;
            if constexpr (GAP == 1) {
                if (steps + gx->used > max_steps) return HGX_ALN_DECLINE_STEPS;
                if (k == 0) {                                        // the state is entered: the gap in front of its known indels
                    hgx_aln_no_memo none;
                    int room = (best.found ? best.nm : max_nm) - nm;   // edits left for the gap and what follows it
                    for (int kind = 0; kind < 2; ++kind)
                        for (int g = 1; g <= gx->n && g <= room; ++g) {
                            const int r2 = kind ? r + g : r;
                            const int32_t P2 = kind ? P : P + g;
                            if (r2 >= R.L || P2 >= hi) break;
                            const int rc = hgx_aln_right<MAXSTK, MAXV, hgx_aln_no_memo, false, 2>(
                                V, R, hi, r2, P2, room - g, max_steps - steps - gx->used, gx->stk, gx->cur, *gx->inner, none, 0, gx);
                            if (rc) return rc;
                            if (!gx->inner->found) continue;
                            if (nl + gx->inner->nl > MAXV) return HGX_ALN_DECLINE_VARS;
                            if (hgx_aln_gap_offer(best, &gx->gd, nm + g, nind, cur, nl, -1, *gx->inner, false, hgx_aln_gap_pack(r, kind, g)))
                                room = best.nm - nm;
                        }
                }
            }
            const int nd = V.dls_off[P + 1] - V.dls_off[P], ni = V.ins_off[P + 1] - V.ins_off[P];
            const int nopt = 1 + nd + ni + nd * ni;
            if (k + 1 < nopt) {
                if (sp == MAXSTK) return HGX_ALN_DECLINE_STACK;
                stk[sp++] = hgx_aln_frame{r, P, nm, nind, nl, k + 1};
            }
            int32_t dv = -1, iv = -1;
            if (k == 0) {
            } else if (k <= nd) dv = V.dls[V.dls_off[P] + k - 1];
            else if (k <= nd + ni) iv = V.ins[V.ins_off[P] + k - 1 - nd];
            else {
                const int idx = k - 1 - nd - ni;
                dv = V.dls[V.dls_off[P] + idx / ni];
                iv = V.ins[V.ins_off[P] + idx % ni];
            }
            int rr = r;
            int32_t PP = P;
            for (int step = 0; step < 2 && !dead; ++step) {
                const bool take_del = step == 1;
                const int32_t v = take_del ? dv : iv;
                if (v < 0) continue;
                if (nl == MAXV) return HGX_ALN_DECLINE_VARS;
                cur[nl++] = v;
                ++nind;
                if (take_del) PP += V.vlen[v];
                else {
                    const int n = hgx_aln_ins_fits(V, R, v, rr);
                    if (n < 0) dead = true;
                    else rr += n;
                }
            }
            if (!dead) {
                if (rr >= R.L) { done = true; end = PP; }
                else if (PP >= hi) dead = true;
                else {
                    int32_t sv = -1;
                    const int c = hgx_aln_base(V, R, rr, PP, &sv);
                    if (c == 1) { if (++nm > walk_nm) dead = true; }
                    else if (c == 2) {
                        if (nl == MAXV) return HGX_ALN_DECLINE_VARS;
                        cur[nl++] = sv;
                    }
                    r = rr + 1;
                    P = PP + 1;
                    k = 0;
                    if (!CLIP && !dead && best.found && hgx_aln_cmp3(nm + (GAP == 1), nind, nl, best.nm, best.nind, best.nl) > 0) dead = true;
                    if (!CLIP && GAP != 1 && !dead && nind > 0 && r < R.L && memo.dominated(0, r, P, nm, nind, nl, cur)) dead = true;
                }
            }
        }
        if constexpr (CLIP) {
            if (r_in < R.L && (dead || nm != nm_in) && R.L - r_in <= clip)
                hgx_aln_clip_offer((&best)[nm_in], R.L - r_in, nind_in, nl_in, end, false, cur, false);
            if (done) hgx_aln_clip_offer((&best)[nm], 0, nind, nl, end, false, cur, false);
            done = dead || done;
            dead = done;
        } else
        if (done && GAP != 1) {
            int c = best.found ? hgx_aln_cmp3(nm, nind, nl, best.nm, best.nind, best.nl) : -1;
            for (int i = 0; c == 0 && i < nl; ++i) c = cur[i] != best.vl[i] ? (cur[i] < best.vl[i] ? -1 : 1) : 0;
            if (c < 0) {
                best.found = 1; best.nm = nm; best.nind = nind; best.nl = nl; best.pos = end;
                for (int i = 0; i < nl; ++i) best.vl[i] = cur[i];
            }
        }
        if (dead || done) {
            if (sp == 0) break;
            const hgx_aln_frame f = stk[--sp];
            r = f.r; P = f.P; nm = f.nm; nind = f.nind; nl = f.nl; k = f.k;
        }
    }
    if constexpr (GAP == 2) gx->used += steps;
    return 0;
}

// every way to have arrived at "read base r0 sits on backbone base Q0" inside the locus [lo, hi): the smallest by
// (NM, indels, variants, pos0, list).  `cur` holds the list backwards.
// GAP = 1: the smallest with ONE novel gap, by (NM, indels, variants, pos0, list, descriptor).  The mirror of the right side: the
// state (r1, P1) from which an option's known events lead to "base r sits on Q" was itself reached by the gap, from (r1, P1 - g)
// or from (r1 - g, P1), and that state was entered from the base in front of it.
template <int MAXSTK, int MAXV, class MEMO, bool CLIP = false, int GAP = 0>
HGX_ALN_HD int hgx_aln_left(const hgx_aln_view &V, const hgx_aln_read &R, int32_t lo, int r0, int32_t Q0, int max_nm, long max_steps,
                            hgx_aln_frame *stk, int32_t *cur, hgx_aln_side<MAXV> &best, MEMO &memo, int clip = 0,
                            hgx_aln_gap_ctx<MAXV> *gx = nullptr) {
    int sp = 0;
    long steps = 0;
    if (!CLIP) best.found = 0;
    if constexpr (GAP == 1) {
        gx->gd = 0;
        gx->used = 0;
        if (max_nm < 1) return 0;
    }
    const int walk_nm = GAP == 1 ? max_nm - 1 : max_nm;
    int r = r0, nm = 0, nind = 0, nl = 0, k = 0;
    int32_t Q = Q0;
    for (;;) {
        bool dead = false, done = false;
        const int r_in = r, nm_in = nm, nind_in = nind, nl_in = nl;      // (CLIP: the state entered, for its clip)
        const int32_t Q_in = Q;
        if (r == 0) done = true;
        else {
            if (++steps > max_steps) return HGX_ALN_DECLINE_STEPS;
            if constexpr (GAP == 1) if (steps + gx->used > max_steps) return HGX_ALN_DECLINE_STEPS;
            const int nde = V.dle_off[Q + 1] - V.dle_off[Q], niq = V.ins_off[Q + 1] - V.ins_off[Q];
            int nopt = 1 + nde + niq;
            for (int j = 0; j < nde; ++j) {
                const int32_t p1 = V.vpos[V.dle[V.dle_off[Q] + j]];
                nopt += V.ins_off[p1 + 1] - V.ins_off[p1];
            }
            if (k + 1 < nopt) {
                if (sp == MAXSTK) return HGX_ALN_DECLINE_STACK;
                stk[sp++] = hgx_aln_frame{r, Q, nm, nind, nl, k + 1};
            }
            int32_t dv = -1, iv = -1;
            if (k == 0) {
            } else if (k <= nde) dv = V.dle[V.dle_off[Q] + k - 1];
            else if (k <= nde + niq) iv = V.ins[V.ins_off[Q] + k - 1 - nde];
            else {
                int idx = k - 1 - nde - niq;
                for (int j = 0; j < nde; ++j) {
                    const int32_t d = V.dle[V.dle_off[Q] + j], p1 = V.vpos[d];
                    const int cnt = V.ins_off[p1 + 1] - V.ins_off[p1];
                    if (idx < cnt) { dv = d; iv = V.ins[V.ins_off[p1] + idx]; break; }
                    idx -= cnt;
                }
            }
            int r1 = r;
            int32_t P1 = dv >= 0 ? V.vpos[dv] : Q;
            if (iv >= 0) {
                const int n = V.vlen[iv];
                if (r - n < 1 || hgx_aln_ins_fits(V, R, iv, r - n) != n) dead = true;
                else r1 = r - n;
            }
            if (!dead) {
                // backwards: the later event of the pair, the deletion, first
                for (int step = 0; step < 2; ++step) {
                    const bool take_del = step == 0;
                    const int32_t v = take_del ? dv : iv;
                    if (v < 0) continue;
                    if (nl == MAXV) return HGX_ALN_DECLINE_VARS;
                    cur[nl++] = v;
                    ++nind;
                }
                if constexpr (GAP == 1) {
                    hgx_aln_no_memo none;
                    int room = (best.found ? best.nm : max_nm) - nm;
                    for (int kind = 0; kind < 2; ++kind)
                        for (int g = 1; g <= gx->n && g <= room; ++g) {
                            const int rg = kind ? r1 - g : r1;               // the state the gap was taken in
                            const int32_t Pg = kind ? P1 : P1 - g;
                            if (rg < 1 || Pg - 1 < lo) break;
                            int32_t sv = -1;
                            const int cb = hgx_aln_base(V, R, rg - 1, Pg - 1, &sv);
                            const int e = g + (cb == 1);
                            if (e > room) continue;
                            const int rc = hgx_aln_left<MAXSTK, MAXV, hgx_aln_no_memo, false, 2>(
                                V, R, lo, rg - 1, Pg - 1, room - e, max_steps - steps - gx->used, gx->stk, gx->cur, *gx->inner, none, 0, gx);
                            if (rc) return rc;
                            if (!gx->inner->found) continue;
                            if (nl + (cb == 2) + gx->inner->nl > MAXV) return HGX_ALN_DECLINE_VARS;
                            if (hgx_aln_gap_offer(best, &gx->gd, nm + e, nind, cur, nl, cb == 2 ? sv : -1, *gx->inner, true,
                                                  hgx_aln_gap_pack(rg, kind, g)))
                                room = best.nm - nm;
                        }
                }
                if (P1 - 1 < lo) dead = true;
                else {
                    int32_t sv = -1;
                    const int c = hgx_aln_base(V, R, r1 - 1, P1 - 1, &sv);
                    if (c == 1) { if (++nm > walk_nm) dead = true; }
                    else if (c == 2) {
                        if (nl == MAXV) return HGX_ALN_DECLINE_VARS;
                        cur[nl++] = sv;
                    }
                    r = r1 - 1;
                    Q = P1 - 1;
                    k = 0;
                    if (!CLIP && !dead && best.found && hgx_aln_cmp3(nm + (GAP == 1), nind, nl, best.nm, best.nind, best.nl) > 0) dead = true;
                    if (!CLIP && GAP != 1 && !dead && nind > 0 && r > 0 && memo.dominated(1, r, Q, nm, nind, nl, cur)) dead = true;
                }
            }
        }
        if constexpr (CLIP) {
            if (r_in > 0 && (dead || nm != nm_in) && r_in <= clip) hgx_aln_clip_offer((&best)[nm_in], r_in, nind_in, nl_in, Q_in, true, cur, true);
            if (done) hgx_aln_clip_offer((&best)[nm], 0, nind, nl, Q, true, cur, true);
            done = dead || done;
            dead = done;
        } else
        if (done && GAP != 1) {
            int c = best.found ? hgx_aln_cmp3(nm, nind, nl, best.nm, best.nind, best.nl) : -1;
            if (c == 0 && Q != best.pos) c = Q < best.pos ? -1 : 1;
            for (int i = 0; c == 0 && i < nl; ++i) {
                const int32_t a = cur[nl - 1 - i];
                c = a != best.vl[i] ? (a < best.vl[i] ? -1 : 1) : 0;
            }
            if (c < 0) {
                best.found = 1; best.nm = nm; best.nind = nind; best.nl = nl; best.pos = Q;
                for (int i = 0; i < nl; ++i) best.vl[i] = cur[nl - 1 - i];
            }
        }
        if (dead || done) {
            if (sp == 0) break;
            const hgx_aln_frame f = stk[--sp];
            r = f.r; Q = f.P; nm = f.nm; nind = f.nind; nl = f.nl; k = f.k;
        }
    }
    if constexpr (GAP == 2) gx->used += steps;
    return 0;
}

// canon(a) of the anchor (read offset o, global backbone position b) of strand R.strand: res.ok = 0 if no alignment is admissible
// through it.  `side` is scratch for ONE side's best: the left side's is parked in `res` meanwhile (so no hgx_aln_join here).
template <int MAXSTK, int MAXV, class MEMO>
HGX_ALN_HD int hgx_aln_canon(const hgx_aln_view &V, const hgx_aln_read &R, int o, int32_t b, int max_edits, long max_steps,
                             hgx_aln_frame *stk, int32_t *cur, hgx_aln_side<MAXV> &side, hgx_aln_res<MAXV> &res, MEMO &memo) {
    const int g = hgx_aln_locus_of(V, b);
    const int32_t lo = V.bb_off[g], hi = V.bb_off[g + 1];
    res.ok = 0;
    memo.reset();
    int rc = hgx_aln_left<MAXSTK, MAXV>(V, R, lo, o, b, max_edits, max_steps, stk, cur, side, memo);
    if (rc) return rc;
    if (!side.found) return 0;
    memo.reset();
    res.nm = side.nm; res.nind = side.nind; res.nvar = side.nl; res.pos0 = side.pos;
    for (int i = 0; i < side.nl; ++i) res.vl[i] = side.vl[i];
    rc = hgx_aln_right<MAXSTK, MAXV>(V, R, hi, o + HGX_ALN_K, b + HGX_ALN_K, max_edits - res.nm, max_steps, stk, cur, side, memo);
    if (rc) return rc;
    if (!side.found) return 0;
    if (res.nvar + side.nl > MAXV) return HGX_ALN_DECLINE_VARS;
    for (int i = 0; i < side.nl; ++i) res.vl[res.nvar + i] = side.vl[i];
    res.nm += side.nm; res.nind += side.nind; res.nvar += side.nl; res.end = side.pos;
    res.locus = g; res.strand = R.strand; res.ok = 1;
    return 0;
}

// canon(a) of the gap tier: the smallest by (NM, indels, variants, pos0, list, descriptor) among the alignments through the anchor
// with ONE novel gap of up to `gap` bases and NM <= max_edits, the gap counted.  The anchor's bases are plain matches, so the gap is
// on one side: the canon is the smaller of (left side with the gap + plain right side) and (plain left side + right side with the
// gap), each made of its sides' smallest as hgx_aln_canon's is.  stk / cur: the outer walks' scratch, stk2 / cur2: the inner
// walks'; `sides`: three entries (the two sides' bests and the inner walks' best).
template <int MAXSTK, int MAXV>
HGX_ALN_HD int hgx_aln_gap_canon(const hgx_aln_view &V, const hgx_aln_read &R, int o, int32_t b, int max_edits, int gap, long max_steps,
                                 hgx_aln_frame *stk, int32_t *cur, hgx_aln_frame *stk2, int32_t *cur2, hgx_aln_side<MAXV> *sides,
                                 hgx_aln_res<MAXV> &res, uint32_t *gd_out) {
    const int g = hgx_aln_locus_of(V, b);
    const int32_t lo = V.bb_off[g], hi = V.bb_off[g + 1];
    res.ok = 0;
    *gd_out = 0;
    if (max_edits < 1) return 0;
    hgx_aln_no_memo memo;
    hgx_aln_side<MAXV> &x = sides[0], &y = sides[1];
    hgx_aln_gap_ctx<MAXV> gx{stk2, cur2, &sides[2], gap, 0, 0};
    // the gap on the left
    int rc = hgx_aln_left<MAXSTK, MAXV, hgx_aln_no_memo, false, 1>(V, R, lo, o, b, max_edits, max_steps, stk, cur, x, memo, 0, &gx);
    if (rc) return rc;
    if (x.found) {
        rc = hgx_aln_right<MAXSTK, MAXV>(V, R, hi, o + HGX_ALN_K, b + HGX_ALN_K, max_edits - x.nm, max_steps, stk, cur, y, memo);
        if (rc) return rc;
        if (y.found) {
            if ((rc = hgx_aln_join(x, y, g, R.strand, res))) return rc;
            *gd_out = gx.gd;
        }
    }
    // the gap on the right
    rc = hgx_aln_left<MAXSTK, MAXV>(V, R, lo, o, b, max_edits - 1, max_steps, stk, cur, x, memo);
    if (rc) return rc;
    if (!x.found) return 0;
    rc = hgx_aln_right<MAXSTK, MAXV, hgx_aln_no_memo, false, 1>(V, R, hi, o + HGX_ALN_K, b + HGX_ALN_K, max_edits - x.nm, max_steps, stk, cur,
                                                                 y, memo, 0, &gx);
    if (rc) return rc;
    if (!y.found) return 0;
    if (x.nl + y.nl > MAXV) return HGX_ALN_DECLINE_VARS;
    int c = -1;
    if (res.ok) {
        c = hgx_aln_cmp3(x.nm + y.nm, x.nind + y.nind, x.nl + y.nl, res.nm, res.nind, res.nvar);
        if (c == 0 && x.pos != res.pos0) c = x.pos < res.pos0 ? -1 : 1;
        for (int i = 0; c == 0 && i < res.nvar; ++i) {
            const int32_t u = i < x.nl ? x.vl[i] : y.vl[i - x.nl];
            c = u != res.vl[i] ? (u < res.vl[i] ? -1 : 1) : 0;
        }
        if (c == 0) c = gx.gd < *gd_out ? -1 : 1;
    }
    if (c < 0) {
        hgx_aln_join(x, y, g, R.strand, res);                  // (the lists fit: checked in front of the comparison)
        *gd_out = gx.gd;
    }
    return 0;
}

// the clip counts of an alignment in one word (clipL, clipR <= HGX_ALN_CLIP_MAX)
HGX_ALN_HD inline uint32_t hgx_aln_clip_pack(int clipL, int clipR) { return (uint32_t)clipL | ((uint32_t)clipR << 16); }
HGX_ALN_HD inline int hgx_aln_clip_l(uint32_t c) { return (int)(c & 0xffff); }
HGX_ALN_HD inline int hgx_aln_clip_r(uint32_t c) { return (int)(c >> 16); }
HGX_ALN_HD inline int hgx_aln_clip_total(uint32_t c) { return hgx_aln_clip_l(c) + hgx_aln_clip_r(c); }

// canon(a) of the clip tier: the smallest by (clipL + clipR, NM, indels, variants, pos0, list) among the alignments through the
// anchor with NM <= max_edits (<= HGX_ALN_CLIP_EDITS) and clipL + clipR <= clip.  For a fixed split (eL, eR) of the edits every
// component in front of pos0 is a sum over the sides and pos0 is the left side's, so the smallest combination of the split is made
// of each side's smallest entry for its e; the canon is the smallest over the splits.  `left` / `right`: scratch for the sides'
// HGX_ALN_CLIP_EDITS + 1 entries each.
template <int MAXSTK, int MAXV>
HGX_ALN_HD int hgx_aln_clip_canon(const hgx_aln_view &V, const hgx_aln_read &R, int o, int32_t b, int max_edits, int clip, long max_steps,
                                  hgx_aln_frame *stk, int32_t *cur, hgx_aln_side<MAXV> *left, hgx_aln_side<MAXV> *right,
                                  hgx_aln_res<MAXV> &res, uint32_t *clips) {
    const int g = hgx_aln_locus_of(V, b);
    const int32_t lo = V.bb_off[g], hi = V.bb_off[g + 1];
    res.ok = 0;
    *clips = 0;
    for (int e = 0; e <= HGX_ALN_CLIP_EDITS; ++e) left[e].found = right[e].found = 0;
    hgx_aln_no_memo memo;
    int rc = hgx_aln_left<MAXSTK, MAXV, hgx_aln_no_memo, true>(V, R, lo, o, b, max_edits, max_steps, stk, cur, *left, memo, clip);
    if (rc) return rc;
    rc = hgx_aln_right<MAXSTK, MAXV, hgx_aln_no_memo, true>(V, R, hi, o + HGX_ALN_K, b + HGX_ALN_K, max_edits, max_steps, stk, cur, *right,
                                                            memo, clip);
    if (rc) return rc;
    int bl = -1, br = -1;
    for (int el = 0; el <= max_edits; ++el) {
        if (!left[el].found) continue;
        for (int er = 0; el + er <= max_edits; ++er) {
            if (!right[er].found || left[el].nm + right[er].nm > clip) continue;
            const hgx_aln_side<MAXV> &x = left[el], &y = right[er];
            int c = -1;
            if (bl >= 0) {
                const hgx_aln_side<MAXV> &p = left[bl], &q = right[br];
                c = hgx_aln_cmp3(x.nm + y.nm, el + er, x.nind + y.nind, p.nm + q.nm, bl + br, p.nind + q.nind);
                if (c == 0) c = hgx_aln_cmp3(x.nl + y.nl, x.pos, 0, p.nl + q.nl, p.pos, 0);
                for (int i = 0; c == 0 && i < x.nl + y.nl; ++i) {
                    const int32_t u = i < x.nl ? x.vl[i] : y.vl[i - x.nl], w = i < p.nl ? p.vl[i] : q.vl[i - p.nl];
                    c = u != w ? (u < w ? -1 : 1) : 0;
                }
            }
            if (c < 0) { bl = el; br = er; }
        }
    }
    if (bl < 0) return 0;
    const hgx_aln_side<MAXV> &x = left[bl], &y = right[br];
    if ((rc = hgx_aln_join(x, y, g, R.strand, res))) return rc;
    res.nm = bl + br;                                          // (the entries' `nm` words hold the clip counts)
    *clips = hgx_aln_clip_pack(x.nm, y.nm);
    return 0;
}

// the eight words in front of an alignment's list: what the pair pick keeps of a candidate (the kernels: in LDS)
struct hgx_aln_head { int32_t ok, nm, nind, nvar, locus, strand, pos0, end; };

// the order of two alignments by their key (NM, indels, variants, locus, strand, pos0, list); H = hgx_aln_res or hgx_aln_head with
// the list beside it (read only where everything in front of it ties)
template <class H> HGX_ALN_HD int hgx_aln_key_cmp(const H &a, const int32_t *avl, const H &b, const int32_t *bvl) {
    int c = hgx_aln_cmp3(a.nm, a.nind, a.nvar, b.nm, b.nind, b.nvar);
    if (c) return c;
    c = hgx_aln_cmp3(a.locus, a.strand, a.pos0, b.locus, b.strand, b.pos0);
    for (int i = 0; c == 0 && i < a.nvar; ++i) c = avl[i] != bvl[i] ? (avl[i] < bvl[i] ? -1 : 1) : 0;
    return c;
}
template <int MAXV> HGX_ALN_HD int hgx_aln_res_cmp(const hgx_aln_res<MAXV> &a, const hgx_aln_res<MAXV> &b) {
    return hgx_aln_key_cmp(a, a.vl, b, b.vl);
}

// the read's alignment among the canon(a) of its anchors: index of the smallest (-1: unaligned) and NH, the number of placements
// of those with the smallest NM.  CLIP (the clip tier; clips[i] = hgx_aln_clip_pack of res[i]): the order is (clipL + clipR, the key,
// clipL) and NH is taken over those with the smallest (clipL + clipR, NM).
template <int MAXV, bool CLIP = false>
HGX_ALN_HD int hgx_aln_pick(const hgx_aln_res<MAXV> *res, int n, int *nh_out, const uint32_t *clips = nullptr) {
    int best = -1;
    for (int i = 0; i < n; ++i) {
        if (!res[i].ok) continue;
        int c = -1;
        if (best >= 0) {
            if constexpr (CLIP) {
                const int ti = hgx_aln_clip_total(clips[i]), tb = hgx_aln_clip_total(clips[best]);
                c = ti != tb ? (ti < tb ? -1 : 1) : hgx_aln_res_cmp(res[i], res[best]);
                if (c == 0 && clips[i] != clips[best]) c = hgx_aln_clip_l(clips[i]) < hgx_aln_clip_l(clips[best]) ? -1 : 1;
            } else c = hgx_aln_res_cmp(res[i], res[best]);
        }
        if (c < 0) best = i;
    }
    *nh_out = 0;
    if (best < 0) return -1;
    const int nm = res[best].nm;
    const int ct = CLIP ? hgx_aln_clip_total(clips[best]) : 0;
    // walk those with NM == nm in (locus, strand, pos0, slot) order
    int nh = 0, last = -1, cur_g = -1, cur_s = -1;
    int32_t cur_end = 0;
    for (;;) {
        int nxt = -1;
        for (int i = 0; i < n; ++i) {
            if (!res[i].ok || res[i].nm != nm) continue;
            if (CLIP && hgx_aln_clip_total(clips[i]) != ct) continue;
            if (last >= 0) {
                const int c = hgx_aln_cmp3(res[i].locus, res[i].strand, res[i].pos0, res[last].locus, res[last].strand, res[last].pos0);
                if (c < 0 || (c == 0 && i <= last)) continue;
            }
            if (nxt >= 0) {
                const int c = hgx_aln_cmp3(res[i].locus, res[i].strand, res[i].pos0, res[nxt].locus, res[nxt].strand, res[nxt].pos0);
                if (c > 0 || (c == 0 && i > nxt)) continue;
            }
            nxt = i;
        }
        if (nxt < 0) break;
        if (res[nxt].locus != cur_g || res[nxt].strand != cur_s || res[nxt].pos0 >= cur_end) {
            ++nh;
            cur_g = res[nxt].locus; cur_s = res[nxt].strand; cur_end = res[nxt].end;
        } else if (res[nxt].end > cur_end) cur_end = res[nxt].end;
        last = nxt;
    }
    *nh_out = nh;
    return best;
}
// the gap tier (gds[i] = the gap descriptor of res[i]): the plain pick and NH, and among the canons that equal the smallest in the
// whole key the one with the smallest descriptor
template <int MAXV> HGX_ALN_HD int hgx_aln_gap_pick(const hgx_aln_res<MAXV> *res, int n, int *nh_out, const uint32_t *gds) {
    int best = hgx_aln_pick(res, n, nh_out);
    for (int i = 0; best >= 0 && i < n; ++i)
        if (res[i].ok && gds[i] < gds[best] && hgx_aln_res_cmp(res[i], res[best]) == 0) best = i;
    return best;
}

// ---- the SAM record ----------------------------------------------------------------------------------------------------------------
struct hgx_aln_out {                       // p == nullptr: count only
    char *p;
    int64_t n;
    HGX_ALN_HD void ch(char c) { if (p) p[n] = c; ++n; }
    HGX_ALN_HD void str(const char *s, int len) { for (int i = 0; i < len; ++i) ch(s[i]); }
    HGX_ALN_HD void num(int64_t v) {
        char t[24];
        int k = 0;
        if (v < 0) { ch('-'); v = -v; }
        do { t[k++] = (char)('0' + v % 10); v /= 10; } while (v);
        while (k) ch(t[--k]);
    }
};

// one of CIGAR (what = 0), MD (1), Zs (2) of the walk, as simulate._truth_record renders them; returns the number of Zs items
// CLIP: the aligned part is read bases [clipL, L - clipR); the walk is that of the part alone (no indel in front of its first base,
// the first Zs gap counts from it) and the CIGAR carries the two S ops around it.
// GAP: `gd` = the alignment's novel gap (0: none), written on entry to its state, in front of the known indels of the state it
// leads to: D and ^bases for a deletion, I for an insertion, no Zs item (inserted bases count into the next item's gap, deleted
// bases do not), as synth._align_read writes them.
template <bool CLIP = false, bool GAP = false>
HGX_ALN_HD inline int hgx_aln_walk_text(const hgx_aln_view &V, const hgx_aln_read &R, int32_t pos0, const int32_t *vl, int nvar, int what,
                                        hgx_aln_out &out, int clipL = 0, int clipR = 0, uint32_t gd = 0) {
    const int r_first = CLIP ? clipL : 0, r_end = CLIP ? R.L - clipR : R.L;
    int r = r_first, vi = 0, md_run = 0, gap = 0, n_zs = 0, run = 0;
    char op = 0;
    int32_t P = pos0;
    auto cigar = [&](char o, int n) {
        if (op == o) run += n;
        else {
            if (op && what == 0) { out.num(run); out.ch(op); }
            op = o; run = n;
        }
    };
    auto zs = [&](char kind, int32_t v) {
        if (what == 2) {
            if (n_zs) out.ch(',');
            out.num(gap); out.ch('|'); out.ch(kind); out.ch('|');
            out.str(V.pool + V.vid_off[v], V.vid_len[v]);
        }
        ++n_zs;
    };
    if (CLIP && clipL > 0 && what == 0) { out.num(clipL); out.ch('S'); }
    while (r < r_end) {
        if constexpr (GAP) {
            if (gd && r == hgx_aln_gap_r(gd)) {
                const int n = hgx_aln_gap_len(gd);
                if (hgx_aln_gap_kind(gd) == 0) {
                    if (what == 1) { out.num(md_run); out.ch('^'); out.str(V.bb + P, n); }
                    md_run = 0;
                    cigar('D', n);
                    P += n;
                } else {
                    cigar('I', n);
                    gap += n;
                    r += n;
                }
                gd = 0;
            }
        }
        if (r > r_first) {
            const int32_t at = P;
            while (vi < nvar && V.vtype[vl[vi]] != HGX_ALN_SGL && V.vpos[vl[vi]] == at) {
                const int32_t v = vl[vi++];
                if (V.vtype[v] == HGX_ALN_DEL) {
                    const int n = V.vlen[v];
                    if (what == 1) { out.num(md_run); out.ch('^'); out.str(V.bb + P, n); }
                    md_run = 0;
                    cigar('D', n);
                    zs('D', v);
                    gap = 0;
                    P += n;
                } else {
                    int n = V.vlen[v];
                    if (n > r_end - r) n = r_end - r;
                    zs('I', v);
                    gap = n;
                    cigar('I', n);
                    r += n;
                }
            }
        }
        if (r >= r_end) break;
        if (R.at(r) == V.bb[P]) { ++md_run; ++gap; }
        else {
            if (what == 1) { out.num(md_run); out.ch(V.bb[P]); }
            md_run = 0;
            if (vi < nvar && V.vtype[vl[vi]] == HGX_ALN_SGL && V.vpos[vl[vi]] == P) { zs('S', vl[vi++]); gap = 0; }
            else ++gap;
        }
        cigar('M', 1);
        ++r;
        ++P;
    }
    if (what == 0 && op) { out.num(run); out.ch(op); }
    if (CLIP && clipR > 0 && what == 0) { out.num(clipR); out.ch('S'); }
    if (what == 1) out.num(md_run);
    return n_zs;
}

// FLAG / RNEXT / PNEXT / YT of a record: `mate` = the other mate's alignment (nullptr: single-end; ok == 0: unaligned)
template <class H> HGX_ALN_HD bool hgx_aln_concordant(const H &a, const H &b, int max_fragment) {
    if (!a.ok || !b.ok || a.locus != b.locus || a.strand == b.strand) return false;
    const H &plus = a.strand == 0 ? a : b, &minus = a.strand == 0 ? b : a;
    if (plus.pos0 > minus.pos0) return false;
    const int32_t left = a.pos0 < b.pos0 ? a.pos0 : b.pos0, right = a.end > b.end ? a.end : b.end;
    return right - left <= max_fragment;
}

// ---- pair-aware placement (opts.pair = 1; the rule in plain Python: tests/align_pair_ref.py) ----------------------------------------
// A mate's candidates are the canon(a) of its anchors (a canon reached through several anchors stands several times: harmless in
// all that follows).  A combination (c1, c2) takes one of each mate.  If one is concordant, the pair is written from the smallest
// concordant one by (NM1 + NM2, indels1 + indels2, variants1 + variants2, key of c1, key of c2); NH of both records = the number of
// distinct (placement of c1, placement of c2) over the concordant combinations of the smallest NM sum, the placements being those of
// the candidates these combinations use.  The pieces both routes run (the host route in loops, k_aln_pair_pick with lanes over
// mate 1's candidates):
//   hgx_aln_pair_sums   the first three components of a combination's order, packed: smaller word = smaller sums
//   hgx_aln_pair_cmp    the whole order of two combinations
//   hgx_aln_covers      x stands before e in (locus, strand, pos0, slot) order, on e's locus and strand, and ends behind e's pos0:
//                       e STARTS a placement iff no candidate in use covers it (the running maximum of the statement: every
//                       candidate of an earlier placement ends at or before the start of the later one), and e's placement is the
//                       last start at or before e
template <class H> HGX_ALN_HD uint64_t hgx_aln_pair_sums(const H &a, const H &b) {
    return ((uint64_t)(uint32_t)(a.nm + b.nm) << 42) | ((uint64_t)(uint32_t)(a.nind + b.nind) << 21) | (uint64_t)(uint32_t)(a.nvar + b.nvar);
}
HGX_ALN_HD inline int hgx_aln_pair_sums_nm(uint64_t sums) { return (int)(sums >> 42); }
template <class H>
HGX_ALN_HD int hgx_aln_pair_cmp(const H &a1, const int32_t *a1vl, const H &a2, const int32_t *a2vl, const H &b1, const int32_t *b1vl,
                                const H &b2, const int32_t *b2vl) {
    const uint64_t sa = hgx_aln_pair_sums(a1, a2), sb = hgx_aln_pair_sums(b1, b2);
    if (sa != sb) return sa < sb ? -1 : 1;
    const int c = hgx_aln_key_cmp(a1, a1vl, b1, b1vl);
    return c ? c : hgx_aln_key_cmp(a2, a2vl, b2, b2vl);
}
template <class H> HGX_ALN_HD bool hgx_aln_before(const H &x, int ix, const H &e, int ie) {      // in (locus, strand, pos0, slot) order
    const int c = hgx_aln_cmp3(x.locus, x.strand, x.pos0, e.locus, e.strand, e.pos0);
    return c < 0 || (c == 0 && ix < ie);
}
template <class H> HGX_ALN_HD bool hgx_aln_covers(const H &x, int ix, const H &e, int ie) {
    return x.locus == e.locus && x.strand == e.strand && hgx_aln_before(x, ix, e, ie) && x.end > e.pos0;
}

// where a record stands in coordinate order (hgx_align_more.order = 1; tests/align_resident_ref.py): the index of its RNAME in the
// header's @SQ order and POS - 1, from the values hgx_aln_line prints -- a clipped record's pos0 is its first ALIGNED base
template <class H> HGX_ALN_HD inline int32_t hgx_aln_pos_in_locus(const hgx_aln_view &V, const H &a) { return a.pos0 - V.bb_off[a.locus]; }
template <class H> HGX_ALN_HD inline uint64_t hgx_aln_coord_key(const hgx_aln_view &V, const H &a) {
    return ((uint64_t)(uint32_t)a.locus << 32) | (uint32_t)hgx_aln_pos_in_locus(V, a);
}

// the whole line (with its '\n'); `name` / `qual` as the file has them (qual == nullptr: 'I' x L)
template <int MAXV, bool CLIP = false, bool GAP = false>
HGX_ALN_HD void hgx_aln_line(const hgx_aln_view &V, const char *name, int name_len, const char *seq, const char *qual, int L,
                             const hgx_aln_res<MAXV> &a, int nh, const hgx_aln_res<MAXV> *mate, int mate_no, int max_fragment,
                             hgx_aln_out &out, int clipL = 0, int clipR = 0, uint32_t gd = 0) {
    const hgx_aln_read R{seq, L, a.strand};
    const int32_t lo = V.bb_off[a.locus];
    int flag = a.strand ? 16 : 0;
    const char *yt = "UU";
    int rnext = 0;                          // 0 '*', 1 '=', 2 the mate's locus
    int64_t pnext = 0;
    if (mate) {
        flag |= 1 | (mate_no == 0 ? 0x40 : 0x80);
        if (!mate->ok) { flag |= 8; rnext = 1; pnext = a.pos0 - lo + 1; yt = "UP"; }
        else {
            if (mate->strand) flag |= 0x20;
            rnext = mate->locus == a.locus ? 1 : 2;
            pnext = mate->pos0 - V.bb_off[mate->locus] + 1;
            if (hgx_aln_concordant(a, *mate, max_fragment)) { flag |= 2; yt = "CP"; }
            else yt = "DP";
        }
    }
    out.str(name, name_len); out.ch('\t');
    out.num(flag); out.ch('\t');
    out.str(V.pool + V.name_off[a.locus], V.name_len[a.locus]); out.ch('\t');
    out.num(a.pos0 - lo + 1); out.ch('\t');                     // (= hgx_aln_pos_in_locus + 1; spelled as before: k_aln_emit's code stays the parent's)
    out.num(nh == 1 ? 60 : 1); out.ch('\t');
    hgx_aln_walk_text<CLIP, GAP>(V, R, a.pos0, a.vl, a.nvar, 0, out, clipL, clipR, gd); out.ch('\t');
    if (rnext == 0) out.ch('*');
    else if (rnext == 1) out.ch('=');
    else out.str(V.pool + V.name_off[mate->locus], V.name_len[mate->locus]);
    out.ch('\t');
    out.num(pnext); out.ch('\t');
    out.ch('0'); out.ch('\t');
    for (int r = 0; r < L; ++r) out.ch(R.at(r));
    out.ch('\t');
    for (int r = 0; r < L; ++r) out.ch(qual ? qual[a.strand ? L - 1 - r : r] : 'I');
    out.str("\tNM:i:", 6); out.num(a.nm);
    out.str("\tMD:Z:", 6);
    hgx_aln_walk_text<CLIP, GAP>(V, R, a.pos0, a.vl, a.nvar, 1, out, clipL, clipR, gd);
    hgx_aln_out count{nullptr, 0};
    if (hgx_aln_walk_text<CLIP, GAP>(V, R, a.pos0, a.vl, a.nvar, 2, count, clipL, clipR, gd)) {
        out.str("\tZs:Z:", 6);
        hgx_aln_walk_text<CLIP, GAP>(V, R, a.pos0, a.vl, a.nvar, 2, out, clipL, clipR, gd);
    }
    out.str("\tNH:i:", 6); out.num(nh);
    out.str("\tYT:Z:", 6); out.str(yt, 2);
    out.ch('\n');
}

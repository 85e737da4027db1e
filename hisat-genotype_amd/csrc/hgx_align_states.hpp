// hgx_align_states.hpp -- the "hgx" aligner's search over STATES: the two tables of the pruned statement
// (tests/align_ref.py::_Search, prune=True) for one (oriented read, locus, window of backbone positions [wlo, whi)), compiled
// into the kernels (hgx_align.hip: a lane per column, rows in sequence) and into the host route (hgx_align_host.cpp: loops).
//
//   right[r][p], r = L .. 1   the smallest (NM, indels, variants, list) over the options at state (r, p): none, a known deletion
//                             that starts at p, a known insertion at p, or the insertion then the deletion; each followed by read
//                             base rr on backbone base pp and right[rr + 1][pp + 1].  An insertion cut by the read's end ends it.
//   left[r][q],  r = 0 .. L-1 the smallest (NM, indels, variants, pos0, list) over the arrivals at "read base r sits on q": plain,
//                             a deletion ending at q, an insertion at q, the insertion then the deletion; each preceded by read
//                             base r1 - 1 on backbone base p1 - 1 and left[r1 - 1][p1 - 1].
// A cell holds its cost, the option taken and pos0 (left) / the backbone end (right); lists are read back by walking the options.
// A tie in cost (and pos0) is decided by the lists in forward order, as the statement's min() decides it.  Right lists are in
// walk order: two chains are walked forwards to their first difference.  Left lists END at the cell: two chains are walked
// backwards in step (lists of equal cost have equal length) and the LAST difference seen is the first in forward order; the walk
// stops where the chains meet.
//
// EXACT, OR DECLINE.  An option that leads to a backbone position inside the locus but outside the window cannot be costed: the
// cell is marked POISONED, and so is every cell with an option that leads to a poisoned one.  canon() of an anchor that reads a
// poisoned cell answers HGX_ALN_DECLINE_WINDOW; nothing approximate is ever returned.
#pragma once
#include "hgx_align_core.hpp"

#define HGX_ALN_DECLINE_WINDOW 8
#define HGX_ALN_STATES_MAX_WINDOW 8192     // the widest window (backbone positions) the kernels take
#define HGX_ALN_STATES_MARGIN 128          // backbone positions beyond the hull of the anchors' diagonals, either side
#define HGX_ALN_ST_POISON 1

struct hgx_st_cell {
    int16_t nm, nind, nvar;                // nm < 0: no way within max_edits
    uint16_t flags;
    int32_t opt;                           // the option taken (index as hgx_aln_right / hgx_aln_left number them)
    int32_t pos;                           // left: pos0; right: the backbone end (global)
};

struct hgx_st_task {
    hgx_aln_read R;
    int32_t lo, hi;                        // the locus (global positions)
    int32_t wlo, whi;                      // the window, lo <= wlo < whi <= hi
    int32_t stride;                        // whi - wlo + 1 columns: right[r][whi] is the boundary column
    int32_t max_edits;
    hgx_st_cell *right, *left;             // (L + 1) * stride cells each
    HGX_ALN_HD hgx_st_cell &rc(int r, int32_t p) const { return right[(size_t)r * (size_t)stride + (size_t)(p - wlo)]; }
    HGX_ALN_HD hgx_st_cell &lc(int r, int32_t q) const { return left[(size_t)r * (size_t)stride + (size_t)(q - wlo)]; }
};

// cells of one table of a read of L bases over a window of w positions
HGX_ALN_HD inline size_t hgx_st_table_cells(int L, int32_t w) { return (size_t)(L + 1) * (size_t)(w + 1); }

// the window of a task whose anchors lie on the diagonals [dmin, dmax] (diagonal = backbone position - read offset)
HGX_ALN_HD inline void hgx_st_window(int32_t lo, int32_t hi, int32_t dmin, int32_t dmax, int L, int32_t margin, int32_t *wlo, int32_t *whi) {
    const int64_t a = (int64_t)dmin - margin, b = (int64_t)dmax + L + margin;
    *wlo = a < lo ? lo : (int32_t)a;
    *whi = b > hi ? hi : (int32_t)b;
}

// ---- options ---------------------------------------------------------------------------------------------------------------------
HGX_ALN_HD inline int hgx_st_right_nopt(const hgx_aln_view &V, int32_t P) {
    const int nd = V.dls_off[P + 1] - V.dls_off[P], ni = V.ins_off[P + 1] - V.ins_off[P];
    return 1 + nd + ni + nd * ni;
}
// option k at state (r, P): false if its insertion does not fit; else its events (insertion first), the read base rr and backbone
// base PP that follow
HGX_ALN_HD inline bool hgx_st_right_apply(const hgx_aln_view &V, const hgx_aln_read &R, int r, int32_t P, int k, int32_t *ev, int *nev,
                                          int *rr, int32_t *PP) {
    const int nd = V.dls_off[P + 1] - V.dls_off[P], ni = V.ins_off[P + 1] - V.ins_off[P];
    int32_t dv = -1, iv = -1;
    if (k == 0) {
    } else if (k <= nd) dv = V.dls[V.dls_off[P] + k - 1];
    else if (k <= nd + ni) iv = V.ins[V.ins_off[P] + k - 1 - nd];
    else {
        const int idx = k - 1 - nd - ni;
        dv = V.dls[V.dls_off[P] + idx / ni];
        iv = V.ins[V.ins_off[P] + idx % ni];
    }
    *nev = 0; *rr = r; *PP = P;
    if (iv >= 0) {
        const int n = hgx_aln_ins_fits(V, R, iv, r);
        if (n < 0) return false;
        *rr += n;
        ev[(*nev)++] = iv;
    }
    if (dv >= 0) { *PP += V.vlen[dv]; ev[(*nev)++] = dv; }
    return true;
}
HGX_ALN_HD inline int hgx_st_left_nopt(const hgx_aln_view &V, int32_t Q) {
    const int nde = V.dle_off[Q + 1] - V.dle_off[Q], niq = V.ins_off[Q + 1] - V.ins_off[Q];
    int nopt = 1 + nde + niq;
    for (int j = 0; j < nde; ++j) {
        const int32_t p1 = V.vpos[V.dle[V.dle_off[Q] + j]];
        nopt += V.ins_off[p1 + 1] - V.ins_off[p1];
    }
    return nopt;
}
// arrival k at "read base r sits on Q": false if its insertion does not fit; else its events BACKWARDS (the deletion, then the
// insertion) and the state (r1, P1) they start from
HGX_ALN_HD inline bool hgx_st_left_apply(const hgx_aln_view &V, const hgx_aln_read &R, int r, int32_t Q, int k, int32_t *ev, int *nev,
                                         int *r1, int32_t *P1) {
    const int nde = V.dle_off[Q + 1] - V.dle_off[Q], niq = V.ins_off[Q + 1] - V.ins_off[Q];
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
    *nev = 0; *r1 = r; *P1 = dv >= 0 ? V.vpos[dv] : Q;
    if (iv >= 0) {
        const int n = V.vlen[iv];
        if (r - n < 1 || hgx_aln_ins_fits(V, R, iv, r - n) != n) return false;
        *r1 = r - n;
    }
    if (dv >= 0) ev[(*nev)++] = dv;
    if (iv >= 0) ev[(*nev)++] = iv;
    return true;
}

// ---- the lists, read back by walking the options ---------------------------------------------------------------------------------
struct hgx_st_rit {                        // forwards from a right state
    int r;
    int32_t p, buf[3];
    int nb, ib, fin;
    HGX_ALN_HD void at(int r_, int32_t p_) { r = r_; p = p_; nb = ib = fin = 0; }
    HGX_ALN_HD void load(const hgx_aln_view &V, const hgx_st_task &T, int k) {
        int nev, rr;
        int32_t PP;
        nb = ib = 0;
        if (!hgx_st_right_apply(V, T.R, r, p, k, buf, &nev, &rr, &PP)) { fin = 1; return; }      // (never: k is an option that was costed)
        nb = nev;
        if (rr >= T.R.L) { fin = 1; return; }
        int32_t sv = -1;
        if (hgx_aln_base(V, T.R, rr, PP, &sv) == 2) buf[nb++] = sv;
        r = rr + 1;
        p = PP + 1;
    }
    HGX_ALN_HD int32_t next(const hgx_aln_view &V, const hgx_st_task &T) {
        while (ib == nb) {
            if (fin || r >= T.R.L) return -1;
            load(V, T, T.rc(r, p).opt);
        }
        return buf[ib++];
    }
};
struct hgx_st_lit {                        // backwards from a left state
    int r;
    int32_t q, buf[3];
    int nb, ib;
    HGX_ALN_HD void at(int r_, int32_t q_) { r = r_; q = q_; nb = ib = 0; }
    HGX_ALN_HD void load(const hgx_aln_view &V, const hgx_st_task &T, int k) {
        int nev, r1;
        int32_t P1;
        nb = ib = 0;
        if (!hgx_st_left_apply(V, T.R, r, q, k, buf, &nev, &r1, &P1)) { r = 0; return; }         // (never)
        nb = nev;
        int32_t sv = -1;
        if (hgx_aln_base(V, T.R, r1 - 1, P1 - 1, &sv) == 2) buf[nb++] = sv;
        r = r1 - 1;
        q = P1 - 1;
    }
    HGX_ALN_HD bool idle() const { return ib == nb; }
    HGX_ALN_HD int32_t next(const hgx_aln_view &V, const hgx_st_task &T) {
        while (ib == nb) {
            if (r <= 0) return -1;
            load(V, T, T.lc(r, q).opt);
        }
        return buf[ib++];
    }
};

// ---- one cell ----------------------------------------------------------------------------------------------------------------------
HGX_ALN_HD inline void hgx_st_right_cell(const hgx_aln_view &V, const hgx_st_task &T, int r, int32_t p) {
    hgx_st_cell c;
    c.nm = -1; c.nind = c.nvar = 0; c.flags = 0; c.opt = 0; c.pos = p;
    const int L = T.R.L;
    if (r == L) { c.nm = 0; T.rc(r, p) = c; return; }
    if (p >= T.hi) { T.rc(r, p) = c; return; }
    if (p >= T.whi) { c.flags = HGX_ALN_ST_POISON; T.rc(r, p) = c; return; }
    const int nopt = hgx_st_right_nopt(V, p);
    for (int k = 0; k < nopt; ++k) {
        int32_t ev[3], PP;
        int nev, rr;
        if (!hgx_st_right_apply(V, T.R, r, p, k, ev, &nev, &rr, &PP)) continue;
        int nm, nind, nvar;
        int32_t end;
        if (rr >= L) { nm = 0; nind = nvar = nev; end = PP; }
        else if (PP >= T.hi) continue;
        else if (PP >= T.whi) { c.flags |= HGX_ALN_ST_POISON; continue; }
        else {
            int32_t sv = -1;
            const int b = hgx_aln_base(V, T.R, rr, PP, &sv);
            const hgx_st_cell s = T.rc(rr + 1, PP + 1);
            c.flags |= s.flags & HGX_ALN_ST_POISON;
            if (s.nm < 0) continue;
            nm = s.nm + (b == 1);
            if (nm > T.max_edits) continue;
            nind = nev + s.nind; nvar = nev + (b == 2) + s.nvar; end = s.pos;
        }
        int cmp = c.nm < 0 ? -1 : hgx_aln_cmp3(nm, nind, nvar, c.nm, c.nind, c.nvar);
        if (cmp == 0) {
            hgx_st_rit a, b;
            a.at(r, p); a.load(V, T, k);
            b.at(r, p); b.load(V, T, c.opt);
            for (int i = 0; i < nvar && cmp == 0; ++i) {
                const int32_t x = a.next(V, T), y = b.next(V, T);
                cmp = x != y ? (x < y ? -1 : 1) : 0;
            }
        }
        if (cmp < 0) { c.nm = (int16_t)nm; c.nind = (int16_t)nind; c.nvar = (int16_t)nvar; c.opt = k; c.pos = end; }
    }
    T.rc(r, p) = c;
}

HGX_ALN_HD inline void hgx_st_left_cell(const hgx_aln_view &V, const hgx_st_task &T, int r, int32_t q) {
    hgx_st_cell c;
    c.nm = -1; c.nind = c.nvar = 0; c.flags = 0; c.opt = 0; c.pos = q;
    if (r == 0) { c.nm = 0; T.lc(r, q) = c; return; }
    const int nopt = hgx_st_left_nopt(V, q);
    for (int k = 0; k < nopt; ++k) {
        int32_t ev[3], P1;
        int nev, r1;
        if (!hgx_st_left_apply(V, T.R, r, q, k, ev, &nev, &r1, &P1)) continue;
        if (P1 - 1 < T.lo) continue;
        if (P1 - 1 < T.wlo) { c.flags |= HGX_ALN_ST_POISON; continue; }
        int32_t sv = -1;
        const int b = hgx_aln_base(V, T.R, r1 - 1, P1 - 1, &sv);
        const hgx_st_cell s = T.lc(r1 - 1, P1 - 1);
        c.flags |= s.flags & HGX_ALN_ST_POISON;
        if (s.nm < 0) continue;
        const int nm = s.nm + (b == 1);
        if (nm > T.max_edits) continue;
        const int nind = nev + s.nind, nvar = nev + (b == 2) + s.nvar;
        int cmp = c.nm < 0 ? -1 : hgx_aln_cmp3(nm, nind, nvar, c.nm, c.nind, c.nvar);
        if (cmp == 0 && s.pos != c.pos) cmp = s.pos < c.pos ? -1 : 1;
        if (cmp == 0) {
            hgx_st_lit x, y;
            x.at(r, q); x.load(V, T, k);
            y.at(r, q); y.load(V, T, c.opt);
            for (int i = 0; i < nvar; ++i) {
                if (x.idle() && y.idle() && x.r == y.r && x.q == y.q) break;           // the chains have met
                const int32_t a = x.next(V, T), d = y.next(V, T);
                if (a < 0 || d < 0) break;
                if (a != d) cmp = a < d ? -1 : 1;
            }
        }
        if (cmp < 0) { c.nm = (int16_t)nm; c.nind = (int16_t)nind; c.nvar = (int16_t)nvar; c.opt = k; c.pos = s.pos; }
    }
    T.lc(r, q) = c;
}

// ---- an anchor ---------------------------------------------------------------------------------------------------------------------
struct hgx_st_anchor { int32_t x, y; };    // read offset | strand << 16, global backbone position (the kernels' int2)
struct hgx_st_cost { int32_t nm, nind, nvar, pos0, end; };

// canon(o, b) as a cost: 1 = admissible, 0 = not, HGX_ALN_DECLINE_WINDOW + 16 = one of its two cells is poisoned
#define HGX_ST_POISONED (HGX_ALN_DECLINE_WINDOW + 16)
HGX_ALN_HD inline int hgx_st_canon_cost(const hgx_st_task &T, int o, int32_t b, hgx_st_cost *c) {
    const hgx_st_cell l = T.lc(o, b), r = T.rc(o + HGX_ALN_K, b + HGX_ALN_K);
    if ((l.flags | r.flags) & HGX_ALN_ST_POISON) return HGX_ST_POISONED;
    if (l.nm < 0 || r.nm < 0 || l.nm + r.nm > T.max_edits) return 0;
    c->nm = l.nm + r.nm; c->nind = l.nind + r.nind; c->nvar = l.nvar + r.nvar; c->pos0 = l.pos; c->end = r.pos;
    return 1;
}
// the order of the statement's canon keys within one task: (NM, indels, variants, pos0), lists aside
HGX_ALN_HD inline int hgx_st_cost_cmp(const hgx_st_cost &a, const hgx_st_cost &b) {
    const int c = hgx_aln_cmp3(a.nm, a.nind, a.nvar, b.nm, b.nind, b.nvar);
    return c ? c : a.pos0 != b.pos0 ? (a.pos0 < b.pos0 ? -1 : 1) : 0;
}
// the list of canon(o, b), nvar <= MAXV entries, forwards
HGX_ALN_HD inline void hgx_st_canon_list(const hgx_aln_view &V, const hgx_st_task &T, int o, int32_t b, int32_t *vl) {
    int n = T.lc(o, b).nvar;
    int k = n;
    hgx_st_lit x;
    x.at(o, b);
    while (k > 0) {
        const int32_t v = x.next(V, T);
        if (v < 0) break;
        vl[--k] = v;
    }
    hgx_st_rit y;
    y.at(o + HGX_ALN_K, b + HGX_ALN_K);
    const int m = T.rc(o + HGX_ALN_K, b + HGX_ALN_K).nvar;
    for (int i = 0; i < m; ++i) {
        const int32_t v = y.next(V, T);
        if (v < 0) break;
        vl[n++] = v;
    }
}

// the task's best canon among its anchors (o | strand << 16, b), in hgx_aln_res form, and the placements of those with the task's
// smallest NM.  res.ok = 0: none admissible.  `tmp` holds MAXV entries.  Returns 0 or a decline code.  (The kernels run the same
// three steps with lanes across the anchors: hgx_align.hip.)
template <int MAXV>
HGX_ALN_HD int hgx_st_reduce(const hgx_aln_view &V, const hgx_st_task &T, int locus, const hgx_st_anchor *anch, int n, hgx_aln_res<MAXV> &res,
                             int32_t *tmp, int *nh_out) {
    res.ok = 0;
    *nh_out = 0;
    hgx_st_cost best{0, 0, 0, 0, 0};
    for (int i = 0; i < n; ++i) {
        hgx_st_cost c;
        const int o = anch[i].x & 0xffff;
        const int rc = hgx_st_canon_cost(T, o, anch[i].y, &c);
        if (rc == HGX_ST_POISONED) return HGX_ALN_DECLINE_WINDOW;
        if (!rc) continue;
        int cmp = res.ok ? hgx_st_cost_cmp(c, best) : -1;
        if (cmp > 0) continue;
        if (c.nvar > MAXV) return HGX_ALN_DECLINE_VARS;
        if (cmp == 0) {
            hgx_st_canon_list(V, T, o, anch[i].y, tmp);
            for (int j = 0; cmp == 0 && j < c.nvar; ++j) cmp = tmp[j] != res.vl[j] ? (tmp[j] < res.vl[j] ? -1 : 1) : 0;
            if (cmp >= 0) continue;
            for (int j = 0; j < c.nvar; ++j) res.vl[j] = tmp[j];
        } else hgx_st_canon_list(V, T, o, anch[i].y, res.vl);
        best = c;
        res.ok = 1; res.nm = c.nm; res.nind = c.nind; res.nvar = c.nvar; res.locus = locus; res.strand = T.R.strand; res.pos0 = c.pos0;
        res.end = c.end;
    }
    if (!res.ok) return 0;
    int nh = 0;
    for (int i = 0; i < n; ++i) {
        hgx_st_cost c;
        if (hgx_st_canon_cost(T, anch[i].x & 0xffff, anch[i].y, &c) != 1 || c.nm != res.nm) continue;
        bool start = true;
        for (int j = 0; j < n && start; ++j) {
            hgx_st_cost d;
            if (j == i || hgx_st_canon_cost(T, anch[j].x & 0xffff, anch[j].y, &d) != 1 || d.nm != res.nm) continue;
            if ((d.pos0 < c.pos0 || (d.pos0 == c.pos0 && j < i)) && d.end > c.pos0) start = false;
        }
        nh += start;
    }
    *nh_out = nh;
    return 0;
}

// the read's pick among its tasks' bests: index of the smallest (-1: unaligned), NH = the placements of the tasks whose smallest
// NM is the read's (placements of different (locus, strand) never merge: hgx_aln_pick)
template <int MAXV>
HGX_ALN_HD int hgx_st_combine(const hgx_aln_res<MAXV> *res, const int32_t *task_nh, int n, int *nh_out) {
    int best = -1;
    for (int i = 0; i < n; ++i)
        if (res[i].ok && (best < 0 || hgx_aln_res_cmp(res[i], res[best]) < 0)) best = i;
    int nh = 0;
    for (int i = 0; best >= 0 && i < n; ++i)
        if (res[i].ok && res[i].nm == res[best].nm) nh += task_nh[i];
    *nh_out = nh;
    return best;
}

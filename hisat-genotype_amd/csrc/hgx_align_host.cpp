// hgx_align_host.cpp -- the "hgx" aligner's C-ABI, index, read files and HOST route.  The host route runs the
// same core as the kernels (hgx_align_core.hpp) with scratch large enough for every read the core takes: it is their checker
// and what finishes a call they decline.  Plain C++: this unit is also compiled on its own, with a main(), for the sanitizers.
#include <zlib.h>

#include <algorithm>
#include <climits>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <unordered_map>

#include "hgx_align.hpp"

extern "C" void hgx_set_error(const char *fmt, ...);
extern "C" const char *hgx_test_switch(const char *name);
void *hgx_host_alloc(size_t bytes);
#ifndef HGX_ALIGN_STANDALONE
#include "hgx_internal.hpp"              // hgx_alignment_from_reads: the hook to the front end's hgx_alignment
#include "hgx_reads.hpp"                 // hgx_reads: a read table made beforehand (hgx_align_reads_dev)
#else
struct hgx_reads;
#endif

namespace {
thread_local int g_route = 0, g_decline = 0;
thread_local int64_t g_reads = 0, g_aligned = 0, g_conc = 0;
thread_local int64_t g_st_reads = 0, g_st_anchors = 0, g_st_cells = 0;
thread_local int64_t g_pr_searched = 0, g_pr_placed = 0, g_pr_changed = 0;
thread_local int64_t g_tr[HGX_ALN_N_TIERS][3] = {};                      // per fallback tier: reads searched, reads written, their bases

template <class T> void csr(const std::vector<std::pair<int32_t, int32_t>> &items, int32_t n_pos, std::vector<T> &off, std::vector<T> &list) {
    off.assign((size_t)n_pos + 1, 0);
    for (auto &it : items) off[(size_t)it.first + 1]++;
    for (int32_t p = 0; p < n_pos; ++p) off[(size_t)p + 1] += off[p];
    list.resize(items.size());
    std::vector<T> fill(off.begin(), off.end() - 1);
    for (auto &it : items) list[(size_t)fill[it.first]++] = it.second;          // items arrive in variant order: kept per position
}

int add_pool(std::vector<char> &pool, const char *s, size_t n) {
    const int off = (int)pool.size();
    pool.insert(pool.end(), s, s + n);
    return off;
}

// ---- read files ------------------------------------------------------------------------------------------------------------------
int slurp(const char *path, std::string &out) {
    gzFile f = gzopen(path, "rb");                     // plain files pass through unchanged
    if (!f) { hgx_set_error("hgx_align_reads: cannot open %s", path); return HGX_EINVAL; }
    char buf[1 << 16];
    int n;
    while ((n = gzread(f, buf, sizeof buf)) > 0) out.append(buf, (size_t)n);
    gzclose(f);
    if (n < 0) { hgx_set_error("hgx_align_reads: %s is damaged", path); return HGX_EPARSE; }
    return HGX_OK;
}
int inflate_text(const char *p, size_t n, std::string &out) {
    if (n < 2 || (unsigned char)p[0] != 0x1f || (unsigned char)p[1] != 0x8b) { out.assign(p, n); return HGX_OK; }
    z_stream z;
    memset(&z, 0, sizeof z);
    if (inflateInit2(&z, 15 + 32) != Z_OK) return HGX_ENOMEM;
    z.next_in = (Bytef *)p;
    z.avail_in = (uInt)n;
    char buf[1 << 16];
    int rc = Z_OK;
    while (rc != Z_STREAM_END) {
        z.next_out = (Bytef *)buf;
        z.avail_out = sizeof buf;
        rc = inflate(&z, Z_NO_FLUSH);
        if (rc != Z_OK && rc != Z_STREAM_END) { inflateEnd(&z); hgx_set_error("hgx_align_reads: damaged gzip text"); return HGX_EPARSE; }
        out.append(buf, sizeof buf - z.avail_out);
        if (rc == Z_STREAM_END && z.avail_in > 0) { if (inflateReset(&z) != Z_OK) break; rc = Z_OK; }      // the next member
    }
    inflateEnd(&z);
    return HGX_OK;
}

struct Rec { size_t name, name_len, seq, seq_len; long qual; };          // offsets into the parsed text; qual < 0: none

// records of one FASTA / FASTQ text; multi-line FASTA bases are joined into `joined`
int parse_reads(const std::string &t, int fastq, std::vector<Rec> &recs, std::string &joined, std::vector<char> &from_joined) {
    size_t k = 0;
    const size_t n = t.size();
    auto line = [&](size_t &b, size_t &e) {            // next line [b, e) without its end, false at the end of the text
        if (k >= n) return false;
        b = k;
        const char *nl = (const char *)memchr(t.data() + k, '\n', n - k);
        e = nl ? (size_t)(nl - t.data()) : n;
        k = e + 1;
        if (e > b && t[e - 1] == '\r') --e;
        return true;
    };
    if (fastq < 0) fastq = n > 0 && t[0] == '@';
    size_t b, e;
    bool have = line(b, e);
    while (have) {
        if (e == b) { have = line(b, e); continue; }
        if (t[b] != (fastq ? '@' : '>')) { hgx_set_error("hgx_align_reads: neither FASTA nor FASTQ at byte %zu", b); return HGX_EPARSE; }
        Rec r{};
        r.name = b + 1;
        size_t q = b + 1;
        while (q < e && t[q] != ' ' && t[q] != '\t') ++q;
        r.name_len = q - r.name;
        if (fastq) {
            size_t sb, se, pb, pe, qb, qe;
            if (!line(sb, se) || !line(pb, pe) || !line(qb, qe) || qe - qb != se - sb) {
                hgx_set_error("hgx_align_reads: truncated FASTQ record at byte %zu", b);
                return HGX_EPARSE;
            }
            r.seq = sb; r.seq_len = se - sb; r.qual = (long)qb;
            from_joined.push_back(0);
            have = line(b, e);
        } else {
            size_t sb = 0, se = 0;
            int n_lines = 0;
            r.qual = -1;
            while ((have = line(b, e)) && !(e > b && t[b] == '>')) {
                if (n_lines == 0) { sb = b; se = e; }
                else {
                    if (n_lines == 1) { r.seq = joined.size(); joined.append(t, sb, se - sb); }
                    joined.append(t, b, e - b);
                }
                ++n_lines;
            }
            if (n_lines <= 1) { r.seq = sb; r.seq_len = se - sb; from_joined.push_back(0); }
            else { r.seq_len = joined.size() - r.seq; from_joined.push_back(1); }
        }
        recs.push_back(r);
    }
    return HGX_OK;
}

// the parsed inputs' records interleaved into the call's table: names, upper-case bases and qualities re-packed into out.text
int table_of(int n_inputs, const std::string *text, const std::vector<std::string> &joined, const std::vector<std::vector<Rec>> &recs,
             const std::vector<std::vector<char>> &fj, hgx_aln_reads &out) {
    if (n_inputs == 2 && recs[0].size() != recs[1].size()) {
        hgx_set_error("hgx_align_reads: %zu reads in the first file, %zu in the second", recs[0].size(), recs[1].size());
        return HGX_EPARSE;
    }
    out.paired = n_inputs == 2;
    for (size_t k = 0; k < recs[0].size(); ++k)
        for (int i = 0; i < n_inputs; ++i) {
            const Rec &r = recs[i][k];
            if (r.seq_len > HGX_ALN_MAX_READ) {
                hgx_set_error("hgx_align_reads: a read of %zu bases (the aligner takes up to %d)", r.seq_len, HGX_ALN_MAX_READ);
                return HGX_EINVAL;
            }
            out.name_off.push_back((int64_t)out.text.size());
            out.name_len.push_back((int32_t)r.name_len);
            out.text.insert(out.text.end(), text[i].data() + r.name, text[i].data() + r.name + r.name_len);
            out.seq_off.push_back((int64_t)out.text.size());
            out.len.push_back((int32_t)r.seq_len);
            const char *s = (fj[i][k] ? joined[i].data() : text[i].data()) + r.seq;
            for (size_t j = 0; j < r.seq_len; ++j) out.text.push_back((char)toupper((unsigned char)s[j]));
            if (r.qual >= 0) {
                out.qual_off.push_back((int64_t)out.text.size());
                out.text.insert(out.text.end(), text[i].data() + r.qual, text[i].data() + r.qual + r.seq_len);
            } else out.qual_off.push_back(-1);
        }
    return HGX_OK;
}

int load_reads(int n_inputs, const char *const *paths, const char *const *texts, const size_t *text_bytes, int fastq, hgx_aln_reads &out) {
    std::vector<std::string> text(n_inputs), joined(n_inputs);
    std::vector<std::vector<Rec>> recs(n_inputs);
    std::vector<std::vector<char>> fj(n_inputs);
    for (int i = 0; i < n_inputs; ++i) {
        int rc;
        if (paths) rc = slurp(paths[i], text[i]);
        else rc = inflate_text(texts[i], text_bytes[i], text[i]);
        if (rc) return rc;
        if ((rc = parse_reads(text[i], fastq, recs[i], joined[i], fj[i]))) return rc;
    }
    return table_of(n_inputs, text.data(), joined, recs, fj, out);
}

// ---- the host route ----------------------------------------------------------------------------------------------------------------
typedef hgx_aln_res<HGX_ALN_HOST_VARS> HostRes;

// the host route's MEMO (hgx_align_core.hpp): the best arrival at every state reached through a known indel, per side of one anchor
struct HostMemo {
    struct Arrival { int nm, nind, nl; std::vector<int32_t> list; };
    std::unordered_map<uint64_t, Arrival> seen[2];
    void reset() { seen[0].clear(); seen[1].clear(); }
    bool dominated(int side, int r, int32_t P, int nm, int nind, int nl, const int32_t *cur) {
        const uint64_t key = ((uint64_t)(uint32_t)r << 32) | (uint32_t)P;
        auto it = seen[side].find(key);
        if (it != seen[side].end()) {
            const Arrival &a = it->second;
            int c = hgx_aln_cmp3(nm, nind, nl, a.nm, a.nind, a.nl);
            // equal costs: equal lengths.  Side 0 lists are in walk order; side 1 lists are held backwards, and the part behind this
            // state is the TAIL of the alignment's list, so they are compared from their last element down
            for (int i = 0; c == 0 && i < nl; ++i) {
                const int32_t x = side ? cur[nl - 1 - i] : cur[i], y = side ? a.list[(size_t)(nl - 1 - i)] : a.list[(size_t)i];
                c = x != y ? (x < y ? -1 : 1) : 0;
            }
            if (c >= 0) return true;
        }
        seen[side][key] = Arrival{nm, nind, nl, std::vector<int32_t>(cur, cur + nl)};
        return false;
    }
};

struct HostScratch {
    std::vector<hgx_aln_frame> stk;
    std::vector<int32_t> cur;
    std::unique_ptr<hgx_aln_side<HGX_ALN_HOST_VARS>> side{new hgx_aln_side<HGX_ALN_HOST_VARS>};
    std::vector<HostRes> res;
    HostMemo memo;
    HostScratch() : stk(HGX_ALN_HOST_VARS), cur(HGX_ALN_HOST_VARS) {}
};

// every anchor of the read, both strands, in the order of the seed offsets and the table's probe run: fn(R, o, b) for the 16-mer at
// offset o of the oriented read R that sits at backbone position b.  A call that returns non-zero ends the loop with that value.
template <class F> int each_anchor(const hgx_aln_view &V, const char *seq, int L, F fn) {
    for (int strand = 0; strand < 2; ++strand) {
        const hgx_aln_read R{seq, L, strand};
        const int n_off = hgx_aln_n_offsets(L);
        for (int k = 0; k < n_off; ++k) {
            const int o = hgx_aln_offset(L, k);
            uint32_t code;
            if (!hgx_aln_seed_code(R, o, &code)) continue;
            for (uint32_t h = hgx_aln_hash(code) & V.hmask; V.hpos[h] >= 0; h = (h + 1) & V.hmask) {
                if (V.hkey[h] != code) continue;
                const int rc = fn(R, o, V.hpos[h]);
                if (rc) return rc;
            }
        }
    }
    return 0;
}

int align_one(const hgx_aln_view &V, const char *seq, int L, int max_edits, HostScratch &S, HostRes &best, int *nh, int *gave_up) {
    S.res.clear();
    const int rc = each_anchor(V, seq, L, [&](const hgx_aln_read &R, int o, int32_t b) {
        S.res.emplace_back();
        const int rc = hgx_aln_canon<HGX_ALN_HOST_VARS, HGX_ALN_HOST_VARS>(V, R, o, b, max_edits, HGX_ALN_HOST_STEPS, S.stk.data(), S.cur.data(),
                                                                          *S.side, S.res.back(), S.memo);
        if (!rc && !S.res.back().ok) S.res.pop_back();
        return rc;
    });
    best.ok = 0;
    if (rc) {                                 // beyond the host route's own limits: this read is left unaligned, the call goes on
        S.res.clear();
        *nh = 0;
        *gave_up = rc;
        return HGX_OK;
    }
    const int b = hgx_aln_pick(S.res.data(), (int)S.res.size(), nh);
    if (b >= 0) best = S.res[(size_t)b];
    return HGX_OK;
}

// ---- the fallback tier (opts.clip > 0: ClipTier; hgx_align_more.gap > 0: GapTier; rescue_clip > 0: RescueTier, both) for a read
// align_one found nothing for: a dearer
// canon over the same anchors, the tier's pick, one extra word for the record.  A tier names its canon, its pick, the scratch it
// needs besides HostScratch's stack and list, its argument of the call and the bases a word counts for, as the kernels' tiers do.
// Both run without the memo: it drops an arrival that a plain search never needs, and that arrival may be the prefix of the
// smallest way with a clip or a gap (hgx_align_core.hpp).
struct NoTier { static constexpr int id = HGX_ALN_TIER_NONE; static constexpr bool CLIP = false, GAP = false; };
struct ClipTier {
    static constexpr int id = HGX_ALN_TIER_CLIP;
    static constexpr bool CLIP = true, GAP = false;                      // (hgx_aln_line's)
    struct Scratch {
        std::vector<hgx_aln_side<HGX_ALN_HOST_VARS>> left, right;
        Scratch() : left(HGX_ALN_CLIP_EDITS + 1), right(HGX_ALN_CLIP_EDITS + 1) {}
    };
    static int canon(const hgx_aln_view &V, const hgx_aln_read &R, int o, int32_t b, int max_edits, int clip, HostScratch &S, Scratch &X,
                     HostRes &res, uint32_t *word) {
        return hgx_aln_clip_canon<HGX_ALN_HOST_VARS, HGX_ALN_HOST_VARS>(V, R, o, b, max_edits, clip, HGX_ALN_HOST_STEPS, S.stk.data(), S.cur.data(),
                                                                       X.left.data(), X.right.data(), res, word);
    }
    static int pick(const HostRes *res, int n, int *nh, const uint32_t *words) { return hgx_aln_pick<HGX_ALN_HOST_VARS, true>(res, n, nh, words); }
    static int bases(uint32_t word) { return hgx_aln_clip_total(word); }
};
struct GapTier {
    static constexpr int id = HGX_ALN_TIER_GAP;
    static constexpr bool CLIP = false, GAP = true;
    struct Scratch {
        std::vector<hgx_aln_frame> stk2;
        std::vector<int32_t> cur2;
        std::vector<hgx_aln_side<HGX_ALN_HOST_VARS>> sides;
        Scratch() : stk2(HGX_ALN_HOST_VARS), cur2(HGX_ALN_HOST_VARS), sides(3) {}
    };
    static int canon(const hgx_aln_view &V, const hgx_aln_read &R, int o, int32_t b, int max_edits, int gap, HostScratch &S, Scratch &X,
                     HostRes &res, uint32_t *word) {
        return hgx_aln_gap_canon<HGX_ALN_HOST_VARS, HGX_ALN_HOST_VARS>(V, R, o, b, max_edits, gap, HGX_ALN_HOST_STEPS, S.stk.data(), S.cur.data(),
                                                                      X.stk2.data(), X.cur2.data(), X.sides.data(), res, word);
    }
    static int pick(const HostRes *res, int n, int *nh, const uint32_t *words) { return hgx_aln_gap_pick(res, n, nh, words); }
    static int bases(uint32_t word) { return hgx_aln_gap_len(word); }
};
template <class T> struct TierScratch {
    typename T::Scratch own;
    std::vector<HostRes> res;
    std::vector<uint32_t> words;
};

// *word = 0 and best.ok = 0 where the tier finds nothing or passes a limit (*gave_up); true: the read has an anchor (it counts as
// searched)
template <class T>
bool align_one_tier(const hgx_aln_view &V, const char *seq, int L, int max_edits, int budget, HostScratch &S, TierScratch<T> &X, HostRes &best,
                    int *nh, uint32_t *word, int *gave_up) {
    X.res.clear();
    X.words.clear();
    best.ok = 0;
    *nh = 0;
    *word = 0;
    int n_anchors = 0;
    const int rc = each_anchor(V, seq, L, [&](const hgx_aln_read &R, int o, int32_t b) {
        ++n_anchors;
        X.res.emplace_back();
        X.words.push_back(0);
        const int rc = T::canon(V, R, o, b, max_edits, budget, S, X.own, X.res.back(), &X.words.back());
        if (!rc && !X.res.back().ok) { X.res.pop_back(); X.words.pop_back(); }
        return rc;
    });
    if (rc) *gave_up = rc;                    // beyond the host route's own limits: left unaligned, as align_one does
    else {
        const int b = T::pick(X.res.data(), (int)X.res.size(), nh, X.words.data());
        if (b >= 0) { best = X.res[(size_t)b]; *word = X.words[(size_t)b]; }
    }
    return n_anchors > 0;
}

// what the host route runs per read that align_one found nothing for.  rescue(): best / nh / the read's two words (at most one of
// them non-zero: which tier wrote the record); the counters are added to here.
template <class T> struct SingleTier : T {
    TierScratch<T> X;
    void rescue(const hgx_aln_view &V, const char *seq, int L, int max_edits, const int *budgets, HostScratch &S, HostRes &best, int *nh,
                uint32_t *clip_word, uint32_t *gap_word, int *gave_up) {
        uint32_t &word = T::CLIP ? *clip_word : *gap_word;
        if (align_one_tier<T>(V, seq, L, max_edits, budgets[T::CLIP ? 0 : 1], S, X, best, nh, &word, gave_up))
            hgx_align_tier_count(T::id, 1, word != 0, T::bases(word));
    }
};
// both tiers (hgx_align_more.rescue_clip > 0; the rule in plain Python: tests/align_rescue_ref.py): the clip tier's result C, then --
// unless cost(C) = clipL + clipR + NM_c <= 1, which no gap undercuts -- the gap tier's G; G is the record iff NM_g < cost(C)
struct RescueTier {
    static constexpr int id = HGX_ALN_TIER_CLIP | HGX_ALN_TIER_GAP;
    static constexpr bool CLIP = true, GAP = true;
    TierScratch<ClipTier> XC;
    TierScratch<GapTier> XG;
    HostRes g;
    void rescue(const hgx_aln_view &V, const char *seq, int L, int max_edits, const int *budgets, HostScratch &S, HostRes &best, int *nh,
                uint32_t *clip_word, uint32_t *gap_word, int *gave_up) {
        *gap_word = 0;
        if (!align_one_tier<ClipTier>(V, seq, L, max_edits, budgets[0], S, XC, best, nh, clip_word, gave_up)) return;
        const int cost = best.ok ? hgx_aln_clip_total(*clip_word) + best.nm : INT_MAX;
        bool searched = false;
        if (cost >= 2 && !*gave_up) {
            int gnh = 0;
            uint32_t gw = 0;
            searched = align_one_tier<GapTier>(V, seq, L, max_edits, budgets[1], S, XG, g, &gnh, &gw, gave_up);
            if (g.ok && g.nm < cost) {
                best = g;
                *nh = gnh;
                *gap_word = gw;
                *clip_word = 0;
            }
        }
        hgx_align_tier_count(HGX_ALN_TIER_CLIP, 1, *clip_word != 0, hgx_aln_clip_total(*clip_word));
        hgx_align_tier_count(HGX_ALN_TIER_GAP, searched, *gap_word != 0, hgx_aln_gap_len(*gap_word));
    }
};

// ---- the host route's states form (hgx_align_states.hpp): the same cells as the kernels, in loops --------------------------------
struct StatesScratch {
    struct A { int32_t strand, locus; hgx_st_anchor a; };
    std::vector<A> all;
    std::vector<hgx_st_anchor> anch;
    std::vector<hgx_st_cell> right, left;
    std::vector<HostRes> res;
    std::vector<int32_t> nh, tmp;
    StatesScratch() : tmp(HGX_ALN_HOST_VARS) {}
};

int align_one_states(const hgx_aln_view &V, const char *seq, int L, int max_edits, StatesScratch &S, HostRes &best, int *nh, int *gave_up) {
    S.all.clear();
    S.res.clear();
    S.nh.clear();
    best.ok = 0;
    *nh = 0;
    each_anchor(V, seq, L, [&](const hgx_aln_read &R, int o, int32_t b) {
        S.all.push_back({R.strand, hgx_aln_locus_of(V, b), {o | (R.strand << 16), b}});
        return 0;
    });
    if (S.all.empty()) return HGX_OK;
    std::stable_sort(S.all.begin(), S.all.end(), [](const StatesScratch::A &a, const StatesScratch::A &b) {
        return a.strand != b.strand ? a.strand < b.strand : a.locus < b.locus;
    });
    int64_t cells = 0;
    for (size_t first = 0; first < S.all.size();) {
        size_t last = first;
        int32_t dmin = INT32_MAX, dmax = INT32_MIN;
        S.anch.clear();
        for (; last < S.all.size() && S.all[last].strand == S.all[first].strand && S.all[last].locus == S.all[first].locus; ++last) {
            const int32_t d = S.all[last].a.y - (S.all[last].a.x & 0xffff);
            dmin = std::min(dmin, d);
            dmax = std::max(dmax, d);
            S.anch.push_back(S.all[last].a);
        }
        hgx_st_task T{};
        T.R = hgx_aln_read{seq, L, S.all[first].strand};
        T.lo = V.bb_off[S.all[first].locus];
        T.hi = V.bb_off[S.all[first].locus + 1];
        T.max_edits = std::min(max_edits, L);
        S.res.emplace_back();
        S.nh.push_back(0);
        // the kernels decline a window they cannot take; here it is widened until nothing leaves it (the whole locus at the latest)
        for (int32_t margin = HGX_ALN_STATES_MARGIN;; margin = margin > (1 << 28) ? margin : margin * 4) {
            hgx_st_window(T.lo, T.hi, dmin, dmax, L, margin, &T.wlo, &T.whi);
            T.stride = T.whi - T.wlo + 1;
            const size_t n_cells = hgx_st_table_cells(L, T.whi - T.wlo);
            S.right.resize(n_cells);
            S.left.resize(n_cells);
            T.right = S.right.data();
            T.left = S.left.data();
            for (int r = L; r >= 1; --r)
                for (int32_t p = T.wlo; p <= T.whi; ++p) hgx_st_right_cell(V, T, r, p);
            for (int r = 0; r < L; ++r)
                for (int32_t q = T.wlo; q < T.whi; ++q) hgx_st_left_cell(V, T, r, q);
            cells += 2 * (int64_t)L * (T.whi - T.wlo);
            const int rc = hgx_st_reduce(V, T, S.all[first].locus, S.anch.data(), (int)S.anch.size(), S.res.back(), S.tmp.data(), &S.nh.back());
            if (rc == HGX_ALN_DECLINE_WINDOW && (T.wlo > T.lo || T.whi < T.hi)) continue;
            if (rc) {
                best.ok = 0;
                *nh = 0;
                *gave_up = rc;
                return HGX_OK;
            }
            break;
        }
        first = last;
    }
    hgx_align_states_count(1, (int64_t)S.all.size(), cells);
    const int b = hgx_st_combine(S.res.data(), S.nh.data(), (int)S.res.size(), nh);
    if (b >= 0) best = S.res[(size_t)b];
    return HGX_OK;
}

// the pair pick (hgx_align_core.hpp) in plain loops over the two mates' candidates: false = no concordant combination
struct PairScratch {
    std::vector<HostRes> cand[2];
    std::vector<char> used[2];
    std::vector<int32_t> place[2], order;
    std::vector<uint64_t> seen;
};

bool pair_pick(PairScratch &S, int max_fragment, int *b1, int *b2, int *nh) {
    const std::vector<HostRes> &c1 = S.cand[0], &c2 = S.cand[1];
    const int n1 = (int)c1.size(), n2 = (int)c2.size();
    int a = -1, b = -1;
    for (int i = 0; i < n1; ++i)
        for (int j = 0; j < n2; ++j)
            if (hgx_aln_concordant(c1[i], c2[j], max_fragment) &&
                (a < 0 || hgx_aln_pair_cmp(c1[i], c1[i].vl, c2[j], c2[j].vl, c1[a], c1[a].vl, c2[b], c2[b].vl) < 0)) { a = i; b = j; }
    if (a < 0) return false;
    const int nm = c1[a].nm + c2[b].nm;
    S.used[0].assign((size_t)n1, 0);
    S.used[1].assign((size_t)n2, 0);
    for (int i = 0; i < n1; ++i)
        for (int j = 0; j < n2; ++j)
            if (c1[i].nm + c2[j].nm == nm && hgx_aln_concordant(c1[i], c2[j], max_fragment)) S.used[0][(size_t)i] = S.used[1][(size_t)j] = 1;
    for (int m = 0; m < 2; ++m) {                        // place[m][e]: the candidate that starts e's placement
        const std::vector<HostRes> &c = S.cand[m];
        const std::vector<char> &u = S.used[m];
        const int n = (int)c.size();
        S.order.clear();
        for (int e = 0; e < n; ++e)
            if (u[(size_t)e]) S.order.push_back(e);
        std::sort(S.order.begin(), S.order.end(), [&](int x, int y) { return hgx_aln_before(c[(size_t)x], x, c[(size_t)y], y); });
        S.place[m].assign((size_t)n, -1);
        int cur = -1;
        for (size_t k = 0; k < S.order.size(); ++k) {
            const int e = S.order[k];
            bool start = true;
            for (size_t q = 0; q < k && start; ++q) start = !hgx_aln_covers(c[(size_t)S.order[q]], S.order[q], c[(size_t)e], e);
            if (start) cur = e;
            S.place[m][(size_t)e] = cur;
        }
    }
    S.seen.clear();
    for (int i = 0; i < n1; ++i)
        for (int j = 0; j < n2; ++j)
            if (c1[i].nm + c2[j].nm == nm && hgx_aln_concordant(c1[i], c2[j], max_fragment))
                S.seen.push_back(((uint64_t)(uint32_t)S.place[0][(size_t)i] << 32) | (uint32_t)S.place[1][(size_t)j]);
    std::sort(S.seen.begin(), S.seen.end());
    *nh = (int)(std::unique(S.seen.begin(), S.seen.end()) - S.seen.begin());
    *b1 = a;
    *b2 = b;
    return true;
}

// T: what the call runs for a read without an end-to-end alignment (NoTier: nothing; SingleTier<ClipTier>, SingleTier<GapTier>,
// RescueTier); it also settles which hgx_aln_line writes the records.  budgets[0 .. 1]: the clip tier's and the gap tier's.
template <class T>
int host_route(const hgx_align_index *ix, const hgx_aln_reads &reads, const hgx_align_opts *o, const int *budgets, std::string &body,
               int64_t *aligned, int64_t *conc, int *gave_up) {
    const hgx_aln_view &V = ix->hv;
    HostScratch S;
    StatesScratch SS;
    PairScratch PS;
    T TS;
    uint32_t cw[2] = {0, 0}, gw[2] = {0, 0};             // each mate's clip counts and gap descriptor (0: that tier did not write it)
    const int per = reads.paired ? 2 : 1;
    const bool pair_aware = per == 2 && o->pair == 1;
    std::vector<HostRes> best(per);
    int nh[2] = {0, 0};
    std::vector<char> line;
    for (size_t k = 0; k < reads.n(); k += per) {
        for (int m = 0; m < per; ++m) {
            const char *seq = reads.text.data() + reads.seq_off[k + m];
            int gu = 0;                                  // this read's own "gave up"
            const int rc = o->search ? align_one_states(V, seq, reads.len[k + m], o->max_edits, SS, best[m], &nh[m], &gu)
                                     : align_one(V, seq, reads.len[k + m], o->max_edits, S, best[m], &nh[m], &gu);
            if (rc) return rc;
            if (pair_aware) PS.cand[m].swap(S.res);      // (a mate that gave up: none)
            cw[m] = gw[m] = 0;
            if constexpr (T::id != HGX_ALN_TIER_NONE)
                if (!best[m].ok && !gu)                  // no end-to-end alignment: the tier(s) over the same anchors
                    TS.rescue(V, seq, reads.len[k + m], o->max_edits, budgets, S, best[m], &nh[m], &cw[m], &gw[m], &gu);
            if (gu) *gave_up = gu;
        }
        if (pair_aware && best[0].ok && best[1].ok) {
            int b1 = -1, b2 = -1, pnh = 0;
            const bool placed = pair_pick(PS, o->max_fragment, &b1, &b2, &pnh);
            bool changed = false;
            if (placed) {
                const HostRes &n1 = PS.cand[0][(size_t)b1], &n2 = PS.cand[1][(size_t)b2];
                changed = hgx_aln_res_cmp(n1, best[0]) != 0 || hgx_aln_res_cmp(n2, best[1]) != 0 || nh[0] != pnh || nh[1] != pnh;
                best[0] = n1;
                best[1] = n2;
                nh[0] = nh[1] = pnh;
            }
            hgx_align_pairs_count(1, placed, changed);
        }
        if (per == 2 && hgx_aln_concordant(best[0], best[1], o->max_fragment)) ++*conc;
        for (int m = 0; m < per; ++m) {
            if (!best[m].ok) continue;
            ++*aligned;
            const size_t i = k + m;
            const char *qual = reads.qual_off[i] >= 0 ? reads.text.data() + reads.qual_off[i] : nullptr;
            const HostRes *mate = per == 2 ? &best[1 - m] : nullptr;
            hgx_aln_out cnt{nullptr, 0}, w{nullptr, 0};
            for (int pass = 0; pass < 2; ++pass) {       // the size, then the bytes
                // (words of 0, a read aligned end to end, give the plain line with any tier's arguments, as in k_aln_emit)
                hgx_aln_line<HGX_ALN_HOST_VARS, T::CLIP, T::GAP>(V, reads.text.data() + reads.name_off[i], reads.name_len[i],
                                                                 reads.text.data() + reads.seq_off[i], qual, reads.len[i], best[m], nh[m], mate, m,
                                                                 o->max_fragment, pass ? w : cnt, hgx_aln_clip_l(cw[m]), hgx_aln_clip_r(cw[m]),
                                                                 gw[m]);
                if (!pass) {
                    line.resize((size_t)cnt.n);
                    w.p = line.data();
                }
            }
            body.append(line.data(), line.size());
        }
    }
    return HGX_OK;
}
}      // namespace

// the loader in its two halves, for a table made ahead of the call (hgx_reads.hpp)
int hgx_aln_inflate_input(const char *path, const char *text, size_t n, std::string &out) {
    return path ? slurp(path, out) : inflate_text(text, n, out);
}
int hgx_aln_reads_of_texts(int n_inputs, const std::string *text, int fastq, hgx_aln_reads &out) {
    std::vector<std::string> joined(n_inputs);
    std::vector<std::vector<Rec>> recs(n_inputs);
    std::vector<std::vector<char>> fj(n_inputs);
    for (int i = 0; i < n_inputs; ++i) {
        const int rc = parse_reads(text[i], fastq, recs[i], joined[i], fj[i]);
        if (rc) return rc;
    }
    return table_of(n_inputs, text, joined, recs, fj, out);
}

void hgx_align_states_count(int64_t reads, int64_t anchors, int64_t cells) {
    g_st_reads += reads;
    g_st_anchors += anchors;
    g_st_cells += cells;
}
void hgx_align_tier_count(int tier, int64_t searched, int64_t found, int64_t bases) {
    g_tr[tier][0] += searched;
    g_tr[tier][1] += found;
    g_tr[tier][2] += bases;
}
void hgx_align_pairs_count(int64_t searched, int64_t placed, int64_t changed) {
    g_pr_searched += searched;
    g_pr_placed += placed;
    g_pr_changed += changed;
}

// hgx_align_more.order = 1 on the host: what hgx_write_bam's std::stable_sort by (rid, pos0) does to the stored file, on the lines
void hgx_align_order_body(const hgx_align_index *ix, std::string &body) {
    struct Line { uint64_t key; size_t off, len; };
    std::unordered_map<std::string, uint32_t> rid;
    for (int g = ix->hv.n_loci - 1; g >= 0; --g) rid[std::string(ix->pool.data() + ix->name_off[g], (size_t)ix->name_len[g])] = (uint32_t)g;
    std::vector<Line> lines;
    for (size_t at = 0; at < body.size();) {
        const char *p = body.data() + at, *e = (const char *)memchr(p, '\n', body.size() - at);
        const size_t len = e ? (size_t)(e - p) + 1 : body.size() - at;
        const char *f = p, *end = p + len;
        for (int k = 0; k < 2 && f < end; ++k) { f = (const char *)memchr(f, '\t', (size_t)(end - f)); f = f ? f + 1 : end; }      // RNAME
        const char *t = (const char *)memchr(f, '\t', (size_t)(end - f));
        uint64_t key = ~0ull;                                // (a line without the two fields: behind the records, where it stood)
        if (t) {
            const auto it = rid.find(std::string(f, (size_t)(t - f)));
            const uint64_t pos = strtoull(t + 1, nullptr, 10);
            if (it != rid.end() && pos > 0) key = ((uint64_t)it->second << 32) | (uint32_t)(pos - 1);
        }
        lines.push_back(Line{key, at, len});
        at += len;
    }
    std::stable_sort(lines.begin(), lines.end(), [](const Line &a, const Line &b) { return a.key < b.key; });
    std::string out;
    out.reserve(body.size());
    for (const Line &l : lines) out.append(body, l.off, l.len);
    body.swap(out);
}

#ifdef HGX_ALIGN_STANDALONE
// the stand-alone build (tools/align_host_main.cpp) has no kernels and none of the library around it
extern "C" void hgx_set_error(const char *fmt, ...) { va_list ap; va_start(ap, fmt); vfprintf(stderr, fmt, ap); va_end(ap); fputc('\n', stderr); }
extern "C" const char *hgx_test_switch(const char *) { return "host"; }
void *hgx_host_alloc(size_t bytes) { return malloc(bytes); }
int hgx_align_device(hgx_align_index *, const hgx_aln_reads &, const hgx_align_opts *, int, int, std::string &, int64_t *, int64_t *,
                     int *decline, hgx_aln_ordered *) {
    *decline = HGX_ALN_DECLINE_SWITCH;
    return HGX_OK;
}
void hgx_align_device_free(hgx_align_index *) {}
#endif

extern "C" int hgx_align_index_create(hgx_align_index **out, int32_t n_loci, const char *const *names, const char *const *backbones,
                                      const int32_t *var_off, const int32_t *var_type, const int32_t *var_pos,
                                      const char *const *var_data, const char *const *var_id) {
    if (!out || n_loci < 1 || !names || !backbones || !var_off) {
        hgx_set_error("invalid argument: hgx_align_index_create");
        return HGX_EINVAL;
    }
    *out = nullptr;
    try {
        std::unique_ptr<hgx_align_index> ix(new hgx_align_index);
        ix->bb_off.push_back(0);
        for (int g = 0; g < n_loci; ++g) {
            const size_t n = strlen(backbones[g]);
            for (size_t k = 0; k < n; ++k) ix->bb.push_back((char)toupper((unsigned char)backbones[g][k]));
            ix->bb_off.push_back((int32_t)ix->bb.size());
            ix->name_off.push_back(add_pool(ix->pool, names[g], strlen(names[g])));
            ix->name_len.push_back((int32_t)strlen(names[g]));
            ix->header += "@SQ\tSN:" + std::string(names[g]) + "\tLN:" + std::to_string(n) + "\n";
        }
        const int32_t n_pos = (int32_t)ix->bb.size();
        std::vector<std::pair<int32_t, int32_t>> sgl, dls, dle, ins;
        const int32_t n_vars = var_off[n_loci];
        for (int g = 0; g < n_loci; ++g) {
            const int32_t lo = ix->bb_off[g], hi = ix->bb_off[g + 1];
            for (int32_t v = var_off[g]; v < var_off[g + 1]; ++v) {
                const int32_t P = lo + var_pos[v];
                ix->vtype.push_back((uint8_t)var_type[v]);
                ix->vpos.push_back(P);
                ix->vid_off.push_back(add_pool(ix->pool, var_id[v], strlen(var_id[v])));
                ix->vid_len.push_back((int32_t)strlen(var_id[v]));
                const bool inside = var_pos[v] >= 0 && P < hi;      // a variant off the backbone can never be walked
                if (var_type[v] == HGX_ALN_SGL) {
                    ix->vlen.push_back(1);
                    ix->vdata.push_back(toupper((unsigned char)var_data[v][0]));
                    if (inside) sgl.emplace_back(P, v);
                } else if (var_type[v] == HGX_ALN_DEL) {
                    const int32_t n = atoi(var_data[v]);
                    ix->vlen.push_back(n);
                    ix->vdata.push_back(0);
                    if (inside && n > 0 && P + n < hi) { dls.emplace_back(P, v); dle.emplace_back(P + n, v); }
                } else if (var_type[v] == HGX_ALN_INS) {
                    const size_t n = strlen(var_data[v]);
                    ix->vlen.push_back((int32_t)n);
                    const int off = (int)ix->pool.size();
                    for (size_t k = 0; k < n; ++k) ix->pool.push_back((char)toupper((unsigned char)var_data[v][k]));
                    ix->vdata.push_back(off);
                    if (inside && n > 0) ins.emplace_back(P, v);
                } else {
                    hgx_set_error("hgx_align_index_create: variant type %d", var_type[v]);
                    return HGX_EINVAL;
                }
            }
        }
        (void)n_vars;
        csr(sgl, n_pos, ix->sgl_off, ix->sgl);
        csr(dls, n_pos, ix->dls_off, ix->dls);
        csr(dle, n_pos, ix->dle_off, ix->dle);
        csr(ins, n_pos, ix->ins_off, ix->ins);
        // the 16-mers of every backbone (windows with a non-ACGT base are not indexed)
        std::vector<std::pair<uint32_t, int32_t>> kmers;
        for (int g = 0; g < n_loci; ++g) {
            const hgx_aln_read R{ix->bb.data() + ix->bb_off[g], ix->bb_off[g + 1] - ix->bb_off[g], 0};
            for (int p = 0; p + HGX_ALN_K <= R.L; ++p) {
                uint32_t code;
                if (hgx_aln_seed_code(R, p, &code)) kmers.emplace_back(code, ix->bb_off[g] + p);
            }
        }
        uint32_t cap = 16;
        while (cap < 2 * kmers.size() + 1) cap <<= 1;
        ix->hkey.assign(cap, 0);
        ix->hpos.assign(cap, -1);
        for (auto &km : kmers) {
            uint32_t h = hgx_aln_hash(km.first) & (cap - 1);
            while (ix->hpos[h] >= 0) h = (h + 1) & (cap - 1);
            ix->hkey[h] = km.first;
            ix->hpos[h] = km.second;
        }
        hgx_aln_view &V = ix->hv;
        V.bb = ix->bb.data(); V.bb_off = ix->bb_off.data(); V.n_loci = n_loci; V.n_pos = n_pos;
        V.hkey = ix->hkey.data(); V.hpos = ix->hpos.data(); V.hmask = cap - 1;
        V.vtype = ix->vtype.data(); V.vpos = ix->vpos.data(); V.vlen = ix->vlen.data(); V.vdata = ix->vdata.data();
        V.vid_off = ix->vid_off.data(); V.vid_len = ix->vid_len.data();
        V.name_off = ix->name_off.data(); V.name_len = ix->name_len.data(); V.pool = ix->pool.data();
        V.sgl_off = ix->sgl_off.data(); V.sgl = ix->sgl.data(); V.dls_off = ix->dls_off.data(); V.dls = ix->dls.data();
        V.dle_off = ix->dle_off.data(); V.dle = ix->dle.data(); V.ins_off = ix->ins_off.data(); V.ins = ix->ins.data();
        *out = ix.release();
        return HGX_OK;
    } catch (const std::exception &e) {
        hgx_set_error("hgx_align_index_create: %s", e.what());
        return HGX_ENOMEM;
    }
}

extern "C" int hgx_align_index_free(hgx_align_index *ix) {
    if (ix) {
        hgx_align_device_free(ix);
        delete ix;
    }
    return HGX_OK;
}

extern "C" int hgx_align_reads(hgx_align_index *ix, int32_t n_inputs, const char *const *paths, const char *const *texts,
                               const size_t *text_bytes, const hgx_align_opts *opts, char **sam_out, size_t *n_bytes_out) {
    return hgx_align_reads_x(ix, n_inputs, paths, texts, text_bytes, opts, nullptr, sam_out, n_bytes_out);
}

// hgx_align_reads_x (kept == nullptr: the text to *sam_out) and hgx_align_reads_resident (kept != nullptr: coordinate order
// whatever `more` says, the ordered text -- header in front -- left in HBM by the kernels' route (kept->d_text) or, where the host
// route gave the bytes, in *host_text).  dr != nullptr (hgx_align_reads_dev, hgx_align_reads_dev_resident): the loading step is
// replaced by a table made beforehand -- in HBM (dr->route == 2: the kernels run over it as it lies; where they decline, text and
// table are copied down for the host route) or the loader's (dr->host).
static int align_call(hgx_align_index *ix, int32_t n_inputs, const char *const *paths, const char *const *texts, const size_t *text_bytes,
                      const hgx_align_opts *opts, const hgx_align_more *more, char **sam_out, size_t *n_bytes_out, hgx_aln_ordered *kept,
                      std::string *host_text, const hgx_reads *dr = nullptr) {
    // (`more` is read up to the fields this build knows and no further than more->bytes: 8 = the first version, `gap` alone)
    if (more && more->bytes < 8) {
        hgx_set_error("invalid argument: hgx_align_reads_x (more.bytes)");
        return HGX_EINVAL;
    }
    const int gap = more ? more->gap : 0;
    const int rescue = more && more->bytes >= 12 ? more->rescue_clip : 0;
    const int order = kept ? 1 : more && more->bytes >= 16 ? more->order : 0;
    if (order < 0 || order > 1) {
        hgx_set_error("invalid argument: hgx_align_reads_x (order)");
        return HGX_EINVAL;
    }
    if (opts && (gap < 0 || gap > HGX_ALN_GAP_MAX || (gap && (opts->search || opts->pair || opts->clip)))) {      // (both tiers: rescue_clip)
        hgx_set_error("invalid argument: hgx_align_reads_x (gap)");
        return HGX_EINVAL;
    }
    // (rescue_clip > 0 with search, pair or opts.clip: gap == 0 or refused above)
    if (opts && (rescue < 0 || rescue > HGX_ALN_CLIP_MAX || (rescue && (gap <= 0 || opts->max_edits > HGX_ALN_CLIP_EDITS)))) {
        hgx_set_error("invalid argument: hgx_align_reads_x (rescue_clip)");
        return HGX_EINVAL;
    }
    if (!ix || (!dr && ((n_inputs != 1 && n_inputs != 2) || (!paths && !(texts && text_bytes)))) || !opts || (!kept && (!sam_out || !n_bytes_out)) ||
        opts->max_edits < 0 || opts->route < 0 || opts->route > 2 || opts->search < 0 || opts->search > 2 ||
        opts->pair < 0 || opts->pair > 1 || (opts->pair && opts->search) ||      // (the states form keeps no candidates to pair)
        opts->clip < 0 || opts->clip > HGX_ALN_CLIP_MAX ||
        (opts->clip && (opts->search || opts->pair || opts->max_edits > HGX_ALN_CLIP_EDITS))) {      // (neither keeps clip counts)
        hgx_set_error("invalid argument: hgx_align_reads");
        return HGX_EINVAL;
    }
    if (!kept) {
        *sam_out = nullptr;
        *n_bytes_out = 0;
    }
    g_route = 0; g_decline = 0; g_reads = g_aligned = g_conc = 0;
    g_st_reads = g_st_anchors = g_st_cells = 0;
    g_pr_searched = g_pr_placed = g_pr_changed = 0;
    memset(g_tr, 0, sizeof g_tr);
    try {
        hgx_aln_reads loaded;
        int rc = HGX_OK;
        if (!dr && (rc = load_reads(n_inputs, paths, texts, text_bytes, opts->fastq, loaded))) return rc;
#ifndef HGX_ALIGN_STANDALONE
        const bool resident = dr && dr->route == 2;          // the table lies in HBM, `loaded` is empty so far
        const hgx_aln_reads &reads = dr && !resident ? dr->host : loaded;
        const size_t n_reads = resident ? (size_t)dr->n : reads.n();
#else
        const hgx_aln_reads &reads = loaded;
        const size_t n_reads = reads.n();
#endif
        g_reads = (int64_t)n_reads;
        std::string body;
        int64_t aligned = 0, conc = 0;
        int decline = 0;
        const char *sw = hgx_test_switch("front");
        if (opts->route == 1 || (opts->route == 0 && sw && !strcmp(sw, "host"))) decline = HGX_ALN_DECLINE_SWITCH;
        else if (opts->route == 0 && !(sw && !strcmp(sw, "device")) && n_reads < 1000) decline = HGX_ALN_DECLINE_GATE;
        hgx_aln_ordered ord;
        ord.keep = kept != nullptr;
        if (!decline && n_reads > 0) {
#ifndef HGX_ALIGN_STANDALONE
            if (resident) {
                std::vector<int32_t> h_len;                  // (the states tier sizes its tables on the host: 4 bytes per read)
                if (opts->search && (rc = hgx_reads_len_to_host(dr, h_len))) return rc;
                rc = hgx_align_device_body(ix, dr->dv, (long)dr->n, dr->max_len, opts->search ? h_len.data() : nullptr, opts, gap, rescue, body,
                                           &aligned, &conc, &decline, order ? &ord : nullptr);
                if (rc) return rc;
            } else
#endif
            if ((rc = hgx_align_device(ix, reads, opts, gap, rescue, body, &aligned, &conc, &decline, order ? &ord : nullptr))) return rc;
        }
#ifndef HGX_ALIGN_STANDALONE
        if (decline && resident && (rc = hgx_reads_to_host(dr, loaded))) return rc;      // (offsets into the text as it lies: no re-pack)
#endif
        if (decline) {
            body.clear();
            aligned = conc = 0;
            g_st_reads = g_st_anchors = g_st_cells = 0;          // what the kernels took before they declined is not this call's answer
            g_pr_searched = g_pr_placed = g_pr_changed = 0;
            memset(g_tr, 0, sizeof g_tr);
            int gave_up = 0;
            const auto route = rescue > 0 ? host_route<RescueTier> : opts->clip > 0 ? host_route<SingleTier<ClipTier>>
                               : gap > 0 ? host_route<SingleTier<GapTier>> : host_route<NoTier>;
            const int budgets[2] = {rescue > 0 ? rescue : opts->clip, gap};
            if ((rc = route(ix, reads, opts, budgets, body, &aligned, &conc, &gave_up))) return rc;
            if (gave_up) fprintf(stderr, "[hgx_align_reads] a read's search passed the host route's limits (code %d): left unaligned\n", gave_up);
        }
        if (order && (decline || ord.unordered)) hgx_align_order_body(ix, body);
        g_route = decline ? 0 : 2;
        g_decline = decline;
        g_aligned = aligned;
        g_conc = conc;
        if (kept) {
            if (ord.d_text) *kept = ord;
            else *host_text = ix->header + body;
            return HGX_OK;
        }
        const size_t total = ix->header.size() + body.size();
        char *out = (char *)hgx_host_alloc(total + 1);
        if (!out) { hgx_set_error("hgx_align_reads: out of memory"); return HGX_ENOMEM; }
        memcpy(out, ix->header.data(), ix->header.size());
        memcpy(out + ix->header.size(), body.data(), body.size());
        out[total] = 0;
        *sam_out = out;
        *n_bytes_out = total;
        return HGX_OK;
    } catch (const std::exception &e) {
        hgx_set_error("hgx_align_reads: %s", e.what());
        return HGX_ENOMEM;
    }
}

extern "C" int hgx_align_reads_x(hgx_align_index *ix, int32_t n_inputs, const char *const *paths, const char *const *texts,
                                 const size_t *text_bytes, const hgx_align_opts *opts, const hgx_align_more *more, char **sam_out,
                                 size_t *n_bytes_out) {
    return align_call(ix, n_inputs, paths, texts, text_bytes, opts, more, sam_out, n_bytes_out, nullptr, nullptr);
}

#ifndef HGX_ALIGN_STANDALONE
// the hgx_alignment over what align_call kept
static int adopt_kept(hgx_align_index *ix, hgx_aln_ordered &kept, const std::string &host_text, hgx_alignment **out, void *stream) {
    std::vector<std::string> refs;
    std::vector<int32_t> lens;
    for (int g = 0; g < ix->hv.n_loci; ++g) {
        refs.emplace_back(ix->pool.data() + ix->name_off[g], (size_t)ix->name_len[g]);
        lens.push_back(ix->bb_off[g + 1] - ix->bb_off[g]);
    }
    return hgx_alignment_from_reads(out, kept.d_text, kept.d_text ? kept.n_bytes : host_text.size(), kept.d_text ? nullptr : host_text.data(),
                                    ix->header.size(), refs, lens, stream);
}

extern "C" int hgx_align_reads_dev(hgx_align_index *ix, const hgx_reads *reads, const hgx_align_opts *opts, const hgx_align_more *more,
                                   char **sam_out, size_t *n_bytes_out) {
    if (!reads) { hgx_set_error("invalid argument: hgx_align_reads_dev"); return HGX_EINVAL; }
    return align_call(ix, reads->n_inputs, nullptr, nullptr, nullptr, opts, more, sam_out, n_bytes_out, nullptr, nullptr, reads);
}

extern "C" int hgx_align_reads_dev_resident(hgx_align_index *ix, const hgx_reads *reads, const hgx_align_opts *opts, const hgx_align_more *more,
                                            hgx_alignment **out, void *stream) {
    if (!out || !reads) { hgx_set_error("invalid argument: hgx_align_reads_dev_resident"); return HGX_EINVAL; }
    *out = nullptr;
    hgx_aln_ordered kept;
    std::string host_text;
    const int rc = align_call(ix, reads->n_inputs, nullptr, nullptr, nullptr, opts, more, nullptr, nullptr, &kept, &host_text, reads);
    if (rc) return rc;
    return adopt_kept(ix, kept, host_text, out, stream);
}

extern "C" int hgx_align_reads_resident(hgx_align_index *ix, int32_t n_inputs, const char *const *paths, const char *const *texts,
                                        const size_t *text_bytes, const hgx_align_opts *opts, const hgx_align_more *more,
                                        hgx_alignment **out, void *stream) {
    if (!out) { hgx_set_error("invalid argument: hgx_align_reads_resident"); return HGX_EINVAL; }
    *out = nullptr;
    hgx_aln_ordered kept;
    std::string host_text;
    const int rc = align_call(ix, n_inputs, paths, texts, text_bytes, opts, more, nullptr, nullptr, &kept, &host_text);
    if (rc) return rc;
    return adopt_kept(ix, kept, host_text, out, stream);
}
#endif

extern "C" int hgx_align_last(int32_t *route, int64_t *reads, int64_t *aligned, int64_t *pairs_concordant, int32_t *decline_code) {
    if (route) *route = g_route;
    if (reads) *reads = g_reads;
    if (aligned) *aligned = g_aligned;
    if (pairs_concordant) *pairs_concordant = g_conc;
    if (decline_code) *decline_code = g_decline;
    return HGX_OK;
}

extern "C" int hgx_align_last_states(int64_t *reads, int64_t *anchors, int64_t *cells) {
    if (reads) *reads = g_st_reads;
    if (anchors) *anchors = g_st_anchors;
    if (cells) *cells = g_st_cells;
    return HGX_OK;
}

extern "C" int hgx_align_last_pairs(int64_t *searched, int64_t *placed, int64_t *changed) {
    if (searched) *searched = g_pr_searched;
    if (placed) *placed = g_pr_placed;
    if (changed) *changed = g_pr_changed;
    return HGX_OK;
}

// the last call's counters of `tier` (zeros if it did not run)
static int tier_last(int tier, int64_t *searched, int64_t *found, int64_t *bases) {
    if (searched) *searched = g_tr[tier][0];
    if (found) *found = g_tr[tier][1];
    if (bases) *bases = g_tr[tier][2];
    return HGX_OK;
}
extern "C" int hgx_align_last_clip(int64_t *searched, int64_t *clipped, int64_t *bases) {
    return tier_last(HGX_ALN_TIER_CLIP, searched, clipped, bases);
}
extern "C" int hgx_align_last_gap(int64_t *searched, int64_t *gapped, int64_t *bases) {
    return tier_last(HGX_ALN_TIER_GAP, searched, gapped, bases);
}

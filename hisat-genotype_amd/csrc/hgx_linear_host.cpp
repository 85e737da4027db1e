// hgx_linear_host.cpp -- the host route of linear-index typing (typing_core.py:1597-1649): the reference's loop, line by line.
// It is the route below the record-count gate, the checker of the device route (hgx_linear.hip) and the finisher of every
// decline (unknown in-gene names, a non-integer or missing AS, a line the reference would raise on, a class-key collision).
#include <algorithm>
#include <cstring>
#include <map>
#include <string>

#include "hgx_internal.hpp"
#include "hgx_linear.hpp"

static inline bool lin_space(char c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r' || c == '\v' || c == '\f'; }

// str.split(): the columns of one line
static void split_cols(const char *p, size_t n, std::vector<std::pair<const char *, size_t>> &cols) {
    cols.clear();
    size_t i = 0;
    while (i < n) {
        while (i < n && lin_space(p[i])) ++i;
        if (i >= n) break;
        const size_t b = i;
        while (i < n && !lin_space(p[i])) ++i;
        cols.emplace_back(p + b, i - b);
    }
}

// int(s) for the plain decimal spellings an aligner writes; false = the reference's int() would raise (or take a form this
// statement does not model: underscores between digits)
static bool parse_int(const char *p, size_t n, int64_t &v) {
    size_t i = 0;
    bool neg = false;
    if (i < n && (p[i] == '+' || p[i] == '-')) neg = p[i++] == '-';
    if (i >= n) return false;
    int64_t x = 0;
    for (; i < n; ++i) {
        if (p[i] < '0' || p[i] > '9') return false;
        x = x * 10 + (p[i] - '0');
        if (x > (int64_t)1 << 40) return false;
    }
    v = neg ? -x : x;
    return true;
}

void hgx_linear_lines(const char *sam, size_t n, std::vector<uint64_t> &start, std::vector<uint64_t> &end) {
    start.clear();
    end.clear();
    size_t i = 0;
    while (i < n) {
        const char *nl = (const char *)memchr(sam + i, '\n', n - i);
        const size_t e = nl ? (size_t)(nl - sam) : n;
        if (e > i) { start.push_back(i); end.push_back(e); }
        i = e + 1;
    }
}

std::string hgx_linear_rname(const char *line, size_t len) {
    std::vector<std::pair<const char *, size_t>> cols;
    split_cols(line, len, cols);
    return cols.size() >= 3 ? std::string(cols[2].first, cols[2].second) : std::string();
}

int32_t hgx_linear_name_id(hgx_linear &out, const hgx_linear_locus &ll, const std::string &s) {
    auto it = ll.id.find(s);
    if (it != ll.id.end()) return it->second;
    for (size_t k = 0; k < out.extra.size(); ++k)
        if (out.extra[k] == s) return (int32_t)(ll.name.size() + k);
    out.extra.push_back(s);
    return (int32_t)(ll.name.size() + out.extra.size() - 1);
}

int hgx_linear_host(hgx_linear &out, const hgx_linear_locus &ll, const char *base, const uint64_t *ls, const uint64_t *le, size_t n_lines,
                    const hgx_linear_opts &o) {
    const std::string gene = o.gene ? o.gene : "";
    out.extra.clear();
    out.count_id.clear(); out.count_val.clear();
    out.cls_off.assign(1, 0); out.cls_ids.clear(); out.cls_count.clear();
    out.n_kept = out.n_groups = 0;
    std::unordered_map<std::string, int32_t> extra_id;        // names outside the locus -> id
    auto name_id = [&](const char *p, size_t len) -> int32_t {
        std::string s(p, len);
        auto it = ll.id.find(s);
        if (it != ll.id.end()) return it->second;
        auto jt = extra_id.find(s);
        if (jt != extra_id.end()) return jt->second;
        const int32_t id = (int32_t)(ll.name.size() + out.extra.size());
        out.extra.push_back(s);
        extra_id.emplace(std::move(s), id);
        return id;
    };
    // the sort key of a name id: Python str order of the names (byte order of UTF-8)
    auto name_of = [&](int32_t id) -> const std::string & {
        return id < (int32_t)ll.name.size() ? ll.name[id] : out.extra[id - ll.name.size()];
    };
    std::unordered_map<int32_t, size_t> count_pos;
    std::map<std::vector<int32_t>, size_t> cls_pos;
    int32_t allele = -1;                                   // the loop's free variable `allele` (core:1617)
    auto add_alleles = [&](std::vector<int32_t> &alleles) {
        auto it = count_pos.find(allele);
        if (it == count_pos.end()) {
            count_pos.emplace(allele, out.count_id.size());
            out.count_id.push_back(allele);
            out.count_val.push_back(1);
        } else {
            out.count_val[it->second] += 1;
        }
        std::sort(alleles.begin(), alleles.end(), [&](int32_t a, int32_t b) { return name_of(a) < name_of(b); });
        auto ct = cls_pos.find(alleles);
        if (ct == cls_pos.end()) {
            cls_pos.emplace(alleles, out.cls_count.size());
            out.cls_ids.insert(out.cls_ids.end(), alleles.begin(), alleles.end());
            out.cls_off.push_back((int32_t)out.cls_ids.size());
            out.cls_count.push_back(1);
        } else {
            out.cls_count[ct->second] += 1;
        }
    };
    std::vector<std::pair<const char *, size_t>> cols;
    std::vector<int32_t> alleles;                          // the set `alleles` (distinct ids)
    std::string prev_read_id;
    bool have_prev = false, have_prev_as = false;
    int64_t prev_as = 0;
    for (size_t line_no = 1; line_no <= n_lines; ++line_no) {
        const char *p = base + ls[line_no - 1];
        const size_t len = le[line_no - 1] - ls[line_no - 1];
        split_cols(p, len, cols);
        if (cols.size() < 3) {
            hgx_set_error("ValueError: not enough values to unpack (expected 3, got %d) on line %zu (typing_core.py:1615)", (int)cols.size(), line_no);
            return HGX_EPARSE;
        }
        int64_t flag;
        if (!parse_int(cols[1].first, cols[1].second, flag)) {
            hgx_set_error("ValueError: invalid literal for int() with base 10: '%.*s' (FLAG, line %zu, typing_core.py:1616)",
                          (int)std::min<size_t>(cols[1].second, 64), cols[1].first, line_no);
            return HGX_EPARSE;
        }
        allele = name_id(cols[2].first, cols[2].second);
        if (flag & 0x4) continue;
        if (cols[2].second < gene.size() || memcmp(cols[2].first, gene.data(), gene.size()) != 0) continue;
        if (std::string(cols[2].first, cols[2].second).find("BACKBONE") != std::string::npos) continue;
        const char *as_p = nullptr;
        size_t as_n = 0;
        for (size_t c = 11; c < cols.size(); ++c)
            if (cols[c].second >= 2 && cols[c].first[0] == 'A' && cols[c].first[1] == 'S') { as_p = cols[c].first; as_n = cols[c].second; }
        if (!as_p) {
            hgx_set_error("AssertionError: a kept record without an AS column on line %zu (typing_core.py:1628)", line_no);
            return HGX_EPARSE;
        }
        int64_t as;
        if (!parse_int(as_p + std::min<size_t>(5, as_n), as_n - std::min<size_t>(5, as_n), as)) {
            hgx_set_error("ValueError: invalid literal for int() with base 10: '%.*s' (AS, line %zu, typing_core.py:1627)",
                          (int)std::min<size_t>(as_n > 5 ? as_n - 5 : 0, 64), as_p + std::min<size_t>(5, as_n), line_no);
            return HGX_EPARSE;
        }
        ++out.n_kept;
        const size_t qn = cols[0].second;
        if (!have_prev || prev_read_id.size() != qn || memcmp(prev_read_id.data(), cols[0].first, qn) != 0) {
            if (!alleles.empty()) {
                if (o.aligner == 0 || (o.aligner == 1 && alleles.size() < 10)) add_alleles(alleles);
                alleles.clear();
            }
            have_prev_as = false;
            ++out.n_groups;
        }
        if (have_prev_as && as < prev_as) continue;
        prev_read_id.assign(cols[0].first, qn);
        have_prev = true;
        prev_as = as;
        have_prev_as = true;
        if (std::find(alleles.begin(), alleles.end(), allele) == alleles.end()) alleles.push_back(allele);
    }
    if (!alleles.empty()) add_alleles(alleles);
    return HGX_OK;
}

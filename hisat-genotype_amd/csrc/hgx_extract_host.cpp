// hgx_extract_host.cpp -- the host route of read extraction: the reference's loop (typing_process.py:1630-1745) over a line
// table, statement by statement.  It checks the device route (tests/test_gpu_extract.py), takes every chunk the device declines
// or that is below the gate, and words the reference's errors.
#include <cstring>
#include <utility>

#include "hgx_internal.hpp"
#include "hgx_extract.hpp"

namespace {
// str.split() / str.strip() without arguments on ASCII text
inline bool ext_sp(char c) { return c == ' ' || (c >= '\t' && c <= '\r') || (c >= 0x1c && c <= 0x1f); }

struct Col { const char *p; uint32_t n; };

// int(s) of Python: a sign, digits, single underscores between digits
bool py_int(const char *p, size_t n, int64_t &v) {
    size_t i = 0;
    bool neg = false;
    if (i < n && (p[i] == '+' || p[i] == '-')) neg = p[i++] == '-';
    if (i >= n || p[i] < '0' || p[i] > '9') return false;
    int64_t x = 0;
    bool prev_us = false;
    for (; i < n; ++i) {
        if (p[i] == '_') {
            if (prev_us) return false;
            prev_us = true;
            continue;
        }
        if (p[i] < '0' || p[i] > '9') return false;
        prev_us = false;
        if (x < ((int64_t)1 << 58)) x = x * 10 + (p[i] - '0');
    }
    if (prev_us) return false;
    v = neg ? -x : x;
    return true;
}

int ext_fail(hgx_extract &h, int kind, const char *what, size_t line_no) {
    static const char *const names[] = {"", "ValueError", "AssertionError", "SystemExit", "IndexError", "TypeError"};
    h.error_kind = kind;
    hgx_set_error("extract_reads: %s: %s (record %zu of the stream)", names[kind], what, line_no);
    return HGX_EPARSE;
}

void put_read(std::string &o, const std::string &name, const std::string &seq, const std::string &qual, bool fastq) {
    o.push_back(fastq ? '@' : '>');
    o += name;
    o.push_back('\n');
    o += seq;
    o.push_back('\n');
    if (fastq) {
        o += "+\n";
        o += qual;
        o.push_back('\n');
    }
}
}  // namespace

void hgx_extract_lines(const char *base, size_t n, std::vector<uint32_t> &ls, std::vector<uint32_t> &le) {
    ls.clear();
    le.clear();
    size_t p = 0;
    while (p < n) {
        const char *nl = (const char *)memchr(base + p, '\n', n - p);
        const size_t e = nl ? (size_t)(nl - base) : n;
        if (base[p] != '@' || e == p) {
            ls.push_back((uint32_t)p);
            le.push_back((uint32_t)e);
        }
        p = e + 1;
    }
}

void hgx_extract_name(const char *line, size_t len, const char *&name, uint32_t &n, uint32_t &key_n) {
    size_t p = 0;
    while (p < len && ext_sp(line[p])) ++p;
    const size_t b = p;
    while (p < len && !ext_sp(line[p])) ++p;
    name = line + b;
    n = (uint32_t)(p - b);
    const char *bar = (const char *)memchr(name, '|', n);
    key_n = bar ? (uint32_t)(bar - name) : n;
}

bool hgx_extract_chk(hgx_extract &h, const char *base, const uint32_t *ls, const uint32_t *le, size_t n_lines) {
    std::string prev = h.prev_name;
    for (size_t i = 0; i < n_lines && i < 2; ++i) {
        const char *nm;
        uint32_t n, kn;
        hgx_extract_name(base + ls[i], le[i] - ls[i], nm, n, kn);
        if (n == 0) return false;
        if (!prev.empty()) {
            if (!h.simulation && h.paired && (prev.size() != n || memcmp(prev.data(), nm, n) != 0)) return false;
            return true;
        }
        if (h.simulation && kn == 0) return false;
        prev.assign(nm, n);
    }
    return !prev.empty() && n_lines >= 2;
}

int hgx_extract_host(hgx_extract &h, const char *base, const uint32_t *ls, const uint32_t *le, size_t n_lines) {
    const bool paired = h.paired != 0, sim = h.simulation != 0, fastq = h.fastq != 0;
    uint64_t fams = 0;                                   // extract_read
    std::vector<uint8_t> fam_wide;                       // the same beyond 64 families
    if (h.n_fam > 64) fam_wide.assign(h.n_fam, 0);
    bool have1 = false, have2 = false, r1f = true, r2f = true;
    std::string s1, q1, s2, q2, chr;
    std::vector<Col> cols;
    auto key_len = [&](const std::string &s) { const size_t b = s.find('|'); return b == std::string::npos ? s.size() : b; };
    auto any = [&]() {
        if (fams) return true;
        for (uint8_t b : fam_wide) if (b) return true;
        return false;
    };
    // the flush of process:1661-1676 (and 1747-1760 after the loop); false: read1[0] / read2[0] of an empty list
    auto flush = [&]() -> bool {
        if (!any()) return true;
        for (int f = 0; f < h.n_fam; ++f) {
            if (!(f < 64 ? (fams >> f) & 1 : fam_wide[f])) continue;
            if (!have1) return false;
            put_read(h.out[2 * f], h.prev_name, s1, q1, fastq);
            if (paired) {
                if (!have2) return false;
                put_read(h.out[2 * f + 1], h.prev_name, s2, q2, fastq);
            }
            ++h.written[f];
        }
        return true;
    };
    auto store = [&](const Col &seq, const Col &qual, bool rev, std::string &s, std::string &q) {
        if (!rev) { s.assign(seq.p, seq.n); q.assign(qual.p, qual.n); return; }
        s.resize(seq.n);
        for (uint32_t k = 0; k < seq.n; ++k) {
            const char c = seq.p[seq.n - 1 - k];
            s[k] = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : c;
        }
        q.assign(qual.p, qual.n);
        for (uint32_t a = 0, b = qual.n; a + 1 < b; ++a, --b) std::swap(q[a], q[b - 1]);
    };
    for (size_t i = 0; i < n_lines; ++i) {
        const size_t rec_no = (size_t)h.n_records + 1;
        const char *line = base + ls[i];
        const size_t len = le[i] - ls[i];
        cols.clear();
        for (size_t p = 0; p < len;) {
            while (p < len && ext_sp(line[p])) ++p;
            if (p >= len) break;
            const size_t b = p;
            while (p < len && !ext_sp(line[p])) ++p;
            cols.push_back(Col{line + b, (uint32_t)(p - b)});
        }
        if (cols.size() < 11) return ext_fail(h, HGX_EXT_ERR_VALUE, "not enough values to unpack (fewer than 11 columns)", rec_no);
        int64_t flag, pos, AS = 0, XS = 0, NH = 0;
        bool hasAS = false, hasXS = false, hasNH = false;
        if (!py_int(cols[1].p, cols[1].n, flag)) return ext_fail(h, HGX_EXT_ERR_VALUE, "FLAG is no integer", rec_no);
        if (!py_int(cols[3].p, cols[3].n, pos)) return ext_fail(h, HGX_EXT_ERR_VALUE, "POS is no integer", rec_no);
        pos -= 1;
        for (size_t c = 11; c < cols.size(); ++c) {
            const Col &t = cols[c];
            if (t.n < 2) continue;
            int64_t *dst = nullptr;
            bool *has = nullptr;
            if (t.p[0] == 'A' && t.p[1] == 'S') { dst = &AS; has = &hasAS; }
            else if (t.p[0] == 'X' && t.p[1] == 'S') { dst = &XS; has = &hasXS; }
            else if (t.p[0] == 'N' && t.p[1] == 'H') { dst = &NH; has = &hasNH; }
            if (!dst) continue;
            if (t.n <= 5 || !py_int(t.p + 5, t.n - 5, *dst)) return ext_fail(h, HGX_EXT_ERR_VALUE, "an AS / XS / NH value is no integer", rec_no);
            *has = true;
        }
        ++h.n_records;
        const std::string name(cols[0].p, cols[0].n);
        if (h.chk_line && !h.prev_name.empty()) {
            h.chk_line = false;
            if (name != h.prev_name && !sim && paired) return ext_fail(h, HGX_EXT_ERR_EXIT, "Paired read names are not the same", rec_no);
        }
        const bool differs = sim ? name.compare(0, key_len(name), h.prev_name, 0, key_len(h.prev_name)) != 0 : name != h.prev_name;
        if (differs) {
            if (!flush()) return ext_fail(h, HGX_EXT_ERR_INDEX, "list index out of range (a group with hits lacks a mate)", rec_no);
            h.prev_name = name;
            ++h.n_groups;
            fams = 0;
            if (!fam_wide.empty()) fam_wide.assign(h.n_fam, 0);
            have1 = have2 = false;
            r1f = r2f = true;
        }
        const bool left = (flag & 0x40) || !paired;
        if ((flag & 0x4) == 0) {
            bool hit = h.aligner == 0 && hasNH && NH == 1;
            if (!hit) {
                if (left) {
                    if (h.aligner == 1) {
                        if (hasAS != hasXS) return ext_fail(h, HGX_EXT_ERR_TYPE, "'>' between str and int (AS or XS is missing)", rec_no);
                        hit = hasAS && AS > XS && r1f;
                    }
                } else hit = r2f;
            }
            if (hit) {
                chr.assign(cols[2].p, cols[2].n);
                auto it = h.chrom_id.find(chr);
                if (it != h.chrom_id.end()) {
                    for (uint32_t r = h.creg_off[it->second]; r < h.creg_off[it->second + 1]; ++r) {
                        if (pos >= h.reg_left[r] && pos < h.reg_right[r]) {
                            const int f = h.reg_fam[r];
                            if (f < 64) fams |= 1ull << f; else fam_wide[f] = 1;
                            break;
                        }
                    }
                }
            }
        }
        if (left) {
            r1f = false;
            if (!have1) {                                       // `if not read1`: the first left record of the group stays
                store(cols[9], cols[10], (flag & 0x10) != 0, s1, q1);
                have1 = true;
            }
        } else {
            if (!(flag & 0x80)) return ext_fail(h, HGX_EXT_ERR_ASSERT, "a paired record with neither 0x40 nor 0x80", rec_no);
            r2f = false;
            store(cols[9], cols[10], (flag & 0x10) != 0, s2, q2);
            have2 = true;
        }
    }
    if (!flush()) return ext_fail(h, HGX_EXT_ERR_INDEX, "list index out of range (a group with hits lacks a mate)", (size_t)h.n_records);
    return HGX_OK;
}

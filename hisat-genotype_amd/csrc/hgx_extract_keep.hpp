// hgx_extract_keep.hpp -- the bookkeeping of the extractor's keep mode (hgx_extract_keep / hgx_extract_take_reads):
// the segment lists, where the joined text of a family lies, and the join itself with the copies behind callbacks.  Plain C++:
// hgx_extract.hip gives it HIP copies, tools/reads_host_main.cpp plain memcpy under the sanitizers.
#pragma once
#include <cstddef>
#include <functional>
#include <string>
#include <vector>

#define HGX_KEEP_ALIGN 64                                // input 2 starts at a multiple of this (HGX_RD_ALIGN)
#define HGX_KEEP_MAX_BYTES ((size_t)1 << 31)             // per family and mate: this much or more is refused

// one chunk's text of one (family, mate): in HBM (d != nullptr: a block of its own, n bytes) or on the host (`host`, n = its size)
struct hgx_keep_seg {
    void *d = nullptr;
    size_t n = 0;
    std::string host;
};
typedef std::vector<std::vector<hgx_keep_seg>> hgx_keep_lists;          // [n_fam * 2], each in chunk order

// what host-route chunks have appended to out[] since the last call becomes one host segment per (family, mate), behind the
// segments already there: called in front of every device chunk's segments and in front of a join, it keeps chunk order
static inline void hgx_keep_flush(std::vector<std::string> &out, hgx_keep_lists &segs) {
    for (size_t k = 0; k < out.size() && k < segs.size(); ++k) {
        if (out[k].empty()) continue;
        hgx_keep_seg sg;
        sg.n = out[k].size();
        sg.host.swap(out[k]);
        out[k].clear();
        segs[k].push_back(std::move(sg));
    }
}

// list k emptied; free_dev gets every device block
static inline void hgx_keep_drop(hgx_keep_lists &segs, size_t k, const std::function<void(void *)> &free_dev) {
    for (hgx_keep_seg &sg : segs[k])
        if (sg.d) free_dev(sg.d);
    segs[k].clear();
}

// where the n_inputs (1 or 2) mates of `family` lie in the joined text: mate 1 at 0, mate 2 at the next multiple of
// HGX_KEEP_ALIGN.  false: mate *bad holds *bad_bytes >= max_bytes
struct hgx_keep_plan {
    size_t in_off[2] = {0, 0}, in_bytes[2] = {0, 0}, text_bytes = 0;
};
static inline bool hgx_keep_layout(const hgx_keep_lists &segs, int family, int n_inputs, hgx_keep_plan &p, int *bad, size_t *bad_bytes,
                                   size_t max_bytes = HGX_KEEP_MAX_BYTES) {
    size_t at = 0;
    p = hgx_keep_plan();
    for (int i = 0; i < n_inputs; ++i) {
        size_t n = 0;
        for (const hgx_keep_seg &sg : segs[(size_t)(2 * family + i)]) {
            if (sg.n >= max_bytes || n + sg.n >= max_bytes) { *bad = i; *bad_bytes = n + sg.n; return false; }      // (before the sum can wrap)
            n += sg.n;
        }
        at = (at + HGX_KEEP_ALIGN - 1) / HGX_KEEP_ALIGN * HGX_KEEP_ALIGN;
        p.in_off[i] = at;
        p.in_bytes[i] = n;
        at += n;
    }
    p.text_bytes = at;
    return true;
}

// the join into a buffer of p.text_bytes + 64 bytes, addressed by offsets: every segment copied to its place in chunk order, the
// gap in front of mate 2 and the 64 bytes behind the text zeroed.  The first non-zero return of a callback ends it.
struct hgx_keep_copy {
    std::function<int(size_t at, const void *dev, size_t n)> from_dev;
    std::function<int(size_t at, const char *host, size_t n)> from_host;
    std::function<int(size_t at, size_t n)> zero;
};
static inline int hgx_keep_join(const hgx_keep_lists &segs, int family, int n_inputs, const hgx_keep_plan &p, const hgx_keep_copy &c) {
    int rc;
    if (n_inputs == 2 && p.in_off[1] > p.in_bytes[0] && (rc = c.zero(p.in_bytes[0], p.in_off[1] - p.in_bytes[0]))) return rc;
    if ((rc = c.zero(p.text_bytes, 64))) return rc;
    for (int i = 0; i < n_inputs; ++i) {
        size_t at = p.in_off[i];
        for (const hgx_keep_seg &sg : segs[(size_t)(2 * family + i)]) {
            if (!sg.n) continue;
            if ((rc = sg.d ? c.from_dev(at, sg.d, sg.n) : c.from_host(at, sg.host.data(), sg.n))) return rc;
            at += sg.n;
        }
    }
    return 0;
}

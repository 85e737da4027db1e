// hgx_linear.hpp -- the linear-index typing route (typing_core.py:1597-1649): shared by the host route (hgx_linear_host.cpp)
// and the device route (hgx_linear.hip).
#pragma once
#include <cstdint>
#include <string>
#include <unordered_map>
#include <vector>

#include "hgx.h"
#include "hgx_records.hpp"

// The names of a locus' alleles as the linear branch meets them in RNAME (ids = allele indices), their name order, and the device
// hash of them (made on the first device-route call, freed with the handle).
struct hgx_linear_locus {
    std::vector<std::string> name;
    std::unordered_map<std::string, int32_t> id;
    std::vector<int32_t> rank;                   // position of name[a] among the sorted names (Python str order = byte order)
    // device copies (hgx_linear.hip)
    hgx_name_view d_names;
    int32_t *d_rank = nullptr;
    int dev = -1;
};

// The result: Gene_counts and Gene_cmpt in dict order over name ids (0..A-1 = the locus' alleles, A.. = `extra` names).
struct hgx_linear {
    int32_t route = 0, decline = 0;              // route 2 = device, 0 = host; decline: HGX_LIN_DECLINE_* (host route only)
    std::vector<std::string> extra;
    std::vector<int32_t> count_id;               // Gene_counts in insertion order
    std::vector<int64_t> count_val;
    std::vector<int32_t> cls_off{0}, cls_ids;       // Gene_cmpt in insertion order: class c = cls_ids[cls_off[c] .. cls_off[c+1]) in name order
    std::vector<int64_t> cls_count;
    int64_t n_kept = 0, n_groups = 0;
};

enum {
    HGX_LIN_DECLINE_NONE = 0,
    HGX_LIN_DECLINE_SMALL = 1,        // below the record-count gate
    HGX_LIN_DECLINE_FORCED = 2,       // front=host
    HGX_LIN_DECLINE_UNKNOWN_NAME = 3, // a kept record names an in-gene allele the locus does not have
    HGX_LIN_DECLINE_AS = 4,           // a kept record without an integer AS
    HGX_LIN_DECLINE_RECORD = 5,       // a line the reference would raise on (fewer than 3 columns, a FLAG that is no integer)
    HGX_LIN_DECLINE_COLLISION = 6,    // two different classes on one 64-bit key
};

constexpr int64_t HGX_LIN_MIN_RECORDS = 1000;

// The host route: the reference's loop over the lines [ls[i], le[i]) of `base` (file order), exactly.
int hgx_linear_host(hgx_linear &out, const hgx_linear_locus &ll, const char *base, const uint64_t *ls, const uint64_t *le, size_t n_lines,
                    const hgx_linear_opts &o);
// Line table of `sam`: [start, end) of every non-empty line (the loop's lines; end excludes the newline).
void hgx_linear_lines(const char *sam, size_t n, std::vector<uint64_t> &start, std::vector<uint64_t> &end);
// The RNAME column of one line (for the final trigger); empty if the line has fewer than three columns.
std::string hgx_linear_rname(const char *line, size_t len);
// A name id for `s`: the locus' allele, or an entry of out.extra (appended on first use).
int32_t hgx_linear_name_id(hgx_linear &out, const hgx_linear_locus &ll, const std::string &s);

// hgx_align_linear.hpp -- what the two routes of the "hgx" aligner on a linear index share besides the core: the index object and
// the hand-over between the host unit (hgx_align_linear_host.cpp) and the kernels' unit (hgx_align_linear.hip).
#pragma once
#include <cstdint>
#include <mutex>
#include <string>
#include <vector>

#include "hgx.h"
#include "hgx_align.hpp"               // hgx_aln_reads: the loader's read table
#include "hgx_align_linear_core.hpp"

struct hgx_dev_reads;                  // hgx_reads.hpp: a read table in HBM

struct hgx_align_linear_index {
    std::vector<char> text, pool;
    std::vector<int32_t> off, name_off, name_len, kal, kpos;
    std::vector<uint64_t> lo, hi, mask;
    std::vector<uint32_t> keys, koff;
    std::string header;                   // @HD and the @SQ lines
    hgx_alnl_view hv{};                   // over the vectors above
    std::mutex mu;                        // the device copy is made on first use (hgx_align_linear.hip)
    int dev_ready = -1;                   // device it lives on
    void *d_block = nullptr;
    hgx_alnl_view dv{};
};

// what a route adds up for hgx_align_linear_last
struct hgx_alnl_counts { int64_t aligned = 0, records = 0, candidates = 0; };

// the kernels' route: the records of `reads` appended to `body`.  *decline != 0: nothing was appended (what earlier chunks appended
// is taken back) and the host route finishes the call.  hgx_alnl_device uploads the loader's table first; hgx_alnl_device_body runs
// over a table that lies in HBM (n reads, the longest max_len).
int hgx_alnl_device(hgx_align_linear_index *ix, const hgx_aln_reads &reads, int max_edits, int k, std::string &body, hgx_alnl_counts *counts,
                    int *decline);
int hgx_alnl_device_body(hgx_align_linear_index *ix, const hgx_dev_reads &rd, long n, int max_len, int max_edits, int k, std::string &body,
                         hgx_alnl_counts *counts, int *decline);
void hgx_alnl_device_free(hgx_align_linear_index *ix);

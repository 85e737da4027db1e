// hgx_extract.hpp -- read extraction from a genome-wide alignment stream (typing_process.py:1630-1745): shared by the host route
// (hgx_extract_host.cpp) and the device route (hgx_extract.hip).
#pragma once
#include <cstdint>
#include <string>
#include <unordered_map>
#include <vector>

#include "hgx.h"
#include "hgx_records.hpp"
#include "hgx_extract_keep.hpp"

enum {
    HGX_EXT_DECLINE_NONE = 0,
    HGX_EXT_DECLINE_SMALL = 1,      // the chunk is below the record-count gate
    HGX_EXT_DECLINE_FORCED = 2,     // front=host
    HGX_EXT_DECLINE_RECORD = 3,     // fewer than 11 columns, a byte the device does not split on as str.split() might (>= 0x80)
    HGX_EXT_DECLINE_VALUE = 4,      // FLAG, POS or an AS / XS / NH value that is no plain integer of 32 bits
    HGX_EXT_DECLINE_MATE = 5,       // a paired record with neither 0x40 nor 0x80 (the reference asserts)
    HGX_EXT_DECLINE_TYPE = 6,       // bowtie2, a left record, and only one of AS / XS (the reference raises TypeError)
    HGX_EXT_DECLINE_INDEX = 7,      // a group with hits but no read 1 / read 2 (IndexError)
    HGX_EXT_DECLINE_FAMILIES = 8,   // more than 64 families
    HGX_EXT_DECLINE_NAMES = 9,      // the stream's first two records (chk_line), or an empty name before '|' in simulation mode
    HGX_EXT_DECLINE_SIZE = 10,      // a chunk's output beyond 32-bit offsets
    HGX_EXT_DECLINE_INFLATE = 11,   // BAM: the device inflate gave a block a bad verdict (the host inflates the chunk and decides)
    HGX_EXT_DECLINE_CHAIN = 12,     // BAM: the ranges of the record walk did not link up, or a block_size below 32
};

// hgx_extract_stats' error_kind: the exception the reference raises at that point
enum { HGX_EXT_ERR_NONE = 0, HGX_EXT_ERR_VALUE = 1, HGX_EXT_ERR_ASSERT = 2, HGX_EXT_ERR_EXIT = 3, HGX_EXT_ERR_INDEX = 4, HGX_EXT_ERR_TYPE = 5 };

// The device route takes a chunk from this many records on: below it the launches and the round trips of the chunk cost more
// than the host loop (DESIGN.md 5.10 has the measurement).
constexpr int64_t HGX_EXT_MIN_RECORDS = 2000;

struct hgx_extract {
    int aligner = 0, paired = 1, simulation = 0, fastq = 1;      // aligner: 0 hisat2, 1 bowtie2, 2 any other name
    int n_fam = 0;
    // the region table by chromosome, .locus order kept inside a chromosome (region_loci[chr], process:1364-1380)
    std::vector<std::string> chrom;
    std::unordered_map<std::string, int32_t> chrom_id;
    std::vector<uint32_t> creg_off;                              // [n_chrom + 1]
    std::vector<int32_t> reg_fam;
    std::vector<int64_t> reg_left, reg_right;
    // the stream
    std::vector<char> buf;                                       // the carried tail, then the bytes fed
    std::string prev_name;                                       // prev_read_name
    bool chk_line = true, finished = false;
    int error_kind = 0;
    int64_t n_records = 0, n_groups = 0, chunks_dev = 0, chunks_host = 0;
    long long up_bytes = 0;
    int last_decline = 0;
    std::vector<int64_t> written;                                // pairs (reads) written per family
    std::vector<std::string> out, taken;                         // [n_fam * 2]: text not yet taken / the block handed out last
    // keep mode (hgx_extract_keep): the text is not collected in `out` but stays, per family and mate, as a list of
    // segments in chunk order -- a device-route chunk's part in a pool block of its own, a host-route chunk's as its string --
    // until hgx_extract_take_reads joins them in HBM
    bool keep = false;
    hgx_keep_lists segs;                                         // [n_fam * 2] (hgx_extract_keep.hpp)
    // a BAM stream (hgx_extract_feed_bam): deflated bytes in, the records read in their binary form
    int mode = 0;                                                // 0 = nothing fed yet, 1 = text, 2 = BAM
    std::vector<unsigned char> comp;                             // BGZF bytes not yet digested (at most one partial block stays)
    size_t comp_pos = 0;                                         // file offset of comp[0]
    bool have_hdr = false;
    std::vector<unsigned char> head;                             // the leading block(s), inflated on the host until the header parses
    std::vector<std::string> refs;                               // the header's reference names
    std::vector<int32_t> reftab;                                 // [n_ref] chromosome index in `chrom`, -1 = none, -2 = a name text would split
    // the carry: the inflated bytes from the first record of the last, possibly unfinished, group on.  After a device chunk it
    // is a pool allocation of its own (copied out of the chunk's stream buffer), after a host chunk a vector; stream_pos = its
    // offset in the inflated file
    std::vector<unsigned char> hcarry;
    void *d_carry = nullptr;
    size_t carry_n = 0, stream_pos = 0;
    bool carry_dev = false;
    int32_t *d_reftab = nullptr;
    // device copies of the region table (hgx_extract.hip)
    hgx_name_view d_chrom;
    uint32_t *d_creg = nullptr;
    int32_t *d_rfam = nullptr;
    long long *d_rl = nullptr, *d_rr = nullptr;
    int dev = -1;
};

// Line table of the records in [base, base + n): [start, end) of every line that does not start with '@' (end excludes the
// newline; blank lines stay: the reference raises on them).
void hgx_extract_lines(const char *base, size_t n, std::vector<uint32_t> &ls, std::vector<uint32_t> &le);
// The read name of a line (first column of line.strip().split(); empty when there is none) and its length before '|'.
void hgx_extract_name(const char *line, size_t len, const char *&name, uint32_t &n, uint32_t &key_n);
// The host route: the reference's loop over the lines, exactly; appends to h.out, keeps h.prev_name / h.chk_line, flushes the
// last group at the end (the caller cuts chunks on group boundaries).  HGX_EPARSE with h.error_kind set where the reference raises.
int hgx_extract_host(hgx_extract &h, const char *base, const uint32_t *ls, const uint32_t *le, size_t n_lines);
// What the loop's chk_line test (process:1651-1659) does with the first records of a chunk while h.chk_line is set: false when the
// host route has to take the chunk (it exits there, or a line has no name).
bool hgx_extract_chk(hgx_extract &h, const char *base, const uint32_t *ls, const uint32_t *le, size_t n_lines);

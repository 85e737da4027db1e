// hgx_reads.hpp -- the read table of the "hgx" aligner made where the FASTA / FASTQ text lies: the hgx_reads
// object, what the device unit (hgx_reads.hip) and the host unit (hgx_reads_host.cpp) hand each other, and the decline codes.
// Plain C++: the host unit is also compiled on its own (tools/reads_host_main.cpp) for the sanitizers.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "hgx_align.hpp"

// why the kernels did not make the table (hgx_reads_last); the host loader made it then.  Where a text breaks several rules the
// SMALLEST code is reported (tests/reads_table_ref.py device_takes).  SWITCH, SIZE and GATE are settled before any kernel runs.
#define HGX_RD_DECLINE_NONE 0
#define HGX_RD_DECLINE_GATE 1            // text below the gate
#define HGX_RD_DECLINE_SWITCH 2          // front=host
#define HGX_RD_DECLINE_EMPTY_LINE 3      // an empty line anywhere (a lone '\r' is one)
#define HGX_RD_DECLINE_MARKER 4          // a record's first line without '@' / '>'; a FASTA sequence line that starts with '>'
#define HGX_RD_DECLINE_TRUNCATED 5       // lines no multiple of 4 / 2
#define HGX_RD_DECLINE_QUAL_LEN 6
#define HGX_RD_DECLINE_LOWER 7           // a base in a-z
#define HGX_RD_DECLINE_COUNT 8           // two inputs, different record counts
#define HGX_RD_DECLINE_READ_LEN 9        // longer than HGX_ALN_MAX_READ
#define HGX_RD_DECLINE_SIZE 10           // the padded text reaches HGX_RD_MAX_BYTES: line starts are 32 bits wide

#define HGX_RD_TILE 4096                 // bytes per tile of the newline pass (align.READS_TILE)
#define HGX_RD_GATE (512 << 10)          // bytes of text from which the kernels make the table: the measured break-even (between 226 KB
                                         // and 452 KB on MI355X) rounded up to a power of two (align.READS_GATE)
#define HGX_RD_MAX_BYTES (((size_t)1 << 32) - 64)      // of text with its padding (input 2 at a multiple of HGX_RD_ALIGN)
#define HGX_RD_ALIGN 64                  // input 2 starts at a multiple of this in the allocation: its 16-byte loads stay aligned

// what the aligner's kernels read a chunk of reads through: offsets into `text`, mates interleaved (2k, 2k + 1) when paired
struct hgx_dev_reads {
    const char *text;
    const int64_t *name_off, *seq_off, *qual_off;
    const int32_t *name_len, *len;
    int paired;
};

struct hgx_reads;
void hgx_reads_dev_free(hgx_reads *r);   // (hgx_reads.hip; a stub in the stand-alone host build) the pool blocks given back, idempotent

struct hgx_reads {
    hgx_reads() = default;
    hgx_reads(const hgx_reads &) = delete;
    hgx_reads &operator=(const hgx_reads &) = delete;
    ~hgx_reads() { hgx_reads_dev_free(this); }      // (an object dropped on an error path gives its blocks back too)
    int n_inputs = 1;
    int route = 0, decline = 0;           // 2: the table was made by the kernels and lies in HBM; 0: by the host loader, in `host`
    int64_t n = 0;                        // reads, both inputs
    int max_len = 0;
    size_t in_off[2] = {0, 0}, in_bytes[2] = {0, 0};      // where each input's text lies in d_text / in `src`
    size_t text_bytes = 0;                // of the allocation's used part (input 2's end)
    // route 2: pool blocks (the text is followed by 64 zeroed bytes)
    void *d_text = nullptr, *d_tab = nullptr;
    hgx_dev_reads dv{};
    // route 0: the loader's table; `src` = the inflated inputs it was made from (Reads.save)
    hgx_aln_reads host;
    std::vector<std::string> src;
};

// ---- hgx_align_host.cpp: the loader in its two halves -------------------------------------------------------------------------------
// input `i` inflated (a path through zlib's gzread, a text through inflate where it starts with the gzip magic)
int hgx_aln_inflate_input(const char *path, const char *text, size_t n, std::string &out);
// parse_reads + the interleave of load_reads over inflated texts
int hgx_aln_reads_of_texts(int n_inputs, const std::string *text, int fastq, hgx_aln_reads &out);

// ---- hgx_align.hip: hgx_align_device without its upload half, over a table that lies in HBM (n reads, the longest max_len).  h_len:
// the reads' lengths on the host, read by the states tier alone (nullptr with opts->search == 0)
int hgx_align_device_body(hgx_align_index *ix, const hgx_dev_reads &rd, long n, int max_len, const int32_t *h_len, const hgx_align_opts *opts,
                          int gap, int rescue_clip, std::string &body, int64_t *aligned, int64_t *concordant, int *decline,
                          hgx_aln_ordered *ord = nullptr);

// ---- hgx_reads_host.cpp ------------------------------------------------------------------------------------------------------------
// the size from which a padded text declines with SIZE: HGX_RD_MAX_BYTES, or what the test switch reads_max_bytes=N says
size_t hgx_reads_max_bytes();
// the loader's table over the inflated texts, which the object keeps from here (a table the kernels declined with code `decline`)
int hgx_reads_host_table(hgx_reads *r, std::vector<std::string> &text, int fastq, int decline);
// what hgx_reads_last reports for the calling thread from here on
void hgx_reads_set_last(const hgx_reads *r);

// ---- hgx_reads.hip (the stand-alone host build has stubs that decline) --------------------------------------------------------------
// the texts uploaded side by side and the table made by the kernels: r->route = 2, or r->decline != 0 and nothing is left in HBM
int hgx_reads_make_dev(hgx_reads *r, const std::string *text, int n_inputs, int fastq, void *stream);
// the same over a text that already lies in HBM (d_text: a pool block of r->text_bytes + 64 bytes with r->in_off / r->in_bytes
// set; the object owns it from here).  On a decline the text stays: the caller copies it down for the loader.
int hgx_reads_table_dev(hgx_reads *r, int fastq, void *stream);
// text and table of a route-2 object copied down as an hgx_aln_reads whose offsets point into the text as it lies
int hgx_reads_to_host(const hgx_reads *r, hgx_aln_reads &out);
// the reads' lengths alone (what the aligner's states tier needs on the host)
int hgx_reads_len_to_host(const hgx_reads *r, std::vector<int32_t> &len);
// the bytes [off, off + n) of a route-2 object's text
int hgx_reads_text_to_host(const hgx_reads *r, size_t off, size_t n, char *out);
void hgx_reads_dev_free(hgx_reads *r);

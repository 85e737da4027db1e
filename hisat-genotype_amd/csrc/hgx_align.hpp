// hgx_align.hpp -- what the two routes of the "hgx" aligner share besides the core: the index and the read table.
#pragma once
#include <cstdint>
#include <mutex>
#include <string>
#include <vector>

#include "hgx.h"
#include "hgx_align_core.hpp"
#include "hgx_align_states.hpp"

#define HGX_ALN_HOST_VARS (3 * HGX_ALN_MAX_READ + 8)     // no alignment of a read the core takes has more variants
#define HGX_ALN_HOST_STEPS (1L << 24)                   // read bases walked per side of one anchor, with the memo: a read beyond it is left unaligned

struct hgx_align_index {
    std::vector<char> bb, pool;
    std::vector<int32_t> bb_off, hpos, vpos, vlen, vdata, vid_off, vid_len, name_off, name_len;
    std::vector<uint32_t> hkey;
    std::vector<uint8_t> vtype;
    std::vector<int32_t> sgl_off, sgl, dls_off, dls, dle_off, dle, ins_off, ins;
    std::string header;                   // the @SQ lines
    hgx_aln_view hv{};                    // over the vectors above
    std::mutex mu;                        // the device copy is made on first use (hgx_align.hip)
    int dev_ready = -1;                   // device it lives on
    void *d_block = nullptr;
    hgx_aln_view dv{};
};

// the reads of one call, mates interleaved (2k, 2k + 1) when paired; `text` holds names, upper-case bases and qualities
struct hgx_aln_reads {
    std::vector<char> text;
    std::vector<int64_t> name_off, seq_off, qual_off;      // qual_off < 0: no qualities (FASTA)
    std::vector<int32_t> name_len, len;
    int paired = 0;
    size_t n() const { return len.size(); }
};

// the kernels' route: the records of `reads` appended to `body`, per-read flags (1 aligned, 2 concordant).  *decline != 0: nothing
// was appended and the host route finishes the call.
// `gap`: hgx_align_more.gap (0: no gap tier).  `rescue_clip`: hgx_align_more.rescue_clip (> 0, with gap > 0: both tiers, the clip
// tier with this budget).
// `ord` (nullptr: hgx_align_more.order = 0, nothing below runs): coordinate order.  The chunks' text stays in HBM and is sorted
// there; with ord->keep the ordered text -- the index's header in front of it, 64 zeroed bytes behind it -- is left in a pool block
// (ord->d_text, ord->n_bytes without the 64; the caller owns it) and `body` stays as it was, else the ordered body is appended to
// `body`.  A body of 4 GB or more cannot be ordered there: it is appended in input order and ord->unordered is set.
struct hgx_aln_ordered {
    bool keep = false;
    void *d_text = nullptr;
    size_t n_bytes = 0;
    bool unordered = false;
};
int hgx_align_device(hgx_align_index *ix, const hgx_aln_reads &reads, const hgx_align_opts *opts, int gap, int rescue_clip,
                     std::string &body, int64_t *aligned, int64_t *concordant, int *decline, hgx_aln_ordered *ord = nullptr);
void hgx_align_device_free(hgx_align_index *ix);
// coordinate order on the host: `body`'s lines stable-sorted by (index of RNAME among the index's loci, POS - 1)
void hgx_align_order_body(const hgx_align_index *ix, std::string &body);

// what the states form took in the calling thread's current call (hgx_align_last_states): added to by either route
void hgx_align_states_count(int64_t reads, int64_t anchors, int64_t cells);
// what the pair pick did in the calling thread's current call (hgx_align_last_pairs): added to by the route that gives the bytes
void hgx_align_pairs_count(int64_t searched, int64_t placed, int64_t changed);
// what a fallback tier did in the calling thread's current call (one triple per tier: a rescue call runs both): added to by the
// route that gives the bytes; hgx_align_last_clip / hgx_align_last_gap report their tier's, zeros where it did not run
enum { HGX_ALN_TIER_NONE = 0, HGX_ALN_TIER_CLIP = 1, HGX_ALN_TIER_GAP = 2, HGX_ALN_N_TIERS = 3 };
void hgx_align_tier_count(int tier, int64_t searched, int64_t found, int64_t bases);

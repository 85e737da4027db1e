// hgx_align_linear_host.cpp -- the "hgx" aligner on a linear index: its C-ABI, the index build and the HOST route.
// The host route runs the same core as the kernels (hgx_align_linear_core.hpp) in plain loops: it is their checker, the route of
// every call they decline and the route of route = auto below the gate.  Read files are loaded by the graph
// aligner's loader (hgx_align_host.cpp).  Plain C++: with -DHGX_ALIGN_STANDALONE this unit and hgx_align_host.cpp build into a
// stand-alone program (tools/align_linear_host_main.cpp) for the sanitizers.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <stdexcept>

#include "hgx_align_linear.hpp"
#include "hgx_reads.hpp"                 // the loader's two halves; hgx_reads: a read table made beforehand

extern "C" void hgx_set_error(const char *fmt, ...);
extern "C" const char *hgx_test_switch(const char *name);
void *hgx_host_alloc(size_t bytes);

namespace {
thread_local int g_route = 0, g_decline = 0;
thread_local int64_t g_reads = 0, g_aligned = 0, g_records = 0, g_candidates = 0;

typedef hgx_alnl_planes<HGX_ALNL_HOST_WORDS> HostPlanes;

// the hits of one read, ordered: keys with the read field 0
void hits_of(const hgx_alnl_view &V, const char *seq, int L, int max_edits, std::vector<uint64_t> &hits, int64_t *candidates) {
    hits.clear();
    const int ns = hgx_alnl_n_seeds(L, max_edits);
    for (int strand = 0; strand < 2 && ns > 0; ++strand) {
        const hgx_aln_read R{seq, L, strand};
        HostPlanes rp;
        hgx_alnl_pack(R, rp);
        for (int j = 0; j < ns; ++j) {
            uint32_t code, b0, b1;
            if (!hgx_alnl_code(rp.lo, rp.hi, rp.mask, (long)j * HGX_ALNL_K, &code)) continue;
            hgx_alnl_bucket(V, code, &b0, &b1);
            *candidates += b1 - b0;
            for (uint32_t e = b0; e < b1; ++e) {
                int32_t pos0;
                int nm;
                if (hgx_alnl_candidate(V, rp, L, j, V.kal[e], V.kpos[e], max_edits, &pos0, &nm))
                    hits.push_back(hgx_alnl_key(0, nm, V.kal[e], pos0, strand));
            }
        }
    }
    std::sort(hits.begin(), hits.end());
}

int host_route(const hgx_align_linear_index *ix, const hgx_aln_reads &reads, int max_edits, int k, std::string &body, hgx_alnl_counts *counts) {
    const hgx_alnl_view &V = ix->hv;
    const int step = reads.paired ? 2 : 1;
    std::vector<uint64_t> hits[2];
    for (size_t first = 0; first + step <= reads.n(); first += step) {
        for (int m = 0; m < step; ++m)
            hits_of(V, reads.text.data() + reads.seq_off[first + m], reads.len[first + m], max_edits, hits[m], &counts->candidates);
        for (int m = 0; m < step; ++m) {
            const size_t i = first + m;
            const int n_hits = (int)hits[m].size();
            const int n_written = std::min(n_hits, k);
            if (!n_written) continue;
            counts->aligned += 1;
            counts->records += n_written;
            const char *name = reads.text.data() + reads.name_off[i], *seq = reads.text.data() + reads.seq_off[i];
            const char *qual = reads.qual_off[i] < 0 ? nullptr : reads.text.data() + reads.qual_off[i];
            const bool mate_wrote = step == 2 && !hits[1 - m].empty();
            const size_t at = body.size();
            hgx_aln_out out{nullptr, 0};                                  // the sizing pass of the line writer, then the writing pass
            for (int pass = 0; pass < 2; ++pass) {
                for (int r = 0; r < n_written; ++r)
                    hgx_alnl_line(V, name, reads.name_len[i], seq, qual, reads.len[i], hits[m][r], r, n_written, n_hits, step == 2 ? m : -1,
                                  mate_wrote, out);
                if (pass == 0) {
                    body.resize(at + (size_t)out.n);
                    out = hgx_aln_out{&body[at], 0};
                }
            }
        }
    }
    return HGX_OK;
}
}      // namespace

#ifdef HGX_ALIGN_STANDALONE
// the stand-alone build has no kernels: the device route declines
int hgx_alnl_device(hgx_align_linear_index *, const hgx_aln_reads &, int, int, std::string &, hgx_alnl_counts *, int *decline) {
    *decline = HGX_ALNL_DECLINE_SWITCH;
    return HGX_OK;
}
void hgx_alnl_device_free(hgx_align_linear_index *) {}
#endif

// typing_common.py:610-641 (the linear index the reference builds from the allele sequences with hisat2-build / bowtie2-build)
extern "C" int hgx_align_linear_index_create(hgx_align_linear_index **out, int32_t n_seqs, const char *const *names, const char *const *seqs) {
    if (!out || n_seqs < 1 || !names || !seqs) {
        hgx_set_error("invalid argument: hgx_align_linear_index_create");
        return HGX_EINVAL;
    }
    if (n_seqs >= (1 << HGX_ALNL_ALLELE_BITS)) {
        hgx_set_error("hgx_align_linear_index_create: %d sequences (up to 2^20 - 1)", (int)n_seqs);
        return HGX_EINVAL;
    }
    *out = nullptr;
    try {
        std::unique_ptr<hgx_align_linear_index> ix(new hgx_align_linear_index);
        ix->header = "@HD\tVN:1.0\tSO:unsorted\n";
        ix->off.push_back(0);
        for (int a = 0; a < n_seqs; ++a) {
            if (!names[a] || !seqs[a]) { hgx_set_error("invalid argument: hgx_align_linear_index_create (sequence %d)", a); return HGX_EINVAL; }
            const size_t n = strlen(seqs[a]);
            if (n >= ((size_t)1 << HGX_ALNL_POS_BITS) || ix->text.size() + n >= ((size_t)1 << 31) - 64 * HGX_ALNL_PLANE_PAD) {
                hgx_set_error("hgx_align_linear_index_create: sequence %d has %zu bases (up to 2^20 - 1 each, 2^31 in all)", a, n);
                return HGX_EINVAL;
            }
            for (size_t k = 0; k < n; ++k) ix->text.push_back((char)toupper((unsigned char)seqs[a][k]));
            ix->off.push_back((int32_t)ix->text.size());
            ix->name_off.push_back((int32_t)ix->pool.size());
            ix->name_len.push_back((int32_t)strlen(names[a]));
            ix->pool.insert(ix->pool.end(), names[a], names[a] + strlen(names[a]));
            ix->header += "@SQ\tSN:" + std::string(names[a]) + "\tLN:" + std::to_string(n) + "\n";
        }
        const size_t total = ix->text.size(), n_words = (total + 63) / 64 + HGX_ALNL_PLANE_PAD;
        ix->lo.assign(n_words, 0); ix->hi.assign(n_words, 0); ix->mask.assign(n_words, 0);
        for (size_t i = 0; i < total; ++i) {
            const int c = hgx_aln_code2(ix->text[i]);
            const uint64_t bit = 1ull << (i & 63);
            if (c < 0) ix->mask[i >> 6] |= bit;
            else {
                if (c & 1) ix->lo[i >> 6] |= bit;
                if (c & 2) ix->hi[i >> 6] |= bit;
            }
        }
        // the seed table: every 16-mer of every allele (windows with a base outside ACGT are not indexed), sorted by (code, place)
        std::vector<uint64_t> kmers;
        for (int a = 0; a < n_seqs; ++a)
            for (long P = ix->off[a]; P + HGX_ALNL_K <= ix->off[a + 1]; ++P) {
                uint32_t code;
                if (hgx_alnl_code(ix->lo.data(), ix->hi.data(), ix->mask.data(), P, &code)) kmers.push_back(((uint64_t)code << 32) | (uint64_t)P);
            }
        std::sort(kmers.begin(), kmers.end());
        ix->kal.resize(kmers.size()); ix->kpos.resize(kmers.size());
        for (size_t e = 0; e < kmers.size(); ++e) {
            const uint32_t code = (uint32_t)(kmers[e] >> 32);
            const int32_t P = (int32_t)(uint32_t)kmers[e];
            if (ix->keys.empty() || ix->keys.back() != code) { ix->keys.push_back(code); ix->koff.push_back((uint32_t)e); }
            const int32_t a = (int32_t)(std::upper_bound(ix->off.begin(), ix->off.end(), P) - ix->off.begin()) - 1;
            ix->kal[e] = a;
            ix->kpos[e] = P - ix->off[a];
        }
        ix->koff.push_back((uint32_t)kmers.size());
        hgx_alnl_view &V = ix->hv;
        V.text = ix->text.data(); V.off = ix->off.data(); V.n_alleles = n_seqs;
        V.lo = ix->lo.data(); V.hi = ix->hi.data(); V.mask = ix->mask.data();
        V.keys = ix->keys.data(); V.n_keys = (int32_t)ix->keys.size(); V.koff = ix->koff.data();
        V.kal = ix->kal.data(); V.kpos = ix->kpos.data();
        V.name_off = ix->name_off.data(); V.name_len = ix->name_len.data(); V.pool = ix->pool.data();
        *out = ix.release();
        return HGX_OK;
    } catch (const std::exception &e) {
        hgx_set_error("hgx_align_linear_index_create: %s", e.what());
        return HGX_ENOMEM;
    }
}

extern "C" int hgx_align_linear_index_free(hgx_align_linear_index *ix) {
    if (ix) {
        hgx_alnl_device_free(ix);
        delete ix;
    }
    return HGX_OK;
}

// hgx_align_linear_reads (dr == nullptr: the inputs are loaded) and hgx_align_linear_reads_dev (dr: a table made beforehand -- in HBM,
// dr->route == 2: the kernels run over it as it lies and, where they decline, text and table are copied down; or the loader's)
static int linear_call(hgx_align_linear_index *ix, int32_t n_inputs, const char *const *paths, const char *const *texts, const size_t *text_bytes,
                       const hgx_align_linear_opts *o, char **sam_out, size_t *n_bytes_out, const hgx_reads *dr) {
    if (!ix || !o || !sam_out || !n_bytes_out || o->bytes < (int32_t)sizeof(hgx_align_linear_opts) ||
        (!dr && ((n_inputs != 1 && n_inputs != 2) || (!paths && !(texts && text_bytes))))) {
        hgx_set_error("invalid argument: hgx_align_linear_reads");
        return HGX_EINVAL;
    }
    if (o->max_edits < 0 || o->max_edits > HGX_ALNL_MAX_EDITS) { hgx_set_error("invalid argument: hgx_align_linear_reads (max_edits is 0 .. 4)"); return HGX_EINVAL; }
    if (o->k < 1 || o->k > HGX_ALNL_MAX_K) { hgx_set_error("invalid argument: hgx_align_linear_reads (k is 1 .. 1024)"); return HGX_EINVAL; }
    if (o->route < 0 || o->route > 2) { hgx_set_error("invalid argument: hgx_align_linear_reads (route)"); return HGX_EINVAL; }
    *sam_out = nullptr;
    *n_bytes_out = 0;
    g_route = g_decline = 0;
    g_reads = g_aligned = g_records = g_candidates = 0;
    try {
        hgx_aln_reads loaded;
        int rc = HGX_OK;
        if (!dr) {
            std::vector<std::string> text(n_inputs);
            for (int i = 0; i < n_inputs; ++i)
                if ((rc = hgx_aln_inflate_input(paths ? paths[i] : nullptr, paths ? nullptr : texts[i], paths ? 0 : text_bytes[i], text[i]))) return rc;
            if ((rc = hgx_aln_reads_of_texts(n_inputs, text.data(), o->fastq, loaded))) return rc;
        }
#ifndef HGX_ALIGN_STANDALONE
        const bool resident = dr && dr->route == 2;              // the table lies in HBM, `loaded` is empty so far
        const hgx_aln_reads &reads = dr && !resident ? dr->host : loaded;
        const size_t n_reads = resident ? (size_t)dr->n : reads.n();
#else
        const hgx_aln_reads &reads = loaded;
        const size_t n_reads = reads.n();
#endif
        g_reads = (int64_t)n_reads;
        int decline = 0;
        const char *sw = hgx_test_switch("front");
        if (o->route == 1 || (o->route == 0 && sw && !strcmp(sw, "host"))) decline = HGX_ALNL_DECLINE_SWITCH;
        else if (o->route == 0 && !(sw && !strcmp(sw, "device")) && (int64_t)n_reads * ix->hv.n_alleles < HGX_ALNL_GATE) decline = HGX_ALNL_DECLINE_GATE;
        std::string body;
        hgx_alnl_counts counts;
        if (!decline && n_reads > 0) {
#ifndef HGX_ALIGN_STANDALONE
            if (resident) rc = hgx_alnl_device_body(ix, dr->dv, (long)dr->n, dr->max_len, o->max_edits, o->k, body, &counts, &decline);
            else
#endif
                rc = hgx_alnl_device(ix, reads, o->max_edits, o->k, body, &counts, &decline);
            if (rc) return rc;
        }
#ifndef HGX_ALIGN_STANDALONE
        if (decline && resident && (rc = hgx_reads_to_host(dr, loaded))) return rc;
#endif
        if (decline) {                                           // (the kernels' route has taken back what its chunks appended and counted)
            if ((rc = host_route(ix, reads, o->max_edits, o->k, body, &counts))) return rc;
        }
        g_route = decline ? 0 : 2;
        g_decline = decline;
        g_aligned = counts.aligned; g_records = counts.records; g_candidates = counts.candidates;
        const size_t total = ix->header.size() + body.size();
        char *out = (char *)hgx_host_alloc(total + 1);
        if (!out) { hgx_set_error("hgx_align_linear_reads: out of memory"); return HGX_ENOMEM; }
        memcpy(out, ix->header.data(), ix->header.size());
        memcpy(out + ix->header.size(), body.data(), body.size());
        out[total] = 0;
        *sam_out = out;
        *n_bytes_out = total;
        return HGX_OK;
    } catch (const std::exception &e) {
        hgx_set_error("hgx_align_linear_reads: %s", e.what());
        return HGX_ENOMEM;
    }
}

// typing_common.py:985-1056 (align_reads: `hisat2 -k 10` / `bowtie2 -k 10` on the linear index)
extern "C" int hgx_align_linear_reads(hgx_align_linear_index *ix, int32_t n_inputs, const char *const *paths, const char *const *texts,
                                      const size_t *text_bytes, const hgx_align_linear_opts *opts, char **sam_out, size_t *n_bytes_out) {
    return linear_call(ix, n_inputs, paths, texts, text_bytes, opts, sam_out, n_bytes_out, nullptr);
}

#ifndef HGX_ALIGN_STANDALONE
extern "C" int hgx_align_linear_reads_dev(hgx_align_linear_index *ix, const hgx_reads *reads, const hgx_align_linear_opts *opts, char **sam_out,
                                          size_t *n_bytes_out) {
    if (!reads) { hgx_set_error("invalid argument: hgx_align_linear_reads_dev"); return HGX_EINVAL; }
    return linear_call(ix, reads->n_inputs, nullptr, nullptr, nullptr, opts, sam_out, n_bytes_out, reads);
}
#endif

extern "C" int hgx_align_linear_last(int32_t *route, int64_t *reads, int64_t *aligned, int64_t *records, int64_t *candidates,
                                     int32_t *decline_code) {
    if (route) *route = g_route;
    if (reads) *reads = g_reads;
    if (aligned) *aligned = g_aligned;
    if (records) *records = g_records;
    if (candidates) *candidates = g_candidates;
    if (decline_code) *decline_code = g_decline;
    return HGX_OK;
}

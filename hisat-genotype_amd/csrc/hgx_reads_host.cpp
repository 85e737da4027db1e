// hgx_reads_host.cpp -- the hgx_reads object's C-ABI and its HOST half: inputs inflated as hgx_align_reads does
// (zlib: a gzip member is one serial deflate stream), the switch, size and gate rules, and -- where the kernels of hgx_reads.hip
// decline -- the table made by the aligner's loader from the same inflated texts.  Plain C++: with -DHGX_READS_STANDALONE this
// unit and hgx_align_host.cpp (-DHGX_ALIGN_STANDALONE) link without the device units (tools/reads_host_main.cpp), for the
// sanitizers.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <stdexcept>

#include "hgx_reads.hpp"

extern "C" void hgx_set_error(const char *fmt, ...);
extern "C" const char *hgx_test_switch(const char *name);

namespace {
thread_local int g_route = 0, g_decline = 0, g_max_len = 0;
thread_local int64_t g_n = 0;

}      // namespace

size_t hgx_reads_max_bytes() {
    const char *sw = hgx_test_switch("reads_max_bytes");
    return sw ? (size_t)strtoull(sw, nullptr, 10) : HGX_RD_MAX_BYTES;
}

void hgx_reads_set_last(const hgx_reads *r) {
    g_route = r->route;
    g_decline = r->decline;
    g_n = r->n;
    g_max_len = r->max_len;
}

#ifdef HGX_READS_STANDALONE
// no kernels in the stand-alone build: every table is the loader's
int hgx_reads_make_dev(hgx_reads *r, const std::string *, int, int, void *) { r->decline = HGX_RD_DECLINE_SWITCH; return HGX_OK; }
int hgx_reads_to_host(const hgx_reads *, hgx_aln_reads &) { return HGX_EINVAL; }
int hgx_reads_text_to_host(const hgx_reads *, size_t, size_t, char *) { return HGX_EINVAL; }
void hgx_reads_dev_free(hgx_reads *) {}
#endif

// the loader's table over the inflated texts, which the object keeps (a table declined with code `decline`)
int hgx_reads_host_table(hgx_reads *r, std::vector<std::string> &text, int fastq, int decline) {
    r->route = 0;
    r->decline = decline;
    r->host = hgx_aln_reads();
    const int rc = hgx_aln_reads_of_texts(r->n_inputs, text.data(), fastq, r->host);
    if (rc) return rc;
    r->n = (int64_t)r->host.n();
    r->max_len = 0;
    for (int32_t l : r->host.len) r->max_len = std::max(r->max_len, (int)l);
    r->src.swap(text);
    for (int i = 0; i < r->n_inputs; ++i) { r->in_off[i] = 0; r->in_bytes[i] = r->src[i].size(); }
    return HGX_OK;
}

extern "C" int hgx_reads_from_text(hgx_reads **out, int32_t n_inputs, const char *const *paths, const char *const *texts,
                                   const size_t *text_bytes, int32_t fastq, void *stream) {
    if (!out || (n_inputs != 1 && n_inputs != 2) || (!paths && !(texts && text_bytes)) || fastq < -1 || fastq > 1) {
        hgx_set_error("invalid argument: hgx_reads_from_text");
        return HGX_EINVAL;
    }
    *out = nullptr;
    try {
        std::vector<std::string> text(n_inputs);
        size_t total = 0;
        for (int i = 0; i < n_inputs; ++i) {
            const int rc = hgx_aln_inflate_input(paths ? paths[i] : nullptr, paths ? nullptr : texts[i], paths ? 0 : text_bytes[i], text[i]);
            if (rc) return rc;
            total += text[i].size();
        }
        std::unique_ptr<hgx_reads> r(new hgx_reads);
        r->n_inputs = n_inputs;
        const char *sw = hgx_test_switch("front");
        int decline = 0;
        if (sw && !strcmp(sw, "host")) decline = HGX_RD_DECLINE_SWITCH;
        else if (total + HGX_RD_ALIGN >= hgx_reads_max_bytes()) decline = HGX_RD_DECLINE_SIZE;      // (whatever the padding turns out to be)
        else if (!(sw && !strcmp(sw, "device")) && total < HGX_RD_GATE) decline = HGX_RD_DECLINE_GATE;
        if (!decline) {
            const int rc = hgx_reads_make_dev(r.get(), text.data(), n_inputs, fastq, stream);
            if (rc) return rc;
            decline = r->decline;
        }
        if (decline) {
            const int rc = hgx_reads_host_table(r.get(), text, fastq, decline);
            if (rc) return rc;
        }
        hgx_reads_set_last(r.get());
        *out = r.release();
        return HGX_OK;
    } catch (const std::exception &e) {
        hgx_set_error("hgx_reads_from_text: %s", e.what());
        return HGX_ENOMEM;
    }
}

extern "C" int hgx_reads_dims(const hgx_reads *r, int32_t *n_inputs, int32_t *route, int32_t *decline, int64_t *n_reads, int32_t *max_len,
                              size_t *table_text_bytes) {
    if (!r) { hgx_set_error("invalid argument: hgx_reads_dims"); return HGX_EINVAL; }
    if (n_inputs) *n_inputs = r->n_inputs;
    if (route) *route = r->route;
    if (decline) *decline = r->decline;
    if (n_reads) *n_reads = r->n;
    if (max_len) *max_len = r->max_len;
    if (table_text_bytes) *table_text_bytes = r->route == 2 ? r->text_bytes : r->host.text.size();
    return HGX_OK;
}

extern "C" int hgx_reads_table(const hgx_reads *r, char *text, int64_t *name_off, int64_t *seq_off, int64_t *qual_off, int32_t *name_len,
                               int32_t *len) {
    if (!r || !text || !name_off || !seq_off || !qual_off || !name_len || !len) {
        hgx_set_error("invalid argument: hgx_reads_table");
        return HGX_EINVAL;
    }
    try {
        hgx_aln_reads down;
        if (r->route == 2) {
            const int rc = hgx_reads_to_host(r, down);
            if (rc) return rc;
        }
        const hgx_aln_reads &t = r->route == 2 ? down : r->host;
        const size_t n = t.n();
        if (!t.text.empty()) memcpy(text, t.text.data(), t.text.size());
        if (n) {
            memcpy(name_off, t.name_off.data(), n * 8);
            memcpy(seq_off, t.seq_off.data(), n * 8);
            memcpy(qual_off, t.qual_off.data(), n * 8);
            memcpy(name_len, t.name_len.data(), n * 4);
            memcpy(len, t.len.data(), n * 4);
        }
        return HGX_OK;
    } catch (const std::exception &e) {
        hgx_set_error("hgx_reads_table: %s", e.what());
        return HGX_ENOMEM;
    }
}

extern "C" int hgx_reads_input_text(const hgx_reads *r, int32_t input, char *text, size_t *n_bytes) {
    if (!r || input < 0 || input >= r->n_inputs || !n_bytes) { hgx_set_error("invalid argument: hgx_reads_input_text"); return HGX_EINVAL; }
    *n_bytes = r->in_bytes[input];
    if (!text) return HGX_OK;
    if (r->route == 2) return hgx_reads_text_to_host(r, r->in_off[input], r->in_bytes[input], text);
    if (r->in_bytes[input]) memcpy(text, r->src[(size_t)input].data(), r->in_bytes[input]);
    return HGX_OK;
}

extern "C" int hgx_reads_last(int32_t *route, int32_t *decline, int64_t *n_reads, int32_t *max_len) {
    if (route) *route = g_route;
    if (decline) *decline = g_decline;
    if (n_reads) *n_reads = g_n;
    if (max_len) *max_len = g_max_len;
    return HGX_OK;
}

extern "C" int hgx_reads_free(hgx_reads *r) {
    if (r) {
        hgx_reads_dev_free(r);
        delete r;
    }
    return HGX_OK;
}

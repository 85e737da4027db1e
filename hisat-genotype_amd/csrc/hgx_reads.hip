// hgx_reads.hip -- the aligner's read table made from FASTA / FASTQ text where it lies in HBM (gfx950, wave64).
// What load_reads of hgx_align_host.cpp does on one host thread (a memchr line walk, a re-pack of every base) for the inputs where
// its rules need no re-pack: the five arrays of hgx_dev_reads point into the text as it lies.  Stages, per input:
//   k_sam_nl<0>    newlines per HGX_RD_TILE bytes (a wavefront reads 1 KB per step, 16 bytes per lane, a SWAR zero-byte test per
//                  dword): the front end's newline pass, shared through hgx_nl_tiles.hpp
//   hgx_scan_u32_dev over the tile counts
//   k_sam_nl<1>    the same walk again, writing every line's start (starts[0] = 0 and, for a last line without '\n', the entry
//                  behind the last one = n + 1, as if a newline stood behind the text, come from the host)
//   k_rd_records   a lane per record (FASTQ: lines 4r .. 4r + 3; FASTA: 2r, 2r + 1): marker, name end, one '\r' per line, the
//                  quality length, the bases word-wise for a-z, the call's longest read; the record is stored at its INTERLEAVED
//                  place (read 2k + i = record k of input i), so the two inputs' tables need no third pass
// A rule the device does not take raises the decline word (atomicMin: the smallest code wins) and the host loader makes the table.
// Every index is bounded by what the host sized the buffers with: tiles by the text's bytes, starts by the newline total that the
// same walk counted, records by the line count.
#include <algorithm>

#include "hgx_common.hpp"
#include "hgx_reads.hpp"

namespace {
constexpr int TILE = HGX_RD_TILE;
static_assert(TILE % 1024 == 0, "a wavefront reads 1 KB per step");

#include "hgx_nl_tiles.hpp"            // SAM_TILE, k_sam_nl<0/1>: the front end's newline pass (hgx_front_lines.hpp), one copy
static_assert(SAM_TILE == TILE, "align.READS_TILE is the shared pass's tile");

__device__ __forceinline__ bool rd_has_lower(const unsigned char *p, uint32_t n) {      // a byte in a-z, eight per look
    uint32_t q = 0;
    for (; q + 8 <= n; q += 8) {
        unsigned long long w;
        __builtin_memcpy(&w, p + q, 8);
        const unsigned long long y = w & 0x7F7F7F7F7F7F7F7FULL;
        const unsigned long long ge = y + 0x1F1F1F1F1F1F1F1FULL, gt = y + 0x0505050505050505ULL;      // bit 7: >= 'a', > 'z' (no carry across bytes)
        if (ge & ~gt & ~w & 0x8080808080808080ULL) return true;
    }
    for (; q < n; ++q)
        if (p[q] >= 'a' && p[q] <= 'z') return true;
    return false;
}

struct RdInput {
    const unsigned char *text;            // the input's first byte
    uint32_t base;                        // where it lies in the allocation (the offsets written count from the allocation's first byte)
    const uint32_t *starts;               // n_lines + 1 entries
    uint32_t n_lines, n_rec;
    int fastq, which, n_inputs;
};
// ctl[0]: the decline word (0xFFFFFFFF: none), ctl[1]: the longest read
__global__ void __launch_bounds__(256) k_rd_records(RdInput in, int64_t *__restrict__ name_off, int64_t *__restrict__ seq_off,
                                                    int64_t *__restrict__ qual_off, int32_t *__restrict__ name_len, int32_t *__restrict__ len,
                                                    uint32_t *ctl) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r > in.n_rec) return;
    const unsigned char *t = in.text;
    const uint32_t per = in.fastq ? 4u : 2u;
    auto line = [&](uint32_t l, uint32_t &b, uint32_t &e) {      // [b, e) without its end and one '\r'
        b = in.starts[l];
        e = in.starts[l + 1] - 1u;
        if (e > b && t[e - 1] == '\r') --e;
    };
    uint32_t code = 0;
    auto bad = [&](uint32_t c) { if (!code || c < code) code = c; };
    if (r == in.n_rec) {                                         // the lines behind the last whole record: the empty-line rule alone
        for (uint32_t l = per * in.n_rec; l < in.n_lines; ++l) {
            uint32_t b, e;
            line(l, b, e);
            if (e == b) bad(HGX_RD_DECLINE_EMPTY_LINE);
        }
        if (code) atomicMin(ctl, code);
        return;
    }
    const uint32_t l0 = per * r;
    uint32_t hb, he, sb, se, qb = 0, qe = 0;
    line(l0, hb, he);
    line(l0 + 1, sb, se);
    uint32_t nb = hb, ne = hb;                                   // the name
    if (he == hb) bad(HGX_RD_DECLINE_EMPTY_LINE);
    else {
        if (t[hb] != (in.fastq ? '@' : '>')) bad(HGX_RD_DECLINE_MARKER);
        nb = ne = hb + 1;
        while (ne < he && t[ne] != ' ' && t[ne] != '\t') ++ne;
    }
    if (se == sb) bad(HGX_RD_DECLINE_EMPTY_LINE);
    if (in.fastq) {
        uint32_t pb, pe;
        line(l0 + 2, pb, pe);
        line(l0 + 3, qb, qe);
        if (pe == pb || qe == qb) bad(HGX_RD_DECLINE_EMPTY_LINE);
        if (qe - qb != se - sb) bad(HGX_RD_DECLINE_QUAL_LEN);
    } else if (se > sb && t[sb] == '>') bad(HGX_RD_DECLINE_MARKER);      // (a header behind a header: the loader's record of 0 bases)
    if (rd_has_lower(t + sb, se - sb)) bad(HGX_RD_DECLINE_LOWER);
    const size_t at = (size_t)r * in.n_inputs + in.which;
    name_off[at] = (int64_t)in.base + nb;
    name_len[at] = (int32_t)(ne - nb);
    seq_off[at] = (int64_t)in.base + sb;
    len[at] = (int32_t)(se - sb);
    qual_off[at] = in.fastq ? (int64_t)in.base + qb : -1;
    atomicMax(ctl + 1, se - sb);
    if (code) atomicMin(ctl, code);
}

size_t tab_bytes(size_t n) { return n * 32 + 64; }
void tab_view(hgx_reads *r, size_t cap) {
    char *p = (char *)r->d_tab;
    r->dv.text = (const char *)r->d_text;
    r->dv.name_off = (const int64_t *)p;
    r->dv.seq_off = (const int64_t *)(p + cap * 8);
    r->dv.qual_off = (const int64_t *)(p + cap * 16);
    r->dv.name_len = (const int32_t *)(p + cap * 24);
    r->dv.len = (const int32_t *)(p + cap * 28);
    r->dv.paired = r->n_inputs == 2;
}
}      // namespace

void hgx_reads_dev_free(hgx_reads *r) {
    if (r->d_text) hgx_pool_free(r->d_text);
    if (r->d_tab) hgx_pool_free(r->d_tab);
    r->d_text = r->d_tab = nullptr;
    r->dv = hgx_dev_reads{};
}

int hgx_reads_table_dev(hgx_reads *r, int fastq, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    const int ni = r->n_inputs;
    r->route = 0;
    r->decline = 0;
    if (r->text_bytes >= hgx_reads_max_bytes()) { r->decline = HGX_RD_DECLINE_SIZE; return HGX_OK; }
    const unsigned char *text = (const unsigned char *)r->d_text;
    DevBuf b_ctl, b_cnt[2], b_base[2], b_scan[2], b_starts[2];
    Drain drain{st};
    ALLOC(b_ctl, 64);
    uint32_t *ctl = b_ctl.as<uint32_t>();                        // [0] decline, [1] longest read, [2 + i] input i's newlines
    HIPCHK(hipMemsetAsync(ctl, 0, 64, st));
    HIPCHK(hipMemsetAsync(ctl, 0xFF, 4, st));
    uint32_t n_tiles[2] = {0, 0};
    unsigned char edge[2][2] = {{0, 0}, {0, 0}};                 // each input's first and last byte
    for (int i = 0; i < ni; ++i) {
        const size_t n = r->in_bytes[i];
        if (!n) continue;
        const unsigned char *t = text + r->in_off[i];
        n_tiles[i] = (uint32_t)((n + TILE - 1) / TILE);
        ALLOC(b_cnt[i], (size_t)n_tiles[i] * 4);
        ALLOC(b_base[i], (size_t)n_tiles[i] * 4 + 16);
        ALLOC(b_scan[i], hgx_scan_u32_scratch_bytes(n_tiles[i]) + 16);
        k_sam_nl<0><<<nblk(n_tiles[i], 4), 256, 0, st>>>(t, n, n_tiles[i], b_cnt[i].as<uint32_t>(), nullptr, nullptr);
        HIPCHK(hipGetLastError());
        TRY(hgx_scan_u32_dev(b_cnt[i].as<uint32_t>(), b_base[i].as<uint32_t>(), n_tiles[i], b_scan[i].p, ctl + 2 + i, st));
        HIPCHK(hipMemcpyAsync(&edge[i][0], t, 1, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(&edge[i][1], t + n - 1, 1, hipMemcpyDeviceToHost, st));
    }
    uint32_t back[4] = {0, 0, 0, 0};
    HIPCHK(hipMemcpyAsync(back, ctl, 16, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    uint32_t n_lines[2] = {0, 0}, n_rec[2] = {0, 0}, behind[2] = {0, 0}, code = 0;
    int fq[2] = {0, 0};
    auto bad = [&](uint32_t c) { if (!code || c < code) code = c; };
    for (int i = 0; i < ni; ++i) {
        const size_t n = r->in_bytes[i];
        fq[i] = fastq < 0 ? (n > 0 && edge[i][0] == '@') : fastq != 0;
        if (!n) continue;
        const uint32_t n_nl = back[2 + i], per = fq[i] ? 4u : 2u;
        const int ends_nl = edge[i][1] == '\n';
        n_lines[i] = n_nl + (ends_nl ? 0u : 1u);
        n_rec[i] = n_lines[i] / per;
        if (n_lines[i] % per) bad(HGX_RD_DECLINE_TRUNCATED);
        ALLOC(b_starts[i], ((size_t)n_nl + 2) * 4);
        HIPCHK(hipMemsetAsync(b_starts[i].p, 0, 4, st));                     // the first line starts at 0
        behind[i] = (uint32_t)n + 1u;
        if (!ends_nl) HIPCHK(hipMemcpyAsync(b_starts[i].as<uint32_t>() + n_nl + 1, &behind[i], 4, hipMemcpyHostToDevice, st));
        k_sam_nl<1><<<nblk(n_tiles[i], 4), 256, 0, st>>>(text + r->in_off[i], n, n_tiles[i], nullptr, b_base[i].as<uint32_t>(),
                                                         b_starts[i].as<uint32_t>());
        HIPCHK(hipGetLastError());
    }
    if (ni == 2 && n_rec[0] != n_rec[1]) bad(HGX_RD_DECLINE_COUNT);
    const size_t cap = (size_t)std::max(n_rec[0], n_rec[1]) * ni;      // (every record has its place, whichever input is the longer)
    if (r->d_tab) { hgx_pool_free(r->d_tab); r->d_tab = nullptr; }
    r->d_tab = hgx_pool_alloc(tab_bytes(cap));
    if (!r->d_tab) { hgx_set_error("device allocation of %zu bytes failed", tab_bytes(cap)); return HGX_ENOMEM; }
    tab_view(r, cap);
    for (int i = 0; i < ni; ++i) {
        if (!r->in_bytes[i]) continue;
        const RdInput in{text + r->in_off[i], (uint32_t)r->in_off[i], b_starts[i].as<uint32_t>(), n_lines[i], n_rec[i], fq[i], i, ni};
        k_rd_records<<<nblk((long)n_rec[i] + 1, 256), 256, 0, st>>>(in, (int64_t *)r->dv.name_off, (int64_t *)r->dv.seq_off, (int64_t *)r->dv.qual_off,
                                                                    (int32_t *)r->dv.name_len, (int32_t *)r->dv.len, ctl);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemcpyAsync(back, ctl, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (back[0] != 0xFFFFFFFFu) bad(back[0]);
    if (back[1] > HGX_ALN_MAX_READ) bad(HGX_RD_DECLINE_READ_LEN);
    if (code) {
        r->decline = (int)code;
        hgx_pool_free(r->d_tab);
        r->d_tab = nullptr;
        r->dv = hgx_dev_reads{};
        return HGX_OK;
    }
    r->route = 2;
    r->n = (int64_t)cap;
    r->max_len = (int)back[1];
    return HGX_OK;
}

int hgx_reads_make_dev(hgx_reads *r, const std::string *text, int n_inputs, int fastq, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    r->n_inputs = n_inputs;
    size_t at = 0;
    for (int i = 0; i < n_inputs; ++i) {
        at = (at + HGX_RD_ALIGN - 1) / HGX_RD_ALIGN * HGX_RD_ALIGN;
        r->in_off[i] = at;
        r->in_bytes[i] = text[i].size();
        at += text[i].size();
    }
    r->text_bytes = at;
    if (at >= hgx_reads_max_bytes()) { r->route = 0; r->decline = HGX_RD_DECLINE_SIZE; return HGX_OK; }
    r->d_text = hgx_pool_alloc(at + 64);
    if (!r->d_text) { hgx_set_error("device allocation of %zu bytes failed", at + 64); return HGX_ENOMEM; }
    // (the gap in front of input 2 and the 64 bytes behind the text are zeroed: no kernel reads them as text, the aligner's
    // kernels may load past a read's last base)
    if (n_inputs == 2 && r->in_off[1] > r->in_bytes[0])
        HIPCHK(hipMemsetAsync((char *)r->d_text + r->in_bytes[0], 0, r->in_off[1] - r->in_bytes[0], st));
    HIPCHK(hipMemsetAsync((char *)r->d_text + at, 0, 64, st));
    for (int i = 0; i < n_inputs; ++i)
        if (!text[i].empty()) HIPCHK(hipMemcpyAsync((char *)r->d_text + r->in_off[i], text[i].data(), text[i].size(), hipMemcpyHostToDevice, st));
    const int rc = hgx_reads_table_dev(r, fastq, stream);
    if (rc || r->decline) {
        (void)hipStreamSynchronize(st);
        hgx_reads_dev_free(r);
    }
    return rc;
}

int hgx_reads_text_to_host(const hgx_reads *r, size_t off, size_t n, char *out) {
    if (n) HIPCHK(hipMemcpy(out, (const char *)r->d_text + off, n, hipMemcpyDeviceToHost));
    return HGX_OK;
}

int hgx_reads_to_host(const hgx_reads *r, hgx_aln_reads &out) {
    const size_t n = (size_t)r->n;
    out.text.resize(r->text_bytes);
    out.name_off.resize(n); out.seq_off.resize(n); out.qual_off.resize(n); out.name_len.resize(n); out.len.resize(n);
    out.paired = r->n_inputs == 2;
    TRY(hgx_reads_text_to_host(r, 0, r->text_bytes, out.text.data()));
    if (n) {
        HIPCHK(hipMemcpy(out.name_off.data(), r->dv.name_off, n * 8, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(out.seq_off.data(), r->dv.seq_off, n * 8, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(out.qual_off.data(), r->dv.qual_off, n * 8, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(out.name_len.data(), r->dv.name_len, n * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(out.len.data(), r->dv.len, n * 4, hipMemcpyDeviceToHost));
    }
    return HGX_OK;
}

int hgx_reads_len_to_host(const hgx_reads *r, std::vector<int32_t> &len) {
    len.resize((size_t)r->n);
    if (r->n) HIPCHK(hipMemcpy(len.data(), r->dv.len, (size_t)r->n * 4, hipMemcpyDeviceToHost));
    return HGX_OK;
}

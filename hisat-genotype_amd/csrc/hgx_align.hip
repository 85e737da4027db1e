// hgx_align.hip -- the "hgx" aligner's kernels (gfx950, wave64).  The per-anchor search, the pick and the record
// text are the core's (hgx_align_core.hpp), the same code the host route runs; this unit is the index in HBM, the grids and the
// fixed-size scratch.  Stages of one chunk of reads:
//   k_aln_seed     a lane per (read, strand, seed offset): the 16-mer's code, the probe of the open-addressing table, one anchor
//                  slot per hit (HGX_ALN_DEV_ANCHORS per read; a read with more declines the call)
//   k_aln_extend   a lane per anchor slot: canon(a) by the core's depth-first search, scratch in the lane's private memory; a limit
//                  reached raises the decline code and writes nothing
//   k_aln_pick     a lane per read: the smallest canon(a) and NH
//   k_aln_emit     a lane per read, twice: record sizes, (exclusive scan,) then the SAM lines at their offsets; the pair's flags are
//                  read off the mate's pick
// Every write is bounds-checked by construction: slots < HGX_ALN_DEV_ANCHORS, a record's bytes = the size the same code counted.
#include "hgx_common.hpp"
#include "hgx_align.hpp"

namespace {
typedef hgx_aln_res<HGX_ALN_DEV_VARS> DevRes;
constexpr int CHUNK = 8192;           // reads per chunk (an even number: mates stay together)

struct DevReads {
    const char *text;
    const int64_t *name_off, *seq_off, *qual_off;
    const int32_t *name_len, *len;
    int paired;
};

__global__ void __launch_bounds__(256)
k_aln_seed(hgx_aln_view V, DevReads rd, long first, int nc, int n_off_max, int32_t *cnt, int2 *anch) {
    const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (long)nc * 2 * n_off_max) return;
    const int k = (int)(gid % n_off_max), strand = (int)((gid / n_off_max) & 1), i = (int)(gid / (2L * n_off_max));
    const int L = rd.len[first + i];
    if (k >= hgx_aln_n_offsets(L)) return;
    const hgx_aln_read R{rd.text + rd.seq_off[first + i], L, strand};
    const int o = hgx_aln_offset(L, k);
    uint32_t code;
    if (!hgx_aln_seed_code(R, o, &code)) return;
    for (uint32_t h = hgx_aln_hash(code) & V.hmask; V.hpos[h] >= 0; h = (h + 1) & V.hmask) {
        if (V.hkey[h] != code) continue;
        const int slot = atomicAdd(&cnt[i], 1);
        if (slot < HGX_ALN_DEV_ANCHORS) anch[(long)i * HGX_ALN_DEV_ANCHORS + slot] = make_int2(o | (strand << 16), V.hpos[h]);
    }
}

__global__ void __launch_bounds__(64)
k_aln_extend(hgx_aln_view V, DevReads rd, long first, int nc, int max_edits, const int32_t *cnt, const int2 *anch, DevRes *res,
             int *decline) {
    const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (long)nc * HGX_ALN_DEV_ANCHORS) return;
    const int i = (int)(gid / HGX_ALN_DEV_ANCHORS), slot = (int)(gid % HGX_ALN_DEV_ANCHORS);
    const int n = cnt[i];
    if (n > HGX_ALN_DEV_ANCHORS) {
        if (slot == 0) atomicMax(decline, HGX_ALN_DECLINE_ANCHORS);
        return;
    }
    if (slot >= n) return;
    hgx_aln_frame stk[HGX_ALN_DEV_STK];
    int32_t cur[HGX_ALN_DEV_VARS];
    hgx_aln_side<HGX_ALN_DEV_VARS> side;
    hgx_aln_no_memo memo;
    const int2 a = anch[gid];
    const hgx_aln_read R{rd.text + rd.seq_off[first + i], rd.len[first + i], a.x >> 16};
    const int rc = hgx_aln_canon<HGX_ALN_DEV_STK, HGX_ALN_DEV_VARS>(V, R, a.x & 0xffff, a.y, max_edits, HGX_ALN_DEV_STEPS, stk, cur, side,
                                                                   res[gid], memo);
    if (rc) { res[gid].ok = 0; atomicMax(decline, rc); }
}

__global__ void __launch_bounds__(64)
k_aln_pick(int nc, const int32_t *cnt, const DevRes *res, int32_t *best, int32_t *nh) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nc) return;
    const int n = cnt[i] < HGX_ALN_DEV_ANCHORS ? cnt[i] : HGX_ALN_DEV_ANCHORS;
    int h = 0;
    best[i] = hgx_aln_pick(res + (long)i * HGX_ALN_DEV_ANCHORS, n, &h);
    nh[i] = h;
}

// out == nullptr: sizes[i] and flags[i] (1 aligned, 2 = mate 1 of a concordant pair); else the line at out + off[i]
__global__ void __launch_bounds__(64)
k_aln_emit(hgx_aln_view V, DevReads rd, long first, int nc, int max_fragment, const DevRes *res, const int32_t *best, const int32_t *nh,
           uint32_t *sizes, int32_t *flags, const uint32_t *off, char *out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nc) return;
    if (best[i] < 0) {
        if (!out) { sizes[i] = 0; flags[i] = 0; }
        return;
    }
    const DevRes &a = res[(long)i * HGX_ALN_DEV_ANCHORS + best[i]];
    DevRes none;
    none.ok = 0;
    const DevRes *mate = nullptr;
    if (rd.paired) {
        const int j = i ^ 1;
        mate = best[j] >= 0 ? &res[(long)j * HGX_ALN_DEV_ANCHORS + best[j]] : &none;
    }
    const long r = first + i;
    hgx_aln_out w{out ? out + off[i] : nullptr, 0};
    hgx_aln_line(V, rd.text + rd.name_off[r], rd.name_len[r], rd.text + rd.seq_off[r], rd.qual_off[r] >= 0 ? rd.text + rd.qual_off[r] : nullptr,
                 rd.len[r], a, nh[i], mate, i & 1, max_fragment, w);
    if (!out) {
        sizes[i] = (uint32_t)w.n;
        flags[i] = 1 | ((rd.paired && !(i & 1) && hgx_aln_concordant(a, *mate, max_fragment)) ? 2 : 0);
    }
}

template <class T> size_t put(std::vector<char> &blk, const std::vector<T> &v) {
    const size_t off = (blk.size() + 15) & ~(size_t)15;
    blk.resize(off + std::max<size_t>(v.size() * sizeof(T), 16));
    if (!v.empty()) memcpy(blk.data() + off, v.data(), v.size() * sizeof(T));
    return off;
}

// the index in HBM, made once per index and device
int ensure_device_index(hgx_align_index *ix) {
    std::lock_guard<std::mutex> g(ix->mu);
    int dev = 0;
    HIPCHK(hipGetDevice(&dev));
    if (ix->dev_ready == dev) return HGX_OK;
    if (ix->d_block) { (void)hipFree(ix->d_block); ix->d_block = nullptr; ix->dev_ready = -1; }
    std::vector<char> blk;
    const size_t o_bb = put(blk, ix->bb), o_bo = put(blk, ix->bb_off), o_hk = put(blk, ix->hkey), o_hp = put(blk, ix->hpos),
                 o_vt = put(blk, ix->vtype), o_vp = put(blk, ix->vpos), o_vl = put(blk, ix->vlen), o_vd = put(blk, ix->vdata),
                 o_io = put(blk, ix->vid_off), o_il = put(blk, ix->vid_len), o_no = put(blk, ix->name_off), o_nl = put(blk, ix->name_len),
                 o_pl = put(blk, ix->pool), o_so = put(blk, ix->sgl_off), o_s = put(blk, ix->sgl), o_do = put(blk, ix->dls_off),
                 o_d = put(blk, ix->dls), o_eo = put(blk, ix->dle_off), o_e = put(blk, ix->dle), o_no2 = put(blk, ix->ins_off),
                 o_n = put(blk, ix->ins);
    HIPCHK(hipMalloc(&ix->d_block, blk.size()));
    HIPCHK(hipMemcpy(ix->d_block, blk.data(), blk.size(), hipMemcpyHostToDevice));
    const char *b = (const char *)ix->d_block;
    hgx_aln_view &V = ix->dv;
    V = ix->hv;
    V.bb = b + o_bb; V.bb_off = (const int32_t *)(b + o_bo); V.hkey = (const uint32_t *)(b + o_hk); V.hpos = (const int32_t *)(b + o_hp);
    V.vtype = (const uint8_t *)(b + o_vt); V.vpos = (const int32_t *)(b + o_vp); V.vlen = (const int32_t *)(b + o_vl);
    V.vdata = (const int32_t *)(b + o_vd); V.vid_off = (const int32_t *)(b + o_io); V.vid_len = (const int32_t *)(b + o_il);
    V.name_off = (const int32_t *)(b + o_no); V.name_len = (const int32_t *)(b + o_nl); V.pool = b + o_pl;
    V.sgl_off = (const int32_t *)(b + o_so); V.sgl = (const int32_t *)(b + o_s); V.dls_off = (const int32_t *)(b + o_do);
    V.dls = (const int32_t *)(b + o_d); V.dle_off = (const int32_t *)(b + o_eo); V.dle = (const int32_t *)(b + o_e);
    V.ins_off = (const int32_t *)(b + o_no2); V.ins = (const int32_t *)(b + o_n);
    ix->dev_ready = dev;
    return HGX_OK;
}
}      // namespace

void hgx_align_device_free(hgx_align_index *ix) {
    if (ix->d_block) (void)hipFree(ix->d_block);
    ix->d_block = nullptr;
    ix->dev_ready = -1;
}

int hgx_align_device(hgx_align_index *ix, const hgx_aln_reads &reads, const hgx_align_opts *opts, std::string &body, int64_t *aligned,
                     int64_t *concordant, int *decline) {
    *decline = 0;
    const size_t body0 = body.size();
    const int64_t aligned0 = *aligned, concordant0 = *concordant;
    const long n = (long)reads.n();
    int max_len = 0;
    for (long i = 0; i < n; ++i) max_len = std::max(max_len, (int)reads.len[i]);
    if (max_len > HGX_ALN_DEV_MAX_READ) { *decline = HGX_ALN_DECLINE_READ_LEN; return HGX_OK; }
    const int n_off_max = hgx_aln_n_offsets(max_len);
    int rc = ensure_device_index(ix);
    if (rc) return rc;
    hipStream_t st = nullptr;
    DevBuf d_text, d_no, d_so, d_qo, d_nl, d_len;
    ALLOC(d_text, reads.text.size() + 16);
    ALLOC(d_no, n * 8); ALLOC(d_so, n * 8); ALLOC(d_qo, n * 8); ALLOC(d_nl, n * 4); ALLOC(d_len, n * 4);
    HIPCHK(hipMemcpy(d_text.p, reads.text.data(), reads.text.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_no.p, reads.name_off.data(), n * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_so.p, reads.seq_off.data(), n * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_qo.p, reads.qual_off.data(), n * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_nl.p, reads.name_len.data(), n * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_len.p, reads.len.data(), n * 4, hipMemcpyHostToDevice));
    const DevReads rd{d_text.as<char>(), d_no.as<int64_t>(), d_so.as<int64_t>(), d_qo.as<int64_t>(), d_nl.as<int32_t>(), d_len.as<int32_t>(),
                      reads.paired};
    const int cmax = (int)std::min<long>(n, CHUNK);
    DevBuf d_cnt, d_anch, d_res, d_best, d_nh, d_sizes, d_off, d_flags, d_scan, d_misc;
    ALLOC(d_cnt, (size_t)cmax * 4);
    ALLOC(d_anch, (size_t)cmax * HGX_ALN_DEV_ANCHORS * sizeof(int2));
    ALLOC(d_res, (size_t)cmax * HGX_ALN_DEV_ANCHORS * sizeof(DevRes));
    ALLOC(d_best, (size_t)cmax * 4); ALLOC(d_nh, (size_t)cmax * 4); ALLOC(d_sizes, (size_t)cmax * 4); ALLOC(d_off, (size_t)cmax * 4);
    ALLOC(d_flags, (size_t)cmax * 4);
    ALLOC(d_scan, hgx_scan_u32_scratch_bytes(cmax) + 16);
    ALLOC(d_misc, 16);                       // [0] decline code, [1] total bytes
    int *d_decline = d_misc.as<int>();
    uint32_t *d_total = d_misc.as<uint32_t>() + 1;
    std::vector<int32_t> flags(cmax);
    std::string text;
    for (long first = 0; first < n; first += CHUNK) {
        const int nc = (int)std::min<long>(CHUNK, n - first);
        HIPCHK(hipMemsetAsync(d_cnt.p, 0, (size_t)nc * 4, st));
        HIPCHK(hipMemsetAsync(d_misc.p, 0, 16, st));
        const long n_seed = (long)nc * 2 * n_off_max;
        if (n_seed > 0)
            k_aln_seed<<<nblk(n_seed, 256), 256, 0, st>>>(ix->dv, rd, first, nc, n_off_max, d_cnt.as<int32_t>(), d_anch.as<int2>());
        k_aln_extend<<<nblk((long)nc * HGX_ALN_DEV_ANCHORS, 64), 64, 0, st>>>(ix->dv, rd, first, nc, opts->max_edits, d_cnt.as<int32_t>(),
                                                                               d_anch.as<int2>(), d_res.as<DevRes>(), d_decline);
        HIPCHK(hipGetLastError());
        int dec = 0;
        HIPCHK(hipMemcpy(&dec, d_decline, 4, hipMemcpyDeviceToHost));
        if (dec) {                               // (a later chunk: what the earlier ones appended is taken back)
            body.resize(body0);
            *aligned = aligned0;
            *concordant = concordant0;
            *decline = dec;
            return HGX_OK;
        }
        k_aln_pick<<<nblk(nc, 64), 64, 0, st>>>(nc, d_cnt.as<int32_t>(), d_res.as<DevRes>(), d_best.as<int32_t>(), d_nh.as<int32_t>());
        k_aln_emit<<<nblk(nc, 64), 64, 0, st>>>(ix->dv, rd, first, nc, opts->max_fragment, d_res.as<DevRes>(), d_best.as<int32_t>(),
                                                d_nh.as<int32_t>(), d_sizes.as<uint32_t>(), d_flags.as<int32_t>(), nullptr, nullptr);
        HIPCHK(hipGetLastError());
        rc = hgx_scan_u32_dev(d_sizes.as<uint32_t>(), d_off.as<uint32_t>(), nc, d_scan.p, d_total, st);
        if (rc) return rc;
        uint32_t total = 0;
        HIPCHK(hipMemcpy(&total, d_total, 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(flags.data(), d_flags.p, (size_t)nc * 4, hipMemcpyDeviceToHost));
        for (int i = 0; i < nc; ++i) { *aligned += flags[i] & 1; *concordant += (flags[i] >> 1) & 1; }
        if (total) {
            DevBuf d_out;
            ALLOC(d_out, (size_t)total);
            k_aln_emit<<<nblk(nc, 64), 64, 0, st>>>(ix->dv, rd, first, nc, opts->max_fragment, d_res.as<DevRes>(), d_best.as<int32_t>(),
                                                    d_nh.as<int32_t>(), nullptr, nullptr, d_off.as<uint32_t>(), d_out.as<char>());
            HIPCHK(hipGetLastError());
            text.resize(total);
            HIPCHK(hipMemcpy(&text[0], d_out.p, total, hipMemcpyDeviceToHost));
            body += text;
        }
    }
    HIPCHK(hipStreamSynchronize(st));
    return HGX_OK;
}

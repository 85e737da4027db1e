// hgx_records.hpp -- what the routes that walk alignment text one thread per record share (hgx_linear.hip, hgx_extract.hip):
// the byte hash, the pooled per-call arrays, a name hash table (host build, upload, device lookup), the group heads / extents
// kernels, and the small host helpers around them.  Nothing here knows which route calls it.
#pragma once
#include <cstdint>

// Device copy of a name table: names back to back in `pool` (name c = pool[off[c] .. off[c + 1])), `slot` an open-addressing
// table of name indices (-1 = free) over fnv1a & mask, linear probing.  Plain data: the routes' handles (hgx_linear.hpp,
// hgx_extract.hpp) hold one, and the host units that include those see only this.
struct hgx_name_view {
    const char *__restrict__ pool = nullptr;
    const uint32_t *__restrict__ off = nullptr;
    const int32_t *__restrict__ slot = nullptr;
    uint32_t mask = 0;
};

#if defined(__HIPCC__)
#include <algorithm>
#include <initializer_list>
#include <string>
#include <vector>

#include "hgx_common.hpp"
#include "hgx_internal.hpp"

__host__ __device__ static inline uint64_t fnv1a(const char *p, size_t n) {
    uint64_t h = 1469598103934665603ull;
    for (size_t i = 0; i < n; ++i) h = (h ^ (uint8_t)p[i]) * 1099511628211ull;
    return h;
}

// index of the name equal to p[0 .. n), or -1 (hash, then length, then bytes)
__device__ static inline int32_t name_lookup(const hgx_name_view &v, const char *p, uint32_t n) {
    for (uint32_t s = (uint32_t)fnv1a(p, n) & v.mask;; s = (s + 1) & v.mask) {
        const int32_t c = v.slot[s];
        if (c < 0) return -1;
        const uint32_t b = v.off[c];
        if (v.off[c + 1] - b != n) continue;
        uint32_t k = 0;
        while (k < n && v.pool[b + k] == p[k]) ++k;
        if (k == n) return c;
    }
}

// A record opens a group where its name differs from the previous record's (hash, then length, then bytes); a group head then
// writes its index at its scanned position.  Off = the width of the routes' text offsets.
template <class Off>
__global__ void k_rec_heads(const char *__restrict__ text, const uint64_t *__restrict__ kh, const Off *__restrict__ koff,
                            const uint32_t *__restrict__ klen, long M, uint32_t *__restrict__ head) {
    const long j = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= M) return;
    uint32_t h = 1;
    if (j > 0 && kh[j] == kh[j - 1] && klen[j] == klen[j - 1]) {
        const char *a = text + koff[j], *b = text + koff[j - 1];
        uint32_t k = 0;
        const uint32_t n = klen[j];
        while (k < n && a[k] == b[k]) ++k;
        h = k == n ? 0u : 1u;
    }
    head[j] = h;
}

static __global__ void k_rec_gstart(const uint32_t *__restrict__ head, const uint32_t *__restrict__ gid, long M, uint32_t *__restrict__ gstart) {
    const long j = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < M && head[j]) gstart[gid[j]] = (uint32_t)j;
}

struct DevBufs {                         // the call's device arrays, from the library's pool (no hipMalloc per array)
    const char *route;                   // "linear route" / "extract route": how the error message starts
    std::vector<void *> ps;
    explicit DevBufs(const char *route_) : route(route_) {}
    ~DevBufs() { for (void *p : ps) hgx_pool_free(p); }
    template <class T> int get(T *&p, size_t n) {
        void *q = hgx_pool_alloc(std::max<size_t>(n, 1) * sizeof(T));
        if (!q) {
            hgx_set_error("%s: device allocation of %zu bytes failed", route, n * sizeof(T));
            return HGX_ENOMEM;
        }
        ps.push_back(q);
        p = (T *)q;
        return HGX_OK;
    }
};

#define RCHK(x) do { int rc_ = (x); if (rc_) return rc_; } while (0)

// the lowest decline code set in a kernel's decline word (bit b = code b; code 0 is "none")
static inline int first_decline(uint32_t d) {
    for (int b = 1; b < 32; ++b)
        if (d & (1u << b)) return b;
    return 0;
}

// hipMalloc'd arrays of a handle, freed on the device that holds them (`dev`; -1 = none, and so afterwards); the caller clears
// its pointers
static inline void free_on_device(int &dev, std::initializer_list<const void *> ps) {
    if (dev < 0) return;
    int cur = 0;
    const bool switched = hipGetDevice(&cur) == hipSuccess && cur != dev && hipSetDevice(dev) == hipSuccess;
    for (const void *p : ps)
        if (p) (void)hipFree(const_cast<void *>(p));
    if (switched) (void)hipSetDevice(cur);
    dev = -1;
}

// a hipMalloc'd copy of n bytes on the current device (at least 16 bytes: an empty array still has an address)
template <class P> static inline bool upload_array(P &d, const void *src, size_t n) {
    void *q = nullptr;
    if (hipMalloc(&q, std::max<size_t>(n, 16)) != hipSuccess) return false;
    d = (P)q;
    return n == 0 || hipMemcpy(q, src, n, hipMemcpyHostToDevice) == hipSuccess;
}

struct NameTable {                       // the host form: what name_table_upload sends
    std::vector<char> pool;
    std::vector<uint32_t> off{0};
    std::vector<int32_t> slot;
    uint32_t mask;
};

// 2 n + 16 slots rounded up to a power of two; a repeated name keeps its first index (it is met first on the probe path)
static inline NameTable name_table_build(const std::vector<std::string> &names) {
    NameTable t;
    uint32_t ns = 16;
    while (ns < 2 * names.size() + 16) ns <<= 1;
    t.mask = ns - 1;
    t.slot.assign(ns, -1);
    for (size_t c = 0; c < names.size(); ++c) {
        uint32_t s = (uint32_t)fnv1a(names[c].data(), names[c].size()) & t.mask;
        while (t.slot[s] >= 0) s = (s + 1) & t.mask;
        t.slot[s] = (int32_t)c;
        t.pool.insert(t.pool.end(), names[c].begin(), names[c].end());
        t.off.push_back((uint32_t)t.pool.size());
    }
    return t;
}

// false: a HIP call failed (hipGetLastError has it); the caller frees what `v` holds with its other arrays
static inline bool name_table_upload(hgx_name_view &v, const std::vector<std::string> &names) {
    const NameTable t = name_table_build(names);
    v.mask = t.mask;
    return upload_array(v.pool, t.pool.data(), t.pool.size()) && upload_array(v.off, t.off.data(), t.off.size() * 4) &&
           upload_array(v.slot, t.slot.data(), t.slot.size() * 4);
}

// The records of a BAM as the text `samtools view <path> [regions]` prints, newline-joined, in file order.  `tot` = the bytes of
// that text; beyond `limit` nothing is built (the caller words the error).  ls / le, if given: [start, end) of every line.
static inline int bam_as_sam_text(const char *path, const char *regions_or_null, size_t limit, std::vector<char> &text, size_t &tot,
                                  std::vector<uint64_t> *ls = nullptr, std::vector<uint64_t> *le = nullptr) {
    hgx_align_lines t;
    t.file_order = true;
    RCHK(hgx_read_alignment_lines(path, regions_or_null, 0, t));
    tot = 0;
    for (size_t i = 0; i < t.lines.size(); ++i) tot += (size_t)t.lines[i].len + 1;
    if (tot > limit) return HGX_OK;
    text.reserve(tot);
    for (size_t i = 0; i < t.lines.size(); ++i) {
        if (ls) ls->push_back(text.size());
        text.insert(text.end(), t.lines[i].p, t.lines[i].p + t.lines[i].len);
        if (le) le->push_back(text.size());
        text.push_back('\n');
    }
    return HGX_OK;
}
#endif  // __HIPCC__

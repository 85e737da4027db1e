// hgx_nl_tiles.hpp -- the newline pass over text in HBM, shared by the front end's SAM line table (hgx_front_lines.hpp, DESIGN.md
// 5.6) and the aligner's read table (hgx_reads.hip, 5.14).  Included INSIDE each unit's anonymous namespace, behind hgx_common.hpp.
//   k_sam_nl<0>   newlines per tile of SAM_TILE bytes (a wavefront reads 1 KB per step, 16 bytes per lane, a SWAR zero-byte test
//                 per dword) -> cnt[tile]
//   (an exclusive scan of cnt -> base)
//   k_sam_nl<1>   the same walk again: starts[l + 1] = the byte behind newline l (starts[0] = 0 is the caller's)
// The text is 16-byte aligned and its buffer padded; `n` cuts the count.
constexpr int SAM_TILE = 4096;
__device__ __forceinline__ uint32_t sam_nl_mask(uint32_t w) {          // bit 8 k + 7 set where byte k of w is '\n'
    const uint32_t x = w ^ 0x0A0A0A0Au;
    return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u;     // exact zero-byte test (no borrow across bytes)
}
template <int PASS>
__global__ void __launch_bounds__(256) k_sam_nl(const unsigned char *__restrict__ text, size_t n, uint32_t n_tiles, uint32_t *__restrict__ cnt,
                                                const uint32_t *__restrict__ base, uint32_t *__restrict__ starts) {
    const uint32_t tile = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (tile >= n_tiles) return;
    const size_t t0 = (size_t)tile * SAM_TILE;
    uint32_t run = PASS == 1 ? base[tile] : 0u;
    for (int k = 0; k < SAM_TILE / 1024; ++k) {
        const size_t at = t0 + (size_t)k * 1024 + 16u * lane;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (at + 16 <= n) v = *reinterpret_cast<const uint4 *>(text + at);            // (the buffer is padded by 64 bytes; `n` cuts the count)
        else if (at < n) { unsigned char tmp[16] = {0}; for (size_t j = 0; at + j < n; ++j) tmp[j] = text[at + j]; __builtin_memcpy(&v, tmp, 16); }
        const uint32_t m0 = sam_nl_mask(v.x), m1 = sam_nl_mask(v.y), m2 = sam_nl_mask(v.z), m3 = sam_nl_mask(v.w);
        const uint32_t c = (uint32_t)(__popc(m0) + __popc(m1) + __popc(m2) + __popc(m3));
        if (PASS == 0) run += c;
        else {
            const uint32_t incl = wave_incl_scan_u32_front(c);
            uint32_t at_line = run + incl - c;
            const uint32_t ms[4] = {m0, m1, m2, m3};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                uint32_t m = ms[q];
                while (m) {
                    const int b = __ffs((int)m) - 1;                          // bit 8 j + 7
                    m &= m - 1;
                    starts[at_line + 1] = (uint32_t)(at + 4u * q + (uint32_t)(b >> 3) + 1u);
                    ++at_line;
                }
            }
            run += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
        }
    }
    if (PASS == 0) {
        const uint32_t tot = (uint32_t)wave_sum_u64(run);
        if (lane == 0) cnt[tile] = tot;
    }
}

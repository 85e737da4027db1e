// bai_host_check.cpp -- the index reader (csrc/hgx_bai.cpp: parse, query, plan) under a sanitizer, as a program of its own.
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -DHGX_BAI_STANDALONE
//       -I include -I hisat-genotype_amd/csrc tools/bai_host_check.cpp -o bai_host_check
//   ./bai_host_check <index.bai> <size of the BAM in bytes> <references in its header>
//
// It runs the reader over every prefix of the index and over copies with one byte changed (every byte, four values each), with a grid
// of regions per reference.  The verdict of each run must be "unusable" (parse fails, another reference count, a region the binning
// scheme does not reach), or a plan -- which either lies inside the file or is refused by hgx_bai_plan_fits, as the reader refuses
// it.  Anything else, or any sanitizer report, fails the program.  tools/bai_host_check.py builds it, makes an index and runs it.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>

#include "hgx_bai.cpp"

namespace {
struct Tally { long unusable = 0, fits = 0, refused = 0, segments = 0; };

void run(const std::vector<unsigned char> &bytes, uint64_t file_size, size_t n_ref, Tally &t) {
    // (a heap copy of exactly n bytes: a read past the end is a report)
    std::vector<unsigned char> own(bytes.begin(), bytes.end());
    own.shrink_to_fit();
    hgx_bai_index ix;
    if (!hgx_bai_parse(own.data(), own.size(), ix) || ix.refs.size() != n_ref) { ++t.unusable; return; }
    static const int64_t grid[][2] = {{0, (int64_t)1 << 29}, {0, 1}, {16383, 16385}, {14884, 18453}, {(int64_t)7 << 14, ((int64_t)7 << 14) + 20},
                                      {300000, 300100}, {((int64_t)1 << 29) - 1, (int64_t)1 << 29}, {(int64_t)1 << 29, ((int64_t)1 << 29) + 5}, {5, 5}};
    for (size_t r = 0; r <= n_ref; ++r) {                    // (one reference beyond the last, too)
        std::vector<hgx_bai_chunk> chunks, segs;
        bool reach = true;
        for (const auto &g : grid) reach = hgx_bai_query(ix, (int32_t)r, g[0], g[1], chunks) && reach;
        if (!hgx_bai_query(ix, -1, 0, 10, chunks)) reach = false;
        hgx_bai_plan(chunks, segs);
        for (size_t k = 0; k + 1 < segs.size(); ++k)
            if (segs[k].end >= segs[k + 1].beg || segs[k].beg >= segs[k].end) { fprintf(stderr, "plan out of order\n"); exit(2); }
        if (hgx_bai_plan_fits(segs, file_size)) {
            for (const hgx_bai_chunk &s : segs)
                if ((s.beg >> 16) >= file_size || (s.end >> 16) > file_size) { fprintf(stderr, "a plan that fits points outside the file\n"); exit(2); }
            ++t.fits;
        } else ++t.refused;
        t.segments += (long)segs.size();
        (void)reach;
    }
}
}   // namespace

int main(int argc, char **argv) {
    if (argc != 4) { fprintf(stderr, "usage: %s index.bai bam_bytes n_ref\n", argv[0]); return 1; }
    std::ifstream f(argv[1], std::ios::binary);
    const std::vector<unsigned char> data((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    const uint64_t file_size = strtoull(argv[2], nullptr, 10);
    const size_t n_ref = (size_t)strtoull(argv[3], nullptr, 10);
    if (data.empty()) { fprintf(stderr, "cannot read %s\n", argv[1]); return 1; }
    Tally whole, prefixes, changed;
    run(data, file_size, n_ref, whole);
    if (whole.fits != (long)n_ref + 1) { fprintf(stderr, "the intact index is not usable\n"); return 2; }
    for (size_t n = 0; n < data.size(); ++n) run(std::vector<unsigned char>(data.begin(), data.begin() + (long)n), file_size, n_ref, prefixes);
    static const unsigned char flips[4] = {0x01, 0x80, 0xff, 0x55};
    for (size_t i = 0; i < data.size(); ++i)
        for (unsigned char x : flips) {
            std::vector<unsigned char> c = data;
            c[i] ^= x;
            run(c, file_size, n_ref, changed);
        }
    printf("index of %zu bytes: %zu prefixes -> %ld unusable, %ld plans that fit, %ld refused; %zu changed copies -> %ld unusable, %ld fit, %ld refused (%ld segments)\n",
           data.size(), data.size(), prefixes.unusable, prefixes.fits, prefixes.refused, data.size() * 4, changed.unusable, changed.fits, changed.refused,
           changed.segments);
    return 0;
}

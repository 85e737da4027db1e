// align_linear_host_main.cpp -- the host route and the index build of the "hgx" aligner on a linear index as a stand-alone program,
// for sanitizer builds (tools/align_linear_host_check.py builds it and runs it over the case table):
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -DHGX_ALIGN_STANDALONE -I include -I hisat-genotype_amd/csrc \
//       hisat-genotype_amd/csrc/hgx_align_host.cpp hisat-genotype_amd/csrc/hgx_align_linear_host.cpp tools/align_linear_host_main.cpp \
//       -lz -o align_linear_host_main
//   align_linear_host_main <index file> <max_edits> <k> <reads> [<mate reads>]  > out.sam
// The index file is text: "<n_seqs>", then one "<name> <length> <sequence>" line per sequence in index order ("<name> 0" for an empty
// sequence).  Nothing of the GPU library is linked: the kernels' route is a stub that declines.  The last line of stderr holds the
// call's counters (hgx_align_linear_last).
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "hgx.h"

int main(int argc, char **argv) {
    if (argc < 5 || argc > 6) {
        fprintf(stderr, "usage: %s index max_edits k reads [mate reads]\n", argv[0]);
        return 2;
    }
    std::ifstream in(argv[1]);
    int n = 0;
    in >> n;
    std::vector<std::string> names(n > 0 ? n : 0), seqs(n > 0 ? n : 0);
    for (int a = 0; a < n; ++a) {
        long len = -1;
        in >> names[a] >> len;
        if (len > 0) in >> seqs[a];                 // (an empty sequence has no third field)
        if (!in || len < 0 || (long)seqs[a].size() != len) { fprintf(stderr, "bad index file (sequence %d)\n", a); return 2; }
    }
    std::vector<const char *> c_names, c_seqs;
    for (auto &s : names) c_names.push_back(s.c_str());
    for (auto &s : seqs) c_seqs.push_back(s.c_str());
    hgx_align_linear_index *ix = nullptr;
    if (hgx_align_linear_index_create(&ix, n, c_names.data(), c_seqs.data())) return 1;
    const hgx_align_linear_opts o{(int32_t)sizeof(hgx_align_linear_opts), atoi(argv[2]), atoi(argv[3]), -1, 1};
    const char *paths[2] = {argv[4], argc == 6 ? argv[5] : nullptr};
    char *sam = nullptr;
    size_t bytes = 0;
    int rc = hgx_align_linear_reads(ix, argc - 4, paths, nullptr, nullptr, &o, &sam, &bytes);
    if (rc == 0) {
        fwrite(sam, 1, bytes, stdout);
        int32_t route = -1, decline = -1;
        int64_t reads = 0, aligned = 0, records = 0, candidates = 0;
        hgx_align_linear_last(&route, &reads, &aligned, &records, &candidates, &decline);
        fprintf(stderr, "route %d decline %d reads %lld aligned %lld records %lld candidates %lld\n", route, decline, (long long)reads,
                (long long)aligned, (long long)records, (long long)candidates);
    }
    free(sam);
    hgx_align_linear_index_free(ix);
    return rc ? 1 : 0;
}

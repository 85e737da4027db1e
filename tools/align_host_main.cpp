// align_host_main.cpp -- the host route of the "hgx" aligner as a stand-alone program, for sanitizer builds:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -DHGX_ALIGN_STANDALONE -I include -I hisat-genotype_amd/csrc \
//       hisat-genotype_amd/csrc/hgx_align_host.cpp tools/align_host_main.cpp -lz -o align_host_main
//   align_host_main <index file> <max_edits> <reads> [<mate reads>] [search=0|1|2] [pair=0|1] [fragment=N] [clip=N] [gap=N] [rescue=G,C]
//                   [order=read|coordinate]  > out.sam
//   (search, pair, fragment, clip: hgx_align_opts.search, .pair, .max_fragment, .clip; gap: hgx_align_more.gap; rescue: hgx_align_more.gap
//   and .rescue_clip; order: hgx_align_more.order; in any order behind the read files)
// The index file is text: "<n_loci>", then per locus "<name> <backbone> <n_vars>" followed by one "<type 0|1|2> <pos> <data> <id>"
// line per variant in Var_list order.  Nothing of the GPU library is linked.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "hgx.h"

int main(int argc, char **argv) {
    int search = 0, pair = 0, fragment = 1000, clip = 0, gap = 0, rescue_clip = 0, order = 0;
    for (; argc > 4; --argc) {
        const char *a = argv[argc - 1];
        if (!strncmp(a, "search=", 7)) search = atoi(a + 7);
        else if (!strncmp(a, "pair=", 5)) pair = atoi(a + 5);
        else if (!strncmp(a, "fragment=", 9)) fragment = atoi(a + 9);
        else if (!strncmp(a, "clip=", 5)) clip = atoi(a + 5);
        else if (!strncmp(a, "gap=", 4)) gap = atoi(a + 4);
        else if (!strncmp(a, "rescue=", 7) && strchr(a, ',')) { gap = atoi(a + 7); rescue_clip = atoi(strchr(a, ',') + 1); }
        else if (!strcmp(a, "order=coordinate")) order = 1;
        else if (!strcmp(a, "order=read")) order = 0;
        else break;
    }
    if (argc < 4 || argc > 5) {
        fprintf(stderr, "usage: %s index max_edits reads [mate reads] [search=0|1|2] [pair=0|1] [fragment=N] [clip=N] [gap=N] [rescue=G,C]\n", argv[0]);
        return 2;
    }
    std::ifstream in(argv[1]);
    int n_loci = 0;
    in >> n_loci;
    std::vector<std::string> names(n_loci), bbs(n_loci), data, ids;
    std::vector<int32_t> off{0}, type, pos;
    for (int g = 0; g < n_loci; ++g) {
        int nv = 0;
        in >> names[g] >> bbs[g] >> nv;
        for (int v = 0; v < nv; ++v) {
            int t, p;
            std::string d, id;
            in >> t >> p >> d >> id;
            type.push_back(t); pos.push_back(p); data.push_back(d); ids.push_back(id);
        }
        off.push_back((int32_t)type.size());
    }
    if (!in) { fprintf(stderr, "bad index file\n"); return 2; }
    std::vector<const char *> c_names, c_bbs, c_data, c_ids;
    for (auto &s : names) c_names.push_back(s.c_str());
    for (auto &s : bbs) c_bbs.push_back(s.c_str());
    for (auto &s : data) c_data.push_back(s.c_str());
    for (auto &s : ids) c_ids.push_back(s.c_str());
    c_data.push_back(nullptr); c_ids.push_back(nullptr); type.push_back(0); pos.push_back(0);
    hgx_align_index *ix = nullptr;
    if (hgx_align_index_create(&ix, n_loci, c_names.data(), c_bbs.data(), off.data(), type.data(), pos.data(), c_data.data(), c_ids.data()))
        return 1;
    hgx_align_opts o{atoi(argv[2]), fragment, -1, 1, search, pair, clip};
    const char *paths[2] = {argv[3], argc == 5 ? argv[4] : nullptr};
    char *sam = nullptr;
    size_t n = 0;
    const hgx_align_more more{(int32_t)sizeof(hgx_align_more), gap, rescue_clip, order};
    const int rc = hgx_align_reads_x(ix, argc - 3, paths, nullptr, nullptr, &o, gap || rescue_clip || order ? &more : nullptr, &sam, &n);
    if (rc == 0) fwrite(sam, 1, n, stdout);
    free(sam);
    hgx_align_index_free(ix);
    return rc ? 1 : 0;
}

// reads_host_main.cpp -- the HOST half of the aligner's read table as a stand-alone program, for sanitizer builds:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -DHGX_ALIGN_STANDALONE -DHGX_READS_STANDALONE -I include
//       -I hisat-genotype_amd/csrc hisat-genotype_amd/csrc/hgx_align_host.cpp hisat-genotype_amd/csrc/hgx_reads_host.cpp
//       tools/reads_host_main.cpp -lz -o reads_host_main                                    (one command line)
//   reads_host_main <fastq -1|0|1> <reads> [<mate reads>]  > table.txt
//   reads_host_main keep <fastq 0|1> <reads> [<mate reads>]  > table.txt
// hgx_reads_from_text over the files (plain or .gz) with the device unit left out: every table is declined (HGX_RD_DECLINE_SWITCH)
// and made by the loader, as after any decline of the kernels.  Prints "reads N longest L", one line "name<TAB>seq<TAB>qual|-" per
// read, and each input's inflated size -- or the loader's error and exit status 1.  The case texts of tests/reads_table_cases.py
// are written to files by tools/reads_host_cases.py.  Nothing of the GPU library is linked.
// `keep`: the bookkeeping of the extractor's keep mode (csrc/hgx_extract_keep.hpp) over the same files.  Each input is cut into five
// "chunks" at odd places; chunks 0, 1 and 3 arrive as a host-route chunk does (appended to the out strings, 0 and 1 in a row), 2 and
// 4 as a device-route chunk does (a block of their own -- here plain memory -- behind a flush); the family in the middle of three
// holds them, its neighbours nothing.  The join (plain memcpy behind the callbacks) must give the inputs back, which then go
// through the loader and are printed as above; the empty families must plan to 0 bytes, the lists must be empty after the drop,
// and a list whose sizes reach 2 GB -- segments that claim their size and hold no byte: only the plan looks at them -- must be
// refused for the mate that has it.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include <cstring>
#include <memory>

#include "hgx.h"
#include "hgx_extract_keep.hpp"
#include "hgx_reads.hpp"

static int print_table(hgx_reads *r);

static int keep_mode(int fastq, int n_inputs, char **paths) {
    const int n_fam = 3, family = 1;
    std::vector<std::string> text(n_inputs), out(2 * n_fam);
    hgx_keep_lists segs(2 * n_fam);
    std::vector<void *> blocks;
    for (int i = 0; i < n_inputs; ++i)
        if (hgx_aln_inflate_input(paths[i], nullptr, 0, text[i])) return 1;
    size_t cut[2][6];
    for (int i = 0; i < n_inputs; ++i) {
        const size_t n = text[i].size();
        const size_t c[6] = {0, n / 7, n / 7 + (n > 3 ? 3 : 0), n / 2 + (n > 1 ? 1 : 0), n - n / 5, n};
        for (int k = 0; k < 6; ++k) cut[i][k] = c[k] < (k ? cut[i][k - 1] : 0) ? cut[i][k - 1] : c[k];
    }
    for (int chunk = 0; chunk < 5; ++chunk) {
        const bool dev = chunk == 2 || chunk == 4;
        if (dev) hgx_keep_flush(out, segs);                      // (as in front of a device chunk's segments)
        for (int i = 0; i < n_inputs; ++i) {
            const char *p = text[i].data() + cut[i][chunk];
            const size_t n = cut[i][chunk + 1] - cut[i][chunk];
            if (!dev) { out[2 * family + i].append(p, n); continue; }
            if (!n) continue;                                    // (a device chunk makes no empty segment)
            hgx_keep_seg sg;
            sg.n = n;
            sg.d = malloc(n);
            memcpy(sg.d, p, n);
            blocks.push_back(sg.d);
            segs[2 * family + i].push_back(sg);
        }
    }
    hgx_keep_flush(out, segs);                                   // (as in front of the join)
    for (const std::string &o : out)
        if (!o.empty()) { fprintf(stderr, "keep: an out string survived the flush\n"); return 3; }
    size_t freed = 0;
    const auto free_dev = [&](void *p) { free(p); ++freed; };
    for (int f = 0; f < n_fam; ++f) {
        hgx_keep_plan plan;
        int bad = -1;
        size_t bad_bytes = 0;
        if (!hgx_keep_layout(segs, f, n_inputs, plan, &bad, &bad_bytes)) { fprintf(stderr, "keep: family %d refused\n", f); return 3; }
        std::vector<char> joined(plan.text_bytes + 64, 'x');
        hgx_keep_copy copy;
        copy.from_dev = [&](size_t at, const void *d, size_t n) { memcpy(joined.data() + at, d, n); return 0; };
        copy.from_host = [&](size_t at, const char *h, size_t n) { memcpy(joined.data() + at, h, n); return 0; };
        copy.zero = [&](size_t at, size_t n) { memset(joined.data() + at, 0, n); return 0; };
        if (hgx_keep_join(segs, f, n_inputs, plan, copy)) return 3;
        if (f != family) {
            if (plan.text_bytes != 0 || plan.in_bytes[0] || plan.in_bytes[1]) { fprintf(stderr, "keep: an empty family is not empty\n"); return 3; }
            continue;
        }
        std::vector<std::string> back(n_inputs);
        for (int i = 0; i < n_inputs; ++i) {
            if (plan.in_off[i] % HGX_KEEP_ALIGN || plan.in_bytes[i] != text[i].size()) { fprintf(stderr, "keep: input %d misplaced\n", i); return 3; }
            back[i].assign(joined.data() + plan.in_off[i], plan.in_bytes[i]);
            if (back[i] != text[i]) { fprintf(stderr, "keep: input %d is not what went in\n", i); return 3; }
        }
        for (size_t q = plan.in_bytes[0]; n_inputs == 2 && q < plan.in_off[1]; ++q)
            if (joined[q]) { fprintf(stderr, "keep: the gap is not zeroed\n"); return 3; }
        for (size_t q = plan.text_bytes; q < plan.text_bytes + 64; ++q)
            if (joined[q]) { fprintf(stderr, "keep: the tail is not zeroed\n"); return 3; }
        std::unique_ptr<hgx_reads> r(new hgx_reads);
        r->n_inputs = n_inputs;
        if (hgx_reads_host_table(r.get(), back, fastq, HGX_RD_DECLINE_SWITCH)) return 1;
        hgx_reads_set_last(r.get());
        if (print_table(r.get())) return 1;
    }
    for (size_t k = 0; k < segs.size(); ++k) hgx_keep_drop(segs, k, free_dev);
    for (const auto &l : segs)
        if (!l.empty()) { fprintf(stderr, "keep: a list survived the drop\n"); return 3; }
    if (freed != blocks.size()) { fprintf(stderr, "keep: %zu of %zu blocks freed\n", freed, blocks.size()); return 3; }
    // the 2 GB rule, on sizes alone: one byte below it passes, at it and beyond it (and where a sum would wrap) mate 2 is refused
    for (int which = 0; which < 4; ++which) {
        hgx_keep_lists big(2);
        hgx_keep_seg a, b;
        a.n = HGX_KEEP_MAX_BYTES - 10;
        b.n = which == 0 ? 9 : which == 1 ? 10 : which == 2 ? HGX_KEEP_MAX_BYTES : ~(size_t)0 - 5;
        big[1].push_back(a);
        big[1].push_back(b);
        hgx_keep_seg small;
        small.n = 100;
        big[0].push_back(small);
        hgx_keep_plan plan;
        int bad = -1;
        size_t bad_bytes = 0;
        const bool ok = hgx_keep_layout(big, 0, 2, plan, &bad, &bad_bytes);
        if (ok != (which == 0) || (!ok && bad != 1)) { fprintf(stderr, "keep: the 2 GB rule, form %d\n", which); return 3; }
        if (ok && (plan.in_off[1] != 128 || plan.in_bytes[1] != HGX_KEEP_MAX_BYTES - 1 || plan.text_bytes != 128 + HGX_KEEP_MAX_BYTES - 1)) {
            fprintf(stderr, "keep: the plan below 2 GB\n");
            return 3;
        }
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc >= 4 && argc <= 5 && !strcmp(argv[1], "keep")) return keep_mode(atoi(argv[2]), argc - 3, argv + 3);
    if (argc < 3 || argc > 4) {
        fprintf(stderr, "usage: %s fastq(-1|0|1) reads [mate reads]\n", argv[0]);
        return 2;
    }
    const char *paths[2] = {argv[2], argc == 4 ? argv[3] : nullptr};
    hgx_reads *r = nullptr;
    if (hgx_reads_from_text(&r, argc - 2, paths, nullptr, nullptr, atoi(argv[1]), nullptr)) return 1;
    const int rc = print_table(r);
    hgx_reads_free(r);
    return rc;
}

static int print_table(hgx_reads *r) {
    int32_t ni = 0, route = 0, decline = 0, longest = 0;
    int64_t n = 0;
    size_t tb = 0;
    hgx_reads_dims(r, &ni, &route, &decline, &n, &longest, &tb);
    std::vector<char> text(tb + 1);
    std::vector<int64_t> no(n + 1), so(n + 1), qo(n + 1);
    std::vector<int32_t> nl(n + 1), len(n + 1);
    if (hgx_reads_table(r, text.data(), no.data(), so.data(), qo.data(), nl.data(), len.data())) return 1;
    printf("reads %lld longest %d route %d decline %d\n", (long long)n, longest, route, decline);
    for (int64_t i = 0; i < n; ++i) {
        fwrite(text.data() + no[i], 1, (size_t)nl[i], stdout);
        putchar('\t');
        fwrite(text.data() + so[i], 1, (size_t)len[i], stdout);
        putchar('\t');
        if (qo[i] >= 0) fwrite(text.data() + qo[i], 1, (size_t)len[i], stdout);
        else putchar('-');
        putchar('\n');
    }
    for (int i = 0; i < ni; ++i) {
        size_t nb = 0;
        hgx_reads_input_text(r, i, nullptr, &nb);
        std::vector<char> in(nb + 1);
        hgx_reads_input_text(r, i, in.data(), &nb);
        printf("input %d: %zu bytes\n", i, nb);
    }
    int32_t lr = 0, ld = 0, lm = 0;
    int64_t ln = 0;
    hgx_reads_last(&lr, &ld, &ln, &lm);
    if (lr != route || ld != decline || ln != n || lm != longest) { fprintf(stderr, "hgx_reads_last disagrees\n"); return 3; }
    return 0;
}

// reader_host_check.cpp -- the alignment reader (csrc/hgx_bam.cpp, hgx_bai.cpp, hgx_bgzf.cpp) as a host program of its own: what it
// gives back and what it tells the device front end's callbacks, as one deterministic text record per case.
//
//   g++ -std=c++17 -g -O1 -pthread [-fsanitize=address,undefined -fno-sanitize-recover=undefined] -I include -I hisat-genotype_amd/csrc
//       tools/reader_host_check.cpp hisat-genotype_amd/csrc/{hgx_bam,hgx_bai,hgx_bgzf,hgx_host}.cpp -lz -ldl -o reader_host_check
//   ./reader_host_check <manifest>          (run in the directory of the input files: the paths in error texts stay relative)
//
// The manifest (tools/reader_host_check.py writes it and the files) holds one case per line, `key=value` fields separated by tabs:
//   case=<name> path=<file> regions=<r1;r2;...> nt=<threads> keep=<0|1> walk=<0|1> text=<0|1> min=<defer_min_bytes> order=<0|1>
//   on_raw=<0|1> inflate=<answer> splice=<answer> early=<0|1>          (a callback is given when its field is there)
//   sw=<name>:<value>,...   env=<NAME>:<value>,...   grow=<file>:<bytes>  (write `path` first: the text of <file> repeated up to <bytes>)
//   dump_raw=<file> dump_parts=<file>                                  (the handed-over stream / the spliced dense stream, for a test to read)
//   tasks=<file>@<regions>,...                                         (hgx_bgzf_tasks_read over these instead of one reader call)
// Only inflated bytes are hashed (CRC-32, as zlib and Python compute it): the record does not depend on the deflate that wrote a file.
// A callback that is given deflated bytes inflates them and hashes the result, which also checks the block table it was given.
#include <unistd.h>
#include <zlib.h>

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <mutex>
#include <sstream>

#include "hgx_internal.hpp"

// ---- what the host units need from the device units -----------------------------------------------------------------------------------
static std::mutex g_err_mu;
static std::string g_err;
extern "C" void hgx_set_error(const char *fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    std::lock_guard<std::mutex> g(g_err_mu);
    g_err = buf;
}
extern "C" int32_t hgx_a_pad(int32_t n) { return (n + 511) / 512 * 512; }
extern "C" int hgx_index_create(hgx_index **, int32_t, int32_t, const uint32_t *, const uint64_t *, const uint64_t *) { return HGX_EINVAL; }

// (the test switches' values are interned and never freed, by design: hgx_host.cpp)
extern "C" const char *__lsan_default_suppressions() { return "leak:hgx_test_switch_set\n"; }

namespace {

typedef std::map<std::string, std::string> Case;

uint32_t crc_of(const void *p, size_t n) { return (uint32_t)crc32(crc32(0L, Z_NULL, 0), (const Bytef *)p, (uInt)n); }

std::vector<std::string> split(const std::string &s, char c) {
    std::vector<std::string> out;
    if (s.empty()) return out;
    std::stringstream ss(s);
    for (std::string part; std::getline(ss, part, c);) out.push_back(part);
    return out;
}

// the blocks of a table inflated one after the other (out_off order is the table's own): their bytes, or false
bool inflate_table(const unsigned char *data, size_t n, const std::vector<hgx_bgzf_block> &blocks, size_t total, std::vector<unsigned char> &out) {
    out.assign(total, 0);
    for (const hgx_bgzf_block &b : blocks) {
        if (b.in_off + b.in_len + 8 > n || b.out_off + b.out_len > total) return false;
        if (!hgx_bam_inflate_block(data, b, out.data() + b.out_off)) return false;
    }
    return true;
}

void print_table(const char *who, const unsigned char *data, size_t n, const std::vector<hgx_bgzf_block> &blocks, size_t total) {
    std::string t;
    char buf[64];
    for (const hgx_bgzf_block &b : blocks) { snprintf(buf, sizeof buf, "%zu %zu %08x\n", b.out_off, b.out_len, b.crc); t += buf; }
    std::vector<unsigned char> text;
    const bool ok = inflate_table(data, n, blocks, total, text);
    printf("  %s blocks=%zu table=%08x inflates=%d bytes=%08x\n", who, blocks.size(), crc_of(t.data(), t.size()), ok ? 1 : 0, crc_of(text.data(), text.size()));
}

void print_deferred(const char *who, const hgx_bam_deferred &d) {
    printf("%s on=%d on_device=%d text=%d filtered=%d body0=%zu regions=%d\n", who, d.on, d.on_device, d.text, d.filtered, d.body0, d.n_regions());
    if (!d.filtered) {
        std::string a;
        for (uint8_t v : d.ref_action) a += (char)('0' + v);
        printf("  keep-all action=%s\n", a.c_str());
    }
    for (int g = 0; g < d.n_regions(); ++g) {
        std::string a;
        for (uint8_t v : d.action_of(g)) a += (char)('0' + v);
        printf("  region %d left0=%lld right0=%lld whole=[%s] name=[%s] action=%s\n", g, (long long)d.left_of(g), (long long)d.right_of(g),
               d.whole_of(g).c_str(), d.name_of(g).c_str(), a.c_str());
    }
}

void print_index_last() {
    int32_t used = 0, why = 0, n_seg = 0;
    int64_t bytes = 0, n_blocks = 0;
    hgx_bam_index_last(&used, &why, &bytes, &n_seg, &n_blocks);
    printf("index used=%d why=%d bytes=%lld segments=%d blocks=%lld\n", used, why, (long long)bytes, n_seg, (long long)n_blocks);
}

struct Range { size_t n, b, e; bool operator<(const Range &o) const { return b != o.b ? b < o.b : e < o.e; } };

void write_file(const std::string &path, const void *p, size_t n) {
    std::ofstream f(path, std::ios::binary);
    f.write((const char *)p, (std::streamsize)n);
}

void run_reader(const Case &c) {
    auto has = [&](const char *k) { return c.count(k) != 0; };
    auto num = [&](const char *k, long d) { return has(k) ? atol(c.at(k).c_str()) : d; };
    hgx_align_lines al;
    std::mutex mu;
    std::vector<Range> ranges;
    std::string events;                              // the callbacks in the order they came
    al.defer_walk = num("walk", 0) != 0;
    al.defer_text = num("text", 0) != 0;
    al.file_order = num("order", 0) != 0;
    al.defer_min_bytes = (size_t)num("min", 0);
    if (num("on_raw", 0))
        al.on_raw = [&](const char *, size_t n, size_t b, size_t e) {
            std::lock_guard<std::mutex> g(mu);
            ranges.push_back(Range{n, b, e});
            if (events.size() < 7 || events.compare(events.size() - 7, 7, " on_raw") != 0) events += " on_raw";
        };
    if (has("inflate"))
        al.inflate_dev = [&](const unsigned char *data, size_t n, const std::vector<hgx_bgzf_block> &blocks, size_t total) {
            std::lock_guard<std::mutex> g(mu);
            events += " inflate_dev";
            printf("cb inflate_dev total=%zu answers=%ld\n", total, num("inflate", 0));
            print_table("inflate_dev", data, n, blocks, total);
            return (int)num("inflate", 0);
        };
    if (has("splice"))
        al.splice_dev = [&](const unsigned char *comp, size_t n, const std::vector<hgx_bgzf_block> &blocks, size_t staged,
                            const std::vector<std::pair<uint64_t, uint64_t>> &parts, size_t total) {
            std::lock_guard<std::mutex> g(mu);
            events += " splice_dev";
            printf("cb splice_dev staged=%zu total=%zu parts=%zu answers=%ld\n", staged, total, parts.size(), num("splice", 0));
            print_table("splice_dev", comp, n, blocks, staged);
            std::vector<unsigned char> text, dense;
            bool ok = inflate_table(comp, n, blocks, staged, text);
            for (const auto &p : parts) {
                printf("  part at=%llu len=%llu\n", (unsigned long long)p.first, (unsigned long long)p.second);
                if (p.first + p.second > staged) ok = false;
                else dense.insert(dense.end(), text.begin() + (long)p.first, text.begin() + (long)(p.first + p.second));
            }
            printf("  dense ok=%d bytes=%zu crc=%08x\n", ok ? 1 : 0, dense.size(), crc_of(dense.data(), dense.size()));
            if (has("dump_parts")) write_file(c.at("dump_parts"), dense.data(), dense.size());
            return (int)num("splice", 0);
        };
    if (num("early", 0)) {
        al.comp_early = [&](const unsigned char *, size_t) { std::lock_guard<std::mutex> g(mu); events += " comp_early"; };
        al.comp_sync = [&]() { std::lock_guard<std::mutex> g(mu); events += " comp_sync"; };
    }
    std::string regions;
    for (const std::string &r : split(has("regions") ? c.at("regions") : "", ';')) regions += (regions.empty() ? "" : "\n") + r;
    { std::lock_guard<std::mutex> g(g_err_mu); g_err.clear(); }
    const int rc = hgx_read_alignment_lines(c.at("path").c_str(), has("regions") ? regions.c_str() : nullptr, (int)num("nt", 1), al, num("keep", 0) != 0);
    events += " return";
    printf("rc=%d err=[%s]\n", rc, rc ? g_err.c_str() : "");
    printf("events=%s\n", events.c_str());
    std::sort(ranges.begin(), ranges.end());
    bool tiles = !ranges.empty();
    size_t at = 0;
    std::string rs;
    for (const Range &r : ranges) {
        tiles = tiles && r.b == at && r.e >= r.b && r.n == ranges[0].n;
        at = r.e;
        rs += " [" + std::to_string(r.b) + "," + std::to_string(r.e) + ")";
    }
    tiles = tiles && at == ranges[0].n;
    printf("cb on_raw calls=%zu n=%zu tiles=%d%s\n", ranges.size(), ranges.empty() ? (size_t)0 : ranges[0].n, tiles ? 1 : 0, rs.c_str());
    print_index_last();
    if (rc) return;
    std::string names;
    for (const std::string &s : al.ref_names) names += (names.empty() ? "" : ",") + s;
    printf("binary=%d ref_names=[%s] raw=%s raw_bytes=%zu raw_crc=%08x chunks=%zu\n", al.binary, names.c_str(), al.raw ? "set" : "null", al.raw_bytes,
           al.raw ? crc_of(al.raw, al.raw_bytes) : 0u, al.chunks.size());
    if (has("dump_raw") && al.raw) write_file(c.at("dump_raw"), al.raw, al.raw_bytes);
    print_deferred("deferred", al.deferred);
    // the line table: every line as "len klen key crc" (a binary record: the bytes of its block_size), all of them in one checksum, the
    // first three and the last shown
    std::string all;
    std::vector<std::string> shown;
    char buf[96];
    for (size_t i = 0; i < al.lines.size(); ++i) {
        const hgx_line &l = al.lines[i];
        snprintf(buf, sizeof buf, "%u %u %016llx %08x\n", l.len, l.klen, (unsigned long long)l.key, crc_of(al.binary ? l.p - 32 : l.p, l.len));
        all += buf;
        if (i < 3 || i + 1 == al.lines.size()) shown.push_back(buf);
    }
    printf("lines n=%zu table=%08x\n", al.lines.size(), crc_of(all.data(), all.size()));
    for (const std::string &s : shown) printf("  %s", s.c_str());
}

void run_tasks(const Case &c) {
    std::vector<std::string> paths, regions;
    for (const std::string &t : split(c.at("tasks"), ',')) {
        const size_t cut = t.find('@');
        paths.push_back(t.substr(0, cut));
        std::string r;
        for (const std::string &x : split(t.substr(cut + 1), ';')) r += (r.empty() ? "" : "\n") + x;
        regions.push_back(r);
    }
    std::vector<const char *> pp, rr;
    for (size_t i = 0; i < paths.size(); ++i) { pp.push_back(paths[i].c_str()); rr.push_back(regions[i].empty() ? nullptr : regions[i].c_str()); }
    std::vector<hgx_bgzf_task> tasks;
    std::mutex mu;
    std::vector<int> told;
    const int rc = hgx_bgzf_tasks_read(tasks, pp.data(), rr.data(), (int)pp.size(), atoi(c.count("nt") ? c.at("nt").c_str() : "2"), nullptr,
                                       [&](int t) { std::lock_guard<std::mutex> g(mu); told.push_back(t); });
    std::sort(told.begin(), told.end());
    std::string ts;
    for (int t : told) ts += " " + std::to_string(t);
    printf("rc=%d on_task=%s\n", rc, ts.c_str());
    print_index_last();
    for (size_t t = 0; t < tasks.size(); ++t) {
        hgx_bgzf_task &T = tasks[t];
        std::string names;
        for (const std::string &s : T.refs) names += (names.empty() ? "" : ",") + s;
        printf("task %zu ok=%d indexed=%d data=%s total=%zu staged=%zu parts=%zu refs=[%s]\n", t, T.ok, T.indexed, T.data ? "set" : "null", T.total, T.staged,
               T.parts.size(), names.c_str());
        for (const auto &p : T.parts) printf("  part at=%llu len=%llu\n", (unsigned long long)p.first, (unsigned long long)p.second);
        if (T.ok) print_table("task", T.data, T.n, T.blocks, T.indexed ? T.staged : T.total);
        else printf("  blocks=%zu\n", T.blocks.size());
        print_deferred("  def", T.def);
        hgx_host_free(T.data);
        T.data = nullptr;
    }
}

}   // namespace

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s manifest\n", argv[0]); return 1; }
    std::ifstream mf(argv[1]);
    if (!mf) { fprintf(stderr, "cannot read %s\n", argv[1]); return 1; }
    for (std::string line; std::getline(mf, line);) {
        if (line.empty() || line[0] == '#') continue;
        Case c;
        for (const std::string &f : split(line, '\t')) {
            const size_t eq = f.find('=');
            if (eq != std::string::npos) c[f.substr(0, eq)] = f.substr(eq + 1);
        }
        printf("== case %s\n", c["case"].c_str());
        if (c.count("grow")) {                       // a big text, made here: <file>:<bytes>
            const std::string g = c["grow"];
            const size_t cut = g.rfind(':');
            std::ifstream src(g.substr(0, cut), std::ios::binary);
            const std::string text((std::istreambuf_iterator<char>(src)), std::istreambuf_iterator<char>());
            const size_t want = (size_t)strtoull(g.c_str() + cut + 1, nullptr, 10);
            std::ofstream f(c["path"], std::ios::binary);
            for (size_t have = 0; have < want && !text.empty(); have += text.size()) f.write(text.data(), (std::streamsize)text.size());
        }
        std::vector<std::pair<std::string, std::string>> sw, env;
        for (const std::string &s : split(c.count("sw") ? c["sw"] : "", ',')) sw.emplace_back(s.substr(0, s.find(':')), s.substr(s.find(':') + 1));
        for (const std::string &s : split(c.count("env") ? c["env"] : "", ',')) env.emplace_back(s.substr(0, s.find(':')), s.substr(s.find(':') + 1));
        for (const auto &s : sw) hgx_test_switch_set(s.first.c_str(), s.second.c_str());
        for (const auto &s : env) setenv(s.first.c_str(), s.second.c_str(), 1);
        if (c.count("tasks")) run_tasks(c);
        else run_reader(c);
        hgx_test_switch_set(nullptr, nullptr);
        for (const auto &s : env) unsetenv(s.first.c_str());
        if (c.count("grow")) unlink(c["path"].c_str());
        fflush(stdout);
    }
    hgx_host_pool_trim();
    return 0;
}

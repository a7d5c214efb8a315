// sas::SaNaive::mems (include/sas.hpp) run on the GPU as a user calls it (std::vector<Seq> in, a
// struct of vectors out) and compared field by field, element for element, with the answers
// recorded in tests/golden/cpp_mems_cases.txt.  tests/golden/make_cpp_mems_cases.py writes that file
// on the CPU from the suite's diagonal-run reference; nothing in it comes from the library.
//
//   test_mems FIXTURE           every run of the fixture, the empty batch and the argument errors
//   test_mems --parse FIXTURE   no GPU: read every record, check the array lengths
//
// Exit status 0 = every check passed.  Built by the Makefile in this directory; run by
// tests/test_cpp_mems.py on the GPU and by tests/test_cpp_mems_host.py (--parse) without one.
#include <cerrno>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <map>
#include <string>
#include <vector>

#include "sas.hpp"

static int failures = 0;
#define EXPECT(cond, ...)                                  \
    do {                                                   \
        if (!(cond)) {                                     \
            failures++;                                    \
            std::fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
            std::fprintf(stderr, __VA_ARGS__);             \
            std::fprintf(stderr, "\n");                    \
        }                                                  \
    } while (0)

using U64s = std::vector<uint64_t>;
using Idx = sas::SaNaive;

struct Fixture {
    std::map<std::string, U64s> rec;
    std::vector<std::string> order;
    const U64s& get(const std::string& name) const {
        static const U64s none;
        const auto it = rec.find(name);
        EXPECT(it != rec.end(), "fixture: no record %s", name.c_str());
        return it == rec.end() ? none : it->second;
    }
};

static bool number(const std::string& tok, uint64_t* v) {
    if (tok.empty() || tok.size() > 19) return false;
    *v = 0;
    for (char c : tok) {
        if (c < '0' || c > '9') return false;
        *v = *v * 10 + (uint64_t)(c - '0');
    }
    return true;
}

// `#` to the end of the line is a comment; a record is `name count` and count unsigned integers
static bool parse(const char* path, Fixture& fx) {
    std::ifstream in(path, std::ios::binary);
    if (!in) {
        std::fprintf(stderr, "cannot open %s\n", path);
        return false;
    }
    const std::string all((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    std::vector<std::string> tok;
    for (size_t i = 0; i < all.size();) {
        const char c = all[i];
        if (c == '#') {
            while (i < all.size() && all[i] != '\n') i++;
        } else if (c == ' ' || c == '\n' || c == '\t' || c == '\r') {
            i++;
        } else {
            size_t j = i;
            while (j < all.size() && !std::strchr(" \n\t\r#", all[j])) j++;
            tok.push_back(all.substr(i, j - i));
            i = j;
        }
    }
    for (size_t i = 0; i < tok.size();) {
        const std::string name = tok[i];
        uint64_t count = 0, v = 0;
        if (number(name, &v) || i + 1 >= tok.size() || !number(tok[i + 1], &count) || count > tok.size() - i - 2 ||
            fx.rec.count(name)) {
            std::fprintf(stderr, "%s: bad record header at token %zu (%s)\n", path, i, name.c_str());
            return false;
        }
        U64s& dst = fx.rec[name];
        fx.order.push_back(name);
        dst.resize(count);
        for (uint64_t j = 0; j < count; j++)
            if (!number(tok[i + 2 + j], &dst[j])) {
                std::fprintf(stderr, "%s: %s entry %llu is no number\n", path, name.c_str(), (unsigned long long)j);
                return false;
            }
        i += 2 + count;
    }
    return true;
}

static std::vector<uint8_t> codes(const Fixture& fx, const std::string& name) {
    std::vector<uint8_t> t;
    for (uint64_t c : fx.get(name)) {
        EXPECT(c <= 3, "%s: code %llu", name.c_str(), (unsigned long long)c);
        t.push_back((uint8_t)c);
    }
    return t;
}

// the runs of the fixture: every record NAME.params names one
static std::vector<std::string> runs_of(const Fixture& fx) {
    std::vector<std::string> runs;
    const std::string tail = ".params";
    for (const std::string& name : fx.order)
        if (name.size() > tail.size() && name.compare(name.size() - tail.size(), tail.size(), tail) == 0)
            runs.push_back(name.substr(0, name.size() - tail.size()));
    return runs;
}

static void shapes(const Fixture& fx) {
    const U64s& qlen = fx.get("qlen");
    uint64_t sum = 0;
    for (uint64_t l : qlen) sum += l;
    EXPECT(sum == fx.get("qbytes").size(), "qlen sums to %llu, qbytes has %zu", (unsigned long long)sum,
           fx.get("qbytes").size());
    const std::vector<std::string> runs = runs_of(fx);
    EXPECT(fx.get("runs").size() == 1 && fx.get("runs")[0] == runs.size() && !runs.empty(), "%zu runs", runs.size());
    EXPECT(fx.get("layout.seg_lo").size() == fx.get("layout.seg_hi").size(), "layout segments");
    for (const std::string& run : runs) {
        EXPECT(fx.get(run + ".params").size() == 4, "%s.params", run.c_str());
        const U64s& off = fx.get(run + ".off");
        EXPECT(off.size() == qlen.size() + 1 && off[0] == 0, "%s.off", run.c_str());
        EXPECT(fx.get(run + ".qflags").size() == qlen.size(), "%s.qflags", run.c_str());
        for (const char* f : {"qpos", "tpos", "len"})
            EXPECT(!off.empty() && fx.get(run + "." + f).size() == off.back(), "%s.%s: %zu entries", run.c_str(), f,
                   fx.get(run + "." + f).size());
    }
}

template <class T>
static void same(const std::string& what, const std::vector<T>& got, const U64s& exp) {
    if (got.size() != exp.size()) {
        EXPECT(false, "%s: %zu entries, expected %zu", what.c_str(), got.size(), exp.size());
        return;
    }
    size_t bad = 0;
    for (size_t i = 0; i < got.size(); i++)
        if ((uint64_t)got[i] != exp[i] && bad++ < 5)
            std::fprintf(stderr, "  %s[%zu] = %llu, expected %llu\n", what.c_str(), i, (unsigned long long)got[i],
                         (unsigned long long)exp[i]);
    EXPECT(bad == 0, "%s: %zu of %zu entries differ", what.c_str(), bad, got.size());
}

static void run(const Fixture& fx) {
    const std::vector<uint8_t> t = codes(fx, "text"), bytes = codes(fx, "qbytes");
    std::vector<sas::Seq> qs;
    size_t at = 0;
    for (uint64_t l : fx.get("qlen")) {
        qs.emplace_back(bytes.data() + at, (size_t)l);
        at += l;
    }
    Idx sa = Idx::build(t);
    EXPECT(sa.n() == t.size(), "n");
    for (const std::string& name : runs_of(fx)) {
        const U64s& p = fx.get(name + ".params");
        if (p.size() != 4) continue;
        if (p[3]) sa.set_layout(fx.get("layout.seq_start"), fx.get("layout.seg_lo"), fx.get("layout.seg_hi"));
        else sa.set_layout({});
        const Idx::Mems r = sa.mems(qs, (uint32_t)p[0], p[1], (uint32_t)p[2]);
        same(name + ".off", r.off, fx.get(name + ".off"));
        same(name + ".qpos", r.qpos, fx.get(name + ".qpos"));
        same(name + ".tpos", r.tpos, fx.get(name + ".tpos"));
        same(name + ".len", r.len, fx.get(name + ".len"));
        same(name + ".qflags", r.qflags, fx.get(name + ".qflags"));
    }
    sa.set_layout({});
    // the empty batch
    const Idx::Mems none = sa.mems({}, 12);
    EXPECT(none.off.size() == 1 && none.off[0] == 0 && none.qpos.empty() && none.tpos.empty() && none.len.empty() &&
               none.qflags.empty(),
           "the empty batch");
    // min_len 0 is refused
    bool threw = false;
    try {
        sa.mems(qs, 0);
    } catch (const std::exception& e) {
        threw = std::strstr(e.what(), "min_len") != nullptr;
    }
    EXPECT(threw, "min_len == 0 must throw and name min_len");
}

int main(int argc, char** argv) {
    const bool parse_only = argc == 3 && std::strcmp(argv[1], "--parse") == 0;
    if (argc != 2 && !parse_only) {
        std::fprintf(stderr, "usage: %s [--parse] FIXTURE\n", argv[0]);
        return 2;
    }
    Fixture fx;
    if (!parse(argv[argc - 1], fx)) return 1;
    shapes(fx);
    if (!failures && !parse_only) {
        try {
            run(fx);
        } catch (const std::exception& e) {
            EXPECT(false, "exception: %s", e.what());
        }
    }
    if (failures) {
        std::fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    std::printf(parse_only ? "mems fixture ok: %zu records\n" : "mems ok: %zu records\n", fx.rec.size());
    return 0;
}

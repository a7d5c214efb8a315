// The batched calls of the C++ host API (include/sas.hpp), run: set_layout / translate, locate,
// match, locate_mismatch, locate_edit, align_edit, map_edit, map_pairs, map_pairs_rescue,
// search_between, cigar and read_fasta_file, each called as a user calls it (std::vector<Seq> in,
// result struct out) and compared field by field, element for element, with the answers recorded in
// tests/golden/cpp_api_cases.txt.  tests/golden/make_cpp_cases.py writes that file on the CPU from
// the suite's numpy references; nothing in it comes from the library.
//
//   test_calls GROUP FIXTURE [DIR]   GROUP: locate match mismatch edit align map pairs rescue
//                                    layout misc (misc writes a small FASTA file into DIR)
//   test_calls --parse FIXTURE       no GPU: read every record, check each group's array lengths
//
// Exit status 0 = every check passed.  Built by the Makefile in this directory; run by
// tests/test_cpp_calls.py on the GPU and by tests/test_cpp_cases_host.py (--parse) without one.
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <map>
#include <stdexcept>
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
using Strs = std::vector<std::string>;

// ---------------------------------------------------------------- the fixture
struct Fixture {
    std::map<std::string, U64s> rec;
    const U64s& get(const std::string& name) const {
        static const U64s none;
        const auto it = rec.find(name);
        EXPECT(it != rec.end(), "fixture: no record %s", name.c_str());
        return it == rec.end() ? none : it->second;
    }
    uint64_t at(const std::string& name, size_t i) const {
        const U64s& v = get(name);
        EXPECT(i < v.size(), "fixture: %s has no entry %zu", name.c_str(), i);
        return i < v.size() ? v[i] : 0;
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
        if (number(name, &v) || i + 1 >= tok.size() || !number(tok[i + 1], &count) || count > tok.size() - i - 2) {
            std::fprintf(stderr, "%s: bad record header at token %zu (%s)\n", path, i, name.c_str());
            return false;
        }
        if (fx.rec.count(name)) {
            std::fprintf(stderr, "%s: record %s twice\n", path, name.c_str());
            return false;
        }
        U64s& dst = fx.rec[name];
        dst.resize(count);
        for (uint64_t j = 0; j < count; j++)
            if (!number(tok[i + 2 + j], &dst[j])) {
                std::fprintf(stderr, "%s: %s entry %llu is no number (%s)\n", path, name.c_str(), (unsigned long long)j,
                             tok[i + 2 + j].c_str());
                return false;
            }
        i += 2 + count;
    }
    return true;
}

// a batch of queries: NAME.qlen and NAME.qbytes (the chars of all queries, one after the other)
struct Batch {
    std::vector<uint8_t> bytes;
    std::vector<sas::Seq> qs;
    Batch() = default;
    Batch(const Batch&) = delete;  // qs points into bytes
    Batch(Batch&&) = default;
};

static Batch batch(const Fixture& fx, const std::string& name) {
    const U64s &len = fx.get(name + ".qlen"), &b = fx.get(name + ".qbytes");
    Batch r;
    uint64_t sum = 0;
    for (uint64_t l : len) sum += l;
    EXPECT(sum == b.size(), "%s: qlen sums to %llu, qbytes has %zu", name.c_str(), (unsigned long long)sum, b.size());
    if (sum != b.size()) return r;
    r.bytes.reserve(b.size() + 1);
    for (uint64_t c : b) {
        EXPECT(c <= 3, "%s.qbytes: code %llu", name.c_str(), (unsigned long long)c);
        r.bytes.push_back((uint8_t)c);
    }
    size_t off = 0;
    for (uint64_t l : len) {
        r.qs.emplace_back(r.bytes.data() + off, (size_t)l);
        off += l;
    }
    return r;
}

static std::vector<uint8_t> text_of(const Fixture& fx, const std::string& name) {
    std::vector<uint8_t> t;
    for (uint64_t c : fx.get(name)) {
        EXPECT(c <= 3, "%s: code %llu", name.c_str(), (unsigned long long)c);
        t.push_back((uint8_t)c);
    }
    return t;
}

// strings are stored as their bytes, byte 10 behind each
static Strs strings(const Fixture& fx, const std::string& name) {
    Strs out;
    std::string cur;
    for (uint64_t c : fx.get(name)) {
        if (c == 10) {
            out.push_back(cur);
            cur.clear();
        } else {
            cur.push_back((char)c);
        }
    }
    EXPECT(cur.empty(), "%s: the last string is not terminated", name.c_str());
    return out;
}

// got == exp, element for element; the first few mismatching indices on failure
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

template <class R>
static void same_cigars(const std::string& what, const R& r, size_t count, const Strs& exp) {
    if (count != exp.size()) {
        EXPECT(false, "%s: %zu alignments, %zu recorded strings", what.c_str(), count, exp.size());
        return;
    }
    size_t bad = 0;
    for (size_t a = 0; a < count; a++) {
        const std::string s = sas::cigar(r, a);
        if (s != exp[a] && bad++ < 5)
            std::fprintf(stderr, "  %s[%zu] = \"%s\", expected \"%s\"\n", what.c_str(), a, s.c_str(), exp[a].c_str());
    }
    EXPECT(bad == 0, "%s: %zu of %zu strings differ", what.c_str(), bad, count);
}

// ---------------------------------------------------------------- array lengths (--parse, and before every run)
static size_t nq_of(const Fixture& fx, const std::string& name) {
    batch(fx, name);
    return fx.get(name + ".qlen").size();
}

static void shape_csr(const Fixture& fx, const std::string& name, size_t nq, const std::vector<const char*>& values) {
    const U64s& off = fx.get(name + ".off");
    EXPECT(off.size() == nq + 1, "%s.off: %zu entries for %zu queries", name.c_str(), off.size(), nq);
    if (off.empty()) return;
    EXPECT(off[0] == 0, "%s.off[0] = %llu", name.c_str(), (unsigned long long)off[0]);
    for (size_t i = 1; i < off.size(); i++) EXPECT(off[i - 1] <= off[i], "%s.off descends at %zu", name.c_str(), i);
    for (const char* v : values)
        EXPECT(fx.get(name + "." + v).size() == off.back(), "%s.%s: %zu entries, off ends at %llu", name.c_str(), v,
               fx.get(name + "." + v).size(), (unsigned long long)off.back());
}

static void shape_per(const Fixture& fx, const std::string& name, size_t count, const std::vector<const char*>& fields) {
    for (const char* f : fields)
        EXPECT(fx.get(name + "." + f).size() == count, "%s.%s: %zu entries, expected %zu", name.c_str(), f,
               fx.get(name + "." + f).size(), count);
}

static void shape_scripts(const Fixture& fx, const std::string& name, size_t count, size_t stride) {
    shape_per(fx, name, count, {"nruns"});
    shape_per(fx, name, count * stride, {"runs"});
    const U64s &nruns = fx.get(name + ".nruns"), &runs = fx.get(name + ".runs");
    const Strs c = strings(fx, name + ".cigar");
    EXPECT(c.size() == count, "%s.cigar: %zu strings, expected %zu", name.c_str(), c.size(), count);
    if (nruns.size() != count || runs.size() != count * stride) return;
    for (size_t a = 0; a < count; a++) {
        EXPECT(nruns[a] <= stride, "%s.nruns[%zu] = %llu > stride", name.c_str(), a, (unsigned long long)nruns[a]);
        for (size_t i = 0; i < stride; i++)
            EXPECT((runs[a * stride + i] != 0) == (i < nruns[a]) && runs[a * stride + i] <= 0xFFFF,
                   "%s.runs: slot %zu of alignment %zu", name.c_str(), i, a);
    }
}

static const std::vector<const char*> kMapFields = {"end", "start", "dist", "strand", "n_best", "n_loci", "qflags"};
static const std::vector<const char*> kPairFields = {"pflags", "n_pairs", "n_best_pairs"};

static void shape_mapped(const Fixture& fx, const std::string& name, size_t nq, size_t stride) {
    shape_per(fx, name, nq, kMapFields);
    shape_scripts(fx, name, nq, stride);
}

static const char* const kMmRuns[] = {"k0", "k2", "k2cap"};
static const char* const kEdRuns[] = {"k1", "k3", "k3cap"};
static const char* const kMapRuns[] = {"both", "fwd"};

static void shape_locate(const Fixture& fx) {
    const size_t nq = nq_of(fx, "locate");
    shape_csr(fx, "locate", nq, {"pos"});
    shape_csr(fx, "locate.capped", nq, {"pos"});
    shape_per(fx, "locate", 1, {"cap"});
    EXPECT(nq_of(fx, "locate.none") > 0, "locate.none is empty");
}

static void shape_match(const Fixture& fx) { shape_per(fx, "match", nq_of(fx, "match"), {"len", "pos", "lo", "hi"}); }

static void shape_mismatch(const Fixture& fx) {
    const size_t nq = nq_of(fx, "mismatch");
    for (const char* run : kMmRuns) {
        const std::string name = std::string("mismatch.") + run;
        shape_per(fx, name, 2, {"params"});
        shape_per(fx, name, nq, {"qflags"});
        shape_csr(fx, name, nq, {"pos", "dist"});
    }
}

static void shape_edit(const Fixture& fx) {
    const size_t nq = nq_of(fx, "edit");
    for (const char* run : kEdRuns) {
        const std::string name = std::string("edit.") + run;
        shape_per(fx, name, 2, {"params"});
        shape_per(fx, name, nq, {"qflags"});
        shape_csr(fx, name, nq, {"end", "dist"});
    }
}

static void shape_align(const Fixture& fx) {
    shape_edit(fx);
    for (const char* run : kEdRuns) {
        const size_t na = fx.get(std::string("edit.") + run + ".end").size();
        const size_t stride = 2 * (size_t)fx.at(std::string("edit.") + run + ".params", 0) + 1;
        shape_per(fx, std::string("align.") + run, na, {"start", "dist"});
        shape_scripts(fx, std::string("align.") + run, na, stride);
    }
    const size_t nq = nq_of(fx, "align.bad");
    shape_per(fx, "align.bad", 1, {"params"});
    shape_csr(fx, "align.bad", nq, {"end", "start", "dist"});
    shape_scripts(fx, "align.bad", fx.get("align.bad.end").size(), 2 * (size_t)fx.at("align.bad.params", 0) + 1);
}

static void shape_map(const Fixture& fx) {
    const size_t nq = nq_of(fx, "map");
    for (const char* run : kMapRuns) {
        const std::string name = std::string("map.") + run;
        shape_per(fx, name, 3, {"params"});
        shape_mapped(fx, name, nq, 2 * (size_t)fx.at(name + ".params", 0) + 1);
    }
}

static void shape_pairs(const Fixture& fx) {
    const size_t nq = nq_of(fx, "pairs");
    EXPECT(nq % 2 == 0, "pairs: an odd number of reads");
    shape_per(fx, "pairs", 4, {"params"});
    const size_t stride = 2 * (size_t)fx.at("pairs.params", 0) + 1;
    shape_mapped(fx, "pairs", nq, stride);
    shape_per(fx, "pairs", nq / 2, kPairFields);
    shape_mapped(fx, "pairs.single", nq, stride);
}

static void shape_rescue(const Fixture& fx) {
    shape_pairs(fx);
    const size_t nq = nq_of(fx, "rescue");
    EXPECT(nq % 2 == 0, "rescue: an odd number of reads");
    shape_per(fx, "rescue", 6, {"params"});
    shape_mapped(fx, "rescue", nq, 2 * (size_t)fx.at("rescue.params", 1) + 1);
    shape_per(fx, "rescue", nq / 2, kPairFields);
    shape_per(fx, "rescue", nq / 2, {"n_rescue"});
}

static void shape_layout(const Fixture& fx) {
    const size_t n = text_of(fx, "layout.text").size(), nq = nq_of(fx, "layout");
    const U64s& ss = fx.get("layout.seq_start");
    EXPECT(ss.size() >= 2 && ss[0] == 0 && ss.back() == n, "layout.seq_start does not run from 0 to n");
    EXPECT(fx.get("layout.seg_lo").size() == fx.get("layout.seg_hi").size(), "layout.seg_lo / seg_hi differ in length");
    shape_per(fx, "layout.edit", 2, {"params"});
    shape_per(fx, "layout.map", 3, {"params"});
    for (const char* side : {"on", "off"}) {
        const std::string e = std::string("layout.edit.") + side, m = std::string("layout.map.") + side;
        shape_per(fx, e, nq, {"qflags"});
        shape_csr(fx, e, nq, {"end", "dist"});
        shape_mapped(fx, m, nq, 2 * (size_t)fx.at("layout.map.params", 0) + 1);
    }
    const size_t np = fx.get("layout.translate.pos").size();
    shape_per(fx, "layout.translate", np, {"span", "one.seq", "one.off", "spans.seq", "spans.off"});
}

static void shape_misc(const Fixture& fx) {
    const size_t nq = nq_of(fx, "between");
    EXPECT(nq % 2 == 0, "between: an odd number of bounds");
    shape_csr(fx, "between", nq / 2, {"pos"});
}

// ---------------------------------------------------------------- the calls
template <class F>
static bool throws_invalid(F f) {
    try {
        f();
    } catch (const std::invalid_argument&) {
        return true;
    } catch (const std::exception&) {
    }
    return false;
}

template <class F>
static bool panics_with(int code, F f) {
    try {
        f();
    } catch (const sas::Panic& e) {
        return e.code == code;
    } catch (const std::exception&) {
    }
    return false;
}

static void run_locate(const Fixture& fx, const Idx& sa) {
    const Batch b = batch(fx, "locate");
    const Idx::Located all = sa.locate(b.qs);
    same("locate.off", all.off, fx.get("locate.off"));
    same("locate.pos", all.pos, fx.get("locate.pos"));
    const Idx::Located capped = sa.locate(b.qs, fx.at("locate.cap", 0));
    same("locate.capped.off", capped.off, fx.get("locate.capped.off"));
    same("locate.capped.pos", capped.pos, fx.get("locate.capped.pos"));
    const Batch nb = batch(fx, "locate.none");  // the sizing call returns 0: no second call
    const Idx::Located none = sa.locate(nb.qs);
    same("locate.none.off", none.off, U64s(nb.qs.size() + 1, 0));
    EXPECT(none.pos.empty(), "locate.none: %zu positions", none.pos.size());
    const Idx::Located empty = sa.locate({});
    EXPECT(empty.off == U64s{0} && empty.pos.empty(), "locate({}): off has %zu entries, pos %zu", empty.off.size(),
           empty.pos.size());
}

static void run_match(const Fixture& fx, const Idx& sa) {
    const Batch b = batch(fx, "match");
    const Idx::Matched r = sa.match(b.qs);
    same("match.len", r.len, fx.get("match.len"));
    same("match.pos", r.pos, fx.get("match.pos"));
    same("match.lo", r.lo, fx.get("match.lo"));
    same("match.hi", r.hi, fx.get("match.hi"));
    const Idx::Matched p = sa.match(b.qs, false);
    same("match(ranges = false).len", p.len, fx.get("match.len"));
    same("match(ranges = false).pos", p.pos, fx.get("match.pos"));
    EXPECT(p.lo.empty() && p.hi.empty(), "match(ranges = false): lo / hi are not empty");
    for (bool ranges : {true, false}) {
        const Idx::Matched e = sa.match({}, ranges);
        EXPECT(e.len.empty() && e.pos.empty() && e.lo.empty() && e.hi.empty(), "match({}) is not empty");
    }
}

static void run_mismatch(const Fixture& fx, const Idx& sa) {
    const Batch b = batch(fx, "mismatch");
    for (const char* run : kMmRuns) {
        const std::string name = std::string("mismatch.") + run;
        const Idx::Mismatched r = sa.locate_mismatch(b.qs, (uint32_t)fx.at(name + ".params", 0), fx.at(name + ".params", 1));
        same(name + ".off", r.off, fx.get(name + ".off"));
        same(name + ".pos", r.pos, fx.get(name + ".pos"));
        same(name + ".dist", r.dist, fx.get(name + ".dist"));
        same(name + ".qflags", r.qflags, fx.get(name + ".qflags"));
    }
    const Idx::Mismatched e = sa.locate_mismatch({}, 2);
    EXPECT(e.off == U64s{0} && e.pos.empty() && e.dist.empty() && e.qflags.empty(), "locate_mismatch({}) is not empty");
}

static Idx::Edited run_edit_one(const Fixture& fx, const Idx& sa, const Batch& b, const std::string& name) {
    Idx::Edited r = sa.locate_edit(b.qs, (uint32_t)fx.at(name + ".params", 0), fx.at(name + ".params", 1));
    same(name + ".off", r.off, fx.get(name + ".off"));
    same(name + ".end", r.end, fx.get(name + ".end"));
    same(name + ".dist", r.dist, fx.get(name + ".dist"));
    same(name + ".qflags", r.qflags, fx.get(name + ".qflags"));
    return r;
}

static void run_edit(const Fixture& fx, const Idx& sa) {
    const Batch b = batch(fx, "edit");
    for (const char* run : kEdRuns) run_edit_one(fx, sa, b, std::string("edit.") + run);
    const Idx::Edited e = sa.locate_edit({}, 3);
    EXPECT(e.off == U64s{0} && e.end.empty() && e.dist.empty() && e.qflags.empty(), "locate_edit({}) is not empty");
}

static void check_aligned(const Fixture& fx, const std::string& name, const Idx::Aligned& r, size_t k) {
    EXPECT(r.stride == 2 * k + 1, "%s: stride %zu for k = %zu", name.c_str(), r.stride, k);
    same(name + ".start", r.start, fx.get(name + ".start"));
    same(name + ".dist", r.dist, fx.get(name + ".dist"));
    same(name + ".nruns", r.nruns, fx.get(name + ".nruns"));
    same(name + ".runs", r.runs, fx.get(name + ".runs"));  // the unused slots are recorded as 0
    same_cigars(name + ".cigar", r, r.nruns.size(), strings(fx, name + ".cigar"));
}

static void run_align(const Fixture& fx, const Idx& sa) {
    const Batch b = batch(fx, "edit");
    for (const char* run : kEdRuns) {  // as a user does: the ends that locate_edit returned
        const std::string name = std::string("edit.") + run;
        const uint32_t k = (uint32_t)fx.at(name + ".params", 0);
        const Idx::Edited e = run_edit_one(fx, sa, b, name);
        check_aligned(fx, std::string("align.") + run, sa.align_edit(b.qs, k, e), k);
    }
    {  // a hand-made Edited: its second end has no alignment within k
        const Batch q = batch(fx, "align.bad");
        const uint32_t k = (uint32_t)fx.at("align.bad.params", 0);
        Idx::Edited e;
        e.off = fx.get("align.bad.off");
        e.end = fx.get("align.bad.end");
        const Idx::Aligned r = sa.align_edit(q.qs, k, e);
        check_aligned(fx, "align.bad", r, k);
        EXPECT(r.start.size() == 2 && r.start[1] == sa.n() && r.dist[1] == SAS_AL_NONE_DIST && r.nruns[1] == 0,
               "align.bad: the end without an alignment is not the `no alignment` record");
    }
    const Idx::Aligned none = sa.align_edit(b.qs, 2, Idx::Edited{});
    EXPECT(none.start.empty() && none.dist.empty() && none.nruns.empty() && none.runs.empty() && none.stride == 5,
           "align_edit of no end is not empty");
    const Idx::Aligned e = sa.align_edit({}, 2, sa.locate_edit({}, 2));
    EXPECT(e.start.empty() && e.dist.empty() && e.nruns.empty() && e.runs.empty() && e.stride == 5,
           "align_edit({}) is not empty");
}

static void check_mapped(const Fixture& fx, const std::string& name, const Idx::Mapped& r, size_t k) {
    EXPECT(r.stride == 2 * k + 1, "%s: stride %zu for k = %zu", name.c_str(), r.stride, k);
    same(name + ".end", r.end, fx.get(name + ".end"));
    same(name + ".start", r.start, fx.get(name + ".start"));
    same(name + ".dist", r.dist, fx.get(name + ".dist"));
    same(name + ".strand", r.strand, fx.get(name + ".strand"));
    same(name + ".n_best", r.n_best, fx.get(name + ".n_best"));
    same(name + ".n_loci", r.n_loci, fx.get(name + ".n_loci"));
    same(name + ".nruns", r.nruns, fx.get(name + ".nruns"));
    same(name + ".runs", r.runs, fx.get(name + ".runs"));
    same(name + ".qflags", r.qflags, fx.get(name + ".qflags"));
    same_cigars(name + ".cigar", r, r.nruns.size(), strings(fx, name + ".cigar"));
}

static void check_pairs(const Fixture& fx, const std::string& name, const Idx::MappedPairs& r, size_t k) {
    check_mapped(fx, name, r, k);
    same(name + ".pflags", r.pflags, fx.get(name + ".pflags"));
    same(name + ".n_pairs", r.n_pairs, fx.get(name + ".n_pairs"));
    same(name + ".n_best_pairs", r.n_best_pairs, fx.get(name + ".n_best_pairs"));
}

static bool empty_mapped(const Idx::Mapped& r) {
    return r.end.empty() && r.start.empty() && r.dist.empty() && r.strand.empty() && r.nruns.empty() &&
           r.qflags.empty() && r.n_best.empty() && r.n_loci.empty() && r.runs.empty();
}

static void run_map(const Fixture& fx, const Idx& sa) {
    const Batch b = batch(fx, "map");
    for (const char* run : kMapRuns) {
        const std::string name = std::string("map.") + run;
        const uint32_t k = (uint32_t)fx.at(name + ".params", 0);
        check_mapped(fx, name, sa.map_edit(b.qs, k, fx.at(name + ".params", 1), (uint32_t)fx.at(name + ".params", 2)), k);
    }
    // the default strands are both
    check_mapped(fx, "map.both", sa.map_edit(b.qs, (uint32_t)fx.at("map.both.params", 0)), fx.at("map.both.params", 0));
    const Idx::Mapped e = sa.map_edit({}, 3);
    EXPECT(empty_mapped(e) && e.stride == 7, "map_edit({}) is not empty");
    EXPECT(panics_with(EINVAL, [&] { sa.map_edit(b.qs, 3, 0, 0); }), "map_edit with no strand must panic with EINVAL");
}

struct PairParams {
    uint32_t k, min_frag, max_frag;
    uint64_t max_seed_hits;
};

static PairParams pair_params(const Fixture& fx) {
    return {(uint32_t)fx.at("pairs.params", 0), (uint32_t)fx.at("pairs.params", 2), (uint32_t)fx.at("pairs.params", 3),
            fx.at("pairs.params", 1)};
}

static void run_pairs(const Fixture& fx, const Idx& sa) {
    const Batch b = batch(fx, "pairs");
    const PairParams p = pair_params(fx);
    check_pairs(fx, "pairs", sa.map_pairs(b.qs, p.k, p.min_frag, p.max_frag, p.max_seed_hits), p.k);
    // each read alone: what the join moved a mate away from
    check_mapped(fx, "pairs.single", sa.map_edit(b.qs, p.k, p.max_seed_hits), p.k);
    const Idx::MappedPairs e = sa.map_pairs({}, p.k, p.min_frag, p.max_frag);
    EXPECT(empty_mapped(e) && e.pflags.empty() && e.n_pairs.empty() && e.n_best_pairs.empty() && e.stride == 2 * p.k + 1,
           "map_pairs({}) is not empty");
    const std::vector<sas::Seq> odd(b.qs.begin(), b.qs.begin() + 3);
    EXPECT(throws_invalid([&] { sa.map_pairs(odd, p.k, p.min_frag, p.max_frag); }),
           "map_pairs of an odd number of reads must throw std::invalid_argument");
    EXPECT(panics_with(EINVAL, [&] { sa.map_pairs(b.qs, p.k, p.max_frag, p.min_frag); }),
           "map_pairs with min_frag > max_frag must panic with EINVAL");
}

static void run_rescue(const Fixture& fx, const Idx& sa) {
    const Batch b = batch(fx, "rescue");
    const uint32_t k = (uint32_t)fx.at("rescue.params", 0), kr = (uint32_t)fx.at("rescue.params", 1);
    const uint32_t lo = (uint32_t)fx.at("rescue.params", 3), hi = (uint32_t)fx.at("rescue.params", 4);
    const Idx::MappedPairsRescue r = sa.map_pairs_rescue(b.qs, k, kr, lo, hi, fx.at("rescue.params", 5), fx.at("rescue.params", 2));
    check_pairs(fx, "rescue", r, kr);
    same("rescue.n_rescue", r.n_rescue, fx.get("rescue.n_rescue"));
    {  // max_anchors = 0 and k_rescue = k: map_pairs' records of the same reads
        const Batch pb = batch(fx, "pairs");
        const PairParams p = pair_params(fx);
        const Idx::MappedPairsRescue same_as = sa.map_pairs_rescue(pb.qs, p.k, p.k, p.min_frag, p.max_frag, 0, p.max_seed_hits);
        check_pairs(fx, "pairs", same_as, p.k);
        same("pairs: n_rescue without rescue", same_as.n_rescue, U64s(pb.qs.size() / 2, 0));
    }
    const Idx::MappedPairsRescue e = sa.map_pairs_rescue({}, k, kr, lo, hi, 4);
    EXPECT(empty_mapped(e) && e.pflags.empty() && e.n_pairs.empty() && e.n_best_pairs.empty() && e.n_rescue.empty() &&
               e.stride == 2 * kr + 1,
           "map_pairs_rescue({}) is not empty");
    const std::vector<sas::Seq> odd(b.qs.begin(), b.qs.begin() + 1);
    EXPECT(throws_invalid([&] { sa.map_pairs_rescue(odd, k, kr, lo, hi, 4); }),
           "map_pairs_rescue of an odd number of reads must throw std::invalid_argument");
    EXPECT(panics_with(EINVAL, [&] { sa.map_pairs_rescue(b.qs, k, kr, hi, lo, 4); }),
           "map_pairs_rescue with min_frag > max_frag must panic with EINVAL");
    EXPECT(panics_with(EINVAL, [&] { sa.map_pairs_rescue(b.qs, kr, k, lo, hi, 4); }),
           "map_pairs_rescue with k_rescue < k must panic with EINVAL");
}

static void layout_answers(const Fixture& fx, const Idx& sa, const Batch& b, const std::string& side) {
    const std::string e = "layout.edit." + side, m = "layout.map." + side;
    const Idx::Edited r = sa.locate_edit(b.qs, (uint32_t)fx.at("layout.edit.params", 0), fx.at("layout.edit.params", 1));
    same(e + ".off", r.off, fx.get(e + ".off"));
    same(e + ".end", r.end, fx.get(e + ".end"));
    same(e + ".dist", r.dist, fx.get(e + ".dist"));
    same(e + ".qflags", r.qflags, fx.get(e + ".qflags"));
    const uint32_t k = (uint32_t)fx.at("layout.map.params", 0);
    check_mapped(fx, m, sa.map_edit(b.qs, k, fx.at("layout.map.params", 1), (uint32_t)fx.at("layout.map.params", 2)), k);
}

static void run_layout(const Fixture& fx) {
    const std::vector<uint8_t> t = text_of(fx, "layout.text");
    Idx sa = Idx::build(t);
    const Batch b = batch(fx, "layout");
    const U64s &ss = fx.get("layout.seq_start"), &lo = fx.get("layout.seg_lo"), &hi = fx.get("layout.seg_hi");
    const U64s& pos = fx.get("layout.translate.pos");
    std::vector<uint32_t> span;
    for (uint64_t s : fx.get("layout.translate.span")) span.push_back((uint32_t)s);

    layout_answers(fx, sa, b, "off");
    EXPECT(panics_with(EINVAL, [&] { sa.translate(pos); }), "translate without a layout must panic with EINVAL");
    sa.set_layout({});  // clearing an index that has none
    layout_answers(fx, sa, b, "off");

    sa.set_layout(ss, lo, hi);
    layout_answers(fx, sa, b, "on");
    {
        const auto one = sa.translate(pos);
        same("layout.translate.one.seq", one.first, fx.get("layout.translate.one.seq"));
        same("layout.translate.one.off", one.second, fx.get("layout.translate.one.off"));
        const auto sp = sa.translate(pos, span);
        same("layout.translate.spans.seq", sp.first, fx.get("layout.translate.spans.seq"));
        same("layout.translate.spans.off", sp.second, fx.get("layout.translate.spans.off"));
        const auto none = sa.translate({});
        EXPECT(none.first.empty() && none.second.empty(), "translate({}) is not empty");
    }
    // the argument errors that the header promises; a refused call leaves the layout as it was
    EXPECT(throws_invalid([&] { sa.set_layout(ss, lo, U64s(hi.begin(), hi.end() - 1)); }),
           "set_layout with seg_lo / seg_hi of different length must throw std::invalid_argument");
    EXPECT(throws_invalid([&] { sa.set_layout(U64s{0}); }),
           "set_layout with a seq_start of one entry must throw std::invalid_argument");
    EXPECT(throws_invalid([&] { sa.translate(pos, std::vector<uint32_t>(pos.size() + 1, 1)); }),
           "translate with a span of the wrong length must throw std::invalid_argument");
    {
        U64s wrong = ss;
        wrong.back() += 1;  // does not end at n
        EXPECT(panics_with(EINVAL, [&] { sa.set_layout(wrong, lo, hi); }), "set_layout past n must panic with EINVAL");
    }
    layout_answers(fx, sa, b, "on");

    sa.set_layout({});  // cleared: the answers of no layout
    layout_answers(fx, sa, b, "off");
}

static void run_misc(const Fixture& fx, const std::vector<uint8_t>& t, Idx& sa, const char* dir) {
    {  // search_between: three (a, b) pairs, the last with a > b
        const Batch b = batch(fx, "between");
        const U64s &off = fx.get("between.off"), &pos = fx.get("between.pos");
        for (size_t i = 0; i + 1 < b.qs.size() && i / 2 + 1 < off.size(); i += 2) {
            const std::vector<size_t> got = sa.search_between(b.qs[i], b.qs[i + 1]);
            same("between pair " + std::to_string(i / 2), got, U64s(pos.begin() + off[i / 2], pos.begin() + off[i / 2 + 1]));
        }
        EXPECT(off.size() == 4 && off[3] == off[2], "between: the third pair (a > b) must be empty in the fixture");
    }
    if (dir) {  // read_fasta_file: lower case, N, header lines, CRLF, a record over two lines
        const std::string path = std::string(dir) + "/calls.fa";
        {
            std::ofstream f(path, std::ios::binary);
            f << ">one first record\r\nACGTacgt\r\nNNRac\r\n>two\r\n\r\nTTGA\r\n>three empty\r\n";
        }
        const std::vector<uint8_t> expect = {0, 1, 2, 3, 0, 1, 2, 3, 0, 0, 0, 0, 1, 3, 3, 2, 0};
        std::vector<uint8_t> got;
        try {
            got = sas::read_fasta_file(path);
        } catch (const std::exception& e) {
            EXPECT(false, "read_fasta_file: %s", e.what());
        }
        same("read_fasta_file", got, U64s(expect.begin(), expect.end()));
        EXPECT(panics_with(ENOENT, [&] { sas::read_fasta_file(path + ".missing"); }),
               "read_fasta_file of a missing file must panic with ENOENT");
        const std::string blank = std::string(dir) + "/empty.fa";
        { std::ofstream f(blank, std::ios::binary); }
        EXPECT(sas::read_fasta_file(blank).empty(), "read_fasta_file of an empty file is not empty");
    } else {
        EXPECT(false, "misc needs a directory to write its FASTA file into");
    }
    {  // moves: the moved-from index destructs cleanly, the moved-to one answers
        const Batch b = batch(fx, "locate");
        Idx moved(std::move(sa));
        EXPECT(sa.raw() == nullptr && moved.raw() != nullptr && moved.n() == t.size(), "move construction");
        same("locate after move construction", moved.locate(b.qs).pos, fx.get("locate.pos"));
        {
            const std::vector<uint8_t> t2 = text_of(fx, "layout.text");
            Idx other = Idx::build(t2);
            EXPECT(other.n() == t2.size() && t2.size() != t.size(), "an index of the second text");
            other = std::move(moved);  // move assignment: `other` now holds the first text's index
            EXPECT(other.n() == t.size() && other.raw() != nullptr, "move assignment");
            same("locate after move assignment", other.locate(b.qs).pos, fx.get("locate.pos"));
            sa = std::move(other);
        }  // `other` (whatever it holds after the move) is destroyed here
        EXPECT(sa.raw() != nullptr && sa.n() == t.size(), "the index moved back");
        same("locate after moving back", sa.locate(b.qs).pos, fx.get("locate.pos"));
    }
}

// ---------------------------------------------------------------- main
struct Group {
    const char* name;
    void (*shape)(const Fixture&);
};
static const Group kGroups[] = {{"locate", shape_locate}, {"match", shape_match},   {"mismatch", shape_mismatch},
                                {"edit", shape_edit},     {"align", shape_align},   {"map", shape_map},
                                {"pairs", shape_pairs},   {"rescue", shape_rescue}, {"layout", shape_layout},
                                {"misc", shape_misc}};

static int usage() {
    std::fprintf(stderr, "usage: test_calls GROUP FIXTURE [DIR] | test_calls --parse FIXTURE\n  groups:");
    for (const Group& g : kGroups) std::fprintf(stderr, " %s", g.name);
    std::fprintf(stderr, "\n");
    return 2;
}

static int finish(const char* what) {
    if (failures) {
        std::fprintf(stderr, "%s: %d failures\n", what, failures);
        return 1;
    }
    std::printf("%s ok\n", what);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 3) return usage();
    const std::string group = argv[1];
    Fixture fx;
    if (!parse(argv[2], fx)) return 1;
    if (group == "--parse") {
        const size_t n = text_of(fx, "text").size();
        EXPECT(n >= 1000 && n <= 2000, "text: %zu chars", n);
        for (const Group& g : kGroups) g.shape(fx);
        std::printf("%zu records\n", fx.rec.size());
        return finish("parse");
    }
    const Group* g = nullptr;
    for (const Group& x : kGroups)
        if (group == x.name) g = &x;
    if (!g) return usage();
    g->shape(fx);
    if (failures) return finish(g->name);  // a fixture that does not fit together: nothing is run
    try {
        if (group == "layout") {
            run_layout(fx);
            return finish(g->name);
        }
        const std::vector<uint8_t> t = text_of(fx, "text");
        Idx sa = Idx::build(t);
        EXPECT(sa.n() == t.size(), "n");
        if (group == "locate") run_locate(fx, sa);
        if (group == "match") run_match(fx, sa);
        if (group == "mismatch") run_mismatch(fx, sa);
        if (group == "edit") run_edit(fx, sa);
        if (group == "align") run_align(fx, sa);
        if (group == "map") run_map(fx, sa);
        if (group == "pairs") run_pairs(fx, sa);
        if (group == "rescue") run_rescue(fx, sa);
        if (group == "misc") run_misc(fx, t, sa, argc > 3 ? argv[3] : nullptr);
    } catch (const sas::Panic& e) {
        EXPECT(false, "uncaught sas::Panic (code %d): %s", e.code, e.what());
    } catch (const std::exception& e) {
        EXPECT(false, "uncaught exception: %s", e.what());
    }
    return finish(g->name);
}

// CPU check of the sequence layout's host code, built with -fsanitize=address,undefined by
// tests/test_layout_host.py (a program of its own: nothing here is loaded into python):
//   - the bisects of suffix-array-searching_amd/csrc/layout.hpp (the functions the kernels call)
//     against linear scans, over random layouts with empty sequences, adjacent segments, gaps at
//     both ends of a sequence, no segment at all, and every position and end of the text and a
//     few past it;
//   - layout_check (sas_check_layout) on the layouts it must accept and on one violation at a
//     time, the message naming the entry;
//   - fasta_layout_read (sas_read_fasta_layout) on the file given as argv[1], with exact-size
//     buffers (an overrun is the sanitizer's to find), sized by a first call with null arrays;
//     a too small buffer is refused.  Prints the counts for the caller to compare.
// Prints "layout host ok".
#include "../../suffix-array-searching_amd/csrc/layout.hpp"
#include "../../suffix-array-searching_amd/csrc/layout_host.hpp"

#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

typedef std::vector<uint64_t> V;

static uint64_t seg_of_pos_ref(const V& lo, const V& hi, uint64_t p) {
    for (size_t i = 0; i < lo.size(); i++)
        if (lo[i] <= p && p < hi[i]) return i;
    return LAYOUT_NONE;
}
static uint64_t seg_of_end_ref(const V& lo, const V& hi, uint64_t e) {
    for (size_t i = 0; i < lo.size(); i++)
        if (lo[i] < e && e <= hi[i]) return i;
    return LAYOUT_NONE;
}
static uint64_t seq_of_end_ref(const V& st, uint64_t e) {
    const uint64_t nseq = st.size() - 1;
    if (e == 0 || e > st[nseq]) return LAYOUT_NONE;
    uint64_t best = LAYOUT_NONE;
    for (uint64_t i = 0; i <= nseq; i++)
        if (st[i] < e) best = i;
    return best;
}

static int check_bisects(const V& st, const V& lo, const V& hi, const char* what) {
    const LayoutView y{st.data(), st.size() - 1, lo.data(), hi.data(), lo.size()};
    const uint64_t n = st.back();
    for (uint64_t p = 0; p <= n + 3; p++) {
        const uint64_t a = layout_seg_of_pos(y, p), b = layout_seg_of_end(y, p), c = layout_seq_of_end(y, p);
        if (a != seg_of_pos_ref(lo, hi, p) || b != seg_of_end_ref(lo, hi, p) || c != seq_of_end_ref(st, p)) {
            printf("FAIL %s: p = %llu: seg_of_pos %llu, seg_of_end %llu, seq_of_end %llu\n", what,
                   (unsigned long long)p, (unsigned long long)a, (unsigned long long)b, (unsigned long long)c);
            return 1;
        }
        if (c != LAYOUT_NONE && (c >= y.nseq || st[c] == st[c + 1])) {
            printf("FAIL %s: end %llu got the empty or missing sequence %llu\n", what, (unsigned long long)p,
                   (unsigned long long)c);
            return 1;
        }
    }
    std::string err;
    if (layout_check(n, st.data(), st.size() - 1, lo.data(), hi.data(), lo.size(), &err)) {
        printf("FAIL %s: a valid layout is refused: %s\n", what, err.c_str());
        return 1;
    }
    return 0;
}

// a random layout: sequences of 0..len chars, in each a few segments with gaps of 0..g chars
static void random_layout(std::mt19937_64& rng, int nseq, int len, V* st, V* lo, V* hi) {
    st->assign(1, 0);
    lo->clear();
    hi->clear();
    for (int s = 0; s < nseq; s++) {
        const uint64_t a = st->back(), l = rng() % 4 == 0 ? 0 : rng() % (uint64_t)(len + 1), b = a + l;
        uint64_t p = a + (l ? rng() % 3 : 0);
        while (p < b) {
            const uint64_t h = p + 1 + rng() % 9;
            lo->push_back(p);
            hi->push_back(h < b ? h : b);
            p = hi->back() + rng() % 3;  // 0: the next segment is adjacent
        }
        st->push_back(b);
    }
}

static int expect_refused(const char* what, uint64_t n, const V& st, const V& lo, const V& hi, const char* word) {
    std::string err;
    const int rc = layout_check(n, st.data(), st.size() - 1, lo.data(), hi.data(), lo.size(), &err);
    if (rc != EINVAL || err.find(word) == std::string::npos) {
        printf("FAIL %s: rc %d, message '%s' (wanted EINVAL naming '%s')\n", what, rc, err.c_str(), word);
        return 1;
    }
    return 0;
}

static int check_reader(const char* path) {
    std::string err;
    FastaLayoutOut z;
    if (int rc = fasta_layout_read(path, &z, &err)) {
        printf("FAIL reader sizing: %d %s\n", rc, err.c_str());
        return 1;
    }
    std::vector<uint8_t> text(z.len);
    V st(z.nseq + 1), lo(z.nseg), hi(z.nseg);
    std::vector<char> names(z.names_len);
    FastaLayoutOut o;
    o.out = text.data();
    o.cap = text.size();
    o.seq_start = st.data();
    o.seq_cap = st.size();
    o.seg_lo = lo.data();
    o.seg_hi = hi.data();
    o.seg_cap = lo.size();
    o.names = names.data();
    o.names_cap = names.size();
    if (int rc = fasta_layout_read(path, &o, &err)) {
        printf("FAIL reader: %d %s\n", rc, err.c_str());
        return 1;
    }
    if (o.len != z.len || o.nseq != z.nseq || o.nseg != z.nseg || o.names_len != z.names_len) {
        printf("FAIL reader: the sizing call and the filling call disagree\n");
        return 1;
    }
    if (layout_check(o.len, st.data(), o.nseq, lo.data(), hi.data(), o.nseg, &err)) {
        printf("FAIL reader: its own layout is refused: %s\n", err.c_str());
        return 1;
    }
    for (uint64_t i = 0; i < o.nseg; i++)  // maximal runs: a gap between two segments of one sequence
        if (i && hi[i - 1] == lo[i]) {
            const LayoutView y{st.data(), o.nseq, lo.data(), hi.data(), o.nseg};
            if (layout_seq_of_end(y, hi[i - 1]) == layout_seq_of_end(y, lo[i] + 1)) {
                printf("FAIL reader: segments %llu and %llu are one run\n", (unsigned long long)(i - 1),
                       (unsigned long long)i);
                return 1;
            }
        }
    // every buffer one entry short is refused, not overrun
    if (o.len) {
        FastaLayoutOut s = o;
        s.cap = o.len - 1;
        if (fasta_layout_read(path, &s, &err) != ENOMEM) return printf("FAIL reader: short text accepted\n"), 1;
    }
    {
        FastaLayoutOut s = o;
        s.seq_cap = o.nseq;
        if (fasta_layout_read(path, &s, &err) != ENOMEM) return printf("FAIL reader: short seq_start accepted\n"), 1;
    }
    if (o.nseg) {
        FastaLayoutOut s = o;
        s.seg_cap = o.nseg - 1;
        if (fasta_layout_read(path, &s, &err) != ENOMEM) return printf("FAIL reader: short segments accepted\n"), 1;
    }
    if (o.names_len) {
        FastaLayoutOut s = o;
        s.names_cap = o.names_len - 1;
        if (fasta_layout_read(path, &s, &err) != ENOMEM) return printf("FAIL reader: short names accepted\n"), 1;
    }
    printf("reader len %llu nseq %llu nseg %llu names_len %llu\n", (unsigned long long)o.len,
           (unsigned long long)o.nseq, (unsigned long long)o.nseg, (unsigned long long)o.names_len);
    return 0;
}

int main(int argc, char** argv) {
    int bad = 0;
    // hand-made: an empty sequence between two, adjacent segments, a gap at both ends, one char
    bad += check_bisects({0, 10, 10, 25, 25}, {1, 4, 10, 20, 24}, {4, 8, 11, 23, 25}, "hand-made");
    bad += check_bisects({0, 7}, {}, {}, "no segment");
    bad += check_bisects({0, 7}, {0}, {7}, "identity");
    bad += check_bisects({0, 0, 0}, {}, {}, "empty text");
    bad += check_bisects({0, 0, 5, 5}, {0}, {5}, "empty sequences around one");
    std::mt19937_64 rng(20240607);
    long layouts = 0;
    for (int round = 0; round < 400 && !bad; round++) {
        V st, lo, hi;
        random_layout(rng, 1 + (int)(rng() % 12), 1 + (int)(rng() % 40), &st, &lo, &hi);
        bad += check_bisects(st, lo, hi, "random");
        layouts++;
    }
    // one violation at a time (n = 20)
    const V st{0, 10, 20}, lo{2, 12}, hi{8, 18};
    bad += expect_refused("seq_start[0] != 0", 20, {1, 10, 20}, lo, hi, "seq_start[0]");
    bad += expect_refused("last start != n", 20, {0, 10, 19}, lo, hi, "seq_start[2]");
    bad += expect_refused("decreasing starts", 20, {0, 12, 11, 20}, {2}, {8}, "seq_start[2]");
    bad += expect_refused("empty segment", 20, st, {2, 12}, {2, 18}, "segment 0");
    bad += expect_refused("overlapping segments", 20, st, {2, 7}, {8, 9}, "segment 1");
    bad += expect_refused("segment across a start", 20, st, {2, 9}, {8, 11}, "seq_start[1]");
    bad += expect_refused("hi > n", 20, st, lo, {8, 21}, "segment 1");
    bad += expect_refused("no sequence", 0, {0}, {}, {}, "nseq");
    if (argc > 1) bad += check_reader(argv[1]);
    if (bad) return 1;
    printf("layout host ok (%ld random layouts)\n", layouts);
    return 0;
}

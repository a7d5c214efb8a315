// layout_host.hpp -- the host side of the sequence layout, plain C++ with no device call, so
// that tests/cpp/layout_host_check.cpp compiles the very code of the library under the host
// sanitizers: the rules of a layout (sas.h: sas_check_layout) and the FASTA / FASTQ reader that
// produces one (sas_read_fasta_layout).  sas_io.hip wraps both into the C ABI.
#pragma once
#include <errno.h>
#include <stdint.h>

#include <cstdio>
#include <string>
#include <vector>

// 0, or EINVAL with *err naming the entry that breaks a rule of sas.h
static inline int layout_check(uint64_t n, const uint64_t* seq_start, uint64_t nseq, const uint64_t* seg_lo,
                               const uint64_t* seg_hi, uint64_t nseg, std::string* err) {
    const auto fail = [&](const std::string& m) {
        *err = m;
        return EINVAL;
    };
    const auto S = [](uint64_t v) { return std::to_string(v); };
    if (nseq == 0) return fail("nseq is 0: a layout has at least one sequence");
    if (nseq >= 0xFFFFFFFFull) return fail("nseq = " + S(nseq) + " does not fit below SAS_SEQ_NONE (2^32 - 1)");
    if (!seq_start || (nseg && (!seg_lo || !seg_hi))) return fail("null array");
    if (seq_start[0] != 0) return fail("seq_start[0] = " + S(seq_start[0]) + ", not 0");
    for (uint64_t i = 0; i < nseq; i++)
        if (seq_start[i + 1] < seq_start[i])
            return fail("seq_start[" + S(i + 1) + "] = " + S(seq_start[i + 1]) + " is below seq_start[" + S(i) +
                        "] = " + S(seq_start[i]));
    if (seq_start[nseq] != n) return fail("seq_start[" + S(nseq) + "] = " + S(seq_start[nseq]) + ", not n = " + S(n));
    uint64_t q = 0;  // the first start that is above the current segment's lo
    for (uint64_t i = 0; i < nseg; i++) {
        const uint64_t lo = seg_lo[i], hi = seg_hi[i];
        if (lo >= hi) return fail("segment " + S(i) + " = [" + S(lo) + ", " + S(hi) + ") is empty");
        if (hi > n) return fail("segment " + S(i) + " = [" + S(lo) + ", " + S(hi) + ") ends past n = " + S(n));
        if (i && lo < seg_hi[i - 1])
            return fail("segment " + S(i) + " = [" + S(lo) + ", " + S(hi) + ") starts before segment " + S(i - 1) +
                        " ends at " + S(seg_hi[i - 1]));
        while (q <= nseq && seq_start[q] <= lo) q++;
        if (q <= nseq && seq_start[q] < hi)
            return fail("segment " + S(i) + " = [" + S(lo) + ", " + S(hi) + ") crosses seq_start[" + S(q) + "] = " +
                        S(seq_start[q]));
    }
    return 0;
}

struct FastaLayoutOut {  // every array may be null (not written); a count is always set
    uint8_t* out = nullptr;
    uint64_t cap = 0, len = 0;
    uint64_t* seq_start = nullptr;  // nseq + 1 entries
    uint64_t seq_cap = 0, nseq = 0;
    uint64_t* seg_lo = nullptr;
    uint64_t* seg_hi = nullptr;
    uint64_t seg_cap = 0, nseg = 0;
    char* names = nullptr;
    uint64_t names_cap = 0, names_len = 0;
};

// The line state machine of sas_read_fasta (the same text bytes), which also notes where each
// record starts, the first word of its header, and the maximal runs of ACGTacgt inside it.
// 0 or an errno value with *err
static inline int fasta_layout_read(const char* path, FastaLayoutOut* o, std::string* err) {
    const auto fail = [&](int code, const std::string& m) {
        *err = m;
        return code;
    };
    FILE* f = fopen(path, "rb");
    if (!f) return fail(ENOENT, std::string("cannot open ") + path);
    struct Closer { FILE* f; ~Closer() { fclose(f); } } closer{f};
    std::vector<unsigned char> buf(1 << 20);
    size_t got = fread(buf.data(), 1, buf.size(), f);
    if (got >= 2 && buf[0] == 0x1f && buf[1] == 0x8b) return fail(ENOTSUP, "gzip input not supported");
    o->len = o->nseq = o->nseg = o->names_len = 0;
    uint64_t n = 0, nseq = 0, nseg = 0, nl = 0;
    bool in_seg = false;
    uint64_t seg_from = 0;
    const auto put_start = [&](uint64_t slot, uint64_t v) {
        if (!o->seq_start) return true;
        if (slot >= o->seq_cap) return false;
        o->seq_start[slot] = v;
        return true;
    };
    const auto close_seg = [&]() {
        if (!in_seg) return true;
        in_seg = false;
        if (o->seg_lo || o->seg_hi) {
            if (nseg >= o->seg_cap) return false;
            if (o->seg_lo) o->seg_lo[nseg] = seg_from;
            if (o->seg_hi) o->seg_hi[nseg] = n;
        }
        nseg++;
        return true;
    };
    const auto put_name = [&](char c) {
        if (o->names) {
            if (nl >= o->names_cap) return false;
            o->names[nl] = c;
        }
        nl++;
        return true;
    };
    if (got) {
        const bool fastq = buf[0] == '@';
        if (!fastq && buf[0] != '>') return fail(EINVAL, "not a FASTA/FASTQ file");
        bool at_line_start = true, header = false, seq_line = false;
        int fq_line = 0;   // FASTQ: 0 header, 1 seq, 2 plus, 3 qual
        int name = 0;      // in a header line: 0 not yet, 1 the marker seen, 2 in the first word, 3 behind it
        for (;;) {
            for (size_t i = 0; i < got; i++) {
                const unsigned char c = buf[i];
                if (at_line_start) {
                    at_line_start = false;
                    if (fastq) {
                        seq_line = (fq_line == 1);
                        header = (fq_line == 0);
                    } else {
                        header = (c == '>');
                        seq_line = !header;
                    }
                    if (header) {  // a record starts here
                        if (!close_seg()) return fail(ENOMEM, "segment arrays too small");
                        if (!put_start(nseq, n)) return fail(ENOMEM, "seq_start too small");
                        nseq++;
                        name = 0;
                    }
                }
                if (c == '\n') {
                    at_line_start = true;
                    if (fastq) fq_line = (fq_line + 1) & 3;
                    if (header) {
                        if (name != 3 && !put_name('\0')) return fail(ENOMEM, "names buffer too small");
                        name = 3;
                        header = false;
                    }
                    continue;
                }
                if (header) {
                    if (name == 0) {
                        name = 1;  // the '>' or '@' itself
                    } else if (name == 1 || name == 2) {
                        if (c == ' ' || c == '\t' || c == '\r') {
                            if (!put_name('\0')) return fail(ENOMEM, "names buffer too small");
                            name = 3;
                        } else {
                            if (!put_name((char)c)) return fail(ENOMEM, "names buffer too small");
                            name = 2;
                        }
                    }
                    continue;
                }
                if (c == '\r' || !seq_line) continue;
                int code = 0;
                bool base = true;
                switch (c) {
                    case 'A': case 'a': code = 0; break;
                    case 'C': case 'c': code = 1; break;
                    case 'G': case 'g': code = 2; break;
                    case 'T': case 't': code = 3; break;
                    default: base = false;  // a gap char: code 0 in the text, in no segment
                }
                if (base && !in_seg) {
                    in_seg = true;
                    seg_from = n;
                } else if (!base && !close_seg()) {
                    return fail(ENOMEM, "segment arrays too small");
                }
                if (o->out) {
                    if (n >= o->cap) return fail(ENOMEM, "output buffer too small");
                    o->out[n] = (uint8_t)code;
                }
                n++;
            }
            got = fread(buf.data(), 1, buf.size(), f);
            if (got == 0) break;
        }
        // a last header line without a line end still names its record
        if (header && name != 3 && !put_name('\0')) return fail(ENOMEM, "names buffer too small");
    }
    if (!close_seg()) return fail(ENOMEM, "segment arrays too small");
    if (!put_start(nseq, n)) return fail(ENOMEM, "seq_start too small");
    o->len = n;
    o->nseq = nseq;
    o->nseg = nseg;
    o->names_len = nl;
    return 0;
}

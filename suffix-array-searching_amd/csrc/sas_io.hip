// sas_io.hip -- real-data inputs for the lookup path.
//
//   sas_read_fasta  replaces read_fasta_file (sas/util.rs:144-169): every record's
//                   sequence, concatenated; A/C/G/T/a/c/g/t -> 0..3 and EVERY other
//                   byte (N, IUPAC codes, ...) -> 0, exactly like the reference's
//                   zero-initialised `map` (:145-155).  FASTA ('>' headers, multi-line
//                   sequences) and FASTQ (4-line records) as needletail parses them;
//                   gzip input is rejected (ENOTSUP).
//   sas_kmer_keys   replaces the --human key extraction of sst/bin/bench.rs:58-76:
//                   vals[j] = 2-bit packed chars [j, j+k) & (4^k - 1) & i32::MAX,
//                   for j < min(n, limit + k - 1) - (k - 1), then vals[0] = i32::MAX.
//   sas_read_fasta_layout  the same text bytes, and what sas_read_fasta forgets: where each
//                   record starts, its name, and the maximal runs of ACGTacgt (the segments),
//                   as sas_set_layout takes them (layout_host.hpp has the reader and the
//                   rules of a layout, plain host code);
//   sas_check_layout / sas_set_layout / sas_get_layout  the layout as a side table of a built
//                   index: three u64 arrays in one device allocation (layout.hpp);
//   sas_translate   k_translate: text position (and span) -> (sequence id, offset), or
//                   SAS_SEQ_NONE when the interval is not inside one segment.
#include "call_io.hpp"
#include "layout_host.hpp"

#include <algorithm>
#include <cstdio>
#include <vector>

static inline int code_of(unsigned char c) {
    switch (c) {
        case 'A': case 'a': return 0;
        case 'C': case 'c': return 1;
        case 'G': case 'g': return 2;
        case 'T': case 't': return 3;
        default: return 0;  // sas/util.rs:145 map = [0; 256]
    }
}

extern "C" int sas_read_fasta(const char* path, uint8_t* out, uint64_t cap, uint64_t* len) {
    if (!path || !len) SAS_FAIL(EINVAL, "sas_read_fasta: null argument");
    FILE* f = fopen(path, "rb");
    if (!f) SAS_FAIL(ENOENT, std::string("sas_read_fasta: cannot open ") + path);
    struct Closer { FILE* f; ~Closer() { fclose(f); } } closer{f};
    std::vector<unsigned char> buf(1 << 20);
    size_t got = fread(buf.data(), 1, buf.size(), f);
    if (got >= 2 && buf[0] == 0x1f && buf[1] == 0x8b) SAS_FAIL(ENOTSUP, "sas_read_fasta: gzip input not supported");
    if (got == 0) { *len = 0; return 0; }
    const bool fastq = buf[0] == '@';
    if (!fastq && buf[0] != '>') SAS_FAIL(EINVAL, "sas_read_fasta: not a FASTA/FASTQ file");
    uint64_t n = 0;
    // line state machine: FASTA: '>' lines are headers, others sequence;
    // FASTQ: lines cycle header / sequence / '+' / quality.
    bool at_line_start = true, header = false;
    int fq_line = 0;  // FASTQ: 0 header, 1 seq, 2 plus, 3 qual
    bool seq_line = false;
    for (;;) {
        for (size_t i = 0; i < got; i++) {
            unsigned char c = buf[i];
            if (at_line_start) {
                at_line_start = false;
                if (fastq) {
                    seq_line = (fq_line == 1);
                } else {
                    header = (c == '>');
                    seq_line = !header;
                }
            }
            if (c == '\n') {
                at_line_start = true;
                if (fastq) fq_line = (fq_line + 1) & 3;
                continue;
            }
            if (c == '\r' || !seq_line) continue;
            if (out) {
                if (n >= cap) SAS_FAIL(ENOMEM, "sas_read_fasta: output buffer too small");
                out[n] = (uint8_t)code_of(c);
            }
            n++;
        }
        got = fread(buf.data(), 1, buf.size(), f);
        if (got == 0) break;
    }
    *len = n;
    return 0;
}

// ---------------------------------------------------------------- the sequence layout
extern "C" int sas_read_fasta_layout(const char* path, uint8_t* out, uint64_t cap, uint64_t* len, uint64_t* seq_start,
                                     uint64_t seq_cap, uint64_t* nseq, uint64_t* seg_lo, uint64_t* seg_hi,
                                     uint64_t seg_cap, uint64_t* nseg, char* names, uint64_t names_cap,
                                     uint64_t* names_len) {
    if (!path || !len || !nseq || !nseg) SAS_FAIL(EINVAL, "sas_read_fasta_layout: null argument");
    FastaLayoutOut o;
    o.out = out;
    o.cap = cap;
    o.seq_start = seq_start;
    o.seq_cap = seq_cap;
    o.seg_lo = seg_lo;
    o.seg_hi = seg_hi;
    o.seg_cap = seg_cap;
    o.names = names;
    o.names_cap = names_cap;
    std::string err;
    const int rc = fasta_layout_read(path, &o, &err);
    if (rc) SAS_FAIL(rc, "sas_read_fasta_layout: " + err);
    *len = o.len;
    *nseq = o.nseq;
    *nseg = o.nseg;
    if (names_len) *names_len = o.names_len;
    return 0;
}

extern "C" int sas_check_layout(uint64_t n, const uint64_t* seq_start, uint64_t nseq, const uint64_t* seg_lo,
                                const uint64_t* seg_hi, uint64_t nseg) {
    std::string err;
    if (layout_check(n, seq_start, nseq, seg_lo, seg_hi, nseg, &err)) SAS_FAIL(EINVAL, "sas_check_layout: " + err);
    return 0;
}

// The layout's three arrays live back to back in one allocation, seq_start (nseq + 1), seg_lo
// (nseg), seg_hi (nseg): sas_set_layout builds the index's view with this, and k_translate the
// view of its LDS copy of the same words
__host__ __device__ static inline LayoutView layout_view_at(const uint64_t* base, uint64_t nseq, uint64_t nseg) {
    return LayoutView{base, nseq, base + nseq + 1, base + nseq + 1 + nseg, nseg};
}
__host__ __device__ static inline uint64_t layout_words(uint64_t nseq, uint64_t nseg) { return nseq + 1 + 2 * nseg; }

extern "C" int sas_set_layout(sas_index* x, const uint64_t* seq_start, uint64_t nseq, const uint64_t* seg_lo,
                              const uint64_t* seg_hi, uint64_t nseg) {
    if (!x) SAS_FAIL(EINVAL, "sas_set_layout: null index");
    DevBuf d;
    std::vector<uint64_t> h;
    LayoutView v{};
    if (nseq) {
        TRY(sas_check_layout(x->n, seq_start, nseq, seg_lo, seg_hi, nseg));
        h.reserve(layout_words(nseq, nseg));
        h.assign(seq_start, seq_start + nseq + 1);
        h.insert(h.end(), seg_lo, seg_lo + nseg);
        h.insert(h.end(), seg_hi, seg_hi + nseg);
    }
    HIP_TRY(hipSetDevice(x->device));
    if (nseq) {
        TRY(d.alloc(h.size() * 8, "sequence layout"));
        HIP_TRY(hipMemcpy(d.p, h.data(), h.size() * 8, hipMemcpyHostToDevice));
        v = layout_view_at(d.as<uint64_t>(), nseq, nseg);
    }
    // nothing that was queued before reads the old arrays once this returns
    HIP_TRY(hipDeviceSynchronize());
    if (x->lay_dev) (void)hipFree(x->lay_dev);
    x->lay_dev = static_cast<uint64_t*>(d.release());
    x->lay = v;
    x->lay_host.swap(h);
    return 0;
}

extern "C" int sas_get_layout(const sas_index* x, uint64_t* nseq, uint64_t* nseg, uint64_t* seq_start,
                              uint64_t* seg_lo, uint64_t* seg_hi) {
    if (!x) SAS_FAIL(EINVAL, "sas_get_layout: null index");
    const uint64_t ns = x->lay.nseq, ng = x->lay.nseg;
    if (nseq) *nseq = ns;
    if (nseg) *nseg = ng;
    if (!ns) return 0;
    const uint64_t* h = x->lay_host.data();
    if (seq_start) std::copy(h, h + ns + 1, seq_start);
    if (seg_lo) std::copy(h + ns + 1, h + ns + 1 + ng, seg_lo);
    if (seg_hi) std::copy(h + ns + 1 + ng, h + ns + 1 + 2 * ng, seg_hi);
    return 0;
}

// sas_translate: one interval per thread, grid-stride.  STAGED: the workgroup copies the three
// arrays into LDS first (TR_LDS_WORDS u64: every human assembly fits) and bisects there;
// otherwise the bisects read global memory.
#define TR_BLOCK 256
#define TR_LDS_WORDS 6144  // 48 KiB
template <bool U32, bool STAGED>
__global__ __launch_bounds__(TR_BLOCK) void k_translate(LayoutView y, const void* __restrict__ pos,
                                                        const uint32_t* __restrict__ span, uint64_t count,
                                                        uint32_t* __restrict__ out_seq, void* __restrict__ out_off) {
    __shared__ uint64_t lds[STAGED ? TR_LDS_WORDS : 1];
    if (STAGED) {
        const uint64_t words = layout_words(y.nseq, y.nseg);
        for (uint64_t i = threadIdx.x; i < words; i += TR_BLOCK) lds[i] = y.seq_start[i];
        __syncthreads();
        y = layout_view_at(lds, y.nseq, y.nseg);
    }
    GRID_STRIDE(i, count) {
        const uint64_t p = U32 ? (uint64_t)static_cast<const uint32_t*>(pos)[i] : static_cast<const uint64_t*>(pos)[i];
        uint64_t sp = span ? span[i] : 1;
        if (sp == 0) sp = 1;
        const uint64_t g = layout_seg_of_pos(y, p);
        uint32_t id = SAS_SEQ_NONE;
        uint64_t off = p;
        if (g != LAYOUT_NONE && sp <= y.seg_hi[g] - p) {  // p < hi: [p, p + sp) ends inside the segment
            const uint64_t s = layout_seq_of_end(y, p + 1);
            id = (uint32_t)s;
            off = p - y.seq_start[s];
        }
        out_seq[i] = id;
        if (U32) static_cast<uint32_t*>(out_off)[i] = (uint32_t)off;
        else static_cast<uint64_t*>(out_off)[i] = off;
    }
}

extern "C" int sas_translate(const sas_index* x, const void* pos, const uint32_t* span_or_null, uint64_t count,
                             uint32_t* out_seq, void* out_off, void* stream, uint32_t flags) {
    if (!x) SAS_FAIL(EINVAL, "sas_translate: null index");
    if (!x->lay.nseq) SAS_FAIL(EINVAL, "sas_translate: the index has no layout (sas_set_layout)");
    if (count && (!pos || !out_seq || !out_off)) SAS_FAIL(EINVAL, "sas_translate: null argument");
    const bool u32 = (flags & SAS_LOCATE_U32) != 0;
    if (u32 && x->n >= (1ull << 32)) SAS_FAIL(EINVAL, "sas_translate: SAS_LOCATE_U32 needs a text of n < 2^32 chars");
    if (count == 0) return 0;
    HIP_TRY(hipSetDevice(x->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t w = u32 ? 4 : 8;
    const bool dev = (flags & SAS_DEVICE_PTRS) != 0;
    DevBuf dpos, dspan;
    HostOutputs ho;
    const void* kpos = pos;
    const uint32_t* kspan = span_or_null;
    uint32_t* kseq = out_seq;
    void* koff = out_off;
    if (!dev) {  // host arrays: copy in, run, copy out (synchronous)
        TRY(host_copy_in(dpos, pos, count * w, "translate positions"));
        kpos = dpos.p;
        if (span_or_null) {
            TRY(host_copy_in(dspan, span_or_null, count * 4, "translate spans"));
            kspan = dspan.as<uint32_t>();
        }
        TRY(ho.twin(out_seq, count * 4, "translate sequence ids", &kseq));
        TRY(ho.twin(out_off, count * w, "translate offsets", &koff));
    }
    const bool staged = layout_words(x->lay.nseq, x->lay.nseg) <= TR_LDS_WORDS;
    const dim3 grid(tile_grid(std::min(grid_for(count, TR_BLOCK), (unsigned)x->num_cus * 8)));
    if (u32) {
        if (staged) hipLaunchKernelGGL((k_translate<true, true>), grid, dim3(TR_BLOCK), 0, st, x->lay, kpos, kspan, count, kseq, koff);
        else hipLaunchKernelGGL((k_translate<true, false>), grid, dim3(TR_BLOCK), 0, st, x->lay, kpos, kspan, count, kseq, koff);
    } else {
        if (staged) hipLaunchKernelGGL((k_translate<false, true>), grid, dim3(TR_BLOCK), 0, st, x->lay, kpos, kspan, count, kseq, koff);
        else hipLaunchKernelGGL((k_translate<false, false>), grid, dim3(TR_BLOCK), 0, st, x->lay, kpos, kspan, count, kseq, koff);
    }
    HIP_TRY(hipGetLastError());
    if (!dev) {
        TRY(ho.copy_back(st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    return 0;
}

__global__ void k_kmer_keys(const uint8_t* __restrict__ text, uint64_t count, uint32_t k, uint32_t* __restrict__ out) {
    for (uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; j < count;
         j += (uint64_t)gridDim.x * blockDim.x) {
        uint32_t dummy = 0;
        uint64_t w = pack_query_word(text + j, k, 0, &dummy);  // chars j..j+k in the top 2k bits
        uint64_t key = w >> (64 - 2 * k);
        out[j] = j == 0 ? 0x7fffffffu : ((uint32_t)key & 0x7fffffffu);
    }
}

extern "C" int sas_kmer_keys(const uint8_t* text, uint64_t n, uint32_t k, uint64_t limit, uint32_t* out,
                             uint64_t* count, uint32_t flags) {
    if (!count || (n && !text)) SAS_FAIL(EINVAL, "sas_kmer_keys: null argument");
    if (k == 0 || k > 16) SAS_FAIL(EINVAL, "sas_kmer_keys: k must be in 1..16 (u32 keys)");
    uint64_t end = n < limit + k - 1 ? n : limit + k - 1;
    uint64_t cnt = end >= k - 1 ? end - (k - 1) : 0;
    *count = cnt;
    if (cnt == 0 || !out) return 0;
    bool dev = flags & SAS_DEVICE_PTRS;
    DevBuf dt, dout;
    const uint8_t* tptr = text;
    uint32_t* optr = out;
    uint64_t tb = cnt + k - 1;
    if (!dev) {
        TRY(dt.alloc(tb + 64, "k-mer text"));  // the packer reads whole words past the end
        HIP_TRY(hipMemcpy(dt.p, text, tb, hipMemcpyHostToDevice));
        tptr = dt.as<uint8_t>();
        TRY(dout.alloc(cnt * 4, "k-mer keys"));
        optr = dout.as<uint32_t>();
    }
    uint64_t blocks = (cnt + 255) / 256;
    if (blocks > 262144) blocks = 262144;
    hipLaunchKernelGGL(k_kmer_keys, dim3((unsigned)blocks), dim3(256), 0, 0, tptr, cnt, k, optr);
    HIP_TRY(hipGetLastError());
    if (!dev) HIP_TRY(hipMemcpy(out, optr, cnt * 4, hipMemcpyDeviceToHost));
    else HIP_TRY(hipDeviceSynchronize());
    return 0;
}

// call_io.hpp -- the scaffolding that every C entry point wraps round its kernels, once each
// (host code only; call_io.hip defines what is not a template and emits no kernel):
//
//   * PoolBuf, pool_scan: stream-ordered scratch from a memory pool (the index's:
//     sas_scratch_pool) and rocPRIM's exclusive scan with its temp buffer from that pool;
//   * QueryArgs: the query argument of a call, ragged or fixed-length, as one value;
//   * host_copy_in, HostQueries, HostOutputs: the host-pointer path of a call, host arrays in,
//     device twins, copy back.  It is synchronous on purpose, plain hipMalloc (DevBuf) and
//     hipMemcpy: the stream-ordered allocator + pageable async copies raced on the null stream;
//   * host_list_total: the step between the two passes of a call that returns per-query lists
//     on host pointers (offsets back, the total reported, ENOSPC);
//   * BadFlag: the per-call invalid-input flag word.
#pragma once
#include "build_util.hpp"

#include <rocprim/device/device_scan.hpp>

#include <algorithm>

struct PoolBuf {  // stream-ordered scratch from the index's pool
    void* p = nullptr;
    hipStream_t st = nullptr;
    ~PoolBuf() { if (p) (void)hipFreeAsync(p, st); }
    template <class T> T* as() { return static_cast<T*>(p); }
    int alloc(hipMemPool_t pool, size_t bytes, hipStream_t s) {
        st = s;
        HIP_TRY(hipMallocFromPoolAsync(&p, bytes ? bytes : 8, pool, s));
        return 0;
    }
};

// out[i] = sum of in[0 .. i) over `count` elements of an iterator of u64 (out may be in)
template <class In>
static int pool_scan(hipMemPool_t pool, hipStream_t st, In in, uint64_t* out, uint64_t count) {
    size_t tbytes = 0;
    HIP_TRY(rocprim::exclusive_scan(nullptr, tbytes, in, out, (uint64_t)0, (size_t)count, rocprim::plus<uint64_t>(),
                                    st));
    PoolBuf tmp;
    TRY(tmp.alloc(pool, tbytes, st));
    HIP_TRY(rocprim::exclusive_scan(tmp.p, tbytes, in, out, (uint64_t)0, (size_t)count, rocprim::plus<uint64_t>(),
                                    st));
    return 0;
}

// The query batch as the seed-and-verify kernels see it (HostQueries::stage hands one out)
struct MmQueries {
    const uint8_t* qbytes;
    const uint64_t* qoff;  // null: fixed-length queries of m chars
    const uint32_t* qlen;
    uint32_t m;
    uint64_t nq;
    __device__ __forceinline__ uint64_t off(uint64_t q) const { return qoff ? qoff[q] : q * (uint64_t)m; }
    __device__ __forceinline__ uint32_t len(uint64_t q) const { return qoff ? qlen[q] : m; }
};

// The query argument as a call's extern "C" wrapper got it: ragged (qoff, qlen) or nq queries of
// m chars each.  The pointers are the caller's, of either kind
struct QueryArgs {
    const uint8_t* qbytes;
    const uint64_t* qoff;
    const uint32_t* qlen;
    uint32_t m;
    bool ragged;
    // no pointer that nq queries need is null
    bool null_ok(uint64_t nq) const { return !nq || (qbytes && (!ragged || (qoff && qlen))); }
    // device pointers: the batch as the kernels see it
    MmQueries device(uint64_t nq) const { return MmQueries{qbytes, ragged ? qoff : nullptr, qlen, m, nq}; }
};

// src[0 .. bytes) of the host in a device buffer of its own (synchronous)
int host_copy_in(DevBuf& d, const void* src, size_t bytes, const std::string& what);

// The host-pointer path's way in: the queries of a call on the device.  The bytes copied are
// those up to the largest qoff + qlen, not their sum: ragged queries may overlap
struct HostQueries {
    DevBuf dq, dqoff, dqlen;
    // Waits for `st`, then copies (synchronous).  label: the call's word in "<label> queries"
    int stage(const char* label, const QueryArgs& q, uint64_t nq, hipStream_t st, MmQueries* Q);
};

// The host-pointer path's way out: the device twins of a call's host outputs.  twin() allocates
// one for a host pointer that is not null and hands out the device pointer (null for null);
// copy_back() queues the copies to the host of every twin made since the last copy_back()
struct HostOutputs {
    static const int MAX = 16;
    DevBuf dev[MAX];
    void* host[MAX];
    size_t bytes[MAX];
    int count = 0, copied = 0;
    int twin_bytes(void* h, size_t nbytes, const char* what, void** d);
    template <class T>
    int twin(T* h, size_t nbytes, const char* what, T** d) {
        void* p = nullptr;
        TRY(twin_bytes(h, nbytes, what, &p));
        *d = static_cast<T*>(p);
        return 0;
    }
    int copy_back(hipStream_t st);
};

// Between the two passes of a host-pointer call that returns per-query lists (sas_locate, and
// seed_list_call's: seed_verify.hpp): copies the twins made so far back, the offsets among them,
// and waits; the total out_off[nq] goes to *total and, where the caller asked, *out_total.  A
// total above the capacity is ENOSPC, "<fn>: <total> <noun>, capacity <capacity> (size <hint>
// from *out_total and call again)", with the offsets and the total written
int host_list_total(HostOutputs& ho, hipStream_t st, const std::string& fn, const char* noun, const char* hint,
                    const uint64_t* out_off, uint64_t nq, uint64_t capacity, uint64_t* out_total, uint64_t* total);

// The invalid-input flag of one call: a 4-byte word of the call's own (plain hipMalloc, not the
// pool) that its kernels OR into, so that concurrent calls on other streams (allowed: the index
// is immutable) never see each other's flags.  A call that reads no flag back leaves it unarmed
// (ptr() is null) and hands its kernels the index's write-only sink instead
struct BadFlag {
    DevBuf d;
    int arm(hipStream_t st);  // allocates the word and clears it on the stream
    uint32_t* ptr() { return d.as<uint32_t>(); }
    int read(hipStream_t st, uint32_t* value);  // queues the copy back and synchronises
};

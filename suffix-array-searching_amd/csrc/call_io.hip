// call_io.hip -- the host-pointer path and the per-call flag word of every call, defined once
// (call_io.hpp declares them).  Host code only.
#include "call_io.hpp"

int host_copy_in(DevBuf& d, const void* src, size_t bytes, const std::string& what) {
    TRY(d.alloc(bytes, what.c_str()));
    if (bytes) HIP_TRY(hipMemcpy(d.p, src, bytes, hipMemcpyHostToDevice));
    return 0;
}

int HostQueries::stage(const char* label, const QueryArgs& q, uint64_t nq, hipStream_t st, MmQueries* Q) {
    const std::string l(label);
    uint64_t span = nq * (uint64_t)q.m;
    if (q.ragged) {
        span = 0;
        for (uint64_t i = 0; i < nq; i++) span = std::max(span, q.qoff[i] + q.qlen[i]);
    }
    TRY(dq.alloc(span + 64, (l + " queries").c_str()));  // the packers read whole words past the end
    HIP_TRY(hipStreamSynchronize(st));
    if (span) HIP_TRY(hipMemcpy(dq.p, q.qbytes, span, hipMemcpyHostToDevice));
    if (q.ragged) {
        TRY(host_copy_in(dqoff, q.qoff, nq * 8, l + " query offsets"));
        TRY(host_copy_in(dqlen, q.qlen, nq * 4, l + " query lengths"));
    }
    *Q = MmQueries{dq.as<uint8_t>(), q.ragged ? dqoff.as<uint64_t>() : nullptr, dqlen.as<uint32_t>(), q.m, nq};
    return 0;
}

int HostOutputs::twin_bytes(void* h, size_t nbytes, const char* what, void** d) {
    *d = nullptr;
    if (!h) return 0;
    if (count == MAX) SAS_FAIL(EINVAL, std::string("HostOutputs: more than ") + std::to_string(MAX) + " outputs");
    TRY(dev[count].alloc(nbytes, what));
    host[count] = h;
    bytes[count] = nbytes;
    *d = dev[count++].p;
    return 0;
}

int HostOutputs::copy_back(hipStream_t st) {
    for (; copied < count; copied++)
        if (bytes[copied])
            HIP_TRY(hipMemcpyAsync(host[copied], dev[copied].p, bytes[copied], hipMemcpyDeviceToHost, st));
    return 0;
}

int host_list_total(HostOutputs& ho, hipStream_t st, const std::string& fn, const char* noun, const char* hint,
                    const uint64_t* out_off, uint64_t nq, uint64_t capacity, uint64_t* out_total, uint64_t* total) {
    TRY(ho.copy_back(st));
    HIP_TRY(hipStreamSynchronize(st));
    *total = out_off[nq];
    if (out_total) *out_total = *total;
    if (*total > capacity)
        SAS_FAIL(ENOSPC, fn + ": " + std::to_string(*total) + " " + noun + ", capacity " + std::to_string(capacity) +
                             " (size " + hint + " from *out_total and call again)");
    return 0;
}

int BadFlag::arm(hipStream_t st) {
    TRY(d.alloc(4, "invalid-input flag"));
    HIP_TRY(hipMemsetAsync(d.p, 0, 4, st));
    return 0;
}

int BadFlag::read(hipStream_t st, uint32_t* value) {
    HIP_TRY(hipMemcpyAsync(value, d.p, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

// build_util.hpp -- host helpers shared by the index builders (sas_build.hip, the build_*.hip
// units, sas_build40.hip) and the calls: launch sizing, owning device buffers, rocPRIM's
// temp buffer, error plumbing.  The builders' own steps are declared in build_steps.hpp.
#pragma once
#include "common.hpp"

#include <cstdlib>

static inline unsigned grid_for(uint64_t count, unsigned block = 256) {
    uint64_t g = (count + block - 1) / block;
    if (g < 1) g = 1;
    if (g > 262144) g = 262144;  // grid-stride beyond
    return (unsigned)g;
}

// debug: SAS_TILE_GRID=g caps at g workgroups the grid of every output-centric tiled kernel
// (k_locate_fill, k_mm_verify, k_ed_verify, k_al_align, k_map_fill, k_map_select, k_pair_heads,
// k_pair_loci, k_pair_join, k_pair_rescue) and of the grid(count) helpers of their calls, so a small batch takes
// the tile loop that a large one needs: g = 1 hands every tile to one workgroup in turn
// (tests/test_gpu_tiles.py).  Read at every call; it only ever lowers a grid: unset, empty or
// non-positive is no cap.  sas_tile_grid_cap (sas.h) returns the cap in force, 0 for none
static inline uint32_t tile_grid_cap() {
    const char* e = getenv("SAS_TILE_GRID");
    if (!e) return 0;
    const long long v = atoll(e);
    return v <= 0 ? 0u : (v > 0xFFFFFFFFll ? 0xFFFFFFFFu : (uint32_t)v);
}
template <class G>
static inline G tile_grid(G blocks) {
    const uint32_t cap = tile_grid_cap();
    return cap && (uint64_t)cap < (uint64_t)blocks ? (G)cap : blocks;
}

#define GRID_STRIDE(i, count) \
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < (count); i += (uint64_t)gridDim.x * blockDim.x)

struct MaxOp {
    __device__ __host__ uint32_t operator()(uint32_t a, uint32_t b) const { return a > b ? a : b; }
};
struct MaxOp64 {
    __device__ __host__ uint64_t operator()(uint64_t a, uint64_t b) const { return a > b ? a : b; }
};

struct DevBuf {
    void* p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    template <class T> T* as() { return static_cast<T*>(p); }
    int alloc(size_t bytes, const char* what) {
        if (p) { (void)hipFree(p); p = nullptr; }
        hipError_t e = hipMalloc(&p, bytes ? bytes : 1);
        if (e != hipSuccess) {
            p = nullptr;
            sas_set_error(ENOMEM, std::string("hipMalloc(") + what + ", " + std::to_string(bytes) + " B): " +
                                      hipGetErrorString(e));
            return ENOMEM;
        }
        return 0;
    }
    // hipExtMallocWithFlags (e.g. hipDeviceMallocContiguous) when mflags != 0, plain
    // hipMalloc if that fails or mflags == 0
    int alloc_flags(size_t bytes, const char* what, unsigned mflags) {
        if (mflags) {
            if (p) { (void)hipFree(p); p = nullptr; }
            if (hipExtMallocWithFlags(&p, bytes ? bytes : 1, mflags) == hipSuccess) return 0;
            p = nullptr;
            (void)hipGetLastError();
        }
        return alloc(bytes, what);
    }
    void* release() { void* q = p; p = nullptr; return q; }
};

#define TRY(x) do { int rc_ = (x); if (rc_) return rc_; } while (0)

// rocPRIM's two calls: fn(nullptr, size) asks for the temp size, fn(tmp.p, size) does the work.
// `have` is tmp's size so far and only grows, so the calls of a loop share one allocation
template <class Fn>
static int with_temp(DevBuf& tmp, size_t& have, const char* what, Fn fn) {
    size_t need = 0;
    HIP_TRY(fn((void*)nullptr, need));
    if (need > have || !tmp.p) {
        TRY(tmp.alloc(need, what));
        have = need;
    }
    HIP_TRY(fn(tmp.p, need));
    return 0;
}
// a temp buffer of this call's own size, in place of tmp's last one (the u32 SA builder)
template <class Fn>
static int with_temp(DevBuf& tmp, const char* what, Fn fn) {
    size_t none = 0;
    return with_temp(tmp, none, what, fn);
}

// table fills (prefix table, bucket table): a rank fills a key gap of up to PT_SMALL entries
// itself; a longer one goes to a list that whole workgroups fill
#define PT_SMALL 256


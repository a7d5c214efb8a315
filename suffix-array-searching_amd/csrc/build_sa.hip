// build_sa.hip -- the u32 suffix array by prefix doubling (n < 2^32 - 64; sas_build40.hip builds
// the packed 40-bit one): one rocPRIM radix sort of (32-char packed key, position) pairs, then
// doubling rounds over the still-tied groups only (h = 32, 64, ...).
#include "build_util.hpp"
#include "build_steps.hpp"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_select.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

__global__ void k_init_pairs(const uint64_t* __restrict__ tw, uint64_t n, uint64_t* __restrict__ keys,
                             uint32_t* __restrict__ vals) {
    GRID_STRIDE(i, n) {
        keys[i] = text_chars32(tw, i);
        vals[i] = (uint32_t)i;
    }
}

// headpos[k] = k if element k starts a new key group (else 0); group id = max-scan.
__global__ void k_heads(const uint64_t* __restrict__ keys, uint64_t cnt, const uint32_t* __restrict__ pos_of,
                        uint32_t* __restrict__ headpos) {
    GRID_STRIDE(k, cnt) {
        bool h = (k == 0) || keys[k] != keys[k - 1];
        headpos[k] = h ? (pos_of ? pos_of[k] : (uint32_t)k) : 0u;
    }
}

// rank[p] = group id; unresolved flag = element's group has size > 1.
__global__ void k_assign(const uint64_t* __restrict__ keys, uint64_t cnt, const uint32_t* __restrict__ list,
                         const uint32_t* __restrict__ sa, const uint32_t* __restrict__ group,
                         uint32_t* __restrict__ rank, uint8_t* __restrict__ unresolved) {
    GRID_STRIDE(k, cnt) {
        uint32_t r = list ? list[k] : (uint32_t)k;
        rank[sa[r]] = group[k];
        bool h0 = (k == 0) || keys[k] != keys[k - 1];
        bool h1 = (k + 1 == cnt) || keys[k + 1] != keys[k];
        unresolved[k] = !(h0 && h1);
    }
}

// Doubling key for the tied element at rank list[k]: (group of p, order of p + h).
// p + h >= n -> the suffix is shorter than h: value n - p (<= h) sorts it
// before every longer one and by length among the short ones (Rust slice order:
// a proper prefix sorts first); otherwise BIG + rank[p + h] with BIG > h.
__device__ __forceinline__ uint64_t second_key(const uint32_t* __restrict__ rank, uint64_t n, uint64_t p,
                                               uint64_t h, uint64_t big) {
    return (p + h < n) ? (big + rank[p + h]) : (n - p);
}

// n < 2^31: one 64-bit key (group << 32 | second) with BIG = 2^31.
__global__ void k_round_keys(const uint32_t* __restrict__ list, uint64_t cnt, const uint32_t* __restrict__ sa,
                             const uint32_t* __restrict__ rank, uint64_t n, uint64_t h,
                             uint64_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    GRID_STRIDE(k, cnt) {
        uint32_t p = sa[list[k]];
        keys[k] = ((uint64_t)rank[p] << 32) | second_key(rank, n, p, h, 0x80000000ull);
        vals[k] = p;
    }
}

// n >= 2^31: LSD two-pass -- sort by the 33-bit second key (BIG = 2^32), then
// stably by the group id gathered from the positions.
__global__ void k_round_second(const uint32_t* __restrict__ list, uint64_t cnt, const uint32_t* __restrict__ sa,
                               const uint32_t* __restrict__ rank, uint64_t n, uint64_t h,
                               uint64_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    GRID_STRIDE(k, cnt) {
        uint32_t p = sa[list[k]];
        keys[k] = second_key(rank, n, p, h, 0x100000000ull);
        vals[k] = p;
    }
}
__global__ void k_round_group(const uint32_t* __restrict__ vals, uint64_t cnt, const uint32_t* __restrict__ rank,
                              uint64_t* __restrict__ keys) {
    GRID_STRIDE(k, cnt) keys[k] = rank[vals[k]];
}

// Group heads of a sorted round, from the (not yet updated) ranks.
__global__ void k_round_heads(const uint32_t* __restrict__ vals, uint64_t cnt, const uint32_t* __restrict__ rank,
                              uint64_t n, uint64_t h, const uint32_t* __restrict__ list,
                              uint32_t* __restrict__ headpos, uint8_t* __restrict__ head) {
    GRID_STRIDE(k, cnt) {
        bool hd = true;
        if (k > 0) {
            uint32_t p = vals[k], q = vals[k - 1];
            hd = rank[p] != rank[q] || second_key(rank, n, p, h, 0x100000000ull) !=
                                           second_key(rank, n, q, h, 0x100000000ull);
        }
        head[k] = hd;
        headpos[k] = hd ? list[k] : 0u;
    }
}

__global__ void k_round_assign(uint64_t cnt, const uint32_t* __restrict__ list, const uint32_t* __restrict__ sa,
                               const uint32_t* __restrict__ group, const uint8_t* __restrict__ head,
                               uint32_t* __restrict__ rank, uint8_t* __restrict__ unresolved) {
    GRID_STRIDE(k, cnt) {
        rank[sa[list[k]]] = group[k];
        bool h1 = (k + 1 == cnt) || head[k + 1];
        unresolved[k] = !(head[k] && h1);
    }
}

__global__ void k_scatter_sa(const uint32_t* __restrict__ list, uint64_t cnt, const uint32_t* __restrict__ vals,
                             uint32_t* __restrict__ sa) {
    GRID_STRIDE(k, cnt) sa[list[k]] = vals[k];
}

// Prefix doubling on the GPU.  sa_out: device u32[n].
int build_sa_gpu(const uint64_t* tw, uint64_t n, uint32_t* sa_out, uint32_t* rounds_out, bool force_wide) {
    hipStream_t st = 0;
    DevBuf keys_a, keys_b, vals_b, rank, aux, list_a, list_b, flags, tmp, counter;
    TRY(keys_a.alloc(n * 8, "sa keys"));
    TRY(keys_b.alloc(n * 8, "sa keys alt"));
    TRY(vals_b.alloc(n * 4, "sa vals alt"));
    hipLaunchKernelGGL(k_init_pairs, dim3(grid_for(n)), dim3(256), 0, st, tw, n, keys_a.as<uint64_t>(), sa_out);
    HIP_TRY(hipGetLastError());

    // 1) sort all suffixes by their 32-char packed prefix
    rocprim::double_buffer<uint64_t> kdb(keys_a.as<uint64_t>(), keys_b.as<uint64_t>());
    rocprim::double_buffer<uint32_t> vdb(sa_out, vals_b.as<uint32_t>());
    TRY(with_temp(tmp, "radix sort temp", [&](void* t, size_t& sz) {
        return rocprim::radix_sort_pairs(t, sz, kdb, vdb, (size_t)n, 0, 64, st);
    }));
    if (vdb.current() != sa_out)
        HIP_TRY(hipMemcpyAsync(sa_out, vdb.current(), n * 4, hipMemcpyDeviceToDevice, st));
    const uint64_t* skeys = kdb.current();
    tmp.alloc(0, "free");

    // 2) group ids + first unresolved list
    TRY(rank.alloc(n * 4, "rank"));
    TRY(aux.alloc(n * 4, "group"));
    TRY(flags.alloc(n, "flags"));
    TRY(list_a.alloc(n * 4, "tied list"));
    TRY(list_b.alloc(n * 4, "tied list alt"));
    TRY(counter.alloc(16, "counter"));
    hipLaunchKernelGGL(k_heads, dim3(grid_for(n)), dim3(256), 0, st, skeys, n, (const uint32_t*)nullptr,
                       aux.as<uint32_t>());
    TRY(with_temp(tmp, "scan temp", [&](void* t, size_t& sz) {
        return rocprim::inclusive_scan(t, sz, aux.as<uint32_t>(), aux.as<uint32_t>(), (size_t)n, MaxOp(), st);
    }));
    hipLaunchKernelGGL(k_assign, dim3(grid_for(n)), dim3(256), 0, st, skeys, n, (const uint32_t*)nullptr, sa_out,
                       aux.as<uint32_t>(), rank.as<uint32_t>(), flags.as<uint8_t>());
    HIP_TRY(hipGetLastError());
    rocprim::counting_iterator<uint32_t> cit(0);
    TRY(with_temp(tmp, "select temp", [&](void* t, size_t& sz) {
        return rocprim::select(t, sz, cit, flags.as<uint8_t>(), list_a.as<uint32_t>(), counter.as<uint64_t>(),
                               (size_t)n, st);
    }));
    uint64_t cnt = 0;
    HIP_TRY(hipMemcpyAsync(&cnt, counter.p, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));

    // 3) doubling rounds over the tied elements only (keys_a/keys_b, vals_b reused)
    uint32_t rounds = 0;
    uint32_t* list = list_a.as<uint32_t>();
    uint32_t* list_next = list_b.as<uint32_t>();
    const bool wide = force_wide || n >= (1ull << 31);
    DevBuf heads;
    if (cnt) TRY(heads.alloc(n, "round heads"));
    for (uint64_t h = 32; cnt > 0; h *= 2) {
        if (h >= 2 * n + 64) SAS_FAIL(EIO, "sa construction did not converge");
        rounds++;
        uint32_t* rv = vals_b.as<uint32_t>();
        uint32_t* rv2 = aux.as<uint32_t>();
        rocprim::double_buffer<uint64_t> k2(keys_a.as<uint64_t>(), keys_b.as<uint64_t>());
        rocprim::double_buffer<uint32_t> v2(rv, rv2);
        auto sort_round = [&](int bits, const char* what) {
            return with_temp(tmp, what, [&](void* t, size_t& sz) {
                return rocprim::radix_sort_pairs(t, sz, k2, v2, (size_t)cnt, 0, bits, st);
            });
        };
        if (!wide) {
            hipLaunchKernelGGL(k_round_keys, dim3(grid_for(cnt)), dim3(256), 0, st, list, cnt, sa_out,
                               rank.as<uint32_t>(), n, h, k2.current(), rv);
            TRY(sort_round(64, "round sort temp"));
        } else {
            hipLaunchKernelGGL(k_round_second, dim3(grid_for(cnt)), dim3(256), 0, st, list, cnt, sa_out,
                               rank.as<uint32_t>(), n, h, k2.current(), rv);
            TRY(sort_round(33, "round sort temp"));
            hipLaunchKernelGGL(k_round_group, dim3(grid_for(cnt)), dim3(256), 0, st, v2.current(), cnt,
                               rank.as<uint32_t>(), k2.current());
            TRY(sort_round(32, "round sort temp 2"));
        }
        const uint32_t* sv = v2.current();
        uint32_t* gbuf = (sv == rv) ? rv2 : rv;  // the free value buffer holds group ids
        hipLaunchKernelGGL(k_round_heads, dim3(grid_for(cnt)), dim3(256), 0, st, sv, cnt, rank.as<uint32_t>(), n, h,
                           list, gbuf, heads.as<uint8_t>());
        hipLaunchKernelGGL(k_scatter_sa, dim3(grid_for(cnt)), dim3(256), 0, st, list, cnt, sv, sa_out);
        TRY(with_temp(tmp, "round scan temp", [&](void* t, size_t& sz) {
            return rocprim::inclusive_scan(t, sz, gbuf, gbuf, (size_t)cnt, MaxOp(), st);
        }));
        hipLaunchKernelGGL(k_round_assign, dim3(grid_for(cnt)), dim3(256), 0, st, cnt, list, sa_out, gbuf,
                           heads.as<uint8_t>(), rank.as<uint32_t>(), flags.as<uint8_t>());
        HIP_TRY(hipGetLastError());
        TRY(with_temp(tmp, "round select temp", [&](void* t, size_t& sz) {
            return rocprim::select(t, sz, list, flags.as<uint8_t>(), list_next, counter.as<uint64_t>(), (size_t)cnt, st);
        }));
        HIP_TRY(hipMemcpyAsync(&cnt, counter.p, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        uint32_t* t = list; list = list_next; list_next = t;
    }
    *rounds_out = rounds;
    return 0;
}

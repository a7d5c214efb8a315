// build_gen.hip -- the reference's random text and queries: ChaCha8Rng on the device (text bytes,
// or packed text words for sas_build_gen) and on the host (query offsets and lengths).
//
// random_string (sas/util.rs:9-15) with ChaCha8Rng::seed_from_u64 (sas/main.rs:38):
// char i = keystream word i >> 30 (rand 0.8.5 UniformInt<u8>, range 4, no rejection).
#include "build_util.hpp"
#include "build_steps.hpp"

#include <cstring>

__device__ __forceinline__ uint32_t rotl32d(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }
#define DQR(a, b, c, d)                    \
    a += b; d ^= a; d = rotl32d(d, 16);   \
    c += d; b ^= c; b = rotl32d(b, 12);   \
    a += b; d ^= a; d = rotl32d(d, 8);    \
    c += d; b ^= c; b = rotl32d(b, 7);

// keystream block `blk`: x[i] = the state after the 8 rounds, s[i] = the input state (the
// output word is x[i] + s[i])
__device__ __forceinline__ void chacha8_block(const ChaKey& key, uint64_t blk, uint32_t (&s)[16], uint32_t (&x)[16]) {
    const uint32_t in[16] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u,
                             key.k[0], key.k[1], key.k[2], key.k[3], key.k[4], key.k[5], key.k[6], key.k[7],
                             (uint32_t)blk, (uint32_t)(blk >> 32), 0u, 0u};
#pragma unroll
    for (int i = 0; i < 16; i++) s[i] = x[i] = in[i];
#pragma unroll
    for (int r = 0; r < 8; r += 2) {
        DQR(x[0], x[4], x[8], x[12]) DQR(x[1], x[5], x[9], x[13])
        DQR(x[2], x[6], x[10], x[14]) DQR(x[3], x[7], x[11], x[15])
        DQR(x[0], x[5], x[10], x[15]) DQR(x[1], x[6], x[11], x[12])
        DQR(x[2], x[7], x[8], x[13]) DQR(x[3], x[4], x[9], x[14])
    }
}

__global__ void k_gen_text(ChaKey key, uint64_t n, uint8_t* __restrict__ out) {
    uint64_t blocks = (n + 15) / 16;
    GRID_STRIDE(blk, blocks) {
        uint32_t s[16], x[16];
        chacha8_block(key, blk, s, x);
        uint64_t base = blk * 16;
        if (base + 16 <= n && (((uintptr_t)(out + base)) & 15) == 0) {
            uint32_t wv[4];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                uint32_t v = 0;
#pragma unroll
                for (int i = 0; i < 4; i++) v |= ((x[4 * q + i] + s[4 * q + i]) >> 30) << (8 * i);
                wv[q] = v;
            }
            *reinterpret_cast<uint4*>(out + base) = make_uint4(wv[0], wv[1], wv[2], wv[3]);
        } else {
            for (int i = 0; i < 16 && base + i < n; i++) out[base + i] = (uint8_t)((x[i] + s[i]) >> 30);
        }
    }
}

// Host ChaCha8Rng (rand_chacha 0.3.1) + rand_core 0.6 seed_from_u64 (PCG32 expansion).
static void h_seed_from_u64(uint64_t state, uint32_t key[8]) {
    const uint64_t MUL = 6364136223846793005ull, INC = 11634580027462260723ull;
    for (int i = 0; i < 8; i++) {
        state = state * MUL + INC;
        uint32_t xs = (uint32_t)(((state >> 18) ^ state) >> 27);
        uint32_t rot = (uint32_t)(state >> 59);
        key[i] = (xs >> rot) | (xs << ((32 - rot) & 31));
    }
}
static inline uint32_t h_rotl(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }
#define HQR(a, b, c, d)                  \
    a += b; d ^= a; d = h_rotl(d, 16);  \
    c += d; b ^= c; b = h_rotl(b, 12);  \
    a += b; d ^= a; d = h_rotl(d, 8);   \
    c += d; b ^= c; b = h_rotl(b, 7);

struct HostRng {
    uint32_t key[8];
    uint64_t blk = UINT64_MAX, pos = 0;
    uint32_t buf[16];
    uint32_t word(uint64_t w) {
        uint64_t b = w >> 4;
        if (b != blk) {
            uint32_t s[16] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u, key[0], key[1], key[2], key[3],
                              key[4], key[5], key[6], key[7], (uint32_t)b, (uint32_t)(b >> 32), 0, 0};
            uint32_t x[16];
            memcpy(x, s, sizeof x);
            for (int r = 0; r < 8; r += 2) {
                HQR(x[0], x[4], x[8], x[12]) HQR(x[1], x[5], x[9], x[13])
                HQR(x[2], x[6], x[10], x[14]) HQR(x[3], x[7], x[11], x[15])
                HQR(x[0], x[5], x[10], x[15]) HQR(x[1], x[6], x[11], x[12])
                HQR(x[2], x[7], x[8], x[13]) HQR(x[3], x[4], x[9], x[14])
            }
            for (int i = 0; i < 16; i++) buf[i] = x[i] + s[i];
            blk = b;
        }
        return buf[w & 15];
    }
    uint64_t next_u64() {  // BlockRng::next_u64: two consecutive words, low first
        uint64_t lo = word(pos), hi = word(pos + 1);
        pos += 2;
        return lo | (hi << 32);
    }
    uint64_t range(uint64_t low, uint64_t high) {  // rand 0.8.5 UniformInt<usize>::sample_single
        uint64_t r = high - low;
        uint64_t zone = (r << __builtin_clzll(r)) - 1;
        for (;;) {
            unsigned __int128 p = (unsigned __int128)next_u64() * r;
            if ((uint64_t)p <= zone) return low + (uint64_t)(p >> 64);
        }
    }
};

extern "C" int sas_gen_text(uint64_t seed, uint64_t n, uint8_t* out, uint32_t flags) {
    if (!out && n) SAS_FAIL(EINVAL, "sas_gen_text: null output");
    if (n == 0) return 0;
    ChaKey key;
    h_seed_from_u64(seed, key.k);
    uint8_t* d = out;
    if (!(flags & SAS_DEVICE_PTRS)) HIP_TRY(hipMalloc(&d, n));
    hipLaunchKernelGGL(k_gen_text, dim3(grid_for((n + 15) / 16)), dim3(256), 0, 0, key, n, d);
    HIP_TRY(hipGetLastError());
    if (!(flags & SAS_DEVICE_PTRS)) {
        HIP_TRY(hipMemcpy(out, d, n, hipMemcpyDeviceToHost));
        HIP_TRY(hipFree(d));
    } else {
        HIP_TRY(hipDeviceSynchronize());
    }
    return 0;
}

extern "C" int sas_gen_queries(uint64_t seed, uint64_t word_pos, uint64_t n, uint64_t nq, uint64_t margin,
                               uint32_t len_lo, uint32_t len_hi, uint64_t* off, uint32_t* len,
                               uint64_t* next_word) {
    if (margin >= n) SAS_FAIL(EINVAL, "sas_gen_queries: margin >= n (gen_range(0..n-margin) is empty)");
    if (len_hi <= len_lo) SAS_FAIL(EINVAL, "sas_gen_queries: empty length range");
    if (nq && (!off || !len)) SAS_FAIL(EINVAL, "sas_gen_queries: null output");
    HostRng r;
    h_seed_from_u64(seed, r.key);
    r.pos = word_pos;
    for (uint64_t k = 0; k < nq; k++) {  // sas/util.rs:20-24
        off[k] = r.range(0, n - margin);
        len[k] = (len_hi == len_lo + 1) ? len_lo : (uint32_t)r.range(len_lo, len_hi);
    }
    if (next_word) *next_word = r.pos;
    return 0;
}

// random_string straight into the index's packed layout (sas_build_gen): text word w holds
// chars [32w, 32w + 32), i.e. keystream blocks 2w and 2w + 1, first char in bits 63..62,
// zero past n (the words k_pack_text would make of k_gen_text's bytes), so a sharded
// rank never holds the n-byte text.
__global__ void k_gen_packed(ChaKey key, uint64_t n, uint64_t* __restrict__ tw, uint64_t words) {
    GRID_STRIDE(w, words) {
        uint64_t v = 0;
        const uint64_t base = w * 32;
        if (base < n) {
#pragma unroll
            for (int h = 0; h < 2; h++) {
                uint32_t s[16], x[16];
                chacha8_block(key, 2 * w + h, s, x);
#pragma unroll
                for (int i = 0; i < 16; i++) {
                    const uint32_t c = 16 * h + i;
                    if (base + c < n) v |= (uint64_t)((x[i] + s[i]) >> 30) << (62 - 2 * c);
                }
            }
        }
        tw[w] = v;
    }
}

void gen_key(uint64_t seed, ChaKey* key) { h_seed_from_u64(seed, key->k); }

int gen_packed_text(const ChaKey& key, uint64_t n, uint64_t* tw, uint64_t words) {
    hipLaunchKernelGGL(k_gen_packed, dim3(grid_for(words)), dim3(256), 0, 0, key, n, tw, words);
    HIP_TRY(hipGetLastError());
    return 0;
}

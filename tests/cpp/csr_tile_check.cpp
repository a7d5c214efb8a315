// CPU check of the tile-owner scalars (suffix-array-searching_amd/csrc/csr_tile.hpp, the functions
// that csr_tile_owners and the locate kernels call): for CSR offset arrays with empty owners at
// the front, in the middle and at the end, a tile inside one owner, slices of exactly SLICE and
// SLICE + 1 owners, a last partial tile and offsets at and beyond 2^32, the owner of every
// element of every tile (of the tiles around every offset, for the arrays of 2^32 elements and
// more) must be the one a linear scan finds.  The tile is walked as the kernel walks it, with
// T = 8 and SLICE = 4 as plain arguments: the owners of its first and last element, the slice
// between them, then per element both the staged bisect (over the clamped u32 slice) and the
// unstaged one (over the u64 offsets); which of the two the kernel would take is counted.
// Prints "csr tile ok".
#include "../../suffix-array-searching_amd/csrc/csr_tile.hpp"

#include <cstdio>
#include <set>
#include <vector>

static const uint32_t T = 8, SLICE = 4;
static long g_elements = 0, g_staged = 0, g_unstaged = 0;
static std::set<uint64_t> g_slices;  // every slice length met

static std::vector<uint64_t> csr(const std::vector<uint64_t>& counts) {
    std::vector<uint64_t> off(counts.size() + 1, 0);
    for (size_t i = 0; i < counts.size(); i++) off[i + 1] = off[i] + counts[i];
    return off;
}

// the reference: the one i with off[i] <= v < off[i + 1]; n for v at or past the total
static uint64_t owner_ref(const std::vector<uint64_t>& off, uint64_t v) {
    const uint64_t n = off.size() - 1;
    for (uint64_t i = 0; i < n; i++)
        if (off[i] <= v && v < off[i + 1]) return i;
    return n;
}

// one tile [t0, min(t0 + T, total)), as csr_tile_owners walks it
static int check_tile(const std::vector<uint64_t>& off, uint64_t t0, const char* what) {
    const uint64_t n = off.size() - 1, total = off[n];
    const uint32_t n_el = (uint32_t)(t0 + T < total ? T : total - t0);
    const uint64_t p0 = csr_owner_of(off.data(), n, t0);
    const uint64_t nps = csr_slice_len(p0, csr_owner_of(off.data(), n, t0 + n_el - 1), n);
    g_slices.insert(nps);
    (nps <= SLICE ? g_staged : g_unstaged) += n_el;
    std::vector<uint32_t> rel(nps);
    for (uint64_t x = 0; x < nps; x++) rel[x] = csr_rel(off[p0 + x], t0, T);
    int bad = 0;
    for (uint32_t e = 0; e < n_el; e++) {
        const uint64_t c = t0 + e, want = owner_ref(off, c);
        const uint64_t s = p0 + csr_bisect_staged(rel.data(), nps, e) - 1;
        const uint64_t u = p0 + csr_bisect_offsets(off.data() + p0, nps, c) - 1;
        const uint64_t o = csr_owner_of(off.data(), n, c);
        g_elements++;
        if (s != want || u != want || o != want || !(off[want] <= c && c < off[want + 1])) {
            std::printf("FAIL %s: tile %llu element %u (slice %llu from owner %llu): staged %llu, unstaged %llu, "
                        "whole array %llu, linear scan %llu\n", what, (unsigned long long)t0, e,
                        (unsigned long long)nps, (unsigned long long)p0, (unsigned long long)s, (unsigned long long)u,
                        (unsigned long long)o, (unsigned long long)want);
            bad++;
        }
    }
    return bad;
}

// v at and past the total, and the element before it
static int check_ends(const std::vector<uint64_t>& off, const char* what) {
    const uint64_t n = off.size() - 1, total = off[n];
    int bad = 0;
    for (uint64_t v : std::vector<uint64_t>{total, total + 1, total + T, total + (1ull << 32), ~0ull})
        if (v >= total && csr_owner_of(off.data(), n, v) != n) {
            std::printf("FAIL %s: v = %llu at or past the total %llu: owner %llu, want %llu\n", what,
                        (unsigned long long)v, (unsigned long long)total,
                        (unsigned long long)csr_owner_of(off.data(), n, v), (unsigned long long)n);
            bad++;
        }
    if (total && csr_owner_of(off.data(), n, total - 1) != owner_ref(off, total - 1)) {
        std::printf("FAIL %s: the last element\n", what);
        bad++;
    }
    return bad;
}

// every tile
static int check_all(const std::vector<uint64_t>& counts, const char* what) {
    const std::vector<uint64_t> off = csr(counts);
    int bad = check_ends(off, what);
    for (uint64_t t0 = 0; t0 < off.back(); t0 += T) bad += check_tile(off, t0, what);
    return bad;
}

// the tiles that hold an offset, their neighbours, the first and the last ones
static int check_around(const std::vector<uint64_t>& counts, const char* what) {
    const std::vector<uint64_t> off = csr(counts);
    const uint64_t total = off.back();
    std::set<uint64_t> tiles = {0, 1, (total - 1) / T, (total - 1) / T - 1, (1ull << 32) / T, (1ull << 32) / T - 1};
    for (uint64_t o : off)
        for (int d = -2; d <= 2; d++)
            if ((int64_t)(o / T) + d >= 0) tiles.insert(o / T + d);
    int bad = check_ends(off, what);
    for (uint64_t t : tiles)
        if (t * T < total) bad += check_tile(off, t * T, what);
    return bad;
}

static int check_rel() {
    const uint64_t P32 = 1ull << 32;
    struct { uint64_t o, t0; uint32_t want; } cases[] = {
        {0, 0, 0}, {5, 0, 5}, {7, 0, 7}, {8, 0, T}, {9, 0, T}, {3, 8, 0}, {8, 8, 0}, {P32 + 3, 0, T},
        {P32, 0, T}, {2 * P32, P32, T}, {P32 + 5, P32 + 1, 4}, {P32 + 1, P32 - 3, 4}, {P32 - 3, P32 + 1, 0},
        {P32 + 8, P32, T}, {~0ull, 0, T}, {~0ull, ~0ull - 3, 3}};
    int bad = 0;
    for (const auto& c : cases)
        if (csr_rel(c.o, c.t0, T) != c.want) {
            std::printf("FAIL clamp: offset %llu relative to tile %llu: %u, want %u\n", (unsigned long long)c.o,
                        (unsigned long long)c.t0, csr_rel(c.o, c.t0, T), c.want);
            bad++;
        }
    return bad;
}

int main() {
    const uint64_t P32 = 1ull << 32;
    int bad = check_rel();
    bad += check_all({0, 0, 3, 0, 0, 5, 1, 0, 0}, "empty owners at the front, the middle and the end; total 9");
    bad += check_all({2, 40, 3}, "tiles inside one owner");
    bad += check_all({40}, "one owner");
    bad += check_all({2, 2, 2, 2, 2, 2, 2, 2}, "slices of SLICE owners");
    g_slices.erase(SLICE + 1);
    bad += check_all({2, 2, 2, 1, 1, 3, 2, 1, 1, 1, 3}, "slices of SLICE + 1 owners");
    if (!g_slices.count(SLICE) || !g_slices.count(SLICE + 1)) {
        std::printf("FAIL: no tile with a slice of exactly SLICE and of SLICE + 1 owners\n");
        bad++;
    }
    bad += check_all({1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1},
                     "a run of empty owners inside a tile; one owner per element");
    bad += check_all({0, 0, 0, 0, 0, 0, 8, 0, 0, 0, 0, 0, 0, 5}, "whole tiles between runs of empties; last tile of 5");
    bad += check_all({1}, "one element");
    bad += check_around({3, P32 - 5, 4, 0, 0, 6, P32, 1, 2}, "owners of 2^32 elements: offsets across 2^32 and 2^33");
    bad += check_around({P32, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 0, 7}, "an offset at 2^32 exactly, then small owners");
    bad += check_around({P32 - 4, 1, 1, 1, 1, 1, 1, 1, 1, 1}, "a tile whose slice crosses 2^32");
    if (g_staged == 0 || g_unstaged == 0) {
        std::printf("FAIL: the cases do not reach both branches (%ld staged, %ld unstaged elements)\n", g_staged,
                    g_unstaged);
        bad++;
    }
    if (bad) {
        std::printf("%d failures in %ld elements\n", bad, g_elements);
        return 1;
    }
    std::printf("csr tile ok: %ld elements, %ld in staged and %ld in unstaged tiles\n", g_elements, g_staged,
                g_unstaged);
    return 0;
}

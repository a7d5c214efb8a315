// CPU check of the bisect step of k_sa_quad_llcp's walk (suffix-array-searching_amd/csrc/
// qllcp_bisect.hpp, the function the kernel calls) at SA sizes around 2^31 and 2^32, where a
// 32-bit l + r wraps.  The uint32_t instance (the kernel's R32 = true) and a plain 64-bit
// restatement of binary_search's loop (sas/sa_search.rs:98-112, with the [L0, U] shortcut) run
// side by side; every probe is answered by a fixed lower bound T.  The mids must be the same
// sequence, the final rank must be T, and the walk must end within 34 steps (a capped loop: a
// wrap that sends l back to the bottom ends the program instead of hanging it).
// Prints "qllcp bisect ok".
#include "../../suffix-array-searching_amd/csrc/qllcp_bisect.hpp"

#include <cstdio>
#include <vector>

static const int STEP_CAP = 34;
static long g_checked = 0, g_wrapping = 0;

// the reference: 64-bit ranks, the sum formed in full
static uint64_t walk_ref(uint64_t n, uint64_t L0, uint64_t U, uint64_t T, std::vector<uint64_t>& mids) {
    uint64_t l = 0, r = n;
    while (l < r) {
        const uint64_t mid = (l + r) >> 1;
        mids.push_back(mid);
        if (mid < L0) l = mid + 1;
        else if (mid >= U) r = mid;
        else if (mid < T) l = mid + 1;  // the probe: SA[mid] < q
        else r = mid;
    }
    return r;
}

// the kernel's loops around qllcp_bisect_step; false: the cap was reached
template <typename rk_t>
static bool walk_step(uint64_t n, uint64_t L0_, uint64_t U_, uint64_t T, std::vector<uint64_t>& mids, uint64_t* rank) {
    const rk_t L0 = (rk_t)L0_, U = (rk_t)U_;
    rk_t l = 0, r = (rk_t)n;
    int steps = 0;
    for (;;) {
        rk_t mid = 0;
        while (l < r) {
            if (++steps > STEP_CAP) return false;
            const bool probe = qllcp_bisect_step<rk_t>(l, r, L0, U, mid);
            mids.push_back(mid);
            if (probe) break;
        }
        if (!(l < r)) break;
        if ((uint64_t)mid < T) l = mid + 1;
        else r = mid;
    }
    *rank = r;
    return true;
}

template <typename rk_t>
static int check(uint64_t n, uint64_t L0, uint64_t U, uint64_t T, const char* what) {
    std::vector<uint64_t> a, b;
    const uint64_t want = walk_ref(n, L0, U, T, a);
    uint64_t got = 0;
    const bool ended = walk_step<rk_t>(n, L0, U, T, b, &got);
    g_checked++;
    for (uint64_t m : a) g_wrapping += 2 * m >= (1ull << 32) ? 1 : 0;  // a mid whose l + r needs 33 bits
    if (want != T || !ended || got != T || a != b || (int)a.size() > STEP_CAP) {
        std::printf("FAIL %s (%d-bit ranks): n=%llu L0=%llu U=%llu T=%llu: ended=%d rank=%llu (reference %llu), "
                    "%zu mids (reference %zu)\n", what, (int)sizeof(rk_t) * 8, (unsigned long long)n,
                    (unsigned long long)L0, (unsigned long long)U, (unsigned long long)T, (int)ended,
                    (unsigned long long)got, (unsigned long long)want, b.size(), a.size());
        for (size_t i = 0; i < a.size() && i < b.size(); i++)
            if (a[i] != b[i]) {
                std::printf("  first differing mid at step %zu: %llu, reference %llu\n", i, (unsigned long long)b[i],
                            (unsigned long long)a[i]);
                break;
            }
        return 1;
    }
    return 0;
}

// every lower bound worth asking in [L0, U]: both edges, their neighbours, the middle
template <typename rk_t>
static int check_interval(uint64_t n, uint64_t L0, uint64_t U, const char* what) {
    int bad = 0;
    std::vector<uint64_t> ts = {L0, L0 + 1, L0 + 2, L0 + (U - L0) / 2, L0 + (U - L0) / 3, U - 2, U - 1, U};
    if (U - L0 <= 200)
        for (uint64_t t = L0; t <= U; t++) ts.push_back(t);
    for (uint64_t t : ts)
        if (t >= L0 && t <= U) bad += check<rk_t>(n, L0, U, t, what);
    return bad;
}

template <typename rk_t>
static int check_size(uint64_t n) {
    int bad = 0;
    const uint64_t P31 = 1ull << 31;
    // [L0, U) at the bottom, in the middle, across 2^31, and in the top 1, 2, 100 and 12345 ranks
    bad += check_interval<rk_t>(n, 0, 1, "bottom 1");
    bad += check_interval<rk_t>(n, 0, 64, "bottom 64");
    bad += check_interval<rk_t>(n, 5, 12345, "bottom");
    bad += check_interval<rk_t>(n, n / 2 - 7, n / 2 + 57, "middle");
    bad += check_interval<rk_t>(n, n / 3, n / 3 + 100000, "middle wide");
    if (n > P31 + 40) {
        bad += check_interval<rk_t>(n, P31 - 40, P31 + 40, "across 2^31");
        bad += check_interval<rk_t>(n, P31 - 1, P31, "up to 2^31");
        bad += check_interval<rk_t>(n, P31, P31 + 1, "from 2^31");
    }
    for (uint64_t top : {1ull, 2ull, 100ull, 12345ull}) {
        bad += check_interval<rk_t>(n, n - top, n, "top ranks, U = sa_n");
        bad += check_interval<rk_t>(n, n - top - 3, n - 3, "top ranks");
        bad += check_interval<rk_t>(n, n - top, n - top, "top ranks, L0 = U");
    }
    bad += check_interval<rk_t>(n, 0, 0, "L0 = U = 0");
    bad += check_interval<rk_t>(n, n / 2, n / 2, "L0 = U in the middle");
    bad += check_interval<rk_t>(n, n, n, "L0 = U = sa_n");
    bad += check_interval<rk_t>(n, 0, n, "no bound at all");
    return bad;
}

static int check_right_bound() {
    int bad = 0;
    const uint64_t ns[] = {(1ull << 31) - 1, 1ull << 31, (1ull << 31) + 12345, (1ull << 32) - 5, (1ull << 32) - 1};
    for (uint64_t n : ns) {
        const uint32_t leaves = (uint32_t)((n + 3) / 4);
        for (uint32_t kU : {0u, 1u, leaves / 2, leaves - 2, leaves - 1})
            for (uint32_t fU = 0; fU <= 4; fU++)
                for (int to_end = 0; to_end < 2; to_end++) {
                    uint64_t want = 4 * (uint64_t)kU + fU;
                    if (to_end || want > n) want = n;
                    const uint64_t g32 = qllcp_right_bound<uint32_t>(kU, fU, to_end != 0, n);
                    const uint64_t g64 = qllcp_right_bound<uint64_t>(kU, fU, to_end != 0, n);
                    if (g32 != want || g64 != want) {
                        std::printf("FAIL right bound: n=%llu kU=%u fU=%u end=%d: %llu / %llu, want %llu\n",
                                    (unsigned long long)n, kU, fU, to_end, (unsigned long long)g32,
                                    (unsigned long long)g64, (unsigned long long)want);
                        bad++;
                    }
                }
    }
    return bad;
}

int main() {
    int bad = 0;
    const uint64_t ns[] = {(1ull << 31) - 1, 1ull << 31, (1ull << 31) + 12345, (1ull << 32) - 5, (1ull << 32) - 1};
    for (uint64_t n : ns) {
        bad += check_size<uint32_t>(n);
        bad += check_size<uint64_t>(n);
    }
    // the kernel's R32 = false instance past 2^32
    bad += check_size<uint64_t>((1ull << 32) + 12345);
    bad += check_size<uint64_t>(1ull << 33);
    bad += check_right_bound();
    if (g_wrapping == 0) {
        std::printf("FAIL: no mid needed a 33-bit sum: the cases do not reach the wrap\n");
        bad++;
    }
    if (bad) {
        std::printf("%d failures in %ld walks\n", bad, g_checked);
        return 1;
    }
    std::printf("qllcp bisect ok: %ld walks, %ld mids whose l + r needs 33 bits\n", g_checked, g_wrapping);
    return 0;
}

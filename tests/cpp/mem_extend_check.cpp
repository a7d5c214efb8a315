// The scalar steps of the maximal-exact-match extension (csrc/mem_extend.hpp), the very functions
// k_mem_verify calls, driven on the CPU beside a char-by-char loop: the first differing char of two
// packed words within a bound (every bound 0..32, a difference at every char, differences behind
// the bound, which must not count, the low and the high bit of a char alone), and whole extensions
// through mem_extend_step at lengths around the word edges, with the text's zero padding behind
// the bound.  Compiled and run by tests/test_mem_extend_host.py.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../suffix-array-searching_amd/csrc/mem_extend.hpp"

static int failures = 0;
#define EXPECT(cond, ...)                                  \
    do {                                                   \
        if (!(cond)) {                                     \
            if (failures++ < 20) {                         \
                std::fprintf(stderr, "FAIL line %d: ", __LINE__); \
                std::fprintf(stderr, __VA_ARGS__);         \
                std::fprintf(stderr, "\n");                \
            }                                              \
        }                                                  \
    } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

// chars -> packed words, 32 a word, the first char in the top bits, zero padded, one spare word
static std::vector<uint64_t> pack(const std::vector<uint8_t>& c) {
    std::vector<uint64_t> w(c.size() / 32 + 2, 0);
    for (size_t i = 0; i < c.size(); i++) w[i >> 5] |= (uint64_t)c[i] << (62 - 2 * (i & 31));
    return w;
}

// 32 chars from char p on (what text_chars32 gives the kernel)
static uint64_t chars32(const std::vector<uint64_t>& w, uint64_t p) {
    const uint32_t s = (uint32_t)(p & 31) << 1;
    const uint64_t a = w[p >> 5], b = w[(p >> 5) + 1];
    return s ? (a << s) | (b >> (64 - s)) : a;
}

static uint32_t char_of(uint64_t w, uint32_t i) { return (uint32_t)(w >> (62 - 2 * i)) & 3u; }

int main() {
    // mem_first_diff against the loop
    for (int round = 0; round < 2000; round++) {
        const uint64_t a = rnd();
        for (uint32_t c = 0; c <= 32; c++) {
            EXPECT(mem_first_diff(a, a, c) == c, "equal words, c = %u", c);
            for (uint32_t at = 0; at < 32; at += (round & 1) ? 1 : 5) {
                for (uint64_t bits = 1; bits <= 3; bits++) {  // the low bit, the high bit, both
                    const uint64_t b = a ^ (bits << (62 - 2 * at)) ^ ((round & 2) && at < 31 ? rnd() >> (2 * at + 2) : 0);
                    uint32_t want = c;
                    for (uint32_t i = 0; i < c; i++)
                        if (char_of(a, i) != char_of(b, i)) {
                            want = i;
                            break;
                        }
                    EXPECT(mem_first_diff(a, b, c) == want, "c = %u, first difference at %u, bits %llu: %u", c, at,
                           (unsigned long long)bits, mem_first_diff(a, b, c));
                }
            }
        }
    }
    // whole extensions: text and query agree for `run` chars from (j, i) on, then differ or end
    const uint32_t runs[] = {0, 1, 5, 31, 32, 33, 63, 64, 65, 95, 96, 97, 200};
    for (uint32_t run : runs)
        for (uint32_t j = 0; j < 70; j += 3)
            for (int ends = 0; ends < 3; ends++) {  // 0: a differing char stops it, 1: the text ends, 2: the query ends
                std::vector<uint8_t> t(j + run + (ends == 1 ? 0 : 40)), q(run + (ends == 2 ? 0 : 40));
                for (auto& c : t) c = (uint8_t)(rnd() & 3);
                for (size_t x = 0; x < q.size(); x++) q[x] = x < run ? t[j + x] : (uint8_t)(rnd() & 3);
                if (ends == 0) q[run] = (uint8_t)((t[j + run] + 1) & 3);
                // all A behind the shorter side: the padding of the other must not extend the match
                if (ends == 1)
                    for (size_t x = run; x < q.size(); x++) q[x] = 0;
                if (ends == 2)
                    for (size_t x = j + run; x < t.size(); x++) t[x] = 0;
                const std::vector<uint64_t> tw = pack(t), qw = pack(q);
                const uint64_t bound = t.size() - j < q.size() ? t.size() - j : q.size();
                uint64_t len = 0;
                bool more = len < bound;
                int steps = 0;
                while (more) {
                    len = mem_extend_step(chars32(tw, j + len), chars32(qw, len), len, bound, &more);
                    steps++;
                }
                EXPECT(len == run, "run %u at j = %u, ends %d: extension gave %llu", run, j, ends,
                       (unsigned long long)len);
                EXPECT(steps <= (int)(run / 32) + 1, "run %u: %d steps", run, steps);
                for (uint64_t p = 0; p < t.size(); p++)
                    if (mem_text_char(tw.data(), p) != t[p]) {
                        EXPECT(false, "mem_text_char at %llu", (unsigned long long)p);
                        break;
                    }
            }
    if (failures) {
        std::fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("mem extend ok\n");
    return 0;
}

// packed12_eq.hpp against field-by-field comparison: the equality test of a 12-bit packed column on its raw dwords.
// A stand-alone host program (built with the sanitizers by tests/test_packed12_eq_host.py).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "packed12_eq.hpp"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {                                          // xorshift64*
    rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
    return (uint32_t)((rng_state * 0x2545F4914F6CDD1Dull) >> 32);
}

static void pack(const uint32_t (&f)[8], uint32_t (&d)[3]) {     // field r = bits [12 r, 12 r + 12) of the 96
    d[0] = d[1] = d[2] = 0;
    for (int r = 0; r < 8; r++)
        for (int b = 0; b < 12; b++)
            if ((f[r] >> b) & 1u) d[(12 * r + b) / 32] |= 1u << ((12 * r + b) % 32);
}

static long checks = 0, failures = 0;

static void check(const uint32_t (&f)[8], uint32_t code, const char *what) {
    uint32_t d[3], pat[3], eq[3], want[3] = { 0, 0, 0 };
    pack(f, d);
    packed12_pattern(code, pat);
    packed12_eq(d, pat, eq);
    bool any = false;
    for (int r = 0; r < 8; r++)
        if (f[r] == code) { want[(12 * r + 11) / 32] |= 1u << ((12 * r + 11) % 32); any = true; }
    checks++;
    if (memcmp(eq, want, sizeof eq) != 0 || packed12_any_eq(d, pat) != any) {
        if (failures++ < 20)
            printf("FAIL %s: code %u fields %u %u %u %u %u %u %u %u: got %08x %08x %08x want %08x %08x %08x\n", what, code, f[0], f[1], f[2], f[3],
                   f[4], f[5], f[6], f[7], eq[0], eq[1], eq[2], want[0], want[1], want[2]);
    }
}

int main() {
    // the pattern is the code in every field
    for (uint32_t code = 0; code < 4096; code++) {
        uint32_t f[8], d[3], pat[3];
        for (int r = 0; r < 8; r++) f[r] = code;
        pack(f, d);
        packed12_pattern(code, pat);
        checks++;
        if (memcmp(d, pat, sizeof d) != 0 && failures++ < 20) printf("FAIL pattern of %u\n", code);
    }
    // all 4096 codes, each against random chunks (some fields forced to the code or to a one-bit neighbour of it)
    for (uint32_t code = 0; code < 4096; code++)
        for (int t = 0; t < 24; t++) {
            uint32_t f[8];
            for (int r = 0; r < 8; r++) {
                const uint32_t k = rnd();
                f[r] = (k >> 12) & 0xFFFu;
                if ((k & 7u) == 0) f[r] = code;
                else if ((k & 7u) == 1) f[r] = code ^ (1u << ((k >> 3) % 12));
            }
            check(f, code, "random");
        }
    const uint32_t codes[] = { 0, 1, 1030, 2047, 2048, 4095, 0x555, 0xAAA };
    for (uint32_t code : codes) {
        for (uint32_t fill : { 0u, 0xFFFu, code ^ 0xFFFu, (code + 1) & 0xFFFu, (code - 1) & 0xFFFu }) {
            uint32_t f[8];
            // the code in each field alone, in adjacent pairs (fields 2 and 5 straddle the dword boundaries), in all
            for (int r = 0; r < 8; r++) {
                for (int q = 0; q < 8; q++) f[q] = fill;
                f[r] = code;
                check(f, code, "alone");
                if (r < 7) { f[r + 1] = code; check(f, code, "pair"); }
            }
            for (int q = 0; q < 8; q++) f[q] = code;
            check(f, code, "all");
            for (int q = 0; q < 8; q++) f[q] = fill;
            check(f, code, "none / fill");
            // every one-bit near-miss of the code in every field: beside the fill, and beside the code in all other fields
            for (int r = 0; r < 8; r++)
                for (int b = 0; b < 12; b++) {
                    for (int q = 0; q < 8; q++) f[q] = fill;
                    f[r] = code ^ (1u << b);
                    check(f, code, "near miss");
                    for (int q = 0; q < 8; q++) f[q] = code;
                    f[r] = code ^ (1u << b);
                    check(f, code, "near miss among matches");
                }
        }
    }
    // codes 0 and 4095 beside all-zero and all-one neighbours
    for (uint32_t code : { 0u, 4095u })
        for (uint32_t other : { 0u, 4095u })
            for (int r = 0; r < 8; r++) {
                uint32_t f[8];
                for (int q = 0; q < 8; q++) f[q] = other;
                f[r] = code;
                check(f, code, "extremes");
                check(f, other, "extremes, the neighbours' code");
            }
    printf("%ld checks, %ld failures\n", checks, failures);
    if (failures) return 1;
    printf("all passed\n");
    return 0;
}

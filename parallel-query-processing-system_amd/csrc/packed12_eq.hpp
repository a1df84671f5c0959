// Equality on a 12-bit packed column without extracting its fields: eight fields = 96 bits = three dwords, tested in
// place.  Plain C++ (host and device), so that a host test can run it against field-by-field comparison.
//
// With pat = the code in all eight fields and t = d ^ pat, a field of t is zero exactly where the row has the code.
// L = 0x7FF in every field: ((t & L) + L) has bit 11 of a field set exactly when the field's low 11 bits are not all
// zero, and the add never carries out of a field (0x7FF + 0x7FF < 0x1000), so ONE 96-bit add serves the two fields
// that straddle a dword.  OR-ing t itself in brings the field's own bit 11; what is then CLEAR at bit 11 is a match.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PQPS_P12_HD __host__ __device__ __forceinline__
#else
#define PQPS_P12_HD inline
#endif

// bit 11 of every field / the 11 bits below it, as the three dwords of a chunk
constexpr uint32_t kP12High[3] = { 0x00800800u, 0x08008008u, 0x80080080u };
constexpr uint32_t kP12Low[3] = { 0xFF7FF7FFu, 0xF7FF7FF7u, 0x7FF7FF7Fu };

// the code (< 4096) in all eight fields
PQPS_P12_HD void packed12_pattern(uint32_t code, uint32_t (&pat)[3]) {
    pat[0] = code | (code << 12) | (code << 24);
    pat[1] = (code >> 8) | (code << 4) | (code << 16) | (code << 28);
    pat[2] = (code >> 4) | (code << 8) | (code << 20);
}

// Marker words of one chunk: bit 12 f + 11 (bit 11 of field f, in the chunk's 96 bits) is set where row f has the code,
// every other bit is zero.
PQPS_P12_HD void packed12_eq(const uint32_t (&d)[3], const uint32_t (&pat)[3], uint32_t (&eq)[3]) {
    const uint32_t t0 = d[0] ^ pat[0], t1 = d[1] ^ pat[1], t2 = d[2] ^ pat[2];
    const uint64_t x = (uint64_t)(t0 & kP12Low[0]) | ((uint64_t)(t1 & kP12Low[1]) << 32);
    const uint64_t s = x + ((uint64_t)kP12Low[0] | ((uint64_t)kP12Low[1] << 32));
    const uint32_t s2 = (t2 & kP12Low[2]) + kP12Low[2] + (s < x ? 1u : 0u);
    eq[0] = ~((uint32_t)s | t0) & kP12High[0];
    eq[1] = ~((uint32_t)(s >> 32) | t1) & kP12High[1];
    eq[2] = ~(s2 | t2) & kP12High[2];
}

// ... and whether any of the chunk's eight rows has it
PQPS_P12_HD bool packed12_any_eq(const uint32_t (&d)[3], const uint32_t (&pat)[3]) {
    uint32_t eq[3];
    packed12_eq(d, pat, eq);
    return (eq[0] | eq[1] | eq[2]) != 0;
}

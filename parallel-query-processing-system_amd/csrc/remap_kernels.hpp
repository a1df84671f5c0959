// remap_kernels.hpp -- dictionary codes through a lookup table: dst[i] = lut[src[i]] (included once by pqps_hip.hip, after
// fused_common.hpp).
//
// No counterpart in the reference.  A batch INSERT merges the batch's dictionary into the table's ONCE on the host; what is
// left for the device is one pass per string column that sends every old code to its position in the union (lut_old), and one
// that translates the batch's own codes (lut_new) -- whatever the number of new strings, where pqps_bump_codes is one pass over
// the column PER new string.  Source and destination widths are 1, 2 or 4 bytes each, the destination never narrower: the same
// kernel widens a column whose dictionary has outgrown its code width.
//
// OWNERSHIP.  A lane owns one CHUNK per trip of a persistent grid: the 16 / SW elements of one 16-byte load (SW = source
// width), which leave as 16, 32 or 64 contiguous, 16-byte aligned bytes of whole dwords (global_store_dwordx4).  Element i is
// read and written by its owner lane only and a chunk is read completely before its first store, so dst == src (equal widths)
// needs no second buffer.
// THE RAGGED END.  The last chunk of a column whose length is no multiple of the chunk is loaded element by element (nothing at
// or past n is read) and stored dword by dword: whole dwords while they lie below n * DW bytes, and the one dword the end cuts
// through blended with what it held (as assign_kernels.hpp blends a lane's own dword) -- no byte at or past n * DW changes.
// LOOKUP FORMS.  REMAP_LDS: every workgroup stages the table into LDS once (up to PQPS_REMAP_LDS_CODES entries = 16 KiB: the
// grid's 8 workgroups per CU fit a CU's 160 KiB); REMAP_GLOBAL: the table is read from memory (a full 2-byte dictionary's
// is 256 KiB: L2).
// A code at or past lut_count never indexes the table: it is stored as 0 and counted -- a popcount-free sum per lane, one DPP
// sum per wave, one 64-bit atomic add per workgroup, as the assign kernels count.  No kernel here waits on another workgroup.
#pragma once

namespace {

constexpr uint32_t kRemapBlock = 256;

struct RemapArgs {
    const char *src;
    char *dst;
    uint64_t n;
    const uint32_t *lut;
    uint32_t lut_count;              // >= 1
    unsigned long long *bad;         // zeroed before the launch; may be nullptr
};

template <int SW, int DW, bool LDS>
__global__ __launch_bounds__(kRemapBlock) void remap_kernel(const RemapArgs a) {
    extern __shared__ uint32_t remap_lds[];                     // LDS form: the table; afterwards (both forms) the waves' bad counts
    constexpr uint32_t E = 16 / SW;                              // elements of a chunk
    constexpr uint32_t W = E * DW / 4;                           // dwords a chunk leaves: 4, 8 or 16
    const uint32_t cnt = a.lut_count;
    if constexpr (LDS) {
        for (uint32_t i = threadIdx.x; i < cnt; i += kRemapBlock) remap_lds[i] = a.lut[i];
        __syncthreads();
    }
    const uint64_t n = a.n, full = n / E, chunks = (n + E - 1) / E;
    uint32_t bad = 0;
    for (uint64_t c = (uint64_t)blockIdx.x * kRemapBlock + threadIdx.x; c < chunks; c += (uint64_t)gridDim.x * kRemapBlock) {
        const bool whole = c < full;
        const uint32_t rem = whole ? E : (uint32_t)(n - c * E);  // valid elements of this chunk
        const char *sp = a.src + c * 16;
        uint32_t v[E];
        if (whole) {
            const uint4 q = ld_x4<true>(sp);
            const uint32_t qq[4] = { q.x, q.y, q.z, q.w };
#pragma unroll
            for (uint32_t i = 0; i < E; i++) {
                if constexpr (SW == 1) v[i] = (qq[i / 4] >> (8 * (i % 4))) & 0xFFu;
                else if constexpr (SW == 2) v[i] = (qq[i / 2] >> (16 * (i % 2))) & 0xFFFFu;
                else v[i] = qq[i];
            }
        } else {
#pragma unroll
            for (uint32_t i = 0; i < E; i++) {
                v[i] = 0;
                if (i < rem) {
                    if constexpr (SW == 1) v[i] = ((const uint8_t *)sp)[i];
                    else if constexpr (SW == 2) v[i] = ((const uint16_t *)sp)[i];
                    else v[i] = ((const uint32_t *)sp)[i];
                }
            }
        }
        uint32_t w[W];
#pragma unroll
        for (uint32_t j = 0; j < W; j++) w[j] = 0;
#pragma unroll
        for (uint32_t i = 0; i < E; i++) {
            const bool in = v[i] < cnt;
            uint32_t o = 0;
            if (in) { if constexpr (LDS) o = remap_lds[v[i]]; else o = a.lut[v[i]]; }
            bad += (!in && i < rem) ? 1u : 0u;
            if constexpr (DW == 1) w[i / 4] |= (o & 0xFFu) << (8 * (i % 4));
            else if constexpr (DW == 2) w[i / 2] |= (o & 0xFFFFu) << (16 * (i % 2));
            else w[i] = o;
        }
        uint32_t *dp = (uint32_t *)(a.dst + c * (uint64_t)(E * DW));
        if (whole) {
#pragma unroll
            for (uint32_t j = 0; j < W; j += 4) *(uint4 *)(dp + j) = make_uint4(w[j], w[j + 1], w[j + 2], w[j + 3]);
        } else {
            const uint32_t vb = rem * DW;                        // valid bytes of the chunk, 1 .. E * DW - 1
#pragma unroll
            for (uint32_t j = 0; j < W; j++) {
                if (j * 4 + 4 <= vb) dp[j] = w[j];
                else if (j * 4 < vb) {                           // the dword the end cuts through (DW 1 and 2 only)
                    const uint32_t k = (1u << (8 * (vb - j * 4))) - 1u;
                    dp[j] = (dp[j] & ~k) | (w[j] & k);
                }
            }
        }
    }
    if (a.bad) {
        const uint32_t wave = wave_sum_u32(bad);
        __syncthreads();                                         // every lookup of the workgroup is done: the LDS is free
        if ((threadIdx.x & 63u) == 0) remap_lds[threadIdx.x >> 6] = wave;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint64_t t = 0;
            for (uint32_t i = 0; i < kRemapBlock / 64; i++) t += remap_lds[i];
            if (t) atomicAdd(a.bad, (unsigned long long)t);
        }
    }
}

template <int SW, int DW>
void remap_launch(bool lds, uint32_t blocks, hipStream_t s, const RemapArgs &a) {
    const size_t floor_bytes = (kRemapBlock / 64) * sizeof(uint32_t);
    if (lds) {
        const size_t bytes = (size_t)a.lut_count * sizeof(uint32_t);
        hipLaunchKernelGGL((remap_kernel<SW, DW, true>), dim3(blocks), dim3(kRemapBlock), bytes < floor_bytes ? floor_bytes : bytes, s, a);
    } else {
        hipLaunchKernelGGL((remap_kernel<SW, DW, false>), dim3(blocks), dim3(kRemapBlock), floor_bytes, s, a);
    }
}

// the six legal width pairs (dst never narrower than src)
inline void remap_launch_widths(uint32_t sw, uint32_t dw, bool lds, uint32_t blocks, hipStream_t s, const RemapArgs &a) {
    if (sw == 1 && dw == 1) remap_launch<1, 1>(lds, blocks, s, a);
    else if (sw == 1 && dw == 2) remap_launch<1, 2>(lds, blocks, s, a);
    else if (sw == 1 && dw == 4) remap_launch<1, 4>(lds, blocks, s, a);
    else if (sw == 2 && dw == 2) remap_launch<2, 2>(lds, blocks, s, a);
    else if (sw == 2 && dw == 4) remap_launch<2, 4>(lds, blocks, s, a);
    else remap_launch<4, 4>(lds, blocks, s, a);
}

}  // namespace

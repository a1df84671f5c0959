// digit_kernels.hpp -- device code of one pass of a radix select (exact percentiles, overall and per group): a histogram of
// one DIGIT of an order-preserving key, per group, under a per-group prefix (included once by pqps_hip.hip, after
// bins_kernels.hpp, whose LDS table, partial rows and group_sum_kernel it uses).
//
// No counterpart in the reference (its engines have no aggregates).  A header of its own rather than a BinSource of
// bins_scan_kernel: the bin of a row here needs the KEY column beside the group column, a 64-bit image and a search of the
// group's prefix slots, none of which Binner has; adding them there would have changed the argument blocks every existing
// instance reads.  What the family shares is reused as it stands: the scan loop, BinsLds<BINS_COUNT>, the store-and-sum
// partial rows with group_sum_kernel, the list walk.
//
// Key image: (u32)(v - key_base) for a column of 1, 2 or 4 bytes or a bit plane (the 32-bit wrap-around makes i32 - lo
// monotone), v - key_base in 64 bits for an 8-byte column.  The host promises image < 2^key_bits; a row whose image has a
// bit at or above key_bits is left out -- nothing is ever indexed with it.
// Bin of a row: t * 2^d + ((image >> shift) & (2^d - 1)), t = (group bin - bin_base) * Q + j for the slot j of the row's
// group whose prefix word equals image >> (shift + d); without prefixes (pass 0) Q = 1 and t is the group's bin.  A row whose
// group bin is not below n_bins, or whose upper bits match no slot (all ones: an unused slot), is left out.
// Where the tables live: BINS_LDS (n_tables * 2^d <= kCountLdsBins u32 counts in dynamic LDS, a partial row per workgroup,
// group_sum_kernel) or BINS_GLOBAL (one global atomic per row into the zeroed output).  Worst case of the LDS path: a
// selection whose rows share one value -- every lane of a wave adds to one counter, as a skewed group column does in
// bins_scan_kernel.
#pragma once

namespace {

constexpr uint32_t kDigitNone = 0xFFFFFFFFu;                            // no bin: the row is left out
constexpr uint32_t kDigitBitsMax = 11;                                  // 2^11 counts: 8 tables in LDS
constexpr uint32_t kDigitSlotsMax = 16;                                 // prefix slots per group
constexpr uint32_t kDigitWordsMax = 1u << 22;                           // n_tables * 2^d u32 counts of one launch (16 MiB)

// How a row gets its bin: the part of the arguments the scan and the list kernels share.
struct DigitSource {
    const void *kcol;                // key column: 1, 2, 4 bytes or a bit plane, or 8 bytes (WIDE)
    const void *gcol;                // group column, NULL: one group
    const uint64_t *prefix;          // [n_bins][slots] prefix words, NULL on pass 0
    uint64_t key_base;
    uint32_t kwidth_log2, gwidth_log2;   // 0, 1, 2 or kWidthLog2Bits (the key: unused when WIDE)
    uint32_t bin_base, n_bins;       // the window of group bins this launch counts
    uint32_t slots;                  // Q: 1 without prefixes
    uint32_t shift, digit_bits, key_bits;
};

struct DigitArgs {
    EvalArgs e;                      // the WHERE, as the COUNT kernels take it -- first: the scan loop reads it in place
    DigitSource src;
    uint32_t *out;                   // GLOBAL: the n_tables * 2^d counts (zeroed)
    uint32_t *parts;                 // LDS: [gridDim.x][stride] partial rows
    uint32_t stride;                 // words per partial row (the counts rounded up to 64)
};

struct DigitListArgs {
    DigitSource src;
    const uint32_t *ids;
    const uint64_t *count;
    uint32_t *out;                   // the n_tables * 2^d counts (zeroed)
    uint64_t n_rows, capacity;
    uint32_t id_base;
};

// The bin of a row with key image `image` in group bin t0, or kDigitNone.  Every index it returns is below
// n_bins * slots * 2^digit_bits.
template <class Src>
__device__ __forceinline__ uint32_t digit_bin(const Src &g, uint64_t image, uint32_t t0) {
    const uint32_t kb = g.key_bits, d = g.digit_bits, sh = g.shift, q = g.slots;
    if (t0 >= g.n_bins || (kb < 64u && (image >> kb) != 0)) return kDigitNone;
    const uint32_t digit = (uint32_t)(image >> sh) & ((1u << d) - 1u);
    uint32_t t = t0;
    if (g.prefix) {                                                     // uniform; shift + d < 64 (checked by the host)
        const uint64_t upper = image >> (sh + d);
        const uint64_t *slot = g.prefix + (uint64_t)t0 * q;
        t = kDigitNone;
        for (uint32_t j = 0; j < q; j++)
            if (slot[j] == upper) t = t0 * q + j;
        if (t == kDigitNone) return kDigitNone;
    }
    return (t << d) | digit;
}

// Dynamic LDS: the table (LDS path)
template <bool WIDE, int PATH, bool NT>
__global__ __launch_bounds__(kBlock, 1) void digit_scan_kernel(const DigitArgs) {
    static_assert(PATH == BINS_LDS || PATH == BINS_GLOBAL, "the digit tables live in LDS or in global memory");
    const auto &g = kernarg<DigitArgs>();
    CArgs &a = g.e;
    extern __shared__ uint64_t bins_lds[];
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t nb = (g.src.n_bins * g.src.slots) << g.src.digit_bits;
    const BinsLds<BINS_COUNT> t(bins_lds, PATH == BINS_LDS ? nb : 0u);
    if constexpr (PATH == BINS_LDS) { t.clear(nb); __syncthreads(); }
    const char *kbase = (const char *)g.src.kcol, *gbase = (const char *)g.src.gcol;
    const uint64_t key_base = g.src.key_base;
    fused_scan_steps<NT>(a, lane, wv, [&](uint64_t step_row0, uint32_t mbits) {
        uint64_t img[16];
        uint32_t t0[16];
        if constexpr (WIDE) {
            load_step_u64<true, NT>(kbase, step_row0, lane, img);
#pragma unroll
            for (int p = 0; p < 16; p++) img[p] -= key_base;
        } else {
            uint32_t v[16];
            load_step_u32<NT>(kbase, g.src.kwidth_log2, step_row0, lane, v);
#pragma unroll
            for (int p = 0; p < 16; p++) img[p] = (uint32_t)(v[p] - (uint32_t)key_base);
        }
        if (gbase) {                                                    // uniform
            load_step_u32<NT>(gbase, g.src.gwidth_log2, step_row0, lane, t0);
#pragma unroll
            for (int p = 0; p < 16; p++) t0[p] -= g.src.bin_base;
        } else {
#pragma unroll
            for (int p = 0; p < 16; p++) t0[p] = 0;
        }
#pragma unroll
        for (int p = 0; p < 16; p++) {
            if (!((mbits >> p) & 1u)) continue;
            const uint32_t b = digit_bin(g.src, img[p], t0[p]);
            if (b < nb) bins_add<PATH, BINS_COUNT>(t, g.out, nb, b, 0);
        }
    });
    if constexpr (PATH == BINS_LDS) {
        __syncthreads();
        t.store_row(g.parts, g.stride, nb);
    }
}

// The same tables over an ID list: ids[0 .. min(*count, capacity)), row = id - id_base; the columns gathered per listed row
// (1, 2, 4 or 8 bytes: no bit plane), an id listed twice counted twice.  LDS: a workgroup table flushed with one atomic per
// counter that has rows; GLOBAL: an atomic per row.
template <bool WIDE, int PATH>
__global__ __launch_bounds__(kBlock) void digit_list_kernel(const DigitListArgs g) {
    extern __shared__ uint64_t bins_lds[];
    const uint32_t nb = (g.src.n_bins * g.src.slots) << g.src.digit_bits;
    const BinsLds<BINS_COUNT> t(bins_lds, PATH == BINS_LDS ? nb : 0u);
    if constexpr (PATH == BINS_LDS) { t.clear(nb); __syncthreads(); }
    for_each_listed_row(g.ids, g.count, g.capacity, g.id_base, g.n_rows, [&](uint64_t row) {
        const uint64_t image = WIDE ? ((const uint64_t *)g.src.kcol)[row] - g.src.key_base
                                    : (uint64_t)(uint32_t)(gather_narrow(g.src.kcol, g.src.kwidth_log2, row) - (uint32_t)g.src.key_base);
        const uint32_t t0 = g.src.gcol ? gather_narrow(g.src.gcol, g.src.gwidth_log2, row) - g.src.bin_base : 0u;
        const uint32_t b = digit_bin(g.src, image, t0);
        if (b < nb) bins_add<PATH, BINS_COUNT>(t, g.out, nb, b, 0);
    });
    if constexpr (PATH == BINS_LDS) {
        __syncthreads();
        t.flush(g.out, nb);
    }
}

}  // namespace

// group_kernels.hpp -- device code of grouped COUNT(*) (included once by pqps_hip.hip, after fused_common.hpp).
//
// No counterpart in the reference (its engines have no aggregates).  A histogram of the matching rows over the values of
// one column: the bin of a row is (value - bin_base) in 32-bit arithmetic -- the dictionary code of a string column, the
// value minus the column's minimum for an i32 column, 0 / 1 for sudo_used.
//
// Fused scan (pqps_filter_group): the shared scan loop (fused_common.hpp) with ONE round of loads of the group column per
// step that holds a match.  Three bin paths, picked on the host by D:
//   SMALL  D <= 16      per-lane counters in VGPRs (8-bit fields of two u64 per step, unpacked into 16 u32 counters), wave
//                       sums on the DPP path (wave_sum_u32), workgroup sum through LDS
//   LDS    D <= 16384   a u32 histogram in dynamic LDS (ds_add_u32 per matching row); 64 KiB at most, so that two
//                       workgroups fit in a CU's 160 KiB
//   GLOBAL D <= 65536   one global atomic per matching row straight into the bins (one lane per scattered address: an order
//                       of magnitude below the shaped-atomic rate -- this path is for correctness at high cardinality, not
//                       for speed)
// SMALL and LDS end the workgroup's loop with plain coalesced stores of its D counts into a partial row of its own
// (store-and-sum rather than atomics: thousands of workgroups adding to the same few bin words would
// queue at the memory side); group_sum_kernel adds the rows up, one atomic per bin per 64 rows.  The grid is persistent
// (a few workgroups per CU), so the partials are grid x D words, not table-sized.
//
// List form (pqps_group_list): the same bins over an ID list (index probes, several passes, a shard's list): a gather of
// the group column per listed row.  Bounds (pqps_column_bounds): min / max of an i32 column.
#pragma once

namespace {

enum GroupPath { GROUP_SMALL = 0, GROUP_LDS = 1, GROUP_GLOBAL = 2 };
constexpr uint32_t kGroupSmallBins = 16;
constexpr uint32_t kGroupLdsBins = 16384;          // 64 KiB of LDS: two workgroups per CU
constexpr uint32_t kGroupMaxBins = 65536;
constexpr uint32_t kGroupSumParts = 64;            // partial rows one workgroup of group_sum_kernel adds up

struct GroupArgs {
    EvalArgs e;                      // the WHERE, as the COUNT kernels take it -- first: the scan loop reads it in place
    const void *gcol;                // group column (bytes, u16, u32 or a bit plane)
    uint32_t *bins;                  // GLOBAL: D u32 bins (zeroed before the launch)
    uint32_t *parts;                 // SMALL / LDS: [gridDim.x][stride] partial counts
    uint32_t stride;                 // words per partial row (D rounded up to 64)
    uint32_t gwidth_log2;            // 0, 1, 2 or kWidthLog2Bits
    uint32_t bin_base;
    uint32_t n_bins;
};

template <int PATH, bool NT>
__global__ __launch_bounds__(kBlock, 1) void group_scan_kernel(const GroupArgs) {
    const auto &g = kernarg<GroupArgs>();
    CArgs &a = g.e;
    extern __shared__ uint32_t hist[];                          // LDS path: n_bins words
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t nb = g.n_bins, base_bin = g.bin_base, wl = g.gwidth_log2;
    const char *gbase = (const char *)g.gcol;
    if constexpr (PATH == GROUP_LDS) {
        for (uint32_t i = threadIdx.x; i < nb; i += kBlock) hist[i] = 0;
        __syncthreads();
    }
    uint32_t cnt[kGroupSmallBins];
#pragma unroll
    for (uint32_t k = 0; k < kGroupSmallBins; k++) cnt[k] = 0;
    fused_scan_steps<NT>(a, lane, wv, [&](uint64_t step_row0, uint32_t mbits) {
        uint32_t v[16];
        load_step_u32<NT>(gbase, wl, step_row0, lane, v);
        if constexpr (PATH == GROUP_SMALL) {
            uint64_t f0 = 0, f1 = 0;                            // 8-bit fields: bins 0 .. 7 and 8 .. 15 (at most 16 rows per lane)
#pragma unroll
            for (int p = 0; p < 16; p++) {
                const uint32_t b = v[p] - base_bin;
                const bool hit = ((mbits >> p) & 1u) && b < nb;
                const uint64_t inc = hit ? 1ull << ((b & 7u) * 8u) : 0ull;
                if (b < 8u) f0 += inc; else f1 += inc;
            }
#pragma unroll
            for (uint32_t k = 0; k < kGroupSmallBins; k++)
                cnt[k] += (uint32_t)((k < 8 ? f0 >> (8 * k) : f1 >> (8 * (k - 8))) & 0xFFu);
        } else {
#pragma unroll
            for (int p = 0; p < 16; p++) {
                const uint32_t b = v[p] - base_bin;
                if (((mbits >> p) & 1u) && b < nb) {
                    if constexpr (PATH == GROUP_LDS) atomicAdd(&hist[b], 1u);
                    else atomicAdd(&g.bins[b], 1u);
                }
            }
        }
    });
    if constexpr (PATH == GROUP_SMALL) {
        __shared__ uint32_t s_small[kWaves][kGroupSmallBins];
#pragma unroll
        for (uint32_t k = 0; k < kGroupSmallBins; k++) {
            if (k < nb) {                                       // uniform
                const uint32_t s = wave_sum_u32(cnt[k]);
                if (lane == 0) s_small[wv][k] = s;
            }
        }
        __syncthreads();
        if (threadIdx.x < g.stride) {                           // the whole partial row: bins past D are zeros
            uint32_t t = 0;
            if (threadIdx.x < nb)
                for (uint32_t w = 0; w < (uint32_t)kWaves; w++) t += s_small[w][threadIdx.x];
            g.parts[(uint64_t)blockIdx.x * g.stride + threadIdx.x] = t;
        }
    } else if constexpr (PATH == GROUP_LDS) {
        __syncthreads();
        uint32_t *row = g.parts + (uint64_t)blockIdx.x * g.stride;
        for (uint32_t i = threadIdx.x; i < g.stride; i += kBlock) row[i] = i < nb ? hist[i] : 0u;
    }
}

// bins[k] += sum of parts[r][k] over the rows r of this workgroup's 64-row slice; 64 bins per workgroup (one per lane),
// the 4 waves take 16 rows each (loads issued together), summed through LDS.  bins zeroed before the launch.
__global__ __launch_bounds__(kBlock) void group_sum_kernel(const uint32_t *__restrict__ parts, uint32_t n_parts, uint32_t stride,
                                                           uint32_t n_bins, uint32_t *__restrict__ bins) {
    __shared__ uint32_t s_sum[kWaves][64];
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t bin = blockIdx.x * 64 + lane;                // < stride: the grid covers stride / 64 bin slices
    const uint32_t r0 = blockIdx.y * kGroupSumParts + wv * (kGroupSumParts / kWaves);
    uint32_t v[kGroupSumParts / kWaves];
#pragma unroll
    for (uint32_t i = 0; i < kGroupSumParts / kWaves; i++)
        v[i] = r0 + i < n_parts ? parts[(uint64_t)(r0 + i) * stride + bin] : 0u;
    uint32_t t = 0;
#pragma unroll
    for (uint32_t i = 0; i < kGroupSumParts / kWaves; i++) t += v[i];
    s_sum[wv][lane] = t;
    __syncthreads();
    if (wv == 0) {
        t = s_sum[0][lane] + s_sum[1][lane] + s_sum[2][lane] + s_sum[3][lane];
        if (t && bin < n_bins) atomicAdd(&bins[bin], t);
    }
}

// The bins over an ID list: ids[0 .. min(*count, capacity)), row = id - id_base.  LDS: a workgroup histogram flushed with
// one atomic per non-zero bin; otherwise one atomic per row into the bins.  bins zeroed before the launch.
template <bool LDS>
__global__ __launch_bounds__(kBlock) void group_list_kernel(const void *col, uint32_t wlog2, uint64_t n_rows, const uint32_t *__restrict__ ids,
                                                            const uint64_t *count, uint64_t capacity, uint32_t id_base, uint32_t bin_base,
                                                            uint32_t n_bins, uint32_t *bins) {
    extern __shared__ uint32_t hist[];
    if constexpr (LDS) {
        for (uint32_t i = threadIdx.x; i < n_bins; i += kBlock) hist[i] = 0;
        __syncthreads();
    }
    for_each_listed_row(ids, count, capacity, id_base, n_rows, [&](uint64_t row) {
        const uint32_t b = gather_narrow(col, wlog2, row) - bin_base;
        if (b >= n_bins) return;
        if constexpr (LDS) atomicAdd(&hist[b], 1u);
        else atomicAdd(&bins[b], 1u);
    });
    if constexpr (LDS) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < n_bins; i += kBlock)
            if (hist[i]) atomicAdd(&bins[i], hist[i]);
    }
}

// min / max of an i32 column, as order-preserving u32 images (v ^ 2^31): out[0] = max of the complemented images (= the
// minimum), out[1] = max of the images; both zeroed before the launch (an empty column leaves INT_MAX / INT_MIN behind
// group_bounds_finish_kernel).
__global__ __launch_bounds__(kBlock) void group_bounds_kernel(const int32_t *__restrict__ col, uint64_t n, uint32_t *out) {
    uint32_t lo_c = 0, hi = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t u = (uint32_t)col[i] ^ 0x80000000u;
        lo_c = max(lo_c, ~u);
        hi = max(hi, u);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        lo_c = max(lo_c, (uint32_t)__shfl_xor((int)lo_c, off, 64));
        hi = max(hi, (uint32_t)__shfl_xor((int)hi, off, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        if (lo_c) atomicMax(&out[0], lo_c);
        if (hi) atomicMax(&out[1], hi);
    }
}

__global__ void group_bounds_finish_kernel(uint32_t *out) {
    const uint32_t lo = ~out[0] ^ 0x80000000u, hi = out[1] ^ 0x80000000u;
    ((int32_t *)out)[0] = (int32_t)lo;
    ((int32_t *)out)[1] = (int32_t)hi;
}

}  // namespace

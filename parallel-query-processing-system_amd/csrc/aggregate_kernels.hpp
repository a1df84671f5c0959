// aggregate_kernels.hpp -- device code of COUNT / SUM / MIN / MAX of a value column, overall or per group (included once by
// pqps_hip.hip, after fused_common.hpp).
//
// No counterpart in the reference (its engines have no aggregates).  One accumulator form for both value widths, four u64
// words per bin:
//   count  matching rows
//   sum    the value sign-extended (i32) or as is (u64), added mod 2^64
//   min    the minimum of the order-preserving u64 IMAGE of the value: (u64)(i64)v ^ 2^63 for i32, v itself for u64
//   max    the maximum of the image
// so that every update is a native 64-bit add / unsigned min / unsigned max (ds_add_u64, ds_min_u64, ds_max_u64,
// global_atomic_add_x2 / umin_x2 / umax_x2 -- no compare-and-swap loops).  The host undoes the image.
//
// Fused scan (pqps_filter_aggregate): the shared scan loop (fused_common.hpp) with one round of value-column loads (one
// ld_x4 per 256-row chunk for an i32 value, two for command_id) and group-column loads per step that holds a match.  Bin paths:
//   ONE    no GROUP BY   per-lane registers, a wave reduction (shuffles, once per workgroup), the 4 waves through LDS
//   LDS    D <= 2304     a table of 28 B per bin in dynamic LDS (u32 count, u64 sum / min / max), 64 KiB at most
//   GLOBAL D <= 65536    four global 64-bit atomics per matching row straight into the output (a correctness path, like
//                        GROUP_GLOBAL: one lane per scattered address)
// ONE and LDS end the workgroup's loop with plain stores of a partial row (store-and-sum); agg_sum_kernel
// combines 64 rows per workgroup with one atomic per bin and field.  No same-address global atomic per row or per wave.
//
// List form (pqps_aggregate_list): the same accumulators over an ID list, gathering the value column (and the group column)
// per listed row.
#pragma once

namespace {

enum AggPath { AGG_ONE = 0, AGG_LDS = 1, AGG_GLOBAL = 2 };
constexpr uint32_t kAggLdsBins = 2304;             // 28 B per bin: 64 512 B of LDS, two workgroups per CU
constexpr uint32_t kAggFields = 4;                 // count, sum, min image, max image
constexpr uint32_t kAggSumParts = 64;              // partial rows one workgroup of agg_sum_kernel combines

struct AggArgs {
    EvalArgs e;                      // the WHERE, as the COUNT kernels take it -- first: the scan loop reads it in place
    const void *vcol;                // value column: i32 or u64
    const void *gcol;                // group column (bytes, u16, u32 or a bit plane); unused by AGG_ONE
    uint64_t *out;                   // GLOBAL: [4][n_bins] (initialised before the launch)
    uint64_t *parts;                 // ONE / LDS: [gridDim.x][4][n_bins] partial rows
    uint32_t gwidth_log2;            // 0, 1, 2 or kWidthLog2Bits
    uint32_t bin_base;
    uint32_t n_bins;
};

// the order-preserving image of the value a sum adds (widen_value)
template <bool U64> __device__ __forceinline__ uint64_t agg_image(uint64_t wide) {
    if constexpr (U64) return wide;
    else return wide ^ 0x8000000000000000ull;
}

// (count, sum, min image, max image) of the 64 lanes, in every lane
__device__ __forceinline__ void wave_reduce_acc(uint64_t &cnt, uint64_t &sum, uint64_t &mn, uint64_t &mx) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        cnt += shfl_xor_u64(cnt, off);
        sum += shfl_xor_u64(sum, off);
        const uint64_t m = shfl_xor_u64(mn, off), x = shfl_xor_u64(mx, off);
        mn = m < mn ? m : mn;
        mx = x > mx ? x : mx;
    }
}

// The four waves' totals through LDS; thread 0 returns the workgroup's in its arguments.
__device__ __forceinline__ void block_reduce_acc(uint64_t &cnt, uint64_t &sum, uint64_t &mn, uint64_t &mx) {
    __shared__ uint64_t s_acc[kWaves][kAggFields];
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    wave_reduce_acc(cnt, sum, mn, mx);
    if (lane == 0) { s_acc[wv][0] = cnt; s_acc[wv][1] = sum; s_acc[wv][2] = mn; s_acc[wv][3] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (uint32_t w = 1; w < (uint32_t)kWaves; w++) {
            cnt += s_acc[w][0]; sum += s_acc[w][1];
            mn = s_acc[w][2] < mn ? s_acc[w][2] : mn;
            mx = s_acc[w][3] > mx ? s_acc[w][3] : mx;
        }
    }
}

// LDS table of the LDS paths: u64 sum / min / max arrays, then u32 counts (n_bins entries each)
struct AggLds {
    unsigned long long *sum, *mn, *mx;
    uint32_t *cnt;
    __device__ __forceinline__ AggLds(void *base, uint32_t nb) {
        sum = (unsigned long long *)base; mn = sum + nb; mx = mn + nb; cnt = (uint32_t *)(mx + nb);
    }
    __device__ __forceinline__ void clear(uint32_t nb) {
        for (uint32_t i = threadIdx.x; i < nb; i += blockDim.x) { sum[i] = 0; mn[i] = ~0ull; mx[i] = 0; cnt[i] = 0; }
    }
    __device__ __forceinline__ void add(uint32_t b, uint64_t wide, uint64_t img) {
        atomicAdd(&cnt[b], 1u);
        atomicAdd(&sum[b], (unsigned long long)wide);
        atomicMin(&mn[b], (unsigned long long)img);
        atomicMax(&mx[b], (unsigned long long)img);
    }
};

// GLOBAL path / list flushes: the four fields of bin b of out[4][n_bins]
__device__ __forceinline__ void agg_global_add(uint64_t *out, uint32_t nb, uint32_t b, uint64_t cnt, uint64_t sum, uint64_t mn, uint64_t mx) {
    unsigned long long *o = (unsigned long long *)out;
    atomicAdd(&o[b], (unsigned long long)cnt);
    atomicAdd(&o[nb + b], (unsigned long long)sum);
    atomicMin(&o[2 * (uint64_t)nb + b], (unsigned long long)mn);
    atomicMax(&o[3 * (uint64_t)nb + b], (unsigned long long)mx);
}

template <int PATH, bool U64, bool NT>
__global__ __launch_bounds__(kBlock, 1) void agg_scan_kernel(const AggArgs) {
    const auto &g = kernarg<AggArgs>();
    CArgs &a = g.e;
    extern __shared__ uint64_t agg_lds[];                       // LDS path: the table
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t nb = g.n_bins, base_bin = g.bin_base, wl = g.gwidth_log2;
    const char *vbase = (const char *)g.vcol;
    const char *gbase = (const char *)g.gcol;
    AggLds t(agg_lds, nb);
    if constexpr (PATH == AGG_LDS) {
        t.clear(nb);
        __syncthreads();
    }
    uint64_t cnt = 0, sum = 0, mn = ~0ull, mx = 0;              // AGG_ONE
    fused_scan_steps<NT>(a, lane, wv, [&](uint64_t step_row0, uint32_t mbits) {
        uint64_t v[16];
        load_step_u64<U64, NT>(vbase, step_row0, lane, v);
        if constexpr (PATH == AGG_ONE) {
            cnt += __popc(mbits);
#pragma unroll
            for (int p = 0; p < 16; p++) {
                const bool hit = (mbits >> p) & 1u;
                const uint64_t img = agg_image<U64>(v[p]);
                sum += hit ? v[p] : 0ull;
                mn = hit && img < mn ? img : mn;
                mx = hit && img > mx ? img : mx;
            }
        } else {
            uint32_t gv[16];
            load_step_u32<NT>(gbase, wl, step_row0, lane, gv);
#pragma unroll
            for (int p = 0; p < 16; p++) {
                const uint32_t b = gv[p] - base_bin;
                if (((mbits >> p) & 1u) && b < nb) {
                    if constexpr (PATH == AGG_LDS) t.add(b, v[p], agg_image<U64>(v[p]));
                    else agg_global_add(g.out, nb, b, 1, v[p], agg_image<U64>(v[p]), agg_image<U64>(v[p]));
                }
            }
        }
    });
    if constexpr (PATH == AGG_ONE) {
        block_reduce_acc(cnt, sum, mn, mx);
        if (threadIdx.x == 0) {
            uint64_t *row = g.parts + (uint64_t)blockIdx.x * kAggFields;
            row[0] = cnt; row[1] = sum; row[2] = mn; row[3] = mx;
        }
    } else if constexpr (PATH == AGG_LDS) {
        __syncthreads();
        uint64_t *row = g.parts + (uint64_t)blockIdx.x * kAggFields * nb;
        for (uint32_t i = threadIdx.x; i < nb; i += kBlock) {
            row[i] = t.cnt[i]; row[nb + i] = t.sum[i]; row[2 * nb + i] = t.mn[i]; row[3 * nb + i] = t.mx[i];
        }
    }
}

// out[.][bin] combined with the partial rows r of this workgroup's 64-row slice: one bin per lane, the 4 waves take 16 rows
// each, combined through LDS, one atomic per field of a bin that has rows.  out initialised before the launch.
__global__ __launch_bounds__(kBlock) void agg_sum_kernel(const uint64_t *__restrict__ parts, uint32_t n_parts, uint32_t n_bins,
                                                         uint64_t *out) {
    __shared__ uint64_t s_acc[kWaves][kAggFields][64];
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t bin = blockIdx.x * 64 + lane;
    const uint32_t r0 = blockIdx.y * kAggSumParts + wv * (kAggSumParts / kWaves);
    uint64_t cnt = 0, sum = 0, mn = ~0ull, mx = 0;
    if (bin < n_bins) {
        for (uint32_t i = 0; i < kAggSumParts / kWaves && r0 + i < n_parts; i++) {
            const uint64_t *row = parts + (uint64_t)(r0 + i) * kAggFields * n_bins;
            const uint64_t m = row[2 * n_bins + bin], x = row[3 * n_bins + bin];
            cnt += row[bin]; sum += row[n_bins + bin];
            mn = m < mn ? m : mn;
            mx = x > mx ? x : mx;
        }
    }
    s_acc[wv][0][lane] = cnt; s_acc[wv][1][lane] = sum; s_acc[wv][2][lane] = mn; s_acc[wv][3][lane] = mx;
    __syncthreads();
    if (wv == 0 && bin < n_bins) {
        for (uint32_t w = 1; w < (uint32_t)kWaves; w++) {
            cnt += s_acc[w][0][lane]; sum += s_acc[w][1][lane];
            mn = s_acc[w][2][lane] < mn ? s_acc[w][2][lane] : mn;
            mx = s_acc[w][3][lane] > mx ? s_acc[w][3][lane] : mx;
        }
        if (cnt) agg_global_add(out, n_bins, bin, cnt, sum, mn, mx);
    }
}

// The accumulators over an ID list: ids[0 .. min(*count, capacity)), row = id - id_base.  gcol == nullptr: no GROUP BY
// (n_bins = 1), per-lane registers reduced per workgroup, one atomic per field and workgroup; LDS: a workgroup table
// flushed with one atomic per field of a bin that has rows; otherwise four atomics per row.  out initialised before the launch.
// The walk is for_each_listed_row's, written out here (why: DESIGN.md §7a).
template <int PATH, bool U64>
__global__ __launch_bounds__(kBlock) void agg_list_kernel(const void *vcol, const void *gcol, uint32_t gwlog2, uint64_t n_rows,
                                                          const uint32_t *__restrict__ ids, const uint64_t *count, uint64_t capacity,
                                                          uint32_t id_base, uint32_t bin_base, uint32_t n_bins, uint64_t *out) {
    extern __shared__ uint64_t agg_lds[];
    AggLds t(agg_lds, n_bins);
    if constexpr (PATH == AGG_LDS) {
        t.clear(n_bins);
        __syncthreads();
    }
    uint64_t cnt = 0, sum = 0, mn = ~0ull, mx = 0;
    uint64_t n = *count;
    if (n > capacity) n = capacity;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t row = (uint64_t)(ids[i] - id_base);
        if (row >= n_rows) continue;                            // (never: a shard's list holds its own rows)
        const uint64_t v = U64 ? ((const uint64_t *)vcol)[row] : widen_value<false>((uint32_t)((const int32_t *)vcol)[row]);
        const uint64_t img = agg_image<U64>(v);
        if constexpr (PATH == AGG_ONE) {
            cnt++; sum += v;
            mn = img < mn ? img : mn;
            mx = img > mx ? img : mx;
        } else {
            const uint32_t b = gather_narrow(gcol, gwlog2, row) - bin_base;
            if (b >= n_bins) continue;
            if constexpr (PATH == AGG_LDS) t.add(b, v, img);
            else agg_global_add(out, n_bins, b, 1, v, img, img);
        }
    }
    if constexpr (PATH == AGG_ONE) {
        block_reduce_acc(cnt, sum, mn, mx);
        if (threadIdx.x == 0 && cnt) agg_global_add(out, 1, 0, cnt, sum, mn, mx);
    } else if constexpr (PATH == AGG_LDS) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < n_bins; i += kBlock)
            if (t.cnt[i]) agg_global_add(out, n_bins, i, t.cnt[i], t.sum[i], t.mn[i], t.mx[i]);
    }
}

}  // namespace

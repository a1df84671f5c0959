// bucket_kernels.hpp -- device code of GROUP BY buckets: string prefixes and number ranges (included once by pqps_hip.hip,
// after fused_common.hpp; it uses no other kernel header).
//
// No counterpart in the reference (its engines have no aggregates).  The bin of a row is (value - bin_base) in 32-bit
// arithmetic, as in group_kernels.hpp; a BUCKET is a contiguous run of bins, given by the ascending u32 run starts
// bounds[0 .. n_buckets] whose last entry is the domain (hipBucketBounds makes them):
//     bucket(b) = (number of entries of bounds[0 .. n_buckets] that are <= b) - 1,     a row with bucket >= n_buckets is left out
// -- exactly the rows with b >= domain, which every entry is <= to.  The count is a branch-free upper-bound search
// (bucket_search): ceil(log2(n_buckets + 2)) rounds, each one clamped load, a compare and a conditional add; the 16 rows a lane
// holds of a step are 16 independent searches advanced round by round, so the 16 loads of a round are in flight together.
// Whatever bounds holds, a bucket that is counted is < n_buckets: nothing is indexed out of range.
//
// Where things live (a workgroup takes at most 64 KiB of dynamic LDS, so that two fit a CU):
//   the bounds       in LDS (copied once per workgroup) whenever n_buckets + 1 words fit beside the bins table; otherwise
//                    read from global memory (at most 256 KiB: L2-resident)
//   COUNT bins       SMALL   n_buckets <= 16      per-lane counters in VGPRs, as GROUP_SMALL
//                    LDS     n_buckets <= 8191    a u32 histogram in LDS beside the bounds (8 B per bucket + the sentinel)
//                    GLOBAL  n_buckets <= 65536   one global atomic per matching row (correctness path); bounds in LDS up to
//                                                 16383 buckets
//   aggregate bins   LDS     n_buckets <= 2047    the 28 B table of aggregate_kernels.hpp beside the bounds (32 B per bucket)
//                    GLOBAL  n_buckets <= 65536   four global 64-bit atomics per matching row; bounds in LDS up to 16383
// SMALL and LDS end in store-and-sum partial rows in the layouts of group_scan_kernel / agg_scan_kernel: the shim adds them
// up with group_sum_kernel / agg_sum_kernel as they are.  The aggregate fields are those of aggregate_kernels.hpp: count, sum
// mod 2^64, min / max of the order-preserving u64 image.
//
// List forms: the same bins over an ID list (for_each_listed_row, gather_narrow), one search per listed row.
#pragma once

namespace {

enum BucketPath { BUCKET_SMALL = 0, BUCKET_LDS = 1, BUCKET_GLOBAL = 2 };
constexpr uint32_t kBucketMax = 65536;
constexpr uint32_t kBucketSmall = 16;
constexpr uint32_t kBucketLdsBytes = 64u << 10;                        // dynamic LDS of one workgroup: two per CU
constexpr uint32_t kBucketAggBinBytes = 3 * 8 + 4;                     // u64 sum / min / max, u32 count
constexpr uint32_t kBucketCountLds = (kBucketLdsBytes - 4) / 8;        // 8191: bins + bounds + the sentinel
constexpr uint32_t kBucketAggLds = (kBucketLdsBytes - 4) / (kBucketAggBinBytes + 4);   // 2047: table + bounds + the sentinel
constexpr uint32_t kBucketBoundsLds = kBucketLdsBytes / 4 - 1;         // 16383: the bounds alone (GLOBAL bins)

struct BucketArgs {
    EvalArgs e;                      // the WHERE, as the COUNT kernels take it -- first: the scan loop reads it in place
    const void *gcol;                // group column: bytes, u16 or u32
    const void *vcol;                // aggregates: value column, i32 or u64
    const uint32_t *bounds;          // n_buckets + 1 ascending run starts in bin space, the last one the domain
    void *out;                       // GLOBAL: n_buckets u32 bins (zeroed) / [4][n_buckets] u64 fields (initialised)
    void *parts;                     // SMALL / LDS: [gridDim.x][stride] u32 / [gridDim.x][4][n_buckets] u64 partial rows
    uint32_t stride;                 // COUNT: words per partial row (n_buckets rounded up to 64)
    uint32_t gwidth_log2;            // 0, 1 or 2
    uint32_t bin_base;
    uint32_t n_buckets;
    uint32_t top;                    // the largest power of two <= n_buckets + 1: the first stride of the search
};

// pos[p] = number of entries of bounds[0 .. n) that are <= b[p]; N independent searches advanced together.
template <int N>
__device__ __forceinline__ void bucket_search(const uint32_t *bounds, uint32_t n, uint32_t top, const uint32_t (&b)[N], uint32_t (&pos)[N]) {
#pragma unroll
    for (int p = 0; p < N; p++) pos[p] = 0;
    for (uint32_t step = top; step; step >>= 1) {                       // uniform
#pragma unroll
        for (int p = 0; p < N; p++) {
            const uint32_t i = pos[p] + step - 1;
            const bool in = i < n;
            const uint32_t v = bounds[in ? i : n - 1];
            pos[p] += in && v <= b[p] ? step : 0u;
        }
    }
}

// The bounds of the workgroup: copied into lds[0 .. n) where IN_LDS (the caller syncs), else where they are.
template <bool IN_LDS>
__device__ __forceinline__ const uint32_t *bucket_bounds(const uint32_t *bounds, uint32_t n, uint32_t *lds) {
    if constexpr (IN_LDS) {
        for (uint32_t i = threadIdx.x; i < n; i += kBlock) lds[i] = bounds[i];
        return lds;
    } else {
        return bounds;
    }
}

template <bool U64> __device__ __forceinline__ uint64_t bucket_image(uint64_t wide) {
    if constexpr (U64) return wide;
    else return wide ^ 0x8000000000000000ull;
}

// The aggregate table in LDS: u64 sum / min / max arrays, then u32 counts (nb entries each), then room for the bounds.
struct BucketTable {
    unsigned long long *sum, *mn, *mx;
    uint32_t *cnt;
    __device__ __forceinline__ BucketTable(void *base, uint32_t nb) {
        sum = (unsigned long long *)base; mn = sum + nb; mx = mn + nb; cnt = (uint32_t *)(mx + nb);
    }
    __device__ __forceinline__ void clear(uint32_t nb) {
        for (uint32_t i = threadIdx.x; i < nb; i += kBlock) { sum[i] = 0; mn[i] = ~0ull; mx[i] = 0; cnt[i] = 0; }
    }
    __device__ __forceinline__ void add(uint32_t k, uint64_t wide, uint64_t img) {
        atomicAdd(&cnt[k], 1u);
        atomicAdd(&sum[k], (unsigned long long)wide);
        atomicMin(&mn[k], (unsigned long long)img);
        atomicMax(&mx[k], (unsigned long long)img);
    }
};

// the four fields of bucket k of out[4][nb]
__device__ __forceinline__ void bucket_global_add(void *out, uint32_t nb, uint32_t k, uint64_t cnt, uint64_t sum, uint64_t mn, uint64_t mx) {
    unsigned long long *o = (unsigned long long *)out;
    atomicAdd(&o[k], (unsigned long long)cnt);
    atomicAdd(&o[nb + k], (unsigned long long)sum);
    atomicMin(&o[2 * (uint64_t)nb + k], (unsigned long long)mn);
    atomicMax(&o[3 * (uint64_t)nb + k], (unsigned long long)mx);
}

// COUNT(*) per bucket, fused with the WHERE.  Dynamic LDS: [bounds, n_buckets + 1 words, where BLDS][bins, n_buckets words, LDS path]
template <int PATH, bool BLDS, bool NT>
__global__ __launch_bounds__(kBlock, 1) void bucket_scan_kernel(const BucketArgs) {
    const auto &g = kernarg<BucketArgs>();
    CArgs &a = g.e;
    extern __shared__ uint32_t bucket_lds[];
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t nb = g.n_buckets, n = nb + 1, top = g.top, base_bin = g.bin_base, wl = g.gwidth_log2;
    const char *gbase = (const char *)g.gcol;
    const uint32_t *bnd = bucket_bounds<BLDS>(g.bounds, n, bucket_lds);
    uint32_t *hist = bucket_lds + (BLDS ? n : 0u);
    if constexpr (PATH == BUCKET_LDS)
        for (uint32_t i = threadIdx.x; i < nb; i += kBlock) hist[i] = 0;
    if constexpr (BLDS || PATH == BUCKET_LDS) __syncthreads();
    uint32_t cnt[kBucketSmall];
#pragma unroll
    for (uint32_t k = 0; k < kBucketSmall; k++) cnt[k] = 0;
    fused_scan_steps<NT>(a, lane, wv, [&](uint64_t step_row0, uint32_t mbits) {
        uint32_t v[16], pos[16];
        load_step_u32<NT>(gbase, wl, step_row0, lane, v);
#pragma unroll
        for (int p = 0; p < 16; p++) v[p] -= base_bin;
        bucket_search<16>(bnd, n, top, v, pos);
        if constexpr (PATH == BUCKET_SMALL) {
            uint64_t f0 = 0, f1 = 0;                            // 8-bit fields: buckets 0 .. 7 and 8 .. 15 (at most 16 rows per lane)
#pragma unroll
            for (int p = 0; p < 16; p++) {
                const uint32_t k = pos[p] - 1u;
                const bool hit = ((mbits >> p) & 1u) && k < nb;
                const uint64_t inc = hit ? 1ull << ((k & 7u) * 8u) : 0ull;
                if (k < 8u) f0 += inc; else f1 += inc;
            }
#pragma unroll
            for (uint32_t k = 0; k < kBucketSmall; k++)
                cnt[k] += (uint32_t)((k < 8 ? f0 >> (8 * k) : f1 >> (8 * (k - 8))) & 0xFFu);
        } else {
#pragma unroll
            for (int p = 0; p < 16; p++) {
                const uint32_t k = pos[p] - 1u;
                if (((mbits >> p) & 1u) && k < nb) {
                    if constexpr (PATH == BUCKET_LDS) atomicAdd(&hist[k], 1u);
                    else atomicAdd(&((uint32_t *)g.out)[k], 1u);
                }
            }
        }
    });
    uint32_t *parts = (uint32_t *)g.parts;
    if constexpr (PATH == BUCKET_SMALL) {
        __shared__ uint32_t s_small[kWaves][kBucketSmall];
#pragma unroll
        for (uint32_t k = 0; k < kBucketSmall; k++) {
            if (k < nb) {                                       // uniform
                const uint32_t s = wave_sum_u32(cnt[k]);
                if (lane == 0) s_small[wv][k] = s;
            }
        }
        __syncthreads();
        if (threadIdx.x < g.stride) {                           // the whole partial row: buckets past n_buckets are zeros
            uint32_t t = 0;
            if (threadIdx.x < nb)
                for (uint32_t w = 0; w < (uint32_t)kWaves; w++) t += s_small[w][threadIdx.x];
            parts[(uint64_t)blockIdx.x * g.stride + threadIdx.x] = t;
        }
    } else if constexpr (PATH == BUCKET_LDS) {
        __syncthreads();
        uint32_t *row = parts + (uint64_t)blockIdx.x * g.stride;
        for (uint32_t i = threadIdx.x; i < g.stride; i += kBlock) row[i] = i < nb ? hist[i] : 0u;
    }
}

// COUNT / SUM / MIN / MAX of a value column per bucket, fused with the WHERE.  Dynamic LDS: [table, 28 B per bucket, LDS
// path][bounds, n_buckets + 1 words, where BLDS]
template <int PATH, bool BLDS, bool U64, bool NT>
__global__ __launch_bounds__(kBlock, 1) void bucket_agg_scan_kernel(const BucketArgs) {
    const auto &g = kernarg<BucketArgs>();
    CArgs &a = g.e;
    extern __shared__ uint64_t bucket_agg_lds[];
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t nb = g.n_buckets, n = nb + 1, top = g.top, base_bin = g.bin_base, wl = g.gwidth_log2;
    const char *vbase = (const char *)g.vcol;
    const char *gbase = (const char *)g.gcol;
    BucketTable t(bucket_agg_lds, nb);
    uint32_t *lds_bounds = PATH == BUCKET_LDS ? t.cnt + nb : (uint32_t *)bucket_agg_lds;
    const uint32_t *bnd = bucket_bounds<BLDS>(g.bounds, n, lds_bounds);
    if constexpr (PATH == BUCKET_LDS) t.clear(nb);
    if constexpr (BLDS || PATH == BUCKET_LDS) __syncthreads();
    fused_scan_steps<NT>(a, lane, wv, [&](uint64_t step_row0, uint32_t mbits) {
        uint64_t v[16];
        uint32_t gv[16], pos[16];
        load_step_u64<U64, NT>(vbase, step_row0, lane, v);
        load_step_u32<NT>(gbase, wl, step_row0, lane, gv);
#pragma unroll
        for (int p = 0; p < 16; p++) gv[p] -= base_bin;
        bucket_search<16>(bnd, n, top, gv, pos);
#pragma unroll
        for (int p = 0; p < 16; p++) {
            const uint32_t k = pos[p] - 1u;
            if (((mbits >> p) & 1u) && k < nb) {
                const uint64_t img = bucket_image<U64>(v[p]);
                if constexpr (PATH == BUCKET_LDS) t.add(k, v[p], img);
                else bucket_global_add(g.out, nb, k, 1, v[p], img, img);
            }
        }
    });
    if constexpr (PATH == BUCKET_LDS) {
        __syncthreads();
        uint64_t *row = (uint64_t *)g.parts + (uint64_t)blockIdx.x * 4 * nb;
        for (uint32_t i = threadIdx.x; i < nb; i += kBlock) {
            row[i] = t.cnt[i]; row[nb + i] = t.sum[i]; row[2 * nb + i] = t.mn[i]; row[3 * nb + i] = t.mx[i];
        }
    }
}

struct BucketListArgs {
    const void *gcol, *vcol;
    const uint32_t *bounds;
    const uint32_t *ids;
    const uint64_t *count;
    void *out;                       // n_buckets u32 bins (zeroed) / [4][n_buckets] u64 fields (initialised)
    uint64_t n_rows, capacity;
    uint32_t gwidth_log2, id_base, bin_base, n_buckets, top;
};

// The bucket counts over an ID list: ids[0 .. min(*count, capacity)), row = id - id_base.  LDS: a workgroup histogram
// flushed with one atomic per non-zero bucket; otherwise one atomic per row.
template <int PATH, bool BLDS>
__global__ __launch_bounds__(kBlock) void bucket_list_kernel(const BucketListArgs g) {
    extern __shared__ uint32_t bucket_lds[];
    const uint32_t nb = g.n_buckets, n = nb + 1;
    const uint32_t *bnd = bucket_bounds<BLDS>(g.bounds, n, bucket_lds);
    uint32_t *hist = bucket_lds + (BLDS ? n : 0u);
    uint32_t *bins = (uint32_t *)g.out;
    if constexpr (PATH == BUCKET_LDS)
        for (uint32_t i = threadIdx.x; i < nb; i += kBlock) hist[i] = 0;
    if constexpr (BLDS || PATH == BUCKET_LDS) __syncthreads();
    for_each_listed_row(g.ids, g.count, g.capacity, g.id_base, g.n_rows, [&](uint64_t row) {
        const uint32_t b[1] = { gather_narrow(g.gcol, g.gwidth_log2, row) - g.bin_base };
        uint32_t pos[1];
        bucket_search<1>(bnd, n, g.top, b, pos);
        const uint32_t k = pos[0] - 1u;
        if (k >= nb) return;
        if constexpr (PATH == BUCKET_LDS) atomicAdd(&hist[k], 1u);
        else atomicAdd(&bins[k], 1u);
    });
    if constexpr (PATH == BUCKET_LDS) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < nb; i += kBlock)
            if (hist[i]) atomicAdd(&bins[i], hist[i]);
    }
}

// The aggregates over an ID list.  LDS: a workgroup table flushed with one atomic per field of a bucket that has rows;
// otherwise four atomics per row.
template <int PATH, bool BLDS, bool U64>
__global__ __launch_bounds__(kBlock) void bucket_agg_list_kernel(const BucketListArgs g) {
    extern __shared__ uint64_t bucket_agg_lds[];
    const uint32_t nb = g.n_buckets, n = nb + 1;
    BucketTable t(bucket_agg_lds, nb);
    uint32_t *lds_bounds = PATH == BUCKET_LDS ? t.cnt + nb : (uint32_t *)bucket_agg_lds;
    const uint32_t *bnd = bucket_bounds<BLDS>(g.bounds, n, lds_bounds);
    if constexpr (PATH == BUCKET_LDS) t.clear(nb);
    if constexpr (BLDS || PATH == BUCKET_LDS) __syncthreads();
    for_each_listed_row(g.ids, g.count, g.capacity, g.id_base, g.n_rows, [&](uint64_t row) {
        const uint32_t b[1] = { gather_narrow(g.gcol, g.gwidth_log2, row) - g.bin_base };
        uint32_t pos[1];
        bucket_search<1>(bnd, n, g.top, b, pos);
        const uint32_t k = pos[0] - 1u;
        if (k >= nb) return;
        const uint64_t v = U64 ? ((const uint64_t *)g.vcol)[row] : widen_value<false>((uint32_t)((const int32_t *)g.vcol)[row]);
        const uint64_t img = bucket_image<U64>(v);
        if constexpr (PATH == BUCKET_LDS) t.add(k, v, img);
        else bucket_global_add(g.out, nb, k, 1, v, img, img);
    });
    if constexpr (PATH == BUCKET_LDS) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < nb; i += kBlock)
            if (t.cnt[i]) bucket_global_add(g.out, nb, i, t.cnt[i], t.sum[i], t.mn[i], t.mx[i]);
    }
}

}  // namespace

// bins_kernels.hpp -- device code of every grouped query that fills a dense array of bins: grouped COUNT(*), COUNT / SUM /
// MIN / MAX of a value column (overall or per group), GROUP BY buckets, and the dense form of GROUP BY two columns
// (included once by pqps_hip.hip, after fused_common.hpp).
//
// No counterpart in the reference (its engines have no aggregates).  One scan kernel template and one list kernel template;
// an instance is picked by three things.
//
// Where the bin of a row comes from (BinSource):
//   BIN_NONE           no GROUP BY: one bin
//   BIN_COLUMN         (value - bin_base) in 32-bit arithmetic -- the dictionary code of a string column, the value minus the
//                      column's minimum for an i32 column, 0 / 1 for sudo_used
//   BIN_BUCKET_LDS /   that bin, then its BUCKET: a contiguous run of bins, given by the ascending u32 run starts
//   BIN_BUCKET_GLOBAL  bounds[0 .. n_bins] whose last entry is the domain (hipBucketBounds makes them):
//                          bucket(b) = (number of entries of bounds[0 .. n_bins] that are <= b) - 1
//                      The count is a branch-free upper-bound search (bucket_search): ceil(log2(n_bins + 2)) rounds, each one
//                      clamped load, a compare and a conditional add; the 16 rows a lane holds of a step are 16 independent
//                      searches advanced round by round, so the 16 loads of a round are in flight together.  The bounds are
//                      copied into LDS once per workgroup whenever n_bins + 1 words fit beside the table (_LDS: up to 16383
//                      buckets), otherwise read from global memory (at most 256 KiB: L2-resident).
//   BIN_PAIR           bin_a * n_b + bin_b of two columns, each as BIN_COLUMN; D = n_a * n_b bins (computed in 64 bits by
//                      the host: 65 536 x 65 536 is 2^32)
// A row is left out when its bin is not below n_bins: a value outside [bin_base, bin_base + n_bins), a bin at or past the
// bucket domain (every entry of bounds is <= it), a pair with either part out of its range (0xFFFFFFFF).  Whatever the
// columns or bounds hold, nothing is indexed out of range.
//
// What a bin holds (BinValue):
//   BINS_COUNT         a u32 count
//   BINS_I32 /         four u64 words, one accumulator form for both value widths:
//   BINS_U64             count  matching rows
//                        sum    the value sign-extended (i32) or as is (u64), added mod 2^64
//                        min    the minimum of the order-preserving u64 IMAGE of the value: (u64)(i64)v ^ 2^63 for i32, v
//                               itself for u64
//                        max    the maximum of the image
//                      so that every update is a native 64-bit add / unsigned min / unsigned max (ds_add_u64, ds_min_u64,
//                      ds_max_u64, global_atomic_add_x2 / umin_x2 / umax_x2 -- no compare-and-swap loops).  The host undoes
//                      the image.
//
// Where the bins live while a workgroup runs (BinPath; the host picks by the number of bins, limits below):
//   BINS_REGS    counts of D <= 16: per-lane counters in VGPRs (8-bit fields of two u64 per step, unpacked into 16 u32
//                counters), wave sums on the DPP path (wave_sum_u32), workgroup sum through LDS.  A value without GROUP BY:
//                per-lane registers, a wave reduction (shuffles, once per workgroup), the 4 waves through LDS.
//   BINS_LDS     a table in dynamic LDS (BinsLds: 4 B per count bin, 28 B per value bin), 64 KiB at most with the bounds
//                beside it, so that two workgroups fit in a CU's 160 KiB
//   BINS_GLOBAL  global atomics per matching row straight into the output (one lane per scattered address: an order of
//                magnitude below the shaped-atomic rate -- this path is for correctness at high cardinality, not for speed)
//   BINS_WIDE    any number of bins (BIN_COLUMN only; the top-N groups' route above kBinsMax): the bins in global memory as
//                BINS_GLOBAL's, behind a write-combining FRONT in LDS (BinsFront): a direct-mapped table of `front` slots
//                (a power of two; 8 B per count slot, 32 B per value slot, kBinsLdsBytes at most), slot = bin & (front - 1),
//                each a tag (the bin, all ones = free) and an accumulator.  A lane claims the slot with ONE compare-and-swap
//                on the tag; where the slot was free or already held its bin the row is added in LDS, otherwise it goes
//                to the global bins with the atomics of BINS_GLOBAL.  Nothing is evicted -- the first bin to arrive keeps
//                its slot, and a bin that owns a third of the rows arrives early -- and the workgroup ends by flushing
//                every claimed slot with one global atomic per field.  front == 0: no table, BINS_GLOBAL's atomics alone.
// REGS and LDS end the workgroup's loop with plain coalesced stores of its bins into a partial row of its own
// (store-and-sum rather than atomics: thousands of workgroups adding to the same few bin words would queue at the memory
// side): [gridDim.x][stride] u32 counts or [gridDim.x][4][n_bins] u64 fields; group_sum_kernel / agg_sum_kernel add the rows
// up, one atomic per bin (and field) per 64 rows.  The grid is persistent (a few workgroups per CU), so the partials are
// grid x D words, not table-sized.  No same-address global atomic per row or per wave on those paths.
//
// Fused scan (bins_scan_kernel): the shared scan loop (fused_common.hpp) with one round of loads of the value column (one
// ld_x4 per 256-row chunk for an i32 value, two for command_id) and of the bin column(s) per step that holds a match.
// List form (bins_list_kernel): the same bins over an ID list (index probes, several passes, a shard's list): the columns
// gathered per listed row, a workgroup table flushed with one atomic per (field of a) bin that has rows.
// Bounds (pqps_column_bounds): min / max of an i32 column.
#pragma once

namespace {

enum BinSource { BIN_NONE = 0, BIN_COLUMN = 1, BIN_BUCKET_LDS = 2, BIN_BUCKET_GLOBAL = 3, BIN_PAIR = 4 };
enum BinPath { BINS_REGS = 0, BINS_LDS = 1, BINS_GLOBAL = 2, BINS_WIDE = 3 };
enum BinValue { BINS_COUNT = 0, BINS_I32 = 1, BINS_U64 = 2 };

constexpr uint32_t kBinsMax = 65536;
constexpr uint32_t kBinsSmall = 16;                                     // counts in registers
constexpr uint32_t kBinsLdsBytes = 64u << 10;                           // dynamic LDS of one workgroup: two per CU
constexpr uint32_t kCountBinBytes = 4;                                  // u32 count
constexpr uint32_t kAggBinBytes = 3 * 8 + 4;                            // u64 sum / min / max, u32 count
constexpr uint32_t kCountLdsBins = kBinsLdsBytes / kCountBinBytes;      // 16384
constexpr uint32_t kAggLdsBins = 2304;                                  // 64 512 B of LDS
constexpr uint32_t kBucketCountLds = (kBinsLdsBytes - 4) / (kCountBinBytes + 4);   // 8191: bins + bounds + the sentinel
constexpr uint32_t kBucketAggLds = (kBinsLdsBytes - 4) / (kAggBinBytes + 4);       // 2047: table + bounds + the sentinel
constexpr uint32_t kBucketBoundsLds = kBinsLdsBytes / 4 - 1;            // 16383: the bounds alone (GLOBAL bins)
constexpr uint32_t kWideCountSlots = kBinsLdsBytes / (kCountBinBytes + 4);    // 8192: u32 tag + u32 count
constexpr uint32_t kWideAggSlots = kBinsLdsBytes / (kAggBinBytes + 4);        // 2048: u32 tag + the 28-byte accumulator
constexpr uint32_t kWideFree = 0xFFFFFFFFu;                              // tag of a free slot (a bin is below n_bins <= 2^32 - 1)
constexpr uint32_t kCompactTile = 1024;                                 // bins one wave of the compaction kernels takes
constexpr uint32_t kAggFields = 4;                                      // count, sum, min image, max image
constexpr uint32_t kGroupSumParts = 64;            // partial rows one workgroup of group_sum_kernel adds up
constexpr uint32_t kAggSumParts = 64;              // partial rows one workgroup of agg_sum_kernel combines

// How a row gets its bin: the part of the arguments the scan and the list kernels share.
struct BinSourceArgs {
    const void *gcol;                // bin column (bytes, u16, u32 or a bit plane); a pair's first; unused by BIN_NONE
    const void *gcol2;               // a pair's second column
    const uint32_t *bounds;          // buckets: n_bins + 1 ascending run starts in bin space, the last one the domain
    uint32_t gwidth_log2, gwidth2_log2;   // 0, 1, 2 or kWidthLog2Bits
    uint32_t bin_base, bin_base2;
    uint32_t n_a, n_b;               // a pair: D_a, D_b; n_bins = n_a * n_b
    uint32_t n_bins;                 // D; buckets: the number of buckets
    uint32_t top;                    // buckets: the largest power of two <= n_bins + 1, the first stride of the search
};

struct BinsArgs {
    EvalArgs e;                      // the WHERE, as the COUNT kernels take it -- first: the scan loop reads it in place
    BinSourceArgs src;
    const void *vcol;                // value column: i32 or u64; unused by BINS_COUNT
    void *out;                       // GLOBAL: n_bins u32 bins (zeroed) / [4][n_bins] u64 fields (initialised before the launch)
    void *parts;                     // REGS / LDS: [gridDim.x][stride] u32 / [gridDim.x][4][n_bins] u64 partial rows
    uint32_t stride;                 // BINS_COUNT: words per partial row (n_bins rounded up to 64)
    uint32_t front;                  // WIDE: slots of the LDS front (a power of two), 0 = none
};

struct BinsListArgs {
    BinSourceArgs src;
    const void *vcol;
    const uint32_t *ids;
    const uint64_t *count;
    void *out;                       // n_bins u32 bins (zeroed) / [4][n_bins] u64 fields (initialised before the launch)
    uint64_t n_rows, capacity;
    uint32_t id_base;
    uint32_t front;                  // WIDE: slots of the LDS front (a power of two), 0 = none
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

// the bin of (a, b), or 0xFFFFFFFF when either part is out of its range
__device__ __forceinline__ uint32_t pair_bin(uint32_t a, uint32_t b, uint32_t a_base, uint32_t b_base, uint32_t n_a, uint32_t n_b) {
    const uint32_t ba = a - a_base, bb = b - b_base;
    return ba < n_a && bb < n_b ? ba * n_b + bb : 0xFFFFFFFFu;
}

// The bins of rows (not BIN_NONE).  Reads only the arguments its SRC uses; `lds`: room for the bounds of BIN_BUCKET_LDS,
// copied here (the caller syncs).
template <int SRC>
struct Binner {
    static constexpr bool BUCKETS = SRC == BIN_BUCKET_LDS || SRC == BIN_BUCKET_GLOBAL;
    const char *col, *col2;
    const uint32_t *bnd;
    uint32_t wl, wl2, base, base2, n_a, n_b, n, top;

    template <class Args>
    __device__ __forceinline__ Binner(const Args &g, uint32_t *lds) {
        col = (const char *)g.gcol; wl = g.gwidth_log2; base = g.bin_base;
        if constexpr (SRC == BIN_PAIR) {
            col2 = (const char *)g.gcol2; wl2 = g.gwidth2_log2; base2 = g.bin_base2; n_a = g.n_a; n_b = g.n_b;
        }
        if constexpr (BUCKETS) {
            n = g.n_bins + 1; top = g.top; bnd = g.bounds;
            if constexpr (SRC == BIN_BUCKET_LDS) {
                for (uint32_t i = threadIdx.x; i < n; i += kBlock) lds[i] = g.bounds[i];
                bnd = lds;
            }
        }
    }

    // column values minus the base -> bins (one column and buckets)
    template <int N>
    __device__ __forceinline__ void finish(uint32_t (&bin)[N]) const {
        if constexpr (BUCKETS) {
            uint32_t pos[N];
            bucket_search<N>(bnd, n, top, bin, pos);
#pragma unroll
            for (int p = 0; p < N; p++) bin[p] = pos[p] - 1u;
        }
    }

    // the bins of a lane's 16 rows of one full step, bin[p] <-> match bit p
    template <bool NT>
    __device__ __forceinline__ void step(uint64_t step_row0, uint32_t lane, uint32_t (&bin)[16]) const {
        load_step_u32<NT>(col, wl, step_row0, lane, bin);
        if constexpr (SRC == BIN_PAIR) {
            uint32_t bv[16];
            load_step_u32<NT>(col2, wl2, step_row0, lane, bv);
#pragma unroll
            for (int p = 0; p < 16; p++) bin[p] = pair_bin(bin[p], bv[p], base, base2, n_a, n_b);
        } else {
#pragma unroll
            for (int p = 0; p < 16; p++) bin[p] -= base;
            finish(bin);
        }
    }

    // the bin of row `row`
    __device__ __forceinline__ uint32_t row(uint64_t row) const {
        const uint32_t a = gather_narrow(col, wl, row);
        if constexpr (SRC == BIN_PAIR) {
            return pair_bin(a, gather_narrow(col2, wl2, row), base, base2, n_a, n_b);
        } else {
            uint32_t bin[1] = { a - base };
            finish(bin);
            return bin[0];
        }
    }
};

// the order-preserving image of the value a sum adds (widen_value)
template <bool U64> __device__ __forceinline__ uint64_t agg_image(uint64_t wide) {
    if constexpr (U64) return wide;
    else return wide ^ 0x8000000000000000ull;
}

// value of row `row` of an i32 or u64 column, widened
template <bool U64> __device__ __forceinline__ uint64_t gather_value(const void *vcol, uint64_t row) {
    return U64 ? ((const uint64_t *)vcol)[row] : widen_value<false>((uint32_t)((const int32_t *)vcol)[row]);
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

// the four fields of bin b of out[4][n_bins]: the GLOBAL path, the list flushes, agg_sum_kernel
__device__ __forceinline__ void agg_global_add(void *out, uint64_t nb, uint32_t b, uint64_t cnt, uint64_t sum, uint64_t mn, uint64_t mx) {
    unsigned long long *o = (unsigned long long *)out;
    atomicAdd(&o[b], (unsigned long long)cnt);
    atomicAdd(&o[nb + b], (unsigned long long)sum);
    atomicMin(&o[2 * nb + b], (unsigned long long)mn);
    atomicMax(&o[3 * nb + b], (unsigned long long)mx);
}

// The bins of a workgroup in LDS, nb of them: with a value u64 sum / min / max arrays, then (always) the u32 counts.  What
// follows the counts (end) is free for the bounds.
template <int VAL>
struct BinsLds {
    static constexpr bool VALUED = VAL != BINS_COUNT, U64 = VAL == BINS_U64;
    unsigned long long *sum, *mn, *mx;
    uint32_t *cnt, *end;
    __device__ __forceinline__ BinsLds(void *base, uint32_t nb) {
        if constexpr (VALUED) { sum = (unsigned long long *)base; mn = sum + nb; mx = mn + nb; cnt = (uint32_t *)(mx + nb); }
        else cnt = (uint32_t *)base;
        end = cnt + nb;
    }
    __device__ __forceinline__ void clear(uint32_t nb) const {
        for (uint32_t i = threadIdx.x; i < nb; i += kBlock) {
            if constexpr (VALUED) { sum[i] = 0; mn[i] = ~0ull; mx[i] = 0; }
            cnt[i] = 0;
        }
    }
    // one row with the (widened) value `wide` into bin b
    __device__ __forceinline__ void add(uint32_t b, uint64_t wide) const {
        atomicAdd(&cnt[b], 1u);
        if constexpr (VALUED) {
            atomicAdd(&sum[b], (unsigned long long)wide);
            atomicMin(&mn[b], (unsigned long long)agg_image<U64>(wide));
            atomicMax(&mx[b], (unsigned long long)agg_image<U64>(wide));
        }
    }
    // the workgroup's partial row (after a sync): plain stores
    __device__ __forceinline__ void store_row(void *parts, uint32_t stride, uint32_t nb) const {
        if constexpr (VALUED) {
            uint64_t *row = (uint64_t *)parts + (uint64_t)blockIdx.x * kAggFields * nb;
            for (uint32_t i = threadIdx.x; i < nb; i += kBlock) {
                row[i] = cnt[i]; row[nb + i] = sum[i]; row[2 * nb + i] = mn[i]; row[3 * nb + i] = mx[i];
            }
        } else {
            uint32_t *row = (uint32_t *)parts + (uint64_t)blockIdx.x * stride;
            for (uint32_t i = threadIdx.x; i < stride; i += kBlock) row[i] = i < nb ? cnt[i] : 0u;   // bins past D are zeros
        }
    }
    // into the output (after a sync): one atomic per (field of a) bin that has rows
    __device__ __forceinline__ void flush(void *out, uint32_t nb) const {
        for (uint32_t i = threadIdx.x; i < nb; i += kBlock) {
            if (!cnt[i]) continue;
            if constexpr (VALUED) agg_global_add(out, nb, i, cnt[i], sum[i], mn[i], mx[i]);
            else atomicAdd(&((uint32_t *)out)[i], cnt[i]);
        }
    }
};

// The write-combining front of BINS_WIDE: `slots` accumulators (a BinsLds table) and, behind them, their u32 tags.
template <int VAL>
struct BinsFront {
    static constexpr bool VALUED = VAL != BINS_COUNT, U64 = VAL == BINS_U64;
    BinsLds<VAL> t;
    uint32_t *tag;
    uint32_t slots;
    __device__ __forceinline__ BinsFront(void *base, uint32_t n) : t(base, n), tag(t.end), slots(n) {}
    __device__ __forceinline__ void clear() const {
        t.clear(slots);
        for (uint32_t i = threadIdx.x; i < slots; i += kBlock) tag[i] = kWideFree;
    }
    // one row with the value `wide` into bin b < nb: its slot where the lane owns or shares it, else the global bins
    __device__ __forceinline__ void add(void *out, uint32_t nb, uint32_t b, uint64_t wide) const {
        if (slots) {
            const uint32_t s = b & (slots - 1u);
            const uint32_t was = atomicCAS(&tag[s], kWideFree, b);
            if (was == kWideFree || was == b) { t.add(s, wide); return; }
        }
        if constexpr (VALUED) agg_global_add(out, nb, b, 1, wide, agg_image<U64>(wide), agg_image<U64>(wide));
        else atomicAdd(&((uint32_t *)out)[b], 1u);
    }
    // every claimed slot into the output (after a sync): one atomic per field
    __device__ __forceinline__ void flush(void *out, uint32_t nb) const {
        for (uint32_t i = threadIdx.x; i < slots; i += kBlock) {
            const uint32_t b = tag[i];
            if (b == kWideFree) continue;
            if constexpr (VALUED) agg_global_add(out, nb, b, t.cnt[i], t.sum[i], t.mn[i], t.mx[i]);
            else atomicAdd(&((uint32_t *)out)[b], t.cnt[i]);
        }
    }
};

// one row with the value `wide` into bin b < nb: the LDS table, or the output in global memory
template <int PATH, int VAL>
__device__ __forceinline__ void bins_add(const BinsLds<VAL> &t, void *out, uint32_t nb, uint32_t b, uint64_t wide) {
    if constexpr (PATH == BINS_LDS) t.add(b, wide);
    else if constexpr (VAL == BINS_COUNT) atomicAdd(&((uint32_t *)out)[b], 1u);
    else agg_global_add(out, nb, b, 1, wide, agg_image<VAL == BINS_U64>(wide), agg_image<VAL == BINS_U64>(wide));
}

// Dynamic LDS: [table, LDS path][bounds, n_bins + 1 words, BIN_BUCKET_LDS]
template <int SRC, int PATH, int VAL, bool NT>
__global__ __launch_bounds__(kBlock, 1) void bins_scan_kernel(const BinsArgs) {
    constexpr bool VALUED = VAL != BINS_COUNT, U64 = VAL == BINS_U64;
    static_assert(PATH != BINS_REGS || (VALUED ? SRC == BIN_NONE : SRC == BIN_COLUMN || SRC == BIN_BUCKET_LDS), "no such register path");
    static_assert(SRC != BIN_NONE || (VALUED && PATH == BINS_REGS), "no GROUP BY: one accumulator in registers");
    static_assert(PATH != BINS_WIDE || SRC == BIN_COLUMN, "the wide bins are those of one column");
    const auto &g = kernarg<BinsArgs>();
    CArgs &a = g.e;
    extern __shared__ uint64_t bins_lds[];
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t nb = g.src.n_bins;
    const char *vbase = (const char *)g.vcol;
    if constexpr (SRC == BIN_NONE) {
        uint64_t cnt = 0, sum = 0, mn = ~0ull, mx = 0;
        fused_scan_steps<NT>(a, lane, wv, [&](uint64_t step_row0, uint32_t mbits) {
            uint64_t v[16];
            load_step_u64<U64, NT>(vbase, step_row0, lane, v);
            cnt += __popc(mbits);
#pragma unroll
            for (int p = 0; p < 16; p++) {
                const bool hit = (mbits >> p) & 1u;
                const uint64_t img = agg_image<U64>(v[p]);
                sum += hit ? v[p] : 0ull;
                mn = hit && img < mn ? img : mn;
                mx = hit && img > mx ? img : mx;
            }
        });
        block_reduce_acc(cnt, sum, mn, mx);
        if (threadIdx.x == 0) {
            uint64_t *row = (uint64_t *)g.parts + (uint64_t)blockIdx.x * kAggFields;
            row[0] = cnt; row[1] = sum; row[2] = mn; row[3] = mx;
        }
    } else if constexpr (PATH == BINS_WIDE) {
        const BinsFront<VAL> f(bins_lds, g.front);
        const Binner<SRC> binner(g.src, nullptr);
        f.clear();
        __syncthreads();
        fused_scan_steps<NT>(a, lane, wv, [&](uint64_t step_row0, uint32_t mbits) {
            uint64_t v[16] = {};
            uint32_t bin[16];
            if constexpr (VALUED) load_step_u64<U64, NT>(vbase, step_row0, lane, v);
            binner.template step<NT>(step_row0, lane, bin);
#pragma unroll
            for (int p = 0; p < 16; p++)
                if (((mbits >> p) & 1u) && bin[p] < nb) f.add(g.out, nb, bin[p], v[p]);
        });
        __syncthreads();
        f.flush(g.out, nb);
    } else {
        const BinsLds<VAL> t(bins_lds, PATH == BINS_LDS ? nb : 0u);
        const Binner<SRC> binner(g.src, t.end);
        if constexpr (PATH == BINS_LDS) t.clear(nb);
        if constexpr (PATH == BINS_LDS || SRC == BIN_BUCKET_LDS) __syncthreads();
        uint32_t cnt[kBinsSmall];                               // REGS
#pragma unroll
        for (uint32_t k = 0; k < kBinsSmall; k++) cnt[k] = 0;
        fused_scan_steps<NT>(a, lane, wv, [&](uint64_t step_row0, uint32_t mbits) {
            uint64_t v[16] = {};
            uint32_t bin[16];
            if constexpr (VALUED) load_step_u64<U64, NT>(vbase, step_row0, lane, v);
            binner.template step<NT>(step_row0, lane, bin);
            if constexpr (PATH == BINS_REGS) {
                uint64_t f0 = 0, f1 = 0;                        // 8-bit fields: bins 0 .. 7 and 8 .. 15 (at most 16 rows per lane)
#pragma unroll
                for (int p = 0; p < 16; p++) {
                    const uint32_t b = bin[p];
                    const bool hit = ((mbits >> p) & 1u) && b < nb;
                    const uint64_t inc = hit ? 1ull << ((b & 7u) * 8u) : 0ull;
                    if (b < 8u) f0 += inc; else f1 += inc;
                }
#pragma unroll
                for (uint32_t k = 0; k < kBinsSmall; k++)
                    cnt[k] += (uint32_t)((k < 8 ? f0 >> (8 * k) : f1 >> (8 * (k - 8))) & 0xFFu);
            } else {
#pragma unroll
                for (int p = 0; p < 16; p++)
                    if (((mbits >> p) & 1u) && bin[p] < nb) bins_add<PATH, VAL>(t, g.out, nb, bin[p], v[p]);
            }
        });
        if constexpr (PATH == BINS_REGS) {
            __shared__ uint32_t s_small[kWaves][kBinsSmall];
#pragma unroll
            for (uint32_t k = 0; k < kBinsSmall; k++) {
                if (k < nb) {                                   // uniform
                    const uint32_t s = wave_sum_u32(cnt[k]);
                    if (lane == 0) s_small[wv][k] = s;
                }
            }
            __syncthreads();
            if (threadIdx.x < g.stride) {                       // the whole partial row: bins past D are zeros
                uint32_t s = 0;
                if (threadIdx.x < nb)
                    for (uint32_t w = 0; w < (uint32_t)kWaves; w++) s += s_small[w][threadIdx.x];
                ((uint32_t *)g.parts)[(uint64_t)blockIdx.x * g.stride + threadIdx.x] = s;
            }
        } else if constexpr (PATH == BINS_LDS) {
            __syncthreads();
            t.store_row(g.parts, g.stride, nb);
        }
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

// The bins over an ID list: ids[0 .. min(*count, capacity)), row = id - id_base.  REGS (no GROUP BY): per-lane registers
// reduced per workgroup, one atomic per field and workgroup; LDS: a workgroup table flushed at the end; GLOBAL: atomics per
// row; WIDE: the front, flushed at the end.  Dynamic LDS as the scan's.
template <int SRC, int PATH, int VAL>
__global__ __launch_bounds__(kBlock) void bins_list_kernel(const BinsListArgs g) {
    constexpr bool VALUED = VAL != BINS_COUNT, U64 = VAL == BINS_U64;
    static_assert((PATH == BINS_REGS) == (SRC == BIN_NONE) && (SRC != BIN_NONE || VALUED), "registers: no GROUP BY, and only then");
    extern __shared__ uint64_t bins_lds[];
    const uint32_t nb = g.src.n_bins;
    if constexpr (SRC == BIN_NONE) {
        uint64_t cnt = 0, sum = 0, mn = ~0ull, mx = 0;
        for_each_listed_row(g.ids, g.count, g.capacity, g.id_base, g.n_rows, [&](uint64_t row) {
            const uint64_t v = gather_value<U64>(g.vcol, row), img = agg_image<U64>(v);
            cnt++; sum += v;
            mn = img < mn ? img : mn;
            mx = img > mx ? img : mx;
        });
        block_reduce_acc(cnt, sum, mn, mx);
        if (threadIdx.x == 0 && cnt) agg_global_add(g.out, 1, 0, cnt, sum, mn, mx);
    } else if constexpr (PATH == BINS_WIDE) {
        const BinsFront<VAL> f(bins_lds, g.front);
        const Binner<SRC> binner(g.src, nullptr);
        f.clear();
        __syncthreads();
        for_each_listed_row(g.ids, g.count, g.capacity, g.id_base, g.n_rows, [&](uint64_t row) {
            const uint32_t b = binner.row(row);
            if (b >= nb) return;
            uint64_t v = 0;
            if constexpr (VALUED) v = gather_value<U64>(g.vcol, row);
            f.add(g.out, nb, b, v);
        });
        __syncthreads();
        f.flush(g.out, nb);
    } else {
        const BinsLds<VAL> t(bins_lds, PATH == BINS_LDS ? nb : 0u);
        const Binner<SRC> binner(g.src, t.end);
        if constexpr (PATH == BINS_LDS) t.clear(nb);
        if constexpr (PATH == BINS_LDS || SRC == BIN_BUCKET_LDS) __syncthreads();
        for_each_listed_row(g.ids, g.count, g.capacity, g.id_base, g.n_rows, [&](uint64_t row) {
            const uint32_t b = binner.row(row);
            if (b >= nb) return;
            uint64_t v = 0;
            if constexpr (VALUED) v = gather_value<U64>(g.vcol, row);
            bins_add<PATH, VAL>(t, g.out, nb, b, v);
        });
        if constexpr (PATH == BINS_LDS) {
            __syncthreads();
            t.flush(g.out, nb);
        }
    }
}

// The bins of a wide answer into compact runs (pqps_bins_compact): two launches with an exclusive scan of tile_runs[0 ..
// tiles] between them -- no workgroup waits for another.  A wave takes the tiles wave, wave + n_waves, ... of kCompactTile
// bins, 64 bins a round; a bin has rows when its count (u32 counts, or the first of the [4][n_bins] u64 fields) is not 0.
template <bool VALUED>
__device__ __forceinline__ uint64_t compact_count_of(const void *bins, uint64_t b) {
    return VALUED ? ((const uint64_t *)bins)[b] : (uint64_t)((const uint32_t *)bins)[b];
}

// tile_runs[t] = the bins with rows among [t * kCompactTile, (t + 1) * kCompactTile); tile_runs[tiles] = 0 (the scan leaves
// the number of runs there)
template <bool VALUED>
__global__ __launch_bounds__(kBlock) void bins_compact_count_kernel(const void *__restrict__ bins, uint64_t n_bins, uint64_t tiles,
                                                                    uint32_t *tile_runs) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t n_waves = (uint64_t)gridDim.x * kWaves;
    for (uint64_t t = (uint64_t)blockIdx.x * kWaves + (threadIdx.x >> 6); t <= tiles; t += n_waves) {
        uint32_t c = 0;
        for (uint32_t r = 0; r < kCompactTile / 64 && t < tiles; r++) {
            const uint64_t b = t * kCompactTile + r * 64u + lane;
            c += (uint32_t)__popcll(__ballot(b < n_bins && compact_count_of<VALUED>(bins, b) != 0));
        }
        if (lane == 0) tile_runs[t] = c;
    }
}

// out: keys[n_runs], counts[n_runs], and VALUED sums / min images / max images [n_runs] each, all u64, ascending by bin:
// the run format of pqps_group_pair_sort.  first[t] = the runs in front of tile t.
template <bool VALUED>
__global__ __launch_bounds__(kBlock) void bins_compact_write_kernel(const void *__restrict__ bins, uint64_t n_bins, uint64_t tiles,
                                                                    const uint32_t *__restrict__ first, uint64_t n_runs, uint64_t *out) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t lt_mask = (1ull << lane) - 1ull;
    const uint64_t n_waves = (uint64_t)gridDim.x * kWaves;
    for (uint64_t t = (uint64_t)blockIdx.x * kWaves + (threadIdx.x >> 6); t < tiles; t += n_waves) {
        uint64_t at = first[t];
        for (uint32_t r = 0; r < kCompactTile / 64; r++) {
            const uint64_t b = t * kCompactTile + r * 64u + lane;
            const uint64_t c = b < n_bins ? compact_count_of<VALUED>(bins, b) : 0ull;
            const uint64_t has = __ballot(c != 0);
            const uint64_t g = at + (uint64_t)__popcll(has & lt_mask);
            if (c != 0 && g < n_runs) {                         // (g < n_runs always: first[] counted the same bins)
                out[g] = b;
                out[n_runs + g] = c;
                if constexpr (VALUED) {
                    const uint64_t *f = (const uint64_t *)bins;
                    out[2 * n_runs + g] = f[n_bins + b];
                    out[3 * n_runs + g] = f[2 * n_bins + b];
                    out[4 * n_runs + g] = f[3 * n_bins + b];
                }
            }
            at += (uint64_t)__popcll(has);
        }
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

// group_pair_kernels.hpp -- device code of the sparse form of GROUP BY two columns: COUNT(*), or COUNT / SUM / MIN / MAX of a
// value column, per pair of values that occurs (included once by pqps_hip.hip, after bins_kernels.hpp, whose accumulator
// helpers it reuses).  The dense form, D <= 65 536, is the BIN_PAIR source of bins_kernels.hpp.
//
// No counterpart in the reference (its engines have no aggregates).  Each column has the bins of the one-column forms --
// (value - base) in 32-bit arithmetic: a dictionary code, an i32 value minus the column's minimum, 0 / 1 -- D_a and D_b of
// them.  A row whose bin_a >= D_a or bin_b >= D_b is left out.
//
// Sparse, any D (pqps_group_pair_sort): pair_keys_kernel builds one u64 key per listed row, bin_a << 32 | bin_b, with the
// row number as payload; the stable LSD radix sort of radix_sort.hpp orders them; pair_heads_kernel counts the heads
// (key[i] != key[i-1]) of every 64-key tile, an exclusive scan of the counts gives each tile the rank of its first head
// and the number of runs; pair_runs_kernel reduces every run into out[rank].  The output is compact: one entry per pair
// that occurs.
#pragma once

namespace {

constexpr uint64_t kPairNoKey = ~0ull;             // key of a listed row outside the bins: sorts last, belongs to no run

// key[i] = bin_a << 32 | bin_b of listed row i (kPairNoKey outside the bins or the table), row[i] = id - id_base
__global__ __launch_bounds__(kBlock) void pair_keys_kernel(const void *acol, uint32_t awl, const void *bcol, uint32_t bwl,
                                                           const uint32_t *__restrict__ ids, uint64_t n, uint32_t id_base, uint64_t n_rows,
                                                           uint32_t a_base, uint32_t b_base, uint32_t n_a, uint32_t n_b,
                                                           uint64_t *key, uint32_t *rows) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t r = ids[i] - id_base;
        uint64_t k = kPairNoKey;
        if (r < n_rows) {
            const uint32_t ba = gather_narrow(acol, awl, r) - a_base, bb = gather_narrow(bcol, bwl, r) - b_base;
            if (ba < n_a && bb < n_b) k = (uint64_t)ba << 32 | bb;
        }
        key[i] = k;
        rows[i] = r;
    }
}

// The one-column form (pqps_group_sort): key[i] = the bin of listed row i, (value - base) in 32-bit arithmetic, where it is
// below n_bins (up to 2^32), kPairNoKey otherwise or outside the table; row[i] = id - id_base
__global__ __launch_bounds__(kBlock) void group_keys_kernel(const void *gcol, uint32_t gwl, const uint32_t *__restrict__ ids, uint64_t n,
                                                            uint32_t id_base, uint64_t n_rows, uint32_t base, uint64_t n_bins,
                                                            uint64_t *key, uint32_t *rows) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t r = ids[i] - id_base;
        uint64_t k = kPairNoKey;
        if (r < n_rows) {
            const uint32_t b = gather_narrow(gcol, gwl, r) - base;
            if (b < n_bins) k = b;
        }
        key[i] = k;
        rows[i] = r;
    }
}

// element i of the sorted keys starts a run
__device__ __forceinline__ bool pair_is_head(const uint64_t *__restrict__ key, uint64_t i, uint64_t k) {
    return k != kPairNoKey && (i == 0 || key[i - 1] != k);
}

// heads[t] = the heads among keys [64 t, 64 t + 64); heads[tiles] = 0 (the exclusive scan leaves the number of runs there)
__global__ __launch_bounds__(kBlock) void pair_heads_kernel(const uint64_t *__restrict__ key, uint64_t n, uint64_t tiles, uint32_t *heads) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t n_waves = (uint64_t)gridDim.x * kWaves;
    for (uint64_t t = (uint64_t)blockIdx.x * kWaves + (threadIdx.x >> 6); t <= tiles; t += n_waves) {
        const uint64_t i = t * 64 + lane;
        const bool head = t < tiles && i < n && pair_is_head(key, i, key[i]);
        const uint32_t c = (uint32_t)__popcll(__ballot(head));
        if (lane == 0) heads[t] = c;
    }
}

// One run's totals into out[rank]: a wave reduction of the per-lane accumulators, then one atomic per field by lane 0.
// o = the counts array; sums, min images and max images follow it, n_runs entries each.  Resets the accumulators.
template <int VAL>
__device__ __forceinline__ void pair_flush_run(unsigned long long *o, uint64_t n_runs, uint64_t rank, uint64_t &cnt, uint64_t &sum,
                                               uint64_t &mn, uint64_t &mx) {
    if (cnt == 0) return;                                       // uniform
    if constexpr (VAL == BINS_COUNT) {
        if ((threadIdx.x & 63) == 0) atomicAdd(&o[rank], (unsigned long long)cnt);
    } else {
        uint64_t c = 0;
        wave_reduce_acc(c, sum, mn, mx);
        if ((threadIdx.x & 63) == 0) {
            atomicAdd(&o[rank], (unsigned long long)cnt);
            atomicAdd(&o[n_runs + rank], (unsigned long long)sum);
            atomicMin(&o[2 * n_runs + rank], (unsigned long long)mn);
            atomicMax(&o[3 * n_runs + rank], (unsigned long long)mx);
        }
        sum = 0; mn = ~0ull; mx = 0;
    }
    cnt = 0;
}

// Run reduction over the sorted (key, row) pairs.  The rank of an element is the number of heads up to and including it,
// minus one: first[t] (heads in front of tile t) + the heads of the tile up to its lane - 1.  Every wave walks a contiguous
// range of 64-key tiles.  A tile without a head behind lane 0 belongs to ONE run: its rows go to per-lane accumulators
// (the count to a wave-uniform one), carried from tile to tile and flushed (pair_flush_run) when the key changes or the
// range ends, so a run that spans waves combines correctly.  A tile that holds several runs is reduced by a segmented scan
// over its lanes (segments = runs), the last lane of each segment doing that run's atomics.  The value is gathered by row
// number here.  Head lanes store the run's key.  out: keys[n_runs], counts[n_runs], and with a value sums / min images /
// max images [n_runs] each (counts and sums zeroed, min images ~0, max images 0 before the launch).
template <int VAL>
__global__ __launch_bounds__(kBlock) void pair_runs_kernel(const uint64_t *__restrict__ key, const uint32_t *__restrict__ rows, uint64_t n,
                                                           uint64_t tiles, const uint32_t *__restrict__ first, const void *vcol,
                                                           uint64_t n_runs, uint64_t *out) {
    constexpr bool U64 = VAL == BINS_U64;
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t n_waves = (uint64_t)gridDim.x * kWaves;
    const uint64_t wave = (uint64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    const uint64_t per = (tiles + n_waves - 1) / n_waves;
    uint64_t t0 = wave * per, t1 = t0 + per;
    if (t1 > tiles) t1 = tiles;
    unsigned long long *o = (unsigned long long *)out + n_runs;
    const uint64_t le_mask = lane == 63 ? ~0ull : (1ull << (lane + 1)) - 1ull;
    uint64_t run_cnt = 0, run_rank = 0;                         // the carried run (uniform)
    uint64_t sum = 0, mn = ~0ull, mx = 0;                       // ... its per-lane accumulators
    for (uint64_t t = t0; t < t1; t++) {
        const uint64_t i = t * 64 + lane;
        const uint64_t k = i < n ? key[i] : kPairNoKey;
        const bool valid = k != kPairNoKey;
        const bool head = pair_is_head(key, i, k);
        const uint64_t hb = __ballot(head), vb = __ballot(valid);
        if (vb == 0) break;                                     // uniform: rows outside the bins sort last, nothing follows them
        const uint64_t rank = (uint64_t)first[t] + (uint64_t)__popcll(hb & le_mask) - 1u;   // (of a valid lane)
        if (head) out[rank] = k;
        uint64_t v = 0, lo = ~0ull, hi = 0;
        if constexpr (VAL != BINS_COUNT) {
            if (valid) {
                const uint32_t r = rows[i];
                v = U64 ? ((const uint64_t *)vcol)[r] : widen_value<false>((uint32_t)((const int32_t *)vcol)[r]);
                lo = hi = agg_image<U64>(v);
            }
        }
        if ((hb & ~1ull) == 0) {                                // uniform: one run in the tile, lane 0 is valid
            const uint64_t r0 = (uint64_t)first[t] + (hb & 1ull) - 1u;
            if (r0 != run_rank) pair_flush_run<VAL>(o, n_runs, run_rank, run_cnt, sum, mn, mx);
            run_rank = r0;
            run_cnt += (uint64_t)__popcll(vb);
            if constexpr (VAL != BINS_COUNT) {
                sum += v;
                mn = lo < mn ? lo : mn;
                mx = hi > mx ? hi : mx;
            }
            continue;
        }
        // several runs in the tile: a segmented inclusive scan, segments starting at lane 0 and at every head
        const uint32_t seg0 = 63u - (uint32_t)__clzll((long long)((hb | 1ull) & le_mask));   // first lane of this lane's segment
        if constexpr (VAL != BINS_COUNT) {
#pragma unroll
            for (uint32_t off = 1; off < 64; off <<= 1) {
                const int src = (int)((lane - off) & 63u);
                const uint64_t s = __shfl((unsigned long long)v, src, 64);
                const uint64_t m = __shfl((unsigned long long)lo, src, 64);
                const uint64_t x = __shfl((unsigned long long)hi, src, 64);
                if (lane >= off && lane - off >= seg0) {
                    v += s;
                    lo = m < lo ? m : lo;
                    hi = x > hi ? x : hi;
                }
            }
        }
        // the last valid lane of a segment: the next lane starts one, or is not valid
        const bool last = valid && (lane == 63 || ((hb >> (lane + 1)) & 1ull) || !((vb >> (lane + 1)) & 1ull));
        if (last) {
            atomicAdd(&o[rank], (unsigned long long)(lane - seg0 + 1u));
            if constexpr (VAL != BINS_COUNT) {
                atomicAdd(&o[n_runs + rank], (unsigned long long)v);
                atomicMin(&o[2 * n_runs + rank], (unsigned long long)lo);
                atomicMax(&o[3 * n_runs + rank], (unsigned long long)hi);
            }
        }
        // the carried run ends here (where it continues into the tile's first segment its atomics combine with that segment's)
        pair_flush_run<VAL>(o, n_runs, run_rank, run_cnt, sum, mn, mx);
    }
    pair_flush_run<VAL>(o, n_runs, run_rank, run_cnt, sum, mn, mx);   // the range ends
}

}  // namespace

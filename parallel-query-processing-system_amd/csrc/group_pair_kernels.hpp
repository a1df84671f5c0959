// group_pair_kernels.hpp -- device code of GROUP BY two columns: COUNT(*), or COUNT / SUM / MIN / MAX of a value column, per
// pair of values (included once by pqps_hip.hip, after fused_common.hpp and its four siblings, whose helpers it reuses).
//
// No counterpart in the reference (its engines have no aggregates).  Each column has the bins of the one-column forms --
// (value - base) in 32-bit arithmetic: a dictionary code, an i32 value minus the column's minimum, 0 / 1 -- D_a and D_b of
// them; the bin of a row is bin_a * D_b + bin_b, D = D_a * D_b in all (computed in 64 bits by the host: 65 536 x 65 536 is
// 2^32).  A row whose bin_a >= D_a or bin_b >= D_b is left out.
//
// Dense, D <= 65 536.  Fused scan (pqps_filter_group_pair): the shared scan loop (fused_common.hpp) with one round of loads
// of A, one of B, and one of the value column per step that holds a match.  ONE kernel template, pair_scan_kernel<PATH,
// VAL, NT>; VAL = PAIR_COUNT compiles the value loads and the four-u64 accumulator out, so COUNT(*) per pair costs what
// grouped COUNT costs plus the second column:
//   PAIR_COUNT  LDS     D <= 16 384   a u32 histogram in dynamic LDS (ds_add_u32 per matching row), 64 KiB at most
//               GLOBAL  D <= 65 536   one global atomic per matching row (a correctness path, like GROUP_GLOBAL)
//   PAIR_I32 / PAIR_U64
//               LDS     D <= 2 304    the 28-byte-per-bin table of aggregate_kernels.hpp (AggLds)
//               GLOBAL  D <= 65 536   four global 64-bit atomics per matching row (like AGG_GLOBAL)
// The LDS paths end with plain stores of a partial row per workgroup (store-and-sum); the rows have the layouts of
// group_scan_kernel's and agg_scan_kernel's, so group_sum_kernel and agg_sum_kernel add them up unchanged.  No same-address
// global atomic per row or per wave on those paths.  List form (pqps_group_pair_list): the same bins over an ID list,
// both columns and the value gathered per listed row, a workgroup table flushed with one atomic per field of a bin with rows.
//
// Sparse, any D (pqps_group_pair_sort): pair_keys_kernel builds one u64 key per listed row, bin_a << 32 | bin_b, with the
// row number as payload; the stable LSD radix sort of radix_sort.hpp orders them; pair_heads_kernel counts the heads
// (key[i] != key[i-1]) of every 64-key tile, an exclusive scan of the counts gives each tile the rank of its first head
// and the number of runs; pair_runs_kernel reduces every run into out[rank].  The output is compact: one entry per pair
// that occurs.
#pragma once

namespace {

enum PairPath { PAIR_LDS = 0, PAIR_GLOBAL = 1 };
enum PairValue { PAIR_COUNT = 0, PAIR_I32 = 1, PAIR_U64 = 2 };
constexpr uint64_t kPairNoKey = ~0ull;             // key of a listed row outside the bins: sorts last, belongs to no run

struct PairArgs {
    EvalArgs e;                      // the WHERE, as the COUNT kernels take it -- first: the scan loop reads it in place
    const void *acol, *bcol;         // group columns (bytes, u16, u32 or a bit plane)
    const void *vcol;                // value column: i32 or u64; unused by PAIR_COUNT
    uint32_t *bins;                  // PAIR_COUNT GLOBAL: D u32 bins (zeroed before the launch)
    uint64_t *out;                   // value GLOBAL: [4][D] (initialised before the launch)
    void *parts;                     // LDS: [gridDim.x][stride] u32 counts, or [gridDim.x][4][D] u64 fields
    uint32_t stride;                 // PAIR_COUNT: words per partial row (D rounded up to 64)
    uint32_t awidth_log2, bwidth_log2;   // 0, 1, 2 or kWidthLog2Bits
    uint32_t a_base, b_base;
    uint32_t n_a, n_b;               // D_a, D_b; D = n_a * n_b <= 65 536 here
};

// the bin of (a, b), or 0xFFFFFFFF when either part is out of its range
__device__ __forceinline__ uint32_t pair_bin(uint32_t a, uint32_t b, uint32_t a_base, uint32_t b_base, uint32_t n_a, uint32_t n_b) {
    const uint32_t ba = a - a_base, bb = b - b_base;
    return ba < n_a && bb < n_b ? ba * n_b + bb : 0xFFFFFFFFu;
}

template <int PATH, int VAL, bool NT>
__global__ __launch_bounds__(kBlock, 1) void pair_scan_kernel(const PairArgs) {
    const auto &g = kernarg<PairArgs>();
    CArgs &a = g.e;
    extern __shared__ uint64_t pair_lds[];                      // LDS path: the histogram or the table
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t na = g.n_a, nb = g.n_b, a0 = g.a_base, b0 = g.b_base, awl = g.awidth_log2, bwl = g.bwidth_log2;
    const uint32_t D = na * nb;
    const char *abase = (const char *)g.acol;
    const char *bbase = (const char *)g.bcol;
    const char *vbase = (const char *)g.vcol;
    uint32_t *hist = (uint32_t *)pair_lds;
    AggLds t(pair_lds, D);
    if constexpr (PATH == PAIR_LDS) {
        if constexpr (VAL == PAIR_COUNT) for (uint32_t i = threadIdx.x; i < D; i += kBlock) hist[i] = 0;
        else t.clear(D);
        __syncthreads();
    }
    fused_scan_steps<NT>(a, lane, wv, [&](uint64_t step_row0, uint32_t mbits) {
        uint32_t bin[16], bv[16];
        load_step_u32<NT>(abase, awl, step_row0, lane, bin);
        load_step_u32<NT>(bbase, bwl, step_row0, lane, bv);
#pragma unroll
        for (int p = 0; p < 16; p++) bin[p] = ((mbits >> p) & 1u) ? pair_bin(bin[p], bv[p], a0, b0, na, nb) : 0xFFFFFFFFu;
        if constexpr (VAL == PAIR_COUNT) {
#pragma unroll
            for (int p = 0; p < 16; p++) {
                if (bin[p] != 0xFFFFFFFFu) {
                    if constexpr (PATH == PAIR_LDS) atomicAdd(&hist[bin[p]], 1u);
                    else atomicAdd(&g.bins[bin[p]], 1u);
                }
            }
        } else {
            constexpr bool U64 = VAL == PAIR_U64;
            uint64_t v[16];
            load_step_u64<U64, NT>(vbase, step_row0, lane, v);
#pragma unroll
            for (int p = 0; p < 16; p++) {
                if (bin[p] != 0xFFFFFFFFu) {
                    if constexpr (PATH == PAIR_LDS) t.add(bin[p], v[p], agg_image<U64>(v[p]));
                    else agg_global_add(g.out, D, bin[p], 1, v[p], agg_image<U64>(v[p]), agg_image<U64>(v[p]));
                }
            }
        }
    });
    if constexpr (PATH == PAIR_LDS) {
        __syncthreads();
        if constexpr (VAL == PAIR_COUNT) {                      // group_scan_kernel's partial row
            uint32_t *row = (uint32_t *)g.parts + (uint64_t)blockIdx.x * g.stride;
            for (uint32_t i = threadIdx.x; i < g.stride; i += kBlock) row[i] = i < D ? hist[i] : 0u;
        } else {                                                // agg_scan_kernel's
            uint64_t *row = (uint64_t *)g.parts + (uint64_t)blockIdx.x * kAggFields * D;
            for (uint32_t i = threadIdx.x; i < D; i += kBlock) {
                row[i] = t.cnt[i]; row[D + i] = t.sum[i]; row[2 * D + i] = t.mn[i]; row[3 * D + i] = t.mx[i];
            }
        }
    }
}

// The bins over an ID list: ids[0 .. min(*count, capacity)), row = id - id_base.  LDS: a workgroup histogram / table flushed
// with one atomic per (field of a) bin that has rows; otherwise atomics per row.  PAIR_COUNT: out = D u32 bins; else
// out = [4][D] u64 fields.  out initialised before the launch.
template <bool LDS, int VAL>
__global__ __launch_bounds__(kBlock) void pair_list_kernel(const void *acol, uint32_t awl, const void *bcol, uint32_t bwl, const void *vcol,
                                                           uint64_t n_rows, const uint32_t *__restrict__ ids, const uint64_t *count,
                                                           uint64_t capacity, uint32_t id_base, uint32_t a_base, uint32_t b_base,
                                                           uint32_t n_a, uint32_t n_b, void *out) {
    extern __shared__ uint64_t pair_lds[];
    const uint32_t D = n_a * n_b;
    uint32_t *hist = (uint32_t *)pair_lds;
    uint32_t *bins = (uint32_t *)out;
    AggLds t(pair_lds, D);
    if constexpr (LDS) {
        if constexpr (VAL == PAIR_COUNT) for (uint32_t i = threadIdx.x; i < D; i += kBlock) hist[i] = 0;
        else t.clear(D);
        __syncthreads();
    }
    for_each_listed_row(ids, count, capacity, id_base, n_rows, [&](uint64_t row) {
        const uint32_t b = pair_bin(gather_narrow(acol, awl, row), gather_narrow(bcol, bwl, row), a_base, b_base, n_a, n_b);
        if (b == 0xFFFFFFFFu) return;
        if constexpr (VAL == PAIR_COUNT) {
            if constexpr (LDS) atomicAdd(&hist[b], 1u);
            else atomicAdd(&bins[b], 1u);
        } else {
            constexpr bool U64 = VAL == PAIR_U64;
            const uint64_t v = U64 ? ((const uint64_t *)vcol)[row] : widen_value<false>((uint32_t)((const int32_t *)vcol)[row]);
            if constexpr (LDS) t.add(b, v, agg_image<U64>(v));
            else agg_global_add((uint64_t *)out, D, b, 1, v, agg_image<U64>(v), agg_image<U64>(v));
        }
    });
    if constexpr (LDS) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < D; i += kBlock) {
            if constexpr (VAL == PAIR_COUNT) { if (hist[i]) atomicAdd(&bins[i], hist[i]); }
            else if (t.cnt[i]) agg_global_add((uint64_t *)out, D, i, t.cnt[i], t.sum[i], t.mn[i], t.mx[i]);
        }
    }
}

// ---- sparse path -------------------------------------------------------------------------------------------------------

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
    if constexpr (VAL == PAIR_COUNT) {
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
    constexpr bool U64 = VAL == PAIR_U64;
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
        if constexpr (VAL != PAIR_COUNT) {
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
            if constexpr (VAL != PAIR_COUNT) {
                sum += v;
                mn = lo < mn ? lo : mn;
                mx = hi > mx ? hi : mx;
            }
            continue;
        }
        // several runs in the tile: a segmented inclusive scan, segments starting at lane 0 and at every head
        const uint32_t seg0 = 63u - (uint32_t)__clzll((long long)((hb | 1ull) & le_mask));   // first lane of this lane's segment
        if constexpr (VAL != PAIR_COUNT) {
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
            if constexpr (VAL != PAIR_COUNT) {
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

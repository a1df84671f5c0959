// first_kernels.hpp -- device code of "the first row of every group" and "the first N rows of every group": per value of a
// group column, the matching rows that come first in the order of a second column (included once by pqps_hip.hip, after
// fused_common.hpp).  One kernel family: the first row is round 0 of the first N.
//
// No counterpart in the reference (SQL: DISTINCT ON, ROW_NUMBER() OVER (PARTITION BY g ORDER BY k [DESC]) <= n, argMin /
// argMax).
// The word of a row is the composite key of the top-K family (topk_kernels.hpp):
//   narrow (i32, dictionary codes, the bool bit)  (img ^ x) << 32 | table_row, img = v ^ 2^31 for i32, the code or the bit
//                                                 otherwise, x = 0xFFFFFFFF for DESC and 0 for ASC, table_row = row_base + row
// so the first row of a bin is the unsigned MINIMUM of its rows' words in both directions, ties to the lowest row number,
// and every update is one native 64-bit unsigned min (ds_min_u64, global_atomic_umin_x2 -- no compare-and-swap loop).  An
// empty bin reads all ones: no real word reaches it, since row numbers stay below 2^32 - 1.
//   wide (command_id) needs 96 bits, so it takes TWO launches of the same kernels, i.e. two scans of the WHERE:
//     pass A   best[b] = min over the bin's rows of v ^ x, x = ~0 for DESC
//     pass B   out[b]  = min of table_row over the bin's rows whose v ^ x equals best[b]
//   out[b] says whether the bin is empty (v ^ x itself may be all ones).
//
// Fused scan (pqps_filter_group_first): the shared scan loop (fused_common.hpp) with one round of key-column loads and one of
// group-column loads per step that holds a match.  Bin paths, chosen on the host by the bins D of the group column:
//   ONE    no GROUP BY   a per-lane minimum, a wave reduction (shuffles, once per workgroup), the 4 waves through LDS
//   LDS    D <= 8192     a table of 8 B per bin in dynamic LDS, 64 KiB at most (two workgroups per CU); ONE ds_min_u64 per
//                        matching row
//   GLOBAL D <= 65536    one global 64-bit atomic min per matching row straight into the output (a correctness path, like
//                        BINS_GLOBAL: one lane per scattered address)
// ONE and LDS end the workgroup's loop with plain stores of a partial row (store-and-combine);
// first_min_kernel takes the minimum of 64 rows per workgroup with one atomic per bin that has a row.  No same-address global
// atomic per row or per wave.  There is no register path for tiny D (per-lane minima of D bins, as BINS_REGS counts): D
// words of 64 bits per lane and a D-fold wave reduction buy nothing the LDS table's one ds_min_u64 does not already give.
//
// List form (pqps_group_first_list): the same words over an ID list, gathering the key column (and the group column) per
// listed row; a workgroup's LDS table is flushed with one atomic per bin that has a row.
//
// ROUNDS (pqps_filter_group_head, pqps_group_head_list).  The words are unique per row, so the r-th row of a bin is the
// minimum word STRICTLY ABOVE the bin's (r-1)-th word.  Round 0 has no floor (FLOOR_NONE): it is the first-row launch, and
// the only one that counts the matching rows.  Round r >= 1 is the same kernel with one more test per matching row,
// w > floor[b], floor = round r-1's output.  A bin whose previous word is all ones is exhausted: nothing is greater than all
// ones, so it stays all ones without a special case.  The rounds depend on each other only through device memory on one
// stream; none needs a host wait.
//   Where the floor lives:
//     FLOOR_LDS   LDS path, D <= 4096, narrow keys   in dynamic LDS beside the min table (16 B x D <= 64 KiB), filled at
//                                                    the start; the larger table is why the grid of a later round differs
//     FLOOR_MEM   ONE                                one word (a pair for command_id), read once into registers
//                 LDS, D <= 8192                     read per MATCHING row from device memory (8 B x D <= 64 KiB: it
//                                                    stays in L2)
//                 GLOBAL, D <= 65536                 the same, and one global atomic min per matching row
//   wide keys (command_id, 96 bits): each round is two passes, the floor the pair (fbest[b], frow[b]) of round r-1:
//     pass A   best[b] = min of k = v ^ x over the bin's rows with (k, row) > (fbest, frow) lexicographically
//     pass B   out[b]  = min of row over the bin's rows with k == best[b] that pass the same test
//   frow all ones means the bin is exhausted (k itself may be all ones, so this case IS tested).  The pair is read from
//   device memory on every grouped path: the wide form already scans twice per round, and a 24 B x D table would halve the
//   bins that fit LDS.
// The list form reads the floor from device memory on every path (a list is a gather per row already); the strict > makes
// an id listed twice one candidate.
//
// SORT FORM (pqps_group_head_sort).  Over a selection sorted by (group, key, row) with repeated ids removed, runs_head_flags
// marks the entries whose rank inside their run of equal group images is below `limit`: in a sorted array an entry has rank
// >= limit exactly when the entry `limit` places before it is in the same run, so keep[i] = i < limit || group[i - limit] !=
// group[i] -- no segmented scan.  list_repeat_flags marks the second and later copies of an id, which the sort leaves
// adjacent.
#pragma once

namespace {

enum FirstPath { FIRST_ONE = 0, FIRST_LDS = 1, FIRST_GLOBAL = 2 };
enum FirstMode { FIRST_NARROW = 0, FIRST_WIDE_A = 1, FIRST_WIDE_B = 2 };
enum FirstFloor { FLOOR_NONE = 0, FLOOR_LDS = 1, FLOOR_MEM = 2 };
constexpr uint32_t kFirstLdsBins = 8192;           // 8 B per bin: 64 KiB of LDS, two workgroups per CU
constexpr uint32_t kFloorLdsBins = 4096;           // 16 B per bin: min table and floor in 64 KiB of LDS
constexpr uint32_t kFirstMinParts = 64;            // partial rows one workgroup of first_min_kernel combines
constexpr uint64_t kFirstEmpty = ~0ull;

struct FirstArgs {
    EvalArgs e;                      // the WHERE, as the COUNT kernels take it -- first: the scan loop reads it in place
    const void *kcol;                // key column (narrow: bytes, u16, u32 or a bit plane; wide: u64); nullptr: every key 0
    const void *gcol;                // group column (bytes, u16, u32 or a bit plane); unused by FIRST_ONE
    uint64_t *out;                   // GLOBAL: [n_bins] (all ones before the launch)
    uint64_t *parts;                 // ONE / LDS: [gridDim.x][n_bins] partial rows
    const uint64_t *best;            // WIDE_B: pass A's [n_bins] of THIS round
    unsigned long long *count;       // FLOOR_NONE: += the matching rows (one atomic per workgroup; zeroed before the launch); may be NULL
    uint64_t kxor;                   // image xor (i32 sign flip, DESC complement)
    uint32_t kwidth_log2;            // narrow: 0, 1, 2 or kWidthLog2Bits
    uint32_t gwidth_log2;            // 0, 1, 2 or kWidthLog2Bits
    uint32_t bin_base;
    uint32_t n_bins;
    uint32_t row_base;               // table-wide row number of row 0
    const uint64_t *floor;           // a later round: the previous round's out[n_bins]
    const uint64_t *floor_best;      // and, wide, its best[n_bins]
};

// The word of a row whose raw key is `raw`: narrow (img ^ x) << 32 | row; pass A the image; pass B the row.
template <int MODE> __device__ __forceinline__ uint64_t first_word(uint64_t raw, uint64_t kxor, uint32_t table_row) {
    if constexpr (MODE == FIRST_NARROW) return ((uint64_t)(((uint32_t)raw) ^ (uint32_t)kxor) << 32) | table_row;
    else if constexpr (MODE == FIRST_WIDE_A) return raw ^ kxor;
    else return table_row;
}

// Does the row (k = v ^ x, w its word: narrow the whole word, wide the table row) lie strictly above the floor?
template <int MODE> __device__ __forceinline__ bool head_above(uint64_t k, uint64_t w, uint64_t frow, uint64_t fbest) {
    if constexpr (MODE == FIRST_NARROW) return w > frow;
    else return frow != kFirstEmpty && (k > fbest || (k == fbest && w > frow));
}

// The minimum of the workgroup's per-lane words; thread 0 returns it.
__device__ __forceinline__ uint64_t block_min_u64(uint64_t m) {
    __shared__ uint64_t s_min[kWaves];
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint64_t o = shfl_xor_u64(m, off);
        m = o < m ? o : m;
    }
    if (lane == 0) s_min[wv] = m;
    __syncthreads();
    if (threadIdx.x == 0)
        for (uint32_t w = 1; w < (uint32_t)kWaves; w++) m = s_min[w] < m ? s_min[w] : m;
    return m;
}

template <int PATH, int MODE, int FLOOR, bool NT>
__global__ __launch_bounds__(kBlock, 1) void first_scan_kernel(const FirstArgs) {
    static_assert(FLOOR != FLOOR_LDS || (PATH == FIRST_LDS && MODE == FIRST_NARROW), "the floor in LDS: narrow keys only");
    const auto &g = kernarg<FirstArgs>();
    CArgs &a = g.e;
    extern __shared__ uint64_t first_lds[];                     // LDS path: the min table [nb], FLOOR_LDS: then the floor [nb]
    unsigned long long *tab = (unsigned long long *)first_lds;
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t nb = g.n_bins, base_bin = g.bin_base, kwl = g.kwidth_log2, gwl = g.gwidth_log2, row_base = g.row_base;
    const uint64_t kxor = g.kxor;
    const char *kbase = (const char *)g.kcol;
    const char *gbase = (const char *)g.gcol;
    const uint64_t *best = g.best;
    const uint64_t *floor = g.floor, *floor_best = g.floor_best;
    unsigned long long *out = (unsigned long long *)g.out;
    if constexpr (PATH == FIRST_LDS) {
        for (uint32_t i = threadIdx.x; i < nb; i += kBlock) {
            tab[i] = kFirstEmpty;
            if constexpr (FLOOR == FLOOR_LDS) first_lds[nb + i] = floor[i];
        }
        __syncthreads();
    }
    uint64_t mine = kFirstEmpty;                                // FIRST_ONE
    uint64_t want0 = 0, frow0 = 0, fbest0 = 0;
    if constexpr (PATH == FIRST_ONE) {
        if constexpr (FLOOR != FLOOR_NONE) frow0 = floor[0];
        if constexpr (FLOOR != FLOOR_NONE && MODE != FIRST_NARROW) fbest0 = floor_best[0];
        if constexpr (MODE == FIRST_WIDE_B) want0 = best[0];
    }
    uint32_t cnt = 0;
    fused_scan_steps<NT>(a, lane, wv, [&](uint64_t step_row0, uint32_t mbits) {
        if constexpr (FLOOR == FLOOR_NONE) cnt += __popc(mbits);
        uint64_t v[16];
        if constexpr (MODE != FIRST_NARROW) {
            load_step_u64<true, NT>(kbase, step_row0, lane, v);
        } else {
            uint32_t u[16];
            if (kbase) load_step_u32<NT>(kbase, kwl, step_row0, lane, u);
            else {
#pragma unroll
                for (int p = 0; p < 16; p++) u[p] = 0;
            }
#pragma unroll
            for (int p = 0; p < 16; p++) v[p] = u[p];
        }
        uint32_t gv[16];
        if constexpr (PATH != FIRST_ONE) load_step_u32<NT>(gbase, gwl, step_row0, lane, gv);
        const uint32_t lane_row0 = row_base + (uint32_t)step_row0 + lane * kRplGeneric;
#pragma unroll
        for (int p = 0; p < 16; p++) {                          // bit p <-> row lane_row0 + (p / 4) * 256 + p % 4
            if (!((mbits >> p) & 1u)) continue;
            const uint32_t row = lane_row0 + (uint32_t)(p / 4) * 256u + (uint32_t)(p % 4);
            const uint64_t w = first_word<MODE>(v[p], kxor, row);
            const uint64_t k = v[p] ^ kxor;                     // (wide only)
            if constexpr (PATH == FIRST_ONE) {
                if constexpr (FLOOR != FLOOR_NONE) {
                    if (!head_above<MODE>(k, MODE == FIRST_NARROW ? w : (uint64_t)row, frow0, fbest0)) continue;
                }
                if constexpr (MODE == FIRST_WIDE_B) { if (k != want0) continue; }
                mine = w < mine ? w : mine;
            } else {
                const uint32_t b = gv[p] - base_bin;
                if (b >= nb) continue;
                if constexpr (FLOOR != FLOOR_NONE) {
                    uint64_t frow, fbest = 0;
                    if constexpr (FLOOR == FLOOR_LDS) frow = first_lds[nb + b];
                    else frow = floor[b];
                    if constexpr (MODE != FIRST_NARROW) fbest = floor_best[b];
                    if (!head_above<MODE>(k, MODE == FIRST_NARROW ? w : (uint64_t)row, frow, fbest)) continue;
                }
                if constexpr (MODE == FIRST_WIDE_B) { if (k != best[b]) continue; }
                if constexpr (PATH == FIRST_LDS) atomicMin(&tab[b], (unsigned long long)w);
                else atomicMin(&out[b], (unsigned long long)w);
            }
        }
    });
    if constexpr (PATH == FIRST_ONE) {
        mine = block_min_u64(mine);
        if (threadIdx.x == 0) g.parts[blockIdx.x] = mine;
    } else if constexpr (PATH == FIRST_LDS) {
        __syncthreads();
        uint64_t *row = g.parts + (uint64_t)blockIdx.x * nb;
        for (uint32_t i = threadIdx.x; i < nb; i += kBlock) row[i] = tab[i];
    }
    if constexpr (FLOOR == FLOOR_NONE) {
        if (g.count) {                                          // (uniform: a kernel argument)
            __shared__ uint32_t s_cnt[kWaves];
            const uint32_t c = wave_sum_u32(cnt);
            if (lane == 0) s_cnt[wv] = c;
            __syncthreads();
            if (threadIdx.x == 0) {
                uint64_t total = 0;
                for (uint32_t i = 0; i < (uint32_t)kWaves; i++) total += s_cnt[i];
                if (total) atomicAdd(g.count, (unsigned long long)total);
            }
        }
    }
}

// out[bin] = min(out[bin], the partial rows r of this workgroup's 64-row slice): one bin per lane, the 4 waves take 16 rows
// each, combined through LDS, one atomic per bin that has a row.  out all ones before the launch.
__global__ __launch_bounds__(kBlock) void first_min_kernel(const uint64_t *__restrict__ parts, uint32_t n_parts, uint32_t n_bins,
                                                           uint64_t *out) {
    __shared__ uint64_t s_min[kWaves][64];
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t bin = blockIdx.x * 64 + lane;
    const uint32_t r0 = blockIdx.y * kFirstMinParts + wv * (kFirstMinParts / kWaves);
    uint64_t m = kFirstEmpty;
    if (bin < n_bins) {
        for (uint32_t i = 0; i < kFirstMinParts / kWaves && r0 + i < n_parts; i++) {
            const uint64_t x = parts[(uint64_t)(r0 + i) * n_bins + bin];
            m = x < m ? x : m;
        }
    }
    s_min[wv][lane] = m;
    __syncthreads();
    if (wv == 0 && bin < n_bins) {
        for (uint32_t w = 1; w < (uint32_t)kWaves; w++) m = s_min[w][lane] < m ? s_min[w][lane] : m;
        if (m != kFirstEmpty) atomicMin((unsigned long long *)&out[bin], (unsigned long long)m);
    }
}

// The words over an ID list: ids[0 .. min(*count, capacity)), row = id - id_base, table_row = id.  gcol == nullptr: no GROUP
// BY (n_bins = 1), per-lane minima reduced per workgroup, one atomic per workgroup; LDS: a workgroup table flushed with one
// atomic per bin that has a row; otherwise one atomic per row.  out all ones before the launch.  MODE as the scan's; FLOOR
// none or memory (floor, floor_best: the previous round's out and best).
template <int PATH, int MODE, int FLOOR>
__global__ __launch_bounds__(kBlock) void first_list_kernel(const void *kcol, uint32_t kwl, uint64_t kxor, const void *gcol, uint32_t gwl,
                                                            uint64_t n_rows, const uint32_t *__restrict__ ids, const uint64_t *count,
                                                            uint64_t capacity, uint32_t id_base, uint32_t bin_base, uint32_t n_bins,
                                                            const uint64_t *best, const uint64_t *floor, const uint64_t *floor_best,
                                                            uint64_t *out_) {
    static_assert(FLOOR != FLOOR_LDS, "the list form reads the floor from device memory");
    extern __shared__ uint64_t first_lds[];
    unsigned long long *tab = (unsigned long long *)first_lds;
    unsigned long long *out = (unsigned long long *)out_;
    if constexpr (PATH == FIRST_LDS) {
        for (uint32_t i = threadIdx.x; i < n_bins; i += kBlock) tab[i] = kFirstEmpty;
        __syncthreads();
    }
    uint64_t mine = kFirstEmpty;
    for_each_listed_row(ids, count, capacity, id_base, n_rows, [&](uint64_t row) {
        const uint64_t raw = gather_key<MODE != FIRST_NARROW>(kcol, kwl, row);
        const uint32_t table_row = (uint32_t)row + id_base;
        const uint64_t w = first_word<MODE>(raw, kxor, table_row);
        uint32_t b = 0;
        if constexpr (PATH != FIRST_ONE) {
            b = gather_narrow(gcol, gwl, row) - bin_base;
            if (b >= n_bins) return;
        }
        if constexpr (FLOOR != FLOOR_NONE) {
            uint64_t fbest = 0;
            if constexpr (MODE != FIRST_NARROW) fbest = floor_best[b];
            if (!head_above<MODE>(raw ^ kxor, MODE == FIRST_NARROW ? w : (uint64_t)table_row, floor[b], fbest)) return;
        }
        if constexpr (MODE == FIRST_WIDE_B) { if ((raw ^ kxor) != best[b]) return; }
        if constexpr (PATH == FIRST_ONE) mine = w < mine ? w : mine;
        else if constexpr (PATH == FIRST_LDS) atomicMin(&tab[b], (unsigned long long)w);
        else atomicMin(&out[b], (unsigned long long)w);
    });
    if constexpr (PATH == FIRST_ONE) {
        mine = block_min_u64(mine);
        if (threadIdx.x == 0 && mine != kFirstEmpty) atomicMin(&out[0], (unsigned long long)mine);
    } else if constexpr (PATH == FIRST_LDS) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < n_bins; i += kBlock)
            if (tab[i] != kFirstEmpty) atomicMin(&out[i], tab[i]);
    }
}

// keep[i] = i < limit || keys[i - limit] != keys[i], i < n (grid-stride; keys sorted, so equal keys are one run).
__global__ __launch_bounds__(kBlock) void runs_head_flags(const uint64_t *__restrict__ keys, uint64_t n, uint64_t limit,
                                                          uint8_t *__restrict__ keep) {
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock)
        keep[i] = i < limit || keys[i - limit] != keys[i];
}

// repeat[i] = i > 0 && ids[i - 1] == ids[i], i < n (grid-stride).
__global__ __launch_bounds__(kBlock) void list_repeat_flags(const uint32_t *__restrict__ ids, uint64_t n, uint8_t *__restrict__ repeat) {
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock)
        repeat[i] = i > 0 && ids[i - 1] == ids[i];
}

}  // namespace

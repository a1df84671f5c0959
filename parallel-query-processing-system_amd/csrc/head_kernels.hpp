// head_kernels.hpp -- device code of "the first N rows of every group" (included once by pqps_hip.hip, after first_kernels.hpp).
//
// No counterpart in the reference (SQL: ROW_NUMBER() OVER (PARTITION BY g ORDER BY k [DESC]) <= n).
//
// ROUNDS FORM.  The words of first_kernels.hpp, (img ^ x) << 32 | table_row, are unique per row, so the r-th row of a bin is
// the minimum word STRICTLY ABOVE the bin's (r-1)-th word.  Round 0 is the first-row launch, unchanged; round r >= 1 is
// head_scan_kernel: first_scan_kernel's body with one more test per matching row, w > floor[b], floor = round r-1's output.
// A bin whose previous word is all ones is exhausted: nothing is greater than all ones, so it stays all ones without a
// special case.  The rounds depend on each other only through device memory on one stream; none needs a host wait.
//   Where the floor lives (HeadPath):
//     HEAD_ONE      no GROUP BY               one word (a pair for command_id), in registers
//     HEAD_LDS2     D <= 4096, narrow keys    in dynamic LDS beside the min table (16 B x D <= 64 KiB), filled at the start
//     HEAD_LDS      D <= 8192                 the min table in LDS (8 B x D); the floor read per MATCHING row from device
//                                             memory (8 B x D <= 64 KiB: it stays in L2)
//     HEAD_GLOBAL   D <= 65536                floor read from device memory, one global atomic min per matching row
//   wide keys (command_id, 96 bits): each round is two passes, the floor the pair (fbest[b], frow[b]) of round r-1:
//     pass A   best[b] = min of k = v ^ x over the bin's rows with (k, row) > (fbest, frow) lexicographically
//     pass B   out[b]  = min of row over the bin's rows with k == best[b] that pass the same test
//   frow all ones means the bin is exhausted (k itself may be all ones, so this case IS tested).  The pair is read from
//   device memory on every grouped path: the wide form already scans twice per round, and a 24 B x D table would halve the
//   bins that fit LDS.
// Partial rows, the combiner (first_min_kernel) and the store-and-combine rule are those of first_kernels.hpp.
//
// LIST FORM.  head_list_kernel is first_list_kernel with the same floor test; the strict > makes an id listed twice one
// candidate.
//
// SORT FORM.  Over a selection sorted by (group, key, row) with repeated ids removed, runs_head_flags marks the entries
// whose rank inside their run of equal group images is below `limit`: in a sorted array an entry has rank >= limit exactly
// when the entry `limit` places before it is in the same run, so keep[i] = i < limit || group[i - limit] != group[i] -- no
// segmented scan.  list_repeat_flags marks the second and later copies of an id, which the sort leaves adjacent.
#pragma once

namespace {

enum HeadPath { HEAD_ONE = 0, HEAD_LDS2 = 1, HEAD_LDS = 2, HEAD_GLOBAL = 3 };
constexpr uint32_t kHeadLds2Bins = 4096;           // 16 B per bin: min table and floor in 64 KiB of LDS

struct HeadArgs {
    FirstArgs f;                     // first: the scan loop reads the WHERE in place; f.best: pass B's [n_bins] of THIS round
    const uint64_t *floor;           // the previous round's out[n_bins]
    const uint64_t *floor_best;      // wide: the previous round's best[n_bins]
};

// Does the row (k = v ^ x, w its word: narrow the whole word, wide the table row) lie strictly above the floor?
template <int MODE> __device__ __forceinline__ bool head_above(uint64_t k, uint64_t w, uint64_t frow, uint64_t fbest) {
    if constexpr (MODE == FIRST_NARROW) return w > frow;
    else return frow != kFirstEmpty && (k > fbest || (k == fbest && w > frow));
}

template <int PATH, int MODE, bool NT>
__global__ __launch_bounds__(kBlock, 1) void head_scan_kernel(const HeadArgs) {
    static_assert(PATH != HEAD_LDS2 || MODE == FIRST_NARROW, "the floor in LDS: narrow keys only");
    const auto &h = kernarg<HeadArgs>();
    const auto &g = h.f;
    CArgs &a = g.e;
    extern __shared__ uint64_t head_lds[];                      // LDS paths: the min table [nb], LDS2: then the floor [nb]
    unsigned long long *tab = (unsigned long long *)head_lds;
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t nb = g.n_bins, base_bin = g.bin_base, kwl = g.kwidth_log2, gwl = g.gwidth_log2, row_base = g.row_base;
    const uint64_t kxor = g.kxor;
    const char *kbase = (const char *)g.kcol;
    const char *gbase = (const char *)g.gcol;
    const uint64_t *best = g.best;
    const uint64_t *floor = h.floor, *floor_best = h.floor_best;
    unsigned long long *out = (unsigned long long *)g.out;
    if constexpr (PATH == HEAD_LDS2 || PATH == HEAD_LDS) {
        for (uint32_t i = threadIdx.x; i < nb; i += kBlock) {
            tab[i] = kFirstEmpty;
            if constexpr (PATH == HEAD_LDS2) head_lds[nb + i] = floor[i];
        }
        __syncthreads();
    }
    uint64_t mine = kFirstEmpty;                                // HEAD_ONE
    uint64_t want0 = 0, frow0 = 0, fbest0 = 0;
    if constexpr (PATH == HEAD_ONE) {
        frow0 = floor[0];
        if constexpr (MODE != FIRST_NARROW) fbest0 = floor_best[0];
        if constexpr (MODE == FIRST_WIDE_B) want0 = best[0];
    }
    fused_scan_steps<NT>(a, lane, wv, [&](uint64_t step_row0, uint32_t mbits) {
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
        if constexpr (PATH != HEAD_ONE) load_step_u32<NT>(gbase, gwl, step_row0, lane, gv);
        const uint32_t lane_row0 = row_base + (uint32_t)step_row0 + lane * kRplGeneric;
#pragma unroll
        for (int p = 0; p < 16; p++) {                          // bit p <-> row lane_row0 + (p / 4) * 256 + p % 4
            if (!((mbits >> p) & 1u)) continue;
            const uint32_t row = lane_row0 + (uint32_t)(p / 4) * 256u + (uint32_t)(p % 4);
            const uint64_t w = first_word<MODE>(v[p], kxor, row);
            const uint64_t k = v[p] ^ kxor;                     // (wide only)
            if constexpr (PATH == HEAD_ONE) {
                if (!head_above<MODE>(k, MODE == FIRST_NARROW ? w : (uint64_t)row, frow0, fbest0)) continue;
                if constexpr (MODE == FIRST_WIDE_B) { if (k != want0) continue; }
                mine = w < mine ? w : mine;
            } else {
                const uint32_t b = gv[p] - base_bin;
                if (b >= nb) continue;
                uint64_t frow, fbest = 0;
                if constexpr (PATH == HEAD_LDS2) frow = head_lds[nb + b];
                else frow = floor[b];
                if constexpr (MODE != FIRST_NARROW) fbest = floor_best[b];
                if (!head_above<MODE>(k, MODE == FIRST_NARROW ? w : (uint64_t)row, frow, fbest)) continue;
                if constexpr (MODE == FIRST_WIDE_B) { if (k != best[b]) continue; }
                if constexpr (PATH == HEAD_GLOBAL) atomicMin(&out[b], (unsigned long long)w);
                else atomicMin(&tab[b], (unsigned long long)w);
            }
        }
    });
    if constexpr (PATH == HEAD_ONE) {
        mine = block_min_u64(mine);
        if (threadIdx.x == 0) g.parts[blockIdx.x] = mine;
    } else if constexpr (PATH != HEAD_GLOBAL) {
        __syncthreads();
        uint64_t *row = g.parts + (uint64_t)blockIdx.x * nb;
        for (uint32_t i = threadIdx.x; i < nb; i += kBlock) row[i] = tab[i];
    }
}

// first_list_kernel with the floor test.  PATH is a FirstPath: the floor is read from device memory on every path (a list is
// a gather per row already).  out all ones before the launch.
template <int PATH, int MODE>
__global__ __launch_bounds__(kBlock) void head_list_kernel(const void *kcol, uint32_t kwl, uint64_t kxor, const void *gcol, uint32_t gwl,
                                                           uint64_t n_rows, const uint32_t *__restrict__ ids, const uint64_t *count,
                                                           uint64_t capacity, uint32_t id_base, uint32_t bin_base, uint32_t n_bins,
                                                           const uint64_t *best, const uint64_t *floor, const uint64_t *floor_best,
                                                           uint64_t *out_) {
    extern __shared__ uint64_t head_lds[];
    unsigned long long *tab = (unsigned long long *)head_lds;
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
        uint64_t fbest = 0;
        if constexpr (MODE != FIRST_NARROW) fbest = floor_best[b];
        if (!head_above<MODE>(raw ^ kxor, MODE == FIRST_NARROW ? w : (uint64_t)table_row, floor[b], fbest)) return;
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

// set_kernels.hpp -- HAVING: dense bins into the presence bitmap of a value set (included once by pqps_hip.hip, after
// fused_common.hpp).
//
// The bins are those the grouped scans leave (pqps_filter_group: n_bins u32 counts; pqps_filter_aggregate and the wide
// bins: the field-major [4][n_bins] u64 -- counts, sums, min images, max images).  Bit b of the bitmap is
//   count[b] != 0  &&  field[b] OP constant
// so a value that no row carries is never a member, whatever its (empty) aggregate compares to.
// A wave takes 64 consecutive bins per round, one per lane: a coalesced streaming load of the count (4 or 8 bytes a lane)
// and of the compared field alone (none for COUNT, 8 bytes otherwise) -- 4, 8 or 16 of the 32 bytes a valued bin has.
// __ballot is the 64 bits of the round; lane 0 stores them as one plain 8-byte vector store (the last round of an n_bins
// that ends in the lower half stores its one u32 word, so nothing past (n_bins + 31) / 32 words is written; lanes past
// n_bins vote 0, which zeroes the tail bits).  The grid is persistent (list_grid, as pqps_bins_compact's); `members` gets
// one 64-bit atomic add per workgroup.  No workgroup waits for another.
#pragma once

namespace {

constexpr uint32_t kHavingBlock = 256;

template <typename T> __device__ __forceinline__ T having_ld(const T *p) { return __builtin_nontemporal_load(p); }

__device__ __forceinline__ bool having_cmp(int op, bool is_signed, uint64_t x, uint64_t c) {
    switch (op) {
    case PQPS_HAVING_EQ: return x == c;
    case PQPS_HAVING_NE: return x != c;
    case PQPS_HAVING_LT: return is_signed ? (int64_t)x < (int64_t)c : x < c;
    case PQPS_HAVING_GT: return is_signed ? (int64_t)x > (int64_t)c : x > c;
    case PQPS_HAVING_LE: return is_signed ? (int64_t)x <= (int64_t)c : x <= c;
    default:             return is_signed ? (int64_t)x >= (int64_t)c : x >= c;
    }
}

// VALUED: the [4][n_bins] u64 fields, FIELD = PQPS_HAVING_COUNT .. _MAX the row of them that is compared; otherwise u32 counts.
template <bool VALUED, int FIELD>
__global__ __launch_bounds__(kHavingBlock) void bins_having_kernel(const void *bins, uint64_t n_bins, int op, int is_signed,
                                                                   uint64_t constant, uint32_t *bitmap, unsigned long long *members) {
    __shared__ uint32_t s_tot[kHavingBlock / 64];
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t rounds = (n_bins + 63) / 64;
    const uint64_t waves = (uint64_t)gridDim.x * (kHavingBlock / 64);
    uint32_t mine = 0;                                               // lane 0: the members of this wave's rounds
    for (uint64_t r = (uint64_t)blockIdx.x * (kHavingBlock / 64) + (threadIdx.x >> 6); r < rounds; r += waves) {
        const uint64_t b = r * 64 + lane;
        bool hit = false;
        if (b < n_bins) {
            uint64_t count, x;
            if constexpr (VALUED) count = having_ld((const uint64_t *)bins + b);
            else count = having_ld((const uint32_t *)bins + b);
            if constexpr (FIELD == PQPS_HAVING_COUNT) x = count;
            else x = having_ld((const uint64_t *)bins + (uint64_t)FIELD * n_bins + b);
            hit = count != 0 && having_cmp(op, FIELD == PQPS_HAVING_SUM && is_signed, x, constant);
        }
        const unsigned long long m = __ballot(hit);
        if (lane == 0) {
            if (r * 64 + 32 < n_bins) *(unsigned long long *)(bitmap + r * 2) = m;   // both words of the round exist
            else bitmap[r * 2] = (uint32_t)m;                                       // the bitmap ends with the lower word
            mine += (uint32_t)__popcll(m);
        }
    }
    if (members) {
        if (lane == 0) s_tot[threadIdx.x >> 6] = mine;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint64_t t = 0;
            for (uint32_t i = 0; i < kHavingBlock / 64; i++) t += s_tot[i];
            if (t) atomicAdd(members, (unsigned long long)t);
        }
    }
}

// The rows the bins hold, *rows += the sum of their counts: what a value set reports as its inner rows (the fused grouped
// scans leave no total).  One streaming load of the count per bin, the workgroup's sum through one LDS word.
template <bool VALUED>
__global__ __launch_bounds__(kHavingBlock) void bins_rows_kernel(const void *bins, uint64_t n_bins, unsigned long long *rows) {
    __shared__ unsigned long long s_sum;
    if (threadIdx.x == 0) s_sum = 0;
    __syncthreads();
    unsigned long long mine = 0;
    for (uint64_t b = (uint64_t)blockIdx.x * kHavingBlock + threadIdx.x; b < n_bins; b += (uint64_t)gridDim.x * kHavingBlock) {
        if constexpr (VALUED) mine += having_ld((const uint64_t *)bins + b);
        else mine += having_ld((const uint32_t *)bins + b);
    }
    if (mine) atomicAdd(&s_sum, mine);
    __syncthreads();
    if (threadIdx.x == 0 && s_sum) atomicAdd(rows, s_sum);
}

}  // namespace

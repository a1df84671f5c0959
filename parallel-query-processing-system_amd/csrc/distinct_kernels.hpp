// distinct_kernels.hpp -- device code of COUNT(DISTINCT value column), overall or per group (included once by pqps_hip.hip,
// after fused_common.hpp).
//
// No counterpart in the reference (its engines have no aggregates).  The accumulator is a PRESENCE BITMAP: G rows (group
// bins, 1 without GROUP BY) of W = ceil(Dv / 32) u32 words, bit v of row g set iff some matching row has group bin g and
// value bin v.  A value bin is (value - v_base) in 32-bit arithmetic, exactly like a group bin: the dictionary code of a
// string column, the value minus the column's minimum for an i32 column, 0 / 1 for sudo_used.  Bits only ever go from 0
// to 1, so every update is an OR, partial bitmaps merge by OR (shards too), and the answer is a popcount per row.
//
// Fused scan (pqps_filter_distinct): the shared scan loop (fused_common.hpp) with one round of value-column loads (and
// group-column loads: 1, 2, 4 bytes or a bit plane each) per step that holds a match.  Bitmap forms:
//   REG    G x Dv <= 64     one u64 mask per lane (bit g * Dv + v), OR-reduced over the wave on the DPP path and over the
//                           workgroup through LDS; the workgroup stores its G x W words into a partial row
//   LDS    G x W <= 16384   the bitmap in dynamic LDS (64 KiB at most: two workgroups per CU).  TEST BEFORE SET: a row
//                           reads its word and ORs only if its bit is clear, so once the bitmap has warmed up a row costs
//                           one LDS read and no atomic.  The workgroup stores its whole bitmap into a partial row.
//   GLOBAL G x W x 32 <= cap  test before set on the HBM word, then a global atomic OR (a correctness path for high
//                           cardinality, like BINS_GLOBAL)
// REG and LDS flush by store-and-OR (dist_or_kernel: 64 partial rows per workgroup, one atomic OR per non-zero word), the
// form agg_sum_kernel uses: a dense bitmap costs every workgroup the same plain stores, where one atomic per non-zero word
// and workgroup would queue thousands of same-address ORs at the memory side.  The matching-row count comes from the same
// loop (popc of the match bits per lane, one plain store per workgroup, summed by dist_or_kernel).
//
// List form (pqps_distinct_list): the same three forms over an ID list, gathering the value and group columns (1, 2 or 4
// bytes) per listed row; REG and LDS flush with one atomic OR per non-zero word and workgroup (a list grid is small).
// Count (dist_count_kernel): distinct[g] = popcount of row g.  Sort form (pqps_distinct_sort): composite keys of the
// listed rows sorted by the stable LSD radix sort of radix_sort.hpp, dist_unique_kernel counts key changes per group.
#pragma once

namespace {

enum DistPath { DIST_REG = 0, DIST_LDS = 1, DIST_GLOBAL = 2 };
constexpr uint32_t kDistRegBits = 64;              // G x Dv of the register form
constexpr uint32_t kDistLdsWords = 16384;          // 64 KiB of LDS: two workgroups per CU
constexpr uint64_t kDistMaxBits = 1ull << 30;      // G x W x 32 of the bitmap forms: 128 MiB per shard
constexpr uint32_t kDistOrParts = 64;              // partial rows one workgroup of dist_or_kernel combines

struct DistArgs {
    EvalArgs e;                      // the WHERE, as the COUNT kernels take it -- first: the scan loop reads it in place
    const void *vcol;                // value column (bytes, u16, u32 or a bit plane)
    const void *gcol;                // group column (the same forms); unused without GROUP BY
    uint32_t *bitmap;                // GLOBAL: [G][W] (zeroed before the launch)
    uint32_t *parts;                 // REG / LDS: [gridDim.x][G * W] partial bitmaps
    uint64_t *totals;                // [gridDim.x] matching rows per workgroup
    uint32_t vwidth_log2, gwidth_log2;   // 0, 1, 2 or kWidthLog2Bits
    uint32_t v_base, g_base;
    uint32_t n_values, n_groups;     // Dv, G
    uint32_t words;                  // W
};

// word (g, w) of the bitmap out of the register form's mask (bit g * Dv + v)
__device__ __forceinline__ uint32_t dist_reg_word(uint64_t mask, uint32_t t, uint32_t nv, uint32_t nw) {
    const uint32_t gb = t / nw, w = t % nw;
    uint32_t word = 0;
    for (uint32_t v = w * 32; v < nv && v < w * 32 + 32; v++) word |= (uint32_t)((mask >> (gb * nv + v)) & 1ull) << (v & 31u);
    return word;
}

// Bit `bit` of word `idx` set, read first: most calls find it set and issue no atomic.
__device__ __forceinline__ void dist_test_set(uint32_t *words, uint64_t idx, uint32_t bit) {
    if (!(words[idx] & bit)) atomicOr(&words[idx], bit);
}

// The workgroup's OR of the lanes' masks (REG) and sum of their counts, through LDS; every thread gets both.
__device__ __forceinline__ void dist_block_reduce(uint64_t &mask, uint64_t &cnt) {
    __shared__ uint64_t s_red[kWaves][2];
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t lo = wave_or_u32((uint32_t)mask), hi = wave_or_u32((uint32_t)(mask >> 32));
    uint64_t c = cnt;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) c += shfl_xor_u64(c, off);
    if (lane == 0) { s_red[wv][0] = (uint64_t)lo | ((uint64_t)hi << 32); s_red[wv][1] = c; }
    __syncthreads();
    mask = 0;
    cnt = 0;
    for (uint32_t w = 0; w < (uint32_t)kWaves; w++) { mask |= s_red[w][0]; cnt += s_red[w][1]; }
}

template <int PATH, bool GROUPED, bool NT>
__global__ __launch_bounds__(kBlock, 1) void dist_scan_kernel(const DistArgs) {
    const auto &g = kernarg<DistArgs>();
    CArgs &a = g.e;
    extern __shared__ uint32_t dist_lds[];                      // LDS form: the bitmap
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t nv = g.n_values, ng = g.n_groups, nw = g.words, vb0 = g.v_base, gb0 = g.g_base;
    const uint32_t vwl = g.vwidth_log2, gwl = g.gwidth_log2;
    const char *vbase = (const char *)g.vcol;
    const char *gbase = (const char *)g.gcol;
    const uint32_t n_words = ng * nw;                           // <= kDistLdsWords on the LDS form
    if constexpr (PATH == DIST_LDS) {
        for (uint32_t i = threadIdx.x; i < n_words; i += kBlock) dist_lds[i] = 0;
        __syncthreads();
    }
    uint64_t mask = 0, cnt = 0;
    fused_scan_steps<NT>(a, lane, wv, [&](uint64_t step_row0, uint32_t mbits) {
        cnt += __popc(mbits);
        uint32_t v[16], gv[16];
        load_step_u32<NT>(vbase, vwl, step_row0, lane, v);
        if constexpr (GROUPED) load_step_u32<NT>(gbase, gwl, step_row0, lane, gv);
#pragma unroll
        for (int p = 0; p < 16; p++) {
            const uint32_t vb = v[p] - vb0;
            const uint32_t gb = GROUPED ? gv[p] - gb0 : 0u;
            const bool hit = ((mbits >> p) & 1u) && vb < nv && gb < ng;
            if constexpr (PATH == DIST_REG) {
                mask |= hit ? 1ull << (gb * nv + vb) : 0ull;     // (G x Dv <= 64: the shift is in range when hit)
            } else if (hit) {
                const uint64_t idx = (uint64_t)gb * nw + (vb >> 5);
                if constexpr (PATH == DIST_LDS) dist_test_set(dist_lds, idx, 1u << (vb & 31u));
                else dist_test_set(g.bitmap, idx, 1u << (vb & 31u));
            }
        }
    });
    dist_block_reduce(mask, cnt);                               // (REG: the mask; every form: the count)
    if (threadIdx.x == 0) g.totals[blockIdx.x] = cnt;
    if constexpr (PATH == DIST_REG) {
        if (threadIdx.x < n_words) g.parts[(uint64_t)blockIdx.x * n_words + threadIdx.x] = dist_reg_word(mask, threadIdx.x, nv, nw);
    } else if constexpr (PATH == DIST_LDS) {
        __syncthreads();
        uint32_t *row = g.parts + (uint64_t)blockIdx.x * n_words;
        for (uint32_t i = threadIdx.x; i < n_words; i += kBlock) row[i] = dist_lds[i];
    }
}

// bitmap[w] |= OR of parts[r][w] over the rows r of this workgroup's 64-row slice (one word per lane, the 4 waves take 16
// rows each, loads issued together, combined through LDS, one atomic OR per non-zero word), and *total += the slice's
// totals (workgroups of the first column).  bitmap and *total zeroed before the launch; n_words may be 0 (totals only).
__global__ __launch_bounds__(kBlock) void dist_or_kernel(const uint32_t *__restrict__ parts, const uint64_t *__restrict__ totals,
                                                         uint32_t n_parts, uint32_t n_words, uint32_t *bitmap,
                                                         unsigned long long *total) {
    __shared__ uint32_t s_or[kWaves][64];
    __shared__ uint64_t s_tot[kWaves];
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t word = blockIdx.x * 64 + lane;
    const uint32_t r0 = blockIdx.y * kDistOrParts + wv * (kDistOrParts / kWaves);
    uint32_t v[kDistOrParts / kWaves];
#pragma unroll
    for (uint32_t i = 0; i < kDistOrParts / kWaves; i++)
        v[i] = word < n_words && r0 + i < n_parts ? parts[(uint64_t)(r0 + i) * n_words + word] : 0u;
    uint32_t t = 0;
#pragma unroll
    for (uint32_t i = 0; i < kDistOrParts / kWaves; i++) t |= v[i];
    s_or[wv][lane] = t;
    if (blockIdx.x == 0) {
        uint64_t c = lane < kDistOrParts / kWaves && r0 + lane < n_parts ? totals[r0 + lane] : 0ull;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) c += shfl_xor_u64(c, off);
        if (lane == 0) s_tot[wv] = c;
    }
    __syncthreads();
    if (wv == 0) {
        t = s_or[0][lane] | s_or[1][lane] | s_or[2][lane] | s_or[3][lane];
        if (t && word < n_words) atomicOr(&bitmap[word], t);
        if (blockIdx.x == 0 && lane == 0) {
            const uint64_t c = s_tot[0] + s_tot[1] + s_tot[2] + s_tot[3];
            if (c) atomicAdd(total, (unsigned long long)c);
        }
    }
}

// distinct[g] += popcount of row g of the bitmap ([n_groups][n_words]): one wave per (row, 256-word segment), lanes read
// words w0 + lane + 64 k (coalesced), one atomic add per wave with bits.  distinct zeroed before the launch.
__global__ __launch_bounds__(kBlock) void dist_count_kernel(const uint32_t *__restrict__ bitmap, uint32_t n_groups, uint64_t n_words,
                                                            unsigned long long *distinct) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t segs = (n_words + 255) / 256;
    const uint64_t items = (uint64_t)n_groups * segs;
    const uint64_t n_waves = (uint64_t)gridDim.x * kWaves;
    for (uint64_t it = (uint64_t)blockIdx.x * kWaves + (threadIdx.x >> 6); it < items; it += n_waves) {
        const uint64_t gb = it / segs, w0 = (it % segs) * 256;
        const uint32_t *row = bitmap + gb * n_words;
        uint32_t c = 0;
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) {
            const uint64_t w = w0 + lane + 64 * k;
            if (w < n_words) c += __popc(row[w]);
        }
        c = wave_sum_u32(c);
        if (lane == 0 && c) atomicAdd(&distinct[gb], (unsigned long long)c);
    }
}

// The bitmap over an ID list: ids[0 .. min(*count, capacity)), row = id - id_base.  REG: per-lane masks reduced per
// workgroup, one atomic OR per non-zero word; LDS: a workgroup bitmap, one atomic OR per non-zero word; GLOBAL: test before
// set on the bitmap.  bitmap zeroed before the launch.
template <int PATH, bool GROUPED>
__global__ __launch_bounds__(kBlock) void dist_list_kernel(const void *vcol, uint32_t vwl, const void *gcol, uint32_t gwl, uint64_t n_rows,
                                                           const uint32_t *__restrict__ ids, const uint64_t *count, uint64_t capacity,
                                                           uint32_t id_base, uint32_t v_base, uint32_t n_values, uint32_t g_base,
                                                           uint32_t n_groups, uint32_t n_words_row, uint32_t *bitmap) {
    extern __shared__ uint32_t dist_lds[];
    const uint32_t n_words = n_groups * n_words_row;             // (REG / LDS: small)
    if constexpr (PATH == DIST_LDS) {
        for (uint32_t i = threadIdx.x; i < n_words; i += kBlock) dist_lds[i] = 0;
        __syncthreads();
    }
    uint64_t mask = 0, unused = 0;
    for_each_listed_row(ids, count, capacity, id_base, n_rows, [&](uint64_t row) {
        const uint32_t vb = gather_narrow(vcol, vwl, row) - v_base;
        const uint32_t gb = GROUPED ? gather_narrow(gcol, gwl, row) - g_base : 0u;
        if (vb >= n_values || gb >= n_groups) return;
        if constexpr (PATH == DIST_REG) mask |= 1ull << (gb * n_values + vb);
        else {
            const uint64_t idx = (uint64_t)gb * n_words_row + (vb >> 5);
            if constexpr (PATH == DIST_LDS) dist_test_set(dist_lds, idx, 1u << (vb & 31u));
            else dist_test_set(bitmap, idx, 1u << (vb & 31u));
        }
    });
    if constexpr (PATH == DIST_REG) {
        dist_block_reduce(mask, unused);
        if (threadIdx.x < n_words) {
            const uint32_t w = dist_reg_word(mask, threadIdx.x, n_values, n_words_row);
            if (w) atomicOr(&bitmap[threadIdx.x], w);
        }
    } else if constexpr (PATH == DIST_LDS) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < n_words; i += kBlock)
            if (dist_lds[i]) atomicOr(&bitmap[i], dist_lds[i]);
    }
}

// Sort form, keys of the listed rows: ids[0 .. n), row = id - id_base, group bin gb (0 without GROUP BY; G for a row
// outside the bins, which dist_unique_kernel skips).  Narrow values: key[i] = gb << 32 | (value - v_base).  WIDE
// (command_id, u64): key[i] = the value, grp[i] = gb.
template <bool WIDE>
__global__ __launch_bounds__(kBlock) void dist_keys_kernel(const void *vcol, uint32_t vwl, const void *gcol, uint32_t gwl,
                                                           const uint32_t *__restrict__ ids, uint64_t n, uint32_t id_base,
                                                           uint32_t v_base, uint32_t g_base, uint32_t n_groups,
                                                           uint64_t *key, uint32_t *grp) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t row = (uint64_t)(ids[i] - id_base);
        uint32_t gb = gcol ? gather_narrow(gcol, gwl, row) - g_base : 0u;
        if (gb > n_groups) gb = n_groups;
        if constexpr (WIDE) {
            key[i] = ((const uint64_t *)vcol)[row];
            grp[i] = gb;
        } else {
            key[i] = (uint64_t)gb << 32 | (uint32_t)(gather_narrow(vcol, vwl, row) - v_base);
        }
    }
}

// out[i] = i: the positions the group sort of the wide keys carries
__global__ __launch_bounds__(kBlock) void dist_iota_kernel(uint32_t *out, uint64_t n) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) out[i] = (uint32_t)i;
}

// wide keys in group order: val[k] = vals_by_value[pos[k]] (pos: the value-sorted positions, carried by the group sort)
__global__ __launch_bounds__(kBlock) void dist_permute_kernel(const uint64_t *__restrict__ vals_by_value, const uint32_t *__restrict__ pos,
                                                              uint64_t n, uint64_t *val) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
        val[i] = vals_by_value[pos[i]];
}

// distinct[g] += the keys of group g that differ from their predecessor, over keys sorted by (group, value): narrow
// key[i] (group = key >> 32), or WIDE (key[i] the value, grp[i] the group).  Every wave walks a contiguous range of
// 64-key tiles; a tile of one group adds popc(ballot(flags)) to a run kept in registers, flushed with one atomic when the
// group changes; a tile that spans groups adds its flags one atomic per lane (at most one such tile per group boundary).
// distinct zeroed before the launch.
template <bool WIDE>
__global__ __launch_bounds__(kBlock) void dist_unique_kernel(const uint64_t *__restrict__ key, const uint32_t *__restrict__ grp, uint64_t n,
                                                             uint32_t n_groups, unsigned long long *distinct) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t tiles = (n + 63) / 64;
    const uint64_t n_waves = (uint64_t)gridDim.x * kWaves;
    const uint64_t wave = (uint64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    const uint64_t per = (tiles + n_waves - 1) / n_waves;
    uint64_t t0 = wave * per, t1 = t0 + per;
    if (t1 > tiles) t1 = tiles;
    uint32_t run_g = 0xFFFFFFFFu;
    uint64_t run_c = 0;
    for (uint64_t t = t0; t < t1; t++) {
        const uint64_t i = t * 64 + lane;
        const bool valid = i < n;
        const uint64_t k = valid ? key[i] : 0ull;
        const uint32_t gb = !valid ? 0xFFFFFFFFu : WIDE ? grp[i] : (uint32_t)(k >> 32);
        bool flag = valid && gb < n_groups;
        if (flag && i > 0) {
            const uint64_t kp = key[i - 1];
            const uint32_t gp = WIDE ? grp[i - 1] : (uint32_t)(kp >> 32);
            flag = kp != k || gp != gb;
        }
        const uint32_t g0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)gb);   // lane 0: always valid
        if (__ballot(valid && gb != g0) == 0) {                 // uniform: one group in the tile
            if (g0 != run_g) {
                if (lane == 0 && run_c && run_g < n_groups) atomicAdd(&distinct[run_g], (unsigned long long)run_c);
                run_g = g0;
                run_c = 0;
            }
            run_c += (uint64_t)__popcll(__ballot(flag));
        } else {
            if (flag) atomicAdd(&distinct[gb], 1ull);
        }
    }
    if (lane == 0 && run_c && run_g < n_groups) atomicAdd(&distinct[run_g], (unsigned long long)run_c);
}

}  // namespace

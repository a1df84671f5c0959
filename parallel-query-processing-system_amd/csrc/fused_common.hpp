// fused_common.hpp -- device scaffolding shared by the fused filter-and-aggregate families: bins_, topk_, order_multi_,
// first_, distinct_, group_pair_ and assign_kernels.hpp (included once by pqps_hip.hip, after filter_kernels.hpp and before them).
//
// A fused scan is the grid-stride form of the COUNT kernels (fused_scan_steps): a wave takes the 1024-row steps wave,
// wave + n_waves, ... of a persistent grid, evaluates the WHERE of each (eval_step_full; match bit p of lane l <-> row
// step_row0 + (p / 4) * 256 + l * 4 + p % 4) and trims the partial last step (rows_below).  Only a step that holds a match
// (wave-uniform) reaches the kernel's body, which loads its own columns in the predicate columns' per-lane pattern
// (load_step_u32 / load_step_u64: RPL = 4, lane l owns rows l*4 .. l*4+3 of each 256-row chunk), so a sparse WHERE reads
// almost nothing beyond its predicate bytes.  The list forms walk an ID list instead (for_each_listed_row) and gather their
// columns per listed row (gather_narrow / gather_key).  No kernel of these families waits on another workgroup.
#pragma once

namespace {

// The kernel-argument segment as the kernel's by-value `Args` parameter laid it out (see kernel_args() of filter_kernels.hpp).
template <class Args>
__device__ __forceinline__ const __attribute__((address_space(4))) Args &kernarg() {
    return *(const __attribute__((address_space(4))) Args *)__builtin_amdgcn_kernarg_segment_ptr();
}

// body(step_row0, mbits) for every step of this wave (wave wv of the workgroup) that holds a match, mbits trimmed to n_rows.
template <bool NT, class Body>
__device__ __forceinline__ void fused_scan_steps(CArgs &a, uint32_t lane, uint32_t wv, const Body &body) {
    const uint64_t wave = (uint64_t)blockIdx.x * kWaves + wv;
    const uint64_t n_waves = (uint64_t)gridDim.x * kWaves;
    const uint64_t n_rows = a.n_rows;
    const uint64_t steps = (n_rows + kStepRows - 1) / kStepRows;
    for (uint64_t step = wave; step < steps; step += n_waves) {
        const uint64_t step_row0 = step * kStepRows;
        uint32_t mbits = eval_step_full<NT>(a, step_row0, lane);
        if (step_row0 + kStepRows > n_rows) mbits &= rows_below<kRplGeneric>(step_row0, n_rows, lane);   // the partial last step
        if (__ballot(mbits != 0u) == 0) continue;               // uniform: no match, no load of the body's columns
        body(step_row0, mbits);
    }
}

// body(row) for every entry of ids[0 .. min(*count, capacity)), grid-stride, row = id - id_base.
template <class Body>
__device__ __forceinline__ void for_each_listed_row(const uint32_t *ids, const uint64_t *count, uint64_t capacity,
                                                    uint32_t id_base, uint64_t n_rows, const Body &body) {
    uint64_t n = *count;
    if (n > capacity) n = capacity;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t row = (uint64_t)(ids[i] - id_base);
        if (row >= n_rows) continue;                            // (never: a shard's list holds its own rows)
        body(row);
    }
}

// value of row `row` of a 1, 2 or 4 byte column
__device__ __forceinline__ uint32_t gather_narrow(const void *col, uint32_t wl, uint64_t row) {
    return wl == 0 ? ((const uint8_t *)col)[row] : wl == 1 ? ((const uint16_t *)col)[row] : ((const uint32_t *)col)[row];
}

// raw sort key of row r: a u64 column (WIDE) or a narrow one of 1 << kwl bytes; nullptr: every key 0
template <bool WIDE>
__device__ __forceinline__ uint64_t gather_key(const void *kcol, uint32_t kwl, uint64_t r) {
    if (!kcol) return 0;
    if constexpr (WIDE) return ((const uint64_t *)kcol)[r];
    else return gather_narrow(kcol, kwl, r);
}

// A 1, 2 or 4 byte column or a bit plane: the values of a lane's 16 rows of one full step, v[p] <-> match bit p.
template <bool NT>
__device__ __forceinline__ void load_step_u32(const char *base, uint32_t wl, uint64_t step_row0, uint32_t lane, uint32_t (&v)[16]) {
    const uint64_t lane_row0 = step_row0 + lane * kRplGeneric;
#pragma unroll
    for (int u = 0; u < 4; u++) {
        const uint64_t r0 = lane_row0 + (uint64_t)u * 256;
        if (wl == 2) {
            const uint4 q = ld_x4<NT>(base + r0 * 4);
            v[4 * u] = q.x; v[4 * u + 1] = q.y; v[4 * u + 2] = q.z; v[4 * u + 3] = q.w;
        } else if (wl == 1) {
            const uint2 q = ld_x2<NT>(base + r0 * 2);
            v[4 * u] = q.x & 0xFFFFu; v[4 * u + 1] = q.x >> 16;
            v[4 * u + 2] = q.y & 0xFFFFu; v[4 * u + 3] = q.y >> 16;
        } else if (wl == kWidthLog2Bits) {                      // bit plane: the lane's 4 rows are a nibble
            const uint32_t q = ld_u8<NT>(base + (r0 >> 3)) >> (uint32_t)(r0 & 4u);
            v[4 * u] = q & 1u; v[4 * u + 1] = (q >> 1) & 1u;
            v[4 * u + 2] = (q >> 2) & 1u; v[4 * u + 3] = (q >> 3) & 1u;
        } else {
            const uint32_t q = ld_x1<NT>(base + r0);
            v[4 * u] = q & 0xFFu; v[4 * u + 1] = (q >> 8) & 0xFFu;
            v[4 * u + 2] = (q >> 16) & 0xFFu; v[4 * u + 3] = q >> 24;
        }
    }
}

// widen_value: a u64 value as is, an i32 value sign-extended.  load_step_u64: the same rows of a u64 or i32 column, widened.
template <bool U64> __device__ __forceinline__ uint64_t widen_value(uint64_t raw) {
    if constexpr (U64) return raw;
    else return (uint64_t)(int64_t)(int32_t)(uint32_t)raw;
}
template <bool U64, bool NT>
__device__ __forceinline__ void load_step_u64(const char *base, uint64_t step_row0, uint32_t lane, uint64_t (&v)[16]) {
    const uint64_t lane_row0 = step_row0 + lane * kRplGeneric;
#pragma unroll
    for (int u = 0; u < 4; u++) {
        const uint64_t r0 = lane_row0 + (uint64_t)u * 256;
        if constexpr (U64) {
            const uint4 q0 = ld_x4<NT>(base + r0 * 8);
            const uint4 q1 = ld_x4<NT>(base + r0 * 8 + 16);
            v[4 * u] = (uint64_t)q0.x | ((uint64_t)q0.y << 32); v[4 * u + 1] = (uint64_t)q0.z | ((uint64_t)q0.w << 32);
            v[4 * u + 2] = (uint64_t)q1.x | ((uint64_t)q1.y << 32); v[4 * u + 3] = (uint64_t)q1.z | ((uint64_t)q1.w << 32);
        } else {
            const uint4 q = ld_x4<NT>(base + r0 * 4);
            v[4 * u] = widen_value<false>(q.x); v[4 * u + 1] = widen_value<false>(q.y);
            v[4 * u + 2] = widen_value<false>(q.z); v[4 * u + 3] = widen_value<false>(q.w);
        }
    }
}

__device__ __forceinline__ uint64_t shfl_xor_u64(uint64_t v, int off) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, off, 64);
    const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), off, 64);
    return (uint64_t)lo | ((uint64_t)hi << 32);
}

// OR over the 64 lanes, returned in every lane (the DPP pattern of wave_sum_u32)
__device__ __forceinline__ uint32_t wave_or_u32(uint32_t v) {
    v |= dpp_or_zero<0xb1>(v);
    v |= dpp_or_zero<0x4e>(v);
    v |= dpp_or_zero<0x124>(v);
    v |= dpp_or_zero<0x128>(v);
    v |= dpp_or_zero<0x142, 0xa>(v);
    v |= dpp_or_zero<0x143, 0xc>(v);
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

}  // namespace

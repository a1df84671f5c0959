// assign_kernels.hpp -- device code of UPDATE SET ... WHERE: constants written in place into the rows a WHERE selects
// (included once by pqps_hip.hip, after fused_common.hpp).
//
// No counterpart in the reference (its parser answers UPDATE with CMD_UNKNOWN).  Up to PQPS_MAX_COLUMNS targets per launch,
// each a column of 1, 2, 4 or 8 bytes and the constant every selected row receives.
//
// OWNERSHIP.  Both kernels walk the table in the fused scans' pattern (fused_common.hpp): a wave takes 1024-row steps, lane l
// owns rows l*4 .. l*4+3 of each of the step's four 256-row chunks, match bit p of the lane <-> row step_row0 + (p / 4) * 256
// + l * 4 + p % 4.  A row is read (by the WHERE) and written (here) by its owner lane only, and a step's WHERE is complete
// before the step's stores begin, so the WHERE sees the values from before the update even where it reads a target column:
// no second buffer, no atomics on the data.  The 4 rows of a lane's chunk are 4 x width contiguous bytes, aligned to their
// size -- one dword of a 1-byte column -- so no two lanes ever store into the same dword.
//
// STORES (assign_chunk), per target and per chunk of a lane, by the chunk's four match bits:
//   none set   nothing: a sparse WHERE touches almost nothing beyond its predicate bytes
//   all set    the four new values in one go, no load: global_store_dword (1-byte column), _dwordx2 (2), _dwordx4 (4), two
//              _dwordx4 (8: 32 bytes; the widest store the ISA has is 16)
//   some set   1 and 2 byte columns: the lane's own dword / two dwords loaded, the matched rows' bytes replaced (a byte mask
//              from the bits, v_and_or_b32 / v_cndmask_b32), stored once -- against up to three global_store_byte / _short
//              with a shift each; the unmatched rows get back the bytes they had (rows past n_rows included: their bits
//              are never set).
//              4 and 8 byte columns: one global_store_dword / _dwordx2 per matched row under the lane mask, no load -- a blend
//              would read 16 / 32 bytes to save at most two stores.
// Plain stores throughout.  The matched rows are counted as member_kernels.hpp counts: a popcount per lane, one DPP sum per
// wave, one 64-bit atomic add per workgroup.  No kernel here waits on another workgroup.
#pragma once

namespace {

struct AssignTarget {
    char *data;
    uint64_t value;                  // the new value's low 1 << width_log2 bytes
    uint32_t width_log2;             // 0 .. 3
    uint32_t reserved;
};

struct AssignArgs {
    EvalArgs e;                      // the WHERE, as the COUNT kernels take it -- first: the scan loop reads it in place
    AssignTarget tgt[PQPS_MAX_COLUMNS];
    uint32_t n_targets;
    unsigned long long *matched;     // zeroed before the launch; may be nullptr
};

struct AssignFlagsArgs {
    const uint8_t *flags;            // one byte per row, != 0: assign
    uint64_t n_rows;
    AssignTarget tgt[PQPS_MAX_COLUMNS];
    uint32_t n_targets;
};

// match bits -> the bytes of their rows in the lane's dword(s)
__device__ __forceinline__ uint32_t byte_mask4(uint32_t m) {       // bit i of m -> byte i of the result
    return ((m & 1u) * 0xFFu) | ((m & 2u) * (0xFF00u >> 1)) | ((m & 4u) * (0xFF0000u >> 2)) | ((m & 8u) * (0xFF000000u >> 3));
}
__device__ __forceinline__ uint32_t half_mask2(uint32_t m) {       // bit i of m (i < 2) -> half-word i of the result
    return ((m & 1u) * 0xFFFFu) | ((m & 2u) * (0xFFFF0000u >> 1));
}

// One target, one chunk of a lane: rows r0 .. r0 + 3 (r0 a multiple of 4), m = their four match bits, not 0.
__device__ __forceinline__ void assign_chunk(char *data, uint32_t wl, uint64_t value, uint64_t r0, uint32_t m) {
    if (wl == 0) {
        uint32_t *p = (uint32_t *)(data + r0);
        const uint32_t v = (uint32_t)(value & 0xFFu) * 0x01010101u;
        if (m == 0xFu) { *p = v; return; }
        const uint32_t k = byte_mask4(m);
        *p = (*p & ~k) | (v & k);
    } else if (wl == 1) {
        uint2 *p = (uint2 *)(data + r0 * 2);
        const uint32_t v = (uint32_t)(value & 0xFFFFu) * 0x00010001u;
        if (m == 0xFu) { *p = make_uint2(v, v); return; }
        const uint32_t k0 = half_mask2(m), k1 = half_mask2(m >> 2);
        uint2 q = *p;
        q.x = (q.x & ~k0) | (v & k0);
        q.y = (q.y & ~k1) | (v & k1);
        *p = q;
    } else if (wl == 2) {
        uint32_t *p = (uint32_t *)(data + r0 * 4);
        const uint32_t v = (uint32_t)value;
        if (m == 0xFu) { *(uint4 *)p = make_uint4(v, v, v, v); return; }
#pragma unroll
        for (uint32_t i = 0; i < 4; i++)
            if ((m >> i) & 1u) p[i] = v;
    } else {
        uint2 *p = (uint2 *)(data + r0 * 8);
        const uint32_t lo = (uint32_t)value, hi = (uint32_t)(value >> 32);
        if (m == 0xFu) {
            ((uint4 *)p)[0] = make_uint4(lo, hi, lo, hi);
            ((uint4 *)p)[1] = make_uint4(lo, hi, lo, hi);
            return;
        }
#pragma unroll
        for (uint32_t i = 0; i < 4; i++)
            if ((m >> i) & 1u) p[i] = make_uint2(lo, hi);
    }
}

// Every target, every chunk of the lane's 16 rows of one step.  T: AssignTarget[] in the kernel-argument segment.
template <class T>
__device__ __forceinline__ void assign_step(const T &tgt, uint32_t n_targets, uint64_t step_row0, uint32_t lane, uint32_t mbits) {
    if (mbits == 0u) return;
    const uint64_t lane_row0 = step_row0 + lane * kRplGeneric;
    for (uint32_t t = 0; t < n_targets; t++) {                      // uniform
        char *data = tgt[t].data;
        const uint32_t wl = tgt[t].width_log2;
        const uint64_t value = tgt[t].value;
#pragma unroll
        for (uint32_t u = 0; u < 4; u++) {
            const uint32_t m = (mbits >> (4 * u)) & 0xFu;
            if (m) assign_chunk(data, wl, value, lane_row0 + (uint64_t)u * 256, m);
        }
    }
}

// The fused form: one persistent grid, the WHERE of a step, then its stores.
template <bool NT>
__global__ __launch_bounds__(kBlock, 1) void assign_scan_kernel(const AssignArgs) {
    const auto &g = kernarg<AssignArgs>();
    CArgs &a = g.e;
    __shared__ uint32_t s_tot[kWaves];
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t n_targets = g.n_targets;
    uint32_t mine = 0;
    fused_scan_steps<NT>(a, lane, wv, [&](uint64_t step_row0, uint32_t mbits) {
        mine += __popc(mbits);
        assign_step(g.tgt, n_targets, step_row0, lane, mbits);
    });
    if (g.matched) {
        const uint32_t wave = wave_sum_u32(mine);
        if (lane == 0) s_tot[wv] = wave;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint64_t t = 0;
            for (uint32_t i = 0; i < (uint32_t)kWaves; i++) t += s_tot[i];
            if (t) atomicAdd(g.matched, (unsigned long long)t);
        }
    }
}

// The flags form: the same steps, lanes and stores, the match bits read from one flag byte per row (only flags[r], r < n_rows).
__global__ __launch_bounds__(kBlock, 1) void assign_flags_kernel(const AssignFlagsArgs) {
    const auto &g = kernarg<AssignFlagsArgs>();
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint64_t wave = (uint64_t)blockIdx.x * kWaves + wv, n_waves = (uint64_t)gridDim.x * kWaves;
    const uint64_t n_rows = g.n_rows;
    const uint64_t steps = (n_rows + kStepRows - 1) / kStepRows;
    const uint8_t *flags = g.flags;
    const uint32_t n_targets = g.n_targets;
    for (uint64_t step = wave; step < steps; step += n_waves) {
        const uint64_t step_row0 = step * kStepRows;
        uint32_t mbits = 0;
#pragma unroll
        for (uint32_t u = 0; u < 4; u++) {
            const uint64_t r0 = step_row0 + lane * kRplGeneric + (uint64_t)u * 256;
            uint32_t q = 0;
            if (r0 + 4 <= n_rows) q = *(const uint32_t *)(flags + r0);
            else for (uint32_t i = 0; r0 + i < n_rows; i++) q |= (uint32_t)flags[r0 + i] << (8 * i);
            const uint32_t m = ((q & 0xFFu) ? 1u : 0u) | ((q & 0xFF00u) ? 2u : 0u) | ((q & 0xFF0000u) ? 4u : 0u) | ((q & 0xFF000000u) ? 8u : 0u);
            mbits |= m << (4 * u);
        }
        assign_step(g.tgt, n_targets, step_row0, lane, mbits);
    }
}

}  // namespace

// count_many_kernels.hpp -- device code of pqps_filter_count_many: several COUNT(*) WHEREs answered by one scan
// (included once by pqps_hip.hip, after fused_common.hpp).
//
// No counterpart in the reference (it has no aggregates).  A launch carries up to PQPS_COUNT_MANY_MAX queries over the
// union of their columns.  The host has reduced them to DISTINCT window leaves (sorted by column, never negated) and, per
// query, a jump program of at most PQPS_TT_LEAVES steps (leaf slot, on_true, on_false; a negated comparison is a step with
// its two targets swapped).
//
// A wave walks the table in the fused scans' pattern (fused_common.hpp): 1024-row steps wave, wave + n_waves, ... of a
// persistent grid, lane l owns rows l*4 .. l*4+3 of each of the step's four 256-row chunks, bit p of a lane's 16-bit mask
// <-> row step_row0 + (p / 4) * 256 + l * 4 + p % 4.  Per step:
//   1. every column of the union is loaded ONCE (the loads of eval_step_full) and every distinct leaf evaluated ONCE into
//      the lane's 16-bit hit mask (leaf_mask).  The masks are picked by a run-time slot afterwards, so they live in LDS --
//      a u16 per lane and leaf, 16 KiB per workgroup at 32 leaves; a lane reads back only what it wrote itself, so no
//      barrier stands in the loop.  (A register array indexed at run time would go to scratch.)
//   2. each query's program runs BACKWARDS on the masks: val[s] = (m & val[on_true]) | (~m & val[on_false]), one v_bfi for
//      sixteen rows.  The steps are unrolled and the targets picked by uniform switches, so val[] stays in registers; a
//      program whose jumps all go to the next step, accept or reject (an AND / OR ladder) takes cm_step_linear instead.
//   3. the accepted rows are counted (popcount) into the lane's accumulator of the query -- again a uniform switch, 16
//      registers.
// The partial last step is evaluated whole (columns are readable up to the next multiple of 1024 rows) and trimmed with
// rows_below.  After the loop a wave sums each accumulator once (DPP), the workgroup adds its total of every query with a
// non-zero total into one of kCountManySlots rows of the context's partial slots (spread as finish_totals spreads them:
// agent-scope atomics on one 128-byte line serialise), and count_many_reduce_kernel -- one workgroup behind the scan, as
// reduce_totals_kernel is behind a COUNT -- sums the rows into counts[0 .. n_queries) and leaves the slots zeroed.  No
// workgroup waits on another.
#pragma once

namespace {

constexpr uint32_t kCountManySlots = kPartialSlots / PQPS_COUNT_MANY_MAX;   // slot rows of 16 u64 = one 128-byte line each
constexpr uint32_t kCmAccept = 6, kCmReject = 7;                             // jump targets as the program words carry them
constexpr uint32_t kCmLinear = 1u << 9;                                      // word x: every jump goes to the next step, accept or reject

struct CountManyArgs {
    const void *col[PQPS_MAX_COLUMNS];
    uint64_t lo[PQPS_MAX_LEAVES];
    uint64_t span[PQPS_MAX_LEAVES];
    uint64_t n_rows;
    uint64_t *partials;              // [kCountManySlots][PQPS_COUNT_MANY_MAX], zero at launch
    // One query = four 32-bit words (32-bit: picked by a run-time index they are still scalar loads):
    //   x  n_steps | constant << 8 | kCmLinear      y  leaf slot of step s in bits 5s .. 5s+4
    //   z  on_true of step s in bits 3s .. 3s+2 (a later step, kCmAccept or kCmReject)      w  on_false, likewise
    uint32_t prog[PQPS_COUNT_MANY_MAX][4];
    uint32_t n_cols, n_leaves, n_queries;
    uint32_t streaming;              // host side only
    uint32_t width_log2[PQPS_MAX_COLUMNS];
    uint32_t leaf_begin[PQPS_MAX_COLUMNS + 1];   // leaves of column c: [leaf_begin[c], leaf_begin[c+1])
};
typedef const __attribute__((address_space(4))) CountManyArgs CmArgs;

// val[t] for a jump target t of step S (t > S, or accept / reject): a uniform switch keeps val in registers
template <int S>
__device__ __forceinline__ uint32_t cm_target(const uint32_t (&val)[PQPS_TT_LEAVES], uint32_t t) {
    switch (t) {                                                // uniform
    case 1: return S < 1 ? val[1] : 0u;
    case 2: return S < 2 ? val[2] : 0u;
    case 3: return S < 3 ? val[3] : 0u;
    case 4: return S < 4 ? val[4] : 0u;
    case 5: return S < 5 ? val[5] : 0u;
    case kCmAccept: return 0xFFFFu;
    default: return 0u;
    }
}

template <int S>
__device__ __forceinline__ void cm_step(uint32_t (&val)[PQPS_TT_LEAVES], const uint4 w, const uint16_t *my_masks) {
    if ((uint32_t)S >= (w.x & 0xFFu)) return;                   // uniform
    const uint32_t m = my_masks[((w.y >> (5 * S)) & 31u) * kBlock];
    const uint32_t vt = cm_target<S>(val, (w.z >> (3 * S)) & 7u), vf = cm_target<S>(val, (w.w >> (3 * S)) & 7u);
    val[S] = (m & vt) | (~m & vf);
}

// A LINEAR program -- every jump goes to the next step, to accept or to reject: an AND / OR ladder in any polarity, i.e. nearly
// every clause of a dashboard -- needs no pick among val[]: with nx = val[S + 1], a target is (nx & a) | o for two uniform
// masks, so a step is three vector operations and no branch on a target.
template <int S>
__device__ __forceinline__ void cm_step_linear(uint32_t &nx, const uint4 w, const uint16_t *my_masks) {
    if ((uint32_t)S >= (w.x & 0xFFu)) return;                   // uniform
    const uint32_t m = my_masks[((w.y >> (5 * S)) & 31u) * kBlock];
    const uint32_t t = (w.z >> (3 * S)) & 7u, f = (w.w >> (3 * S)) & 7u;
    const uint32_t vt = (nx & (t == (uint32_t)S + 1u ? 0xFFFFu : 0u)) | (t == kCmAccept ? 0xFFFFu : 0u);
    const uint32_t vf = (nx & (f == (uint32_t)S + 1u ? 0xFFFFu : 0u)) | (f == kCmAccept ? 0xFFFFu : 0u);
    nx = (m & vt) | (~m & vf);
}

__device__ __forceinline__ void cm_add(uint32_t (&acc)[PQPS_COUNT_MANY_MAX], uint32_t q, uint32_t c) {
    switch (q) {                                                // uniform: keeps acc in registers
    case 0: acc[0] += c; break;   case 1: acc[1] += c; break;   case 2: acc[2] += c; break;   case 3: acc[3] += c; break;
    case 4: acc[4] += c; break;   case 5: acc[5] += c; break;   case 6: acc[6] += c; break;   case 7: acc[7] += c; break;
    case 8: acc[8] += c; break;   case 9: acc[9] += c; break;   case 10: acc[10] += c; break; case 11: acc[11] += c; break;
    case 12: acc[12] += c; break; case 13: acc[13] += c; break; case 14: acc[14] += c; break; default: acc[15] += c; break;
    }
}

// The values of a lane's 16 rows of one step of a 1, 2 or 4 byte column, v[p] <-> mask bit p: the loads of eval_step_full (one
// dwordx4 / dwordx2 / dword per 256-row chunk).  `at` = the column at the step's first row, wave-uniform, so the address is a scalar base plus
// the lane's 32-bit byte offset and nothing per lane and column stays live across steps.
template <bool NT>
__device__ __forceinline__ void cm_load_u32(const char *at, uint32_t wl, uint32_t lane, uint32_t (&v)[16]) {
#pragma unroll
    for (uint32_t u = 0; u < 4; u++) {
        if (wl == 2) {
            const uint4 q = ld_x4<NT>(at + (lane * 16u + u * 1024u));
            v[4 * u] = q.x; v[4 * u + 1] = q.y; v[4 * u + 2] = q.z; v[4 * u + 3] = q.w;
        } else if (wl == 1) {
            const uint2 q = ld_x2<NT>(at + (lane * 8u + u * 512u));
            v[4 * u] = q.x & 0xFFFFu; v[4 * u + 1] = q.x >> 16;
            v[4 * u + 2] = q.y & 0xFFFFu; v[4 * u + 3] = q.y >> 16;
        } else {
            const uint32_t q = ld_x1<NT>(at + (lane * 4u + u * 256u));
            v[4 * u] = q & 0xFFu; v[4 * u + 1] = (q >> 8) & 0xFFu;
            v[4 * u + 2] = (q >> 16) & 0xFFu; v[4 * u + 3] = q >> 24;
        }
    }
}

// Hit masks of every leaf of the union for one step, into the lane's column of the LDS table.
template <bool NT>
__device__ __forceinline__ void cm_leaf_masks(CmArgs &g, uint64_t step_row0, uint32_t lane, uint16_t *my_masks) {
    const uint32_t n_cols = g.n_cols;
    for (uint32_t c = 0; c < n_cols; c++) {                     // uniform
        const char *base = (const char *)g.col[c];
        const uint32_t wl = g.width_log2[c];
        const uint32_t kb = g.leaf_begin[c], ke = g.leaf_begin[c + 1];
        if (wl == 3) {
            const char *at = base + step_row0 * 8;
#pragma unroll
            for (uint32_t h = 0; h < 2; h++) {                  // two halves keep live registers down
                uint64_t v[8];
#pragma unroll
                for (uint32_t u = 0; u < 2; u++) {
                    const char *p = at + (lane * 32u + (2 * h + u) * 2048u);
                    const uint4 q0 = ld_x4<NT>(p), q1 = ld_x4<NT>(p + 16);
                    v[4 * u + 0] = (uint64_t)q0.x | ((uint64_t)q0.y << 32); v[4 * u + 1] = (uint64_t)q0.z | ((uint64_t)q0.w << 32);
                    v[4 * u + 2] = (uint64_t)q1.x | ((uint64_t)q1.y << 32); v[4 * u + 3] = (uint64_t)q1.z | ((uint64_t)q1.w << 32);
                }
                for (uint32_t k = kb; k < ke; k++) {            // uniform; operands come in SGPRs
                    const uint32_t m = leaf_mask<uint64_t, 8>(v, g.lo[k], g.span[k]);
                    if (h == 0) my_masks[k * kBlock] = (uint16_t)m;
                    else my_masks[k * kBlock] |= (uint16_t)(m << 8);
                }
            }
        } else if (wl == kWidthLog2Bits) {                      // bit plane: the lane's 4 rows of a chunk are a nibble of byte lane / 2
            const char *at = base + (step_row0 >> 3) + (lane >> 1);
            uint32_t bits = 0;
#pragma unroll
            for (uint32_t u = 0; u < 4; u++) bits |= ((ld_u8<NT>(at + u * 32u) >> ((lane & 1u) * 4u)) & 0xFu) << (4 * u);
            for (uint32_t k = kb; k < ke; k++)                  // the window test of a 0 / 1 value: the bits, their complement, all or none
                my_masks[k * kBlock] = (uint16_t)bit_leaf_hits(bits, g.lo[k], g.span[k]);
        } else {
            uint32_t v[16];
            cm_load_u32<NT>(base + (step_row0 << wl), wl, lane, v);
            for (uint32_t k = kb; k < ke; k++)
                my_masks[k * kBlock] = (uint16_t)leaf_mask<uint32_t, 16>(v, (uint32_t)g.lo[k], (uint32_t)g.span[k]);
        }
    }
}

template <bool NT>
__global__ __launch_bounds__(kBlock, 1) void count_many_scan_kernel(const CountManyArgs) {
    CmArgs &g = kernarg<CountManyArgs>();
    __shared__ uint16_t s_mask[PQPS_MAX_LEAVES][kBlock];        // [leaf][thread]: 16 KiB
    __shared__ uint32_t s_tot[kWaves][PQPS_COUNT_MANY_MAX];
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // uniform, and the compiler knows: steps and bases stay scalar
    uint16_t *my_masks = &s_mask[0][threadIdx.x];
    const uint32_t n_queries = g.n_queries;
    const uint64_t n_rows = g.n_rows;
    const uint64_t wave = (uint64_t)blockIdx.x * kWaves + wv, n_waves = (uint64_t)gridDim.x * kWaves;
    const uint64_t steps = (n_rows + kStepRows - 1) / kStepRows;
    uint32_t acc[PQPS_COUNT_MANY_MAX];
#pragma unroll
    for (uint32_t q = 0; q < PQPS_COUNT_MANY_MAX; q++) acc[q] = 0;

    for (uint64_t step = wave; step < steps; step += n_waves) {
        const uint64_t step_row0 = step * kStepRows;
        cm_leaf_masks<NT>(g, step_row0, lane, my_masks);
        uint32_t live = 0xFFFFu;
        if (step_row0 + kStepRows > n_rows) live = rows_below<kRplGeneric>(step_row0, n_rows, lane);   // the partial last step
        for (uint32_t q = 0; q < n_queries; q++) {              // uniform
            const uint4 w = make_uint4(g.prog[q][0], g.prog[q][1], g.prog[q][2], g.prog[q][3]);
            uint32_t res;
            if (w.x & kCmLinear) {                              // uniform
                res = 0;
                cm_step_linear<5>(res, w, my_masks);
                cm_step_linear<4>(res, w, my_masks);
                cm_step_linear<3>(res, w, my_masks);
                cm_step_linear<2>(res, w, my_masks);
                cm_step_linear<1>(res, w, my_masks);
                cm_step_linear<0>(res, w, my_masks);
            } else {
                uint32_t val[PQPS_TT_LEAVES];
                val[0] = (w.x >> 8) & 1u ? 0xFFFFu : 0u;        // no step: the constant
                cm_step<5>(val, w, my_masks);
                cm_step<4>(val, w, my_masks);
                cm_step<3>(val, w, my_masks);
                cm_step<2>(val, w, my_masks);
                cm_step<1>(val, w, my_masks);
                cm_step<0>(val, w, my_masks);
                res = val[0];
            }
            cm_add(acc, q, (uint32_t)__popc(res & live));
        }
    }

#pragma unroll
    for (uint32_t q = 0; q < PQPS_COUNT_MANY_MAX; q++) {
        if (q < n_queries) {                                    // uniform
            const uint32_t t = wave_sum_u32(acc[q]);
            if (lane == 0) s_tot[wv][q] = t;
        }
    }
    __syncthreads();
    if (threadIdx.x < n_queries) {
        uint64_t t = 0;
        for (uint32_t i = 0; i < (uint32_t)kWaves; i++) t += s_tot[i][threadIdx.x];
        if (t) atomicAdd((unsigned long long *)&g.partials[(blockIdx.x & (kCountManySlots - 1)) * PQPS_COUNT_MANY_MAX + threadIdx.x],
                         (unsigned long long)t);
    }
}

// One workgroup: counts[q] = the sum of column q of the slot rows, every slot requested at once and left zeroed for the
// next query (reduce_totals_kernel reads the same words as one array).
__global__ __launch_bounds__(kBlock) void count_many_reduce_kernel(uint64_t *partials, uint64_t *counts, uint32_t n_queries) {
    constexpr uint32_t kPer = kPartialSlots / kBlock;
    __shared__ unsigned long long s_sum[PQPS_COUNT_MANY_MAX];
    if (threadIdx.x < PQPS_COUNT_MANY_MAX) s_sum[threadIdx.x] = 0;
    uint64_t v[kPer];
#pragma unroll
    for (uint32_t k = 0; k < kPer; k++) v[k] = partials[threadIdx.x + k * kBlock];   // (kBlock is a multiple of 16: all of query threadIdx.x & 15)
    uint64_t local = 0;
#pragma unroll
    for (uint32_t k = 0; k < kPer; k++) {
        local += v[k];
        if (v[k]) partials[threadIdx.x + k * kBlock] = 0;
    }
    __syncthreads();
    if (local) atomicAdd(&s_sum[threadIdx.x & (PQPS_COUNT_MANY_MAX - 1)], (unsigned long long)local);
    __syncthreads();
    if (threadIdx.x < n_queries) counts[threadIdx.x] = s_sum[threadIdx.x];
}

}  // namespace

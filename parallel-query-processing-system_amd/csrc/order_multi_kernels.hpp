// order_multi_kernels.hpp -- device code of ORDER BY k1 [DESC], ... , kN [DESC] LIMIT K (included once by pqps_hip.hip,
// after topk_kernels.hpp).
//
// The keys of a row are packed into ONE unsigned number whose ascending order is the lexicographic order of the keys, each
// in its own direction.  Field j of a row holding value v in its column:
//     bin = v - base_j (32-bit arithmetic)        field = min(bin, mask_j) ^ (descending ? mask_j : 0)
//     packed |= field << shift_j                    mask_j = 2^bits_j - 1
// The min never bites for a caller whose bases and bit counts are exact; it keeps a value outside its domain out of the
// neighbouring fields.  With T = the sum of the bits the composite key is
//     T <= 32 (PACK32)   one u64: packed << 32 | row     -- bit for bit the narrow key of topk_kernels.hpp
//     T <= 64 (PACK64)   the pair (packed, row)          -- the wide key
// so WaveTopK<WIDE>, topk_select_kernel<WIDE, false>, the radix sort and the host's merge take them as they are.
//
// topk_pack_scan_kernel<WIDE, NF, NT>: topk_scan_kernel's loop with NF key columns.  NF is a template parameter, and a
// column's loads are split from their unpacking (issue_step_raw / unpack_step_raw): the width branches of the issue phase
// hold loads only, so no wait lands inside them, and the 4 x NF loads of a step are in flight together before the first
// field is unpacked and reduced.  The fields' parameters are read from the kernel-argument segment in the step that uses
// them (scalar loads the scalar cache serves), not kept in SGPRs across the WHERE's evaluation.
// order_pack_keys_kernel<WIDE>: the same keys of the entries of an ID list, gathered by row (byte columns only).
#pragma once

namespace {

constexpr int kOrderMaxFields = 4;

struct OrderField {
    const void *col;                 // 1, 2 or 4 bytes per row, or (scan only) a bit plane
    uint32_t wl;                     // 0, 1, 2 or kWidthLog2Bits
    uint32_t base, mask, shift;
    uint32_t flip;                   // mask when descending, else 0
};

struct PackArgs {
    EvalArgs e;                      // the WHERE -- first: the scan loop reads it in place
    OrderField f[kOrderMaxFields];
    void *parts;                     // [gridDim.x * kWaves][k] keys, each wave's sorted K best
    unsigned long long *count;       // += the matching rows (one atomic per workgroup; zeroed before the launch)
    uint32_t row_base;               // table-wide row number of row 0
    uint32_t k, cap;
};

__device__ __forceinline__ uint32_t order_field(uint32_t v, uint32_t base, uint32_t mask, uint32_t flip) {
    const uint32_t bin = v - base;
    return (bin < mask ? bin : mask) ^ flip;
}

// The raw words of a lane's 16 rows of one full step of a 1, 2 or 4 byte column or a bit plane: load_step_u32 in two halves,
// the loads here and what they mean in unpack_step_raw.
template <bool NT>
__device__ __forceinline__ void issue_step_raw(const char *base, uint32_t wl, uint64_t step_row0, uint32_t lane, uint4 (&q)[4]) {
    const uint64_t lane_row0 = step_row0 + lane * kRplGeneric;
    if (wl == 2) {
#pragma unroll
        for (int u = 0; u < 4; u++) q[u] = ld_x4<NT>(base + (lane_row0 + (uint64_t)u * 256) * 4);
    } else if (wl == 1) {
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const uint2 t = ld_x2<NT>(base + (lane_row0 + (uint64_t)u * 256) * 2);
            q[u].x = t.x; q[u].y = t.y;
        }
    } else if (wl == kWidthLog2Bits) {                          // bit plane: the lane's 4 rows are a nibble of this byte
#pragma unroll
        for (int u = 0; u < 4; u++) q[u].x = ld_u8<NT>(base + ((lane_row0 + (uint64_t)u * 256) >> 3));
    } else {
#pragma unroll
        for (int u = 0; u < 4; u++) q[u].x = ld_x1<NT>(base + lane_row0 + (uint64_t)u * 256);
    }
}

__device__ __forceinline__ void unpack_step_raw(uint32_t wl, uint32_t lane, const uint4 (&q)[4], uint32_t (&v)[16]) {
#pragma unroll
    for (int u = 0; u < 4; u++) {
        if (wl == 2) {
            v[4 * u] = q[u].x; v[4 * u + 1] = q[u].y; v[4 * u + 2] = q[u].z; v[4 * u + 3] = q[u].w;
        } else if (wl == 1) {
            v[4 * u] = q[u].x & 0xFFFFu; v[4 * u + 1] = q[u].x >> 16;
            v[4 * u + 2] = q[u].y & 0xFFFFu; v[4 * u + 3] = q[u].y >> 16;
        } else if (wl == kWidthLog2Bits) {                      // rows lane * 4 + u * 256 ..: bit (lane * 4) & 4 of the byte on
            const uint32_t t = q[u].x >> ((lane * kRplGeneric) & 4u);
            v[4 * u] = t & 1u; v[4 * u + 1] = (t >> 1) & 1u;
            v[4 * u + 2] = (t >> 2) & 1u; v[4 * u + 3] = (t >> 3) & 1u;
        } else {
            v[4 * u] = q[u].x & 0xFFu; v[4 * u + 1] = (q[u].x >> 8) & 0xFFu;
            v[4 * u + 2] = (q[u].x >> 16) & 0xFFu; v[4 * u + 3] = q[u].x >> 24;
        }
    }
}

template <bool WIDE> struct PackWord;
template <> struct PackWord<false> { using type = uint32_t; };
template <> struct PackWord<true> { using type = uint64_t; };

template <bool WIDE> __device__ __forceinline__ TKey<WIDE> packed_key(typename PackWord<WIDE>::type packed, uint32_t row);
template <> __device__ __forceinline__ TKey<false> packed_key<false>(uint32_t packed, uint32_t row) {
    return TKey<false>{((uint64_t)packed << 32) | row};
}
template <> __device__ __forceinline__ TKey<true> packed_key<true>(uint64_t packed, uint32_t row) {
    return TKey<true>{packed, row};
}

template <bool WIDE, int NF, bool NT>
__global__ __launch_bounds__(kBlock, 1) void topk_pack_scan_kernel(const PackArgs) {
    using W = typename PackWord<WIDE>::type;
    const auto &g = kernarg<PackArgs>();
    CArgs &a = g.e;
    extern __shared__ uint64_t topk_lds[];
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t row_base = g.row_base;
    const uint64_t wave = (uint64_t)blockIdx.x * kWaves + wv;
    const uint64_t n_waves = (uint64_t)gridDim.x * kWaves;
    const uint64_t n_rows = a.n_rows;
    const uint64_t steps = (n_rows + kStepRows - 1) / kStepRows;
    WaveTopK<WIDE> w;
    w.init((TKey<WIDE> *)topk_lds + (uint64_t)wv * g.cap, g.cap, g.k, lane);
    uint32_t cnt = 0;
    for (uint64_t step = wave; step < steps; step += n_waves) {     // fused_scan_steps, written out
        const uint64_t step_row0 = step * kStepRows;
        uint32_t mbits = eval_step_full<NT>(a, step_row0, lane);
        if (step_row0 + kStepRows > n_rows) mbits &= rows_below<kRplGeneric>(step_row0, n_rows, lane);
        if (__ballot(mbits != 0u) == 0) continue;
        cnt += __popc(mbits);
        const __attribute__((address_space(4))) PackArgs *gs = &g;
        asm volatile("" : "+s"(gs));                            // the fields are read here, in every step that gets here
        uint4 q[NF][4] = {};
#pragma unroll
        for (int j = 0; j < NF; j++) issue_step_raw<NT>((const char *)gs->f[j].col, gs->f[j].wl, step_row0, lane, q[j]);
        W packed[16];
#pragma unroll
        for (int p = 0; p < 16; p++) packed[p] = 0;
#pragma unroll
        for (int j = 0; j < NF; j++) {
            const uint32_t base = gs->f[j].base, mask = gs->f[j].mask, shift = gs->f[j].shift, flip = gs->f[j].flip;
            uint32_t u[16];
            unpack_step_raw(gs->f[j].wl, lane, q[j], u);
#pragma unroll
            for (int p = 0; p < 16; p++) packed[p] |= (W)order_field(u[p], base, mask, flip) << shift;
        }
        const uint32_t lane_row0 = row_base + (uint32_t)step_row0 + lane * kRplGeneric;
#pragma unroll
        for (int p = 0; p < 16; p++)                            // bit p <-> row lane_row0 + (p / 4) * 256 + p % 4
            w.push((mbits >> p) & 1u, packed_key<WIDE>(packed[p], lane_row0 + (uint32_t)(p / 4) * 256u + (uint32_t)(p % 4)), lane);
    }
    w.store((TKey<WIDE> *)g.parts + wave * g.k, lane);
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

struct PackListArgs {
    OrderField f[kOrderMaxFields];
    uint32_t n_fields, id_base;
};

// The key of every entry of rows[0 .. n) (table-wide; local row rows[i] - id_base of the fields' columns).  keys: the
// composite TKey<WIDE> of the top-K rounds; packed: the packed word alone as u64, the radix sort's key.  Either may be NULL.
template <bool WIDE>
__global__ __launch_bounds__(kBlock) void order_pack_keys_kernel(const uint32_t *__restrict__ rows, uint64_t n, const PackListArgs g,
                                                                 TKey<WIDE> *__restrict__ keys, uint64_t *__restrict__ packed) {
    using W = typename PackWord<WIDE>::type;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t row = rows[i];
        const uint64_t r = (uint64_t)(row - g.id_base);
        W pk = 0;
        for (uint32_t j = 0; j < g.n_fields; j++) {
            const OrderField &f = g.f[j];
            pk |= (W)order_field(gather_narrow(f.col, f.wl, r), f.base, f.mask, f.flip) << f.shift;
        }
        if (keys) keys[i] = packed_key<WIDE>(pk, row);
        if (packed) packed[i] = (uint64_t)pk;
    }
}

}  // namespace

// member_kernels.hpp -- set membership of one column, row by row: the member pass of a WHERE with LIKE / IN (included once by
// pqps_hip.hip, after fused_common.hpp).
//
// The host has decided the set (include/hipPredicate.h); the device only asks "is this row's code in it".  A thread owns the 8
// rows of one plane byte: one streaming load of 8, 16, 32 or 64 bytes (ld_x2 / ld_x4 of filter_kernels.hpp), eight lookups,
// one store -- the plane byte, or the eight flag bytes as one 8-byte store.  Lookup forms:
//   MEMBER_LDS     the bitmap staged into LDS by every workgroup (up to PQPS_MEMBER_LDS_BITS bits = 32 KiB: five workgroups
//                  per CU by LDS, more than the two the streaming loads need to cover each other's latency)
//   MEMBER_GLOBAL  the bitmap read from global memory: 2^27 bits are 16 MiB, which stay in L2 / Infinity Cache
//   MEMBER_LIST    binary search in the ascending u64 list (command_id, far-apart i32 values): log2(n_list) dependent loads
// Rows at and past n_rows are never members; a plane is written up to the padded row count, bytes only for real rows.
// No kernel here waits on another workgroup.
#pragma once

namespace {

enum { MEMBER_LDS = 0, MEMBER_GLOBAL = 1, MEMBER_LIST = 2 };
constexpr uint32_t kMemberLdsWords = PQPS_MEMBER_LDS_BITS / 32;
constexpr uint32_t kMemberBlock = 256;

struct MemberArgs {
    const char *col;
    uint64_t n_rows;
    uint64_t octets;             // groups of 8 rows to write: plane: padded rows / 8, bytes: ceil(n_rows / 8)
    uint32_t base;
    uint64_t n_bits;
    const uint32_t *bitmap;
    const uint64_t *list;
    uint32_t n_list;
    uint8_t *out;
    unsigned long long *count;   // zeroed by the host side before the launch; may be nullptr
};

// the values of rows [r0, r0 + 8) of a column of WIDTH bytes, zero-extended (r0 a multiple of 8, the column 16-byte aligned)
template <int WIDTH>
__device__ __forceinline__ void member_load8(const char *col, uint64_t r0, uint64_t (&v)[8]) {
    if constexpr (WIDTH == 1) {
        const uint2 q = ld_x2<true>(col + r0);
#pragma unroll
        for (int i = 0; i < 4; i++) { v[i] = (q.x >> (8 * i)) & 0xFFu; v[4 + i] = (q.y >> (8 * i)) & 0xFFu; }
    } else if constexpr (WIDTH == 2) {
        const uint4 q = ld_x4<true>(col + r0 * 2);
        v[0] = q.x & 0xFFFFu; v[1] = q.x >> 16; v[2] = q.y & 0xFFFFu; v[3] = q.y >> 16;
        v[4] = q.z & 0xFFFFu; v[5] = q.z >> 16; v[6] = q.w & 0xFFFFu; v[7] = q.w >> 16;
    } else if constexpr (WIDTH == 4) {
        const uint4 q0 = ld_x4<true>(col + r0 * 4), q1 = ld_x4<true>(col + r0 * 4 + 16);
        v[0] = q0.x; v[1] = q0.y; v[2] = q0.z; v[3] = q0.w; v[4] = q1.x; v[5] = q1.y; v[6] = q1.z; v[7] = q1.w;
    } else {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint4 q = ld_x4<true>(col + r0 * 8 + 16 * i);
            v[2 * i] = (uint64_t)q.x | ((uint64_t)q.y << 32);
            v[2 * i + 1] = (uint64_t)q.z | ((uint64_t)q.w << 32);
        }
    }
}

template <int FORM>
__device__ __forceinline__ bool member_test(const MemberArgs &a, const uint32_t *words, uint64_t v) {
    if constexpr (FORM == MEMBER_LIST) {
        uint32_t lo = 0, hi = a.n_list;                            // first entry >= v
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (a.list[mid] < v) lo = mid + 1; else hi = mid;
        }
        return lo < a.n_list && a.list[lo] == v;
    } else {
        const uint32_t idx = (uint32_t)v - a.base;                 // a value below base wraps far past n_bits
        if ((uint64_t)idx >= a.n_bits) return false;
        return (words[idx >> 5] >> (idx & 31u)) & 1u;
    }
}

template <int WIDTH, int FORM, bool PLANE>
__global__ __launch_bounds__(kMemberBlock) void member_kernel(const MemberArgs a) {
    __shared__ uint32_t s_bits[FORM == MEMBER_LDS ? kMemberLdsWords : 1];
    __shared__ uint32_t s_tot[kMemberBlock / 64];
    const uint32_t *words = a.bitmap;
    if constexpr (FORM == MEMBER_LDS) {
        const uint32_t n_words = (uint32_t)((a.n_bits + 31) / 32);  // <= kMemberLdsWords: the host side chose this form
        for (uint32_t w = threadIdx.x; w < n_words; w += kMemberBlock) s_bits[w] = a.bitmap[w];
        __syncthreads();
        words = s_bits;
    }
    uint32_t mine = 0;
    for (uint64_t o = (uint64_t)blockIdx.x * kMemberBlock + threadIdx.x; o < a.octets; o += (uint64_t)gridDim.x * kMemberBlock) {
        const uint64_t r0 = o * 8;
        uint32_t bits = 0;
        if (r0 < a.n_rows) {
            uint64_t v[8];
            member_load8<WIDTH>(a.col, r0, v);
#pragma unroll
            for (int i = 0; i < 8; i++) bits |= member_test<FORM>(a, words, v[i]) ? (1u << i) : 0u;
            if (r0 + 8 > a.n_rows) bits &= (1u << (uint32_t)(a.n_rows - r0)) - 1u;
        }
        mine += __popc(bits);
        if constexpr (PLANE) {
            a.out[o] = (uint8_t)bits;
        } else if (r0 + 8 <= a.n_rows) {
            uint2 q;
            q.x = (bits & 1u) | ((bits & 2u) << 7) | ((bits & 4u) << 14) | ((bits & 8u) << 21);
            q.y = ((bits >> 4) & 1u) | ((bits & 0x20u) << 3) | ((bits & 0x40u) << 10) | ((bits & 0x80u) << 17);
            *(uint2 *)(a.out + r0) = q;
        } else {
            for (uint64_t i = 0; r0 + i < a.n_rows; i++) a.out[r0 + i] = (uint8_t)((bits >> i) & 1u);
        }
    }
    if (a.count) {
        const uint32_t wave = wave_sum_u32(mine);
        if ((threadIdx.x & 63u) == 0) s_tot[threadIdx.x >> 6] = wave;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t t = 0;
            for (uint32_t i = 0; i < kMemberBlock / 64; i++) t += s_tot[i];
            if (t) atomicAdd(a.count, (unsigned long long)t);
        }
    }
}

template <int WIDTH, int FORM>
void member_launch(bool plane, uint32_t blocks, hipStream_t s, const MemberArgs &a) {
    if (plane) hipLaunchKernelGGL((member_kernel<WIDTH, FORM, true>), dim3(blocks), dim3(kMemberBlock), 0, s, a);
    else hipLaunchKernelGGL((member_kernel<WIDTH, FORM, false>), dim3(blocks), dim3(kMemberBlock), 0, s, a);
}

template <int FORM>
void member_launch_width(uint32_t width, bool plane, uint32_t blocks, hipStream_t s, const MemberArgs &a) {
    if (width == 1) member_launch<1, FORM>(plane, blocks, s, a);
    else if (width == 2) member_launch<2, FORM>(plane, blocks, s, a);
    else if (width == 4) member_launch<4, FORM>(plane, blocks, s, a);
    else if constexpr (FORM == MEMBER_LIST) member_launch<8, FORM>(plane, blocks, s, a);
}

}  // namespace

// topk_kernels.hpp -- device code of ORDER BY column [DESC] LIMIT K (included once by pqps_hip.hip, after fused_common.hpp).
//
// No counterpart in the reference (it parses ORDER BY and executes none).  Every row is one COMPOSITE key whose ascending
// order is the answer's order -- key ascending or descending, ties by ascending table-wide row number:
//   narrow (i32, dictionary codes, the bool bit)  one u64: (img ^ x) << 32 | row, img = v ^ 2^31 for i32, the code or the
//                                                 bit otherwise, x = 0xFFFFFFFF for DESC and 0 for ASC
//   wide   (command_id)                           two u64 words (v ^ x, row), x = ~0 for DESC
// so every comparison is a native unsigned one (two for the wide form).  The all-ones key is the empty slot: no real key
// reaches it, since row numbers stay below 2^32 - 1.
//
// Selection, one WAVE at a time (no barrier inside the persistent loop): a wave keeps `cap` keys in LDS (cap a power of
// two >= 2 K and >= K + 64), the empty slots holding all-ones, and a threshold tau = its K-th best so far (all-ones until
// it holds K).  Every 64 candidates (one row slot of a step, or 64 list entries) are one ballot: the lanes whose key is
// below tau append it behind `fill`.  When the next 64 might not fit, the wave bitonic-sorts its buffer, keeps the K best
// and tightens tau (compact).  A compaction admits cap - K >= K new keys, so each key costs amortised O(log^2 cap) LDS
// compare-exchanges whatever the order of the input -- also when every match beats tau (a key monotone in scan
// direction, such as ORDER BY command_id DESC over the synthetic table).
//
// topk_scan_kernel (pqps_filter_topk): the shared scan loop (fused_common.hpp) with the key loads per step that holds a
// match, written out in this kernel (why: DESIGN.md §7a).  At the end every wave stores its sorted K best as a partial row and
// every workgroup adds its match count with ONE atomic.  topk_select_kernel: one wave per `chunk` consecutive keys of a partial-row
// array (the follow-up rounds: grid x 4 x K keys to K), or of an ID list whose keys it gathers (pqps_topk_list); rounds until one wave is left.
#pragma once

namespace {

constexpr uint32_t kTopkMax = 1024;          // narrow keys: 2048 x 8 B = 16 KiB of LDS per wave, 2 workgroups per CU
constexpr uint32_t kTopkMaxWide = 512;       // command_id: 16 B per key, the same 16 KiB per wave
constexpr uint32_t kTopkMinCap = 128;        // cap >= K + 64 for every K (a ballot appends at most 64)
constexpr uint64_t kTopkChunk = 16;          // a follow-up wave selects from at least 16 K keys

template <bool WIDE> struct TKey;
template <> struct TKey<false> {
    uint64_t a;
    __device__ __forceinline__ bool operator<(const TKey &o) const { return a < o.a; }
    __device__ __forceinline__ static TKey top() { return TKey{~0ull}; }
};
template <> struct TKey<true> {
    uint64_t a, b;                           // image, row
    __device__ __forceinline__ bool operator<(const TKey &o) const { return a < o.a || (a == o.a && b < o.b); }
    __device__ __forceinline__ static TKey top() { return TKey{~0ull, ~0ull}; }
};

template <bool WIDE> __device__ __forceinline__ TKey<WIDE> make_key(uint64_t raw, uint64_t kxor, uint32_t row);
template <> __device__ __forceinline__ TKey<false> make_key<false>(uint64_t raw, uint64_t kxor, uint32_t row) {
    return TKey<false>{((uint64_t)(((uint32_t)raw) ^ (uint32_t)kxor) << 32) | row};
}
template <> __device__ __forceinline__ TKey<true> make_key<true>(uint64_t raw, uint64_t kxor, uint32_t row) {
    return TKey<true>{raw ^ kxor, row};
}

// LDS written by some lanes of the wave and read by others: program order within the wave, nothing moved across
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// One wave's candidate buffer (the members are the same in every lane).
template <bool WIDE> struct WaveTopK {
    TKey<WIDE> *buf;
    uint32_t cap, k, fill;
    TKey<WIDE> tau;

    __device__ __forceinline__ void init(TKey<WIDE> *b, uint32_t c, uint32_t kk, uint32_t lane) {
        buf = b; cap = c; k = kk; fill = 0;
        tau = TKey<WIDE>::top();
        for (uint32_t i = lane; i < cap; i += 64) buf[i] = TKey<WIDE>::top();
        wave_lds_sync();
    }
    // ascending bitonic sort of all cap slots (the empty ones sort last)
    __device__ __forceinline__ void sort(uint32_t lane) {
        for (uint32_t size = 2; size <= cap; size <<= 1) {
            for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
                for (uint32_t i = lane; i < cap / 2; i += 64) {
                    const uint32_t lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
                    const bool up = (lo & size) == 0;
                    const TKey<WIDE> x = buf[lo], y = buf[hi];
                    if ((y < x) == up) { buf[lo] = y; buf[hi] = x; }
                }
                wave_lds_sync();
            }
        }
    }
    // the K best sorted in front, the rest emptied, tau = the K-th best once there are K
    __device__ __forceinline__ void compact(uint32_t lane) {
        sort(lane);
        if (fill > k) fill = k;
        for (uint32_t i = k + lane; i < cap; i += 64) buf[i] = TKey<WIDE>::top();
        wave_lds_sync();
        if (fill == k) tau = buf[k - 1];
    }
    // one candidate per lane: appended if valid and below tau
    __device__ __forceinline__ void push(bool valid, const TKey<WIDE> &key, uint32_t lane) {
        const bool want = valid && key < tau;
        const uint64_t m = __ballot(want);
        if (m == 0) return;
        const uint32_t n = (uint32_t)__popcll(m);
        if (fill + n > cap) compact(lane);                      // (uniform) then fill <= k <= cap - 64
        const uint64_t below = lane ? m & (~0ull >> (64 - lane)) : 0ull;
        if (want) buf[fill + (uint32_t)__popcll(below)] = key;
        fill += n;
        wave_lds_sync();
    }
    // sorted K best to out[0 .. k)
    __device__ __forceinline__ void store(TKey<WIDE> *out, uint32_t lane) {
        compact(lane);
        for (uint32_t i = lane; i < k; i += 64) out[i] = buf[i];
    }
};

struct TopkArgs {
    EvalArgs e;                      // the WHERE, as the COUNT kernels take it -- first: the scan loop reads it in place
    const void *kcol;                // key column (narrow: bytes, u16, u32 or a bit plane; wide: u64); nullptr: every key 0
    void *parts;                     // [gridDim.x * kWaves][k] keys, each wave's sorted K best
    unsigned long long *count;       // += the matching rows (one atomic per workgroup; zeroed before the launch)
    uint64_t kxor;                   // image xor (i32 sign flip, DESC complement)
    uint32_t kwidth_log2;            // narrow: 0, 1, 2 or kWidthLog2Bits
    uint32_t row_base;               // table-wide row number of row 0
    uint32_t k, cap;
};

template <bool WIDE, bool NT>
__global__ __launch_bounds__(kBlock, 1) void topk_scan_kernel(const TopkArgs) {
    const auto &g = kernarg<TopkArgs>();
    CArgs &a = g.e;
    extern __shared__ uint64_t topk_lds[];
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const char *kbase = (const char *)g.kcol;
    const uint64_t kxor = g.kxor;
    const uint32_t wl = g.kwidth_log2, row_base = g.row_base;
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
        uint64_t v[16];
        if constexpr (WIDE) {
            load_step_u64<true, NT>(kbase, step_row0, lane, v);
        } else {
            uint32_t u[16];
            if (kbase) load_step_u32<NT>(kbase, wl, step_row0, lane, u);
            else {
#pragma unroll
                for (int p = 0; p < 16; p++) u[p] = 0;
            }
#pragma unroll
            for (int p = 0; p < 16; p++) v[p] = u[p];
        }
        const uint32_t lane_row0 = row_base + (uint32_t)step_row0 + lane * kRplGeneric;
#pragma unroll
        for (int p = 0; p < 16; p++)                            // bit p <-> row lane_row0 + (p / 4) * 256 + p % 4
            w.push((mbits >> p) & 1u, make_key<WIDE>(v[p], kxor, lane_row0 + (uint32_t)(p / 4) * 256u + (uint32_t)(p % 4)), lane);
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

// Wave gw of the launch selects from keys [gw * chunk, min(n, (gw + 1) * chunk)) and stores its sorted K best at
// out[gw * k].  GATHER: key i is that of list entry ids[i] (table-wide row; local row ids[i] - id_base of `kcol`, whose
// width is 1 << kwl bytes; nullptr: every key 0); otherwise in[i].  Waves past n_waves store nothing.
template <bool WIDE, bool GATHER>
__global__ __launch_bounds__(kBlock) void topk_select_kernel(const TKey<WIDE> *__restrict__ in, const uint32_t *__restrict__ ids,
                                                             const void *kcol, uint32_t kwl, uint64_t kxor, uint32_t id_base,
                                                             uint64_t n, uint64_t chunk, uint64_t n_waves, uint32_t k, uint32_t cap,
                                                             TKey<WIDE> *__restrict__ out) {
    extern __shared__ uint64_t topk_lds[];
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint64_t gw = (uint64_t)blockIdx.x * kWaves + wv;
    if (gw >= n_waves) return;                                  // (no barrier below)
    WaveTopK<WIDE> w;
    w.init((TKey<WIDE> *)topk_lds + (uint64_t)wv * cap, cap, k, lane);
    const uint64_t begin = gw * chunk;
    const uint64_t end = begin + chunk < n ? begin + chunk : n;
    for (uint64_t base = begin; base < end; base += 64) {
        const uint64_t i = base + lane;
        const bool valid = i < end;
        TKey<WIDE> key = TKey<WIDE>::top();
        if (valid) {
            if constexpr (GATHER) {
                const uint32_t row = ids[i];
                key = make_key<WIDE>(gather_key<WIDE>(kcol, kwl, (uint64_t)(row - id_base)), kxor, row);
            } else {
                key = in[i];
            }
        }
        w.push(valid, key, lane);
    }
    w.store(out + gw * k, lane);
}

// Full sort, between the two stable passes: the sort key of every row of the row-sorted list, as u64 (narrow images
// zero-extended).  rows[i] table-wide, kcol as topk_select_kernel's.
template <bool WIDE>
__global__ __launch_bounds__(kBlock) void topk_sort_keys_kernel(const uint32_t *__restrict__ rows, uint64_t n, const void *kcol, uint32_t kwl,
                                                                uint64_t kxor, uint32_t id_base, uint64_t *__restrict__ keys) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t raw = gather_key<WIDE>(kcol, kwl, (uint64_t)(rows[i] - id_base));
        keys[i] = WIDE ? raw ^ kxor : (uint64_t)(((uint32_t)raw) ^ (uint32_t)kxor);
    }
}

}  // namespace

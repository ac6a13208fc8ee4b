// emurx_wave.h — wave64 and workgroup primitives of the device passes (gfx950): the launch
// constants, loads through the global address space, DPP reductions, prefix scans over a wave
// and over a workgroup, and the wave-scope LDS hand-off.  Nothing here knows about frames:
// emurx_parse.h (the parser) includes it, and the passes that only scan, count or copy
// (respond, learn, tx framing, route) take their cross-lane code from here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <tuple>

namespace emurx {

constexpr int kWave = 64;
constexpr int kBlock = 256;
constexpr int kWaves = kBlock / kWave;

// loads through the global address space (global_load_*): pointers rebuilt from integers or
// kept in a struct would otherwise compile to flat loads, which also count on lgkmcnt and
// make the compiler serialise them with LDS traffic
typedef unsigned emurx_v4u __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint4 gld16(const void* p) {
    const emurx_v4u v = *(const __attribute__((address_space(1))) emurx_v4u*)p;
    return make_uint4(v.x, v.y, v.z, v.w);
}
typedef unsigned emurx_v3u __attribute__((ext_vector_type(3)));
__device__ __forceinline__ uint3 gld12(const void* p) {  // 4-byte aligned
    const emurx_v3u v = *(const __attribute__((address_space(1))) emurx_v3u*)p;
    return make_uint3(v.x, v.y, v.z);
}
__device__ __forceinline__ uint32_t gld4(const void* p) { return *(const __attribute__((address_space(1))) uint32_t*)p; }
__device__ __forceinline__ uint32_t gld1(const void* p) { return *(const __attribute__((address_space(1))) uint8_t*)p; }

__device__ __forceinline__ void wait_vm0() { __builtin_amdgcn_s_waitcnt(0x0F70); }  // vmcnt(0)

// Wave-scope LDS hand-off: what this wave's lanes wrote to LDS (or its LDS-DMA landed, after
// wait_vm0) before the call, any of its lanes may read after it.  No workgroup barrier: the
// words belong to the wave.
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ uint32_t lane_id() { return __lane_id(); }
// lanes below this one in mask m
__device__ __forceinline__ uint32_t mbcnt(uint64_t m) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// a lane's rank among the `in` lanes that hold its id (the lanes below it), and every present
// id's lane count into cnt[id], written by that id's first lane: one iteration of scalar
// bookkeeping per distinct id present.  A lane that is not `in` carries an id that no `in` lane
// has (the callers pass 0xff) and gets rank 0.  Called converged.
__device__ __forceinline__ uint32_t wave_rank_by_id(uint32_t id, bool in, uint32_t lane, uint32_t* cnt) {
    uint32_t rank = 0;
    uint64_t left = __ballot(in);
    while (left) {
        const uint32_t lead = (uint32_t)__ffsll((long long)left) - 1;
        const uint32_t g = (uint32_t)__builtin_amdgcn_readlane((int)id, (int)lead);
        const uint64_t m = __ballot(id == g);
        if (id == g) rank = mbcnt(m);
        if (lane == lead) cnt[g] = (uint32_t)__popcll(m);
        left &= ~m;
    }
    return rank;
}

// wave64 reductions on the DPP network (quad perms, row rotates, row broadcasts; result is
// read from lane 63 into a scalar register): no LDS traffic, 6 VALU + 1 readlane
template <int kCtrl, int kRowMask = 0xf>
__device__ __forceinline__ uint32_t dpp(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, kCtrl, kRowMask, 0xf, false);
}
template <class Op>
__device__ __forceinline__ uint32_t wave_reduce(uint32_t v, Op op) {
    v = op(v, dpp<0xb1>(v));        // quad_perm [1,0,3,2]
    v = op(v, dpp<0x4e>(v));        // quad_perm [2,3,0,1]
    v = op(v, dpp<0x124>(v));       // row_ror:4
    v = op(v, dpp<0x128>(v));       // row_ror:8
    v = op(v, dpp<0x142, 0xa>(v));  // row_bcast:15
    v = op(v, dpp<0x143, 0xc>(v));  // row_bcast:31
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
    return wave_reduce(v, [](uint32_t x, uint32_t y) { return min(x, y); });
}
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
    return wave_reduce(v, [](uint32_t x, uint32_t y) { return max(x, y); });
}
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
    return wave_reduce(v, [](uint32_t x, uint32_t y) { return x + y; });
}
// lane l - 1's value (0 in lane 0): one DPP move across the whole wave (wave_shr:1); called
// with every lane active
__device__ __forceinline__ uint32_t wave_prev(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x138, 0xf, 0xf, true);
}
__device__ __forceinline__ uint32_t dpp_row_sum(uint32_t v) {
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true);  // row_shr:1
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, true);  // row_shr:2
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, true);  // row_shr:4
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, true);  // row_shr:8
    return v;  // lane 15 of each row: the row's total
}

// ---------------------------------------------------------------------------------------
// prefix scans.  The scanned values are uint32_t or unsigned long long, any mix of them.
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t scan_up(uint32_t v, uint32_t d) { return (uint32_t)__shfl_up((int)v, d); }
__device__ __forceinline__ unsigned long long scan_up(unsigned long long v, uint32_t d) { return __shfl_up(v, d); }
// Inclusive wave64 prefix sums of one or more per-lane values, in place; called converged.
// One loop for all of them: a step's shuffles are issued together, then its adds.
template <typename... T>
__device__ __forceinline__ void wave_incl_scan(T&... v) {
    const uint32_t lane = lane_id();
#pragma unroll
    for (uint32_t d = 1; d < kWave; d <<= 1)
        [&](auto... u) { ((v += lane >= d ? u : 0), ...); }(scan_up(v, d)...);
}
// lane 63's value (after wave_incl_scan: the wave's total), in a scalar register
__device__ __forceinline__ uint32_t wave_last(uint32_t v) { return (uint32_t)__builtin_amdgcn_readlane((int)v, kWave - 1); }

// One wave's totals in LDS, a field per scanned value.
template <typename T, typename... U>
struct ScanTotals {
    T v;
    ScanTotals<U...> rest;
    __device__ __forceinline__ void put(T x, U... y) { v = x; rest.put(y...); }
    __device__ __forceinline__ void add_to(bool on, T& x, U&... y) const { x += on ? v : 0; rest.add_to(on, y...); }
};
template <typename T>
struct ScanTotals<T> {
    T v;
    __device__ __forceinline__ void put(T x) { v = x; }
    __device__ __forceinline__ void add_to(bool on, T& x) const { x += on ? v : 0; }
};
// what block_incl_scan needs in LDS; the caller declares it __shared__
template <uint32_t kLanes, typename... T>
struct BlockScanLds {
    ScanTotals<T...> wave[kLanes / kWave];
};
// Inclusive prefix sums over a workgroup of kLanes lanes (lane order: threadIdx.x), in place;
// returns the workgroup's totals, the same in every lane.  Called by the whole workgroup,
// converged.  It may be called again with the same lds, as in a loop with a workgroup-uniform
// trip count: the first barrier keeps this call's LDS writes behind the previous call's reads.
// A kernel that makes one call only says kAgain = false and saves that barrier.
template <uint32_t kLanes, bool kAgain = true, typename... T>
__device__ __forceinline__ std::tuple<T...> block_incl_scan(BlockScanLds<kLanes, T...>& lds, T&... v) {
    const uint32_t wv = threadIdx.x / kWave;
    wave_incl_scan(v...);
    if (kAgain) __syncthreads();
    if (lane_id() == kWave - 1) lds.wave[wv].put(v...);
    __syncthreads();
    std::tuple<T...> total{};
#pragma unroll 4  // four LDS reads in flight; all 16 at once cost a scan kernel 40 registers
    for (uint32_t w = 0; w < kLanes / kWave; ++w) {
        const ScanTotals<T...> s = lds.wave[w];
        s.add_to(w < wv, v...);  // selects, not branches: the unrolled reads stay in flight together
        std::apply([&](T&... t) { s.add_to(true, t...); }, total);
    }
    return total;
}

}  // namespace emurx

// emurx_txplan.hip — the tx planner and the egress slots' output pass (gfx950).
//
// k_tx_plan: the emurx_tx_desc of every frame of a batch, derived from the frame's own headers
// (include/emu_rx.h emurx_tx_plan_dev), so that a caller that only holds finished frames can use
// emurx_tx_checksum_dev.  The walk is the rx parser's without its checksum tests; p: the frame,
// len: its length, be16: a big-endian byte pair.
//   L2    len < 14 -> BAD.  EtherType at 12; each 0x8100 / 0x88a8 tag advances 4 bytes and needs
//         the next EtherType inside len (else BAD); a third tag -> BAD.            parser.go:700-741
//   IPv4  BAD unless len >= l3 + 20, version 4, IHL * 4 >= 20, len >= l3 + IHL * 4 and totlen >=
//         IHL * 4; then ops = EMURX_TX_IPV4_HDR, l4 = l3 + IHL * 4.                parser.go:771-862
//         l3 + totlen != len -> LENGTH (the header op alone: the L4 span of the checksum call is
//         p[l4:len], as the Go callers slice it, tcp_output.go:64-70, udp.go:143-150).
//         be16(p + l3 + 6) & 0x3fff, or a protocol that is none of 6 / 17 / 1 -> HDR (IGMP with
//         its 24-byte header, igmp.go:1179-1186).  Else TCP4 / UDP4 / ICMP4, outcome L4; BAD when
//         len < l4 + 20 / 8 / 4.
//   IPv6  BAD unless len >= l3 + 40 and version 6; l3 + 40 + plen != len -> LENGTH, ops 0.
//         Extension headers {0, 43, 50, 51, 60, 135, 139, 140} of (p[o + 1] << 3) + 8 bytes; fewer
//         than 8 bytes left or a header ending past len -> BAD.                    parser.go:864-952
//         Final next header 6 / 17 / 58 -> TCP6 / UDP6 / ICMP6, outcome L4, osize = l4 - l3 - 40,
//         with osize > 0 EMURX_TX_V6_NH and nh (ipv6/mld.go:1271); any other -> NONE.
//   else  NONE.
//   EMURX_TXP_UDP0_KEEP: a UDP checksum field 00 00 stays (IPv4 -> HDR, IPv6 -> NONE).
// One frame per lane, as k_tx_csum: the descriptor load first, then the frame's first 96 bytes
// into the lane's LDS window by LDS-DMA (the rx window path's WinSrc; only the vectors the frame
// has), and the walk reads its header bytes there.  A long IPv6 extension chain reads on from
// global memory (WinSrc::u8 past the window).  No tables.  The outcome counts are wave ballots
// summed in scalar registers over the workgroup's tiles, then one add per outcome and workgroup.
//
// k_egr_out: what an egress slot's chain produced, into the slot's pinned result block (as
// k_ans_out does for a slot's answers).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/emu_rx.h"
#include "emurx_kernels.h"
#include "emurx_parse.h"

namespace emurx {

constexpr uint32_t kTxpWinVec = 6;                       // 16-byte vectors per lane: 96 bytes
constexpr uint32_t kTxpSlab = kTxpWinVec * 16 * kWave;   // 6 KiB per wave
constexpr uint32_t kTxpMaxGrid = 2048;                   // workgroups; the tiles beyond are taken in turns

typedef unsigned emurx_v2u __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint2 gld8(const void* p) {  // 8-byte aligned, through the global address space
    const emurx_v2u v = *(const __attribute__((address_space(1))) emurx_v2u*)p;
    return make_uint2(v.x, v.y);
}

struct TxPlan {
    uint32_t l3, l4, osize, ops, nh, oc;
};

__device__ __forceinline__ bool txp_is_ext(uint32_t nh) {
    constexpr uint64_t kLow = 1ull << 0 | 1ull << 43 | 1ull << 50 | 1ull << 51 | 1ull << 60;
    return nh < 64 ? (kLow >> nh) & 1 : nh == 135 || nh == 139 || nh == 140;
}

// the rule above for one frame; every byte it reads lies below len
template <class S>
__device__ __forceinline__ TxPlan tx_plan(const S& s, uint32_t len, bool keep) {
    const TxPlan bad{0, 0, 0, 0, 0, EMURX_TXP_BAD}, none{0, 0, 0, 0, 0, EMURX_TXP_NONE};
    if (len < 14) return bad;
    uint32_t et = be16(s, 12), l3 = 14;
    for (uint32_t tags = 0; et == 0x8100 || et == 0x88a8; ++tags) {
        if (tags == 2 || len < l3 + 4) return bad;
        et = be16(s, l3 + 2);
        l3 += 4;
    }
    if (et == 0x0800) {
        if (len < l3 + 20) return bad;
        const uint32_t vi = s.u8(l3), ihl = (vi & 0xf) << 2, tot = be16(s, l3 + 2);
        if ((vi >> 4) != 4 || ihl < 20 || len < l3 + ihl || tot < ihl) return bad;
        const uint32_t l4 = l3 + ihl;
        if (l3 + tot != len) return TxPlan{l3, l4, 0, EMURX_TX_IPV4_HDR, 0, EMURX_TXP_LENGTH};
        const TxPlan hdr{l3, l4, 0, EMURX_TX_IPV4_HDR, 0, EMURX_TXP_HDR};
        const uint32_t proto = s.u8(l3 + 9);
        const bool tcp = proto == 6, udp = proto == 17;
        if ((be16(s, l3 + 6) & 0x3fff) || !(tcp || udp || proto == 1)) return hdr;
        if (len < l4 + (tcp ? 20u : udp ? 8u : 4u)) return bad;
        if (udp && keep && be16(s, l4 + 6) == 0) return hdr;
        const uint32_t kind = tcp ? EMURX_TX_L4_TCP4 : udp ? EMURX_TX_L4_UDP4 : EMURX_TX_L4_ICMP4;
        return TxPlan{l3, l4, 0, EMURX_TX_IPV4_HDR | (kind << EMURX_TX_L4_SHIFT), 0, EMURX_TXP_L4};
    }
    if (et == 0x86dd) {
        if (len < l3 + 40 || (s.u8(l3) >> 4) != 6) return bad;
        if (l3 + 40 + be16(s, l3 + 4) != len) return TxPlan{0, 0, 0, 0, 0, EMURX_TXP_LENGTH};
        uint32_t nh = s.u8(l3 + 6), o = l3 + 40;
        while (txp_is_ext(nh)) {  // each round advances at least 8 bytes towards len
            if (len < o + 8) return bad;
            const uint32_t hl = (s.u8(o + 1) << 3) + 8;
            if (len < o + hl) return bad;
            nh = s.u8(o);
            o += hl;
        }
        const bool tcp = nh == 6, udp = nh == 17;
        if (!(tcp || udp || nh == 58)) return none;
        if (len < o + (tcp ? 20u : udp ? 8u : 4u)) return bad;
        if (udp && keep && be16(s, o + 6) == 0) return none;
        const uint32_t kind = tcp ? EMURX_TX_L4_TCP6 : udp ? EMURX_TX_L4_UDP6 : EMURX_TX_L4_ICMP6;
        const uint32_t osize = o - l3 - 40;
        return TxPlan{l3, o, osize, (kind << EMURX_TX_L4_SHIFT) | (osize ? EMURX_TX_V6_NH : 0u), osize ? nh : 0u,
                      EMURX_TXP_L4};
    }
    return none;
}

__global__ __launch_bounds__(kBlock) void k_tx_plan(const uint8_t* __restrict__ frames,
                                                    const emurx_desc* __restrict__ desc, uint32_t n, uint32_t flags,
                                                    emurx_tx_desc* __restrict__ txd, uint8_t* __restrict__ outcome,
                                                    unsigned long long* __restrict__ info) {
    __shared__ __attribute__((aligned(16))) uint32_t s_slab[kWaves][kTxpSlab / 4];
    __shared__ uint32_t s_cnt[kWaves][8];
    const uint32_t lane = lane_id(), wv = threadIdx.x / kWave;
    const uint32_t nt = (n + kBlock - 1) / kBlock;
    const bool keep = flags & EMURX_TXP_UDP0_KEEP;
    uint32_t cnt[5] = {0, 0, 0, 0, 0};  // wave-uniform: this wave's frames per outcome
    for (uint32_t t = blockIdx.x; t < nt; t += gridDim.x) {  // workgroup-uniform
        const uint32_t i = t * kBlock + threadIdx.x;
        const bool live = i < n;
        const uint2 d = live ? gld8(desc + i) : make_uint2(0, 0);  // {off} {len | vport << 16 | pad << 24}
        const uint32_t len = d.y & 0xffff;
        // the lane's window: vector k of lane l at slab byte k * 1 KiB + l * 16 (one DMA row per
        // k); only the aligned 16-byte blocks that hold frame bytes are read
        const uintptr_t fa = (uintptr_t)(frames + d.x);
        const uint4* src = reinterpret_cast<const uint4*>(fa & ~(uintptr_t)15);
        const uint32_t head = (uint32_t)(fa & 15), nv = live && len ? (head + len + 15) >> 4 : 0u;
        uint4* dst = reinterpret_cast<uint4*>(s_slab[wv]);
#pragma unroll
        for (uint32_t k = 0; k < kTxpWinVec; ++k)
            if (k < nv)
                __builtin_amdgcn_global_load_lds(src + k, (__attribute__((address_space(3))) void*)(dst + k * kWave), 16, 0,
                                                 0);
        wait_vm0();  // vmcnt(0): the windows landed
        wave_lds_sync();
        const WinSrc w{reinterpret_cast<const uint8_t*>(s_slab[wv]), s_slab[wv], lane * 16, head,
                       min(kTxpWinVec * 16 - head, len), frames + d.x};
        TxPlan p{0, 0, 0, 0, 0, EMURX_TXP_BAD};
        if (live) p = tx_plan(w, len, keep);
        if (live) {
            reinterpret_cast<uint4*>(txd)[i] =
                make_uint4(d.x, len | (p.l3 << 16), p.l4 | (p.osize << 16), p.ops | (p.nh << 8));
            if (outcome) outcome[i] = (uint8_t)p.oc;
        }
#pragma unroll
        for (uint32_t k = 0; k < 5; ++k) cnt[k] += (uint32_t)__popcll(__ballot(live && p.oc == k));
        wave_lds_sync();  // the next round's DMA rows land behind this round's reads
    }
    if (lane == 0) {
#pragma unroll
        for (uint32_t k = 0; k < 5; ++k) s_cnt[wv][k] = cnt[k];
    }
    __syncthreads();
    if (threadIdx.x < 5) {
        const uint32_t c = s_cnt[0][threadIdx.x] + s_cnt[1][threadIdx.x] + s_cnt[2][threadIdx.x] + s_cnt[3][threadIdx.x];
        if (c) atomicAdd(info + threadIdx.x, (unsigned long long)c);
    }
}

// ---- an egress slot's results to the host ---------------------------------------------------
// One launch behind the slot's chain (plan, checksum, framing).  The framing's counts are known
// only on the device; every workgroup reads them and the grid copies, with 16-byte stores over
// the bus into the slot's pinned result block, exactly what was produced: the head (the planner's
// info words, then the framing's {n_msgs, bytes}), msg_off[n_msgs + 1], the two per-frame byte
// arrays and the messages.  The counts are clamped to the regions' capacities (the host checks
// the head against the same capacities).  Regions start on 256-byte boundaries on both sides
// and their capacities are whole 16-byte vectors.
__global__ __launch_bounds__(kBlock) void k_egr_out(const emurx_egr_out a) {
    const uint64_t nmsg = min((uint64_t)a.tx_info[0], (uint64_t)a.n);
    const uint64_t txb = min((uint64_t)a.tx_info[1], a.tx_cap);
    const uint64_t gid = (uint64_t)blockIdx.x * kBlock + threadIdx.x, gsz = (uint64_t)gridDim.x * kBlock;
    auto copy = [&](const void* src, void* dst, uint64_t bytes) {
        const uint64_t nv = (bytes + 15) >> 4;
        for (uint64_t v = gid; v < nv; v += gsz)
            reinterpret_cast<uint4*>(dst)[v] = gld16(reinterpret_cast<const uint4*>(src) + v);
    };
    if (blockIdx.x == 0 && threadIdx.x < EMURX_EGR_HEAD_WORDS / 2) {  // the head: two words per lane
        auto word = [&](uint32_t i) -> unsigned long long {
            return i < EMURX_TXP_INFO_WORDS ? a.plan_info[i] : i < EMURX_TXP_INFO_WORDS + 2 ? a.tx_info[i - EMURX_TXP_INFO_WORDS] : 0ull;
        };
        const unsigned long long w0 = word(2 * threadIdx.x), w1 = word(2 * threadIdx.x + 1);
        reinterpret_cast<uint4*>(a.h_head)[threadIdx.x] =
            make_uint4((uint32_t)w0, (uint32_t)(w0 >> 32), (uint32_t)w1, (uint32_t)(w1 >> 32));
    }
    copy(a.msg_off, a.h_msg_off, (nmsg + 1) * 8);
    copy(a.plan, a.h_plan, a.n);
    copy(a.status, a.h_status, a.n);
    copy(a.tx, a.h_tx, txb);
}

}  // namespace emurx

int emurx_launch_tx_plan(const uint8_t* frames, const emurx_desc* desc, uint32_t n, uint32_t flags, emurx_tx_desc* txd,
                         uint8_t* outcome, uint64_t* info, hipStream_t st) {
    using namespace emurx;
    if (!EMURX_HIP_OK(hipMemsetAsync(info, 0, EMURX_TXP_INFO_WORDS * sizeof(uint64_t), st))) return -1;
    if (!n) return 0;
    const uint32_t g = std::min<uint32_t>((n + kBlock - 1) / kBlock, kTxpMaxGrid);
    return EMURX_HIP_OK(emurx_launch(k_tx_plan, dim3(g), dim3(kBlock), 0, st, frames, desc, n, flags, txd, outcome,
                                     reinterpret_cast<unsigned long long*>(info)))
               ? 0
               : -1;
}

int emurx_launch_egr_out(const emurx_egr_out& a, hipStream_t st) {
    using namespace emurx;
    // a workgroup per 4 KiB of what the batch can at most produce, at most 256: a workgroup
    // with nothing to copy ends after reading the two counts
    const uint64_t vol = a.tx_cap + 10ull * a.n;
    const uint32_t g = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(vol / 4096, 1), 256);
    return EMURX_HIP_OK(emurx_launch(k_egr_out, dim3(g), dim3(kBlock), 0, st, a)) ? 0 : -1;
}

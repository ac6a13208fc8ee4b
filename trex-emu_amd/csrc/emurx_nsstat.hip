// emurx_nsstat.hip — the per-Namespace counters of the ARP, ICMPv4 and ICMPv6 / ND handlers of a
// classified batch, folded on the device (gfx950) into one event per Namespace, and per frame
// whether its Go handler still has to run.  The rule with its Go lines is in include/emu_rx.h
// (HandleRxArpPacket plugins/arp/arp.go:904-946, HandleRxIcmpPacket plugins/icmp/icmp.go:396-462,
// HandleRxIpv6Packet plugins/ipv6/ipv6.go:465-539, the ND handler plugins/ipv6/nd.go:1546-1776);
// the type and code constants are gopacket's (layers/icmp4.go:20-43: echo reply 0, destination
// unreachable 3 with codes Net 0 .. FragmentationNeeded 4, echo request 8, timestamp request 13;
// layers/icmp6.go:21-52: destination unreachable 1 with codes 0..6, echo request 128, echo reply
// 129, MLD 130..132 and 143, router solicitation 133 .. redirect 137).
// emurx_nsstat_dev / emurx_nsstat_ts_dev (the timestamp reply's two outcomes), three launches:
//   k_nss_decide   one frame per lane: the record's second half says whether the frame is a
//                  candidate; only a candidate's descriptor, its two outcome bytes, its ns_id and
//                  the type / code / operation / destination-MAC / source bytes the rule names are
//                  read.  A frame with done 1 bumps one or two counters of its Namespace.  They are
//                  combined in a set in LDS keyed by (ns_id, counter): a wave whose done-1 frames
//                  all bump the same counters of one Namespace (a ping burst) adds its popcount from
//                  one lane, any other wave one LDS atomic per lane and counter.  Then one global
//                  atomic add per occupied slot: per distinct (ns_id, counter) of the workgroup, into
//                  the handle's dense accumulator rows [max_ns][24] = {cnt[22], 0, 0}.  The add
//                  that finds a row's "first" counter zero (every done-1 frame bumps exactly one of
//                  those: kNssFirst) sets the row's flag, a word of its own in a dense array beside
//                  the rows (a flag inside the 96-byte rows would cost the scan a cache line a row).
//   k_nss_scan     one workgroup: the tiles' done counts; an exclusive scan of the max_ns row
//                  flags (8 per lane as two 16-byte loads, 8,192 per round), which replaces each
//                  set flag by its row's ordinal + 1; distinct Namespaces against ev_cap; d_info.
//                  Without a done-1 frame in the batch no row was touched: the scan skips the flags.
//   k_nss_emit     one lane per Namespace: a row with an ordinal goes out as the event there
//                  (ascending ns_id), frames = the sum of its first counters, unless the batch
//                  overflows; either way the lane zeroes the row and its flag, so that rows and
//                  flags are all zero again when the call ends and no call pays for a memset.
// A batch without candidates costs the read of the records' second halves and one done byte per
// frame, and two launches that find nothing to do.
#include <hip/hip_runtime.h>

#include "../../include/emu_rx.h"
#include "emurx_kernels.h"
#include "emurx_parse.h"
#include "emurx_rsp_dev.h"

namespace emurx {

constexpr uint32_t kNssTile = EMURX_QUEUE_TILE;  // frames per workgroup, one per lane
static_assert(kNssTile == kBlock, "one frame per lane of a 256-lane workgroup");
constexpr uint32_t kNssRow = EMURX_NSC_WORDS + 2;  // an accumulator row: cnt[22] and two zero words (16-byte aligned rows)
static_assert(kNssRow * 4 == sizeof(emurx_nsstat_ev) && kNssRow <= 32, "a row is as large as an event; 5 bits of counter index");
constexpr uint32_t kNssSlots = 4 * kBlock;  // the workgroup's set: at most two keys per lane, so never more than half full
constexpr uint32_t kNssScanBlock = 1024, kNssScanPer = 8;  // flags per lane and round of the scan: 8,192 rows a round
constexpr uint32_t kNssMaxNs = 1u << 27;  // ns_id * 32 + counter + 1 is a 32-bit key
// the counter every done-1 frame bumps exactly one of: their sum is the event's `frames`
constexpr uint32_t kNssFirst = 1u << EMURX_NSC_ARP_QUERY | 1u << EMURX_NSC_ARP_REPLY | 1u << EMURX_NSC_ARP_ERR_NO_BROADCAST |
                               1u << EMURX_NSC_ARP_ERR_WRONG_OP | 1u << EMURX_NSC_ICMP_ECHO | 1u << EMURX_NSC_ICMP_NO_CLIENT |
                               1u << EMURX_NSC_ICMP_ERR_MCAST | 1u << EMURX_NSC_ICMP_ERR_UNHANDLED | 1u << EMURX_NSC_V6_ECHO |
                               1u << EMURX_NSC_V6_NO_CLIENT | 1u << EMURX_NSC_V6_ERR_MCAST | 1u << EMURX_NSC_V6_ERR_UNHANDLED |
                               1u << EMURX_NSC_ND_RX_NS | 1u << EMURX_NSC_ND_RX_NA | 1u << EMURX_NSC_ICMP_ERR_TOO_SHORT;

struct NssPlan {
    uint32_t done, cnt;  // cnt: the counters the frame bumps, a bit each (one of kNssFirst, at most one other)
};
__device__ __forceinline__ NssPlan nss_plan(uint32_t done, uint32_t cnt = 0) { return {done, cnt}; }
__device__ __forceinline__ NssPlan nss_count(uint32_t a) { return {1u, 1u << a}; }
__device__ __forceinline__ NssPlan nss_count(uint32_t a, uint32_t b) { return {1u, 1u << a | 1u << b}; }

// The record's words: as in emurx_respond.hip
__device__ __forceinline__ uint32_t nss_lk(const uint4& b) { return (b.w >> (8 + EMURX_FLAG_LK_SHIFT)) & 7u; }
__device__ __forceinline__ bool nss_candidate(const uint4& b, uint32_t kinds) {
    const uint32_t proto = b.z >> 24, status = b.w & 0xff;
    if (status != EMURX_ST_OK) return false;
    if (proto == EMURX_CB_ARP) return kinds & EMURX_RSPK_ARP;
    if (proto == EMURX_CB_ICMP) return kinds & EMURX_RSPK_ICMP;  // the timestamp kind comes with ICMP only
    return proto == EMURX_CB_ICMPV6 && (kinds & (EMURX_RSPK_ICMPV6 | EMURX_RSPK_ND));
}

// The decision for a candidate frame; ro, lo: its responder and learn outcomes
__device__ NssPlan nss_decide(const uint8_t* __restrict__ frames, const emurx_desc& d, const uint4& b, uint32_t kinds,
                              uint32_t ro, uint32_t lo) {
    const uint32_t proto = b.z >> 24, lk = nss_lk(b), l3 = b.x >> 16, l4 = b.y & 0xffffu, len = d.len;
    const uint8_t* f = frames + d.off;
    if (d.pad == EMURX_DESC_HOLE) return nss_plan(0);
    if (lk == EMURX_LK_NO_NS || lk == EMURX_LK_NS_NO_PLUGIN) return nss_plan(2);  // the handler returns PARSER_ERR
    if (lk < EMURX_LK_NS_LEVEL) return nss_plan(0);
    if (proto == EMURX_CB_ARP) {  // arp.go:904-946
        if (l3 < 14 || l3 + 28 > len || lo == EMURX_LRN_HOST) return nss_plan(0);
        const uint32_t op = gld1(f + l3 + 6) << 8 | gld1(f + l3 + 7);
        if (op == 1) {
            if (lk == EMURX_LK_NO_CLIENT) return nss_count(EMURX_NSC_ARP_QUERY, EMURX_NSC_ARP_QUERY_NOT_FOR_US);
            if (lk == EMURX_LK_CLIENT_NO_PLUGIN) return nss_count(EMURX_NSC_ARP_QUERY);
            if (lk == EMURX_LK_CLIENT && ro == EMURX_RSP_ARP) return nss_count(EMURX_NSC_ARP_QUERY, EMURX_NSC_ARP_TX_REPLY);
            return nss_plan(0);  // the handler answers, and counts everything itself
        }
        if (op == 2) {
            const bool bcast = rsp_le32(f) == 0xffffffffu && (gld1(f + 4) & gld1(f + 5)) == 0xffu;
            return nss_count(bcast ? EMURX_NSC_ARP_ERR_NO_BROADCAST : EMURX_NSC_ARP_REPLY);
        }
        return nss_count(EMURX_NSC_ARP_ERR_WRONG_OP);
    }
    if (proto == EMURX_CB_ICMP) {  // icmp.go:396-462
        if (l3 < 14 || l3 + 20 > len || l4 + 8 > len) return nss_plan(0);
        if (lk == EMURX_LK_NO_CLIENT) return nss_count(EMURX_NSC_ICMP_NO_CLIENT);
        if (lk != EMURX_LK_CLIENT) return nss_plan(0);
        if (ro == EMURX_RSP_DROP_MCAST) return nss_count(EMURX_NSC_ICMP_ERR_MCAST);
        if (ro == EMURX_RSP_ICMP) return nss_count(EMURX_NSC_ICMP_ECHO);
        if (kinds & EMURX_RSPK_TS) {  // HandleEcho(ps, true): icmp.go:322-323, :313
            if (ro == EMURX_RSP_TS) return nss_count(EMURX_NSC_ICMP_ECHO);
            if (ro == EMURX_RSP_DROP_SHORT) return nss_count(EMURX_NSC_ICMP_ERR_TOO_SHORT);
        }
        const uint32_t type = gld1(f + l4), code = gld1(f + l4 + 1);
        // echo request, timestamp request, echo reply, destination unreachable: the handler's
        if ((code == 0 && (type == 8 || type == 13 || type == 0)) || (type == 3 && code <= 4)) return nss_plan(0);
        return nss_count(EMURX_NSC_ICMP_ERR_UNHANDLED);
    }
    // icmpv6: ipv6.go:465-539
    if (l3 < 14 || l3 + 40 > l4 || l4 + 4 > len) return nss_plan(0);
    const uint32_t type = gld1(f + l4), code = gld1(f + l4 + 1);
    if (type == 128 && code == 0) {
        if (!(kinds & EMURX_RSPK_ICMPV6)) return nss_plan(0);
        if (lk == EMURX_LK_NO_CLIENT)  // a multicast source (:499) hides in NO_CLIENT
            return gld1(f + l3 + 8) == 0xffu ? nss_plan(0) : nss_count(EMURX_NSC_V6_NO_CLIENT);
        if (lk != EMURX_LK_CLIENT) return nss_plan(0);
        if (ro == EMURX_RSP_ICMPV6) return nss_count(EMURX_NSC_V6_ECHO);
        if (ro == EMURX_RSP_DROP_MCAST) return nss_count(EMURX_NSC_V6_ERR_MCAST);
        return nss_plan(0);
    }
    if (lk != EMURX_LK_NS_LEVEL) return nss_plan(0);
    if (code == 0 && (type == 135 || type == 136)) {
        if (!(kinds & EMURX_RSPK_ND)) return nss_plan(0);
        if (type == 136)  // nd.go:1687-1776
            return lo == EMURX_LRN_ND_NA ? nss_count(EMURX_NSC_ND_RX_NA, EMURX_NSC_ND_RX_NA_LEARN) : nss_plan(0);
        if (ro != EMURX_RSP_ND || !(lo == EMURX_LRN_NONE || lo == EMURX_LRN_ND_NS)) return nss_plan(0);
        uint32_t src[4];
        rsp_load16((uintptr_t)f, len, (int)(l3 + 8), src);  // NdClientCtx.Respond nd.go:1239-1247
        return nss_count(EMURX_NSC_ND_RX_NS, ip6_unspecified(src) ? EMURX_NSC_ND_TX_DAD_ERROR : EMURX_NSC_ND_TX_ADV_UNICAST);
    }
    // echo reply, MLD, router solicitation and advertisement, redirect, MLDv2 report; destination unreachable
    if (code == 0 && ((type >= 129 && type <= 134) || type == 137 || type == 143)) return nss_plan(0);
    if (type == 1 && code <= 6) return nss_plan(0);
    return (kinds & EMURX_RSPK_ICMPV6) ? nss_count(EMURX_NSC_V6_ERR_UNHANDLED) : nss_plan(0);
}

// v more of key (ns_id * 32 + counter + 1; 0 = a free slot) in the workgroup's set: linear probing;
// the set is never more than half full, so a free slot always ends the probe
__device__ __forceinline__ void nss_lds_add(uint32_t* s_key, uint32_t* s_val, uint32_t key, uint32_t v) {
    for (uint32_t q = (key * 0x9E3779B1u) >> 22, t = 0; t < kNssSlots; q = (q + 1) & (kNssSlots - 1), ++t) {
        uint32_t cur = __hip_atomic_load(&s_key[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (cur == 0) cur = atomicCAS(&s_key[q], 0u, key);
        if (cur == 0 || cur == key) {
            atomicAdd(&s_val[q], v);
            return;
        }
    }
}
static_assert(kNssSlots == 1u << 10, "the hash keeps 10 bits");

// tile sums: done 1 | done 2 << 10 | candidates left at done 0 << 20 (each <= 256)
__global__ __launch_bounds__(kBlock) void k_nss_decide(const uint8_t* __restrict__ frames, const emurx_desc* __restrict__ desc,
                                                       const emurx_rec* __restrict__ rec, uint32_t n, uint32_t kinds,
                                                       const uint8_t* __restrict__ rsp, const uint8_t* __restrict__ lrn,
                                                       uint32_t ns_lim, uint32_t* __restrict__ acc, uint32_t* __restrict__ flag,
                                                       uint32_t* __restrict__ tsum,
                                                       uint8_t* __restrict__ done) {
    __shared__ uint32_t s_sum;
    __shared__ uint32_t s_key[kNssSlots], s_val[kNssSlots];
    for (uint32_t j = threadIdx.x; j < kNssSlots; j += kBlock) s_key[j] = s_val[j] = 0;
    if (threadIdx.x == 0) s_sum = 0;
    __syncthreads();
    const uint32_t i = blockIdx.x * kNssTile + threadIdx.x, lane = lane_id();
    NssPlan p = nss_plan(0);
    uint32_t ns = 0;
    bool cand = false;
    if (i < n) {
        const uint4 b = gld16(reinterpret_cast<const uint4*>(rec + i) + 1);
        if (nss_candidate(b, kinds)) {
            const emurx_desc d = desc[i];
            const uint32_t proto = b.z >> 24;  // the learn outcome decides for arp, and for icmpv6 with the ND kind
            const bool needs_lrn = proto == EMURX_CB_ARP || (proto == EMURX_CB_ICMPV6 && (kinds & EMURX_RSPK_ND));
            p = nss_decide(frames, d, b, kinds, gld1(rsp + i), needs_lrn ? gld1(lrn + i) : 0u);
            cand = d.pad != EMURX_DESC_HOLE;
            if (p.done == 1) {
                ns = gld4(rec + i);  // ns_id: the record's first word
                if (ns >= ns_lim) p = nss_plan(0);  // no row for it
            }
        }
        if (done) done[i] = (uint8_t)p.done;
    }
    const bool on = p.done == 1;
    const uint32_t c = wave_sum_u32((on ? 1u : 0u) | (p.done == 2 ? 1u << 10 : 0u) | (cand && p.done == 0 ? 1u << 20 : 0u));
    if (lane == 0 && c) atomicAdd(&s_sum, c);
    const unsigned long long m = __ballot(on);
    if (m) {  // wave-uniform
        const uint32_t L = (uint32_t)__ffsll((long long)m) - 1u;
        const uint32_t ns0 = (uint32_t)__builtin_amdgcn_readlane((int)ns, (int)L);
        const uint32_t c0 = (uint32_t)__builtin_amdgcn_readlane((int)p.cnt, (int)L);
        const bool same = __ballot(on && (ns != ns0 || p.cnt != c0)) == 0;  // one Namespace, the same counters
        if (same ? lane == L : on) {
            const uint32_t v = same ? (uint32_t)__popcll(m) : 1u;
            for (uint32_t bits = p.cnt; bits; bits &= bits - 1) nss_lds_add(s_key, s_val, ns * 32u + (uint32_t)__ffs((int)bits), v);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) tsum[blockIdx.x] = s_sum;
    if (!(s_sum & 0x3ffu)) return;  // workgroup-uniform: no frame with done 1, an empty set
    for (uint32_t j = threadIdx.x; j < kNssSlots; j += kBlock) {
        const uint32_t key = s_key[j];
        if (!key) continue;
        const uint32_t w = (key - 1) & 31u;
        const uint32_t ns = (key - 1) >> 5;
        const uint32_t old = __hip_atomic_fetch_add(acc + (size_t)ns * kNssRow + w, s_val[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        // the row's first frames of this batch: the scan looks at the flags alone
        if (old == 0 && ((kNssFirst >> w) & 1u)) __hip_atomic_store(flag + ns, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// info: {events written, distinct Namespaces, overflow, frames done 1, done 2, candidates left at 0, 0, 0};
// flag[ns]: 1 for a row the batch touched, in; the row's ordinal + 1, out (0 for every other row).
// flag has nflag words, max_ns rounded up to a multiple of kNssScanPer: the words past max_ns stay 0
__global__ __launch_bounds__(kNssScanBlock) void k_nss_scan(uint32_t* __restrict__ flag, uint32_t nflag,
                                                            const uint32_t* __restrict__ tsum, uint32_t ntiles, uint32_t ev_cap,
                                                            unsigned long long* __restrict__ info) {
    __shared__ BlockScanLds<kNssScanBlock, uint32_t> s_scan;
    __shared__ uint32_t s_dc[3];
    if (threadIdx.x < 3) s_dc[threadIdx.x] = 0;
    uint32_t dc[3] = {0, 0, 0};
    for (uint32_t t = threadIdx.x; t < ntiles; t += kNssScanBlock) {
        const uint32_t v = tsum[t];
        dc[0] += v & 0x3ffu;
        dc[1] += (v >> 10) & 0x3ffu;
        dc[2] += v >> 20;
    }
    __syncthreads();  // s_dc is zero before anyone adds to it
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const uint32_t s = wave_sum_u32(dc[k]);
        if (lane_id() == 0 && s) atomicAdd(&s_dc[k], s);
    }
    __syncthreads();
    uint32_t base = 0;
    // a batch without a done-1 frame has added to no row: every flag is zero already
    const uint32_t rows = s_dc[0] ? nflag : 0u;
    for (uint32_t r0 = 0; r0 < rows; r0 += kNssScanBlock * kNssScanPer) {  // workgroup-uniform trip count
        const uint32_t r = r0 + threadIdx.x * kNssScanPer;
        uint4 a = make_uint4(0, 0, 0, 0), b = a;  // this lane's eight flags
        if (r < rows) {
            a = gld16(flag + r);
            b = gld16(flag + r + 4);
        }
        const uint32_t v[kNssScanPer] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        uint32_t cnt = 0;
#pragma unroll
        for (uint32_t j = 0; j < kNssScanPer; ++j) cnt += v[j] ? 1u : 0u;
        uint32_t c = cnt;
        const auto [total] = block_incl_scan<kNssScanBlock>(s_scan, c);
        uint32_t k = base + c - cnt;
#pragma unroll
        for (uint32_t j = 0; j < kNssScanPer; ++j)
            if (v[j]) flag[r + j] = ++k;  // the ordinal + 1
        base += total;
    }
    if (threadIdx.x < EMURX_NSS_INFO_WORDS) {
        const uint32_t k = threadIdx.x;
        const bool over = base > ev_cap;
        info[k] = k == 0 ? (over ? 0u : base) : k == 1 ? base : k == 2 ? (over ? 1u : 0u) : k < 6 ? s_dc[k - 3] : 0u;
    }
}

__global__ __launch_bounds__(kBlock) void k_nss_emit(uint32_t* __restrict__ acc, uint32_t* __restrict__ flag, uint32_t max_ns,
                                                     uint32_t ev_cap, const unsigned long long* __restrict__ info,
                                                     uint2* __restrict__ ev) {
    const uint32_t ns = blockIdx.x * kBlock + threadIdx.x;
    if (ns >= max_ns) return;
    const uint32_t k1 = gld4(flag + ns);
    if (k1 == 0) return;
    const uint32_t k = k1 - 1;
    flag[ns] = 0;
    uint4* row = reinterpret_cast<uint4*>(acc + (size_t)ns * kNssRow);  // 96-byte rows of a 256-byte aligned block
    uint32_t w[kNssRow];
#pragma unroll
    for (uint32_t j = 0; j < kNssRow / 4; ++j) {
        const uint4 v = gld16(row + j);
        w[4 * j] = v.x, w[4 * j + 1] = v.y, w[4 * j + 2] = v.z, w[4 * j + 3] = v.w;
        row[j] = make_uint4(0, 0, 0, 0);  // rows and flags are all zero again when the call ends
    }
    if (info[2] != 0 || k >= ev_cap) return;  // overflow: nothing is written
    uint32_t fr = 0;
#pragma unroll
    for (uint32_t j = 0; j < EMURX_NSC_WORDS; ++j) fr += (kNssFirst >> j) & 1u ? w[j] : 0u;
    uint2* e = ev + (size_t)k * (kNssRow / 2);  // emurx_nsstat_ev: ns_id, frames, cnt[22]
    e[0] = make_uint2(ns, fr);
#pragma unroll
    for (uint32_t j = 0; j < EMURX_NSC_WORDS / 2; ++j) e[1 + j] = make_uint2(w[2 * j], w[2 * j + 1]);
}

}  // namespace emurx

// scratch: the accumulator rows u32 [max_ns][24], then the rows' flags u32 [max_ns rounded up to 8]
// and the tile sums u32 [tiles of max_frames].  Rows and flags start, and every call leaves them,
// all zero (emurx_nss_scratch_bytes of zeros do for a start).
struct NssScratch {
    uint32_t *acc, *flag, *tsum;
    size_t bytes;
};
static uint32_t nss_flags(uint32_t max_ns) { return (max_ns + emurx::kNssScanPer - 1) / emurx::kNssScanPer * emurx::kNssScanPer; }
static NssScratch nss_scratch(void* base, uint32_t max_frames, uint32_t max_ns) {
    const size_t mt = ((size_t)max_frames + emurx::kNssTile - 1) / emurx::kNssTile;
    emurx_carver c(base);  // the initialisers run in order
    return {c.take<uint32_t>((size_t)max_ns * emurx::kNssRow), c.take<uint32_t>(nss_flags(max_ns)), c.take<uint32_t>(mt), c.bytes()};
}
size_t emurx_nss_scratch_bytes(uint32_t max_frames, uint32_t max_ns) { return nss_scratch(nullptr, max_frames, max_ns).bytes; }

int emurx_launch_nsstat(const uint8_t* frames, const emurx_desc* desc, const emurx_rec* rec, uint32_t n, uint32_t kinds,
                        const uint8_t* rsp_outcome, const uint8_t* lrn_outcome, emurx_nsstat_ev* ev, uint32_t ev_cap,
                        uint8_t* done, uint64_t* info, void* scratch, uint32_t max_frames, uint32_t max_ns, hipStream_t st) {
    using namespace emurx;
    unsigned long long* inf = reinterpret_cast<unsigned long long*>(info);
    if (n == 0) return EMURX_HIP_OK(hipMemsetAsync(inf, 0, 8 * (size_t)EMURX_NSS_INFO_WORDS, st)) ? 0 : -1;
    const uint32_t nt = (n + kNssTile - 1) / kNssTile;
    const NssScratch s = nss_scratch(scratch, max_frames, max_ns);  // sized by the handle, not by n
    hipError_t e = emurx_launch(k_nss_decide, dim3(nt), dim3(kBlock), 0, st, frames, desc, rec, n, kinds, rsp_outcome,
                                lrn_outcome, max_ns < kNssMaxNs ? max_ns : kNssMaxNs, s.acc, s.flag, s.tsum, done);
    if (e == hipSuccess)
        e = emurx_launch(k_nss_scan, dim3(1), dim3(kNssScanBlock), 0, st, s.flag, nss_flags(max_ns), s.tsum, nt, ev_cap, inf);
    if (e == hipSuccess)
        e = emurx_launch(k_nss_emit, dim3((max_ns + kBlock - 1) / kBlock), dim3(kBlock), 0, st, s.acc, s.flag, max_ns, ev_cap,
                         inf, reinterpret_cast<uint2*>(ev));
    return EMURX_HIP_OK(e) ? 0 : -1;
}

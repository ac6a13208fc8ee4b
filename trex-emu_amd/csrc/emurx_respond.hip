// emurx_respond.hip — the stateless answers on the device (gfx950): the ARP reply to a
// request for a client's IPv4 (src/emu/plugins/arp/arp.go:904-933 -> Respond :776-790), the
// ICMPv4 echo reply (plugins/icmp/icmp.go:396-461 -> HandleEcho :289-325), the ICMPv6 echo
// reply (plugins/ipv6/ipv6.go:465-504 -> HandleEcho :315-357) and the neighbour advertisement
// to a neighbour solicitation (plugins/ipv6/nd.go:1546-1685 -> NdClientCtx.Respond :1220-1253);
// and, with the caller's time of day, the ICMPv4 timestamp reply (icmp.go:396-461 -> HandleEcho(ps,
// true) :289-325, iptime :281-287, checksum layers/icmp4.go:252-256 over layers/tcpip.go:76-94).
// emurx_respond_dev / emurx_respond_kinds_dev / emurx_respond_ts_dev, three launches:
//   k_rsp_decide   one frame per lane: the record (32 B) says whether the frame is a candidate
//                  (status OK; lookup EMURX_LK_CLIENT, callback arp / icmp / icmpv6; or lookup
//                  EMURX_LK_NS_LEVEL, callback icmpv6: a neighbour solicitation if its type says
//                  so; each only if `kinds` selects it); only a candidate's descriptor and a few
//                  header bytes are read (ARP: one probe of the IPv4 table; a solicitation: its
//                  addresses as 16-byte spans, one probe of the MAC or the IPv6 table, the client
//                  info for an RA prefix).  Outcome and reply length per frame; per 256-frame tile
//                  the replies, their 16-byte rows and the DROP_MCAST / HOST counts.
//   k_rsp_scan     one workgroup: exclusive scan of the tiles' replies and rows, d_info.
//   k_rsp_emit     one workgroup per tile that has a reply: ordinals and byte offsets by a scan
//                  of the tile's plans in LDS, the descriptors, then the tile's output rows dealt
//                  over the 256 lanes (a 9216 B echo is 576 rows over 256 lanes, not one lane's
//                  loop).  A reply row is one 16-byte span of the request (two aligned loads,
//                  funnel-shifted; shifted by the stripped extension headers from l3 + 40 on),
//                  patched in registers: the swapped Ethernet and IP addresses, which the frame's
//                  own lane put into LDS once per reply, and at most six rewritten bytes (type,
//                  checksum, payload length, next header).  The ARP reply (42-50 B) and the
//                  neighbour advertisement (86-94 B, six rows, checksummed in registers), both
//                  built from their templates, are written by their frame's own lane.
//                  A timestamp reply (kTs) is an echo reply's rows with eight more rewritten bytes
//                  and a checksum over the rest of the frame, [l4, len): each row adds the 16-bit
//                  halves of its patched bytes inside the span to the reply's LDS accumulator as
//                  it is written, and behind a barrier the reply's own lane stores the checksum.
// The kernels are templated on the kinds that need code of their own (kNd, kTs): a call without
// them runs instantiations that hold none of it.
// A batch without candidates costs the read of d_rec and one outcome byte per frame: the emit
// workgroups of tiles without a reply leave after one 8-byte load.
#include <hip/hip_runtime.h>

#include "../../include/emu_rx.h"
#include "emurx_kernels.h"
#include "emurx_parse.h"
#include "emurx_rsp_dev.h"

namespace emurx {

constexpr uint32_t kRspTile = EMURX_QUEUE_TILE;  // frames per workgroup, one per lane
static_assert(kRspTile == kBlock, "one frame per lane of a 256-lane workgroup");
constexpr uint32_t kRspScanBlock = 1024;

// the plan of a frame (kept as outcome << 16 | reply length; a length is a descriptor's u16)
struct RspPlan {
    uint32_t outcome, len;
};

// UpdateInetChecksum (gopacket layers/icmp4.go:238-250): ~cs + ~old + new, folded, complemented
__device__ __forceinline__ uint32_t rsp_update_csum(uint32_t cs, uint32_t oldv, uint32_t newv) {
    uint32_t s = (~cs & 0xffffu) + (~oldv & 0xffffu) + newv;
    while (s > 0xffffu) s = (s >> 16) + (s & 0xffffu);
    return ~s & 0xffffu;
}

// the client of (record's tunnel key, ip) in the IPv4 table, with its MAC (CLookupByIPv4)
__device__ __forceinline__ IpHit rsp_probe_ip4(const emurx_dev_tables& T, uint32_t ns, uint32_t vport, uint32_t v0,
                                               uint32_t v1, uint32_t ip) {
    const uint32_t b = emurx_ip4_hash(emurx_tk_hash(vport, v0, v1), ip) & T.ip4_mask;
    return resolve_ip4(T, b, ld_bucket(T.ip4_tab, b), ns, ip);
}

// The record's words (emurx_rec): ns, client, vlan0, vlan1, vport | l3 << 16, l4 | l7 << 16,
// l7_len | next_hdr << 16 | proto << 24, status | flags << 8 | rsv << 16
__device__ __forceinline__ uint32_t rsp_lk(const uint4& b) { return (b.w >> (8 + EMURX_FLAG_LK_SHIFT)) & 7u; }
template <bool kNd, bool kTs>  // kNd: kinds has EMURX_RSPK_ND; kTs: EMURX_RSPK_TS
__device__ __forceinline__ bool rsp_candidate(const uint4& b, uint32_t kinds) {
    const uint32_t proto = b.z >> 24, status = b.w & 0xff, lk = rsp_lk(b);
    if (status != EMURX_ST_OK) return false;
    constexpr uint32_t kIcmp = kTs ? EMURX_RSPK_ICMP | EMURX_RSPK_TS : EMURX_RSPK_ICMP;  // the kinds the icmp callback serves
    if (lk == EMURX_LK_CLIENT)
        return (proto == EMURX_CB_ARP && (kinds & EMURX_RSPK_ARP)) || (proto == EMURX_CB_ICMP && (kinds & kIcmp)) ||
               (proto == EMURX_CB_ICMPV6 && (kinds & EMURX_RSPK_ICMPV6));
    return kNd && lk == EMURX_LK_NS_LEVEL && proto == EMURX_CB_ICMPV6;
}
template <bool kTs = false>
__device__ __forceinline__ bool rsp_is_reply(uint32_t outcome) {
    return (outcome >= EMURX_RSP_ARP && outcome <= EMURX_RSP_ICMPV6) || outcome == EMURX_RSP_ND ||
           (kTs && outcome == EMURX_RSP_TS);
}

// The decision for a candidate frame.  Header offsets that do not fit the frame (no record of
// emurx_classify_dev for these descriptors has them) give EMURX_RSP_HOST: never guess.
template <bool kTs>
__device__ RspPlan rsp_decide(const uint8_t* __restrict__ frames, const emurx_desc& d, const uint4& a, const uint4& b,
                              const emurx_dev_tables& T, uint32_t kinds) {
    const uint32_t proto = b.z >> 24, l3 = b.x >> 16, l4 = b.y & 0xffffu, len = d.len;
    const uint8_t* f = frames + d.off;
    if (d.pad == EMURX_DESC_HOLE) return {EMURX_RSP_NONE, 0};
    if (l3 < 14 || l3 > len) return {EMURX_RSP_HOST, 0};
    if (proto == EMURX_CB_ARP) {
        if (l3 + 28 > len) return {EMURX_RSP_HOST, 0};
        const uint32_t tpa = rsp_le32(f + l3 + 24);
        const IpHit h = rsp_probe_ip4(T, a.x, b.x & 0xffffu, a.z, a.w, tpa);
        // a handle that does not hold the client (partitioned, or tables changed since the classify)
        if (h.cid != a.y || h.cid == EMURX_ID_NONE) return {EMURX_RSP_HOST, 0};
        return {EMURX_RSP_ARP, 42u + 4u * ((a.z != 0) + (a.w != 0))};
    }
    const bool group_src = gld1(f + 6) & 1;  // broadcast or group bit: eth.IsBroadcast() || IsMcast() after the swap
    if (proto == EMURX_CB_ICMP) {
        if (l3 + 20 > len || l4 + 8 > len) return {EMURX_RSP_HOST, 0};
        if (!rsp_ip4_src_ok(rsp_le32(f + l3 + 12))) return {EMURX_RSP_DROP_MCAST, 0};  // icmp.go:429-436
        const uint32_t tc = gld1(f + l4) << 8 | gld1(f + l4 + 1);
        if (tc == 0x0d00u) {  // timestamp request: the time of day is the caller's (kTs), else the handler's
            if (!kTs || !(kinds & EMURX_RSPK_TS)) return {EMURX_RSP_HOST, 0};
            if (group_src) return {EMURX_RSP_DROP_MCAST, 0};          // icmp.go:295-299
            if (len - l4 < 20) return {EMURX_RSP_DROP_SHORT, 0};      // :312-316, behind the multicast test
            if (l4 & 1u) return {EMURX_RSP_HOST, 0};  // no parse of ours: the rows sum on the 16-bit grid
            return {EMURX_RSP_TS, len};
        }
        if (tc != 0x0800u || (kTs && !(kinds & EMURX_RSPK_ICMP))) return {EMURX_RSP_NONE, 0};
        if (group_src) return {EMURX_RSP_DROP_MCAST, 0};
        return {EMURX_RSP_ICMP, len};
    }
    // ICMPv6 echo request (EMURX_LK_CLIENT implies type 128, code 0)
    if (l3 + 40 > l4 || l4 + 8 > len) return {EMURX_RSP_HOST, 0};
    if (group_src) return {EMURX_RSP_DROP_MCAST, 0};
    // the extension headers go (ipv6.go:331-345); a next header that disagrees with l4 is no parse of ours
    const uint32_t strip = l4 - l3 - 40;
    if ((gld1(f + l3 + 6) != 58) != (strip != 0)) return {EMURX_RSP_HOST, 0};
    return {EMURX_RSP_ICMPV6, len - strip};
}

// The decision for a neighbour solicitation candidate (nd.go:1546-1685; the rule with its
// citations is in include/emu_rx.h).  A reply if and only if the Go handler would reach
// nd.Respond; HOST where a lane cannot cheaply decide.
__device__ RspPlan rsp_decide_nd(const uint8_t* __restrict__ frames, const emurx_desc& d, const uint4& a, const uint4& b,
                                 const emurx_dev_tables& T) {
    const uint32_t l3 = b.x >> 16, l4 = b.y & 0xffffu, len = d.len;
    const uint8_t* f = frames + d.off;
    if (d.pad == EMURX_DESC_HOLE) return {EMURX_RSP_NONE, 0};
    if (l3 < 14 || l3 + 40 > l4 || l4 + 4 > len) return {EMURX_RSP_HOST, 0};
    if (gld1(f + l4) != 135 || gld1(f + l4 + 1) != 0) return {EMURX_RSP_NONE, 0};
    return rsp_nd_checks(  // emurx_rsp_dev.h
        f, l3, l4, len, [](uint32_t o) { return RspPlan{o, 0}; },
        [&](const uint32_t(&w)[4], bool, uint2, const uint32_t(&)[4]) -> RspPlan {
            const bool global = ip6_global(w);
            if (!(ip6_link_local(w) || global)) return {EMURX_RSP_NONE, 0};
            const uint32_t tk = emurx_tk_hash(b.x & 0xffffu, a.z, a.w);
            if (!rsp_nd_client(T, a.x, tk, w, global).ok) return {EMURX_RSP_NONE, 0};
            return {EMURX_RSP_ND, 86u + 4u * ((a.z != 0) + (a.w != 0))};
        });
}

// tile sums: x = replies | DROP_MCAST << 10 | HOST << 20 (each <= 256), y = the replies' 16-byte rows
// (at most 256 * 576 < 2^18); with kTs, y also carries DROP_SHORT << 20 (kRspRowBits).
// kNd: whether the call answers solicitations; without them (emurx_respond_dev) the kernel holds
// none of that path.  Eight waves per SIMD asked for: left to itself the compiler spends 106 SGPRs
// on the nested divergent branches of the (cold) solicitation path, one wave per SIMD less for
// every batch.
constexpr uint32_t kRspRowBits = 20, kRspRowMask = (1u << kRspRowBits) - 1u;
template <bool kNd, bool kTs>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_rsp_decide(
    const uint8_t* __restrict__ frames, const emurx_desc* __restrict__ desc, const emurx_rec* __restrict__ rec, uint32_t n,
    uint32_t kinds, const emurx_dev_tables T, uint32_t* __restrict__ plan, uint2* __restrict__ tsum,
    uint8_t* __restrict__ outcome) {
    __shared__ uint32_t s_sum[2];
    if (threadIdx.x < 2) s_sum[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t i = blockIdx.x * kRspTile + threadIdx.x;
    RspPlan p{EMURX_RSP_NONE, 0};
    if (i < n) {
        const uint4 b = gld16(reinterpret_cast<const uint4*>(rec + i) + 1);
        if (rsp_candidate<kNd, kTs>(b, kinds)) {
            const uint4 a = gld16(reinterpret_cast<const uint4*>(rec + i));
            if (!kNd || rsp_lk(b) == EMURX_LK_CLIENT) p = rsp_decide<kTs>(frames, desc[i], a, b, T, kinds);
            else p = rsp_decide_nd(frames, desc[i], a, b, T);
        }
        if (outcome) outcome[i] = (uint8_t)p.outcome;
    }
    const bool reply = rsp_is_reply<kTs>(p.outcome);
    const uint32_t c = wave_sum_u32((reply ? 1u : 0u) | (p.outcome == EMURX_RSP_DROP_MCAST ? 1u << 10 : 0u) |
                                    (p.outcome == EMURX_RSP_HOST ? 1u << 20 : 0u));
    const uint32_t r = wave_sum_u32((reply ? (p.len + 15) >> 4 : 0u) |
                                    (kTs && p.outcome == EMURX_RSP_DROP_SHORT ? 1u << kRspRowBits : 0u));
    if (lane_id() == 0 && (c | r)) {
        atomicAdd(&s_sum[0], c);
        atomicAdd(&s_sum[1], r);
    }
    __syncthreads();
    if (threadIdx.x == 0) tsum[blockIdx.x] = make_uint2(s_sum[0], s_sum[1]);
    // the plans are read by the emit pass of tiles that have a reply only
    if ((s_sum[0] & 0x3ffu) && i < n) plan[i] = p.outcome << 16 | p.len;
}

// info: {n_out, bytes needed, count of outcomes 1..9, zeros}, info_words (8 or
// EMURX_RSP_INFO_WORDS) of them: the scan writes bytes needed, DROP_MCAST, HOST and (kTs)
// DROP_SHORT and zeroes the rest; the emit pass adds n_out, the replies by kind and NOSPC
template <bool kTs>
__global__ __launch_bounds__(kRspScanBlock) void k_rsp_scan(const uint2* __restrict__ tsum, uint32_t ntiles,
                                                            uint32_t* __restrict__ tord,
                                                            unsigned long long* __restrict__ trow,
                                                            unsigned long long* __restrict__ info, uint32_t info_words) {
    __shared__ BlockScanLds<kRspScanBlock, uint32_t, unsigned long long> s_scan;
    __shared__ uint32_t s_dh[kTs ? 3 : 2];
    if (threadIdx.x < (kTs ? 3 : 2)) s_dh[threadIdx.x] = 0;
    uint32_t cbase = 0, drop = 0, host = 0, shrt = 0;
    // rows are counted in 64 bits (r, the round's total and rbase): a batch of fewer than 2^26
    // jumbo echo requests (576 rows each) can hold more than 2^32 of them
    unsigned long long rbase = 0;
    for (uint32_t t0 = 0; t0 < ntiles; t0 += kRspScanBlock) {  // workgroup-uniform trip count
        const uint32_t t = t0 + threadIdx.x;
        uint2 v = t < ntiles ? tsum[t] : make_uint2(0, 0);
        if (kTs) {
            shrt += v.y >> kRspRowBits;
            v.y &= kRspRowMask;
        }
        const uint32_t cnt = v.x & 0x3ffu;
        drop += (v.x >> 10) & 0x3ffu;
        host += v.x >> 20;
        uint32_t c = cnt;
        unsigned long long r = v.y;
        const auto [ctot, rtot] = block_incl_scan<kRspScanBlock>(s_scan, c, r);
        if (t < ntiles) {
            tord[t] = cbase + c - cnt;
            trow[t] = rbase + r - v.y;
        }
        cbase += ctot;
        rbase += rtot;
    }
    drop = wave_sum_u32(drop);
    host = wave_sum_u32(host);
    if (kTs) shrt = wave_sum_u32(shrt);
    __syncthreads();
    if (lane_id() == 0) {
        atomicAdd(&s_dh[0], drop);
        atomicAdd(&s_dh[1], host);
        if (kTs) atomicAdd(&s_dh[2], shrt);
    }
    __syncthreads();
    if (threadIdx.x < info_words) {
        const uint32_t k = threadIdx.x;
        info[k] = k == 1 ? rbase * 16ull : k == 2 + EMURX_RSP_DROP_MCAST - 1 ? s_dh[0] : k == 2 + EMURX_RSP_HOST - 1 ? s_dh[1]
                  : kTs && k == 2 + EMURX_RSP_DROP_SHORT - 1 ? s_dh[kTs ? 2 : 0] : 0ull;
    }
}

// the mask of the bytes [lo, hi) of a row (0 <= lo < hi <= 16) that lie in its dword d
__device__ __forceinline__ uint32_t rsp_bytes(int lo, int hi, int d) {
    const int a = max(lo - 4 * d, 0), b = min(hi - 4 * d, 4);
    if (a >= b) return 0;
    return (b == 4 ? 0xffffffffu : (1u << (8 * b)) - 1u) & ~((1u << (8 * a)) - 1u);
}
// byte `pos` of the reply, if it lies in the row that starts at y0, becomes v
__device__ __forceinline__ void rsp_set_byte(uint32_t o[4], uint32_t y0, uint32_t pos, uint32_t v) {
    const uint32_t j = pos - y0;
    if (j >= 16) return;
    // selects on the four words, not a store at a computed index (which would put the row in scratch)
    const uint32_t sh = 8 * (j & 3), w = j >> 2, m = ~(0xffu << sh), x = v << sh;
    o[0] = w == 0 ? (o[0] & m) | x : o[0];
    o[1] = w == 1 ? (o[1] & m) | x : o[1];
    o[2] = w == 2 ? (o[2] & m) | x : o[2];
    o[3] = w == 3 ? (o[3] & m) | x : o[3];
}

// what the rows' lanes need of a reply, per reply of the tile
struct RspReply {
    uint32_t src;    // the request's offset in the frame buffer
    uint32_t lens;   // request length | kind (EMURX_RSP_*, 0: do not write) << 16
    uint32_t l3l4;   // l3 | the request's l4 << 16
    uint32_t cs;     // the new checksum | the new IPv6 payload length << 16
};

// the reply whose rows hold row x of the tile: the last k with s_row[k] <= x
__device__ __forceinline__ uint32_t rsp_row_owner(const uint32_t* s_row, uint32_t replies, uint32_t x) {
    uint32_t lo = 0, hi = replies;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (s_row[mid] <= x) lo = mid;
        else hi = mid;
    }
    return lo;
}
// A timestamp reply's rewritten ICMP bytes in the row that starts at y0 (icmp.go:310-319): type 14,
// the checksum field zero (UpdateChecksum zeroes it before it sums, layers/icmp4.go:252-256),
// receive and transmit timestamp = ipt, big-endian.  The eight time bytes may straddle two rows.
__device__ __forceinline__ void rsp_ts_patch(uint32_t o[4], uint32_t y0, uint32_t l4, uint32_t ipt) {
    rsp_set_byte(o, y0, l4, 14u);
    rsp_set_byte(o, y0, l4 + 2, 0u);
    rsp_set_byte(o, y0, l4 + 3, 0u);
#pragma unroll
    for (uint32_t j = 0; j < 8; ++j) rsp_set_byte(o, y0, l4 + 12 + j, (ipt >> (24 - 8 * (j & 3))) & 0xff);
}

template <bool kTs>
__global__ __launch_bounds__(kBlock) void k_rsp_emit(const uint8_t* __restrict__ frames,
                                                     const emurx_desc* __restrict__ desc,
                                                     const emurx_rec* __restrict__ rec, uint32_t n,
                                                     const emurx_dev_tables T, const uint32_t* __restrict__ plan,
                                                     const uint2* __restrict__ tsum, const uint32_t* __restrict__ tord,
                                                     const unsigned long long* __restrict__ trow,
                                                     uint8_t* __restrict__ out, unsigned long long cap,
                                                     emurx_desc* __restrict__ odesc, uint32_t* __restrict__ osrc,
                                                     uint8_t* __restrict__ outcome, unsigned long long* __restrict__ info,
                                                     uint32_t ipt) {
    __shared__ alignas(16) BlockScanLds<kBlock, uint32_t, uint32_t> s_scan;  // aligned: its 8-byte pairs are stored whole
    __shared__ uint32_t s_row[kRspTile + 1];  // first row (in the tile) of reply k; [replies] = the tile's rows
    __shared__ RspReply s_rep[kRspTile];
    __shared__ uint32_t s_mac[kRspTile][3];   // an echo reply's first 12 bytes: the Ethernet addresses swapped
    __shared__ uint32_t s_ip[kRspTile][10];   // its IP addresses swapped (8 or 32 bytes) between two pad dwords
    constexpr uint32_t kCnt = kTs ? 9 : 8;
    // by outcome: written replies by kind (1..3, 7, 8), NOSPC (6); with kTs, from word 16 on, per
    // reply of the tile a timestamp reply's sum of 16-bit halves over [l4, len) (one array: the
    // instantiation without kTs keeps its LDS layout)
    __shared__ uint32_t s_cnt[kTs ? 16 + kRspTile : 8];
    uint32_t* const s_acc = s_cnt + (kTs ? 16 : 0);
    const uint32_t t = blockIdx.x;
    uint2 ts = tsum[t];
    if (kTs) ts.y &= kRspRowMask;
    const uint32_t replies = ts.x & 0x3ffu;
    if (!replies) return;  // workgroup-uniform
    const uint32_t i = t * kRspTile + threadIdx.x;
    if (threadIdx.x < kCnt) s_cnt[threadIdx.x] = 0;
    const uint32_t ord0 = tord[t];
    const unsigned long long row0 = trow[t];
    const uint32_t p = i < n ? plan[i] : 0u;
    const uint32_t kind = p >> 16, rlen = p & 0xffffu;
    const bool reply = rsp_is_reply<kTs>(kind);
    const uint32_t rows = reply ? (rlen + 15) >> 4 : 0u;
    // ordinal and first row inside the tile (the one scan of this launch: kAgain = false)
    uint32_t k = reply ? 1u : 0u, r = rows;
    block_incl_scan<kBlock, false>(s_scan, k, r);
    k -= reply ? 1u : 0u;
    r -= rows;
    if (threadIdx.x == 0) s_row[replies] = ts.y;
    // the reply's place: EMURX_RSP_NOSPC when it does not fit out_cap (or emurx_desc's 32-bit
    // offset); offsets ascend, so the replies that fit are a prefix and keep their ordinals
    const unsigned long long off = (row0 + r) * 16ull, end = off + 16ull * rows;
    const bool fits = end <= cap && end <= (1ull << 32);
    uint32_t tsfix = 0;  // a timestamp reply written: the offset of its checksum in `out` (never 0: off + l4 + 2)
    if (reply) {
        const uint4 a = gld16(reinterpret_cast<const uint4*>(rec + i));
        const uint4 b = gld16(reinterpret_cast<const uint4*>(rec + i) + 1);
        const emurx_desc d = desc[i];
        const uint32_t l3 = b.x >> 16, l4 = b.y & 0xffffu, vport = b.x & 0xffffu;
        const uint8_t* f = frames + d.off;
        RspReply e{d.off, (uint32_t)d.len, l3 | l4 << 16, 0};
        if (fits) {
            odesc[ord0 + k] = emurx_desc{(uint32_t)off, (uint16_t)rlen, (uint8_t)vport, 0};
            osrc[ord0 + k] = i;
            if (kind == EMURX_RSP_ARP) {
                // the template's reply (arp.go:621-636,776-790, ns_ctx.go:634-653): the frame's own
                // lane writes its 3 or 4 rows.  The client's MAC is the IPv4 slot's (the probe of
                // k_rsp_decide again; a miss now cannot happen on one stream: the reply is still
                // the decided length, with a zero MAC)
                const uint32_t tpa = rsp_le32(f + l3 + 24);
                const IpHit h = rsp_probe_ip4(T, a.x, vport, a.z, a.w, tpa);
                const uint32_t m03 = h.cid == a.y ? h.mlo : 0u, m45 = h.cid == a.y ? h.mhip & 0xffffu : 0u;
                const uint32_t s03 = rsp_le32(f + l3 + 8), s45 = gld1(f + l3 + 12) | gld1(f + l3 + 13) << 8;
                const uint32_t spa = rsp_le32(f + l3 + 14);
                const uint32_t ntag = (a.z != 0) + (a.w != 0);
                const uint32_t tag0 = __builtin_bswap32(a.z ? a.z : a.w), tag1 = __builtin_bswap32(a.w);
                // dst = the request's sender hardware address, src = the client; then, from the
                // EtherType on: 0806 0001 0800 06 04 0002, client MAC, target IP, sender MAC, sender IP
                const uint32_t head[3] = {s03, s45 | m03 << 16, m03 >> 16 | m45 << 16};
                const uint32_t body[8] = {0x01000608u, 0x04060008u, 0x00000200u | m03 << 16, m03 >> 16 | m45 << 16,
                                          tpa, s03, s45 | spa << 16, spa >> 16};
                uint32_t w[16];
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    const uint32_t w0 = j < 3 ? head[j] : j < 11 ? body[j - 3] : 0u;
                    const uint32_t w1 = j < 3 ? head[j] : j == 3 ? tag0 : j < 12 ? body[j - 4] : 0u;
                    const uint32_t w2 = j < 3 ? head[j] : j == 3 ? tag0 : j == 4 ? tag1 : j < 13 ? body[j - 5] : 0u;
                    w[j] = ntag == 0 ? w0 : ntag == 1 ? w1 : w2;
                }
                uint4* o = reinterpret_cast<uint4*>(out + off);
#pragma unroll
                for (uint32_t j = 0; j < 4; ++j)
                    if (j < rows) o[j] = make_uint4(w[4 * j], w[4 * j + 1], w[4 * j + 2], w[4 * j + 3]);
            } else if (kind == EMURX_RSP_ND) {
                // the template's advertisement (nd.go:835-865, 1220-1253): the frame's own lane
                // writes its six rows.  An EUI-64 target names the client's MAC; for any other
                // target the MAC is the IPv6 slot's (the probe of k_rsp_decide again; on a miss,
                // as for ARP, the reply keeps the decided length, with a zero MAC)
                const uintptr_t Fa = (uintptr_t)f;
                uint32_t tg[4], sa[4], m[4];
                rsp_load16(Fa, d.len, (int)(l4 + 8), tg);
                rsp_load16(Fa, d.len, (int)(l3 + 8), sa);
                rsp_load16(Fa, d.len, 0, m);
                uint32_t m03, m45;
                if (rsp_nd_eui(tg)) {
                    const uint2 em = eui_mac(tg[2], tg[3]);
                    m03 = em.x;
                    m45 = em.y;
                } else {
                    const RspNdHit h = rsp_nd_ip6(T, a.x, emurx_tk_hash(vport, a.z, a.w), tg);
                    m03 = h.ok ? h.mlo : 0u;
                    m45 = h.ok ? h.mhi : 0u;
                }
                const bool dad = ip6_unspecified(sa);
                // the IPv6 packet's 18 words: header, source, destination, 88 00 cs cs, fl 00 00 00,
                // the target, 02 01 + the MAC.  Unicast: from the target to the request's source,
                // flags 0x60; duplicate address detection: from the client's link-local address
                // (fe80:: + EUI-64 of the MAC) to ff02::1, flags 0
                uint32_t P[18];
                P[0] = 0x00000060u;
                P[1] = 0xff3a2000u;
                const uint32_t ll2 = ((m03 & 0xffu) ^ 2u) | (m03 & 0xffff00u) | 0xff000000u;
                const uint32_t ll3 = 0xfeu | (m03 >> 24) << 8 | m45 << 16;
                P[2] = dad ? 0x000080feu : tg[0];
                P[3] = dad ? 0u : tg[1];
                P[4] = dad ? ll2 : tg[2];
                P[5] = dad ? ll3 : tg[3];
                P[6] = dad ? 0x000002ffu : sa[0];
                P[7] = dad ? 0u : sa[1];
                P[8] = dad ? 0u : sa[2];
                P[9] = dad ? 0x01000000u : sa[3];
                P[10] = 0x00000088u;
                P[11] = dad ? 0u : 0x60u;
#pragma unroll
                for (int j = 0; j < 4; ++j) P[12 + j] = tg[j];
                P[16] = 0x00000102u | m03 << 16;
                P[17] = m03 >> 16 | m45 << 16;
                // FixIcmpL4Checksum (ip6.go:54-56): the pseudo header (addresses, length 32, next
                // header 58) and the 32 bytes; every word sits at an even offset, so the sum of
                // little-endian halves is the byte-swapped sum and its complement goes in as is
                uint32_t acc = sad16(0x20000000u, sad16(0x3a000000u, 0u));
#pragma unroll
                for (int j = 2; j < 18; ++j) acc = sad16(P[j], acc);
                P[10] |= (~fold16(acc) & 0xffffu) << 16;
                const uint32_t ntag = (a.z != 0) + (a.w != 0);
                const uint32_t tag0 = __builtin_bswap32(a.z ? a.z : a.w), tag1 = __builtin_bswap32(a.w);
                // dst = the request's Ethernet source or 33:33:00:00:00:01, src = the client; from
                // the EtherType on, the packet sits two bytes off the dword grid
                const uint32_t d03 = dad ? 0x00003333u : m[1] >> 16 | m[2] << 16, d45 = dad ? 0x0100u : m[2] >> 16;
                const uint32_t head[3] = {d03, d45 | m03 << 16, m03 >> 16 | m45 << 16};
                uint32_t body[19];
                body[0] = 0xdd86u | P[0] << 16;
#pragma unroll
                for (int j = 1; j < 18; ++j) body[j] = P[j - 1] >> 16 | P[j] << 16;
                body[18] = P[17] >> 16;
                uint4* o = reinterpret_cast<uint4*>(out + off);
#pragma unroll
                for (int r4 = 0; r4 < 6; ++r4) {  // rows == 6 for 86, 90 and 94 bytes
                    uint32_t w[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int j = 4 * r4 + q;
                        const uint32_t w0 = j < 3 ? head[j] : j < 22 ? body[j - 3] : 0u;
                        const uint32_t w1 = j < 3 ? head[j] : j == 3 ? tag0 : j < 23 ? body[j - 4] : 0u;
                        const uint32_t w2 = j < 3 ? head[j] : j == 3 ? tag0 : j == 4 ? tag1 : body[j - 5];
                        w[q] = ntag == 0 ? w0 : ntag == 1 ? w1 : w2;
                    }
                    o[r4] = make_uint4(w[0], w[1], w[2], w[3]);
                }
            } else {
                const uint32_t l4n = kind == EMURX_RSP_ICMP ? l4 : l3 + 40;  // the reply's l4
                const uint32_t ocs = gld1(f + l4 + 2) << 8 | gld1(f + l4 + 3);
                const uint32_t ncs = kind == EMURX_RSP_ICMP ? rsp_update_csum(ocs, 0x0800u, 0x0000u)
                                                            : rsp_update_csum(ocs, 0x8000u, 0x8100u);
                uint32_t plen = 0;
                if (kind == EMURX_RSP_ICMPV6)  // PayloadLength() - optionbytes, uint16 (ipv6.go:335)
                    plen = ((gld1(f + l3 + 4) << 8 | gld1(f + l3 + 5)) - (l4 - l4n)) & 0xffffu;
                e.cs = ncs | plen << 16;
                if (kTs) s_acc[k] = 0;
                if (kTs && kind == EMURX_RSP_TS) tsfix = (uint32_t)off + l4 + 2;  // even: l4 is, off a multiple of 16
                e.lens |= kind << 16;
                // the swapped addresses, once per reply: Ethernet (row 0's first 12 bytes) and IP
                const uintptr_t Fa = (uintptr_t)f;
                uint32_t m[4], s[4], t[4] = {0, 0, 0, 0};
                rsp_load16(Fa, d.len, 0, m);
                s_mac[k][0] = m[1] >> 16 | m[2] << 16;
                s_mac[k][1] = m[2] >> 16 | m[0] << 16;
                s_mac[k][2] = m[0] >> 16 | m[1] << 16;
                const bool v6 = kind == EMURX_RSP_ICMPV6;
                rsp_load16(Fa, d.len, (int)(l3 + (v6 ? 8u : 12u)), s);  // IPv4: source, destination in s[0], s[1]
                if (v6) rsp_load16(Fa, d.len, (int)(l3 + 24), t);
                s_ip[k][0] = 0;  // the pad ahead: a dword that begins before the addresses
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    s_ip[k][1 + j] = v6 ? t[j] : j == 0 ? s[1] : j == 1 ? s[0] : 0u;
                    s_ip[k][5 + j] = v6 ? s[j] : 0u;
                }
                s_ip[k][9] = 0;
            }
        } else if (outcome) {
            outcome[i] = EMURX_RSP_NOSPC;
        }
        s_row[k] = r;
        s_rep[k] = e;
        atomicAdd(&s_cnt[fits ? kind : (uint32_t)EMURX_RSP_NOSPC], 1u);
    }
    __syncthreads();
    if (threadIdx.x < kCnt) {  // info[1 + outcome] counts the outcome; info[0] = the replies written
        // (ND is no outcome of the eight-word form: its count is 0 there and info[8] is not touched)
        const uint32_t j = threadIdx.x;
        const uint32_t c = j ? s_cnt[j]
                             : s_cnt[EMURX_RSP_ARP] + s_cnt[EMURX_RSP_ICMP] + s_cnt[EMURX_RSP_ICMPV6] + s_cnt[EMURX_RSP_ND] +
                                   (kTs ? s_cnt[kTs ? EMURX_RSP_TS : 0] : 0u);
        if (c) atomicAdd(&info[j ? 1u + j : 0u], (unsigned long long)c);
    }
    const uint32_t R = ts.y;
    // ---- the echo (and timestamp) replies' rows, dealt over the lanes.
    // A timestamp reply's checksum covers the rest of the frame, [l4, len), so it is known only once
    // every row of the reply has been seen: its rows go out with the checksum field zero and add the
    // sum of the 16-bit halves of their bytes inside the span to the reply's accumulator; behind a
    // barrier the reply's own lane stores the two checksum bytes (below).  l4 is even and a row
    // starts at a multiple of 16, so a little-endian half is a byte-swapped pair of tcpipChecksum
    // (layers/tcpip.go:76-94), an odd last byte lands in the pair's high byte once swapped, and a
    // u32 holds the sum of any frame a u16 length describes (32,768 halves).
    for (uint32_t x = threadIdx.x; x < R; x += kBlock) {
        const uint32_t lo = rsp_row_owner(s_row, replies, x);
        const RspReply e = s_rep[lo];
        const uint32_t ek = e.lens >> 16;
        if (ek != EMURX_RSP_ICMP && ek != EMURX_RSP_ICMPV6 && !(kTs && ek == EMURX_RSP_TS)) continue;  // ARP, or no room
        const bool v6 = ek == EMURX_RSP_ICMPV6;
        const uint32_t flen = e.lens & 0xffffu, l3 = e.l3l4 & 0xffffu, l4 = e.l3l4 >> 16;
        const uint32_t strip = v6 ? l4 - l3 - 40 : 0u;
        const uint32_t y0 = 16 * (x - s_row[lo]);
        // One shifted 16-byte span of the request per row: reply[y] = E[y], or E[y + strip] from
        // l3 + 40 on (IPv6: p[l4:] moved down).  A row that straddles l3 + 40 takes the shifted
        // span: its bytes below l3 + 40 are all address bytes (32 of them end there), which
        // come from the swapped copy in LDS like the Ethernet addresses of row 0.
        const uintptr_t F = (uintptr_t)(frames + e.src);
        uint32_t o[4];
        rsp_load16(F, flen, (int)(y0 + (v6 && y0 + 16 > l3 + 40 ? strip : 0u)), o);
        if (y0 == 0) {
            o[0] = s_mac[lo][0];
            o[1] = s_mac[lo][1];
            o[2] = s_mac[lo][2];
        }
        const uint32_t astart = l3 + (v6 ? 8u : 12u), aend = astart + (v6 ? 32u : 8u);
        if (y0 + 16 > astart && y0 < aend) {
#pragma unroll
            for (int dw = 0; dw < 4; ++dw) {
                const int a = (int)astart - (int)(y0 + 4 * dw), b = (int)aend - (int)(y0 + 4 * dw);  // in this dword
                if (a < 4 && b > 0) {
                    const uint32_t q = (uint32_t)(4 - a);  // s_ip byte of the dword's first byte (one pad dword ahead)
                    const uint32_t v = __builtin_amdgcn_alignbyte(s_ip[lo][(q >> 2) + 1], s_ip[lo][q >> 2], q & 3);
                    const uint32_t m = rsp_bytes(a, b, 0);
                    o[dw] = (o[dw] & ~m) | (v & m);
                }
            }
        }
        const uint32_t tpos = v6 ? l3 + 40 : l4;
        if (kTs && ek == EMURX_RSP_TS) {
            rsp_ts_patch(o, y0, l4, ipt);
            if (y0 + 16 > l4) {  // the patched bytes of this row that lie in [l4, len)
                const int b0 = max((int)l4 - (int)y0, 0), b1 = min((int)flen - (int)y0, 16);
                uint32_t acc = 0;
#pragma unroll
                for (int dw = 0; dw < 4; ++dw) acc = sad16(o[dw] & rsp_bytes(b0, b1, dw), acc);
                atomicAdd(&s_acc[lo], acc);
            }
        } else {
            rsp_set_byte(o, y0, tpos, v6 ? 129u : 0u);
            rsp_set_byte(o, y0, tpos + 2, (e.cs >> 8) & 0xff);
            rsp_set_byte(o, y0, tpos + 3, e.cs & 0xff);
        }
        if (strip) {
            rsp_set_byte(o, y0, l3 + 4, e.cs >> 24);
            rsp_set_byte(o, y0, l3 + 5, (e.cs >> 16) & 0xff);
            rsp_set_byte(o, y0, l3 + 6, 58u);
        }
        *reinterpret_cast<uint4*>(out + (row0 + x) * 16ull) = make_uint4(o[0], o[1], o[2], o[3]);
    }
    // ---- the timestamp replies' checksums: only a tile that wrote such a reply comes here
    if (kTs && s_cnt[kTs ? EMURX_RSP_TS : 0]) {  // workgroup-uniform
        __syncthreads();  // every row's sum is in, and every row's store is ordered before the store below
        // the complement of the folded sum, still in the halves' byte order: one 16-bit store puts
        // its low byte first, the checksum's first byte in memory (a folded sum of 0xffff stores 0x0000)
        if (tsfix) *reinterpret_cast<uint16_t*>(out + tsfix) = (uint16_t)(~fold16(s_acc[k]) & 0xffffu);
    }
}

}  // namespace emurx

// scratch: plan u32 [n], tile sums uint2 [ntiles], tile ordinals u32 [ntiles], tile rows u64 [ntiles]
struct RspScratch {
    uint32_t* plan;
    uint2* tsum;
    uint32_t* tord;
    unsigned long long* trow;
    size_t bytes;
};
static RspScratch rsp_scratch(void* base, uint32_t n) {
    const size_t nt = ((size_t)n + emurx::kRspTile - 1) / emurx::kRspTile;
    emurx_carver c(base);  // the initialisers run in order
    return {c.take<uint32_t>(n), c.take<uint2>(nt), c.take<uint32_t>(nt), c.take<unsigned long long>(nt), c.bytes()};
}
size_t emurx_rsp_scratch_bytes(uint32_t n) { return rsp_scratch(nullptr, n).bytes; }

int emurx_launch_respond(const uint8_t* frames, const emurx_desc* desc, const emurx_rec* rec, uint32_t n,
                         uint32_t kinds, const emurx_dev_tables& T, uint8_t* out, uint64_t cap, emurx_desc* out_desc,
                         uint32_t* out_src, uint8_t* outcome, uint64_t* info, uint32_t info_words, uint32_t ip_time_ms,
                         void* scratch, hipStream_t st) {
    using namespace emurx;
    unsigned long long* inf = reinterpret_cast<unsigned long long*>(info);
    if (n == 0) return EMURX_HIP_OK(hipMemsetAsync(inf, 0, 8 * (size_t)info_words, st)) ? 0 : -1;
    const uint32_t nt = (n + kRspTile - 1) / kRspTile;
    const RspScratch s = rsp_scratch(scratch, n);
    // a call without the timestamp kind runs the instantiations that hold none of its code
    const bool nd = kinds & EMURX_RSPK_ND, tsk = kinds & EMURX_RSPK_TS;
    const auto decide = tsk ? (nd ? k_rsp_decide<true, true> : k_rsp_decide<false, true>)
                            : (nd ? k_rsp_decide<true, false> : k_rsp_decide<false, false>);
    hipError_t e = emurx_launch(decide, dim3(nt), dim3(kBlock), 0, st, frames, desc, rec, n, kinds, T, s.plan, s.tsum,
                                outcome);
    if (e == hipSuccess)
        e = emurx_launch(tsk ? k_rsp_scan<true> : k_rsp_scan<false>, dim3(1), dim3(kRspScanBlock), 0, st, s.tsum, nt, s.tord,
                         s.trow, inf, info_words);
    if (e == hipSuccess)
        e = emurx_launch(tsk ? k_rsp_emit<true> : k_rsp_emit<false>, dim3(nt), dim3(kBlock), 0, st, frames, desc, rec, n, T,
                         s.plan, s.tsum, s.tord, s.trow, out, (unsigned long long)cap, out_desc, out_src, outcome, inf,
                         ip_time_ms);
    return EMURX_HIP_OK(e) ? 0 : -1;
}

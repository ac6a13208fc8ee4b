// emurx_ping.hip — the echo replies and destination-unreachable messages of a classified batch,
// folded on the device (gfx950) into one event per ping {ns_id, client_id, family, identifier}:
// PluginIcmpNs.HandleEchoReply / HandleDestinationUnreachable (src/emu/plugins/icmp/icmp.go:328-393),
// PluginIpv6Ns.HandleEchoReply / HandleDestinationUnreachable (plugins/ipv6/ipv6.go:359-462) and
// Ping.HandleEchoReply (plugins/ping/ping.go:246-295).  The rule with its citations is in
// include/emu_rx.h.  emurx_ping_dev, five launches:
//   k_png_decide   one frame per lane: the record's second half says whether the frame is a
//                  candidate; only a candidate's descriptor and bytes are read.  A frame with
//                  outcome 1..4 leaves its key {ns, client, family << 16 | ident}, its sequence
//                  number, its class (malformed, bad latency, accepted) and its latency in a
//                  32-byte row of its own (fr[i]).  ns_id and client_id are not in the frame (the
//                  ICMPv6 client comes from a MAC probe), so the key is kept there.
//   k_png_fold     a frame with outcome 1..4 claims a slot of the set by one compare-and-swap of
//                  the slot's owner word (0 -> frame index + 1 | five bits of the hash), as the
//                  learning fold does, or finds the slot whose owner's key equals its own: the
//                  owner's key is fr[owner], which the previous launch wrote, so nothing but the
//                  owner word is published and no atomic needs an ordering.  The key's
//                  accumulator is the row of its owner frame (acc[owner]): everything that does
//                  not depend on order goes in by relaxed atomics (the counts, the latency sum and
//                  maximum, ~first / last, the indices of the first and last accepted reply and of
//                  the last zero latency; all start from zero).
//   k_png_mark     the frame whose index equals its row's `last` emits the event; an accepted
//                  reply of a key with more than one adds its latency to the row's minimum if it
//                  lies behind the key's last zero latency (final since the fold), and is marked
//                  for the ordered pass.  Per 256-frame tile the emitters and the marked frames.
//   k_png_scan     one workgroup: the exclusive scan of the tiles' emitters, the outcome counts,
//                  distinct keys against ev_cap, d_info; then the ordered pass, n_succ: it walks
//                  the tiles that hold a marked frame in rx order, 1,024 frames a step; a marked
//                  frame finds its predecessor (the nearest marked frame of its row before it) in
//                  the step's LDS image (its marked frames alone, compacted in rx order) or, failing that, in the row's carry word, which the last
//                  frame of each row in a step leaves.  A key with one accepted reply (in real
//                  traffic nearly every key) has no marked frame; the steps that hold one are
//                  a bitmap in LDS, so the walk visits those alone, and of such a step only the
//                  tiles that hold one: the others may still carry an earlier call's row indices.
//   (k_png_out     a slot's ping stage only, emurx_ingest_set_ping: the results into pinned memory)
//   k_png_emit     an emitter's event goes to the tile's ordinal + its rank in the tile (frame
//                  order = ascending `last`), unless the batch overflows; either way the emitter
//                  zeroes its row and its slot, so that the scratch is as the call found it.
// A batch without candidates costs the read of the records' second halves and one outcome byte
// per frame: the workgroups of the other passes leave after one 8-byte load.
#include <hip/hip_runtime.h>

#include "../../include/emu_rx.h"
#include "emurx_kernels.h"
#include "emurx_parse.h"
#include "emurx_rsp_dev.h"

namespace emurx {

constexpr uint32_t kPngTile = EMURX_QUEUE_TILE;  // frames per workgroup, one per lane
static_assert(kPngTile == kBlock, "one frame per lane of a 256-lane workgroup");
static_assert(sizeof(emurx_ping_ev) == 80 && offsetof(emurx_ping_ev, lat_sum) == 48, "k_png_emit writes ten 8-byte words");
constexpr uint32_t kPngScanBlock = 1024;  // also the frames of one step of the ordered pass
constexpr uint32_t kPngStepTiles = kPngScanBlock / kPngTile;
// the steps of the largest batch (n < EMURX_TX_ZMQ_MAX_FRAMES), a bit each
constexpr uint32_t kPngStepWords = EMURX_TX_ZMQ_MAX_FRAMES / kPngScanBlock / 32;
constexpr uint32_t kPngNone = 0xffffffffu;
// row_of[i]: the frame's row | class << 26 | emits << 30 | marked << 31; rows are below 2^26
constexpr uint32_t kPngRowMask = (1u << 26) - 1, kPngClsShift = 26, kPngEmits = 1u << 30, kPngMarked = 1u << 31;
enum : uint32_t { kPngClsNone = 0, kPngClsMalformed = 1, kPngClsBadLatency = 2, kPngClsOk = 3 };
// an accumulator row, 24 words: the 64-bit words sit at even offsets of the 32-byte aligned rows
enum : uint32_t {
    kAccReply = 0, kAccUnreach, kAccMalformed, kAccBadLat, kAccOk, kAccSucc, kAccNoClient, kAccMcast,
    kAccNFirst,    // ~first
    kAccLast,
    kAccNFirstOk,  // ~index of the first accepted reply
    kAccLastOk,    // index of the last accepted reply + 1
    kAccLastZero,  // index of the last accepted reply with latency 0, + 1
    kAccSlot,      // the key's slot in the set + 1: the claimer's store
    kAccCarry,     // the ordered pass: seq + 1 of the row's last marked frame so far
    kAccPad,
    kAccLatSum = 16, kAccLatMax = 18, kAccNegMin = 20,  // u64 each; ~(minimum behind the last zero)
    kAccWords = 24
};

struct PngPlan {
    uint32_t outcome, cid, ident, seq, cls;
    unsigned long long lat;
};
__device__ __forceinline__ PngPlan png_plan(uint32_t outcome) { return {outcome, EMURX_ID_NONE, 0, 0, kPngClsNone, 0}; }
__device__ __forceinline__ bool png_folds(uint32_t o) { return o >= EMURX_PNG_REPLY && o <= EMURX_PNG_MCAST; }

// The record's words: as in emurx_respond.hip
__device__ __forceinline__ uint32_t png_lk(const uint4& b) { return (b.w >> (8 + EMURX_FLAG_LK_SHIFT)) & 7u; }
__device__ __forceinline__ bool png_candidate(const uint4& b, uint32_t fams) {
    const uint32_t proto = b.z >> 24, status = b.w & 0xff;
    if (status != EMURX_ST_OK) return false;
    if (proto == EMURX_CB_ICMP) return fams & EMURX_PNGK_V4;
    return proto == EMURX_CB_ICMPV6 && (fams & EMURX_PNGK_V6);
}

__device__ __forceinline__ uint32_t png_be16(const uint8_t* p) { return gld1(p) << 8 | gld1(p + 1); }
__device__ __forceinline__ unsigned long long png_be64(const uint8_t* p) {
    const uint32_t hi = __builtin_bswap32(rsp_le32(p)), lo = __builtin_bswap32(rsp_le32(p + 4));
    return (unsigned long long)hi << 32 | lo;
}

// An echo reply whose 24 bytes from e = p + l4 fit the frame (Ping.HandleEchoReply ping.go:246-295)
__device__ PngPlan png_reply(const uint8_t* e, uint32_t cid, unsigned long long now) {
    PngPlan p = {EMURX_PNG_REPLY, cid, png_be16(e + 4), png_be16(e + 6), kPngClsMalformed, 0};
    if (png_be64(e + 8) != EMURX_PING_MAGIC) return p;  // :255-259
    const long long ts = (long long)png_be64(e + 16), nw = (long long)now;  // now < 2^63
    // latency < 0 || latency > 5 s with Time.Sub saturating (:266-270): nw - 5e9 cannot wrap
    if (ts > nw || ts < nw - (long long)EMURX_PING_TIMEOUT_NS) {
        p.cls = kPngClsBadLatency;
        return p;
    }
    p.cls = kPngClsOk;
    p.lat = (unsigned long long)(nw - ts);
    return p;
}

// The decision for a candidate frame; a, b: the record's halves
__device__ PngPlan png_decide(const uint8_t* __restrict__ frames, const emurx_desc& d, const uint4& a, const uint4& b,
                              const emurx_dev_tables& T, unsigned long long now) {
    const uint32_t proto = b.z >> 24, lk = png_lk(b), l3 = b.x >> 16, l4 = b.y & 0xffffu, len = d.len;
    const uint8_t* f = frames + d.off;
    if (d.pad == EMURX_DESC_HOLE) return png_plan(EMURX_PNG_NONE);
    if (proto == EMURX_CB_ICMP) {  // icmp.go:396-462, 328-393
        if (l3 < 14 || l3 + 20 > len || l4 + 8 > len) return png_plan(EMURX_PNG_HOST);
        if (lk != EMURX_LK_CLIENT && lk != EMURX_LK_CLIENT_NO_PLUGIN) return png_plan(EMURX_PNG_NONE);
        const uint32_t type = gld1(f + l4), code = gld1(f + l4 + 1);
        const bool reply = type == 0 && code == 0;
        if (!reply && !(type == 3 && code <= 4)) return png_plan(EMURX_PNG_NONE);
        if (!rsp_ip4_src_ok(rsp_le32(f + l3 + 12))) return png_plan(EMURX_PNG_MCAST);  // :433-436
        if (l4 != l3 + 20) return png_plan(EMURX_PNG_HOST);  // IHL > 5: IPv4.DecodeFromBytes fails on the 20-byte slice
        // GetIcmpClientByMac(dst) :349-351, :384-386: IsUnicastToMe has matched the destination MAC
        // with the client's, so it is the record's client; the classifier does not look at the
        // client's plugins for this callback (lookup CLIENT either way), the client info table does
        if (lk == EMURX_LK_CLIENT_NO_PLUGIN || !(client_info(T, a.y).plugins & (1u << EMURX_PLUG_ICMP)))
            return png_plan(EMURX_PNG_NO_CLIENT);
        if (reply) {
            if (len - (l4 + 8) < 16) return png_plan(EMURX_PNG_HOST);  // :182-185
            return png_reply(f + l4, a.y, now);
        }
        if (len < l4 + 36) return png_plan(EMURX_PNG_HOST);  // :378
        return {EMURX_PNG_UNREACH, a.y, png_be16(f + l4 + 32), 0, kPngClsNone, 0};
    }
    // icmpv6: ipv6.go:517-532, 359-462
    if (l3 < 14 || l3 + 40 > l4 || l4 + 4 > len) return png_plan(EMURX_PNG_HOST);
    const uint32_t type = gld1(f + l4), code = gld1(f + l4 + 1);
    const bool reply = type == 129 && code == 0;
    if ((!reply && !(type == 1 && code <= 6)) || lk != EMURX_LK_NS_LEVEL) return png_plan(EMURX_PNG_NONE);
    if (len - l4 < (reply ? 24u : 72u)) return png_plan(EMURX_PNG_HOST);  // :389, :445
    // GetIcmpClientByMac(dst) :559-573; CLookupByMac finds no zero MAC (core/ns_ctx.go:262-265)
    const uint32_t mlo = rsp_le32(f), mhi = gld1(f + 4) | gld1(f + 5) << 8;
    if (mlo == 0 && mhi == 0) return png_plan(EMURX_PNG_NO_CLIENT);
    const uint32_t bk = emurx_mac_hash(emurx_tk_hash(b.x & 0xffffu, a.z, a.w), mlo, mhi) & T.mac_mask;
    const uint2 c = resolve_mac(T, bk, ld_bucket(T.mac_tab, bk), a.x, mlo, mhi);
    if (c.x == EMURX_ID_NONE || !(c.y & (1u << EMURX_PLUG_IPV6))) return png_plan(EMURX_PNG_NO_CLIENT);  // :397-399, :453-455
    if (reply) return png_reply(f + l4, c.x, now);
    return {EMURX_PNG_UNREACH, c.x, png_be16(f + l4 + 52), 0, kPngClsNone, 0};
}

// tile sums: x = REPLY | UNREACH << 10 | NO_CLIENT << 20, y = MCAST | HOST << 10 (each <= 256)
__device__ __forceinline__ uint32_t png_tile_folds(const uint2& ts) {
    return (ts.x & 0x3ffu) + ((ts.x >> 10) & 0x3ffu) + (ts.x >> 20) + (ts.y & 0x3ffu);
}

// fr[i]: {client, ident | family << 16 | outcome << 24, seq, ns} {latency, 0, 0}; the key is
// words 0, 1 & 0xffffff and 3 (a Namespace-level outcome has client 0xffffffff and ident 0)
__global__ __launch_bounds__(kBlock) void k_png_decide(const uint8_t* __restrict__ frames, const emurx_desc* __restrict__ desc,
                                                       const emurx_rec* __restrict__ rec, uint32_t n, uint32_t fams,
                                                       unsigned long long now, const emurx_dev_tables T,
                                                       uint4* __restrict__ fr, uint2* __restrict__ tsum,
                                                       uint8_t* __restrict__ outcome) {
    __shared__ uint32_t s_sum[2];
    if (threadIdx.x < 2) s_sum[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t i = blockIdx.x * kPngTile + threadIdx.x, lane = lane_id();
    PngPlan p = png_plan(EMURX_PNG_NONE);
    uint32_t ns = 0, fam = 0;
    if (i < n) {
        const uint4 b = gld16(reinterpret_cast<const uint4*>(rec + i) + 1);
        if (png_candidate(b, fams)) {
            const uint4 a = gld16(reinterpret_cast<const uint4*>(rec + i));
            p = png_decide(frames, desc[i], a, b, T, now);
            ns = a.x;
            fam = (b.z >> 24) == EMURX_CB_ICMP ? 4u : 6u;
        }
        if (outcome) outcome[i] = (uint8_t)p.outcome;
    }
    const uint32_t o = p.outcome;
    const uint32_t cx = wave_sum_u32((o == EMURX_PNG_REPLY ? 1u : 0u) | (o == EMURX_PNG_UNREACH ? 1u << 10 : 0u) |
                                     (o == EMURX_PNG_NO_CLIENT ? 1u << 20 : 0u));
    const uint32_t cy = wave_sum_u32((o == EMURX_PNG_MCAST ? 1u : 0u) | (o == EMURX_PNG_HOST ? 1u << 10 : 0u));
    if (lane == 0 && (cx | cy)) {
        atomicAdd(&s_sum[0], cx);
        atomicAdd(&s_sum[1], cy);
    }
    __syncthreads();
    const uint2 ts = make_uint2(s_sum[0], s_sum[1]);
    if (threadIdx.x == 0) tsum[blockIdx.x] = ts;
    if (!png_tile_folds(ts) || i >= n) return;  // the rows are read by the later passes of tiles that fold only
    const bool nsl = o == EMURX_PNG_NO_CLIENT || o == EMURX_PNG_MCAST;
    fr[2 * (size_t)i] = make_uint4(nsl ? EMURX_ID_NONE : p.cid, (nsl ? 0u : p.ident) | fam << 16 | o << 24 | p.cls << 28, p.seq, ns);
    fr[2 * (size_t)i + 1] = make_uint4((uint32_t)p.lat, (uint32_t)(p.lat >> 32), 0, 0);
}

__device__ __forceinline__ uint32_t png_hash(uint32_t ns, uint32_t cid, uint32_t fi) {
    uint32_t h = ns * 0x9E3779B1u ^ cid * 0x85EBCA6Bu ^ fi * 0xC2B2AE35u;
    h ^= h >> 15;
    h *= 0x2C1B3C6Du;
    h ^= h >> 12;
    h *= 0x297A2D39u;
    return h ^ h >> 15;
}

// The row of the key of frame i (its fr row k, hash h) in the set of mask + 1 owner words, owner =
// frame + 1 | the hash's top five bits << 27 (n < 2^26): claimed for frame i by one
// compare-and-swap, or found; the owner's key is fr[owner], which the decide launch wrote.  The
// batch's part of the set has at least twice as many slots as the batch has frames, so a free
// slot always ends the probe; the trip count is bounded all the same.
__device__ __forceinline__ uint32_t png_insert(uint32_t* own, uint32_t mask, const uint4* __restrict__ fr, const uint4& k,
                                               uint32_t h, uint32_t i, uint32_t& slot) {
    const uint32_t mine = (i + 1) | (h >> 27) << 27;
    for (uint32_t p = h & mask, t = 0; t <= mask; p = (p + 1) & mask, ++t) {
        uint32_t cur = __hip_atomic_load(own + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == 0 && __hip_atomic_compare_exchange_strong(own + p, &cur, mine, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                             __HIP_MEMORY_SCOPE_AGENT)) {
            slot = p;
            return i;
        }
        if ((cur ^ mine) >> 27) continue;  // another hash
        const uint32_t j = (cur & 0x7ffffffu) - 1;
        const uint4 o = gld16(fr + 2 * (size_t)j);
        if (o.x == k.x && ((o.y ^ k.y) & 0xffffffu) == 0 && o.w == k.w) return j;
    }
    return kPngNone;
}

__device__ __forceinline__ void png_add(uint32_t* row, uint32_t w, uint32_t v = 1) {
    __hip_atomic_fetch_add(row + w, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void png_max(uint32_t* row, uint32_t w, uint32_t v) {
    __hip_atomic_fetch_max(row + w, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void png_max64(uint32_t* row, uint32_t w, unsigned long long v) {
    __hip_atomic_fetch_max(reinterpret_cast<unsigned long long*>(row + w), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(kBlock) void k_png_fold(uint32_t n, const uint2* __restrict__ tsum, const uint4* __restrict__ fr,
                                                     uint32_t* own, uint32_t mask, uint32_t* acc,
                                                     uint32_t* __restrict__ row_of) {
    const uint32_t t = blockIdx.x;
    if (!png_tile_folds(tsum[t])) return;  // workgroup-uniform
    const uint32_t i = t * kPngTile + threadIdx.x;
    if (i >= n) return;
    const uint4 k = gld16(fr + 2 * (size_t)i);
    const uint32_t o = (k.y >> 24) & 0xfu, cls = k.y >> 28;
    uint32_t r = kPngNone;
    if (png_folds(o)) {
        uint32_t slot = kPngNone;
        const uint32_t row = png_insert(own, mask, fr, k, png_hash(k.w, k.x, k.y & 0xffffffu), i, slot);
        if (row != kPngNone) {
            uint32_t* a = acc + (size_t)row * kAccWords;
            if (slot != kPngNone) a[kAccSlot] = slot + 1;  // the claimer alone; read by the emit launch
            png_add(a, o == EMURX_PNG_REPLY ? kAccReply : o == EMURX_PNG_UNREACH ? kAccUnreach
                                                      : o == EMURX_PNG_NO_CLIENT ? kAccNoClient : kAccMcast);
            png_max(a, kAccNFirst, ~i);
            png_max(a, kAccLast, i);
            if (cls == kPngClsMalformed) png_add(a, kAccMalformed);
            if (cls == kPngClsBadLatency) png_add(a, kAccBadLat);
            if (cls == kPngClsOk) {
                const uint4 l = gld16(fr + 2 * (size_t)i + 1);
                const unsigned long long lat = (unsigned long long)l.y << 32 | l.x;
                png_add(a, kAccOk);
                png_max(a, kAccNFirstOk, ~i);
                png_max(a, kAccLastOk, i + 1);
                if (lat == 0) png_max(a, kAccLastZero, i + 1);
                else {
                    __hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(a + kAccLatSum), lat, __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT);
                    png_max64(a, kAccLatMax, lat);
                }
            }
            r = row | cls << kPngClsShift;
        }
    }
    row_of[i] = r;
}

// tcnt[t]: the tile's emitters | its marked frames << 16
__global__ __launch_bounds__(kBlock) void k_png_mark(uint32_t n, const uint2* __restrict__ tsum, const uint4* __restrict__ fr,
                                                     uint32_t* acc, uint32_t* __restrict__ row_of,
                                                     uint32_t* __restrict__ tcnt) {
    __shared__ uint32_t s_cnt;
    const uint32_t t = blockIdx.x;
    if (!png_tile_folds(tsum[t])) {  // workgroup-uniform
        if (threadIdx.x == 0) tcnt[t] = 0;
        return;
    }
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    const uint32_t i = t * kPngTile + threadIdx.x;
    bool emits = false, marked = false;
    if (i < n) {
        const uint32_t r = row_of[i];
        if (r != kPngNone) {
            uint32_t* a = acc + (size_t)(r & kPngRowMask) * kAccWords;
            emits = gld4(a + kAccLast) == i;
            if (((r >> kPngClsShift) & 3u) == kPngClsOk && gld4(a + kAccOk) > 1) {
                marked = true;
                if (i + 1 > gld4(a + kAccLastZero)) {  // behind the key's last zero latency
                    const uint4 l = gld16(fr + 2 * (size_t)i + 1);
                    png_max64(a, kAccNegMin, ~((unsigned long long)l.y << 32 | l.x));
                }
            }
            if (emits || marked) row_of[i] = r | (emits ? kPngEmits : 0u) | (marked ? kPngMarked : 0u);
        }
    }
    const uint32_t c = (uint32_t)__popcll(__ballot(emits)) | (uint32_t)__popcll(__ballot(marked)) << 16;
    if (lane_id() == 0 && c) atomicAdd(&s_cnt, c);
    __syncthreads();
    if (threadIdx.x == 0) tcnt[t] = s_cnt;
}

// info: {events written, distinct keys, overflow, frames with outcome 1..5}; then the ordered pass
__global__ __launch_bounds__(kPngScanBlock) void k_png_scan(uint32_t n, const uint2* __restrict__ tsum,
                                                            const uint32_t* __restrict__ tcnt, uint32_t ntiles,
                                                            uint32_t ev_cap, const uint4* __restrict__ fr,
                                                            const uint32_t* __restrict__ row_of, uint32_t* acc,
                                                            uint32_t* __restrict__ tord, unsigned long long* __restrict__ info) {
    __shared__ BlockScanLds<kPngScanBlock, uint32_t> s_scan;
    __shared__ uint32_t s_oc[5], s_marked;
    __shared__ uint32_t s_row[kPngScanBlock], s_seq[kPngScanBlock], s_next[kPngScanBlock];
    __shared__ uint32_t s_step[kPngStepWords];  // the steps that hold a marked frame
    __shared__ uint32_t s_wcnt[kPngScanBlock / kWave];
    const uint32_t tid = threadIdx.x;
    const uint32_t nwords = ((ntiles + kPngStepTiles - 1) / kPngStepTiles + 31) / 32;
    if (tid < 5) s_oc[tid] = 0;
    if (tid == 5) s_marked = 0;
    for (uint32_t w = tid; w < nwords; w += kPngScanBlock) s_step[w] = 0;
    __syncthreads();
    uint32_t base = 0, marked = 0, oc[5] = {0, 0, 0, 0, 0};
    for (uint32_t t0 = 0; t0 < ntiles; t0 += kPngScanBlock) {  // workgroup-uniform trip count
        const uint32_t t = t0 + tid;
        const uint2 v = t < ntiles ? tsum[t] : make_uint2(0, 0);
        const uint32_t tc = t < ntiles ? tcnt[t] : 0u, cnt = tc & 0xffffu;
        marked += tc >> 16;
        if (tc >> 16) atomicOr(&s_step[t / kPngStepTiles / 32], 1u << (t / kPngStepTiles % 32));
        oc[0] += v.x & 0x3ffu;
        oc[1] += (v.x >> 10) & 0x3ffu;
        oc[2] += v.x >> 20;
        oc[3] += v.y & 0x3ffu;
        oc[4] += v.y >> 10;
        uint32_t c = cnt;
        const auto [total] = block_incl_scan<kPngScanBlock>(s_scan, c);
        if (t < ntiles) tord[t] = base + c - cnt;
        base += total;
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const uint32_t s = wave_sum_u32(oc[k]);
        if (lane_id() == 0 && s) atomicAdd(&s_oc[k], s);
    }
    const uint32_t ms = wave_sum_u32(marked);
    if (lane_id() == 0 && ms) atomicAdd(&s_marked, ms);
    __syncthreads();
    if (tid < EMURX_PNG_INFO_WORDS) {
        const bool over = base > ev_cap;
        info[tid] = tid == 0 ? (over ? 0u : base) : tid == 1 ? base : tid == 2 ? (over ? 1u : 0u) : s_oc[tid - 3];
    }
    if (!s_marked) return;  // workgroup-uniform: no key has two accepted replies
    // ---- the ordered pass: kPngStepTiles tiles a step, in rx order, the steps with a marked frame
    // alone (workgroup-uniform: every lane reads the same words of the bitmap)
    for (uint32_t w = 0; w < nwords; ++w) {
        for (uint32_t bits = s_step[w]; bits; bits &= bits - 1) {
            const uint32_t t0 = (w * 32 + (uint32_t)__ffs((int)bits) - 1) * kPngStepTiles;
            const uint32_t i = t0 * kPngTile + tid, mt = t0 + tid / kPngTile;
            // row_of and fr are this call's only in a tile that folded: a tile without a marked frame
            // may hold an earlier call's words, marks included
            const bool mine = mt < ntiles && (tcnt[mt] >> 16) != 0;
            const uint32_t r = i < n && mine ? row_of[i] : kPngNone;
            const bool on = r != kPngNone && (r & kPngMarked);
            const uint32_t row = r & kPngRowMask, seq = on ? gld4(reinterpret_cast<const uint32_t*>(fr + 2 * (size_t)i) + 2) : 0u;
            // the step's marked frames, compacted in rx order: a frame looks back over those alone
            const unsigned long long bal = __ballot(on);
            if (lane_id() == 0) s_wcnt[tid / kWave] = (uint32_t)__popcll(bal);
            __syncthreads();
            uint32_t pos = mbcnt(bal);
            for (uint32_t v = 0; v < tid / kWave; ++v) pos += s_wcnt[v];
            if (on) {
                s_row[pos] = row;
                s_seq[pos] = seq;
                s_next[pos] = 0;
            }
            __syncthreads();
            uint32_t* a = acc + (size_t)row * kAccWords;
            if (on) {
                uint32_t prev = 0;  // seq + 1 of the predecessor; 0: none, the key's first accepted reply
                bool found = false;
                for (uint32_t q = pos; q-- > 0;)
                    if (s_row[q] == row) {
                        prev = s_seq[q] + 1;
                        s_next[q] = 1;  // q is not its row's last frame of this step
                        found = true;
                        break;
                    }
                // the carry: written by this workgroup in an earlier step, behind a barrier
                if (!found) prev = __hip_atomic_load(a + kAccCarry, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (prev && (prev & 0xffffu) == seq) png_add(a, kAccSucc);  // prev - 1 + 1 == seq mod 2^16
            }
            __syncthreads();
            if (on && !s_next[pos]) __hip_atomic_store(a + kAccCarry, seq + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(kBlock) void k_png_emit(uint32_t n, const uint2* __restrict__ tsum, const uint4* __restrict__ fr,
                                                     const uint32_t* __restrict__ row_of, const uint32_t* __restrict__ tord,
                                                     uint32_t* own, uint32_t* acc, uint32_t ev_cap,
                                                     const unsigned long long* __restrict__ info, uint2* __restrict__ ev) {
    __shared__ uint32_t s_w[kWaves];
    const uint32_t t = blockIdx.x;
    if (!png_tile_folds(tsum[t])) return;  // workgroup-uniform
    const bool over = info[2] != 0;
    const uint32_t i = t * kPngTile + threadIdx.x, lane = lane_id(), wv = threadIdx.x / kWave;
    const uint32_t r = i < n ? row_of[i] : kPngNone;
    const bool emits = r != kPngNone && (r & kPngEmits);
    const unsigned long long bal = __ballot(emits);
    if (lane == 0) s_w[wv] = (uint32_t)__popcll(bal);
    __syncthreads();
    if (!emits) return;
    uint32_t k = tord[t] + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
    for (uint32_t w = 0; w < wv; ++w) k += s_w[w];
    uint4* row = reinterpret_cast<uint4*>(acc + (size_t)(r & kPngRowMask) * kAccWords);
    uint32_t w[kAccWords];
#pragma unroll
    for (uint32_t j = 0; j < kAccWords / 4; ++j) {
        const uint4 v = gld16(row + j);
        w[4 * j] = v.x, w[4 * j + 1] = v.y, w[4 * j + 2] = v.z, w[4 * j + 3] = v.w;
        row[j] = make_uint4(0, 0, 0, 0);  // rows and slots are all zero again when the call ends
    }
    if (w[kAccSlot]) own[w[kAccSlot] - 1] = 0;
    if (over || k >= ev_cap) return;
    const uint4 key = gld16(fr + 2 * (size_t)i);  // the key's last frame is this one: the key is its own
    uint32_t sf = 0, sl = 0;
    unsigned long long mn = 0;
    if (w[kAccOk]) {
        sf = gld4(reinterpret_cast<const uint32_t*>(fr + 2 * (size_t)~w[kAccNFirstOk]) + 2);
        sl = gld4(reinterpret_cast<const uint32_t*>(fr + 2 * (size_t)(w[kAccLastOk] - 1)) + 2);
        const unsigned long long ng = (unsigned long long)w[kAccNegMin + 1] << 32 | w[kAccNegMin];
        // one accepted reply: its latency is the maximum
        mn = w[kAccOk] == 1 ? ((unsigned long long)w[kAccLatMax + 1] << 32 | w[kAccLatMax]) : ng ? ~ng : 0ull;
    }
    uint2* e = ev + 10 * (size_t)k;  // emurx_ping_ev
    e[0] = make_uint2(key.w, key.x);
    e[1] = make_uint2((key.y & 0xffffffu) | (w[kAccLastZero] ? 1u << 24 : 0u), ~w[kAccNFirst]);
    e[2] = make_uint2(w[kAccLast], w[kAccReply]);
    e[3] = make_uint2(w[kAccUnreach], w[kAccMalformed]);
    e[4] = make_uint2(w[kAccBadLat], w[kAccOk]);
    e[5] = make_uint2(w[kAccSucc], sf | sl << 16);
    e[6] = make_uint2(w[kAccLatSum], w[kAccLatSum + 1]);
    e[7] = make_uint2((uint32_t)mn, (uint32_t)(mn >> 32));
    e[8] = make_uint2(w[kAccLatMax], w[kAccLatMax + 1]);
    e[9] = make_uint2(w[kAccNoClient], w[kAccMcast]);
}

// A slot's ping stage to the host (emurx_ingest_set_ping): one launch behind emurx_ping_dev on the
// slot's stream reads the stage's counts on the device and copies, with 16-byte stores over the
// bus into the slot's pinned block (as k_ans_out does), the info words, the n outcome bytes and
// the events written, no more.  The regions start on 256-byte boundaries on both sides and hold
// whole 16-byte vectors; the event count is clamped to the pinned region's capacity (the host
// checks info[0] against the same capacity and fails the batch).
__global__ __launch_bounds__(kBlock) void k_png_out(const unsigned long long* __restrict__ info, const emurx_ping_ev* __restrict__ ev,
                                                    const uint8_t* __restrict__ outcome, uint32_t n, uint32_t ev_cap,
                                                    uint8_t* h_info, uint8_t* h_ev, uint8_t* h_outcome) {
    const uint64_t nev = min((uint64_t)info[0], (uint64_t)ev_cap);
    const uint64_t gid = (uint64_t)blockIdx.x * kBlock + threadIdx.x, gsz = (uint64_t)gridDim.x * kBlock;
    auto copy = [&](const void* src, void* dst, uint64_t bytes) {
        const uint64_t nv = (bytes + 15) >> 4;
        for (uint64_t v = gid; v < nv; v += gsz)
            reinterpret_cast<uint4*>(dst)[v] = gld16(reinterpret_cast<const uint4*>(src) + v);
    };
    copy(info, h_info, 8 * (uint64_t)EMURX_PNG_INFO_WORDS);
    copy(outcome, h_outcome, n);
    copy(ev, h_ev, nev * sizeof(emurx_ping_ev));
}

}  // namespace emurx

// scratch: the accumulator rows u32 [max_frames][24] (a key's row is its owner frame's), the
// frames' rows uint4 [max_frames][2], the set's owner words u32 [slots], then row indices u32
// [max_frames], tile sums uint2, tile counts u32 and tile ordinals u32 [tiles of max_frames].
// The accumulator rows and the owner words start, and every call leaves them, all zero.
struct PngScratch {
    uint32_t* acc;
    uint4* fr;
    uint32_t *own, *row_of;
    uint2* tsum;
    uint32_t *tcnt, *tord;
    size_t bytes;
};
static PngScratch png_scratch(void* base, uint32_t max_frames) {
    const size_t mt = ((size_t)max_frames + emurx::kPngTile - 1) / emurx::kPngTile;
    emurx_carver c(base);  // the initialisers run in order
    return {c.take<uint32_t>((size_t)max_frames * emurx::kAccWords), c.take<uint4>(2 * (size_t)max_frames),
            c.take<uint32_t>(emurx_lrn_slots(max_frames)), c.take<uint32_t>(max_frames), c.take<uint2>(mt),
            c.take<uint32_t>(mt), c.take<uint32_t>(mt), c.bytes()};
}
size_t emurx_png_scratch_bytes(uint32_t max_frames) { return png_scratch(nullptr, max_frames).bytes; }

int emurx_png_scratch_clear(void* scratch, uint32_t max_frames, hipStream_t st) {
    const PngScratch s = png_scratch(scratch, max_frames);
    return EMURX_HIP_OK(hipMemsetAsync(s.acc, 0, (size_t)max_frames * emurx::kAccWords * 4, st)) &&
                   EMURX_HIP_OK(hipMemsetAsync(s.own, 0, (size_t)emurx_lrn_slots(max_frames) * 4, st))
               ? 0
               : -1;
}

int emurx_launch_ping(const uint8_t* frames, const emurx_desc* desc, const emurx_rec* rec, uint32_t n, uint32_t fams,
                      uint64_t now_unix_ns, const emurx_dev_tables& T, emurx_ping_ev* ev, uint32_t ev_cap, uint8_t* outcome,
                      uint64_t* info, void* scratch, uint32_t max_frames, hipStream_t st) {
    using namespace emurx;
    unsigned long long* inf = reinterpret_cast<unsigned long long*>(info);
    if (n == 0) return EMURX_HIP_OK(hipMemsetAsync(inf, 0, 8 * (size_t)EMURX_PNG_INFO_WORDS, st)) ? 0 : -1;
    const uint32_t nt = (n + kPngTile - 1) / kPngTile;
    const PngScratch s = png_scratch(scratch, max_frames);  // sized by the handle's max_frames, not by n
    const uint32_t mask = emurx_lrn_slots(n) - 1;  // as the learning fold: at least twice the batch's frames
    hipError_t e = emurx_launch(k_png_decide, dim3(nt), dim3(kBlock), 0, st, frames, desc, rec, n, fams,
                                (unsigned long long)now_unix_ns, T, s.fr, s.tsum, outcome);
    if (e == hipSuccess) e = emurx_launch(k_png_fold, dim3(nt), dim3(kBlock), 0, st, n, s.tsum, s.fr, s.own, mask, s.acc, s.row_of);
    if (e == hipSuccess) e = emurx_launch(k_png_mark, dim3(nt), dim3(kBlock), 0, st, n, s.tsum, s.fr, s.acc, s.row_of, s.tcnt);
    if (e == hipSuccess)
        e = emurx_launch(k_png_scan, dim3(1), dim3(kPngScanBlock), 0, st, n, s.tsum, s.tcnt, nt, ev_cap, s.fr, s.row_of, s.acc,
                         s.tord, inf);
    if (e == hipSuccess)
        e = emurx_launch(k_png_emit, dim3(nt), dim3(kBlock), 0, st, n, s.tsum, s.fr, s.row_of, s.tord, s.own, s.acc, ev_cap, inf,
                         reinterpret_cast<uint2*>(ev));
    return EMURX_HIP_OK(e) ? 0 : -1;
}

int emurx_launch_ping_out(const uint64_t* info, const emurx_ping_ev* ev, const uint8_t* outcome, uint32_t n, uint32_t ev_cap,
                          uint8_t* h_info, uint8_t* h_ev, uint8_t* h_outcome, hipStream_t st) {
    using namespace emurx;
    // as k_ans_out: a workgroup per tile of the batch, at most 256
    const uint32_t g = std::min<uint32_t>(std::max<uint32_t>((n + kBlock - 1) / kBlock, 1), 256);
    return EMURX_HIP_OK(emurx_launch(k_png_out, dim3(g), dim3(kBlock), 0, st, reinterpret_cast<const unsigned long long*>(info), ev,
                                     outcome, n, ev_cap, h_info, h_ev, h_outcome))
               ? 0
               : -1;
}

// emurx_learn.hip — the ARP and ND cache learning of a classified batch, folded on the device
// (gfx950) into one event per distinct (Namespace, kind, IP, MAC): PluginArpNs.ArpLearn
// (src/emu/plugins/arp/arp.go:886-901, called from HandleRxArpPacket :904-946) and NdLearn
// (plugins/ipv6/nd.go:1611-1620 for a solicitation, :1687-1776 for an advertisement).  The rule
// with its citations is in include/emu_rx.h.  emurx_learn_dev, four launches:
//   k_lrn_decide   one frame per lane: the record's second half says whether the frame is a
//                  candidate (status OK; callback arp with the Namespace's plugin found, or
//                  callback icmpv6 at Namespace level; each only if `kinds` selects it); only a
//                  candidate's descriptor and header bytes are read.  A learning frame's key is
//                  seven words {ns, ip[4], mac, mac | kind << 16}.  A wave first folds its equal
//                  keys among its lanes (a batch is a few keys repeated: one ballot round per
//                  distinct key the wave holds), and the lowest lane of each group, its leader,
//                  alone goes to the set: it claims a slot by one compare-and-swap of the slot's
//                  owner word (0 -> frame index + 1 | five bits of the hash) or finds the slot
//                  whose owner's key equals its own; linear probing.  The owner's key is read from
//                  the owner's frame through that frame index: the frames are the call's input,
//                  which no kernel writes, so no multi-word key is ever published through the slot,
//                  there is no publish race and no atomic needs an ordering.  count, ~first and
//                  last of the group go in by atomicAdd / atomicMax on the slot (relaxed, agent
//                  scope; all three start from zero).  The highest lane of each group, the only
//                  one that can be the key's last frame, keeps the slot's index and its kind.
//   k_lrn_mark     the frame whose index equals its slot's `last` emits the event: the others
//                  drop their slot index; per 256-frame tile the count of emitters.
//   k_lrn_scan     one workgroup: exclusive scan of the tiles' emitters, the outcome counts,
//                  distinct keys against ev_cap, d_info.
//   k_lrn_emit     an emitter's event (the slot's count, first, last; the key from the emitter's own
//                  frame) goes to the tile's ordinal + its rank in the tile (frame order =
//                  ascending `last`), unless the batch overflows; either way the emitter
//                  zeroes its slot, so that the set is empty again when the call ends and no
//                  call pays for clearing slots it does not use.
// A batch without candidates costs the read of the records' second halves and one outcome byte
// per frame: the workgroups of the other passes leave after one 8-byte load.
#include <hip/hip_runtime.h>

#include "../../include/emu_rx.h"
#include "emurx_kernels.h"
#include "emurx_parse.h"
#include "emurx_rsp_dev.h"

namespace emurx {

constexpr uint32_t kLrnTile = EMURX_QUEUE_TILE;  // frames per workgroup, one per lane
static_assert(kLrnTile == kBlock, "one frame per lane of a 256-lane workgroup");
constexpr uint32_t kLrnScanBlock = 1024;
constexpr uint32_t kLrnNone = 0xffffffffu;
constexpr uint32_t kLrnLdsSlots = 2 * kBlock;  // the workgroup-level set
constexpr uint32_t kLrnKindShift = 28, kLrnSlotMask = (1u << kLrnKindShift) - 1;  // a slot index | kind << 28

// a frame's key: ns, the IP (ARP: the IPv4 address in ip[0], zeros behind it), the MAC's bytes
// 0..3, its bytes 4..5 | kind << 16 (the event's last word as it is written)
struct LrnKey {
    uint32_t ns, ip[4], mlo, mhk;
};
struct LrnPlan {
    uint32_t outcome;
    LrnKey k;
};
__device__ __forceinline__ LrnPlan lrn_plan(uint32_t outcome) { return {outcome, {0, {0, 0, 0, 0}, 0, 0}}; }
__device__ __forceinline__ bool lrn_learns(uint32_t outcome) { return outcome >= EMURX_LRN_ARP_REQ && outcome <= EMURX_LRN_ND_NA; }
__device__ __forceinline__ uint32_t lrn_hash(const LrnKey& k) {  // emurx_tables.h: the host calls it too
    return emurx_lrn_hash(k.ns, k.ip[0], k.ip[1], k.ip[2], k.ip[3], k.mlo, k.mhk);
}

// The record's words: as in emurx_respond.hip
__device__ __forceinline__ uint32_t lrn_lk(const uint4& b) { return (b.w >> (8 + EMURX_FLAG_LK_SHIFT)) & 7u; }
template <bool kNd>  // kNd: kinds has EMURX_LRNK_ND
__device__ __forceinline__ bool lrn_candidate(const uint4& b, uint32_t kinds) {
    const uint32_t proto = b.z >> 24, status = b.w & 0xff, lk = lrn_lk(b);
    if (status != EMURX_ST_OK) return false;
    // the Namespace exists and has the arp plugin (arp.go:956-969): every lookup from NS_LEVEL up
    if (proto == EMURX_CB_ARP) return (kinds & EMURX_LRNK_ARP) && lk >= EMURX_LK_NS_LEVEL;
    return kNd && proto == EMURX_CB_ICMPV6 && lk == EMURX_LK_NS_LEVEL;
}

// ARP (arp.go:904-946): a request is learned before its target is looked up, a reply unless it
// came to the broadcast address; the key is the sender's protocol and hardware address
__device__ LrnPlan lrn_decide_arp(const uint8_t* __restrict__ frames, const emurx_desc& d, const uint4& a, const uint4& b) {
    const uint32_t l3 = b.x >> 16, len = d.len;
    const uint8_t* f = frames + d.off;
    if (d.pad == EMURX_DESC_HOLE) return lrn_plan(EMURX_LRN_NONE);
    if (l3 < 14 || l3 + 28 > len) return lrn_plan(EMURX_LRN_HOST);
    uint32_t w[4];  // p[l3 + 6 ..]: the operation, the sender's hardware address (6), its IP (4)
    rsp_load16((uintptr_t)f, len, (int)(l3 + 6), w);
    const uint32_t op = __builtin_bswap32(w[0]) >> 16;
    uint32_t kind = EMURX_LRN_ARP_REQ;
    if (op == 2) {
        uint32_t e[4];
        rsp_load16((uintptr_t)f, len, 0, e);
        if (e[0] == 0xffffffffu && (e[1] & 0xffffu) == 0xffffu) return lrn_plan(EMURX_LRN_NONE);  // pktRxErrNoBroadcast
        kind = EMURX_LRN_ARP_REPLY;
    } else if (op != 1) {
        return lrn_plan(EMURX_LRN_NONE);  // pktRxErrWrongOp
    }
    return {kind, {a.x, {w[2], 0, 0, 0}, w[0] >> 16 | w[1] << 16, w[1] >> 16 | kind << 16}};
}

// ND (nd.go:1546-1620, 1687-1776).  A solicitation: the responder's own checks, then the source
// is learned if it is global, came with its link-layer address and is no client's of this
// Namespace.  An advertisement: the target is learned from an override with a target
// link-layer address, unless it is one of this Namespace's clients' own.
__device__ LrnPlan lrn_decide_nd(const uint8_t* __restrict__ frames, const emurx_desc& d, const uint4& a, const uint4& b,
                                 const emurx_dev_tables& T) {
    const uint32_t l3 = b.x >> 16, l4 = b.y & 0xffffu, len = d.len;
    const uint8_t* f = frames + d.off;
    if (d.pad == EMURX_DESC_HOLE) return lrn_plan(EMURX_LRN_NONE);
    if (l3 < 14 || l3 + 40 > l4 || l4 + 4 > len) return lrn_plan(EMURX_LRN_HOST);
    const uint32_t type = gld1(f + l4);
    if (gld1(f + l4 + 1) != 0 || (type != 135 && type != 136)) return lrn_plan(EMURX_LRN_NONE);
    const uint32_t tk = emurx_tk_hash(b.x & 0xffffu, a.z, a.w);
    if (type == 135)
        return rsp_nd_checks(  // the responder's own (emurx_rsp_dev.h), its HOST included
            f, l3, l4, len, [](uint32_t o) { return lrn_plan(o == EMURX_RSP_HOST ? EMURX_LRN_HOST : EMURX_LRN_NONE); },
            [&](const uint32_t(&)[4], bool slla, uint2 mac, const uint32_t(&src)[4]) -> LrnPlan {
                if (!slla || !ip6_global(src)) return lrn_plan(EMURX_LRN_NONE);
                const uint32_t bk = emurx_ip6_hash(tk, src[0], src[1], src[2], src[3]) & T.ip6_mask;
                if (resolve_ip6(T, bk, ld_bucket(T.ip6_tab, bk), a.x, src).cid != EMURX_ID_NONE)
                    return lrn_plan(EMURX_LRN_NONE);  // our own address
                return {EMURX_LRN_ND_NS, {a.x, {src[0], src[1], src[2], src[3]}, mac.x, mac.y | EMURX_LRN_ND_NS << 16}};
            });
    uint32_t w[4];
    if (len - (l4 + 4) < 20) return lrn_plan(EMURX_LRN_NONE);  // pktRxErrTooShort
    const uint32_t nopt = len - (l4 + 24);
    if (nopt > 8) return lrn_plan(EMURX_LRN_HOST);  // a lane walks no option chain
    if (nopt != 8) return lrn_plan(EMURX_LRN_NONE);  // no target link-layer address, or a truncated option
    const uintptr_t F = (uintptr_t)f;
    rsp_load16(F, len, (int)(l4 + 24), w);
    if ((w[0] & 0xffffu) != 0x0102u) return lrn_plan(EMURX_LRN_NONE);
    const uint32_t mlo = w[0] >> 16 | w[1] << 16, mhi = w[1] >> 16;  // a zero MAC is learned: no check in :1710-1724
    if (gld1(f + l3 + 7) != 255) return lrn_plan(EMURX_LRN_NONE);
    if (!(gld1(f + l4 + 4) & 0x20u)) return lrn_plan(EMURX_LRN_NONE);  // no override
    rsp_load16(F, len, (int)(l4 + 8), w);  // the target
    if (!(ip6_link_local(w) || ip6_global(w))) return lrn_plan(EMURX_LRN_NONE);
    if (rsp_nd_eui(w)) {
        uint2 m;
        if (rsp_nd_eui_client(T, a.x, tk, w, m).x != EMURX_ID_NONE) return lrn_plan(EMURX_LRN_NONE);  // ours
    } else {
        const uint32_t bk = emurx_ip6_hash(tk, w[0], w[1], w[2], w[3]) & T.ip6_mask;
        if (resolve_ip6(T, bk, ld_bucket(T.ip6_tab, bk), a.x, w).cid != EMURX_ID_NONE) return lrn_plan(EMURX_LRN_NONE);  // pktRxNeighborAdvWithOwnAddr
    }
    return {EMURX_LRN_ND_NA, {a.x, {w[0], w[1], w[2], w[3]}, mlo, mhi | EMURX_LRN_ND_NA << 16}};
}

__device__ __forceinline__ uint32_t lrn_bcast(uint32_t v, uint32_t lane) {  // lane: wave-uniform
    return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)lane);
}
// The key of frame j, a learning frame of this batch, read as a key of `kind`: false when the
// frame is of another kind (its key differs then, whatever its bytes).  A frame that learns has
// passed the bounds checks of its own kind, so the offsets fit where the kind is its own; the
// spans are read within the frame's bounds regardless (rsp_load16).
__device__ __forceinline__ bool lrn_key_at(const uint8_t* __restrict__ frames, const emurx_desc* __restrict__ desc,
                                           const emurx_rec* __restrict__ rec, uint32_t j, uint32_t kind, LrnKey& k) {
    const uint4 a = gld16(reinterpret_cast<const uint4*>(rec + j)), b = gld16(reinterpret_cast<const uint4*>(rec + j) + 1);
    const emurx_desc d = desc[j];
    const uint32_t proto = b.z >> 24, l3 = b.x >> 16, l4 = b.y & 0xffffu, len = d.len;
    const uintptr_t F = (uintptr_t)(frames + d.off);
    uint32_t w[4], o[4];
    if (kind <= EMURX_LRN_ARP_REPLY) {
        if (proto != EMURX_CB_ARP) return false;
        rsp_load16(F, len, (int)(l3 + 6), w);
        if ((__builtin_bswap32(w[0]) >> 16) != kind) return false;  // the operation is the kind
        k = {a.x, {w[2], 0, 0, 0}, w[0] >> 16 | w[1] << 16, w[1] >> 16 | kind << 16};
        return true;
    }
    if (proto != EMURX_CB_ICMPV6 || l4 >= len || gld1(frames + d.off + l4) != (kind == EMURX_LRN_ND_NS ? 135u : 136u)) return false;
    rsp_load16(F, len, (int)(kind == EMURX_LRN_ND_NS ? l3 + 8 : l4 + 8), w);  // the source, or the target
    rsp_load16(F, len, (int)(l4 + 24), o);                                    // the option
    k = {a.x, {w[0], w[1], w[2], w[3]}, o[0] >> 16 | o[1] << 16, o[1] >> 16 | kind << 16};
    return true;
}

// The slot of key k (hash h, kind `kind`) in the set of mask + 1 slots {owner, count, ~first,
// last}, owner = frame + 1 | the hash's top five bits << 27 (n < 2^26): claimed for frame i by
// one compare-and-swap of the owner word, or found: the tag says whether the owner's key is worth
// reading, and the key is read from the owner's frame, which nobody writes.  Nothing but the
// owner word is published, so the atomics need no ordering (relaxed, agent scope).  The batch's
// part of the set has at least twice as many slots as the batch has frames, so a free slot always
// ends the probe; the trip count is bounded all the same.
__device__ __forceinline__ uint32_t lrn_insert(uint4* slots, uint32_t mask, const uint8_t* __restrict__ frames,
                                               const emurx_desc* __restrict__ desc, const emurx_rec* __restrict__ rec,
                                               const LrnKey& k, uint32_t h, uint32_t i, bool& claimed) {
    const uint32_t mine = (i + 1) | (h >> 27) << 27, kind = k.mhk >> 16;
    claimed = false;
    for (uint32_t p = h & mask, t = 0; t <= mask; p = (p + 1) & mask, ++t) {
        uint32_t* own = reinterpret_cast<uint32_t*>(slots + p);
        uint32_t cur = __hip_atomic_load(own, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == 0 && __hip_atomic_compare_exchange_strong(own, &cur, mine, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                             __HIP_MEMORY_SCOPE_AGENT)) {
            claimed = true;
            return p;
        }
        if ((cur ^ mine) >> 27) continue;  // another hash
        LrnKey o;
        if (lrn_key_at(frames, desc, rec, (cur & 0x7ffffffu) - 1, kind, o) && o.ns == k.ns && o.ip[0] == k.ip[0] &&
            o.ip[1] == k.ip[1] && o.ip[2] == k.ip[2] && o.ip[3] == k.ip[3] && o.mlo == k.mlo && o.mhk == k.mhk)
            return p;
    }
    return kLrnNone;
}

// tile sums: x = ARP_REQ | ARP_REPLY << 10 | ND_NS << 20, y = ND_NA | HOST << 10 (each <= 256)
__device__ __forceinline__ uint32_t lrn_tile_learners(const uint2& ts) {
    return (ts.x & 0x3ffu) + ((ts.x >> 10) & 0x3ffu) + (ts.x >> 20) + (ts.y & 0x3ffu);
}

template <bool kNd>
__global__ __launch_bounds__(kBlock) void k_lrn_decide(const uint8_t* __restrict__ frames, const emurx_desc* __restrict__ desc,
                                                       const emurx_rec* __restrict__ rec, uint32_t n, uint32_t kinds,
                                                       const emurx_dev_tables T, uint4* slots, uint32_t mask,
                                                       uint32_t* __restrict__ slot_of,
                                                       uint2* __restrict__ tsum, uint8_t* __restrict__ outcome) {
    __shared__ uint32_t s_sum[3];  // the tile sums, and the waves' leaders
    __shared__ uint32_t s_own[kLrnLdsSlots];  // the workgroup's set: owner lane + 1, 0 free
    __shared__ uint32_t s_k[8][kBlock];       // a wave leader's key and its hash, by lane
    __shared__ uint32_t s_agg[3][kBlock];     // count, ~first, last of the keys an owner lane holds
    __shared__ uint32_t s_slot[kBlock];       // its slot in the global set
    if (threadIdx.x < 3) s_sum[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t i = blockIdx.x * kLrnTile + threadIdx.x, lane = lane_id();
    LrnPlan p = lrn_plan(EMURX_LRN_NONE);
    if (i < n) {
        const uint4 b = gld16(reinterpret_cast<const uint4*>(rec + i) + 1);
        if (lrn_candidate<kNd>(b, kinds)) {
            const uint4 a = gld16(reinterpret_cast<const uint4*>(rec + i));
            if (!kNd || (b.z >> 24) == EMURX_CB_ARP) p = lrn_decide_arp(frames, desc[i], a, b);
            else p = lrn_decide_nd(frames, desc[i], a, b, T);
        }
        if (outcome) outcome[i] = (uint8_t)p.outcome;
    }
    const uint32_t o = p.outcome;
    const bool learns = lrn_learns(o);
    const uint32_t cx = wave_sum_u32((o == EMURX_LRN_ARP_REQ ? 1u : 0u) | (o == EMURX_LRN_ARP_REPLY ? 1u << 10 : 0u) |
                                     (o == EMURX_LRN_ND_NS ? 1u << 20 : 0u));
    const uint32_t cy = wave_sum_u32((o == EMURX_LRN_ND_NA ? 1u : 0u) | (o == EMURX_LRN_HOST ? 1u << 10 : 0u));
    if (lane == 0 && (cx | cy)) {
        atomicAdd(&s_sum[0], cx);
        atomicAdd(&s_sum[1], cy);
    }
    // ---- the wave's equal keys fold among its lanes: one round per distinct key
    uint32_t h = 0, leader = lane, cnt = 0, top = lane;
    unsigned long long pend = __ballot(learns);
    if (pend) {  // wave-uniform
        h = lrn_hash(p.k);
        while (pend) {
            const uint32_t L = (uint32_t)__ffsll((long long)pend) - 1u;
            // every broadcast is issued by the whole wave: no short circuit
            const uint32_t ne = (h ^ lrn_bcast(h, L)) | (p.k.ns ^ lrn_bcast(p.k.ns, L)) | (p.k.ip[0] ^ lrn_bcast(p.k.ip[0], L)) |
                                (p.k.ip[1] ^ lrn_bcast(p.k.ip[1], L)) | (p.k.ip[2] ^ lrn_bcast(p.k.ip[2], L)) |
                                (p.k.ip[3] ^ lrn_bcast(p.k.ip[3], L)) | (p.k.mlo ^ lrn_bcast(p.k.mlo, L)) |
                                (p.k.mhk ^ lrn_bcast(p.k.mhk, L));
            const bool eq = learns && ne == 0;
            const unsigned long long m = __ballot(eq) & pend;  // holds L
            const uint32_t hi = 63u - (uint32_t)__clzll((long long)m);
            if ((m >> lane) & 1ull) {
                leader = L;
                top = hi;
            }
            if (lane == L) cnt = (uint32_t)__popcll(m);
            pend &= ~m;
        }
    }
    const bool lead = learns && leader == lane;
    const uint32_t nlead = (uint32_t)__popcll(__ballot(lead));
    if (lane == 0 && nlead) atomicAdd(&s_sum[2], nlead);
    __syncthreads();
    const uint2 ts = make_uint2(s_sum[0], s_sum[1]);
    if (threadIdx.x == 0) tsum[blockIdx.x] = ts;
    if (!lrn_tile_learners(ts)) return;  // workgroup-uniform: a tile that learns nothing is done
    const uint32_t tid = threadIdx.x;
    uint32_t bown = tid;  // the lane that takes this leader's key to the global set
    uint32_t acnt = cnt, anf = ~i, ala = i + (top - lane);  // the group's count, ~first (the leader is its first), last
    // ---- where the waves folded at least half of their frames away, keys repeat: the waves'
    // leaders then fold among the workgroup too, in a set in LDS built like the global one (an
    // owner word per slot, the owner's key in its own row of s_k), so that one lane per distinct
    // key of the tile goes to the global set: a quarter of the atomics on a hot slot.  A tile of
    // distinct keys would only pay the barriers (workgroup-uniform choice).
    const bool fold = 2 * s_sum[2] <= lrn_tile_learners(ts);
    if (fold) {
        for (uint32_t j = tid; j < kLrnLdsSlots; j += kBlock) s_own[j] = 0;
        if (lead) {
            s_k[0][tid] = p.k.ns;
            s_k[1][tid] = p.k.ip[0];
            s_k[2][tid] = p.k.ip[1];
            s_k[3][tid] = p.k.ip[2];
            s_k[4][tid] = p.k.ip[3];
            s_k[5][tid] = p.k.mlo;
            s_k[6][tid] = p.k.mhk;
            s_k[7][tid] = h;
            s_agg[0][tid] = s_agg[1][tid] = s_agg[2][tid] = 0;
        }
        __syncthreads();
        if (lead) {
            for (uint32_t q = (h >> 9) & (kLrnLdsSlots - 1), t = 0; t < kLrnLdsSlots; q = (q + 1) & (kLrnLdsSlots - 1), ++t) {
                const uint32_t cur = atomicCAS(&s_own[q], 0u, tid + 1);
                if (cur == 0) break;  // claimed (twice as many slots as lanes: a free one always ends the probe)
                const uint32_t c = cur - 1;
                if (s_k[7][c] == h && s_k[0][c] == p.k.ns && s_k[1][c] == p.k.ip[0] && s_k[2][c] == p.k.ip[1] &&
                    s_k[3][c] == p.k.ip[2] && s_k[4][c] == p.k.ip[3] && s_k[5][c] == p.k.mlo && s_k[6][c] == p.k.mhk) {
                    bown = c;
                    break;
                }
            }
            atomicAdd(&s_agg[0][bown], acnt);
            atomicMax(&s_agg[1][bown], anf);
            atomicMax(&s_agg[2][bown], ala);
        }
        __syncthreads();
        if (lead && bown == tid) {
            acnt = s_agg[0][tid];
            anf = s_agg[1][tid];
            ala = s_agg[2][tid];
        }
    }
    uint32_t slot = kLrnNone;
    if (lead && bown == tid) {
        bool claimed;
        slot = lrn_insert(slots, mask, frames, desc, rec, p.k, h, i, claimed);
        if (slot != kLrnNone) {
            uint32_t* s = reinterpret_cast<uint32_t*>(slots + slot);
            __hip_atomic_fetch_add(s + 1, acnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            // ~first and last only grow, so a value read earlier that already covers ours still
            // does: a found slot (a key that repeats) is read once, and most groups then have
            // nothing to add but their count; a slot just claimed takes both without a read
            unsigned long long fl = 0;
            if (!claimed)
                fl = __hip_atomic_load(reinterpret_cast<unsigned long long*>(s + 2), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if ((uint32_t)fl < anf) __hip_atomic_fetch_max(s + 2, anf, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if ((uint32_t)(fl >> 32) < ala || claimed) __hip_atomic_fetch_max(s + 3, ala, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if (fold) {
        if (lead && bown == tid) s_slot[tid] = slot;
        __syncthreads();
        if (lead) slot = s_slot[bown];
    }
    // the highest lane of a wave's group alone can be its key's last frame: it keeps the slot
    slot = (uint32_t)__shfl((int)slot, (int)leader);
    if (!learns || top != lane) slot = kLrnNone;
    else if (slot != kLrnNone) slot |= o << kLrnKindShift;  // the emit pass reads the key as this kind
    // the slot indices are read by the later passes of tiles that learn only
    if (i < n) slot_of[i] = slot;
}

// the emitters: per tile their count; every other frame drops its slot index
__global__ __launch_bounds__(kBlock) void k_lrn_mark(const uint4* __restrict__ slots, uint32_t n,
                                                     const uint2* __restrict__ tsum, uint32_t* __restrict__ slot_of,
                                                     uint32_t* __restrict__ tcnt) {
    __shared__ uint32_t s_cnt;
    const uint32_t t = blockIdx.x;
    if (!lrn_tile_learners(tsum[t])) {  // workgroup-uniform
        if (threadIdx.x == 0) tcnt[t] = 0;
        return;
    }
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    const uint32_t i = t * kLrnTile + threadIdx.x;
    bool emits = false;
    if (i < n) {
        const uint32_t s = slot_of[i];
        if (s != kLrnNone) {
            emits = gld4(reinterpret_cast<const uint32_t*>(slots + (s & kLrnSlotMask)) + 3) == i;
            if (!emits) slot_of[i] = kLrnNone;
        }
    }
    const uint32_t c = (uint32_t)__popcll(__ballot(emits));
    if (lane_id() == 0 && c) atomicAdd(&s_cnt, c);
    __syncthreads();
    if (threadIdx.x == 0) tcnt[t] = s_cnt;
}

// info: {events written, distinct keys, overflow, frames with outcome 1..5}
__global__ __launch_bounds__(kLrnScanBlock) void k_lrn_scan(const uint2* __restrict__ tsum, const uint32_t* __restrict__ tcnt,
                                                            uint32_t ntiles, uint32_t ev_cap, uint32_t* __restrict__ tord,
                                                            unsigned long long* __restrict__ info) {
    __shared__ BlockScanLds<kLrnScanBlock, uint32_t> s_scan;
    __shared__ uint32_t s_oc[5];
    if (threadIdx.x < 5) s_oc[threadIdx.x] = 0;
    uint32_t base = 0, oc[5] = {0, 0, 0, 0, 0};
    for (uint32_t t0 = 0; t0 < ntiles; t0 += kLrnScanBlock) {  // workgroup-uniform trip count
        const uint32_t t = t0 + threadIdx.x;
        const uint2 v = t < ntiles ? tsum[t] : make_uint2(0, 0);
        const uint32_t cnt = t < ntiles ? tcnt[t] : 0u;
        oc[0] += v.x & 0x3ffu;
        oc[1] += (v.x >> 10) & 0x3ffu;
        oc[2] += v.x >> 20;
        oc[3] += v.y & 0x3ffu;
        oc[4] += v.y >> 10;
        uint32_t c = cnt;
        const auto [total] = block_incl_scan<kLrnScanBlock>(s_scan, c);
        if (t < ntiles) tord[t] = base + c - cnt;
        base += total;
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const uint32_t s = wave_sum_u32(oc[k]);
        if (lane_id() == 0 && s) atomicAdd(&s_oc[k], s);
    }
    __syncthreads();
    if (threadIdx.x < EMURX_LRN_INFO_WORDS) {
        const uint32_t k = threadIdx.x;
        const bool over = base > ev_cap;
        info[k] = k == 0 ? (over ? 0u : base) : k == 1 ? base : k == 2 ? (over ? 1u : 0u) : s_oc[k - 3];
    }
}

__global__ __launch_bounds__(kBlock) void k_lrn_emit(const uint8_t* __restrict__ frames, const emurx_desc* __restrict__ desc,
                                                     const emurx_rec* __restrict__ rec, uint4* slots, uint32_t n,
                                                     const uint2* __restrict__ tsum, const uint32_t* __restrict__ slot_of,
                                                     const uint32_t* __restrict__ tord, uint32_t ev_cap,
                                                     const unsigned long long* __restrict__ info, uint2* __restrict__ ev) {
    __shared__ uint32_t s_w[kWaves];
    const uint32_t t = blockIdx.x;
    if (!lrn_tile_learners(tsum[t])) return;  // workgroup-uniform
    const bool over = info[2] != 0;
    const uint32_t i = t * kLrnTile + threadIdx.x, lane = lane_id(), wv = threadIdx.x / kWave;
    const uint32_t sk = i < n ? slot_of[i] : kLrnNone;
    const bool emits = sk != kLrnNone;
    const unsigned long long bal = __ballot(emits);
    if (lane == 0) s_w[wv] = (uint32_t)__popcll(bal);
    __syncthreads();
    if (!emits) return;
    uint32_t k = tord[t] + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
    for (uint32_t w = 0; w < wv; ++w) k += s_w[w];
    const uint32_t s = sk & kLrnSlotMask;
    const uint4 v = gld16(slots + s);
    slots[s] = make_uint4(0, 0, 0, 0);  // the set is empty again when the call ends
    if (over || k >= ev_cap) return;
    LrnKey key;  // the key's last frame is this one: the key is its own
    if (!lrn_key_at(frames, desc, rec, i, sk >> kLrnKindShift, key)) return;
    uint2* e = ev + 5 * (size_t)k;  // emurx_learn_ev: ns, count, first, last, ip[16], mac[6], kind, pad
    e[0] = make_uint2(key.ns, v.y);
    e[1] = make_uint2(~v.z, v.w);
    e[2] = make_uint2(key.ip[0], key.ip[1]);
    e[3] = make_uint2(key.ip[2], key.ip[3]);
    e[4] = make_uint2(key.mlo, key.mhk);
}

}  // namespace emurx

// scratch: the set uint4 [slots], then slot indices u32 [max_frames], tile sums uint2, tile
// emitters u32 and tile ordinals u32 [tiles of max_frames].  The set starts, and every call
// leaves it, all zero.
uint32_t emurx_lrn_slots(uint32_t max_frames) {
    uint32_t s = 128;
    while (s < 2ull * max_frames && s < (1u << 27)) s <<= 1;
    return s;
}
struct LrnScratch {
    uint4* slots;
    uint32_t* slot_of;
    uint2* tsum;
    uint32_t *tcnt, *tord;
    size_t bytes;
};
static LrnScratch lrn_scratch(void* base, uint32_t max_frames) {
    const size_t mt = ((size_t)max_frames + emurx::kLrnTile - 1) / emurx::kLrnTile;
    emurx_carver c(base);  // the initialisers run in order; the set (a power of two >= 2 KiB) takes no padding
    return {c.take<uint4>(emurx_lrn_slots(max_frames)), c.take<uint32_t>(max_frames), c.take<uint2>(mt),
            c.take<uint32_t>(mt), c.take<uint32_t>(mt), c.bytes()};
}
size_t emurx_lrn_scratch_bytes(uint32_t max_frames) { return lrn_scratch(nullptr, max_frames).bytes; }

int emurx_launch_learn(const uint8_t* frames, const emurx_desc* desc, const emurx_rec* rec, uint32_t n, uint32_t kinds,
                       const emurx_dev_tables& T, emurx_learn_ev* ev, uint32_t ev_cap, uint8_t* outcome, uint64_t* info,
                       void* scratch, uint32_t max_frames, hipStream_t st) {
    using namespace emurx;
    unsigned long long* inf = reinterpret_cast<unsigned long long*>(info);
    if (n == 0) return EMURX_HIP_OK(hipMemsetAsync(inf, 0, 8 * (size_t)EMURX_LRN_INFO_WORDS, st)) ? 0 : -1;
    const uint32_t nt = (n + kLrnTile - 1) / kLrnTile;
    const LrnScratch s = lrn_scratch(scratch, max_frames);  // sized by the handle's max_frames, not by n
    // the slots this batch probes: a power of two, at least twice its frames (never full), so a
    // small batch's keys stay within a few cache lines of a large handle's set
    const uint32_t mask = emurx_lrn_slots(n) - 1;
    const auto decide = (kinds & EMURX_LRNK_ND) ? k_lrn_decide<true> : k_lrn_decide<false>;
    hipError_t e = emurx_launch(decide, dim3(nt), dim3(kBlock), 0, st, frames, desc, rec, n, kinds, T, s.slots, mask,
                                s.slot_of, s.tsum, outcome);
    if (e == hipSuccess) e = emurx_launch(k_lrn_mark, dim3(nt), dim3(kBlock), 0, st, s.slots, n, s.tsum, s.slot_of, s.tcnt);
    if (e == hipSuccess)
        e = emurx_launch(k_lrn_scan, dim3(1), dim3(kLrnScanBlock), 0, st, s.tsum, s.tcnt, nt, ev_cap, s.tord, inf);
    if (e == hipSuccess)
        e = emurx_launch(k_lrn_emit, dim3(nt), dim3(kBlock), 0, st, frames, desc, rec, s.slots, n, s.tsum, s.slot_of,
                         s.tord, ev_cap, inf, reinterpret_cast<uint2*>(ev));
    return EMURX_HIP_OK(e) ? 0 : -1;
}

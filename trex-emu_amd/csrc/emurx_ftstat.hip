// emurx_ftstat.hip — the TCP / UDP frames of a classified batch that the transport plugin refuses,
// folded on the device (gfx950) into one event per client: what HandleRxTransPacket
// (src/emu/plugins/transport/plugin_transport.go:74-128) -> TransportCtx.handleRxPacket
// (client_ctx.go:912-969) -> handleRxTcpNewFlow / handleRxUdpNewFlow (:829-906) add to ftStats
// (:158-197) for a frame that reaches no socket.  The rule with its citations is in
// include/emu_rx.h.  emurx_ftstat_dev, four launches:
//   k_ft_fold   one frame per lane.  The record's second half says whether the frame is a
//               candidate; a candidate's descriptor, the record's first half and, for lookup
//               CLIENT, its flow word decide; only an outcome 1..3 reads its one frame byte (the
//               family).  The lanes of a wave that hold one client are combined first: one
//               iteration of ballots per distinct client present, and the group's first lane (its
//               lowest frame) alone touches memory.  It claims a slot of the set by one
//               compare-and-swap of the slot's owner word (0 -> frame index + 1 | five bits of the
//               hash), as the learning and ping folds do, or finds the slot whose owner's client
//               equals its own: the owner's key is rec[owner].client_id, which the classify wrote,
//               so nothing but the owner word is published and no atomic needs an ordering.  The
//               client's accumulator is the row of its owner frame (acc[owner]): the group's
//               counts go in by two 64-bit adds, ~first and last by two maxima, all relaxed at
//               agent scope and all starting from zero.  A flood on one client is four atomics a
//               wave, not four a frame.
//   k_ft_mark   the frame whose index equals its row's `last` emits the event; per tile the emitters.
//   k_ft_scan   one workgroup: the exclusive scan of the tiles' emitters, the outcome counts,
//               distinct clients against ev_cap, d_info.
//   k_ft_emit   an emitter's event goes to the tile's ordinal + its rank in the tile (frame order =
//               ascending `last`), unless the batch overflows; either way the emitter zeroes its
//               row and its slot, so that the scratch is as the call found it.
//   (k_ft_out   a slot's flow stage only, emurx_ingest_set_flows: the results into pinned memory)
// A batch without a refused frame costs the read of the records' second halves, of the candidates'
// descriptors, first halves and flow words and one outcome byte per frame: the workgroups of the
// other passes leave after one 8-byte load.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/emu_rx.h"
#include "emurx_kernels.h"
#include "emurx_wave.h"

namespace emurx {

constexpr uint32_t kFtTile = EMURX_QUEUE_TILE;  // frames per workgroup, one per lane
static_assert(kFtTile == kBlock, "one frame per lane of a 256-lane workgroup");
static_assert(sizeof(emurx_ft_ev) == 48 && EMURX_FTC_WORDS == 7, "k_ft_emit writes six 8-byte words");
constexpr uint32_t kFtScanBlock = 1024;
constexpr uint32_t kFtNone = 0xffffffffu;
constexpr uint32_t kFtEmits = 1u << 31;  // row_of[i]: the frame's row | emits << 31; rows are below 2^26
// an accumulator row, 8 words, 32-byte aligned: two 64-bit words, then four 32-bit ones
enum : uint32_t {
    kFtAccA = 0,    // u64: NO_SYN frames | NO_SRV_TCP frames << 32
    kFtAccB = 2,    // u64: NO_SRV_UDP frames | IPv6 frames << 32
    kFtNFirst = 4,  // ~first
    kFtLast = 5,
    kFtSlot = 6,    // the client's slot in the set + 1: the claimer's store
    kFtAccWords = 8
};

// The record's second half: {vport | l3 << 16, l4 | l7 << 16, l7_len | next_hdr << 16 | proto << 24,
// status | flags << 8 | rsv << 16}
__device__ __forceinline__ uint32_t ft_lk(const uint4& b) { return (b.w >> (8 + EMURX_FLAG_LK_SHIFT)) & 7u; }
__device__ __forceinline__ bool ft_rec_candidate(const uint4& b) {
    const uint32_t proto = b.z >> 24;
    return (b.w & 0xff) == EMURX_ST_OK && (proto == EMURX_CB_TCP || proto == EMURX_CB_UDP);
}

// The outcome byte of a candidate (status OK, tcp / udp callback, no hole); cid, ns: the record's
__device__ uint32_t ft_decide(const uint8_t* __restrict__ frames, const emurx_desc& d, const uint4& b, uint32_t ns,
                              uint32_t cid, const uint32_t* __restrict__ flow, uint32_t i, uint32_t max_ns,
                              uint32_t max_clients) {
    const uint32_t lk = ft_lk(b);
    // plugin_transport.go:74-128: the handler would only return PARSER_ERR
    if (lk == EMURX_LK_NO_NS || lk == EMURX_LK_NS_NO_PLUGIN || lk == EMURX_LK_NO_CLIENT || lk == EMURX_LK_CLIENT_NO_PLUGIN)
        return EMURX_FT_ERR;
    if (lk != EMURX_LK_CLIENT || cid >= max_clients || ns >= max_ns) return EMURX_FT_NONE;
    const uint32_t f = gld4(flow + i);
    const bool tcp = (b.z >> 24) == EMURX_CB_TCP;
    uint32_t o;
    if (f == EMURX_FLOW_NO_CTX) return EMURX_FT_ERR;  // :75-78
    else if (f == EMURX_FLOW_NO_SYN) {
        if (!tcp) return EMURX_FT_NONE;  // the classifier never produces it
        o = EMURX_FT_NO_SYN;             // client_ctx.go:837, :842
    } else if (f == EMURX_FLOW_NO_SERVER) o = tcp ? EMURX_FT_NO_SRV_TCP : EMURX_FT_NO_SRV_UDP;  // :851 / :878, :886
    else return EMURX_FT_NONE;  // a flow id, NEW, UNKNOWN, NONE: the handler runs and counts itself
    // the family, as client_ctx.go:918-920 and get_tuple read it: the one byte of the frame
    const uint32_t l3 = b.x >> 16;
    if (l3 < 14 || l3 >= d.len) return EMURX_FT_NONE;
    return (gld1(frames + d.off + l3) >> 4) == 4 ? o : o | EMURX_FT_V6;
}

// tile sums: x = NO_SYN | NO_SRV_TCP << 10 | NO_SRV_UDP << 20, y = ERR | candidates at NONE << 10 (each <= 256)
__device__ __forceinline__ uint32_t ft_tile_folds(const uint2& ts) { return ts.x; }

__device__ __forceinline__ uint32_t ft_hash(uint32_t cid) {
    uint32_t h = cid * 0x9E3779B1u;
    h ^= h >> 15;
    h *= 0x2C1B3C6Du;
    h ^= h >> 12;
    h *= 0x297A2D39u;
    return h ^ h >> 15;
}

// The row of client cid (hash h) in the set of mask + 1 owner words, owner = frame + 1 | the hash's
// top five bits << 27 (n < 2^26): claimed for frame i by one compare-and-swap, or found; the owner's
// key is its record's client_id.  The batch's part of the set has at least twice as many slots as
// the batch has frames, so a free slot always ends the probe; the trip count is bounded all the same.
__device__ __forceinline__ uint32_t ft_insert(uint32_t* own, uint32_t mask, const emurx_rec* __restrict__ rec, uint32_t n,
                                              uint32_t cid, uint32_t h, uint32_t i, uint32_t& slot) {
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
        if (j >= n) continue;  // no owner of this batch
        if (gld4(reinterpret_cast<const uint32_t*>(rec + j) + 1) == cid) return j;
    }
    return kFtNone;
}

__global__ __launch_bounds__(kBlock) void k_ft_fold(const uint8_t* __restrict__ frames, const emurx_desc* __restrict__ desc,
                                                    const emurx_rec* __restrict__ rec, const uint32_t* __restrict__ flow,
                                                    uint32_t n, uint32_t max_ns, uint32_t max_clients, uint32_t* own,
                                                    uint32_t mask, uint32_t* acc, uint32_t* __restrict__ row_of,
                                                    uint2* __restrict__ tsum, uint8_t* __restrict__ outcome) {
    __shared__ uint32_t s_sum[2];
    if (threadIdx.x < 2) s_sum[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t i = blockIdx.x * kFtTile + threadIdx.x, lane = lane_id();
    uint32_t ob = EMURX_FT_NONE, cid = 0;
    bool cand = false;
    if (i < n) {
        const uint4 b = gld16(reinterpret_cast<const uint4*>(rec + i) + 1);
        if (ft_rec_candidate(b)) {
            const emurx_desc d = desc[i];
            if (d.pad != EMURX_DESC_HOLE) {
                const uint2 a = *reinterpret_cast<const uint2*>(rec + i);  // ns_id, client_id
                cand = true;
                cid = a.y;
                ob = ft_decide(frames, d, b, a.x, cid, flow, i, max_ns, max_clients);
            }
        }
        if (outcome) outcome[i] = (uint8_t)ob;
    }
    const uint32_t o = ob & 7u;
    const bool folds = o >= EMURX_FT_NO_SYN && o <= EMURX_FT_NO_SRV_UDP, v6 = (ob & EMURX_FT_V6) != 0;
    const uint64_t m1 = __ballot(o == EMURX_FT_NO_SYN), m2 = __ballot(o == EMURX_FT_NO_SRV_TCP),
                   m3 = __ballot(o == EMURX_FT_NO_SRV_UDP), m6 = __ballot(folds && v6);
    const uint32_t cx = (uint32_t)__popcll(m1) | (uint32_t)__popcll(m2) << 10 | (uint32_t)__popcll(m3) << 20;
    const uint32_t cy = (uint32_t)__popcll(__ballot(o == EMURX_FT_ERR)) | (uint32_t)__popcll(__ballot(cand && ob == EMURX_FT_NONE)) << 10;
    if (lane == 0 && (cx | cy)) {
        atomicAdd(&s_sum[0], cx);
        atomicAdd(&s_sum[1], cy);
    }
    // the wave's lanes of one client, combined: the group's first lane keeps its counts and its last lane
    uint32_t lead = lane, glast = lane, g1 = 0, g2 = 0, g3 = 0, g6 = 0;
    for (uint64_t left = m1 | m2 | m3; left;) {  // wave-uniform
        const uint32_t l0 = (uint32_t)__ffsll((long long)left) - 1;
        const uint32_t g = (uint32_t)__builtin_amdgcn_readlane((int)cid, (int)l0);
        const uint64_t m = __ballot(folds && cid == g);
        if (folds && cid == g) lead = l0;
        if (lane == l0) {
            glast = 63u - (uint32_t)__clzll((long long)m);
            g1 = (uint32_t)__popcll(m & m1), g2 = (uint32_t)__popcll(m & m2), g3 = (uint32_t)__popcll(m & m3);
            g6 = (uint32_t)__popcll(m & m6);
        }
        left &= ~m;
    }
    uint32_t row = kFtNone;
    if (folds && lead == lane) {
        uint32_t slot = kFtNone;
        row = ft_insert(own, mask, rec, n, cid, ft_hash(cid), i, slot);
        if (row != kFtNone) {
            uint32_t* a = acc + (size_t)row * kFtAccWords;
            if (slot != kFtNone) a[kFtSlot] = slot + 1;  // the claimer alone; read by the emit launch
            if (g1 | g2)
                __hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(a + kFtAccA), (unsigned long long)g2 << 32 | g1,
                                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (g3 | g6)
                __hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(a + kFtAccB), (unsigned long long)g6 << 32 | g3,
                                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_max(a + kFtNFirst, ~i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_max(a + kFtLast, i - lane + glast, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    row = (uint32_t)__shfl((int)row, (int)lead);  // every lane of a group takes its first lane's row
    __syncthreads();
    const uint2 ts = make_uint2(s_sum[0], s_sum[1]);
    if (threadIdx.x == 0) tsum[blockIdx.x] = ts;
    // the row indices are read by the later passes of tiles that fold only
    if (ft_tile_folds(ts) && i < n) row_of[i] = folds ? row : kFtNone;
}

// tcnt[t]: the tile's emitters
__global__ __launch_bounds__(kBlock) void k_ft_mark(uint32_t n, const uint2* __restrict__ tsum, const uint32_t* __restrict__ acc,
                                                    uint32_t* __restrict__ row_of, uint32_t* __restrict__ tcnt) {
    __shared__ uint32_t s_cnt;
    const uint32_t t = blockIdx.x;
    if (!ft_tile_folds(tsum[t])) {  // workgroup-uniform
        if (threadIdx.x == 0) tcnt[t] = 0;
        return;
    }
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    const uint32_t i = t * kFtTile + threadIdx.x;
    bool emits = false;
    if (i < n) {
        const uint32_t r = row_of[i];
        if (r != kFtNone && r < n) {
            emits = gld4(acc + (size_t)r * kFtAccWords + kFtLast) == i;
            if (emits) row_of[i] = r | kFtEmits;
        }
    }
    const uint32_t c = (uint32_t)__popcll(__ballot(emits));
    if (lane_id() == 0 && c) atomicAdd(&s_cnt, c);
    __syncthreads();
    if (threadIdx.x == 0) tcnt[t] = s_cnt;
}

// info: {events written, distinct clients, overflow, frames NO_SYN, NO_SRV_TCP, NO_SRV_UDP, ERR,
// candidates left at NONE}
__global__ __launch_bounds__(kFtScanBlock) void k_ft_scan(const uint2* __restrict__ tsum, const uint32_t* __restrict__ tcnt,
                                                          uint32_t ntiles, uint32_t ev_cap, uint32_t* __restrict__ tord,
                                                          unsigned long long* __restrict__ info) {
    __shared__ BlockScanLds<kFtScanBlock, uint32_t> s_scan;
    __shared__ uint32_t s_oc[5];
    const uint32_t tid = threadIdx.x;
    if (tid < 5) s_oc[tid] = 0;
    __syncthreads();
    uint32_t base = 0, oc[5] = {0, 0, 0, 0, 0};
    for (uint32_t t0 = 0; t0 < ntiles; t0 += kFtScanBlock) {  // workgroup-uniform trip count
        const uint32_t t = t0 + tid;
        const uint2 v = t < ntiles ? tsum[t] : make_uint2(0, 0);
        const uint32_t cnt = t < ntiles ? tcnt[t] : 0u;
        oc[0] += v.x & 0x3ffu;
        oc[1] += (v.x >> 10) & 0x3ffu;
        oc[2] += v.x >> 20;
        oc[3] += v.y & 0x3ffu;
        oc[4] += v.y >> 10;
        uint32_t c = cnt;
        const auto [total] = block_incl_scan<kFtScanBlock>(s_scan, c);
        if (t < ntiles) tord[t] = base + c - cnt;
        base += total;
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const uint32_t s = wave_sum_u32(oc[k]);
        if (lane_id() == 0 && s) atomicAdd(&s_oc[k], s);
    }
    __syncthreads();
    if (tid < EMURX_FT_INFO_WORDS) {
        const bool over = base > ev_cap;
        info[tid] = tid == 0 ? (over ? 0u : base) : tid == 1 ? base : tid == 2 ? (over ? 1u : 0u) : s_oc[tid - 3];
    }
}

__global__ __launch_bounds__(kBlock) void k_ft_emit(uint32_t n, const uint2* __restrict__ tsum, const emurx_rec* __restrict__ rec,
                                                    const uint32_t* __restrict__ row_of, const uint32_t* __restrict__ tord,
                                                    uint32_t* own, uint32_t mask, uint32_t* acc, uint32_t ev_cap,
                                                    const unsigned long long* __restrict__ info, uint2* __restrict__ ev) {
    __shared__ uint32_t s_w[kWaves];
    const uint32_t t = blockIdx.x;
    if (!ft_tile_folds(tsum[t])) return;  // workgroup-uniform
    const bool over = info[2] != 0;
    const uint32_t i = t * kFtTile + threadIdx.x, lane = lane_id(), wv = threadIdx.x / kWave;
    const uint32_t r = i < n ? row_of[i] : kFtNone;
    const bool emits = r != kFtNone && (r & kFtEmits);
    const unsigned long long bal = __ballot(emits);
    if (lane == 0) s_w[wv] = (uint32_t)__popcll(bal);
    __syncthreads();
    if (!emits) return;
    uint32_t k = tord[t] + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
    for (uint32_t w = 0; w < wv; ++w) k += s_w[w];
    uint4* row = reinterpret_cast<uint4*>(acc + (size_t)(r & ~kFtEmits) * kFtAccWords);
    const uint4 lo = gld16(row), hi = gld16(row + 1);
    row[0] = make_uint4(0, 0, 0, 0);  // rows and slots are all zero again when the call ends
    row[1] = make_uint4(0, 0, 0, 0);
    if (hi.z && hi.z - 1 <= mask) own[hi.z - 1] = 0;
    if (over || k >= ev_cap) return;
    // the client's last frame is this one: ns_id and client_id are its record's
    const uint2 key = *reinterpret_cast<const uint2*>(rec + i);
    const uint32_t n1 = lo.x, n2 = lo.y, n3 = lo.z, n6 = lo.w, frames = n1 + n2 + n3;
    uint2* e = ev + 6 * (size_t)k;  // emurx_ft_ev
    e[0] = make_uint2(key.x, key.y);
    e[1] = make_uint2(~hi.x, hi.y);
    e[2] = make_uint2(frames, frames - n6);  // frames, cnt[LOOKUP_V4]
    e[3] = make_uint2(n6, n1 + n2);          // cnt[LOOKUP_V6], cnt[NEW_TCP]
    e[4] = make_uint2(n1, n3);               // cnt[NEW_TCP_NO_SYN], cnt[NEW_UDP]
    e[5] = make_uint2(n2 + n3, 0);           // cnt[NEW_NO_CB], zero
}

// A slot's flow stage to the host (emurx_ingest_set_flows): one launch behind emurx_ftstat_dev on
// the slot's stream reads the stage's counts on the device and copies, with 16-byte stores over the
// bus into the slot's pinned block (as k_png_out does), the info words, the n flow words, the n
// outcome bytes and the events written, no more.  The regions start on 256-byte boundaries on both
// sides and hold whole 16-byte vectors; the event count is clamped to the pinned region's capacity
// (the host checks info[0] against the same capacity and fails the batch).
__global__ __launch_bounds__(kBlock) void k_ft_out(const unsigned long long* __restrict__ info, const emurx_ft_ev* __restrict__ ev,
                                                   const uint32_t* __restrict__ flow, const uint8_t* __restrict__ outcome,
                                                   uint32_t n, uint32_t ev_cap, uint8_t* h_info, uint8_t* h_ev, uint8_t* h_flow,
                                                   uint8_t* h_outcome) {
    const uint64_t nev = min((uint64_t)info[0], (uint64_t)ev_cap);
    const uint64_t gid = (uint64_t)blockIdx.x * kBlock + threadIdx.x, gsz = (uint64_t)gridDim.x * kBlock;
    auto copy = [&](const void* src, void* dst, uint64_t bytes) {
        const uint64_t nv = (bytes + 15) >> 4;
        for (uint64_t v = gid; v < nv; v += gsz)
            reinterpret_cast<uint4*>(dst)[v] = gld16(reinterpret_cast<const uint4*>(src) + v);
    };
    copy(info, h_info, 8 * (uint64_t)EMURX_FT_INFO_WORDS);
    copy(flow, h_flow, 4 * (uint64_t)n);
    copy(outcome, h_outcome, n);
    copy(ev, h_ev, nev * sizeof(emurx_ft_ev));
}

}  // namespace emurx

// scratch: the accumulator rows u32 [max_frames][8] (a client's row is its owner frame's), the set's
// owner words u32 [slots], then row indices u32 [max_frames], tile sums uint2, tile counts u32 and
// tile ordinals u32 [tiles of max_frames].  The accumulator rows and the owner words start, and
// every call leaves them, all zero.
struct FtScratch {
    uint32_t *acc, *own, *row_of;
    uint2* tsum;
    uint32_t *tcnt, *tord;
    size_t bytes;
};
static FtScratch ft_scratch(void* base, uint32_t max_frames) {
    const size_t mt = ((size_t)max_frames + emurx::kFtTile - 1) / emurx::kFtTile;
    emurx_carver c(base);  // the initialisers run in order
    return {c.take<uint32_t>((size_t)max_frames * emurx::kFtAccWords), c.take<uint32_t>(emurx_lrn_slots(max_frames)),
            c.take<uint32_t>(max_frames), c.take<uint2>(mt), c.take<uint32_t>(mt), c.take<uint32_t>(mt), c.bytes()};
}
size_t emurx_ft_scratch_bytes(uint32_t max_frames) { return ft_scratch(nullptr, max_frames).bytes; }

int emurx_ft_scratch_clear(void* scratch, uint32_t max_frames, hipStream_t st) {
    const FtScratch s = ft_scratch(scratch, max_frames);
    return EMURX_HIP_OK(hipMemsetAsync(s.acc, 0, (size_t)max_frames * emurx::kFtAccWords * 4, st)) &&
                   EMURX_HIP_OK(hipMemsetAsync(s.own, 0, (size_t)emurx_lrn_slots(max_frames) * 4, st))
               ? 0
               : -1;
}

int emurx_launch_ftstat(const uint8_t* frames, const emurx_desc* desc, const emurx_rec* rec, const uint32_t* flow, uint32_t n,
                        uint32_t max_ns, uint32_t max_clients, emurx_ft_ev* ev, uint32_t ev_cap, uint8_t* outcome,
                        uint64_t* info, void* scratch, uint32_t max_frames, hipStream_t st) {
    using namespace emurx;
    unsigned long long* inf = reinterpret_cast<unsigned long long*>(info);
    if (n == 0) return EMURX_HIP_OK(hipMemsetAsync(inf, 0, 8 * (size_t)EMURX_FT_INFO_WORDS, st)) ? 0 : -1;
    const uint32_t nt = (n + kFtTile - 1) / kFtTile;
    const FtScratch s = ft_scratch(scratch, max_frames);  // sized by the handle's max_frames, not by n
    const uint32_t mask = emurx_lrn_slots(n) - 1;  // as the learning fold: at least twice the batch's frames
    hipError_t e = emurx_launch(k_ft_fold, dim3(nt), dim3(kBlock), 0, st, frames, desc, rec, flow, n, max_ns, max_clients,
                                s.own, mask, s.acc, s.row_of, s.tsum, outcome);
    if (e == hipSuccess) e = emurx_launch(k_ft_mark, dim3(nt), dim3(kBlock), 0, st, n, s.tsum, s.acc, s.row_of, s.tcnt);
    if (e == hipSuccess) e = emurx_launch(k_ft_scan, dim3(1), dim3(kFtScanBlock), 0, st, s.tsum, s.tcnt, nt, ev_cap, s.tord, inf);
    if (e == hipSuccess)
        e = emurx_launch(k_ft_emit, dim3(nt), dim3(kBlock), 0, st, n, s.tsum, rec, s.row_of, s.tord, s.own, mask, s.acc, ev_cap,
                         inf, reinterpret_cast<uint2*>(ev));
    return EMURX_HIP_OK(e) ? 0 : -1;
}

int emurx_launch_ft_out(const uint64_t* info, const emurx_ft_ev* ev, const uint32_t* flow, const uint8_t* outcome, uint32_t n,
                        uint32_t ev_cap, uint8_t* h_info, uint8_t* h_ev, uint8_t* h_flow, uint8_t* h_outcome, hipStream_t st) {
    using namespace emurx;
    // as k_png_out: a workgroup per tile of the batch, at most 256
    const uint32_t g = std::min<uint32_t>(std::max<uint32_t>((n + kBlock - 1) / kBlock, 1), 256);
    return EMURX_HIP_OK(emurx_launch(k_ft_out, dim3(g), dim3(kBlock), 0, st, reinterpret_cast<const unsigned long long*>(info), ev,
                                     flow, outcome, n, ev_cap, h_info, h_ev, h_flow, h_outcome))
               ? 0
               : -1;
}

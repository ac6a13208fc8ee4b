// emurx_pingtx.hip — the send side of the ping plugin on the device (gfx950): echo requests
// generated from resident templates (src/emu/plugins/ping/ping.go:317-341, Ping.sendPing, over the
// packets of PreparePingPacketTemplate, plugins/icmp/icmp.go:208-237 and plugins/ipv6/ipv6.go:216-262).
// A request {id, seq, count, ts} stands for `count` frames: template `id` with the sequence number
// seq + k at icmp_off + 6, the timestamp at icmp_off + 16 and the checksum at icmp_off + 2 that
// sendPing's chain of incremental updates leaves (gopacket layers/icmp4.go:238-285), which is
//   ~fold(~cs_t + ~seq_t + seq + sum over the four 16-bit words of (~ts_t + ts))
// with cs_t, seq_t and ts_t the template's own fields: nine adds per frame and no sum over a frame.
// emurx_pingtx_dev, three launches:
//   k_ptx_count   one request per lane: the slot head of its id (8 bytes) gives the frame length;
//                 per request its first frame and first 16-byte output chunk inside its 256-request
//                 tile (one workgroup scan), per tile the totals.
//   k_ptx_scan    one workgroup: exclusive scan of the tiles' frames and chunks, the needed bytes
//                 and frames into d_info.
//   k_ptx_emit    the first workgroups, one per tile of requests, give each request its outcome and
//                 count the outcomes; the others deal the output's 16-byte chunks over their lanes,
//                 1,024 chunks per workgroup, whatever request they belong to: a chunk finds its tile
//                 and its request by bisection of the scanned offsets, copies its 16 template bytes
//                 with one load and one store and overlays the patched bytes that fall inside it.
//                 The chunk that starts a frame writes its descriptor.  A burst of 60,000 frames
//                 from one request is dealt like 60,000 requests of one.
// k_ptx_apply ships edited slots of the template store (emurx_api.cpp, ship_pingtx).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/emu_rx.h"
#include "emurx_kernels.h"
#include "emurx_wave.h"

namespace emurx {

constexpr uint32_t kPtxTile = kBlock;        // requests per tile
constexpr uint32_t kPtxScanBlock = 1024;
constexpr uint32_t kPtxPer = 4;              // chunks per lane of an emit workgroup
constexpr uint32_t kPtxChunks = kBlock * kPtxPer;

// 16 bytes from an 8-byte aligned address (a template's bytes start 8 bytes into its slot; the
// requests are 8-byte aligned)
typedef unsigned emurx_v4u_a8 __attribute__((ext_vector_type(4), aligned(8)));
__device__ __forceinline__ uint4 gld16_a8(const void* p) {
    const emurx_v4u_a8 v = *(const __attribute__((address_space(1))) emurx_v4u_a8*)p;
    return make_uint4(v.x, v.y, v.z, v.w);
}
typedef unsigned emurx_v2u __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint2 gld8(const void* p) {
    const emurx_v2u v = *(const __attribute__((address_space(1))) emurx_v2u*)p;
    return make_uint2(v.x, v.y);
}

// what a request asks for: its slot head (len | icmp_off << 16, vport) if its id is in use
struct PtxReq {
    uint32_t id, seq, count;
    uint32_t len, icmp_off, vport;  // len == 0: the id is free or out of range
    unsigned long long ts;
};
__device__ __forceinline__ PtxReq ptx_req(const emurx_pingtx_req* __restrict__ req, uint32_t r,
                                          const uint8_t* __restrict__ store, uint32_t max_pings) {
    const uint4 q = gld16_a8(req + r);
    PtxReq p{q.x, q.y & 0xffffu, q.y >> 16, 0, 0, 0, (unsigned long long)q.w << 32 | q.z};
    if (p.id < max_pings) {
        const uint2 hd = gld8(store + (size_t)p.id * EMURX_PINGTX_SLOT);
        p.len = hd.x & 0xffffu;
        p.icmp_off = hd.x >> 16;
        p.vport = hd.y & 0xffu;
    }
    return p;
}

__global__ __launch_bounds__(kBlock) void k_ptx_count(const emurx_pingtx_req* __restrict__ req, uint32_t n,
                                                      const uint8_t* __restrict__ store, uint32_t max_pings,
                                                      uint32_t* __restrict__ rfrm, uint32_t* __restrict__ rrow,
                                                      uint2* __restrict__ tsum) {
    __shared__ BlockScanLds<kBlock, uint32_t, uint32_t> s_scan;
    const uint32_t r = blockIdx.x * kPtxTile + threadIdx.x;
    uint32_t frames = 0, rows = 0;
    if (r < n) {
        const PtxReq p = ptx_req(req, r, store, max_pings);
        frames = p.len ? p.count : 0u;
        rows = frames * ((p.len + 15) >> 4);  // at most 65,535 * 16
    }
    // a tile holds at most 256 * 65,535 frames and 16 times as many chunks: 32 bits
    uint32_t f = frames, c = rows;
    const auto [ftot, ctot] = block_incl_scan<kBlock, false>(s_scan, f, c);
    if (r < n) {
        rfrm[r] = f - frames;
        rrow[r] = c - rows;
    }
    if (threadIdx.x == 0) tsum[blockIdx.x] = make_uint2(ftot, ctot);
}

// tfrm / trow [ntiles + 1]: the first frame and chunk of every tile, the totals behind them;
// info = {0, bytes needed, frames needed, 0, ...}: the emit pass adds the written frames and the
// requests per outcome
__global__ __launch_bounds__(kPtxScanBlock) void k_ptx_scan(const uint2* __restrict__ tsum, uint32_t ntiles,
                                                            unsigned long long* __restrict__ tfrm,
                                                            unsigned long long* __restrict__ trow,
                                                            unsigned long long* __restrict__ info) {
    __shared__ BlockScanLds<kPtxScanBlock, unsigned long long, unsigned long long> s_scan;
    unsigned long long fbase = 0, cbase = 0;
    for (uint32_t t0 = 0; t0 < ntiles; t0 += kPtxScanBlock) {  // workgroup-uniform trip count
        const uint32_t t = t0 + threadIdx.x;
        const uint2 v = t < ntiles ? tsum[t] : make_uint2(0, 0);
        unsigned long long f = v.x, c = v.y;
        const auto [ftot, ctot] = block_incl_scan<kPtxScanBlock>(s_scan, f, c);
        if (t < ntiles) {
            tfrm[t] = fbase + f - v.x;
            trow[t] = cbase + c - v.y;
        }
        fbase += ftot;
        cbase += ctot;
    }
    if (threadIdx.x == 0) {
        tfrm[ntiles] = fbase;
        trow[ntiles] = cbase;
    }
    if (threadIdx.x < EMURX_PTX_INFO_WORDS)
        info[threadIdx.x] = threadIdx.x == 1 ? cbase * 16ull : threadIdx.x == 2 ? fbase : 0ull;
}

// byte `pos` of the frame, if it lies in the chunk that starts at y0, becomes v: selects on the
// four words, not a store at a computed index (which would put the chunk in scratch)
__device__ __forceinline__ void ptx_set_byte(uint32_t o[4], uint32_t y0, uint32_t pos, uint32_t v) {
    const uint32_t j = pos - y0;
    if (j >= 16) return;
    const uint32_t sh = 8 * (j & 3), w = j >> 2, m = ~(0xffu << sh), x = v << sh;
    o[0] = w == 0 ? (o[0] & m) | x : o[0];
    o[1] = w == 1 ? (o[1] & m) | x : o[1];
    o[2] = w == 2 ? (o[2] & m) | x : o[2];
    o[3] = w == 3 ? (o[3] & m) | x : o[3];
}
__device__ __forceinline__ uint32_t ptx_be16(const uint8_t* p) { return gld1(p) << 8 | gld1(p + 1); }

// the last index in [lo, hi) whose offset is at most x (off[lo] <= x): requests and tiles without
// frames share their successor's offset, so this is the one that holds chunk x
template <typename T>
__device__ __forceinline__ uint32_t ptx_owner(const T* __restrict__ off, uint32_t lo, uint32_t hi, T x) {
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (off[mid] <= x) lo = mid;
        else hi = mid;
    }
    return lo;
}

// does a request that ends at chunk `cend` and frame `fend` fit the output?  The ends ascend with
// the request index, so the requests that fit are a prefix and sit where the scan put them.
__device__ __forceinline__ bool ptx_fits(unsigned long long cend, unsigned long long fend, unsigned long long cap,
                                         uint32_t desc_cap) {
    return cend * 16ull <= cap && fend <= desc_cap;
}

__global__ __launch_bounds__(kBlock) void k_ptx_emit(const emurx_pingtx_req* __restrict__ req, uint32_t n,
                                                     const uint8_t* __restrict__ store, uint32_t max_pings,
                                                     const uint32_t* __restrict__ rfrm, const uint32_t* __restrict__ rrow,
                                                     const unsigned long long* __restrict__ tfrm,
                                                     const unsigned long long* __restrict__ trow, uint32_t ntiles,
                                                     uint8_t* __restrict__ out, unsigned long long cap,
                                                     emurx_desc* __restrict__ odesc, uint32_t desc_cap, uint32_t off_base,
                                                     uint8_t* __restrict__ fzero0, uint8_t* __restrict__ fzero1,
                                                     uint8_t* __restrict__ outcome, unsigned long long* __restrict__ info) {
    if (blockIdx.x < ntiles) {  // workgroup-uniform: this workgroup gives a tile's requests their outcomes
        __shared__ uint32_t s_cnt[4];  // requests with outcome 0..2, frames written
        if (threadIdx.x < 4) s_cnt[threadIdx.x] = 0;
        __syncthreads();
        const uint32_t t = blockIdx.x, r = t * kPtxTile + threadIdx.x;
        uint32_t oc = 3, frames = 0;  // 3: no request
        if (r < n) {
            const PtxReq p = ptx_req(req, r, store, max_pings);
            frames = p.len ? p.count : 0u;
            const unsigned long long fend = tfrm[t] + rfrm[r] + frames;
            const unsigned long long cend = trow[t] + rrow[r] + (unsigned long long)frames * ((p.len + 15) >> 4);
            oc = !p.len ? EMURX_PTX_BAD_ID : frames && !ptx_fits(cend, fend, cap, desc_cap) ? EMURX_PTX_NOSPC : EMURX_PTX_OK;
            if (outcome) outcome[r] = (uint8_t)oc;
            if (oc != EMURX_PTX_OK) frames = 0;
        }
        const uint32_t written = wave_sum_u32(frames);  // at most 64 * 65,535
        for (uint32_t k = 0; k < 3; ++k) {
            const uint32_t c = (uint32_t)__popcll(__ballot(oc == k));
            if (lane_id() == 0 && c) atomicAdd(&s_cnt[k], c);
        }
        if (lane_id() == 0 && written) atomicAdd(&s_cnt[3], written);
        __syncthreads();
        if (threadIdx.x < 4 && s_cnt[threadIdx.x])
            atomicAdd(&info[threadIdx.x == 3 ? 0 : 3 + threadIdx.x], (unsigned long long)s_cnt[threadIdx.x]);
        return;
    }
    const unsigned long long total = trow[ntiles];
    const unsigned long long c0 = (unsigned long long)(blockIdx.x - ntiles) * kPtxChunks;
    if (c0 >= total) return;  // workgroup-uniform
    // the tiles this workgroup's chunks lie in: two bisections every lane makes alike
    const unsigned long long clast = min(c0 + kPtxChunks, total) - 1;
    const uint32_t tlo = ptx_owner(trow, 0u, ntiles, c0), thi = ptx_owner(trow, tlo, ntiles, clast);
#pragma unroll
    for (uint32_t j = 0; j < kPtxPer; ++j) {
        const unsigned long long c = c0 + j * kBlock + threadIdx.x;
        if (c >= total) continue;
        const uint32_t t = ptx_owner(trow, tlo, thi + 1, c);
        const unsigned long long cbase = trow[t];
        const uint32_t r = ptx_owner(rrow, t * kPtxTile, min(n, (t + 1) * kPtxTile), (uint32_t)(c - cbase));
        const PtxReq p = ptx_req(req, r, store, max_pings);
        const uint32_t rows = (p.len + 15) >> 4;
        const uint32_t x = (uint32_t)(c - cbase) - rrow[r];  // the chunk inside the request: below 2^20
        const uint32_t k = x / rows, q = x - k * rows;       // its frame and the chunk inside the frame
        const unsigned long long f0 = tfrm[t] + rfrm[r];
        if (!ptx_fits(c - x + (unsigned long long)p.count * rows, f0 + p.count, cap, desc_cap)) continue;
        const uint8_t* tm = store + (size_t)p.id * EMURX_PINGTX_SLOT + 8;
        const uint4 v = gld16_a8(tm + 16 * q);
        uint32_t o[4] = {v.x, v.y, v.z, v.w};
        const uint32_t y0 = 16 * q, io = p.icmp_off;
        if (y0 < io + 24 && y0 + 16 > io + 2) {  // a patched byte lies in this chunk
            const uint32_t seq = (p.seq + k) & 0xffffu;
            if (y0 < io + 4) {  // the checksum does
                uint32_t s = (~ptx_be16(tm + io + 2) & 0xffffu) + (~ptx_be16(tm + io + 6) & 0xffffu) + seq;
#pragma unroll
                for (uint32_t i = 0; i < 4; ++i)
                    s += (~ptx_be16(tm + io + 16 + 2 * i) & 0xffffu) + ((uint32_t)(p.ts >> (48 - 16 * i)) & 0xffffu);
                s = (s >> 16) + (s & 0xffffu);  // eleven terms of at most 0xffff: below 2^20, two folds
                s = (s >> 16) + (s & 0xffffu);
                const uint32_t cs = ~s & 0xffffu;
                ptx_set_byte(o, y0, io + 2, cs >> 8);
                ptx_set_byte(o, y0, io + 3, cs & 0xffu);
            }
            ptx_set_byte(o, y0, io + 6, seq >> 8);
            ptx_set_byte(o, y0, io + 7, seq & 0xffu);
#pragma unroll
            for (uint32_t i = 0; i < 8; ++i) ptx_set_byte(o, y0, io + 16 + i, (uint32_t)(p.ts >> (56 - 8 * i)) & 0xffu);
        }
        *reinterpret_cast<uint4*>(out + c * 16ull) = make_uint4(o[0], o[1], o[2], o[3]);
        if (q == 0) {  // {off, len, vport, pad 0}
            *reinterpret_cast<uint2*>(odesc + f0 + k) = make_uint2(off_base + (uint32_t)(c * 16ull), p.len | p.vport << 16);
            if (fzero0) fzero0[f0 + k] = fzero1[f0 + k] = 0;  // an egress slot's plan and status bytes of the frame
        }
    }
}

// an edited slot: {id, zeros} and the slot's 256 bytes, 17 16-byte vectors; 16 lanes copy one slot
__global__ __launch_bounds__(kBlock) void k_ptx_apply(const uint4* __restrict__ delta, uint32_t n, uint4* __restrict__ store) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x, e = i >> 4, j = i & 15;
    if (e >= n) return;
    const uint32_t id = delta[(size_t)e * 17].x;
    store[(size_t)id * 16 + j] = delta[(size_t)e * 17 + 1 + j];
}

}  // namespace emurx

// scratch: per request its first frame and chunk inside its tile, per tile the sums, then the
// scanned tile offsets with the totals behind them
struct PtxScratch {
    uint32_t *rfrm, *rrow;
    uint2* tsum;
    unsigned long long *tfrm, *trow;
    size_t bytes;
};
static PtxScratch ptx_scratch(void* base, uint32_t n) {
    const size_t nt = ((size_t)n + emurx::kPtxTile - 1) / emurx::kPtxTile;
    emurx_carver c(base);  // the initialisers run in order
    return {c.take<uint32_t>(n), c.take<uint32_t>(n), c.take<uint2>(nt), c.take<unsigned long long>(nt + 1),
            c.take<unsigned long long>(nt + 1), c.bytes()};
}
size_t emurx_ptx_scratch_bytes(uint32_t n) { return ptx_scratch(nullptr, n).bytes; }

int emurx_launch_pingtx_apply(const void* delta, uint32_t n, uint8_t* store, hipStream_t st) {
    using namespace emurx;
    if (n == 0) return 0;
    return EMURX_HIP_OK(emurx_launch(k_ptx_apply, dim3((n * 16 + kBlock - 1) / kBlock), dim3(kBlock), 0, st,
                                     static_cast<const uint4*>(delta), n, reinterpret_cast<uint4*>(store)))
               ? 0
               : -1;
}

int emurx_launch_pingtx(const emurx_pingtx_req* req, uint32_t n, const uint8_t* store, uint32_t max_pings, uint8_t* out,
                        uint64_t cap, emurx_desc* out_desc, uint32_t desc_cap, uint32_t off_base, uint8_t* fzero0,
                        uint8_t* fzero1, uint8_t* outcome, uint64_t* info, void* scratch, hipStream_t st) {
    using namespace emurx;
    unsigned long long* inf = reinterpret_cast<unsigned long long*>(info);
    if (n == 0) return EMURX_HIP_OK(hipMemsetAsync(inf, 0, 8 * (size_t)EMURX_PTX_INFO_WORDS, st)) ? 0 : -1;
    const uint32_t nt = (n + kPtxTile - 1) / kPtxTile;
    const PtxScratch s = ptx_scratch(scratch, n);
    // the descriptor's offset is 32 bits: nothing may end past 4 GiB
    const unsigned long long room = (1ull << 32) - off_base, lim = cap < room ? cap : room;
    // the chunks the call can write at most, which size the grid: the capacity's, the requests'
    // (65,535 frames of 16 chunks each) and the descriptors'
    unsigned long long chunks = lim / 16;
    chunks = std::min(chunks, (unsigned long long)n * 65535ull * 16ull);
    chunks = std::min(chunks, (unsigned long long)desc_cap * 16ull);
    const uint32_t nb = (uint32_t)((chunks + kPtxChunks - 1) / kPtxChunks);
    hipError_t e = emurx_launch(k_ptx_count, dim3(nt), dim3(kBlock), 0, st, req, n, store, max_pings, s.rfrm, s.rrow, s.tsum);
    if (e == hipSuccess) e = emurx_launch(k_ptx_scan, dim3(1), dim3(kPtxScanBlock), 0, st, s.tsum, nt, s.tfrm, s.trow, inf);
    if (e == hipSuccess)
        e = emurx_launch(k_ptx_emit, dim3(nt + nb), dim3(kBlock), 0, st, req, n, store, max_pings, s.rfrm, s.rrow, s.tfrm,
                         s.trow, nt, out, lim, out_desc, desc_cap, off_base, fzero0, fzero1, outcome, inf);
    return EMURX_HIP_OK(e) ? 0 : -1;
}

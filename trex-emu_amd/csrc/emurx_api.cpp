// emurx_api.cpp — C-ABI of the MI355X receive path (include/emu_rx.h).
//
// Owns the Namespace / Client tables (emurx_mirror.*: the Go maps plus the image of every
// device table, edited slot by slot), ships the edited 64-byte blocks to the device before
// the next batch that reads them (one H2D copy + one k_apply launch, stream-ordered against
// every stream that read the tables, no host synchronisation), the device scratch of a batch,
// and the host batch entry points that replace VethIFZmq.OnRxStream's per-frame loop
// (src/emu/core/veth_zmq.go:277-320).  No exception or abort crosses the ABI.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <array>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <new>
#include <string>
#include <vector>

#include "../../include/emu_rx.h"
#include "emurx_kernels.h"
#include "emurx_mirror.h"
#include "emurx_tables.h"

using emurx_host::Blocks;
using emurx_host::Hash;
using emurx_host::Mirror;

namespace {

uint16_t be16(const uint8_t* p) { return (uint16_t)((p[0] << 8) | p[1]); }
uint32_t be32(const uint8_t* p) {
    return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
}
uint32_t le32(const uint8_t* p) { return p[0] | (p[1] << 8) | (p[2] << 16) | ((uint32_t)p[3] << 24); }

template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    int alloc(size_t count) {
        if (count <= n && p) return 0;
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
        if (!EMURX_HIP_OK(hipMalloc((void**)&p, std::max<size_t>(count, 1) * sizeof(T)))) return -1;
        n = count;
        return 0;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
};
template <class T>
struct PinBuf {
    T* p = nullptr;
    size_t n = 0;
    int alloc(size_t count) {
        if (count <= n && p) return 0;
        if (p) (void)hipHostFree(p);
        p = nullptr;
        n = 0;
        if (!EMURX_HIP_OK(hipHostMalloc((void**)&p, std::max<size_t>(count, 1) * sizeof(T), hipHostMallocDefault)))
            return -1;
        n = count;
        return 0;
    }
    void release() {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        n = 0;
    }
};

// a typed place inside a slot's result block (IngestSlot::h_res / d_res)
template <class T>
struct View {
    T* p = nullptr;
};
// One in-flight batch of the batched ZMQ ingest: pinned staging + device scratch + results.
// The results (records, descriptors, packed queues, message status, qoff, folded histogram)
// share one device block and one pinned block of the same layout (set_results): the pipeline
// copies them back with one D2H, and the one-launch path writes the pinned block directly.
struct IngestSlot {
    hipStream_t st = nullptr;
    hipEvent_t done = nullptr;
    bool pending = false;
    uint32_t nmsg = 0, slots = 0;  // messages and descriptor slots of the batch in flight
    PinBuf<uint8_t> h_buf;         // messages, written by the caller (+64 B pad)
    PinBuf<uint32_t> h_ctl;        // emurx_msg[nmsg], slot_base[nmsg + 1]
    PinBuf<uint32_t> h_mframes;
    PinBuf<uint8_t> h_mstatus;
    PinBuf<uint8_t> h_res;                 // the result block, pinned
    View<uint32_t> h_stat, h_qlist, h_qoff;
    View<emurx_rec> h_rec;
    View<emurx_desc> h_desc;
    View<uint64_t> h_hist;
    DevBuf<uint8_t> d_buf;
    DevBuf<uint32_t> d_ctl, d_qlist, d_tile_cnt, d_seg_off;
    DevBuf<uint64_t> d_hist;               // zero between batches (k_qscan clears it)
    DevBuf<uint8_t> d_res;                 // the result block, device
    View<uint32_t> d_stat, d_packed, d_qoff;
    View<emurx_desc> d_desc;
    View<emurx_rec> d_rec;
    View<uint64_t> d_hist_out;
    size_t res_bytes = 0;                  // the current batch's result block
    // the fused small-batch path's scratch (k_ingest_small), zero between batches
    DevBuf<uint32_t> d_qseg, d_tcnt, d_ticket;
    DevBuf<uint64_t> d_hsmall;
    PinBuf<uint32_t> h_done;  // the small path's completion word: the batch's seq, written last
    uint32_t seq = 0;
    bool small = false;       // the batch in flight took the small path
    std::vector<uint32_t> remap;          // slot -> frame index, only when a message fell short
    // answers (emurx_ingest_set_answers): the chain's outputs, sized once for cfg.max_frames /
    // cfg.max_bytes; the per-frame outcome arrays join the result block (set_results)
    uint32_t ans_kinds = 0;               // the setting for later submits (EMURX_RSPK_*, 0: off)
    uint32_t ans_batch = 0;               // the kinds of the batch in flight / last waited for
    uint32_t ans_time = 0;                // emurx_ingest_set_time: ip_time_ms of the slot's next submits
    bool waited = false;                  // a batch has been waited for
    uint64_t ans_rsp_cap = 0, ans_tx_cap = 0;
    uint32_t ans_r_cap = 0, ans_ev_cap = 0, ans_ns_cap = 0;
    DevBuf<uint8_t> d_rsp_out, d_tx;
    DevBuf<emurx_desc> d_rsp_desc;
    DevBuf<uint32_t> d_rsp_src;
    DevBuf<uint64_t> d_tx_off, d_ainfo;   // d_ainfo: rsp, lrn, nss and tx info, as the answer block's head
    DevBuf<emurx_learn_ev> d_lev;
    DevBuf<emurx_nsstat_ev> d_nsev;
    View<uint8_t> d_rspo, d_lrno, d_donef, h_rspo, h_lrno, h_donef;  // [n] in the result block
    PinBuf<uint8_t> h_ans;                // the pinned answer block (k_ans_out writes it)
    View<uint64_t> h_ahead, h_tx_off;
    View<uint8_t> h_tx;
    View<uint32_t> h_src;
    View<emurx_learn_ev> h_lev;
    View<emurx_nsstat_ev> h_nsev;
    // the ping stage (emurx_ingest_set_ping), behind nsstat in the chain: its outputs, sized once
    uint32_t png_fams = 0, png_batch = 0;  // the setting for later submits; the batch in flight / last waited for
    uint64_t png_now = 0;                  // emurx_ingest_set_now: now_unix_ns of the slot's next submits
    uint32_t png_ev_cap = 0;               // events the pinned block holds
    DevBuf<emurx_ping_ev> d_pev;
    DevBuf<uint64_t> d_pinfo;
    DevBuf<uint8_t> d_pngo;
    PinBuf<uint8_t> h_png;                 // the pinned block (k_png_out writes it)
    View<uint64_t> h_pinfo;
    View<uint8_t> h_pngo;
    View<emurx_ping_ev> h_pev;
    // the flow stage (emurx_ingest_set_flows): k_rx's flow words and the fold's outputs, sized once
    bool flw_on = false, flw_batch = false;  // the setting for later submits; the batch in flight / last waited for
    uint32_t flw_ev_cap = 0;                 // events the device array and the pinned block hold
    DevBuf<uint32_t> d_flow;
    DevBuf<emurx_ft_ev> d_fev;
    DevBuf<uint64_t> d_finfo;
    DevBuf<uint8_t> d_fto;
    PinBuf<uint8_t> h_flw;                   // the pinned block (k_ft_out writes it)
    View<uint64_t> h_finfo;
    View<uint32_t> h_flow;
    View<uint8_t> h_fto;
    View<emurx_ft_ev> h_fev;
    void release() {
        if (st) (void)hipStreamSynchronize(st);
        d_flow.release(); d_fev.release(); d_finfo.release(); d_fto.release(); h_flw.release();
        d_pev.release(); d_pinfo.release(); d_pngo.release(); h_png.release();
        d_rsp_out.release(); d_tx.release(); d_rsp_desc.release(); d_rsp_src.release(); d_tx_off.release();
        d_ainfo.release(); d_lev.release(); d_nsev.release(); h_ans.release();
        d_qseg.release(); d_tcnt.release(); d_ticket.release(); d_hsmall.release(); h_done.release();
        h_buf.release(); h_ctl.release(); h_mframes.release(); h_mstatus.release(); h_res.release();
        d_buf.release(); d_ctl.release(); d_qlist.release(); d_tile_cnt.release(); d_seg_off.release();
        d_hist.release(); d_res.release();
        if (done) (void)hipEventDestroy(done);
        if (st) (void)hipStreamDestroy(st);
        done = nullptr;
        st = nullptr;
        pending = false;
    }
};

// One in-flight batch of outgoing frames (emurx_egress_*): the caller's pinned frame area and
// descriptors, their device copies, the chain's device outputs and the pinned result block that
// k_egr_out writes.  Everything is sized once, by the slot's first emurx_egress_buffer, for
// cfg.max_frames and cfg.max_bytes.
struct EgressSlot {
    hipStream_t st = nullptr;
    hipEvent_t done = nullptr;
    bool pending = false, submitted = false;
    uint32_t n = 0;             // frames of the batch in flight / last waited for
    uint64_t tx_cap = 0;        // its out_cap: 8 n + bytes
    uint64_t cap = 0;           // message bytes the blocks hold: 8 max_frames + max_bytes, whole vectors
    PinBuf<uint8_t> h_frames;   // written by the caller (+64 B pad)
    PinBuf<emurx_desc> h_desc;  // written by the caller
    DevBuf<uint8_t> d_frames, d_plan, d_status, d_tx;
    DevBuf<emurx_desc> d_desc;
    DevBuf<emurx_tx_desc> d_txd;
    DevBuf<uint64_t> d_msg_off, d_info;  // d_info: the planner's info words, then the framing's two
    PinBuf<uint8_t> h_res;               // the pinned result block
    View<uint64_t> h_head, h_msg_off;
    View<uint8_t> h_plan, h_status, h_tx;
    // echo requests behind the plain frames (emurx_egress_ping_buffer / _submit_ping)
    PinBuf<emurx_pingtx_req> h_req;      // written by the caller
    DevBuf<emurx_pingtx_req> d_req;
    DevBuf<uint64_t> d_pinfo;            // the generator's info words (the submit's sizes are exact: not read)
    uint64_t ping_seq = 0, ping_done = 0;  // batches with requests submitted / waited for (PingTx::limbo)
    void release() {
        if (st) (void)hipStreamSynchronize(st);
        h_req.release(); d_req.release(); d_pinfo.release();
        h_frames.release(); h_desc.release(); h_res.release();
        d_frames.release(); d_plan.release(); d_status.release(); d_tx.release(); d_desc.release(); d_txd.release();
        d_msg_off.release(); d_info.release();
        if (done) (void)hipEventDestroy(done);
        if (st) (void)hipStreamDestroy(st);
        done = nullptr;
        st = nullptr;
        pending = false;
    }
};

// one staging slot of the table-delta ring: pinned entries, read by k_apply over the bus
// (no copy launch: a delta is a few KiB)
struct DeltaSlot {
    PinBuf<emurx_delta> h;
    hipEvent_t ev = nullptr;  // recorded after the k_apply that read h
    bool used = false;
};
constexpr int kDeltaRing = 4;
constexpr size_t kMaxReaders = 16;

// The resident ping templates (emurx_pingtx_*).  The shadow is the host's truth; an edit marks its
// id, and the marked slots travel ahead of the next launch that reads the store (ship_pingtx) as
// 272-byte entries in a ring of pinned buffers that one k_ptx_apply launch reads directly, like the
// table deltas.  Everything is sized by emurx_pingtx_reserve: the vectors below never grow.
struct PingTx {
    static constexpr uint32_t kEntry = 16 + EMURX_PINGTX_SLOT;  // {id, zeros}, the slot
    uint32_t max = 0;                    // 0: not reserved
    DevBuf<uint8_t> d_store;             // max slots + 16 bytes (a slot's last chunk is read whole)
    std::vector<uint8_t> shadow;         // max slots
    std::vector<uint16_t> len;           // per id, 0: free
    std::vector<uint8_t> marked;         // per id: in `dirty`
    std::vector<uint32_t> dirty;         // ids edited since the last shipment
    std::vector<uint32_t> free_ids;      // min-heap of the ids that may be handed out
    // removed ids wait here, in removal order, until every egress batch with requests that was
    // submitted before the remove has been waited for: seq = the slots' ping_seq at the remove
    struct Limbo {
        uint32_t id;
        uint64_t seq[EMURX_EGRESS_SLOTS];
    };
    std::vector<Limbo> limbo;            // ring of max entries
    uint32_t limbo_head = 0, limbo_n = 0;
    // the shipment: staging ring, the streams that read the store since the last shipment, and
    // which shipment every stream has waited for (the table shipment's bookkeeping)
    uint32_t stage_cap = 0;              // entries per staging buffer
    PinBuf<uint8_t> stage[kDeltaRing];
    hipEvent_t stage_ev[kDeltaRing] = {};
    bool stage_used[kDeltaRing] = {};
    uint32_t stage_i = 0;
    hipEvent_t ship_ev = nullptr, reader_ev[kMaxReaders] = {};
    uint64_t ship_gen = 0;
    std::vector<hipStream_t> readers;
    std::vector<std::pair<hipStream_t, uint64_t>> waited;
    // the generator's scratch, sized for cfg.max_frames requests, handed from call to call by event
    DevBuf<uint8_t> d_scratch;
    hipEvent_t scr_ev = nullptr;
    bool scr_recorded = false;
    void release() {
        d_store.release();
        d_scratch.release();
        for (int k = 0; k < kDeltaRing; ++k) {
            stage[k].release();
            if (stage_ev[k]) (void)hipEventDestroy(stage_ev[k]);
            stage_ev[k] = nullptr;
        }
        for (auto& e : reader_ev) {
            if (e) (void)hipEventDestroy(e);
            e = nullptr;
        }
        if (ship_ev) (void)hipEventDestroy(ship_ev);
        if (scr_ev) (void)hipEventDestroy(scr_ev);
        ship_ev = scr_ev = nullptr;
        max = 0;
    }
};

}  // namespace

struct emurx_ctx {
    emurx_cfg cfg{};
    bool host_only = false;  // cfg.device < 0: the table mirror alone, no HIP calls
    hipStream_t stream = nullptr;
    uint32_t cb_mask = 0;  // Parser.Init: every callback parserNotSupported (eapol nil)

    Mirror m;  // Go maps + device table images (emurx_mirror.h)

    // device tables: the 8 hash images (emurx_host::kTab*) and the dense ns info
    DevBuf<uint32_t> d_tab[emurx_host::kNumTabs];
    DevBuf<uint32_t> d_nsinfo;
    // table shipment: delta ring, the streams that read the tables since the last shipment,
    // and which shipment every stream has waited for
    DeltaSlot ring[kDeltaRing];
    uint32_t ring_i = 0;
    hipEvent_t ship_ev = nullptr;
    uint64_t ship_gen = 0;
    std::vector<hipStream_t> readers;
    std::vector<hipEvent_t> reader_ev;
    std::vector<std::pair<hipStream_t, uint64_t>> waited;
    uint64_t shipped_blocks = 0, shipped_whole = 0;  // counters (emurx_table_stats)

    // batched host ingest: EMURX_INGEST_SLOTS public slots + one private to emurx_rx_stream
    IngestSlot ing[EMURX_INGEST_SLOTS + 1];
    bool ingest_small = true;  // small batches in one launch (k_ingest_small); EMURX_INGEST_SMALL=0: never
    bool ingest_spin = true;   // wait for them on their completion word; EMURX_INGEST_SPIN=0: on the event
    // the one-launch path's bounds: its tiles must all be resident (the device's capacity for
    // k_ingest_small, measured at emurx_open), and a workgroup waits for the others at most
    // EMURX_INGEST_SPIN_US (default 200 us) plus 0.1 ns per byte of the batch's messages (the
    // tiles read them over PCIe at 20-50 GB/s, so a bigger batch's tiles arrive further apart:
    // at most 1.2 ms for the largest one-launch batch); 0 forces the degraded pack (tests)
    uint32_t small_tiles = EMURX_SMALL_TILES;
    double spin_base_us = 200.0;
    uint32_t wall_khz = 100000;  // the GPU's wall clock (hipDeviceAttributeWallClockRate)

    // tx ZMQ framing scratch (emurx_tx_zmq_dev): per-level chain transfer tables
    DevBuf<uint8_t> d_txz;
    // the tx write kernel's image per call (EMURX_TXZ_*), from the bounds of the tiles' output
    // rows an earlier call's chain kernel folded into two scratch words: copied back behind that
    // call (an event, no synchronisation) as the staging slab's feedback is, the first call and
    // then at most every txz_every-th (8, doubled when a decision repeats, up to 256).  Every
    // image writes every tile correctly; the choice is speed only.  EMURX_TXZ=wide|narrow|long
    // forces one.
    PinBuf<uint32_t> txz_fb;
    hipEvent_t txz_ev = nullptr;
    bool txz_pending = false;
    int txz_variant = EMURX_TXZ_WIDE, txz_mode = -1;
    uint32_t txz_calls = 0, txz_last_copy = 0, txz_every = 8, txz_same = 0;
    int last_txz = -1;
    // the device responder's scratch (emurx_respond_dev): plans and tile sums, no state between calls
    DevBuf<uint8_t> d_rsp;
    // the cache-learning fold's scratch (emurx_learn_dev), sized at emurx_open from max_frames: its
    // set is zero between calls; a call whose launches failed half way leaves it to be cleared
    DevBuf<uint8_t> d_lrn;
    bool lrn_dirty = false;
    // the per-Namespace counter fold's scratch (emurx_nsstat_dev), sized at emurx_open from max_frames
    // and max_ns: its accumulator rows and flags are zero between calls, cleared like the learning set
    DevBuf<uint8_t> d_nss;
    bool nss_dirty = false;
    // the ping fold's scratch (emurx_ping_dev), sized at emurx_open from max_frames: its accumulator
    // rows and its set are zero between calls, cleared like the learning set
    DevBuf<uint8_t> d_png;
    bool png_dirty = false;
    // the scratch of the fold of refused TCP / UDP frames (emurx_ftstat_dev), sized at emurx_open from
    // max_frames: its accumulator rows and its set are zero between calls, cleared like the learning set
    DevBuf<uint8_t> d_fts;
    bool fts_dirty = false;
    // the answer and flow stages of ingest slots (emurx_ingest_set_answers, _set_flows) share the scratches above:
    // each stage waits for the previous one's event and records its own
    hipEvent_t ans_ev = nullptr;
    bool ans_recorded = false;
    // egress slots (emurx_egress_*): their framing uses d_txz and joins the same hand-off
    EgressSlot egr[EMURX_EGRESS_SLOTS];
    // the resident ping templates and their generator (emurx_pingtx_*)
    PingTx ptx;

    // Namespace-partition packing scratch (emurx_route_dev / emurx_classify_route_dev /
    // emurx_parse_route_dev): one set per stream, so routes of batches pipelined over several
    // streams run side by side; past kRouteSets streams a set changes hands behind an event
    struct RouteScratch {
        hipStream_t st = nullptr;
        bool used = false;
        hipEvent_t done = nullptr;                      // recorded after each route on st
        DevBuf<uint32_t> cnt, grp, goff;                // grp: zero between batches
        DevBuf<uint32_t> tcur;                          // tail cursors of the partitioned source
        void release() {
            cnt.release(); grp.release(); goff.release(); tcur.release();
            if (done) (void)hipEventDestroy(done);
            done = nullptr;
        }
    };
    static constexpr size_t kRouteSets = 4;
    RouteScratch route[kRouteSets];
    uint32_t route_next = 0;  // the set a new stream takes over when all are in use

    // k_rx staging slab per launch (emurx_launch_batch): the narrow 6 KiB slab runs 6
    // workgroups per CU instead of 5, but a wave whose frames span 6-7 KiB then takes the
    // slower window path.  Sampled tiles report how many of their waves fall in that band
    // into device words; the first launch and then at most every `stage_every`-th copies them to pinned
    // memory behind itself (stream order, an event, no synchronisation), and the first
    // launch after the copy has landed decides.  The kernel
    // writing host memory directly was tried: host reads of lines the GPU keeps writing made
    // some launches 5x slower.  The tight 5 KiB slab runs 7 workgroups per CU (64-byte frames:
    // 4,352 B per wave); a wave over 5 KiB then takes the window path with an 80-byte window,
    // so it is chosen by the same 1 % rule on the waves over 5 KiB, and only at the second
    // decision in a row that sees it eligible, the first of which chose narrow: one sample is
    // too little evidence.  Any decision that sees more than 1 % of the waves over 5 KiB leaves
    // it at once.  EMURX_STAGE=wide|narrow|tight forces one size (tests, A/B).
    // The same sampled waves write a second word each behind the first 256, {gen << 2, lookups
    // uniform << 1, parse uniform}: which of them took the uniform-wave path (emurx_parse.h).
    // EMURX_UNIFORM=0 switches that path off (default on); emurx_last_uniform reads the words
    DevBuf<uint32_t> d_stage_fb;  // 64 sampled tiles x 4 waves: gen << 3 | over_5k << 2 | has_frames << 1 | mid
    bool uniform = true;
    PinBuf<uint32_t> stage_fb;    // its copy
    uint32_t stage_gen = 0, stage_mode = 0;  // 0 auto, 1 wide, 2 narrow, 3 tight
    bool stage_copy = false, stage_pending = false;
    uint32_t stage_copy_gen = 0;
    // launches between copy-backs: 8, doubled after each decision that repeats the one before
    // it (from the second in a row), up to 256; back to 8 when a decision changes the slab.  A
    // copy-back is a blit between two k_rx launches on the caller's stream (it breaks the
    // overlap with the next launch): config B's 20-step command ran 2-3 % slower with one per 8
    uint32_t stage_every = 8, stage_same = 0;
    hipEvent_t stage_ev = nullptr;
    uint32_t stage_bytes = emurx::kStageWide;  // the slab of the next launch (emurx::kStage*)
    bool stage_tight_ok = false;        // the last decision saw the tight slab eligible
    uint32_t last_stage = 0;

    // the Namespace-owner exchange's communicator (emurx_comm.cpp), or none
    emurx_comm_state* comm = nullptr;

    // timing ring: 2 events per batch (around the k_rx launch)
    std::vector<hipEvent_t> ev;
    uint32_t slots = 0, ev_head = 0, ev_count = 0, stride = 1, batch_seq = 0;

    emurx_dev_tables tables() const {
        using namespace emurx_host;
        emurx_dev_tables T{};
        T.ns_tab = d_tab[kTabNs].p;
        T.ns_info = d_nsinfo.p;
        T.mac_tab = d_tab[kTabMac].p;
        T.ip4_tab = d_tab[kTabIp4].p;
        T.ip6_tab = d_tab[kTabIp6].p;
        T.ci_tab = d_tab[kTabCi].p;
        T.ns_mask = m.ns_t.mask();
        T.mac_mask = m.mac_t.mask();
        T.ip4_mask = m.ip4_t.mask();
        T.ip6_mask = m.ip6_t.mask();
        T.ci_mask = m.ci_t.mask();
        T.max_ns = cfg.max_ns;
        T.cb_mask = cb_mask;
        T.ft_on = m.n_ctx ? 1u : 0u;
        T.ft4_tab = d_tab[kTabFt4].p;
        T.ft6_tab = d_tab[kTabFt6].p;
        T.srv_tab = d_tab[kTabSrv].p;
        T.ft4_mask = m.ft4_t.mask();
        T.ft6_mask = m.ft6_t.mask();
        T.srv_mask = m.srv_t.mask();
        return T;
    }
};

namespace {

// every entry point re-binds the handle's device (goroutines migrate between OS threads);
// hipGetDevice is a thread-local read, hipSetDevice only when the thread is elsewhere
int bind(emurx_t* h) {
    if (h->host_only) return EMURX_EDEVICE;
    int cur = -1;
    if (EMURX_HIP_OK(hipGetDevice(&cur)) && cur == h->cfg.device) return EMURX_OK;
    return EMURX_HIP_OK(hipSetDevice(h->cfg.device)) ? EMURX_OK : EMURX_EDEVICE;
}

uint64_t& waited_gen(emurx_t* h, hipStream_t s) {
    for (auto& w : h->waited)
        if (w.first == s) return w.second;
    h->waited.emplace_back(s, 0);
    return h->waited.back().second;
}

// Ship the edited table blocks on `st`: after every stream that read the tables since the
// last shipment (an event recorded on it now, waited on by st), before every later reader
// (ship_ev, waited on by each reader stream once).  Edited blocks travel as emurx_delta
// entries in a ring of pinned buffers that one k_apply launch reads directly.
// Whole images (first upload, a rebuilt or grown table, or a quarter of a table edited)
// are copied synchronously; growing a device table waits for the device first, since
// batches in flight may still read the old buffer.
int ship_tables(emurx_t* h, hipStream_t st) {
    using namespace emurx_host;
    Mirror& m = h->m;
    for (size_t k = 0; k < h->readers.size(); ++k) {
        const hipStream_t r = h->readers[k];
        if (r == st) continue;
        while (h->reader_ev.size() <= k) {  // one event per reader slot (slots skipped above included)
            hipEvent_t e;
            if (!EMURX_HIP_OK(hipEventCreateWithFlags(&e, hipEventDisableTiming))) return EMURX_EDEVICE;
            h->reader_ev.push_back(e);
        }
        if (!EMURX_HIP_OK(hipEventRecord(h->reader_ev[k], r)) || !EMURX_HIP_OK(hipStreamWaitEvent(st, h->reader_ev[k], 0)))
            return EMURX_EDEVICE;
    }
    Blocks* img[kNumTabs + 1];
    DevBuf<uint32_t>* dev[kNumTabs + 1];
    for (int k = 0; k < kNumTabs; ++k) {
        img[k] = m.hashes(k);
        dev[k] = &h->d_tab[k];
    }
    img[kNumTabs] = &m.nsinfo;
    dev[kNumTabs] = &h->d_nsinfo;
    bool whole = false, grow = false;
    size_t nd = 0;
    for (int k = 0; k <= kNumTabs; ++k) {
        if (!img[k]->all && img[k]->dirty.size() * 4 > img[k]->nblocks()) img[k]->all = true;
        whole = whole || img[k]->all;
        grow = grow || (img[k]->all && img[k]->img.size() > dev[k]->n);
        if (!img[k]->all) nd += img[k]->dirty.size();
    }
    if (grow && !EMURX_HIP_OK(hipDeviceSynchronize())) return EMURX_EDEVICE;
    if (whole) {
        if (!EMURX_HIP_OK(hipStreamSynchronize(st))) return EMURX_EDEVICE;
        // a table whose device allocation fails is rebuilt at half its spread and tried again
        // (emurx_cfg: memory traded for lookup latency, down to 2 slots per entry);
        // EMURX_DEBUG_TABLE_LIMIT (bytes) fails every larger allocation, for tests
        static const size_t lim = getenv("EMURX_DEBUG_TABLE_LIMIT") ? strtoull(getenv("EMURX_DEBUG_TABLE_LIMIT"), nullptr, 0)
                                                                     : ~(size_t)0;
        for (int k = 0; k <= kNumTabs; ++k) {
            if (!img[k]->all) continue;
            while (img[k]->img.size() * 4 > lim || dev[k]->alloc(img[k]->img.size())) {
                if (k == kNumTabs || !m.shrink(k)) return EMURX_ENOMEM;
                // the out-of-memory status our own hipMalloc left pending: recovered from here
                if (hipPeekAtLastError() == hipErrorOutOfMemory) (void)hipGetLastError();
            }
            if (!EMURX_HIP_OK(hipMemcpy(dev[k]->p, img[k]->img.data(), img[k]->img.size() * 4, hipMemcpyHostToDevice)))
                return EMURX_EDEVICE;
            h->shipped_whole++;
        }
    }
    if (nd) {
        DeltaSlot& s = h->ring[h->ring_i++ % kDeltaRing];
        if (s.used && !EMURX_HIP_OK(hipEventSynchronize(s.ev))) return EMURX_EDEVICE;
        if (s.h.alloc(nd)) return EMURX_ENOMEM;
        size_t j = 0;
        for (int k = 0; k <= kNumTabs; ++k) {
            if (img[k]->all) continue;
            for (uint32_t b : img[k]->dirty) {
                emurx_delta& e = s.h.p[j++];
                e.dst = (uint64_t)(uintptr_t)(dev[k]->p + (size_t)b * EMURX_BUCKET_WORDS);
                e.pad = 0;
                memcpy(e.w, &img[k]->img[(size_t)b * EMURX_BUCKET_WORDS], sizeof(e.w));
            }
        }
        if (emurx_launch_apply(s.h.p, (uint32_t)nd, st) || !EMURX_HIP_OK(hipEventRecord(s.ev, st)))
            return EMURX_EDEVICE;
        s.used = true;
        h->shipped_blocks += nd;
    }
    m.clean_all();
    if (!EMURX_HIP_OK(hipEventRecord(h->ship_ev, st))) return EMURX_EDEVICE;
    waited_gen(h, st) = ++h->ship_gen;
    h->readers.clear();
    return EMURX_OK;
}

// Before a launch on `st` that reads the tables: ship pending edits, or wait for the last
// shipment if this stream has not yet; remember st as a reader for the next shipment.
int prepare_read(emurx_t* h, hipStream_t st) {
    int rc;
    if (h->m.pending()) {
        if ((rc = ship_tables(h, st))) return rc;
    } else {
        uint64_t& w = waited_gen(h, st);
        if (w < h->ship_gen) {
            if (!EMURX_HIP_OK(hipStreamWaitEvent(st, h->ship_ev, 0))) return EMURX_EDEVICE;
            w = h->ship_gen;
        }
    }
    if (std::find(h->readers.begin(), h->readers.end(), st) == h->readers.end()) {
        if (h->readers.size() >= kMaxReaders) {  // many distinct streams: drain them all once
            if (!EMURX_HIP_OK(hipDeviceSynchronize())) return EMURX_EDEVICE;
            h->readers.clear();
        }
        h->readers.push_back(st);
    }
    if (h->waited.size() > 4 * kMaxReaders) h->waited.clear();  // forgotten streams wait again: harmless
    return EMURX_OK;
}

uint32_t ntiles(uint32_t n) { return (n + EMURX_QUEUE_TILE - 1) / EMURX_QUEUE_TILE; }
size_t queue_cap(uint32_t n) { return (size_t)ntiles(n) * EMURX_QUEUE_TILE; }

// the staging slab of the next k_rx launch in bytes (see emurx_ctx::stage_fb); advances
// stage_gen (29 bits: the feedback word's other three are the wave's facts)
constexpr uint32_t kStageGenMask = 0x1fffffffu;
uint32_t choose_stage_(emurx_t* h) {
    ++h->stage_gen;
    h->stage_gen &= kStageGenMask;
    if (h->stage_mode) return h->stage_mode == 3 ? emurx::kStageTight : h->stage_mode == 2 ? emurx::kStageNarrow : emurx::kStageWide;
    // decide as soon as the last copy-back has landed (an event query, no waiting)
    if (h->stage_pending && hipEventQuery(h->stage_ev) == hipSuccess) {  // "not ready" is no error
        h->stage_pending = false;
        // the sampled waves of the 16 launches up to the copied one (a 1M-frame launch
        // rewrites all 256 words, a small one only the first few)
        uint32_t waves = 0, mid = 0, over = 0;
        for (int i = 0; i < 256; ++i) {
            const uint32_t w = h->stage_fb.p[i];
            const uint32_t age = (h->stage_copy_gen - (w >> 3)) & kStageGenMask;
            if ((w >> 3) && age < 16) {
                waves += (w >> 1) & 1;
                mid += w & 1;
                over += (w >> 2) & 1;
            }
        }
        // a wave in the 6-7 KiB band costs several staged waves on the window path; below
        // 1% of the sampled waves the extra workgroup per CU wins (configs B, E), above it
        // loses (C)
        if (waves) {
            // over counts the band's waves too, so an eligible sample is a narrow one as well
            const bool narrow = mid * 100 <= waves, tight_ok = over * 100 <= waves;
            const uint32_t bytes = !narrow ? emurx::kStageWide
                                   : tight_ok && h->stage_tight_ok ? emurx::kStageTight : emurx::kStageNarrow;
            h->stage_tight_ok = tight_ok;
            if (bytes != h->stage_bytes) {
                h->stage_same = 0;
                h->stage_every = 8;
            } else if (++h->stage_same >= 2 && h->stage_every < 256) {
                h->stage_every *= 2;
            }
            h->stage_bytes = bytes;
        }
    }
    // the first launch and then at most every stage_every-th copies its samples back
    if (!h->stage_pending &&
        (!h->stage_copy_gen || ((h->stage_gen - h->stage_copy_gen) & kStageGenMask) >= h->stage_every))
        h->stage_copy = true;
    return h->stage_bytes;
}
int stage_copy_back(emurx_t* h, hipStream_t st) {
    if (!h->stage_copy) return 0;
    h->stage_copy = false;
    if (!EMURX_HIP_OK(hipMemcpyAsync(h->stage_fb.p, h->d_stage_fb.p, 256 * sizeof(uint32_t), hipMemcpyDeviceToHost, st)) ||
        !EMURX_HIP_OK(hipEventRecord(h->stage_ev, st)))
        return -1;
    h->stage_pending = true;
    h->stage_copy_gen = h->stage_gen;
    return 0;
}
uint32_t choose_stage(emurx_t* h) {
    return h->last_stage = choose_stage_(h);
}

// route scratch of stream st for batches of up to max_frames: per-tile counts, per-group sums
// (kept zero between routes) and group offsets.  A stream keeps its set; a new stream takes a
// free one, or the next in turn after waiting (on the device) for its last route.
int route_scratch(emurx_t* h, uint32_t n, hipStream_t st, emurx_t::RouteScratch** out) {
    const size_t gw = 1024 * 16, tiles = std::max<size_t>(ntiles(std::max(n, h->cfg.max_frames)), 1);
    if (tiles > 1024u * 64u) return EMURX_EINVAL;  // 16M frames per batch
    emurx_t::RouteScratch* r = nullptr;
    for (auto& x : h->route)
        if (x.used && x.st == st) r = &x;
    if (!r)
        for (auto& x : h->route)
            if (!r && !x.used) r = &x;
    if (!r) {
        r = &h->route[h->route_next++ % emurx_t::kRouteSets];
        if (!EMURX_HIP_OK(hipStreamWaitEvent(st, r->done, 0))) return EMURX_EDEVICE;
    }
    if (!r->done && !EMURX_HIP_OK(hipEventCreateWithFlags(&r->done, hipEventDisableTiming))) return EMURX_EDEVICE;
    r->st = st;
    r->used = true;
    if (!r->grp.p) {
        if (r->grp.alloc(gw) || !EMURX_HIP_OK(hipMemset(r->grp.p, 0, gw * sizeof(uint32_t)))) return EMURX_ENOMEM;
    }
    if (r->cnt.alloc(tiles * 16) || r->goff.alloc(gw) || r->tcur.alloc(EMURX_MAX_PARTS * EMURX_TAIL_SHARDS * EMURX_TAIL_CURSOR_STRIDE))
        return EMURX_ENOMEM;
    *out = r;
    return EMURX_OK;
}
// after a route's last launch on st: its scratch set may change hands behind this event
int route_done(emurx_t::RouteScratch* r, hipStream_t st) {
    return EMURX_HIP_OK(hipEventRecord(r->done, st)) ? EMURX_OK : EMURX_EDEVICE;
}

// A launch path may ship table edits (k_apply, cross-stream events, a synchronisation for a
// whole or grown table) and bakes the table addresses, which a later growth reallocates, into
// its kernel arguments: it must not be recorded into a hipGraph
int not_capturing(hipStream_t st) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (!EMURX_HIP_OK(hipStreamIsCapturing(st, &cs))) return EMURX_EDEVICE;
    return cs == hipStreamCaptureStatusNone ? EMURX_OK : EMURX_EINVAL;
}

// one k_rx launch; kind: 0 parse only, 1 classify, 2 parse + lookup keys (partitioned source);
// rt: kind 1 the route count pass fused in (emurx_classify_route_dev), kind 2 the packing
// of the lookup records (emurx_parse_route_dev)
int run_dev(emurx_t* h, const uint8_t* frames, const emurx_desc* desc, uint32_t n, const emurx_dev_out* out,
            hipStream_t st, int kind, const emurx_route_args* rt) {
    int rc;
    if ((rc = not_capturing(st))) return rc;
    if (kind == 1 && (rc = prepare_read(h, st))) return rc;
    emurx_dev_tables T = h->tables();
    const hipEvent_t* ev = nullptr;
    if (h->slots && (h->batch_seq++ % h->stride) == 0) {
        const uint32_t s = h->ev_head;
        ev = &h->ev[2 * s];
        h->ev_head = (s + 1) % h->slots;
        h->ev_count = std::min(h->ev_count + 1, h->slots);
    }
    const uint32_t stage = choose_stage(h);
    int r = emurx_launch_batch(frames, desc, n, T, kind, *out, st, ev, stage, h->d_stage_fb.p, h->stage_gen, h->uniform, rt);
    if (!r) r = stage_copy_back(h, st);
    return r ? EMURX_EDEVICE : EMURX_OK;
}

int check_batch_args(emurx_t* h, const uint8_t* frames, const emurx_desc* desc, uint32_t n,
                     const emurx_dev_out* out) {
    if (!h || !out || !out->hist || (n && (!frames || !desc))) return EMURX_EINVAL;
    if (((uintptr_t)frames & 15) || ((uintptr_t)desc & 7)) return EMURX_EINVAL;  // 16-B staging loads
    if (n > h->cfg.max_frames) return EMURX_ENOMEM;
    if (out->qlist && out->qcap < queue_cap(n)) return EMURX_EINVAL;
    return bind(h);
}

// ---- batched ZMQ ingest (emurx_ingest_*; emurx_rx_stream uses the private last slot) ----
int ingest_buffer(emurx_t* h, uint32_t slot, size_t bytes, uint8_t** buf) {
    IngestSlot& s = h->ing[slot];
    if (s.pending || bytes > 0xFFFFFFFFull - 64) return EMURX_EINVAL;
    if (s.h_buf.alloc(bytes + 64) || s.d_buf.alloc(bytes + 64)) return EMURX_ENOMEM;
    *buf = s.h_buf.p;
    return EMURX_OK;
}

// Does a batch fit the one-launch path (k_ingest_small)?  At most EMURX_SMALL_MSGS messages and
// EMURX_SMALL_TILES tiles of descriptor slots, and every tile's messages (those with slots in
// it, and those whose status word it writes: tile min(base / 256, tiles - 1)) within the
// kernel's LDS budget, counted exactly as the kernel stages them: 16-byte vectors from the
// message's aligned start, plus two of slack.
bool small_fits(const uint32_t* ctl, uint32_t nmsg, uint32_t n, uint32_t max_tiles, uint32_t trange[EMURX_SMALL_TILES]) {
    if (nmsg > EMURX_SMALL_MSGS || n > std::min<uint32_t>(max_tiles, EMURX_SMALL_TILES) * EMURX_QUEUE_TILE) return false;
    const uint32_t nt = std::max<uint32_t>(ntiles(n), 1);
    const uint32_t* base = ctl + 2 * (size_t)nmsg;
    uint64_t vec[EMURX_SMALL_TILES] = {0};
    uint32_t lo[EMURX_SMALL_TILES], hi[EMURX_SMALL_TILES];
    for (uint32_t t = 0; t < nt; ++t) lo[t] = UINT32_MAX, hi[t] = 0;
    for (uint32_t m = 0; m < nmsg; ++m) {
        const uint32_t off = ctl[2 * m], len = ctl[2 * m + 1];
        const uint64_t v = len ? (((off & 15u) + (uint64_t)len + 15) >> 4) + 2 : 0;
        const uint32_t b0 = base[m], b1 = base[m + 1], ts = std::min(b0 / EMURX_QUEUE_TILE, nt - 1);
        uint32_t t0 = ts, t1 = ts;
        if (b1 > b0) {
            t0 = std::min(t0, b0 / EMURX_QUEUE_TILE);
            t1 = std::max(t1, std::min((b1 - 1) / EMURX_QUEUE_TILE, nt - 1));
        }
        for (uint32_t t = t0; t <= t1; ++t) {
            vec[t] += v;
            lo[t] = std::min(lo[t], m);
            hi[t] = std::max(hi[t], m);
        }
    }
    for (uint32_t t = 0; t < nt; ++t) {
        if (vec[t] * 16 > EMURX_SMALL_LDS) return false;
        trange[t] = lo[t] == UINT32_MAX ? 0u : lo[t] | ((hi[t] - lo[t] + 1) << 16);
    }
    return true;
}

// the result block of a batch of n descriptor slots and nmsg messages (256-byte aligned parts):
// allocates both copies and points the views into them
int set_results(IngestSlot& s, uint32_t n, uint32_t nmsg, bool answers) {
    // one layout for both copies (and, over no block, for their size)
    auto carve = [&](uint8_t* block, View<emurx_rec>& rec, View<emurx_desc>& desc, View<uint32_t>& q,
                     View<uint32_t>& stat, View<uint32_t>& qoff, View<uint64_t>& hist, View<uint8_t>* fl) {
        emurx_carver c(block);
        rec.p = c.take<emurx_rec>(n);
        desc.p = c.take<emurx_desc>(n);
        q.p = c.take<uint32_t>(n);
        stat.p = c.take<uint32_t>(nmsg);
        qoff.p = c.take<uint32_t>(EMURX_NUM_QUEUES + 1);
        hist.p = c.take<uint64_t>(2 * EMURX_HIST_BINS);
        // a batch with answers: the responder's, the learner's and nsstat's per-frame bytes ride the same copy
        for (int k = 0; k < 3 && answers; ++k) fl[k].p = c.take<uint8_t>(n);
        return c.bytes();
    };
    View<emurx_rec> rec;
    View<emurx_desc> desc;
    View<uint32_t> q, stat, qoff;
    View<uint64_t> hist;
    View<uint8_t> fl[3];
    const size_t total = carve(nullptr, rec, desc, q, stat, qoff, hist, fl);
    if (s.h_res.alloc(total) || s.d_res.alloc(total)) return EMURX_ENOMEM;
    carve(s.h_res.p, s.h_rec, s.h_desc, s.h_qlist, s.h_stat, s.h_qoff, s.h_hist, fl);
    s.h_rspo = fl[0], s.h_lrno = fl[1], s.h_donef = fl[2];
    carve(s.d_res.p, s.d_rec, s.d_desc, s.d_packed, s.d_stat, s.d_qoff, s.d_hist_out, fl);
    s.d_rspo = fl[0], s.d_lrno = fl[1], s.d_donef = fl[2];
    s.res_bytes = total;
    return EMURX_OK;
}

int stage_chain(emurx_t* h, IngestSlot& s, uint32_t n);  // below: the answer stages and the flow stage of a slot

int ingest_submit(emurx_t* h, uint32_t slot, const emurx_msg* msgs, uint32_t nmsg) {
    IngestSlot& s = h->ing[slot];
    if (s.pending || (nmsg && (!msgs || !s.h_buf.p))) return EMURX_EINVAL;
    int rc = bind(h);
    if (rc) return rc;
    if (!s.st && !EMURX_HIP_OK(hipStreamCreateWithFlags(&s.st, hipStreamNonBlocking))) return EMURX_EDEVICE;
    if (!s.done && !EMURX_HIP_OK(hipEventCreateWithFlags(&s.done, hipEventDisableTiming))) return EMURX_EDEVICE;
    const size_t cap = s.h_buf.p ? s.h_buf.n - 64 : 0;
    if (s.h_ctl.alloc((size_t)3 * nmsg + 1)) return EMURX_ENOMEM;
    uint32_t* ctl = s.h_ctl.p;
    uint32_t* base = ctl + 2 * (size_t)nmsg;
    uint64_t S = 0;
    size_t end = 0;
    for (uint32_t m = 0; m < nmsg; ++m) {
        const uint64_t e = (uint64_t)msgs[m].off + msgs[m].len;
        if (e > cap) return EMURX_EINVAL;
        end = std::max<size_t>(end, (size_t)e);
        ctl[2 * m] = msgs[m].off;
        ctl[2 * m + 1] = msgs[m].len;
        base[m] = (uint32_t)S;
        // descriptor slots: the frames the header announces, at most one per 4 bytes of the
        // first 64 KiB (the uint16 running offset never passes 65535 on an accepted frame)
        const uint8_t* p = s.h_buf.p + msgs[m].off;
        const uint32_t len = msgs[m].len;
        if (len >= 4 && (be32(p) >> 16) == EMURX_ZMQ_MAGIC)
            S += std::min<uint32_t>(be32(p) & 0xffff, (std::min<uint32_t>(len, 65536) - 4) / 4);
        if (S > h->cfg.max_frames) return EMURX_ENOSPC;
    }
    base[nmsg] = (uint32_t)S;
    const uint32_t kinds = s.ans_kinds;
    const bool flows = s.flw_on;
    if ((kinds || flows) && end > h->cfg.max_bytes) return EMURX_ENOSPC;  // the stages' buffers are sized for max_bytes
    const uint32_t n = (uint32_t)S, nt = ntiles(n);
    const size_t qcap = std::max<size_t>(queue_cap(n), EMURX_QUEUE_TILE);
    const size_t hw = (size_t)EMURX_HIST_SHARDS * 2 * EMURX_HIST_BINS;
    const bool fresh_hist = !s.d_hist.p;
    if (s.d_ctl.alloc((size_t)3 * nmsg + 1) || s.d_qlist.alloc(EMURX_NUM_QUEUES * qcap) ||
        s.d_tile_cnt.alloc((size_t)std::max<uint32_t>(nt, 1) * 16) ||
        s.d_seg_off.alloc((size_t)std::max<uint32_t>(nt, 1) * 16) || s.d_hist.alloc(hw) || set_results(s, n, nmsg, kinds != 0) ||
        s.h_mframes.alloc(nmsg) || s.h_mstatus.alloc(nmsg))
        return EMURX_ENOMEM;
    hipStream_t st = s.st;
    if ((rc = prepare_read(h, st))) return rc;  // table deltas ordered against every reader
    // the pipeline's histogram shards start zeroed (k_qscan leaves them zero)
    if (fresh_hist && !EMURX_HIP_OK(hipMemsetAsync(s.d_hist.p, 0, hw * sizeof(uint64_t), st))) return EMURX_EDEVICE;
    uint32_t trange[EMURX_SMALL_TILES];
    // (a batch with answers or flows takes the pipeline: the one-launch path leaves no frame in device memory)
    if (h->ingest_small && !kinds && !flows && small_fits(ctl, nmsg, n, h->small_tiles, trange)) {
        // one launch: control words and messages read from the pinned buffers, every result
        // written into the pinned result buffers (no copies)
        if (!s.d_ticket.p) {
            if (s.d_qseg.alloc((size_t)EMURX_SMALL_TILES * EMURX_NUM_QUEUES * EMURX_QUEUE_TILE) ||
                s.d_tcnt.alloc((size_t)EMURX_SMALL_TILES * 16) || s.d_hsmall.alloc(2 * EMURX_HIST_BINS) ||
                s.h_done.alloc(1) || s.d_ticket.alloc(3))
                return EMURX_ENOMEM;
            *(volatile uint32_t*)s.h_done.p = s.seq;
            if (!EMURX_HIP_OK(hipMemsetAsync(s.d_hsmall.p, 0, 2 * EMURX_HIST_BINS * sizeof(uint64_t), st)) ||
                !EMURX_HIP_OK(hipMemsetAsync(s.d_ticket.p, 0, 3 * sizeof(uint32_t), st)))
                return EMURX_EDEVICE;
        }
        if (emurx_launch_ingest_small(s.h_buf.p, ctl, nmsg, n, h->tables(), s.h_rec.p, s.h_desc.p, s.h_qlist.p,
                                      s.h_stat.p, s.h_qoff.p, s.h_hist.p, s.d_qseg.p, s.d_tcnt.p, s.d_hsmall.p,
                                      s.d_ticket.p, s.h_done.p, (s.seq + 1) & 0x7fffffffu,
                                      h->spin_base_us > 0 ? (uint32_t)((h->spin_base_us + 1e-4 * (double)end) * h->wall_khz / 1000.0) : 0u,
                                      trange, st) ||
            !EMURX_HIP_OK(hipEventRecord(s.done, st)))
            return EMURX_EDEVICE;
        s.seq = (s.seq + 1) & 0x7fffffffu;  // bit 31 of the completion word: the batch was degraded
        s.small = true;
        s.ans_batch = 0;
        s.png_batch = 0;
        s.flw_batch = false;
        s.pending = true;
        s.nmsg = nmsg;
        s.slots = n;
        return EMURX_OK;
    }
    const auto H2D = hipMemcpyHostToDevice, D2H = hipMemcpyDeviceToHost;
    bool ok = EMURX_HIP_OK(hipMemcpyAsync(s.d_ctl.p, ctl, ((size_t)3 * nmsg + 1) * 4, H2D, st));
    if (end) ok = ok && EMURX_HIP_OK(hipMemcpyAsync(s.d_buf.p, s.h_buf.p, end, H2D, st));
    if (!ok) return EMURX_EDEVICE;
    if (emurx_launch_zmq_walk(s.d_buf.p, s.d_ctl.p, nmsg, s.d_desc.p, s.d_stat.p, st)) return EMURX_EDEVICE;
    if (n) {
        const emurx_dev_out o{s.d_rec.p, s.d_qlist.p, (uint32_t)qcap, s.d_tile_cnt.p, s.d_hist.p, flows ? s.d_flow.p : nullptr};
        const uint32_t stage = choose_stage(h);
        if (emurx_launch_batch(s.d_buf.p, s.d_desc.p, n, h->tables(), true, o, st, nullptr, stage,
                               h->d_stage_fb.p, h->stage_gen, h->uniform) ||
            stage_copy_back(h, st))
            return EMURX_EDEVICE;
    }
    if (emurx_launch_queue_pack(s.d_qlist.p, (uint32_t)qcap, s.d_tile_cnt.p, n, s.d_seg_off.p, s.d_packed.p,
                                s.d_qoff.p, s.d_hist.p, s.d_hist_out.p, st))
        return EMURX_EDEVICE;
    if ((kinds || flows) && (rc = stage_chain(h, s, n))) return rc;
    // every result in one copy: records, descriptors, packed queues, status, qoff, histogram
    ok = EMURX_HIP_OK(hipMemcpyAsync(s.h_res.p, s.d_res.p, s.res_bytes, D2H, st)) &&
         EMURX_HIP_OK(hipEventRecord(s.done, st));
    if (!ok) return EMURX_EDEVICE;
    s.small = false;
    s.ans_batch = kinds;
    s.png_batch = kinds ? s.png_fams : 0;
    s.flw_batch = flows;
    s.pending = true;
    s.nmsg = nmsg;
    s.slots = n;
    return EMURX_OK;
}

// The small path's completion: spin on the pinned word k_ingest_small writes after every result
// (a few microseconds sooner than the end-of-kernel signal hipEventSynchronize waits for).
// Bounded: after 2 ms the caller waits on the event, which also reports a failed kernel.
bool spin_done(const uint32_t* word, uint32_t seq) {
    const volatile uint32_t* w = word;
    const auto t0 = std::chrono::steady_clock::now();
    for (uint32_t k = 1;; ++k) {
        if ((*w & 0x7fffffffu) == seq) {
            std::atomic_thread_fence(std::memory_order_acquire);
            return true;
        }
#if defined(__x86_64__)
        __builtin_ia32_pause();
#endif
        if ((k & 255) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) return false;
    }
}

int ingest_wait(emurx_t* h, uint32_t slot, emurx_ingest_result* res) {
    IngestSlot& s = h->ing[slot];
    if (!s.pending) return EMURX_EINVAL;
    int rc = bind(h);
    if (rc) return rc;
    s.pending = false;
    s.waited = true;
    const uint32_t ans = s.ans_batch, png = s.png_batch;
    const bool flw = s.flw_batch;
    s.ans_batch = s.png_batch = 0;  // set again below, once the answers are checked and renumbered
    s.flw_batch = false;
    if (!(s.small && h->ingest_spin && spin_done(s.h_done.p, s.seq)) && !EMURX_HIP_OK(hipEventSynchronize(s.done)))
        return EMURX_EDEVICE;
    memset(res, 0, sizeof(*res));
    emurx_counters& d = res->delta;
    d.rx_batch = s.nmsg;  // one OnRxStream per message, veth_zmq.go:278
    uint64_t nf = 0;
    for (uint32_t m = 0; m < s.nmsg; ++m) {
        const uint32_t w = s.h_stat.p[m], f = w & 0xffffff, e = w >> 24;
        s.h_mframes.p[m] = f;
        s.h_mstatus.p[m] = (uint8_t)e;
        nf += f;
        if (e == EMURX_MSG_PARSE_ERR) d.rx_parse_err++;
        if (e == EMURX_MSG_PANIC) d.ref_panic++;
    }
    if (nf > s.slots) return EMURX_EDEVICE;
    if (nf < s.slots) {  // messages that announced more frames than they carried: close the holes
        const uint32_t* base = s.h_ctl.p + 2 * (size_t)s.nmsg;
        s.remap.assign(s.slots, EMURX_ID_NONE);
        uint32_t c = 0;
        for (uint32_t m = 0; m < s.nmsg; ++m) {
            const uint32_t f = s.h_mframes.p[m];
            if (c != base[m] && f) {
                memmove(s.h_rec.p + c, s.h_rec.p + base[m], (size_t)f * sizeof(emurx_rec));
                memmove(s.h_desc.p + c, s.h_desc.p + base[m], (size_t)f * sizeof(emurx_desc));
                for (View<uint8_t>* v : {&s.h_rspo, &s.h_lrno, &s.h_donef})
                    if (ans) memmove(v->p + c, v->p + base[m], f);
                if (png) memmove(s.h_pngo.p + c, s.h_pngo.p + base[m], f);
                if (flw) {
                    memmove(s.h_fto.p + c, s.h_fto.p + base[m], f);
                    memmove(s.h_flow.p + c, s.h_flow.p + base[m], (size_t)f * sizeof(uint32_t));
                }
            }
            for (uint32_t k = 0; k < f; ++k) s.remap[base[m] + k] = c + k;
            c += f;
        }
        for (uint64_t i = 0; i < nf; ++i) {
            const uint32_t j = s.h_qlist.p[i];
            if (j >= s.slots || s.remap[j] == EMURX_ID_NONE) return EMURX_EDEVICE;
            s.h_qlist.p[i] = s.remap[j];
        }
    }
    if (ans) {
        // the counts k_ans_out copied by are the head's, clamped to the block's capacities: a count
        // past its capacity (the sizing argument of emurx_ingest_set_answers broken) fails the batch
        const uint64_t* hd = s.h_ahead.p;
        const uint64_t nrep = hd[0], nlrn = hd[EMURX_ANS_HEAD_LRN], nns = hd[EMURX_ANS_HEAD_NSS],
                       ntx = hd[EMURX_ANS_HEAD_TX], txb = hd[EMURX_ANS_HEAD_TX + 1];
        if (nrep > s.ans_r_cap || ntx > s.ans_r_cap || txb > s.ans_tx_cap || nlrn > s.ans_ev_cap || nns > s.ans_ns_cap)
            return EMURX_EDEVICE;
        // slot numbers -> the closed numbering (monotone: ascending `last` survives)
        auto closed = [&](uint32_t& j) {
            if (j >= s.slots || s.remap[j] == EMURX_ID_NONE) return false;
            j = s.remap[j];
            return true;
        };
        if (nf < s.slots) {
            for (uint64_t k = 0; k < nrep; ++k)
                if (!closed(s.h_src.p[k])) return EMURX_EDEVICE;
            for (uint64_t k = 0; k < nlrn; ++k)
                if (!closed(s.h_lev.p[k].first) || !closed(s.h_lev.p[k].last)) return EMURX_EDEVICE;
        }
        if (png) {
            const uint64_t npng = s.h_pinfo.p[0];
            if (npng > s.png_ev_cap) return EMURX_EDEVICE;
            for (uint64_t k = 0; k < npng && nf < s.slots; ++k)
                if (!closed(s.h_pev.p[k].first) || !closed(s.h_pev.p[k].last)) return EMURX_EDEVICE;
            s.png_batch = png;
        }
        s.ans_batch = ans;
    }
    if (flw) {
        const uint64_t nev = s.h_finfo.p[0];
        if (nev > s.flw_ev_cap) return EMURX_EDEVICE;
        for (uint64_t k = 0; k < nev && nf < s.slots; ++k) {  // slot numbers -> the closed numbering (monotone)
            for (uint32_t* j : {&s.h_fev.p[k].first, &s.h_fev.p[k].last}) {
                if (*j >= s.slots || s.remap[*j] == EMURX_ID_NONE) return EMURX_EDEVICE;
                *j = s.remap[*j];
            }
        }
        s.flw_batch = true;
    }
    memcpy(res->qoff, s.h_qoff.p, sizeof(res->qoff));
    if (res->qoff[EMURX_NUM_QUEUES] != nf) return EMURX_EDEVICE;
    res->one_launch = s.small ? 1u : 0u;
    res->degraded = s.small ? (*(volatile uint32_t*)s.h_done.p >> 31) : 0u;
    emurx_hist_to_counters(s.h_hist.p, &d);
    d.rx_pkts = nf;  // VethIFZmq.OnRx veth_zmq.go:233-234
    for (int b = 0; b < EMURX_HIST_BINS; ++b) d.rx_bytes += s.h_hist.p[2 * b + 1];
    res->rec = s.h_rec.p;
    res->desc = s.h_desc.p;
    res->qlist = s.h_qlist.p;
    res->msg_frames = s.h_mframes.p;
    res->msg_status = s.h_mstatus.p;
    res->n_frames = (uint32_t)nf;
    res->n_msgs = s.nmsg;
    return EMURX_OK;
}

}  // namespace

// handle internals for emurx_comm.cpp (emurx_kernels.h)
int emurx_handle_bind(emurx_t* h) { return bind(h); }
int emurx_handle_device(const emurx_t* h) { return h->host_only ? -1 : h->cfg.device; }
hipStream_t emurx_handle_stream(emurx_t* h) { return h->stream; }
emurx_comm_state*& emurx_handle_comm(emurx_t* h) { return h->comm; }

extern "C" {

int emurx_abi_version(void) { return EMURX_ABI_VERSION; }

const char* emurx_strerror(int code) {
    switch (code) {
    case EMURX_OK: return "ok";
    case EMURX_EINVAL: return "invalid argument";
    case EMURX_ENOMEM: return "out of memory / capacity exceeded";
    case EMURX_EEXIST: return "already exists";
    case EMURX_ENOENT: return "not found";
    case EMURX_EDEVICE: return "HIP runtime error";
    case EMURX_ENOSPC: return "output buffer too small";
    case EMURX_ECOMM: return "RCCL communication error";
    default: return "unknown error";
    }
}

int emurx_open(const emurx_cfg* cfg, emurx_t** out) {
    if (!cfg || !out || cfg->max_ns == 0 || cfg->max_clients == 0 || cfg->max_frames == 0) return EMURX_EINVAL;
    emurx_t* h = new (std::nothrow) emurx_ctx();
    if (!h) return EMURX_ENOMEM;
    h->cfg = *cfg;
    if (h->cfg.max_bytes == 0) h->cfg.max_bytes = 1u << 20;
    h->host_only = cfg->device < 0;
    try {
        h->m.open(cfg->max_ns, cfg->max_clients);
    } catch (...) {
        delete h;
        return EMURX_ENOMEM;
    }
    if (h->host_only) {
        *out = h;
        return EMURX_OK;
    }
    int rc = bind(h);
    if (rc) { delete h; return rc; }
    if (!EMURX_HIP_OK(hipStreamCreate(&h->stream))) { delete h; return EMURX_EDEVICE; }
    if (const char* e = getenv("EMURX_STAGE")) h->stage_mode = !strcmp(e, "wide") ? 1 : !strcmp(e, "narrow") ? 2 : !strcmp(e, "tight") ? 3 : 0;
    if (const char* e = getenv("EMURX_UNIFORM")) h->uniform = strcmp(e, "0") != 0;
    if (const char* e = getenv("EMURX_INGEST_SMALL")) h->ingest_small = strcmp(e, "0") != 0;
    if (const char* e = getenv("EMURX_TXZ"))
        h->txz_mode = !strcmp(e, "wide") ? EMURX_TXZ_WIDE : !strcmp(e, "narrow") ? EMURX_TXZ_NARROW
                    : !strcmp(e, "long") ? EMURX_TXZ_LONG : -1;
    if (const char* e = getenv("EMURX_INGEST_SPIN")) h->ingest_spin = strcmp(e, "0") != 0;
    {
        // the one-launch ingest's wait bound in wall-clock ticks, and its grid cap
        int khz = 100000;
        if (EMURX_HIP_OK(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, cfg->device)) && khz > 0)
            h->wall_khz = (uint32_t)khz;
        if (const char* e = getenv("EMURX_INGEST_SPIN_US")) h->spin_base_us = std::min(std::max(0.0, strtod(e, nullptr)), 1e6);
        const uint32_t cap = emurx_ingest_small_capacity(cfg->device);
        h->small_tiles = std::min<uint32_t>(EMURX_SMALL_TILES, cap);
    }
    if (h->stage_fb.alloc(256) || h->d_stage_fb.alloc(3 * emurx::kFbWords) ||
        !EMURX_HIP_OK(hipEventCreateWithFlags(&h->stage_ev, hipEventDisableTiming)) ||
        !EMURX_HIP_OK(hipEventCreateWithFlags(&h->ship_ev, hipEventDisableTiming)) ||
        !EMURX_HIP_OK(hipMemset(h->d_stage_fb.p, 0, 3 * emurx::kFbWords * sizeof(uint32_t)))) {
        emurx_close(h);
        return EMURX_ENOMEM;
    }
    for (auto& s : h->ring)
        if (!EMURX_HIP_OK(hipEventCreateWithFlags(&s.ev, hipEventDisableTiming))) {
            emurx_close(h);
            return EMURX_EDEVICE;
        }
    memset(h->stage_fb.p, 0, 256 * sizeof(uint32_t));
    if (h->d_lrn.alloc(emurx_lrn_scratch_bytes(cfg->max_frames)) ||
        !EMURX_HIP_OK(hipMemset(h->d_lrn.p, 0, (size_t)emurx_lrn_slots(cfg->max_frames) * 16))) {
        emurx_close(h);
        return EMURX_ENOMEM;
    }
    if (h->d_nss.alloc(emurx_nss_scratch_bytes(cfg->max_frames, cfg->max_ns)) ||
        !EMURX_HIP_OK(hipMemset(h->d_nss.p, 0, emurx_nss_scratch_bytes(cfg->max_frames, cfg->max_ns)))) {
        emurx_close(h);
        return EMURX_ENOMEM;
    }
    if (h->d_png.alloc(emurx_png_scratch_bytes(cfg->max_frames)) ||
        emurx_png_scratch_clear(h->d_png.p, cfg->max_frames, h->stream) || !EMURX_HIP_OK(hipStreamSynchronize(h->stream))) {
        emurx_close(h);
        return EMURX_ENOMEM;
    }
    if (h->d_fts.alloc(emurx_ft_scratch_bytes(cfg->max_frames)) ||
        emurx_ft_scratch_clear(h->d_fts.p, cfg->max_frames, h->stream) || !EMURX_HIP_OK(hipStreamSynchronize(h->stream))) {
        emurx_close(h);
        return EMURX_ENOMEM;
    }
    emurx_t::RouteScratch* rs = nullptr;
    if ((rc = ship_tables(h, h->stream)) || (rc = route_scratch(h, cfg->max_frames, h->stream, &rs)) == EMURX_ENOMEM) {
        emurx_close(h);
        return rc ? rc : EMURX_ENOMEM;
    }
    *out = h;
    return EMURX_OK;
}

void emurx_close(emurx_t* h) {
    if (!h) return;
    if (h->host_only) {
        delete h;
        return;
    }
    bind(h);
    (void)hipDeviceSynchronize();
    emurx_comm_free(h->comm);
    h->comm = nullptr;
    for (auto& s : h->ing) s.release();
    for (auto& s : h->egr) s.release();
    h->ptx.release();
    h->stage_fb.release();
    h->d_stage_fb.release();
    if (h->stage_ev) (void)hipEventDestroy(h->stage_ev);
    if (h->ship_ev) (void)hipEventDestroy(h->ship_ev);
    for (auto& s : h->ring) {
        s.h.release();
        if (s.ev) (void)hipEventDestroy(s.ev);
    }
    for (auto e : h->reader_ev) (void)hipEventDestroy(e);
    for (auto& t : h->d_tab) t.release();
    h->d_nsinfo.release();
    for (auto& r : h->route) r.release();
    h->d_txz.release();
    h->d_rsp.release();
    h->d_lrn.release();
    h->d_nss.release();
    h->d_png.release();
    h->d_fts.release();
    h->txz_fb.release();
    if (h->txz_ev) (void)hipEventDestroy(h->txz_ev);
    if (h->ans_ev) (void)hipEventDestroy(h->ans_ev);
    for (auto& e : h->ev)
        if (e) (void)hipEventDestroy(e);
    h->ev.clear();
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

// Parser.Register parser.go:528-565 (unknown names are ignored, as in Go)
int emurx_register(emurx_t* h, const char* p) {
    if (!h || !p) return EMURX_EINVAL;
    static const struct { const char* name; uint32_t bits; } tab[] = {
        {"arp", 1u << EMURX_CB_ARP},         {"icmp", 1u << EMURX_CB_ICMP},
        {"igmp", 1u << EMURX_CB_IGMP},       {"dhcp", 1u << EMURX_CB_DHCP},
        {"dhcpsrv", 1u << EMURX_CB_DHCPSRV}, {"icmpv6", 1u << EMURX_CB_ICMPV6},
        {"dhcpv6", 1u << EMURX_CB_DHCPV6},   {"dot1x", 1u << EMURX_CB_EAPOL},
        {"mdns", 1u << EMURX_CB_MDNS},       {"ppp", 1u << EMURX_CB_PPP},
        {"transport", (1u << EMURX_CB_TCP) | (1u << EMURX_CB_UDP)}};
    for (auto& t : tab)
        if (!strcmp(p, t.name)) h->cb_mask |= t.bits;
    return EMURX_OK;
}
int emurx_set_callbacks_mask(emurx_t* h, uint32_t mask) {
    if (!h) return EMURX_EINVAL;
    h->cb_mask = mask & ((1u << EMURX_NUM_CB) - 1u);
    return EMURX_OK;
}
uint32_t emurx_get_callbacks_mask(const emurx_t* h) { return h ? h->cb_mask : 0; }

// ---- tables (emurx_mirror.cpp: Go map semantics + device image edits) ----------------------
// CThreadCtx.AddNs / RemoveNs thread_ctx.go:786-812
int emurx_ns_add(emurx_t* h, const uint8_t key[12], uint32_t ns_id, uint32_t plugin_mask) {
    if (!h || !key) return EMURX_EINVAL;
    return h->m.ns_add(key, ns_id, plugin_mask);
}
int emurx_ns_remove(emurx_t* h, const uint8_t key[12]) {
    if (!h || !key) return EMURX_EINVAL;
    return h->m.ns_remove(key);
}
int emurx_ns_set_plugins(emurx_t* h, uint32_t ns_id, uint32_t plugin_mask) {
    if (!h) return EMURX_EINVAL;
    return h->m.ns_set_plugins(ns_id, plugin_mask);
}
// CNSCtx.AddClient ns_ctx.go:332-389
int emurx_client_add(emurx_t* h, uint32_t ns_id, uint32_t cid, const uint8_t mac[6], const uint8_t ipv4[4],
                     const uint8_t ipv6[16], const uint8_t dhcpv6[16], uint32_t plugin_mask) {
    if (!h || !mac) return EMURX_EINVAL;
    return h->m.client_add(ns_id, cid, mac, ipv4, ipv6, dhcpv6, plugin_mask);
}
// ctx_client_add rpc_base_cmds.go:350-406: the listed clients in order, stop at the first error
int emurx_clients_add(emurx_t* h, const emurx_client_spec* c, uint32_t n, uint32_t* n_added) {
    if (!h || (n && !c)) return EMURX_EINVAL;
    uint32_t k = 0;
    int rc = EMURX_OK;
    for (; k < n; ++k)
        if ((rc = h->m.client_add(c[k].ns_id, c[k].client_id, c[k].mac, c[k].ipv4, c[k].ipv6, c[k].dhcpv6,
                                  c[k].plugin_mask)))
            break;
    if (n_added) *n_added = k;
    return rc;
}
// CNSCtx.RemoveClient ns_ctx.go:392-440
int emurx_client_remove(emurx_t* h, uint32_t ns_id, const uint8_t mac[6]) {
    if (!h || !mac) return EMURX_EINVAL;
    return h->m.client_remove(ns_id, mac);
}
int emurx_client_set_plugins(emurx_t* h, uint32_t cid, uint32_t plugin_mask) {
    if (!h) return EMURX_EINVAL;
    return h->m.client_set_plugins(cid, plugin_mask);
}
// CNSCtx.UpdateClientIpv4 / Ipv6 / DIpv6 ns_ctx.go:442-533
int emurx_client_update_ipv4(emurx_t* h, uint32_t cid, const uint8_t ipv4[4]) {
    return h && ipv4 ? h->m.update_addr(cid, 4, ipv4) : EMURX_EINVAL;
}
int emurx_client_update_ipv6(emurx_t* h, uint32_t cid, const uint8_t ipv6[16]) {
    return h && ipv6 ? h->m.update_addr(cid, 6, ipv6) : EMURX_EINVAL;
}
int emurx_client_update_dipv6(emurx_t* h, uint32_t cid, const uint8_t d[16]) {
    return h && d ? h->m.update_addr(cid, 7, d) : EMURX_EINVAL;
}
int emurx_client_set_ra(emurx_t* h, uint32_t cid, const uint8_t prefix[16], uint8_t plen) {
    if (!h || !prefix) return EMURX_EINVAL;
    return h->m.client_set_ra(cid, prefix, plen);
}
// transport flow tables (TransportCtx.addFlowv4/6 / removeFlowv4/6 client_ctx.go:597-651,
// serverCb / lookupServerPort :1142-1155, GetTransportCtx socketApi.go:174-193)
int emurx_flow_add(emurx_t* h, uint32_t cid, const uint8_t* tuple, uint32_t tlen, uint32_t flow_id) {
    return h ? h->m.flow_add(cid, tuple, tlen, flow_id) : EMURX_EINVAL;
}
int emurx_flow_remove(emurx_t* h, uint32_t cid, const uint8_t* tuple, uint32_t tlen) {
    return h ? h->m.flow_remove(cid, tuple, tlen) : EMURX_EINVAL;
}
int emurx_server_add(emurx_t* h, uint32_t cid, uint16_t port, uint8_t proto) {
    return h ? h->m.server_add(cid, port, proto) : EMURX_EINVAL;
}
int emurx_server_remove(emurx_t* h, uint32_t cid, uint16_t port, uint8_t proto) {
    return h ? h->m.server_remove(cid, port, proto) : EMURX_EINVAL;
}
int emurx_client_set_transport(emurx_t* h, uint32_t cid, int has_ctx) {
    return h ? h->m.client_set_transport(cid, has_ctx != 0) : EMURX_EINVAL;
}

int emurx_sync(emurx_t* h, void* stream) {
    if (!h) return EMURX_EINVAL;
    if (h->host_only) return EMURX_OK;  // nothing to ship to
    int rc = bind(h);
    if (rc) return rc;
    return prepare_read(h, stream ? (hipStream_t)stream : h->stream);
}
int emurx_table_stats(const emurx_t* h, uint64_t* delta_blocks, uint64_t* whole_tables, uint64_t* image_bytes) {
    if (!h) return EMURX_EINVAL;
    if (delta_blocks) *delta_blocks = h->shipped_blocks;
    if (whole_tables) *whole_tables = h->shipped_whole;
    if (image_bytes) {
        uint64_t b = h->m.nsinfo.img.size() * 4;
        for (int k = 0; k < emurx_host::kNumTabs; ++k) b += h->m.hashes(k)->img.size() * 4;
        *image_bytes = b;
    }
    return EMURX_OK;
}
int emurx_set_partition(emurx_t* h, uint32_t n_parts, uint32_t part) {
    if (!h || n_parts == 0 || n_parts > EMURX_MAX_PARTS || part >= n_parts) return EMURX_EINVAL;
    h->m.set_partition(n_parts, part);
    return EMURX_OK;
}
uint64_t emurx_table_gen(const emurx_t* h) { return h ? h->m.gen : 0; }
int emurx_recs_stale(const emurx_t* h, const emurx_rec* rec, uint32_t n, uint64_t gen, uint8_t* stale) {
    if (!h || (n && (!rec || !stale))) return EMURX_EINVAL;
    for (uint32_t i = 0; i < n; ++i) stale[i] = h->m.stale(rec[i], gen) ? 1 : 0;
    return EMURX_OK;
}
int emurx_image_lookup(emurx_t* h, uint32_t table, const uint32_t* key, uint32_t* value) {
    if (!h) return EMURX_EINVAL;
    return h->m.image_lookup(table, key, value);
}
int emurx_image_probe(emurx_t* h, uint32_t table, const uint32_t* key, uint32_t out[6]) {
    if (!h) return EMURX_EINVAL;
    return h->m.image_probe(table, key, out);
}
int emurx_image_check(emurx_t* h, uint64_t* mismatched) {
    using namespace emurx_host;
    if (!h || !mismatched) return EMURX_EINVAL;
    int rc = bind(h);
    if (rc) return rc;
    if ((rc = prepare_read(h, h->stream))) return rc;
    if (!EMURX_HIP_OK(hipStreamSynchronize(h->stream))) return EMURX_EDEVICE;
    uint64_t bad = 0;
    std::vector<uint32_t> buf;
    for (int k = 0; k <= kNumTabs; ++k) {
        const Blocks& b = k < kNumTabs ? *h->m.hashes(k) : h->m.nsinfo;
        const DevBuf<uint32_t>& d = k < kNumTabs ? h->d_tab[k] : h->d_nsinfo;
        buf.resize(b.img.size());
        if (b.img.size() > d.n) return EMURX_EDEVICE;
        if (!buf.empty() && !EMURX_HIP_OK(hipMemcpy(buf.data(), d.p, buf.size() * 4, hipMemcpyDeviceToHost)))
            return EMURX_EDEVICE;
        for (size_t i = 0; i < buf.size(); ++i) bad += buf[i] != b.img[i];
    }
    *mismatched = bad;
    return EMURX_OK;
}

// ---- data path ---------------------------------------------------------------------------
// the offset walk of VethIFZmq.OnRxStream veth_zmq.go:277-320 (uint16 running offset)
int emurx_zmq_descriptors(const uint8_t* msg, size_t len, emurx_desc* out, uint32_t cap,
                          uint32_t* n_out, int* parse_err) {
    if (!n_out || !parse_err || (len && !msg)) return EMURX_EINVAL;
    *n_out = 0;
    *parse_err = 0;
    const uint32_t blen = (uint32_t)len;
    if (blen < 4) { *parse_err = 1; return EMURX_OK; }
    uint32_t header = be32(msg);
    if ((header >> 16) != EMURX_ZMQ_MAGIC) { *parse_err = 1; return EMURX_OK; }
    const int pkts = (int)(header & 0xffff);
    uint16_t of = 4;
    for (int i = 0; i < pkts; ++i) {
        if (blen < (uint32_t)(uint16_t)(of + 4)) { *parse_err = 1; return EMURX_OK; }
        if ((uint16_t)(of + 4) < of) { *parse_err = 2; return EMURX_OK; }
        header = be32(msg + of);
        if ((header & 0xff000000u) != 0xAA000000u) { *parse_err = 1; return EMURX_OK; }
        const uint8_t vport = (uint8_t)(header >> 16);
        const uint16_t plen = (uint16_t)header;
        if (blen < (uint32_t)(uint16_t)(of + 4 + plen)) { *parse_err = 1; return EMURX_OK; }
        if (plen > EMURX_MAX_FRAME) { *parse_err = 2; return EMURX_OK; }
        if ((uint16_t)(of + 4 + plen) < (uint16_t)(of + 4)) { *parse_err = 2; return EMURX_OK; }
        if (*n_out >= cap) return EMURX_ENOSPC;
        out[*n_out] = emurx_desc{(uint32_t)(uint16_t)(of + 4), plen, vport, 0};
        ++*n_out;
        of = (uint16_t)(of + 4 + plen);
    }
    return EMURX_OK;
}

void emurx_hist_to_counters(const uint64_t hist[2 * EMURX_HIST_BINS], emurx_counters* c) {
    if (!hist || !c) return;
    uint64_t* s = c->parser;
    for (uint32_t st = 0; st < EMURX_NUM_STATUS; ++st) {
        for (uint32_t cb = 0; cb < (st <= EMURX_ST_NOT_SUPPORTED ? (uint32_t)EMURX_NUM_CB : 1u); ++cb) {
            const uint32_t b = st <= EMURX_ST_NOT_SUPPORTED ? EMURX_HIST_BIN(st, cb) : EMURX_HIST_BIN(st, 0);
            const uint64_t pk = hist[2 * b], by = hist[2 * b + 1];
            if (!pk) continue;
            if (st >= EMURX_ST_PANIC_L4LEN) { c->ref_panic += pk; continue; }
            if (st <= EMURX_ST_NOT_SUPPORTED) {
                switch (cb) {  // parser.go:602-713 / :787-799
                case EMURX_CB_ARP: s[EMURX_PC_arpPkts] += pk; s[EMURX_PC_arpBytes] += by; break;
                case EMURX_CB_ICMP: s[EMURX_PC_icmpPkts] += pk; s[EMURX_PC_icmpBytes] += by; break;
                case EMURX_CB_IGMP: s[EMURX_PC_igmpPkts] += pk; s[EMURX_PC_igmpBytes] += by; break;
                case EMURX_CB_TCP: s[EMURX_PC_tcpPkts] += pk; s[EMURX_PC_tcpBytes] += by; break;
                case EMURX_CB_ICMPV6: s[EMURX_PC_Icmpv6Pkt] += pk; s[EMURX_PC_Icmpv6Bytes] += by; break;
                case EMURX_CB_EAPOL: s[EMURX_PC_eapolPkts] += pk; s[EMURX_PC_eapolBytes] += by; break;
                case EMURX_CB_PPP: break;
                default:
                    s[EMURX_PC_udpPkts] += pk; s[EMURX_PC_udpBytes] += by;
                    if (cb == EMURX_CB_MDNS) { s[EMURX_PC_mDnsPkts] += pk; s[EMURX_PC_mDnsBytes] += by; }
                    if (cb == EMURX_CB_DHCP || cb == EMURX_CB_DHCPV6) { s[EMURX_PC_dhcpPkts] += pk; s[EMURX_PC_dhcpBytes] += by; }
                    if (cb == EMURX_CB_DHCPSRV) { s[EMURX_PC_dhcpSrvPkts] += pk; s[EMURX_PC_dhcpSrvBytes] += by; }
                }
                if (st == EMURX_ST_NOT_SUPPORTED) s[EMURX_PC_errParser] += pk;
                continue;
            }
            static const int err_counter[EMURX_NUM_STATUS] = {
                -1, -1, EMURX_PC_errPacketIsTooShort, EMURX_PC_errEAPolTooShort, EMURX_PC_errArpTooShort,
                EMURX_PC_errDot1qTooShort, EMURX_PC_errToManyDot1q, EMURX_PC_errIPv4TooShort,
                EMURX_PC_errIPv4HeaderTooShort, EMURX_PC_errIPv4Fragment, EMURX_PC_errIPv4cs,
                EMURX_PC_errIPv6TooShort, EMURX_PC_errIPv6HopLimitDrop, EMURX_PC_errIPv6Empty,
                EMURX_PC_errIPv6OptJumbo, EMURX_PC_errIPv6Fragment, EMURX_PC_errIcmpv4TooShort,
                EMURX_PC_errIcmpv4Cse, EMURX_PC_errTcpTooShort, EMURX_PC_tcpCsErr, EMURX_PC_errUdpTooShort,
                EMURX_PC_udpCsErr, EMURX_PC_errIcmpv6TooShort, EMURX_PC_errIcmpv6Cse,
                EMURX_PC_errIcmpv6Unsupported, EMURX_PC_errL4ProtoUnsupported,
                EMURX_PC_errL3ProtoUnsupported, -1, -1, -1, -1};
            s[err_counter[st]] += pk;
            s[EMURX_PC_errParser] += pk;  // HandleRxPacket thread_ctx.go:368-369
        }
    }
}

int emurx_classify_dev(emurx_t* h, const uint8_t* d_frames, const emurx_desc* d_desc, uint32_t n,
                       const emurx_dev_out* out, void* stream) {
    int rc = check_batch_args(h, d_frames, d_desc, n, out);
    if (rc) return rc;
    return run_dev(h, d_frames, d_desc, n, out, stream ? (hipStream_t)stream : h->stream, 1, nullptr);
}
int emurx_parse_dev(emurx_t* h, const uint8_t* d_frames, const emurx_desc* d_desc, uint32_t n,
                    const emurx_dev_out* out, void* stream) {
    int rc = check_batch_args(h, d_frames, d_desc, n, out);
    if (rc) return rc;
    return run_dev(h, d_frames, d_desc, n, out, stream ? (hipStream_t)stream : h->stream, 0, nullptr);
}

int emurx_classify_route_dev(emurx_t* h, const uint8_t* d_frames, const emurx_desc* d_desc, uint32_t n,
                             const emurx_dev_out* out, uint32_t n_parts, uint32_t my_rank, uint32_t cap,
                             emurx_route_rec* d_send, uint32_t* d_send_count, void* stream) {
    int rc = check_batch_args(h, d_frames, d_desc, n, out);
    if (rc) return rc;
    if (!out->rec || !d_send_count || n_parts == 0 || n_parts > EMURX_MAX_PARTS || my_rank >= n_parts ||
        (n && (!d_send || cap == 0)) || ((uintptr_t)d_send & 7))
        return EMURX_EINVAL;
    hipStream_t st = stream ? (hipStream_t)stream : h->stream;
    // before anything is enqueued: nothing of a refused call may end up in the caller's graph
    if ((rc = not_capturing(st))) return rc;
    emurx_t::RouteScratch* rs = nullptr;
    if ((rc = route_scratch(h, n, st, &rs))) return rc;
    const emurx_route_args rt{n_parts, my_rank, cap, rs->cnt.p, rs->grp.p, nullptr, nullptr};
    if (n && (rc = run_dev(h, d_frames, d_desc, n, out, st, 1, &rt))) {
        // k_rx may have added its owner counts into grp before the failure; only k_route_scan
        // clears them, so clear them here or the next route on this set starts from garbage
        (void)hipMemsetAsync(rs->grp.p, 0, rs->grp.n * sizeof(uint32_t), st);
        return rc;
    }
    if (emurx_launch_route(out->rec, n, n_parts, my_rank, cap, d_send, d_send_count, rs->cnt.p, rs->grp.p,
                           rs->goff.p, st, true)) {
        (void)hipMemsetAsync(rs->grp.p, 0, rs->grp.n * sizeof(uint32_t), st);
        return EMURX_EDEVICE;
    }
    return route_done(rs, st);
}

// the whole send / receive buffer of n_parts lookup regions in 32-byte units fits 32 bits (k_rx
// kind 2 addresses heads by such units)
static bool lookup_regions_fit(uint32_t n_parts, uint32_t cap, uint32_t tail_cap) {
    return EMURX_LOOKUP_REGION_BYTES(cap, tail_cap) / 32 * n_parts < (1ull << 32) &&
           (uint64_t)EMURX_TAIL_SHARDS * tail_cap < (1ull << 32) - 4;
}

int emurx_parse_route_dev(emurx_t* h, const uint8_t* d_frames, const emurx_desc* d_desc, uint32_t n,
                          const emurx_dev_out* out, uint32_t n_parts, uint32_t my_rank, uint32_t cap,
                          uint32_t tail_cap, emurx_lookup_rec* d_send, uint32_t* d_send_count, void* stream) {
    int rc = check_batch_args(h, d_frames, d_desc, n, out);
    if (rc) return rc;
    if (!d_send_count || n_parts == 0 || n_parts > EMURX_MAX_PARTS || my_rank >= n_parts ||
        (n && (!d_send || cap == 0)) || ((uintptr_t)d_send & 15) || !lookup_regions_fit(n_parts, cap, tail_cap))
        return EMURX_EINVAL;
    hipStream_t st = stream ? (hipStream_t)stream : h->stream;
    // before anything is enqueued: nothing of a refused call may end up in the caller's graph
    if ((rc = not_capturing(st))) return rc;
    emurx_t::RouteScratch* rs = nullptr;
    if ((rc = route_scratch(h, n, st, &rs))) return rc;
    // owner counts from the L2 headers + group scan, then k_rx packs at those offsets
    if (emurx_launch_owner_count(d_frames, d_desc, n, n_parts, d_send_count, rs->cnt.p, rs->grp.p, rs->goff.p,
                                 rs->tcur.p, st))
        return EMURX_EDEVICE;
    // tcp / udp heads carry their c5tuplekey while ANY client has a TransportCtx: the maps are
    // complete on every partition's handle, the flow tables only on the owner's
    const uint32_t tup_on = h->m.n_ctx_all ? 1u : 0u;
    const emurx_route_args rt{n_parts, my_rank, cap, rs->cnt.p, rs->grp.p, rs->goff.p, d_send,
                              tail_cap, rs->tcur.p, d_send_count, tup_on};
    if (n && (rc = run_dev(h, d_frames, d_desc, n, out, st, 2, &rt))) return rc;
    return route_done(rs, st);
}

int emurx_zmq_walk_dev(emurx_t* h, const uint8_t* d_buf, const uint32_t* d_ctl, uint32_t nmsg, emurx_desc* d_desc,
                       uint32_t* d_msg_stat, uint32_t flags, void* stream) {
    if (!h || (nmsg && (!d_buf || !d_ctl || !d_desc || !d_msg_stat)) || ((uintptr_t)d_desc & 7) ||
        ((uintptr_t)d_ctl & 7) || (flags & ~EMURX_WALK_NO_KEYS))
        return EMURX_EINVAL;
    int rc = bind(h);
    if (rc) return rc;
    hipStream_t st = stream ? (hipStream_t)stream : h->stream;
    if ((rc = not_capturing(st))) return rc;
    return emurx_launch_zmq_walk(d_buf, d_ctl, nmsg, d_desc, d_msg_stat, st, !(flags & EMURX_WALK_NO_KEYS))
               ? EMURX_EDEVICE
               : EMURX_OK;
}

int emurx_lookup_dev(emurx_t* h, const emurx_lookup_rec* d_recv, const uint32_t* d_recv_count, uint32_t n_parts,
                     uint32_t cap, uint32_t tail_cap, emurx_route_rec* d_out, uint32_t* d_flow, void* stream) {
    if (!h || !d_recv_count || n_parts == 0 || n_parts > EMURX_MAX_PARTS || (cap && (!d_recv || !d_out)) ||
        ((uintptr_t)d_recv & 15) || ((uintptr_t)d_out & 7) || !lookup_regions_fit(n_parts, cap, tail_cap))
        return EMURX_EINVAL;
    int rc = bind(h);
    if (rc) return rc;
    hipStream_t st = stream ? (hipStream_t)stream : h->stream;
    if ((rc = not_capturing(st)) || (rc = prepare_read(h, st))) return rc;
    return emurx_launch_lookup(d_recv, d_recv_count, n_parts, cap, tail_cap, h->tables(), d_out, d_flow, st) ? EMURX_EDEVICE
                                                                                                    : EMURX_OK;
}

int emurx_rx_stream(emurx_t* h, const uint8_t* msg, size_t len, emurx_rec* out_rec,
                    uint32_t* out_qlist, uint32_t out_cap, uint32_t* n_out,
                    uint32_t out_qoff[EMURX_NUM_QUEUES + 1], emurx_counters* delta) {
    if (!h || !n_out || !out_qoff || !delta || (len && !msg)) return EMURX_EINVAL;
    memset(delta, 0, sizeof(*delta));
    *n_out = 0;
    int rc = bind(h);
    if (rc) return rc;
    // one message through the batched ingest (device framing walk), on the private slot
    const uint32_t slot = EMURX_INGEST_SLOTS;
    uint8_t* buf = nullptr;
    if ((rc = ingest_buffer(h, slot, std::max<size_t>(len, 1), &buf))) return rc;
    if (len) memcpy(buf, msg, len);
    memset(buf + len, 0, 64);
    const emurx_msg m{0, (uint32_t)len};
    if ((rc = ingest_submit(h, slot, &m, 1))) return rc;
    emurx_ingest_result r;
    if ((rc = ingest_wait(h, slot, &r))) return rc;
    if (r.n_frames > out_cap) return EMURX_ENOSPC;
    if (r.n_frames && (!out_rec || !out_qlist)) return EMURX_EINVAL;
    if (r.n_frames) {
        memcpy(out_rec, r.rec, (size_t)r.n_frames * sizeof(emurx_rec));
        memcpy(out_qlist, r.qlist, (size_t)r.n_frames * 4);
    }
    memcpy(out_qoff, r.qoff, sizeof(r.qoff));
    *delta = r.delta;
    *n_out = r.n_frames;
    return EMURX_OK;
}

int emurx_ingest_buffer(emurx_t* h, uint32_t slot, size_t bytes, uint8_t** buf) {
    if (!h || !buf || slot >= EMURX_INGEST_SLOTS) return EMURX_EINVAL;
    int rc = bind(h);
    return rc ? rc : ingest_buffer(h, slot, bytes, buf);
}
int emurx_ingest_submit(emurx_t* h, uint32_t slot, const emurx_msg* msgs, uint32_t nmsg) {
    if (!h || slot >= EMURX_INGEST_SLOTS) return EMURX_EINVAL;
    return ingest_submit(h, slot, msgs, nmsg);
}
int emurx_ingest_wait(emurx_t* h, uint32_t slot, emurx_ingest_result* res) {
    if (!h || !res || slot >= EMURX_INGEST_SLOTS) return EMURX_EINVAL;
    return ingest_wait(h, slot, res);
}
int emurx_ingest_stream(emurx_t* h, uint32_t slot, void** stream) {
    if (!h || !stream || slot >= EMURX_INGEST_SLOTS) return EMURX_EINVAL;
    int rc = bind(h);
    if (rc) return rc;
    IngestSlot& s = h->ing[slot];
    if (!s.st && !EMURX_HIP_OK(hipStreamCreateWithFlags(&s.st, hipStreamNonBlocking))) return EMURX_EDEVICE;
    *stream = (void*)s.st;
    return EMURX_OK;
}

void emurx_hist_fold(const uint64_t* shards, uint64_t out[2 * EMURX_HIST_BINS]) {
    for (int b = 0; b < 2 * EMURX_HIST_BINS; ++b) out[b] = 0;
    if (!shards) return;
    for (int s = 0; s < EMURX_HIST_SHARDS; ++s)
        for (int b = 0; b < 2 * EMURX_HIST_BINS; ++b) out[b] += shards[(size_t)s * 2 * EMURX_HIST_BINS + b];
}

int emurx_set_timing(emurx_t* h, uint32_t slots, uint32_t stride) {
    if (!h) return EMURX_EINVAL;
    int rc = bind(h);
    if (rc) return rc;
    (void)hipDeviceSynchronize();
    for (auto& e : h->ev)
        if (e) (void)hipEventDestroy(e);
    h->ev.assign((size_t)slots * 2, nullptr);
    // timing only: no system-scope fence at the record (on gfx950 that fence is a cache
    // write-back and invalidate, which both inflated the bracketed launch and slowed the next)
    for (auto& e : h->ev)
        if (!EMURX_HIP_OK(hipEventCreateWithFlags(&e, hipEventDisableSystemFence))) { h->slots = 0; return EMURX_EDEVICE; }
    h->slots = slots;
    h->stride = stride ? stride : 1;
    h->ev_head = h->ev_count = h->batch_seq = 0;
    return EMURX_OK;
}

uint32_t emurx_last_stage(const emurx_t* h) { return h ? h->last_stage : 0; }
int emurx_last_uniform(emurx_t* h, uint32_t words[EMURX_UNI_WORDS]) {
    static_assert(EMURX_UNI_WORDS == emurx::kFbWords, "one path word per sampled wave");
    if (!h || !words) return EMURX_EINVAL;
    if (bind(h)) return EMURX_EDEVICE;  // a host-only handle launches nothing
    if (!EMURX_HIP_OK(hipDeviceSynchronize()) ||
        !EMURX_HIP_OK(hipMemcpy(words, h->d_stage_fb.p + emurx::kFbWords, EMURX_UNI_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost)))
        return EMURX_EDEVICE;
    // the words of the most recent launch alone (k_rx tags them with its generation)
    for (uint32_t i = 0; i < EMURX_UNI_WORDS; ++i)
        words[i] = h->stage_gen && (words[i] >> 2) == h->stage_gen ? EMURX_UNI_SAMPLED | (words[i] & 3u) : 0u;
    return EMURX_OK;
}
int emurx_last_trim(emurx_t* h, uint32_t words[EMURX_UNI_WORDS]) {
    if (!h || !words) return EMURX_EINVAL;
    if (bind(h)) return EMURX_EDEVICE;
    if (!EMURX_HIP_OK(hipDeviceSynchronize()) ||
        !EMURX_HIP_OK(hipMemcpy(words, h->d_stage_fb.p + 2 * emurx::kFbWords, EMURX_UNI_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost)))
        return EMURX_EDEVICE;
    for (uint32_t i = 0; i < EMURX_UNI_WORDS; ++i)  // as emurx_last_uniform: the most recent launch's words alone
        words[i] = h->stage_gen && (words[i] >> 2) == h->stage_gen ? EMURX_UNI_SAMPLED | (words[i] & EMURX_TRIM_RANGE) : 0u;
    return EMURX_OK;
}
int32_t emurx_last_txz(const emurx_t* h) {
    if (!h || h->last_txz < 0) return -1;
    return h->last_txz == EMURX_TXZ_NARROW ? 4608 : h->last_txz == EMURX_TXZ_LONG ? 0 : 6144;
}

int emurx_kernel_times(emurx_t* h, float* batch_ms, uint32_t cap, uint32_t* n_out) {
    if (!h || !n_out || (cap && !batch_ms)) return EMURX_EINVAL;
    *n_out = 0;
    if (!h->slots || !h->ev_count) return EMURX_OK;
    int rc = bind(h);
    if (rc) return rc;
    const uint32_t last = (h->ev_head + h->slots - 1) % h->slots;
    if (!EMURX_HIP_OK(hipEventSynchronize(h->ev[2 * last + 1]))) return EMURX_EDEVICE;
    const uint32_t n = std::min(h->ev_count, cap);
    const uint32_t first = (h->ev_head + h->slots - h->ev_count) % h->slots;
    for (uint32_t k = 0; k < n; ++k) {
        const uint32_t s = (first + (h->ev_count - n) + k) % h->slots;
        if (!EMURX_HIP_OK(hipEventElapsedTime(&batch_ms[k], h->ev[2 * s], h->ev[2 * s + 1])))
            return EMURX_EDEVICE;
    }
    *n_out = n;
    h->ev_count = 0;
    return EMURX_OK;
}

int emurx_tx_checksum_dev(emurx_t* h, uint8_t* d_frames, const emurx_tx_desc* d_desc, uint32_t n,
                          uint8_t* d_status, void* stream) {
    if (!h || (n && (!d_frames || !d_desc))) return EMURX_EINVAL;
    if ((uintptr_t)d_desc & 15) return EMURX_EINVAL;  // one 16-byte load per descriptor
    int rc = bind(h);
    if (rc) return rc;
    hipStream_t st = stream ? (hipStream_t)stream : h->stream;
    return emurx_launch_tx_csum(d_frames, d_desc, n, d_status, st) ? EMURX_EDEVICE : EMURX_OK;
}

// the framing scratch for n frames: grows on demand behind a synchronisation of `st` (a launch
// in flight may still read the old one)
static int txz_reserve(emurx_t* h, uint32_t n, hipStream_t st) {
    const size_t need = emurx_txz_scratch_bytes(n);
    if (need > h->d_txz.n) {
        (void)hipStreamSynchronize(st);
        if (h->d_txz.alloc(need)) return EMURX_ENOMEM;
        // the chain's arrival counters (and the feedback words) start at zero (each call's last
        // arrival resets its own counter)
        if (!EMURX_HIP_OK(hipMemset(h->d_txz.p, 0, need))) return EMURX_EDEVICE;
        h->txz_pending = false;
    }
    return EMURX_OK;
}

int emurx_tx_zmq_counted_dev(emurx_t* h, const uint8_t* d_frames, const emurx_desc* d_desc, uint32_t n_max,
                             const uint64_t* d_count, uint8_t* d_out, uint64_t out_cap, uint64_t* d_msg_off,
                             uint64_t* d_info, void* stream) {
    if (!h || !d_msg_off || !d_info || !d_count || (n_max && (!d_frames || !d_desc || (!d_out && out_cap))))
        return EMURX_EINVAL;
    if (n_max >= EMURX_TX_ZMQ_MAX_FRAMES || ((uintptr_t)d_out & 15) || ((uintptr_t)d_desc & 7) || ((uintptr_t)d_count & 7))
        return EMURX_EINVAL;
    int rc = bind(h);
    if (rc) return rc;
    hipStream_t st = stream ? (hipStream_t)stream : h->stream;
    if ((rc = txz_reserve(h, n_max, st))) return rc;
    // the write's image as the plain calls last chose it; a counted call samples no feedback
    const int variant = h->txz_mode >= 0 ? h->txz_mode : h->txz_variant;
    if (emurx_launch_tx_zmq(d_frames, d_desc, n_max, d_out, out_cap, d_msg_off, d_info, h->d_txz.p, st, variant, false,
                            d_count))
        return EMURX_EDEVICE;
    h->last_txz = variant;
    return EMURX_OK;
}

int emurx_tx_zmq_dev(emurx_t* h, const uint8_t* d_frames, const emurx_desc* d_desc, uint32_t n,
                     uint8_t* d_out, uint64_t out_cap, uint64_t* d_msg_off, uint64_t* d_info, void* stream) {
    if (!h || !d_msg_off || !d_info || (n && (!d_frames || !d_desc || (!d_out && out_cap))))
        return EMURX_EINVAL;
    if (n >= EMURX_TX_ZMQ_MAX_FRAMES || ((uintptr_t)d_out & 15) || ((uintptr_t)d_desc & 7)) return EMURX_EINVAL;
    int rc = bind(h);
    if (rc) return rc;
    hipStream_t st = stream ? (hipStream_t)stream : h->stream;
    if ((rc = txz_reserve(h, n, st))) return rc;
    if (!h->txz_ev && (h->txz_fb.alloc(2) || !EMURX_HIP_OK(hipEventCreateWithFlags(&h->txz_ev, hipEventDisableTiming))))
        return EMURX_ENOMEM;
    if (h->txz_pending && hipEventQuery(h->txz_ev) == hipSuccess) {  // "not ready" is no error
        h->txz_pending = false;
        // hi: the largest upper bound of a sampled tile's output rows; lo: the smallest lower
        // bound (0 words: nothing sampled, the choice stands)
        const uint32_t hi = h->txz_fb.p[0], lo = ~h->txz_fb.p[1];
        const int v = !hi                                ? h->txz_variant
                      : hi <= emurx_txz_img_narrow_rows ? EMURX_TXZ_NARROW
                      : lo > emurx_txz_img_wide_rows    ? EMURX_TXZ_LONG
                                                        : EMURX_TXZ_WIDE;
        if (v != h->txz_variant) {
            h->txz_same = 0;
            h->txz_every = 8;
        } else if (++h->txz_same >= 2 && h->txz_every < 256) {
            h->txz_every *= 2;
        }
        h->txz_variant = v;
    }
    const bool fb = h->txz_mode < 0 && n && !h->txz_pending && (!h->txz_calls || h->txz_calls - h->txz_last_copy >= h->txz_every);
    ++h->txz_calls;
    const int variant = h->txz_mode >= 0 ? h->txz_mode : h->txz_variant;
    if (emurx_launch_tx_zmq(d_frames, d_desc, n, d_out, out_cap, d_msg_off, d_info, h->d_txz.p, st, variant, fb))
        return EMURX_EDEVICE;
    h->last_txz = variant;
    if (fb) {  // the two words behind this call, then cleared for the next sample
        if (!EMURX_HIP_OK(hipMemcpyAsync(h->txz_fb.p, h->d_txz.p, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, st)) ||
            !EMURX_HIP_OK(hipMemsetAsync(h->d_txz.p, 0, 2 * sizeof(uint32_t), st)) ||
            !EMURX_HIP_OK(hipEventRecord(h->txz_ev, st)))
            return EMURX_EDEVICE;
        h->txz_pending = true;
        h->txz_last_copy = h->txz_calls;
    }
    return EMURX_OK;
}

// emurx_respond_dev, emurx_respond_kinds_dev and emurx_respond_ts_dev: one implementation, the
// answers chosen by `kinds` out of the entry point's `allowed`, the words of d_info that are
// written by `info_words`; ip_time_ms is read for EMURX_RSPK_TS alone
static int respond_kinds(emurx_t* h, const uint8_t* d_frames, const emurx_desc* d_desc, const emurx_rec* d_rec,
                         uint32_t n, uint32_t kinds, uint32_t allowed, uint32_t ip_time_ms, uint32_t info_words,
                         uint8_t* d_out, uint64_t out_cap, emurx_desc* d_out_desc, uint32_t* d_out_src,
                         uint8_t* d_outcome, uint64_t* d_info, void* stream) {
    if (!h || !d_info || (n && (!d_frames || !d_desc || !d_rec || !d_out_desc || !d_out_src || (!d_out && out_cap))))
        return EMURX_EINVAL;
    if (kinds == 0 || (kinds & ~allowed)) return EMURX_EINVAL;
    if (n >= EMURX_TX_ZMQ_MAX_FRAMES || ((uintptr_t)d_out & 15) || ((uintptr_t)d_rec & 15) || ((uintptr_t)d_desc & 7) ||
        ((uintptr_t)d_out_desc & 7) || ((uintptr_t)d_info & 7))
        return EMURX_EINVAL;
    int rc = bind(h);
    if (rc) return rc;
    hipStream_t st = stream ? (hipStream_t)stream : h->stream;
    // the ARP reply reads the IPv4 table, the neighbour advertisement the MAC, IPv6 and client-info
    // tables: behind the shipment of pending edits, like a classify
    if ((rc = not_capturing(st)) || (rc = prepare_read(h, st))) return rc;
    const size_t need = emurx_rsp_scratch_bytes(n);
    if (need > h->d_rsp.n) {  // grows on demand; a launch in flight may still read the old one
        (void)hipStreamSynchronize(st);
        if (h->d_rsp.alloc(need)) return EMURX_ENOMEM;
    }
    return emurx_launch_respond(d_frames, d_desc, d_rec, n, kinds, h->tables(), d_out, out_cap, d_out_desc, d_out_src,
                                d_outcome, d_info, info_words, ip_time_ms, h->d_rsp.p, st)
               ? EMURX_EDEVICE
               : EMURX_OK;
}

int emurx_respond_dev(emurx_t* h, const uint8_t* d_frames, const emurx_desc* d_desc, const emurx_rec* d_rec,
                      uint32_t n, uint8_t* d_out, uint64_t out_cap, emurx_desc* d_out_desc, uint32_t* d_out_src,
                      uint8_t* d_outcome, uint64_t* d_info, void* stream) {
    return respond_kinds(h, d_frames, d_desc, d_rec, n, EMURX_RSPK_ARP | EMURX_RSPK_ICMP | EMURX_RSPK_ICMPV6,
                         EMURX_RSPK_ALL, 0, 8, d_out, out_cap, d_out_desc, d_out_src, d_outcome, d_info, stream);
}

int emurx_respond_kinds_dev(emurx_t* h, const uint8_t* d_frames, const emurx_desc* d_desc, const emurx_rec* d_rec,
                            uint32_t n, uint32_t kinds, uint8_t* d_out, uint64_t out_cap, emurx_desc* d_out_desc,
                            uint32_t* d_out_src, uint8_t* d_outcome, uint64_t* d_info, void* stream) {
    return respond_kinds(h, d_frames, d_desc, d_rec, n, kinds, EMURX_RSPK_ALL, 0, EMURX_RSP_INFO_WORDS, d_out, out_cap,
                         d_out_desc, d_out_src, d_outcome, d_info, stream);
}

int emurx_respond_ts_dev(emurx_t* h, const uint8_t* d_frames, const emurx_desc* d_desc, const emurx_rec* d_rec,
                         uint32_t n, uint32_t kinds, uint32_t ip_time_ms, uint8_t* d_out, uint64_t out_cap,
                         emurx_desc* d_out_desc, uint32_t* d_out_src, uint8_t* d_outcome, uint64_t* d_info, void* stream) {
    return respond_kinds(h, d_frames, d_desc, d_rec, n, kinds, EMURX_RSPK_ALL_TS, ip_time_ms, EMURX_RSP_INFO_WORDS, d_out,
                         out_cap, d_out_desc, d_out_src, d_outcome, d_info, stream);
}

uint32_t emurx_learn_max_events(const emurx_t* h) { return h ? emurx_lrn_slots(h->cfg.max_frames) / 2 : 0; }

uint32_t emurx_learn_key_hash(const uint32_t key[7]) {
    return key ? emurx_lrn_hash(key[0], key[1], key[2], key[3], key[4], key[5], key[6]) : 0;
}

int emurx_learn_dev(emurx_t* h, const uint8_t* d_frames, const emurx_desc* d_desc, const emurx_rec* d_rec, uint32_t n,
                    uint32_t kinds, emurx_learn_ev* d_ev, uint32_t ev_cap, uint8_t* d_outcome, uint64_t* d_info,
                    void* stream) {
    if (!h || !d_info || !d_ev || (n && (!d_frames || !d_desc || !d_rec))) return EMURX_EINVAL;
    if (kinds == 0 || (kinds & ~EMURX_LRNK_ALL)) return EMURX_EINVAL;
    if (ev_cap == 0 || ev_cap > emurx_learn_max_events(h)) return EMURX_EINVAL;
    if (n >= EMURX_TX_ZMQ_MAX_FRAMES || ((uintptr_t)d_rec & 15) || ((uintptr_t)d_desc & 7) || ((uintptr_t)d_ev & 7) ||
        ((uintptr_t)d_info & 7))
        return EMURX_EINVAL;
    int rc = bind(h);
    if (rc) return rc;
    if (n > h->cfg.max_frames) return EMURX_ENOMEM;  // the scratch is sized at emurx_open
    hipStream_t st = stream ? (hipStream_t)stream : h->stream;
    // a solicitation's source and an advertisement's target are looked up in the MAC, IPv6 and
    // client-info tables: behind the shipment of pending edits, like a classify
    if ((rc = not_capturing(st)) || (rc = prepare_read(h, st))) return rc;
    if (h->lrn_dirty) {
        if (!EMURX_HIP_OK(hipMemsetAsync(h->d_lrn.p, 0, (size_t)emurx_lrn_slots(h->cfg.max_frames) * 16, st)))
            return EMURX_EDEVICE;
        h->lrn_dirty = false;
    }
    if (emurx_launch_learn(d_frames, d_desc, d_rec, n, kinds, h->tables(), d_ev, ev_cap, d_outcome, d_info, h->d_lrn.p,
                           h->cfg.max_frames, st)) {
        h->lrn_dirty = true;
        return EMURX_EDEVICE;
    }
    return EMURX_OK;
}

uint32_t emurx_nsstat_max_events(const emurx_t* h) { return h ? std::min(h->cfg.max_frames, h->cfg.max_ns) : 0; }

// emurx_nsstat_dev and emurx_nsstat_ts_dev: one implementation, `kinds` out of the entry point's `allowed`
static int nsstat_kinds(emurx_t* h, const uint8_t* d_frames, const emurx_desc* d_desc, const emurx_rec* d_rec, uint32_t n,
                        uint32_t kinds, uint32_t allowed, const uint8_t* d_rsp_outcome, const uint8_t* d_lrn_outcome,
                        emurx_nsstat_ev* d_ev, uint32_t ev_cap, uint8_t* d_done, uint64_t* d_info, void* stream) {
    if (!h || !d_info || !d_ev || (n && (!d_frames || !d_desc || !d_rec || !d_rsp_outcome))) return EMURX_EINVAL;
    if (kinds == 0 || (kinds & ~allowed)) return EMURX_EINVAL;
    // the timestamp rule refines the icmp handler's
    if ((kinds & EMURX_RSPK_TS) && !(kinds & EMURX_RSPK_ICMP)) return EMURX_EINVAL;
    // the learn outcome decides for ARP and ND frames
    if (n && (kinds & (EMURX_RSPK_ARP | EMURX_RSPK_ND)) && !d_lrn_outcome) return EMURX_EINVAL;
    if (ev_cap == 0 || ev_cap > emurx_nsstat_max_events(h)) return EMURX_EINVAL;
    if (((uintptr_t)d_rec & 15) || ((uintptr_t)d_desc & 7) || ((uintptr_t)d_ev & 7) || ((uintptr_t)d_info & 7))
        return EMURX_EINVAL;
    int rc = bind(h);
    if (rc) return rc;
    if (n > h->cfg.max_frames) return EMURX_ENOMEM;  // the scratch is sized at emurx_open
    hipStream_t st = stream ? (hipStream_t)stream : h->stream;
    // no table is read, but the records are a classify's: behind the shipment like the calls they come from
    if ((rc = not_capturing(st)) || (rc = prepare_read(h, st))) return rc;
    if (h->nss_dirty) {
        if (!EMURX_HIP_OK(hipMemsetAsync(h->d_nss.p, 0, emurx_nss_scratch_bytes(h->cfg.max_frames, h->cfg.max_ns), st))) return EMURX_EDEVICE;
        h->nss_dirty = false;
    }
    if (emurx_launch_nsstat(d_frames, d_desc, d_rec, n, kinds, d_rsp_outcome, d_lrn_outcome, d_ev, ev_cap, d_done, d_info,
                            h->d_nss.p, h->cfg.max_frames, h->cfg.max_ns, st)) {
        h->nss_dirty = true;
        return EMURX_EDEVICE;
    }
    return EMURX_OK;
}

int emurx_nsstat_dev(emurx_t* h, const uint8_t* d_frames, const emurx_desc* d_desc, const emurx_rec* d_rec, uint32_t n,
                     uint32_t kinds, const uint8_t* d_rsp_outcome, const uint8_t* d_lrn_outcome, emurx_nsstat_ev* d_ev,
                     uint32_t ev_cap, uint8_t* d_done, uint64_t* d_info, void* stream) {
    return nsstat_kinds(h, d_frames, d_desc, d_rec, n, kinds, EMURX_RSPK_ALL, d_rsp_outcome, d_lrn_outcome, d_ev, ev_cap,
                        d_done, d_info, stream);
}

int emurx_nsstat_ts_dev(emurx_t* h, const uint8_t* d_frames, const emurx_desc* d_desc, const emurx_rec* d_rec, uint32_t n,
                        uint32_t kinds, const uint8_t* d_rsp_outcome, const uint8_t* d_lrn_outcome, emurx_nsstat_ev* d_ev,
                        uint32_t ev_cap, uint8_t* d_done, uint64_t* d_info, void* stream) {
    return nsstat_kinds(h, d_frames, d_desc, d_rec, n, kinds, EMURX_RSPK_ALL_TS, d_rsp_outcome, d_lrn_outcome, d_ev, ev_cap,
                        d_done, d_info, stream);
}

uint32_t emurx_ping_max_events(const emurx_t* h) { return emurx_learn_max_events(h); }

int emurx_ping_dev(emurx_t* h, const uint8_t* d_frames, const emurx_desc* d_desc, const emurx_rec* d_rec, uint32_t n,
                   uint32_t fams, uint64_t now_unix_ns, emurx_ping_ev* d_ev, uint32_t ev_cap, uint8_t* d_outcome,
                   uint64_t* d_info, void* stream) {
    if (!h || !d_info || !d_ev || (n && (!d_frames || !d_desc || !d_rec))) return EMURX_EINVAL;
    if (fams == 0 || (fams & ~EMURX_PNGK_ALL) || (now_unix_ns >> 63)) return EMURX_EINVAL;
    if (ev_cap == 0 || ev_cap > emurx_ping_max_events(h)) return EMURX_EINVAL;
    if (n >= EMURX_TX_ZMQ_MAX_FRAMES || ((uintptr_t)d_rec & 15) || ((uintptr_t)d_desc & 7) || ((uintptr_t)d_ev & 7) ||
        ((uintptr_t)d_info & 7))
        return EMURX_EINVAL;
    int rc = bind(h);
    if (rc) return rc;
    if (n > h->cfg.max_frames) return EMURX_ENOMEM;  // the scratch is sized at emurx_open
    hipStream_t st = stream ? (hipStream_t)stream : h->stream;
    // an ICMPv6 frame's client is looked up in the MAC table: behind the shipment of pending edits, like a classify
    if ((rc = not_capturing(st)) || (rc = prepare_read(h, st))) return rc;
    if (h->png_dirty) {
        if (emurx_png_scratch_clear(h->d_png.p, h->cfg.max_frames, st)) return EMURX_EDEVICE;
        h->png_dirty = false;
    }
    if (emurx_launch_ping(d_frames, d_desc, d_rec, n, fams, now_unix_ns, h->tables(), d_ev, ev_cap, d_outcome, d_info,
                          h->d_png.p, h->cfg.max_frames, st)) {
        h->png_dirty = true;
        return EMURX_EDEVICE;
    }
    return EMURX_OK;
}

uint32_t emurx_ftstat_max_events(const emurx_t* h) { return h ? std::min(h->cfg.max_frames, h->cfg.max_clients) : 0; }

int emurx_ftstat_dev(emurx_t* h, const uint8_t* d_frames, const emurx_desc* d_desc, const emurx_rec* d_rec,
                     const uint32_t* d_flow, uint32_t n, emurx_ft_ev* d_ev, uint32_t ev_cap, uint8_t* d_outcome,
                     uint64_t* d_info, void* stream) {
    if (!h || !d_info || !d_ev || (n && (!d_frames || !d_desc || !d_rec || !d_flow))) return EMURX_EINVAL;
    if (ev_cap == 0 || ev_cap > emurx_ftstat_max_events(h)) return EMURX_EINVAL;
    if (n >= EMURX_TX_ZMQ_MAX_FRAMES || ((uintptr_t)d_rec & 15) || ((uintptr_t)d_desc & 7) || ((uintptr_t)d_ev & 7) ||
        ((uintptr_t)d_info & 7) || ((uintptr_t)d_flow & 3))
        return EMURX_EINVAL;
    int rc = bind(h);
    if (rc) return rc;
    if (n > h->cfg.max_frames) return EMURX_ENOMEM;  // the scratch is sized at emurx_open
    hipStream_t st = stream ? (hipStream_t)stream : h->stream;
    // no table is read, but the records and flow words are a classify's: behind the shipment like the call they come from
    if ((rc = not_capturing(st)) || (rc = prepare_read(h, st))) return rc;
    if (h->fts_dirty) {
        if (emurx_ft_scratch_clear(h->d_fts.p, h->cfg.max_frames, st)) return EMURX_EDEVICE;
        h->fts_dirty = false;
    }
    if (emurx_launch_ftstat(d_frames, d_desc, d_rec, d_flow, n, h->cfg.max_ns, h->cfg.max_clients, d_ev, ev_cap, d_outcome,
                            d_info, h->d_fts.p, h->cfg.max_frames, st)) {
        h->fts_dirty = true;
        return EMURX_EDEVICE;
    }
    return EMURX_OK;
}

uint32_t emurx_ns_owner(const uint8_t key[12], uint32_t n_parts) {
    if (!key || n_parts == 0) return 0;
    return emurx_owner(emurx_tk_hash(le32(key), le32(key + 4), le32(key + 8)), n_parts);
}
uint8_t emurx_owner_key(const uint8_t key[12]) {
    if (!key) return 0;
    return (uint8_t)emurx_owner_key(emurx_tk_hash(le32(key), le32(key + 4), le32(key + 8)));
}
int emurx_desc_keys_dev(emurx_t* h, const uint8_t* d_frames, emurx_desc* d_desc, uint32_t n, void* stream) {
    if (!h || (n && (!d_frames || !d_desc)) || ((uintptr_t)d_desc & 7)) return EMURX_EINVAL;
    int rc = bind(h);
    if (rc) return rc;
    return emurx_launch_desc_keys(d_frames, d_desc, n, stream ? (hipStream_t)stream : h->stream) ? EMURX_EDEVICE
                                                                                                 : EMURX_OK;
}

int emurx_route_dev(emurx_t* h, const emurx_rec* d_rec, uint32_t n, uint32_t n_parts, uint32_t my_rank,
                    uint32_t cap, emurx_route_rec* d_send, uint32_t* d_send_count, void* stream) {
    if (!h || !d_send_count || n_parts == 0 || n_parts > EMURX_MAX_PARTS || my_rank >= n_parts ||
        (n && (!d_rec || !d_send || cap == 0)))
        return EMURX_EINVAL;
    if (((uintptr_t)d_rec & 15) || ((uintptr_t)d_send & 7)) return EMURX_EINVAL;
    int rc = bind(h);
    if (rc) return rc;
    hipStream_t st = stream ? (hipStream_t)stream : h->stream;
    // before anything is enqueued: nothing of a refused call may end up in the caller's graph
    if ((rc = not_capturing(st))) return rc;
    emurx_t::RouteScratch* rs = nullptr;
    if ((rc = route_scratch(h, n, st, &rs))) return rc;
    if (emurx_launch_route(d_rec, n, n_parts, my_rank, cap, d_send, d_send_count, rs->cnt.p, rs->grp.p, rs->goff.p,
                           st, false))
        return EMURX_EDEVICE;
    return route_done(rs, st);
}

}  // extern "C"

// ---- answers on an ingest slot (emurx_ingest_set_answers / emurx_ingest_answers) -------------
namespace {

// What a batch of at most max_bytes message bytes can produce.  A frame the responder answers, or
// the learner folds, has header offsets that fit it (l3 >= 14 and, for ARP, l3 + 28 <= len; the
// other kinds need more), so it is at least 42 bytes long: at most max_bytes / 42 replies and
// learn events.  A reply is the frame's own length (ICMP, the timestamp reply), shorter (ICMPv6), at most 50 bytes (ARP)
// or at most 94 (ND), so align16(reply) <= max(align16(len), 96) <= len + 54 for len >= 42: the
// replies take at most max_bytes * 96 / 42 bytes, and their framing 8 bytes per reply more.
struct AnsCaps {
    uint64_t rsp, tx;
    uint32_t r, ev, ns;
};
AnsCaps answer_caps(const emurx_t* h) {
    AnsCaps c;
    const uint64_t mb = h->cfg.max_bytes;
    c.r = (uint32_t)std::min<uint64_t>(h->cfg.max_frames, mb / 42 + 1);
    c.ev = c.r;
    c.ns = std::min(emurx_nsstat_max_events(h), h->cfg.max_frames);
    c.rsp = ((mb * 96 / 42 + 96) + 15) & ~(uint64_t)15;
    c.tx = (c.rsp + 8ull * c.r + 15) & ~(uint64_t)15;
    return c;
}

// The four info blocks of a slot's answer stages, laid out in d_ainfo as the answer block's head
struct AnsInfo {
    uint64_t *rsp, *lrn, *nss, *tx;
};
AnsInfo answer_info(IngestSlot& s) {
    uint64_t* p = s.d_ainfo.p;
    return {p, p + EMURX_ANS_HEAD_LRN, p + EMURX_ANS_HEAD_NSS, p + EMURX_ANS_HEAD_TX};
}

// The answer stages of a batch of n descriptor slots (answers on): respond, the counted framing of
// the replies, learn, nsstat and, where the slot has it on, the ping fold.
int answer_stages(emurx_t* h, IngestSlot& s, uint32_t n) {
    hipStream_t st = s.st;
    const uint32_t kinds = s.ans_kinds;
    const AnsInfo inf = answer_info(s);
    // the slot's time of day rides the launch as an argument: batches in flight keep their own
    int rc = respond_kinds(h, s.d_buf.p, s.d_desc.p, s.d_rec.p, n, kinds, EMURX_RSPK_ALL_TS, s.ans_time,
                           EMURX_RSP_INFO_WORDS, s.d_rsp_out.p, s.ans_rsp_cap, s.d_rsp_desc.p, s.d_rsp_src.p, s.d_rspo.p,
                           inf.rsp, st);
    if (rc) return rc;
    if ((rc = emurx_tx_zmq_counted_dev(h, s.d_rsp_out.p, s.d_rsp_desc.p, n, inf.rsp, s.d_tx.p, s.ans_tx_cap,
                                       s.d_tx_off.p, inf.tx, st)))
        return rc;
    const uint32_t lk = ((kinds & EMURX_RSPK_ARP) ? EMURX_LRNK_ARP : 0u) | ((kinds & EMURX_RSPK_ND) ? EMURX_LRNK_ND : 0u);
    if (lk) {
        rc = emurx_learn_dev(h, s.d_buf.p, s.d_desc.p, s.d_rec.p, n, lk, s.d_lev.p, emurx_learn_max_events(h),
                             s.d_lrno.p, inf.lrn, st);
    } else {  // nothing to learn from: every outcome EMURX_LRN_NONE, no event
        rc = EMURX_HIP_OK(hipMemsetAsync(inf.lrn, 0, EMURX_LRN_INFO_WORDS * sizeof(uint64_t), st)) &&
                     (!n || EMURX_HIP_OK(hipMemsetAsync(s.d_lrno.p, 0, n, st)))
                 ? EMURX_OK
                 : EMURX_EDEVICE;
    }
    if (rc) return rc;
    if ((rc = emurx_nsstat_ts_dev(h, s.d_buf.p, s.d_desc.p, s.d_rec.p, n, kinds, s.d_rspo.p, s.d_lrno.p, s.d_nsev.p,
                                  emurx_nsstat_max_events(h), s.d_donef.p, inf.nss, st)))
        return rc;
    // the ping stage, with the slot's own time of day as a launch argument
    if (s.png_fams)
        rc = emurx_ping_dev(h, s.d_buf.p, s.d_desc.p, s.d_rec.p, n, s.png_fams, s.png_now, s.d_pev.p, emurx_ping_max_events(h),
                            s.d_pngo.p, s.d_pinfo.p, st);
    return rc;
}

// What the answer stages produced, into the slot's pinned blocks: k_png_out, then k_ans_out.
int answer_out(IngestSlot& s, uint32_t n) {
    hipStream_t st = s.st;
    const AnsInfo inf = answer_info(s);
    if (s.png_fams && emurx_launch_ping_out(s.d_pinfo.p, s.d_pev.p, s.d_pngo.p, n, s.png_ev_cap, reinterpret_cast<uint8_t*>(s.h_pinfo.p),
                                            reinterpret_cast<uint8_t*>(s.h_pev.p), s.h_pngo.p, st))
        return EMURX_EDEVICE;
    const emurx_ans_out a{reinterpret_cast<const unsigned long long*>(inf.rsp),
                          reinterpret_cast<const unsigned long long*>(inf.tx),
                          reinterpret_cast<const unsigned long long*>(inf.lrn),
                          reinterpret_cast<const unsigned long long*>(inf.nss),
                          s.d_tx.p,
                          reinterpret_cast<const unsigned long long*>(s.d_tx_off.p),
                          s.d_rsp_src.p,
                          s.d_lev.p,
                          s.d_nsev.p,
                          reinterpret_cast<uint8_t*>(s.h_ahead.p),
                          s.h_tx.p,
                          reinterpret_cast<uint8_t*>(s.h_tx_off.p),
                          reinterpret_cast<uint8_t*>(s.h_src.p),
                          reinterpret_cast<uint8_t*>(s.h_lev.p),
                          reinterpret_cast<uint8_t*>(s.h_nsev.p),
                          s.ans_tx_cap,
                          s.ans_r_cap,
                          s.ans_ev_cap,
                          s.ans_ns_cap};
    return emurx_launch_ans_out(a, n, st) ? EMURX_EDEVICE : EMURX_OK;
}

// The stage chain of a batch of n descriptor slots, on the slot's stream behind k_rx and the queue
// pack, for a slot with answers on, flows on or both: the answer stages, then the fold of the
// refused transport frames (emurx_ingest_set_flows), serialised across slots because the stages'
// scratch is the handle's (each chain waits for the previous one's event and records its own
// behind its last fold), then the launches that copy out.  No allocation and no host
// synchronisation: emurx_ingest_set_answers / _set_ping / _set_flows sized everything.
int stage_chain(emurx_t* h, IngestSlot& s, uint32_t n) {
    hipStream_t st = s.st;
    const bool answers = s.ans_kinds != 0, flows = s.flw_on;
    if (n >= EMURX_TX_ZMQ_MAX_FRAMES) return EMURX_ENOSPC;
    if (h->ans_recorded && !EMURX_HIP_OK(hipStreamWaitEvent(st, h->ans_ev, 0))) return EMURX_EDEVICE;
    int rc;
    if (answers && (rc = answer_stages(h, s, n))) return rc;
    if (flows && (rc = emurx_ftstat_dev(h, s.d_buf.p, s.d_desc.p, s.d_rec.p, s.d_flow.p, n, s.d_fev.p, s.flw_ev_cap, s.d_fto.p,
                                        s.d_finfo.p, st)))
        return rc;
    // the shared scratch is free again: the next slot's stages may start while this one copies out
    if (!EMURX_HIP_OK(hipEventRecord(h->ans_ev, st))) return EMURX_EDEVICE;
    h->ans_recorded = true;
    if (answers && (rc = answer_out(s, n))) return rc;
    if (flows && emurx_launch_ft_out(s.d_finfo.p, s.d_fev.p, s.d_flow.p, s.d_fto.p, n, s.flw_ev_cap,
                                     reinterpret_cast<uint8_t*>(s.h_finfo.p), reinterpret_cast<uint8_t*>(s.h_fev.p),
                                     reinterpret_cast<uint8_t*>(s.h_flow.p), s.h_fto.p, st))
        return EMURX_EDEVICE;
    return EMURX_OK;
}

// emurx_ingest_set_answers and emurx_ingest_set_answers_ts: `kinds` out of the entry point's `allowed`
int set_answers(emurx_t* h, uint32_t slot, uint32_t kinds, uint32_t allowed) {
    if (!h || slot >= EMURX_INGEST_SLOTS || (kinds & ~allowed)) return EMURX_EINVAL;
    if ((kinds & EMURX_RSPK_TS) && !(kinds & EMURX_RSPK_ICMP)) return EMURX_EINVAL;
    int rc = bind(h);
    if (rc) return rc;
    IngestSlot& s = h->ing[slot];
    if (s.pending) return EMURX_EINVAL;
    if (!kinds) s.png_fams = 0;  // no chain, no ping stage
    if (!kinds || s.h_ans.p) {  // off, or sized by an earlier call
        s.ans_kinds = kinds;
        return EMURX_OK;
    }
    // everything the chain needs, now: no submit allocates or synchronises for it.  The shared
    // scratches may be in use by launches in flight, so the device is idle before they grow.
    if (!EMURX_HIP_OK(hipDeviceSynchronize())) return EMURX_EDEVICE;
    const uint32_t mf = std::min<uint32_t>(h->cfg.max_frames, EMURX_TX_ZMQ_MAX_FRAMES - 1);
    if (!h->ans_ev && !EMURX_HIP_OK(hipEventCreateWithFlags(&h->ans_ev, hipEventDisableTiming))) return EMURX_EDEVICE;
    if ((rc = txz_reserve(h, mf, h->stream))) return rc;
    if (emurx_rsp_scratch_bytes(mf) > h->d_rsp.n && h->d_rsp.alloc(emurx_rsp_scratch_bytes(mf))) return EMURX_ENOMEM;
    const AnsCaps c = answer_caps(h);
    // device arrays: a descriptor, a source index and a message offset per descriptor slot (the
    // stages' own capacities), the events at the stages' ev_cap; two elements of slack each, so
    // that k_ans_out's last 16-byte vector of any count is readable
    if (s.d_rsp_out.alloc(c.rsp + 16) || s.d_tx.alloc(c.tx + 16) || s.d_rsp_desc.alloc((size_t)mf + 2) ||
        s.d_rsp_src.alloc((size_t)mf + 4) || s.d_tx_off.alloc((size_t)mf + 3) || s.d_ainfo.alloc(EMURX_ANS_HEAD_WORDS) ||
        s.d_lev.alloc((size_t)emurx_learn_max_events(h) + 2) || s.d_nsev.alloc((size_t)emurx_nsstat_max_events(h) + 2))
        return EMURX_ENOMEM;
    if (!EMURX_HIP_OK(hipMemset(s.d_ainfo.p, 0, EMURX_ANS_HEAD_WORDS * sizeof(uint64_t)))) return EMURX_EDEVICE;
    auto carve = [&](uint8_t* block) {
        emurx_carver k(block);
        s.h_ahead.p = k.take<uint64_t>(EMURX_ANS_HEAD_WORDS);
        s.h_tx_off.p = k.take<uint64_t>((size_t)c.r + 1);
        s.h_src.p = k.take<uint32_t>(c.r);
        s.h_lev.p = k.take<emurx_learn_ev>(c.ev);
        s.h_nsev.p = k.take<emurx_nsstat_ev>(c.ns);
        s.h_tx.p = k.take<uint8_t>(c.tx);
        return k.bytes();
    };
    if (s.h_ans.alloc(carve(nullptr))) return EMURX_ENOMEM;
    carve(s.h_ans.p);
    memset(s.h_ahead.p, 0, EMURX_ANS_HEAD_WORDS * sizeof(uint64_t));
    s.ans_rsp_cap = c.rsp, s.ans_tx_cap = c.tx, s.ans_r_cap = c.r, s.ans_ev_cap = c.ev, s.ans_ns_cap = c.ns;
    s.ans_kinds = kinds;
    return EMURX_OK;
}

}  // namespace

extern "C" {

int emurx_ingest_set_answers(emurx_t* h, uint32_t slot, uint32_t kinds) {
    return set_answers(h, slot, kinds, EMURX_RSPK_ALL);
}

int emurx_ingest_set_answers_ts(emurx_t* h, uint32_t slot, uint32_t kinds) {
    return set_answers(h, slot, kinds, EMURX_RSPK_ALL_TS);
}

int emurx_ingest_set_time(emurx_t* h, uint32_t slot, uint32_t ip_time_ms) {
    if (!h || slot >= EMURX_INGEST_SLOTS) return EMURX_EINVAL;
    IngestSlot& s = h->ing[slot];
    if (s.pending) return EMURX_EINVAL;
    s.ans_time = ip_time_ms;
    return EMURX_OK;
}

int emurx_ingest_set_ping(emurx_t* h, uint32_t slot, uint32_t fams) {
    if (!h || slot >= EMURX_INGEST_SLOTS || (fams & ~EMURX_PNGK_ALL)) return EMURX_EINVAL;
    int rc = bind(h);
    if (rc) return rc;
    IngestSlot& s = h->ing[slot];
    if (s.pending || (fams && !s.ans_kinds)) return EMURX_EINVAL;  // the stage is part of the answer chain
    if (!fams || s.h_png.p) {  // off, or sized by an earlier call
        s.png_fams = fams;
        return EMURX_OK;
    }
    // everything the stage needs, now: no submit allocates or synchronises for it.  A folded frame
    // is at least 42 bytes long (l3 >= 14, 20 bytes of IPv4 header and 8 of ICMP, or more), so a
    // batch has at most max_bytes / 42 events: the answer block's bound.
    const uint32_t mf = std::min<uint32_t>(h->cfg.max_frames, EMURX_TX_ZMQ_MAX_FRAMES - 1);
    const uint32_t cap = answer_caps(h).ev;
    if (s.d_pev.alloc((size_t)emurx_ping_max_events(h) + 1) || s.d_pinfo.alloc(EMURX_PNG_INFO_WORDS) || s.d_pngo.alloc((size_t)mf + 16))
        return EMURX_ENOMEM;
    auto carve = [&](uint8_t* block) {
        emurx_carver k(block);
        s.h_pinfo.p = k.take<uint64_t>(EMURX_PNG_INFO_WORDS);
        s.h_pngo.p = k.take<uint8_t>((size_t)mf + 16);
        s.h_pev.p = k.take<emurx_ping_ev>(cap);
        return k.bytes();
    };
    if (s.h_png.alloc(carve(nullptr))) return EMURX_ENOMEM;
    carve(s.h_png.p);
    memset(s.h_pinfo.p, 0, EMURX_PNG_INFO_WORDS * sizeof(uint64_t));
    s.png_ev_cap = cap;
    s.png_fams = fams;
    return EMURX_OK;
}

int emurx_ingest_set_now(emurx_t* h, uint32_t slot, uint64_t now_unix_ns) {
    if (!h || slot >= EMURX_INGEST_SLOTS || (now_unix_ns >> 63)) return EMURX_EINVAL;
    IngestSlot& s = h->ing[slot];
    if (s.pending) return EMURX_EINVAL;
    s.png_now = now_unix_ns;
    return EMURX_OK;
}

int emurx_ingest_ping(emurx_t* h, uint32_t slot, emurx_ping_out* out) {
    if (!h || !out || slot >= EMURX_INGEST_SLOTS) return EMURX_EINVAL;
    const IngestSlot& s = h->ing[slot];
    if (s.pending || !s.waited) return EMURX_EINVAL;
    if (!s.png_batch) return EMURX_ENOENT;
    memset(out, 0, sizeof(*out));
    out->ev = s.h_pev.p;
    out->n_ev = (uint32_t)s.h_pinfo.p[0];
    out->outcome = s.h_pngo.p;
    memcpy(out->info, s.h_pinfo.p, sizeof(out->info));
    return EMURX_OK;
}

int emurx_ingest_set_flows(emurx_t* h, uint32_t slot, uint32_t on) {
    if (!h || slot >= EMURX_INGEST_SLOTS) return EMURX_EINVAL;
    int rc = bind(h);
    if (rc) return rc;
    IngestSlot& s = h->ing[slot];
    if (s.pending) return EMURX_EINVAL;
    if (!on || s.h_flw.p) {  // off, or sized by an earlier call
        s.flw_on = on != 0;
        return EMURX_OK;
    }
    // everything the stage needs, now: no submit allocates or synchronises for it.  A folded frame
    // is at least 42 bytes long (l3 >= 14, 20 bytes of IPv4 header and 8 of UDP, or more), so a
    // batch has at most max_bytes / 42 events beside emurx_ftstat_max_events: the fold's ev_cap,
    // which no batch can exceed, and the capacity of the pinned block.
    if (!h->ans_ev && !EMURX_HIP_OK(hipEventCreateWithFlags(&h->ans_ev, hipEventDisableTiming))) return EMURX_EDEVICE;
    const uint32_t mf = std::min<uint32_t>(h->cfg.max_frames, EMURX_TX_ZMQ_MAX_FRAMES - 1);
    const uint32_t cap = (uint32_t)std::min<uint64_t>(emurx_ftstat_max_events(h), (uint64_t)h->cfg.max_bytes / 42 + 1);
    // the device arrays are readable to the next 16-byte boundary past any count (k_ft_out)
    if (s.d_flow.alloc((size_t)mf + 4) || s.d_fev.alloc((size_t)cap + 1) || s.d_finfo.alloc(EMURX_FT_INFO_WORDS) ||
        s.d_fto.alloc((size_t)mf + 16))
        return EMURX_ENOMEM;
    if (!EMURX_HIP_OK(hipMemset(s.d_finfo.p, 0, EMURX_FT_INFO_WORDS * sizeof(uint64_t)))) return EMURX_EDEVICE;
    auto carve = [&](uint8_t* block) {
        emurx_carver k(block);
        s.h_finfo.p = k.take<uint64_t>(EMURX_FT_INFO_WORDS);
        s.h_flow.p = k.take<uint32_t>((size_t)mf + 4);
        s.h_fto.p = k.take<uint8_t>((size_t)mf + 16);
        s.h_fev.p = k.take<emurx_ft_ev>(cap);
        return k.bytes();
    };
    if (s.h_flw.alloc(carve(nullptr))) return EMURX_ENOMEM;
    carve(s.h_flw.p);
    memset(s.h_finfo.p, 0, EMURX_FT_INFO_WORDS * sizeof(uint64_t));
    s.flw_ev_cap = cap;
    s.flw_on = true;
    return EMURX_OK;
}

int emurx_ingest_flows(emurx_t* h, uint32_t slot, emurx_flows_out* out) {
    if (!h || !out || slot >= EMURX_INGEST_SLOTS) return EMURX_EINVAL;
    const IngestSlot& s = h->ing[slot];
    if (s.pending || !s.waited) return EMURX_EINVAL;
    if (!s.flw_batch) return EMURX_ENOENT;
    memset(out, 0, sizeof(*out));
    out->flow = s.h_flow.p;
    out->outcome = s.h_fto.p;
    out->ev = s.h_fev.p;
    out->n_ev = (uint32_t)s.h_finfo.p[0];
    memcpy(out->info, s.h_finfo.p, sizeof(out->info));
    return EMURX_OK;
}

int emurx_ingest_answers(emurx_t* h, uint32_t slot, emurx_answers* out) {
    if (!h || !out || slot >= EMURX_INGEST_SLOTS) return EMURX_EINVAL;
    const IngestSlot& s = h->ing[slot];
    if (s.pending || !s.waited) return EMURX_EINVAL;
    if (!s.ans_batch) return EMURX_ENOENT;
    const uint64_t* hd = s.h_ahead.p;
    memset(out, 0, sizeof(*out));
    out->tx = s.h_tx.p;
    out->tx_msg_off = s.h_tx_off.p;
    out->n_tx_msgs = (uint32_t)hd[EMURX_ANS_HEAD_TX];
    out->n_replies = (uint32_t)hd[0];
    out->tx_bytes = hd[EMURX_ANS_HEAD_TX + 1];
    out->reply_src = s.h_src.p;
    out->rsp_outcome = s.h_rspo.p;
    out->lrn_outcome = s.h_lrno.p;
    out->done = s.h_donef.p;
    out->learn_ev = s.h_lev.p;
    out->n_learn = (uint32_t)hd[EMURX_ANS_HEAD_LRN];
    out->ns_ev = s.h_nsev.p;
    out->n_ns = (uint32_t)hd[EMURX_ANS_HEAD_NSS];
    memcpy(out->rsp_info, hd, sizeof(out->rsp_info));
    memcpy(out->lrn_info, hd + EMURX_ANS_HEAD_LRN, sizeof(out->lrn_info));
    memcpy(out->nss_info, hd + EMURX_ANS_HEAD_NSS, sizeof(out->nss_info));
    return EMURX_OK;
}

}  // extern "C"

// ---- the resident ping templates and their generator (emurx_pingtx_*) ---------------------------
namespace {

// Ship the edited template slots on `st`: behind every stream that read the store since the last
// shipment, ahead of every later reader (ship_tables' rule, with the store's own bookkeeping).
// The staging buffers hold stage_cap slots each; more edits take several of them, and a buffer
// still in use by an earlier k_ptx_apply is waited for on the host.
int ship_pingtx(emurx_t* h, hipStream_t st) {
    PingTx& x = h->ptx;
    for (size_t k = 0; k < x.readers.size(); ++k) {
        if (x.readers[k] == st) continue;
        if (!EMURX_HIP_OK(hipEventRecord(x.reader_ev[k], x.readers[k])) ||
            !EMURX_HIP_OK(hipStreamWaitEvent(st, x.reader_ev[k], 0)))
            return EMURX_EDEVICE;
    }
    for (size_t at = 0; at < x.dirty.size(); at += x.stage_cap) {
        const uint32_t k = x.stage_i++ % kDeltaRing;
        if (x.stage_used[k] && !EMURX_HIP_OK(hipEventSynchronize(x.stage_ev[k]))) return EMURX_EDEVICE;
        const uint32_t cnt = (uint32_t)std::min<size_t>(x.stage_cap, x.dirty.size() - at);
        for (uint32_t j = 0; j < cnt; ++j) {
            const uint32_t id = x.dirty[at + j];
            uint8_t* e = x.stage[k].p + (size_t)j * PingTx::kEntry;
            memset(e, 0, 16);
            memcpy(e, &id, 4);
            memcpy(e + 16, &x.shadow[(size_t)id * EMURX_PINGTX_SLOT], EMURX_PINGTX_SLOT);
            x.marked[id] = 0;
        }
        if (emurx_launch_pingtx_apply(x.stage[k].p, cnt, x.d_store.p, st) || !EMURX_HIP_OK(hipEventRecord(x.stage_ev[k], st)))
            return EMURX_EDEVICE;
        x.stage_used[k] = true;
    }
    x.dirty.clear();
    if (!EMURX_HIP_OK(hipEventRecord(x.ship_ev, st))) return EMURX_EDEVICE;
    ++x.ship_gen;
    x.readers.clear();
    return EMURX_OK;
}

// Before a launch on `st` that reads the store: ship pending edits, or wait for the last shipment
// if this stream has not yet; remember st as a reader for the next shipment.
int pingtx_prepare_read(emurx_t* h, hipStream_t st) {
    PingTx& x = h->ptx;
    int rc;
    uint64_t* w = nullptr;
    for (auto& e : x.waited)
        if (e.first == st) w = &e.second;
    if (!w) {
        if (x.waited.size() >= 4 * kMaxReaders) x.waited.clear();  // forgotten streams wait again: harmless
        x.waited.emplace_back(st, 0);  // within the capacity emurx_pingtx_reserve set
        w = &x.waited.back().second;
    }
    if (!x.dirty.empty()) {
        if ((rc = ship_pingtx(h, st))) return rc;
    } else if (*w < x.ship_gen) {
        if (!EMURX_HIP_OK(hipStreamWaitEvent(st, x.ship_ev, 0))) return EMURX_EDEVICE;
    }
    *w = x.ship_gen;
    if (std::find(x.readers.begin(), x.readers.end(), st) == x.readers.end()) {
        if (x.readers.size() >= kMaxReaders) {  // many distinct streams: drain them all once
            if (!EMURX_HIP_OK(hipDeviceSynchronize())) return EMURX_EDEVICE;
            x.readers.clear();
        }
        x.readers.push_back(st);
    }
    return EMURX_OK;
}

// one generator call on st: behind the store's shipment and the scratch's previous user
int pingtx_run(emurx_t* h, const emurx_pingtx_req* d_req, uint32_t n_req, uint8_t* d_out, uint64_t out_cap,
               emurx_desc* d_out_desc, uint32_t desc_cap, uint32_t off_base, uint8_t* fzero0, uint8_t* fzero1,
               uint8_t* d_outcome, uint64_t* d_info, hipStream_t st) {
    PingTx& x = h->ptx;
    int rc;
    if ((rc = pingtx_prepare_read(h, st))) return rc;
    if (x.scr_recorded && !EMURX_HIP_OK(hipStreamWaitEvent(st, x.scr_ev, 0))) return EMURX_EDEVICE;
    if (emurx_launch_pingtx(d_req, n_req, x.d_store.p, x.max, d_out, out_cap, d_out_desc, desc_cap, off_base, fzero0, fzero1,
                            d_outcome, d_info, x.d_scratch.p, st) ||
        !EMURX_HIP_OK(hipEventRecord(x.scr_ev, st)))
        return EMURX_EDEVICE;
    x.scr_recorded = true;
    return EMURX_OK;
}

void pingtx_mark(PingTx& x, uint32_t id) {
    if (x.marked[id]) return;
    x.marked[id] = 1;
    x.dirty.push_back(id);  // at most one entry per id: within the reserved capacity
}

}  // namespace

extern "C" {

int emurx_pingtx_reserve(emurx_t* h, uint32_t max_pings) {
    if (!h || max_pings == 0 || max_pings > (1u << 24)) return EMURX_EINVAL;
    int rc = bind(h);
    if (rc) return rc;
    PingTx& x = h->ptx;
    if (x.max) return EMURX_EEXIST;
    const size_t bytes = (size_t)max_pings * EMURX_PINGTX_SLOT;
    auto fail = [&](int code) {
        x.release();
        return code;
    };
    try {
        x.shadow.assign(bytes, 0);
        x.len.assign(max_pings, 0);
        x.marked.assign(max_pings, 0);
        x.dirty.clear();
        x.dirty.reserve(max_pings);
        x.free_ids.resize(max_pings);
        for (uint32_t i = 0; i < max_pings; ++i) x.free_ids[i] = i;  // ascending: a min-heap as it stands
        x.limbo.assign(max_pings, PingTx::Limbo{});
        x.readers.reserve(kMaxReaders);
        x.waited.reserve(4 * kMaxReaders);
    } catch (...) {  // bad_alloc, length_error: no exception crosses the ABI
        return fail(EMURX_ENOMEM);
    }
    x.limbo_head = x.limbo_n = 0;
    x.stage_cap = std::min<uint32_t>(max_pings, 1024);
    if (x.d_store.alloc(bytes + 16) || x.d_scratch.alloc(emurx_ptx_scratch_bytes(h->cfg.max_frames))) return fail(EMURX_ENOMEM);
    for (int k = 0; k < kDeltaRing; ++k) {
        if (x.stage[k].alloc((size_t)x.stage_cap * PingTx::kEntry)) return fail(EMURX_ENOMEM);
        if (!EMURX_HIP_OK(hipEventCreateWithFlags(&x.stage_ev[k], hipEventDisableTiming))) return fail(EMURX_EDEVICE);
        x.stage_used[k] = false;
    }
    for (auto& e : x.reader_ev)
        if (!EMURX_HIP_OK(hipEventCreateWithFlags(&e, hipEventDisableTiming))) return fail(EMURX_EDEVICE);
    if (!EMURX_HIP_OK(hipEventCreateWithFlags(&x.ship_ev, hipEventDisableTiming)) ||
        !EMURX_HIP_OK(hipEventCreateWithFlags(&x.scr_ev, hipEventDisableTiming)) ||
        !EMURX_HIP_OK(hipMemset(x.d_store.p, 0, bytes + 16)))  // every slot free
        return fail(EMURX_EDEVICE);
    x.scr_recorded = false;
    x.ship_gen = 0;
    x.max = max_pings;
    return EMURX_OK;
}

int emurx_pingtx_add(emurx_t* h, const uint8_t* tmpl, uint32_t len, uint32_t icmp_off, uint32_t vport, uint32_t* id) {
    if (!h || !tmpl || !id) return EMURX_EINVAL;
    PingTx& x = h->ptx;
    if (!x.max || len > EMURX_PINGTX_MAX_LEN || icmp_off > len || icmp_off + 24 > len || vport > 255) return EMURX_EINVAL;
    if (be16(tmpl + icmp_off + 2) == 0xffff) return EMURX_EINVAL;  // the chain depends on its path there
    // the removed ids whose last readers have been waited for may be handed out again
    while (x.limbo_n) {
        const PingTx::Limbo& l = x.limbo[x.limbo_head];
        bool ready = true;
        for (int k = 0; k < EMURX_EGRESS_SLOTS; ++k) ready = ready && h->egr[k].ping_done >= l.seq[k];
        if (!ready) break;
        x.free_ids.push_back(l.id);  // within the capacity: an id is in one place at a time
        std::push_heap(x.free_ids.begin(), x.free_ids.end(), std::greater<uint32_t>());
        x.limbo_head = (x.limbo_head + 1) % x.max;
        --x.limbo_n;
    }
    if (x.free_ids.empty()) return EMURX_ENOSPC;
    std::pop_heap(x.free_ids.begin(), x.free_ids.end(), std::greater<uint32_t>());
    const uint32_t i = x.free_ids.back();
    x.free_ids.pop_back();
    uint8_t* s = &x.shadow[(size_t)i * EMURX_PINGTX_SLOT];
    memset(s, 0, EMURX_PINGTX_SLOT);
    const uint16_t l16 = (uint16_t)len, o16 = (uint16_t)icmp_off;
    memcpy(s, &l16, 2);
    memcpy(s + 2, &o16, 2);
    s[4] = (uint8_t)vport;
    memcpy(s + 8, tmpl, len);
    x.len[i] = l16;
    pingtx_mark(x, i);
    *id = i;
    return EMURX_OK;
}

int emurx_pingtx_remove(emurx_t* h, uint32_t id) {
    if (!h) return EMURX_EINVAL;
    PingTx& x = h->ptx;
    if (id >= x.max || !x.len[id]) return EMURX_ENOENT;
    x.len[id] = 0;
    memset(&x.shadow[(size_t)id * EMURX_PINGTX_SLOT], 0, 8);  // len 0: free
    pingtx_mark(x, id);
    PingTx::Limbo& l = x.limbo[(x.limbo_head + x.limbo_n++) % x.max];
    l.id = id;
    for (int k = 0; k < EMURX_EGRESS_SLOTS; ++k) l.seq[k] = h->egr[k].ping_seq;
    return EMURX_OK;
}

int emurx_pingtx_dev(emurx_t* h, const emurx_pingtx_req* d_req, uint32_t n_req, uint8_t* d_out, uint64_t out_cap,
                     emurx_desc* d_out_desc, uint32_t desc_cap, uint8_t* d_outcome, uint64_t* d_info, void* stream) {
    if (!h || !d_info || (n_req && (!d_req || !d_out_desc || (!d_out && out_cap)))) return EMURX_EINVAL;
    if (((uintptr_t)d_out & 15) || ((uintptr_t)d_req & 7) || ((uintptr_t)d_out_desc & 7) || ((uintptr_t)d_info & 7))
        return EMURX_EINVAL;
    int rc = bind(h);
    if (rc) return rc;
    if (!h->ptx.max) return EMURX_EINVAL;
    if (n_req > h->cfg.max_frames) return EMURX_ENOMEM;
    hipStream_t st = stream ? (hipStream_t)stream : h->stream;
    if ((rc = not_capturing(st))) return rc;
    return pingtx_run(h, d_req, n_req, d_out, out_cap, d_out_desc, desc_cap, 0, nullptr, nullptr, d_outcome, d_info, st);
}

}  // extern "C"

// ---- the tx planner and the egress slots ---------------------------------------------------------
extern "C" {

int emurx_tx_plan_dev(emurx_t* h, const uint8_t* d_frames, const emurx_desc* d_desc, uint32_t n, uint32_t flags,
                      emurx_tx_desc* d_txdesc, uint8_t* d_outcome, uint64_t* d_info, void* stream) {
    if (!h || !d_info || (flags & ~EMURX_TXP_UDP0_KEEP) || (n && (!d_frames || !d_desc || !d_txdesc))) return EMURX_EINVAL;
    if (((uintptr_t)d_desc & 7) || ((uintptr_t)d_txdesc & 15) || ((uintptr_t)d_info & 7)) return EMURX_EINVAL;
    if (n > h->cfg.max_frames) return EMURX_ENOMEM;
    int rc = bind(h);
    if (rc) return rc;
    hipStream_t st = stream ? (hipStream_t)stream : h->stream;
    if ((rc = not_capturing(st))) return rc;
    return emurx_launch_tx_plan(d_frames, d_desc, n, flags, d_txdesc, d_outcome, d_info, st) ? EMURX_EDEVICE : EMURX_OK;
}

int emurx_egress_buffer(emurx_t* h, uint32_t slot, uint8_t** frames, emurx_desc** desc) {
    if (!h || !frames || !desc || slot >= EMURX_EGRESS_SLOTS) return EMURX_EINVAL;
    int rc = bind(h);
    if (rc) return rc;
    EgressSlot& s = h->egr[slot];
    if (s.pending) return EMURX_EINVAL;
    if (!s.h_res.p) {
        // everything the chain needs, now: no submit allocates or synchronises for it.  The
        // framing scratch may be in use by launches in flight, so the device is idle before it grows.
        if (!EMURX_HIP_OK(hipDeviceSynchronize())) return EMURX_EDEVICE;
        const uint32_t mf = std::min<uint32_t>(h->cfg.max_frames, EMURX_TX_ZMQ_MAX_FRAMES - 1);
        const size_t mb = h->cfg.max_bytes;
        if (!s.st && !EMURX_HIP_OK(hipStreamCreateWithFlags(&s.st, hipStreamNonBlocking))) return EMURX_EDEVICE;
        if (!s.done && !EMURX_HIP_OK(hipEventCreateWithFlags(&s.done, hipEventDisableTiming))) return EMURX_EDEVICE;
        if (!h->ans_ev && !EMURX_HIP_OK(hipEventCreateWithFlags(&h->ans_ev, hipEventDisableTiming))) return EMURX_EDEVICE;
        if ((rc = txz_reserve(h, mf, h->stream))) return rc;
        // the plain framing call's feedback words and event (emurx_tx_zmq_dev creates them on demand)
        if (!h->txz_ev && (h->txz_fb.alloc(2) || !EMURX_HIP_OK(hipEventCreateWithFlags(&h->txz_ev, hipEventDisableTiming))))
            return EMURX_ENOMEM;
        const uint64_t cap = (8ull * mf + mb + 15) & ~15ull;
        // device arrays with slack: frames are read as the aligned 16-byte blocks that hold them,
        // and k_egr_out reads to the next 16-byte boundary past any count
        if (s.h_frames.alloc(mb + 64) || s.h_desc.alloc((size_t)mf + 1) || s.d_frames.alloc(mb + 64) ||
            s.d_desc.alloc((size_t)mf + 2) || s.d_txd.alloc((size_t)mf + 1) || s.d_plan.alloc((size_t)mf + 16) ||
            s.d_status.alloc((size_t)mf + 16) || s.d_tx.alloc(cap + 16) || s.d_msg_off.alloc((size_t)mf + 3) ||
            s.d_info.alloc(EMURX_EGR_HEAD_WORDS))
            return EMURX_ENOMEM;
        if (!EMURX_HIP_OK(hipMemset(s.d_info.p, 0, EMURX_EGR_HEAD_WORDS * sizeof(uint64_t)))) return EMURX_EDEVICE;
        auto carve = [&](uint8_t* block) {
            emurx_carver k(block);
            s.h_head.p = k.take<uint64_t>(EMURX_EGR_HEAD_WORDS);
            s.h_msg_off.p = k.take<uint64_t>((size_t)mf + 2);
            s.h_plan.p = k.take<uint8_t>((size_t)mf + 16);
            s.h_status.p = k.take<uint8_t>((size_t)mf + 16);
            s.h_tx.p = k.take<uint8_t>(cap);
            return k.bytes();
        };
        if (s.h_res.alloc(carve(nullptr))) return EMURX_ENOMEM;
        carve(s.h_res.p);
        memset(s.h_head.p, 0, EMURX_EGR_HEAD_WORDS * sizeof(uint64_t));
        s.cap = cap;
    }
    *frames = s.h_frames.p;
    *desc = s.h_desc.p;
    return EMURX_OK;
}

// emurx_egress_submit and emurx_egress_submit_ping: n plain frames, then the frames of n_req echo
// requests (none: the plain submit, enqueue for enqueue)
static int egress_submit(emurx_t* h, uint32_t slot, uint32_t n, uint64_t bytes, uint32_t flags, uint32_t n_req) {
    if (!h || slot >= EMURX_EGRESS_SLOTS || (flags & ~EMURX_TXP_UDP0_KEEP)) return EMURX_EINVAL;
    int rc = bind(h);
    if (rc) return rc;
    EgressSlot& s = h->egr[slot];
    if (s.pending || !s.h_res.p) return EMURX_EINVAL;  // in flight, or no emurx_egress_buffer yet
    if (n_req && !s.h_req.p) return EMURX_EINVAL;      // no emurx_egress_ping_buffer yet
    if (n > h->cfg.max_frames || n_req > h->cfg.max_frames) return EMURX_ENOMEM;
    if (bytes > h->cfg.max_bytes || n >= EMURX_TX_ZMQ_MAX_FRAMES) return EMURX_ENOSPC;
    const emurx_desc* hd = s.h_desc.p;
    for (uint32_t i = 0; i < n; ++i)
        if ((uint64_t)hd[i].off + hd[i].len > bytes) return EMURX_EINVAL;
    // the requests against the per-id lengths: G frames and B bytes, exact
    uint64_t G = 0, B = 0;
    for (uint32_t r = 0; r < n_req; ++r) {
        const emurx_pingtx_req& q = s.h_req.p[r];
        if (q.id >= h->ptx.max || !h->ptx.len[q.id]) return EMURX_EINVAL;
        G += q.count;
        B += (uint64_t)q.count * ((h->ptx.len[q.id] + 15u) & ~15u);
    }
    const uint64_t gen_at = (bytes + 15) & ~15ull;  // the generated frames' place in the frame area
    if (n + G > h->cfg.max_frames) return EMURX_ENOMEM;
    if (n_req && gen_at + B > h->cfg.max_bytes) return EMURX_ENOSPC;
    if (n + G >= EMURX_TX_ZMQ_MAX_FRAMES) return EMURX_ENOSPC;
    const uint32_t nf = n + (uint32_t)G;
    hipStream_t st = s.st;
    uint64_t* plan_info = s.d_info.p;
    uint64_t* tx_info = s.d_info.p + EMURX_TXP_INFO_WORDS;
    // 1. the frames, their descriptors and the requests; 2. the plan; 3. the checksums, in place
    if (bytes && !EMURX_HIP_OK(hipMemcpyAsync(s.d_frames.p, s.h_frames.p, bytes, hipMemcpyHostToDevice, st))) return EMURX_EDEVICE;
    if (n && !EMURX_HIP_OK(hipMemcpyAsync(s.d_desc.p, hd, (size_t)n * sizeof(emurx_desc), hipMemcpyHostToDevice, st)))
        return EMURX_EDEVICE;
    if (n_req && !EMURX_HIP_OK(hipMemcpyAsync(s.d_req.p, s.h_req.p, (size_t)n_req * sizeof(emurx_pingtx_req),
                                              hipMemcpyHostToDevice, st)))
        return EMURX_EDEVICE;
    if (emurx_launch_tx_plan(s.d_frames.p, s.d_desc.p, n, flags, s.d_txd.p, s.d_plan.p, plan_info, st) ||
        emurx_launch_tx_csum(s.d_frames.p, s.d_txd.p, n, s.d_status.p, st))
        return EMURX_EDEVICE;
    if (n_req) {
        // the generated frames behind the plain ones, their descriptors from index n on; they are
        // finished as they are written: the generator gives each EMURX_TXP_NONE / EMURX_TX_OK
        if ((rc = pingtx_run(h, s.d_req.p, n_req, s.d_frames.p + gen_at, B, s.d_desc.p + n, (uint32_t)G, (uint32_t)gen_at,
                             s.d_plan.p + n, s.d_status.p + n, nullptr, s.d_pinfo.p, st)))
            return rc;
        ++s.ping_seq;
    }
    // 4. the framing, whose scratch is the handle's: behind the previous user's event, and the
    // next one (an ingest slot's answer stages, another egress batch) waits for this one's
    const uint64_t out_cap = 8ull * nf + bytes + B;
    if (h->ans_recorded && !EMURX_HIP_OK(hipStreamWaitEvent(st, h->ans_ev, 0))) return EMURX_EDEVICE;
    if ((rc = emurx_tx_zmq_dev(h, s.d_frames.p, s.d_desc.p, nf, s.d_tx.p, out_cap, s.d_msg_off.p, tx_info, st))) return rc;
    if (!EMURX_HIP_OK(hipEventRecord(h->ans_ev, st))) return EMURX_EDEVICE;
    h->ans_recorded = true;
    // 5. what was produced, into the pinned result block
    const emurx_egr_out a{reinterpret_cast<const unsigned long long*>(plan_info),
                          reinterpret_cast<const unsigned long long*>(tx_info),
                          s.d_tx.p,
                          reinterpret_cast<const unsigned long long*>(s.d_msg_off.p),
                          s.d_plan.p,
                          s.d_status.p,
                          reinterpret_cast<uint8_t*>(s.h_head.p),
                          s.h_tx.p,
                          reinterpret_cast<uint8_t*>(s.h_msg_off.p),
                          s.h_plan.p,
                          s.h_status.p,
                          out_cap,
                          nf};
    if (emurx_launch_egr_out(a, st) || !EMURX_HIP_OK(hipEventRecord(s.done, st))) return EMURX_EDEVICE;
    s.n = nf;
    s.tx_cap = out_cap;
    s.pending = true;
    s.submitted = true;
    return EMURX_OK;
}

int emurx_egress_submit(emurx_t* h, uint32_t slot, uint32_t n, uint64_t bytes, uint32_t flags) {
    return egress_submit(h, slot, n, bytes, flags, 0);
}

int emurx_egress_ping_buffer(emurx_t* h, uint32_t slot, emurx_pingtx_req** req) {
    if (!h || !req || slot >= EMURX_EGRESS_SLOTS) return EMURX_EINVAL;
    int rc = bind(h);
    if (rc) return rc;
    EgressSlot& s = h->egr[slot];
    if (s.pending || !s.h_res.p || !h->ptx.max) return EMURX_EINVAL;
    if (!s.h_req.p) {
        const size_t mf = std::max<size_t>(h->cfg.max_frames, 1);
        if (s.h_req.alloc(mf) || s.d_req.alloc(mf) || s.d_pinfo.alloc(EMURX_PTX_INFO_WORDS)) return EMURX_ENOMEM;
    }
    *req = s.h_req.p;
    return EMURX_OK;
}

int emurx_egress_submit_ping(emurx_t* h, uint32_t slot, uint32_t n, uint64_t bytes, uint32_t flags, uint32_t n_req) {
    return egress_submit(h, slot, n, bytes, flags, n_req);
}

int emurx_egress_wait(emurx_t* h, uint32_t slot, emurx_egress_result* res) {
    if (!h || !res || slot >= EMURX_EGRESS_SLOTS) return EMURX_EINVAL;
    int rc = bind(h);
    if (rc) return rc;
    EgressSlot& s = h->egr[slot];
    if (!s.submitted) return EMURX_EINVAL;
    if (s.pending) {
        if (!EMURX_HIP_OK(hipEventSynchronize(s.done))) return EMURX_EDEVICE;
        s.pending = false;
        s.ping_done = s.ping_seq;  // removed template ids this batch may have read can be handed out again
    }
    const uint64_t* hd = s.h_head.p;
    const uint64_t nmsg = hd[EMURX_TXP_INFO_WORDS], txb = hd[EMURX_TXP_INFO_WORDS + 1];
    // the framing never needs more than 8 n + bytes for frames that do not overlap
    if (nmsg > s.n || txb > s.tx_cap) return EMURX_ENOSPC;
    memset(res, 0, sizeof(*res));
    res->msgs = s.h_tx.p;
    res->msg_off = s.h_msg_off.p;
    res->n_msgs = (uint32_t)nmsg;
    res->n_frames = s.n;
    res->bytes = txb;
    res->plan = s.h_plan.p;
    res->status = s.h_status.p;
    memcpy(res->plan_info, hd, sizeof(res->plan_info));
    return EMURX_OK;
}

}  // extern "C"

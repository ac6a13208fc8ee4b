"""RxPath — Python surface of the C-ABI, shaped like the reference's rx entry points.

    RxPath.register(name)         Parser.Register          src/emu/core/parser.go:528-565
    RxPath.ns_add / ns_remove     CThreadCtx.AddNs/RemoveNs src/emu/core/thread_ctx.go:786-812
    RxPath.client_add / remove    CNSCtx.AddClient/RemoveClient src/emu/core/ns_ctx.go:332-440
    RxPath.on_rx_stream(msg)      VethIFZmq.OnRxStream     src/emu/core/veth_zmq.go:277-320
    RxPath.classify_dev(...)      the same, device-resident (frames already in HBM)

Device memory is plain torch CUDA tensors (plumbing only); every call goes through
libemurx.so — there is no Python or CPU implementation of the data path.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import abi


def _u8(x, n):
    if x is None:
        return None
    a = np.frombuffer(bytes(x), dtype=np.uint8).copy()
    if a.size != n:
        raise ValueError(f"expected {n} bytes, got {a.size}")
    return a


def _p(a):
    return None if a is None else a.ctypes.data


class RxPath:
    """device < 0: a host-only handle (table mirror, generations, image queries; no GPU)."""

    def __init__(self, device: int = 0, max_ns: int = 4096, max_clients: int = 65536,
                 max_frames: int = 1 << 20, max_bytes: int = 1 << 20):
        self.lib = abi.load()
        cfg = abi.Cfg(device, max_ns, max_clients, max_frames, max_bytes)
        h = C.c_void_p()
        abi.check(self.lib.emurx_open(C.byref(cfg), C.byref(h)), "emurx_open")
        self.h = h
        self.cfg = cfg

    def close(self):
        if getattr(self, "h", None):
            self.lib.emurx_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    # ---- registration ----------------------------------------------------------------
    def register(self, protocol: str):
        return abi.check(self.lib.emurx_register(self.h, protocol.encode()), "register")

    def register_all(self):
        for p in ("arp", "icmp", "igmp", "dhcp", "dhcpsrv", "icmpv6", "dhcpv6", "dot1x", "mdns",
                  "ppp", "transport"):
            self.register(p)

    def set_callbacks_mask(self, mask: int):
        return abi.check(self.lib.emurx_set_callbacks_mask(self.h, mask), "set_callbacks_mask")

    @property
    def callbacks_mask(self) -> int:
        return int(self.lib.emurx_get_callbacks_mask(self.h))

    # ---- tables (return codes are passed through: they mirror Go's error returns) ------
    def ns_add(self, key: bytes, ns_id: int, plugins: int = abi.PLUG_ALL) -> int:
        k = _u8(key, 12)
        return self.lib.emurx_ns_add(self.h, _p(k), ns_id, plugins)

    def ns_remove(self, key: bytes) -> int:
        k = _u8(key, 12)
        return self.lib.emurx_ns_remove(self.h, _p(k))

    def ns_set_plugins(self, ns_id: int, plugins: int) -> int:
        return self.lib.emurx_ns_set_plugins(self.h, ns_id, plugins)

    def client_add(self, ns_id, cid, mac, ipv4=None, ipv6=None, dhcpv6=None,
                   plugins: int = abi.PLUG_ALL) -> int:
        a = [_u8(mac, 6), _u8(ipv4, 4), _u8(ipv6, 16), _u8(dhcpv6, 16)]
        return self.lib.emurx_client_add(self.h, ns_id, cid, *[_p(x) for x in a], plugins)

    def clients_add(self, spec: np.ndarray) -> tuple[int, int]:
        """ctx_client_add: CLIENT_SPEC_DTYPE rows in order -> (rc of the first failure or 0,
        clients added)."""
        a = np.ascontiguousarray(spec, dtype=abi.CLIENT_SPEC_DTYPE)
        k = C.c_uint32()
        rc = self.lib.emurx_clients_add(self.h, _p(a) if len(a) else None, len(a), C.byref(k))
        return rc, k.value

    def client_remove(self, ns_id, mac) -> int:
        m = _u8(mac, 6)
        return self.lib.emurx_client_remove(self.h, ns_id, _p(m))

    def client_set_plugins(self, cid, plugins) -> int:
        return self.lib.emurx_client_set_plugins(self.h, cid, plugins)

    def client_update_ipv4(self, cid, ip) -> int:
        a = _u8(ip, 4)
        return self.lib.emurx_client_update_ipv4(self.h, cid, _p(a))

    def client_update_ipv6(self, cid, ip) -> int:
        a = _u8(ip, 16)
        return self.lib.emurx_client_update_ipv6(self.h, cid, _p(a))

    def client_update_dipv6(self, cid, ip) -> int:
        a = _u8(ip, 16)
        return self.lib.emurx_client_update_dipv6(self.h, cid, _p(a))

    def client_set_ra(self, cid, prefix, plen) -> int:
        a = _u8(prefix, 16)
        return self.lib.emurx_client_set_ra(self.h, cid, _p(a), plen)

    # transport flow tables (TransportCtx.addFlowv4/6, serverCb; include/emu_rx.h)
    def flow_add(self, cid, tuple_bytes, flow_id) -> int:
        t = np.frombuffer(bytes(tuple_bytes), np.uint8).copy()
        rc = self.lib.emurx_flow_add(self.h, cid, _p(t), len(t), flow_id)
        self._transport = self.any_transport or rc == 0
        return rc

    def flow_remove(self, cid, tuple_bytes) -> int:
        t = np.frombuffer(bytes(tuple_bytes), np.uint8).copy()
        return self.lib.emurx_flow_remove(self.h, cid, _p(t), len(t))

    def server_add(self, cid, port, proto) -> int:
        rc = self.lib.emurx_server_add(self.h, cid, port, proto)
        self._transport = self.any_transport or rc == 0
        return rc

    def server_remove(self, cid, port, proto) -> int:
        return self.lib.emurx_server_remove(self.h, cid, port, proto)

    def client_set_transport(self, cid, has_ctx) -> int:
        rc = self.lib.emurx_client_set_transport(self.h, cid, int(has_ctx))
        self._transport = self.any_transport or (rc == 0 and bool(has_ctx))
        return rc

    def sync(self, stream=None):
        return abi.check(self.lib.emurx_sync(self.h, stream), "sync")

    # ---- host batch (ZMQ message) ------------------------------------------------------
    def on_rx_stream(self, msg: bytes, cap: int | None = None):
        cap = cap or int(self.cfg.max_frames)
        m = np.frombuffer(bytes(msg), dtype=np.uint8).copy() if len(msg) else np.zeros(1, np.uint8)
        rec = np.zeros(cap, dtype=abi.REC_DTYPE)
        qlist = np.zeros(cap, dtype=np.uint32)
        qoff = np.zeros(abi.NUM_QUEUES + 1, dtype=np.uint32)
        cnt = abi.Counters()
        n = C.c_uint32()
        abi.check(self.lib.emurx_rx_stream(self.h, _p(m), len(msg), _p(rec), _p(qlist), cap,
                                           C.byref(n), _p(qoff), C.byref(cnt)), "rx_stream")
        k = n.value
        return rec[:k], qlist[:k], qoff, cnt

    # ---- device-resident batch -----------------------------------------------------------
    def classify_dev(self, frames, desc, n: int, rec=None, qlist=None, qcap: int = 0, tile_cnt=None,
                     hist=None, stream=None, classify: bool = True, flow=None):
        """frames/desc/rec/qlist/tile_cnt/hist: device tensors (or raw device addresses).
        Tile t's frames of queue q land in qlist[q*qcap + t*QUEUE_TILE :][:tile_cnt[t*16+q]]
        (see pack_queues); hist holds HIST_SHARDS accumulating copies (see hist_fold)."""
        out = abi.DevOut(_addr(rec), _addr(qlist), qcap, _addr(tile_cnt), _addr(hist), _addr(flow))
        fn = self.lib.emurx_classify_dev if classify else self.lib.emurx_parse_dev
        return abi.check(fn(self.h, _addr(frames), _addr(desc), n, C.byref(out),
                            _stream(stream)), "classify_dev")

    def classify_call(self, frames, desc, n: int, rec=None, qlist=None, qcap: int = 0, tile_cnt=None,
                      hist=None, stream=None, classify: bool = True, flow=None):
        """classify_dev with every argument resolved once: returns a zero-argument callable
        that enqueues the same batch again (one C call, no Python-side argument work)."""
        out = abi.DevOut(_addr(rec), _addr(qlist), qcap, _addr(tile_cnt), _addr(hist), _addr(flow))
        fn = self.lib.emurx_classify_dev if classify else self.lib.emurx_parse_dev
        args = (self.h, _addr(frames), _addr(desc), n, C.byref(out), _stream(stream))

        def call():
            rc = fn(*args)
            if rc:
                abi.check(rc, "classify_dev")
        call.keep = out
        return call

    def set_timing(self, slots: int = 1024, stride: int = 1):
        """Time every `stride`-th batch with HIP events (0 slots disables)."""
        return abi.check(self.lib.emurx_set_timing(self.h, slots, stride), "set_timing")

    def kernel_times(self, cap: int = 1 << 16):
        """Device ms of every batch launched since the previous call (HIP events recorded on
        the launch stream around the k_rx launch)."""
        a = np.zeros(cap, np.float32)
        n = C.c_uint32()
        abi.check(self.lib.emurx_kernel_times(self.h, _p(a), cap, C.byref(n)), "kernel_times")
        return a[: n.value]

    def last_stage(self) -> int:
        """LDS staging bytes per wave of the most recent k_rx launch (7168 or 6144)."""
        return int(self.lib.emurx_last_stage(self.h))

    def last_uniform(self) -> np.ndarray:
        """Which path the sampled waves of the most recent k_rx launch took (waits for the
        device): 256 words, [(tile // 64 % 64) * 4 + wave] = abi.UNI_SAMPLED | abi.UNI_PARSE |
        abi.UNI_LOOKUP for a sampled wave (the waves of every 64th tile), 0 otherwise."""
        w = np.zeros(abi.UNI_WORDS, np.uint32)
        abi.check(self.lib.emurx_last_uniform(self.h, _p(w)), "last_uniform")
        return w

    def last_trim(self) -> np.ndarray:
        """The same sampled waves as last_uniform, same layout: abi.UNI_SAMPLED | abi.TRIM_RANGE
        (the wave took its byte range from its end lanes instead of reducing)."""
        w = np.zeros(abi.UNI_WORDS, np.uint32)
        abi.check(self.lib.emurx_last_trim(self.h, _p(w)), "last_trim")
        return w

    def last_txz(self) -> int:
        """LDS image bytes per wave of the last tx framing write (6144, 4608, 0; -1 before)."""
        return int(self.lib.emurx_last_txz(self.h))

    # ---- batched host ingest (many ZMQ messages per GPU round trip) -------------------------
    def ingest_buffer(self, slot: int, nbytes: int) -> np.ndarray:
        """The slot's pinned staging buffer as a writable uint8 view of `nbytes`."""
        p = C.c_void_p()
        abi.check(self.lib.emurx_ingest_buffer(self.h, slot, nbytes, C.byref(p)), "ingest_buffer")
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(max(nbytes, 1),))[:nbytes]

    def ingest_submit(self, slot: int, msgs) -> None:
        """msgs: MSG_DTYPE array (or [(off, len), ...]) of messages in the slot buffer."""
        a = np.asarray(msgs)
        a = np.ascontiguousarray(a).view(np.uint32) if a.dtype.names else np.asarray(msgs, dtype=np.uint32)
        m = np.ascontiguousarray(a).reshape(-1, 2)
        abi.check(self.lib.emurx_ingest_submit(self.h, slot, _p(m) if len(m) else None, len(m)),
                  "ingest_submit")

    def ingest_stream(self, slot: int) -> int:
        """The slot's hipStream_t as an integer (for torch.cuda.ExternalStream)."""
        p = C.c_void_p()
        abi.check(self.lib.emurx_ingest_stream(self.h, slot, C.byref(p)), "ingest_stream")
        return int(p.value)

    def ingest_wait(self, slot: int, copy: bool = True) -> dict:
        """Results of the slot's batch: rec, desc, qlist, qoff, msg_frames, msg_status,
        counters (views into library memory unless copy)."""
        r = abi.IngestResult()
        abi.check(self.lib.emurx_ingest_wait(self.h, slot, C.byref(r)), "ingest_wait")
        n, m = int(r.n_frames), int(r.n_msgs)

        def view(ptr, count, dt):
            if not count:
                return np.zeros(0, dt)
            b = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(count * np.dtype(dt).itemsize,))
            v = b.view(dt)
            return v.copy() if copy else v
        return dict(rec=view(r.rec, n, abi.REC_DTYPE), desc=view(r.desc, n, abi.DESC_DTYPE),
                    qlist=view(r.qlist, n, np.uint32), qoff=np.array(r.qoff, np.uint32),
                    msg_frames=view(r.msg_frames, m, np.uint32), msg_status=view(r.msg_status, m, np.uint8),
                    counters=r.delta.as_dict(), n=n, one_launch=bool(r.one_launch), degraded=bool(r.degraded))

    def ingest_set_answers(self, slot: int, kinds: int) -> None:
        """Run the device answer chain (respond, tx framing, learn, nsstat) on the slot's later
        batches: kinds abi.RSPK_* bits, 0 turns it off (include/emu_rx.h emurx_ingest_set_answers)."""
        if kinds & abi.RSPK_TS:  # the timestamp reply: its own entry point (the slot's time: ingest_set_time)
            abi.check(self.lib.emurx_ingest_set_answers_ts(self.h, slot, kinds), "ingest_set_answers_ts")
            return
        abi.check(self.lib.emurx_ingest_set_answers(self.h, slot, kinds), "ingest_set_answers")

    def ingest_set_time(self, slot: int, ip_time: int) -> None:
        """The time of day (milliseconds since midnight UTC, the reference's iptime()) that the
        slot's next submits put into timestamp replies (include/emu_rx.h emurx_ingest_set_time)."""
        abi.check(self.lib.emurx_ingest_set_time(self.h, slot, ip_time & 0xFFFFFFFF), "ingest_set_time")

    def ingest_answers(self, slot: int, n_frames: int) -> dict:
        """The answers of the slot's batch, after its ingest_wait (n_frames: that result's n), as
        numpy copies: tx (the framed replies), tx_msg_off, reply_src, rsp_outcome, lrn_outcome,
        done, learn_ev, ns_ev, rsp_info, lrn_info, nss_info, n_replies, n_tx_msgs, tx_bytes."""
        a = abi.Answers()
        abi.check(self.lib.emurx_ingest_answers(self.h, slot, C.byref(a)), "ingest_answers")

        def copy(ptr, count, dt):
            if not count:
                return np.zeros(0, dt)
            b = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(count * np.dtype(dt).itemsize,))
            return b.view(dt).copy()
        return dict(tx=copy(a.tx, int(a.tx_bytes), np.uint8), tx_msg_off=copy(a.tx_msg_off, a.n_tx_msgs + 1, np.uint64),
                    reply_src=copy(a.reply_src, a.n_replies, np.uint32), rsp_outcome=copy(a.rsp_outcome, n_frames, np.uint8),
                    lrn_outcome=copy(a.lrn_outcome, n_frames, np.uint8), done=copy(a.done, n_frames, np.uint8),
                    learn_ev=copy(a.learn_ev, a.n_learn, abi.LEARN_EV_DTYPE), ns_ev=copy(a.ns_ev, a.n_ns, abi.NSSTAT_EV_DTYPE),
                    rsp_info=np.array(a.rsp_info, np.uint64), lrn_info=np.array(a.lrn_info, np.uint64),
                    nss_info=np.array(a.nss_info, np.uint64), n_replies=int(a.n_replies), n_tx_msgs=int(a.n_tx_msgs),
                    tx_bytes=int(a.tx_bytes))

    def ingest_set_ping(self, slot: int, fams: int) -> None:
        """Run the ping fold behind nsstat in the slot's answer chain on its later batches: fams
        abi.PNGK_* bits, 0 turns it off; answers must be on (include/emu_rx.h emurx_ingest_set_ping)."""
        abi.check(self.lib.emurx_ingest_set_ping(self.h, slot, fams), "ingest_set_ping")

    def ingest_set_now(self, slot: int, now_unix_ns: int) -> None:
        """The time.Now().UnixNano() that the slot's next submits pass to the ping fold
        (include/emu_rx.h emurx_ingest_set_now)."""
        abi.check(self.lib.emurx_ingest_set_now(self.h, slot, now_unix_ns), "ingest_set_now")

    def ingest_ping(self, slot: int, n_frames: int) -> dict:
        """The ping fold of the slot's batch, after its ingest_wait (n_frames: that result's n), as
        numpy copies: ev (abi.PING_EV_DTYPE, ascending `last`), outcome u8 [n_frames], info."""
        a = abi.PingOut()
        abi.check(self.lib.emurx_ingest_ping(self.h, slot, C.byref(a)), "ingest_ping")

        def copy(ptr, count, dt):
            if not count:
                return np.zeros(0, dt)
            b = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(count * np.dtype(dt).itemsize,))
            return b.view(dt).copy()
        return dict(ev=copy(a.ev, a.n_ev, abi.PING_EV_DTYPE), outcome=copy(a.outcome, n_frames, np.uint8),
                    info=np.array(a.info, np.uint64))

    def ingest_set_flows(self, slot: int, on: bool) -> None:
        """Return the per-frame flow words and fold the refused TCP / UDP frames on the slot's later
        batches; independent of answers (include/emu_rx.h emurx_ingest_set_flows)."""
        abi.check(self.lib.emurx_ingest_set_flows(self.h, slot, 1 if on else 0), "ingest_set_flows")

    def ingest_flows(self, slot: int, n_frames: int) -> dict:
        """The flow decisions of the slot's batch, after its ingest_wait (n_frames: that result's
        n), as numpy copies: flow u32 [n_frames], outcome u8 [n_frames], ev (abi.FT_EV_DTYPE,
        ascending `last`), info."""
        a = abi.FlowsOut()
        abi.check(self.lib.emurx_ingest_flows(self.h, slot, C.byref(a)), "ingest_flows")

        def copy(ptr, count, dt):
            if not count:
                return np.zeros(0, dt)
            b = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(count * np.dtype(dt).itemsize,))
            return b.view(dt).copy()
        return dict(flow=copy(a.flow, n_frames, np.uint32), outcome=copy(a.outcome, n_frames, np.uint8),
                    ev=copy(a.ev, a.n_ev, abi.FT_EV_DTYPE), info=np.array(a.info, np.uint64))

    # ---- tx-side checksum generation ------------------------------------------------------
    def tx_checksum_dev(self, frames, desc, n: int, status=None, stream=None):
        """Rewrite the checksums selected by each TX_DESC_DTYPE descriptor, in place on the
        device buffer `frames` (include/emu_rx.h emurx_tx_checksum_dev)."""
        return abi.check(self.lib.emurx_tx_checksum_dev(self.h, _addr(frames), _addr(desc), n, _addr(status),
                                                        _stream(stream)), "tx_checksum_dev")

    def tx_zmq_dev(self, frames, desc, n: int, out, cap: int, msg_off, info, stream=None):
        """Pack the n frames into ZMQ messages as VethIFZmq.Send x n + FlushTx would
        (include/emu_rx.h emurx_tx_zmq_dev): messages back to back in `out`, msg_off u64
        [n + 1], info u64 {n_msgs, total bytes}."""
        return abi.check(self.lib.emurx_tx_zmq_dev(self.h, _addr(frames), _addr(desc), n, _addr(out), cap,
                                                   _addr(msg_off), _addr(info), _stream(stream)), "tx_zmq_dev")

    def tx_zmq_counted_dev(self, frames, desc, n_max: int, count, out, cap: int, msg_off, info, stream=None):
        """tx_zmq_dev over the first min(count[0], n_max) descriptors, `count` a u64 in device
        memory read when the kernels run (include/emu_rx.h emurx_tx_zmq_counted_dev): the
        responder's info is the intended count.  msg_off u64 [n_max + 1]."""
        return abi.check(self.lib.emurx_tx_zmq_counted_dev(self.h, _addr(frames), _addr(desc), n_max, _addr(count),
                                                           _addr(out), cap, _addr(msg_off), _addr(info),
                                                           _stream(stream)), "tx_zmq_counted_dev")

    def tx_plan_dev(self, frames, desc, n: int, txdesc, outcome, info, flags: int = 0, stream=None):
        """The TX_DESC_DTYPE descriptor of every frame, derived from the frame itself
        (include/emu_rx.h emurx_tx_plan_dev): txdesc [n], outcome u8 [n] (abi.TXP_*, may be None),
        info u64 [abi.TXP_INFO_WORDS]; flags abi.TXP_UDP0_KEEP."""
        return abi.check(self.lib.emurx_tx_plan_dev(self.h, _addr(frames), _addr(desc), n, flags, _addr(txdesc),
                                                    _addr(outcome), _addr(info), _stream(stream)), "tx_plan_dev")

    # ---- egress slots: tx from host memory ------------------------------------------------
    def egress_buffer(self, slot: int):
        """The slot's pinned frame area (uint8 [cfg.max_bytes]) and descriptor array (abi.DESC_DTYPE
        [cfg.max_frames]) as writable views (include/emu_rx.h emurx_egress_buffer)."""
        f, d = C.c_void_p(), C.c_void_p()
        abi.check(self.lib.emurx_egress_buffer(self.h, slot, C.byref(f), C.byref(d)), "egress_buffer")
        mb, mf = int(self.cfg.max_bytes), int(self.cfg.max_frames)
        frames = np.ctypeslib.as_array(C.cast(f, C.POINTER(C.c_uint8)), shape=(max(mb, 1),))[:mb]
        desc = np.ctypeslib.as_array(C.cast(d, C.POINTER(C.c_uint8)), shape=(max(mf, 1) * 8,)).view(abi.DESC_DTYPE)[:mf]
        return frames, desc

    def egress_submit(self, slot: int, n: int, nbytes: int, flags: int = 0) -> None:
        """Enqueue the slot's first n descriptors and nbytes of frames: plan, checksums, framing
        (include/emu_rx.h emurx_egress_submit)."""
        abi.check(self.lib.emurx_egress_submit(self.h, slot, n, nbytes, flags), "egress_submit")

    def egress_wait(self, slot: int, copy: bool = True) -> dict:
        """The slot's finished batch: msgs (the ZMQ messages back to back), msg_off u64 [n_msgs + 1],
        plan and status u8 [n_frames], plan_info, n_msgs, n_frames, bytes (views into library
        memory unless copy)."""
        r = abi.EgressResult()
        abi.check(self.lib.emurx_egress_wait(self.h, slot, C.byref(r)), "egress_wait")

        def view(ptr, count, dt):
            if not count:
                return np.zeros(0, dt)
            b = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(count * np.dtype(dt).itemsize,))
            v = b.view(dt)
            return v.copy() if copy else v
        n, m = int(r.n_frames), int(r.n_msgs)
        return dict(msgs=view(r.msgs, int(r.bytes), np.uint8), msg_off=view(r.msg_off, m + 1, np.uint64),
                    plan=view(r.plan, n, np.uint8), status=view(r.status, n, np.uint8),
                    plan_info=np.array(r.plan_info, np.uint64), n_msgs=m, n_frames=n, bytes=int(r.bytes))

    # ---- the send side of ping: resident templates ------------------------------------------
    def pingtx_reserve(self, max_pings: int) -> int:
        """Allocate the template store for max_pings pings, once per handle (include/emu_rx.h
        emurx_pingtx_reserve); the error code is returned."""
        return self.lib.emurx_pingtx_reserve(self.h, max_pings)

    def pingtx_add(self, tmpl: bytes, icmp_off: int, vport: int) -> tuple[int, int]:
        """A Ping's packet template into the store (emurx_pingtx_add): (error code, id)."""
        i = C.c_uint32(0xFFFFFFFF)
        rc = self.lib.emurx_pingtx_add(self.h, bytes(tmpl), len(tmpl), icmp_off, vport, C.byref(i))
        return rc, int(i.value)

    def pingtx_remove(self, tid: int) -> int:
        return self.lib.emurx_pingtx_remove(self.h, tid)

    def pingtx_dev(self, req, n_req: int, out, cap: int, out_desc, desc_cap: int, outcome, info, stream=None):
        """The echo requests of n_req abi.PINGTX_REQ_DTYPE requests (device memory), generated from
        the resident templates (include/emu_rx.h emurx_pingtx_dev): frames at 16-byte aligned
        offsets in `out`, out_desc [desc_cap] (the descriptors tx_zmq_dev takes), outcome u8 [n_req]
        (abi.PTX_*, or None), info u64[abi.PTX_INFO_WORDS].  The error code is returned."""
        return self.lib.emurx_pingtx_dev(self.h, _addr(req), n_req, _addr(out), cap, _addr(out_desc), desc_cap,
                                         _addr(outcome), _addr(info), _stream(stream))

    def egress_ping_buffer(self, slot: int) -> np.ndarray:
        """The slot's pinned request array (abi.PINGTX_REQ_DTYPE [cfg.max_frames]) as a writable view
        (include/emu_rx.h emurx_egress_ping_buffer)."""
        p = C.c_void_p()
        abi.check(self.lib.emurx_egress_ping_buffer(self.h, slot, C.byref(p)), "egress_ping_buffer")
        mf = int(self.cfg.max_frames)
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(max(mf, 1) * 16,)).view(abi.PINGTX_REQ_DTYPE)[:mf]

    def egress_submit_ping(self, slot: int, n: int, nbytes: int, n_req: int, flags: int = 0) -> int:
        """egress_submit with the frames of the slot's first n_req requests behind the n plain frames
        (include/emu_rx.h emurx_egress_submit_ping); the error code is returned."""
        return self.lib.emurx_egress_submit_ping(self.h, slot, n, nbytes, flags, n_req)

    def respond_dev(self, frames, desc, rec, n: int, out, cap: int, out_desc, out_src, outcome, info, stream=None,
                    kinds=None, ip_time=None):
        """The ARP / ICMPv4 echo / ICMPv6 echo replies of a classified batch, built on the device
        (include/emu_rx.h emurx_respond_dev): replies compacted in rx order into `out` at 16-byte
        aligned offsets, out_desc / out_src [n] (the descriptors tx_zmq_dev takes, the rx frame
        index), outcome u8 [n] (abi.RSP_*, or None), info u64[8] {n_out, bytes needed, frames per
        outcome 1..6}.  With kinds (abi.RSPK_*, emurx_respond_kinds_dev) only the selected answers
        are built, the neighbour advertisement (RSPK_ND) among them, and info is
        u64[abi.RSP_INFO_WORDS] {n_out, bytes needed, frames per outcome 1..7, zeros}.  With ip_time
        (milliseconds since midnight UTC; emurx_respond_ts_dev) kinds may hold RSPK_TS: timestamp
        requests are answered with that time, and info counts the outcomes 1..9."""
        if ip_time is not None:
            return abi.check(self.lib.emurx_respond_ts_dev(self.h, _addr(frames), _addr(desc), _addr(rec), n,
                                                           abi.RSPK_ALL_TS if kinds is None else kinds, ip_time & 0xFFFFFFFF,
                                                           _addr(out), cap, _addr(out_desc), _addr(out_src), _addr(outcome),
                                                           _addr(info), _stream(stream)), "respond_ts_dev")
        if kinds is None:
            return abi.check(self.lib.emurx_respond_dev(self.h, _addr(frames), _addr(desc), _addr(rec), n, _addr(out), cap,
                                                        _addr(out_desc), _addr(out_src), _addr(outcome), _addr(info),
                                                        _stream(stream)), "respond_dev")
        return abi.check(self.lib.emurx_respond_kinds_dev(self.h, _addr(frames), _addr(desc), _addr(rec), n, kinds,
                                                          _addr(out), cap, _addr(out_desc), _addr(out_src), _addr(outcome),
                                                          _addr(info), _stream(stream)), "respond_kinds_dev")

    def learn_max_events(self) -> int:
        """The largest ev_cap learn_dev takes: half the slot count of the handle's set."""
        return int(self.lib.emurx_learn_max_events(self.h))

    def learn_dev(self, frames, desc, rec, n: int, ev, ev_cap: int, outcome, info, kinds: int = abi.LRNK_ALL,
                  stream=None):
        """The ARP / ND cache learning of a classified batch folded on the device into one event
        per distinct (ns, kind, ip, mac) (include/emu_rx.h emurx_learn_dev): ev
        abi.LEARN_EV_DTYPE [ev_cap], written in ascending `last`; outcome u8 [n] (abi.LRN_*, or
        None); info u64[abi.LRN_INFO_WORDS] {events written, distinct keys, overflow, frames per
        outcome 1..5}.  On overflow (distinct keys > ev_cap) no event is written."""
        return abi.check(self.lib.emurx_learn_dev(self.h, _addr(frames), _addr(desc), _addr(rec), n, kinds, _addr(ev),
                                                  ev_cap, _addr(outcome), _addr(info), _stream(stream)), "learn_dev")

    def nsstat_max_events(self) -> int:
        """The largest ev_cap nsstat_dev takes: min(max_frames, max_ns)."""
        return int(self.lib.emurx_nsstat_max_events(self.h))

    def nsstat_dev(self, frames, desc, rec, n: int, rsp_outcome, lrn_outcome, ev, ev_cap: int, done, info,
                   kinds: int = abi.RSPK_ALL, stream=None):
        """The ARP / ICMP / ICMPv6 / ND handlers' per-Namespace counters of a classified batch, folded
        on the device (include/emu_rx.h emurx_nsstat_dev): rsp_outcome / lrn_outcome u8 [n] are the
        outcome arrays of respond_dev(kinds=...) and learn_dev on the same batch (lrn_outcome may be
        None without RSPK_ARP and RSPK_ND); ev abi.NSSTAT_EV_DTYPE [ev_cap], written in ascending
        ns_id; done u8 [n] (0 the Go handler runs, 1 skip it, 2 skip it and count errParser; or
        None); info u64[abi.NSS_INFO_WORDS] {events written, distinct Namespaces, overflow, frames
        done 1, done 2, candidates left at 0, 0, 0}.  On overflow (distinct > ev_cap) no event is
        written.  With RSPK_TS in kinds (emurx_nsstat_ts_dev) rsp_outcome is that of
        respond_dev(kinds=..., ip_time=...)."""
        if kinds & abi.RSPK_TS:
            return abi.check(self.lib.emurx_nsstat_ts_dev(self.h, _addr(frames), _addr(desc), _addr(rec), n, kinds,
                                                          _addr(rsp_outcome), _addr(lrn_outcome), _addr(ev), ev_cap,
                                                          _addr(done), _addr(info), _stream(stream)), "nsstat_ts_dev")
        return abi.check(self.lib.emurx_nsstat_dev(self.h, _addr(frames), _addr(desc), _addr(rec), n, kinds,
                                                   _addr(rsp_outcome), _addr(lrn_outcome), _addr(ev), ev_cap, _addr(done),
                                                   _addr(info), _stream(stream)), "nsstat_dev")

    def ping_max_events(self) -> int:
        """The largest ev_cap ping_dev takes (that of learn_dev)."""
        return int(self.lib.emurx_ping_max_events(self.h))

    def ping_dev(self, frames, desc, rec, n: int, now_unix_ns: int, ev, ev_cap: int, outcome, info,
                 fams: int = abi.PNGK_ALL, stream=None):
        """The echo replies and destination-unreachable messages of a classified batch folded on the
        device into one event per {ns_id, client_id, family, ident} (include/emu_rx.h
        emurx_ping_dev): now_unix_ns is the batch's one time.Now().UnixNano(); ev abi.PING_EV_DTYPE
        [ev_cap], written in ascending `last`; outcome u8 [n] (abi.PNG_*, or None); info
        u64[abi.PNG_INFO_WORDS] {events written, distinct keys, overflow, frames per outcome 1..5}.
        On overflow (distinct keys > ev_cap) no event is written."""
        return abi.check(self.lib.emurx_ping_dev(self.h, _addr(frames), _addr(desc), _addr(rec), n, fams, now_unix_ns,
                                                 _addr(ev), ev_cap, _addr(outcome), _addr(info), _stream(stream)),
                         "ping_dev")

    def ftstat_max_events(self) -> int:
        """The largest ev_cap ftstat_dev takes: min(max_frames, max_clients)."""
        return int(self.lib.emurx_ftstat_max_events(self.h))

    def ftstat_dev(self, frames, desc, rec, flow, n: int, ev, ev_cap: int, outcome, info, stream=None):
        """The TCP / UDP frames of a classified batch that the transport plugin refuses, folded on the
        device into one event per client (include/emu_rx.h emurx_ftstat_dev): flow u32 [n] is the
        flow array of the classify_dev call that wrote rec; ev abi.FT_EV_DTYPE [ev_cap], written in
        ascending `last`; outcome u8 [n] (abi.FT_* | abi.FT_V6, or None); info u64[abi.FT_INFO_WORDS]
        {events written, distinct clients, overflow, frames NO_SYN, NO_SRV_TCP, NO_SRV_UDP, ERR,
        candidates left at NONE}.  On overflow (distinct clients > ev_cap) no event is written."""
        return abi.check(self.lib.emurx_ftstat_dev(self.h, _addr(frames), _addr(desc), _addr(rec), _addr(flow), n, _addr(ev),
                                                   ev_cap, _addr(outcome), _addr(info), _stream(stream)), "ftstat_dev")

    # ---- Namespace-partitioned exchange ---------------------------------------------------
    def classify_route_dev(self, frames, desc, n: int, rec, qlist, qcap: int, tile_cnt, hist, n_parts: int,
                           my_rank: int, cap: int, send, send_count, stream=None, flow=None):
        """classify_dev + route_dev in one call, the route's counting pass inside k_rx
        (include/emu_rx.h emurx_classify_route_dev)."""
        out = abi.DevOut(_addr(rec), _addr(qlist), qcap, _addr(tile_cnt), _addr(hist), _addr(flow))
        return abi.check(self.lib.emurx_classify_route_dev(self.h, _addr(frames), _addr(desc), n, C.byref(out),
                                                           n_parts, my_rank, cap, _addr(send), _addr(send_count),
                                                           _stream(stream)), "classify_route_dev")

    def route_dev(self, rec, n: int, n_parts: int, my_rank: int, cap: int, send, send_count, stream=None):
        """Pack the batch's records with a Namespace into their owners' send regions
        (send[d*cap:][:send_count[d]], frame order; include/emu_rx.h emurx_route_dev)."""
        return abi.check(self.lib.emurx_route_dev(self.h, _addr(rec), n, n_parts, my_rank, cap, _addr(send),
                                                  _addr(send_count), _stream(stream)), "route_dev")

    # ---- owner-partitioned classification ----------------------------------------------------
    def set_partition(self, n_parts: int, part: int):
        """Device tables hold only the Namespaces this partition owns (emurx_set_partition)."""
        return abi.check(self.lib.emurx_set_partition(self.h, n_parts, part), "set_partition")

    def parse_route_dev(self, frames, desc, n: int, rec, qlist, qcap: int, tile_cnt, hist, n_parts: int,
                        my_rank: int, cap: int, send, send_count, stream=None, tail_cap=None):
        """Parse + lookup keys, packed into the owners' regions (abi.lookup_region_bytes(cap,
        tail_cap) bytes each: LOOKUP_REC_DTYPE heads + tail shards); send_count [2 * n_parts]
        {heads, tail overflow}.  tail_cap defaults to default_tail_cap(cap)."""
        if tail_cap is None:
            tail_cap = self.default_tail_cap(cap)
        out = abi.DevOut(_addr(rec), _addr(qlist), qcap, _addr(tile_cnt), _addr(hist), None)
        return abi.check(self.lib.emurx_parse_route_dev(self.h, _addr(frames), _addr(desc), n, C.byref(out),
                                                        n_parts, my_rank, cap, tail_cap, _addr(send),
                                                        _addr(send_count), _stream(stream)), "parse_route_dev")

    def default_tail_cap(self, cap: int) -> int:
        """Tail units per shard when the caller gives none: room for a sixteenth of
        the heads to carry one unit (ICMPv6 keys), or, once any client has a TransportCtx (tcp /
        udp heads then carry their c5tuplekey: 1 unit over IPv4, 3 over IPv6), for every head to
        carry three.  A shard that still overflows is reported in send_count[2 d + 1]."""
        return abi.tail_capacity(cap, 3.0 if self.any_transport else 1 / 16)

    @property
    def any_transport(self) -> bool:
        """Some client has a TransportCtx on this handle (flows, listeners or the mark): what
        makes the source attach tuples (emurx_parse_route_dev)."""
        return bool(getattr(self, "_transport", False))

    def desc_keys_dev(self, frames, desc, n: int, stream=None):
        """Write every frame's owner key into its descriptor's pad byte, in place
        (include/emu_rx.h emurx_desc_keys_dev): what the device framing walk does."""
        return abi.check(self.lib.emurx_desc_keys_dev(self.h, _addr(frames), _addr(desc), n, _stream(stream)),
                         "desc_keys_dev")

    def zmq_walk_dev(self, buf, ctl, nmsg: int, desc, msg_stat, keys: bool = True, stream=None):
        """The framing walk alone on device-resident messages (include/emu_rx.h
        emurx_zmq_walk_dev): ctl = emurx_msg[nmsg] then slot_base[nmsg + 1] (uint32)."""
        return abi.check(self.lib.emurx_zmq_walk_dev(self.h, _addr(buf), _addr(ctl), nmsg, _addr(desc),
                                                     _addr(msg_stat), 0 if keys else abi.WALK_NO_KEYS,
                                                     _stream(stream)), "zmq_walk_dev")

    def lookup_dev(self, recv, recv_count, n_parts: int, cap: int, out, flow=None, stream=None, tail_cap=None):
        """The owner's lookups over received lookup regions (parse_route_dev's layout; recv_count
        [2 * n_parts]) -> ROUTE_REC_DTYPE slots."""
        if tail_cap is None:
            tail_cap = self.default_tail_cap(cap)
        return abi.check(self.lib.emurx_lookup_dev(self.h, _addr(recv), _addr(recv_count), n_parts, cap, tail_cap,
                                                   _addr(out), _addr(flow), _stream(stream)), "lookup_dev")

    # ---- the library-owned communicator (include/emu_rx.h emurx_comm_*, emurx_exchange_dev) ----
    def comm_init(self, uid: bytes, nranks: int, rank: int):
        """Join the exchange's communicator (ncclCommInitRank; blocks until every rank joined).
        uid: comm_unique_id() of one rank, handed to every rank out of band."""
        u = _u8(uid, abi.COMM_ID_BYTES)
        _torch_first()
        return abi.check(self.lib.emurx_comm_init(self.h, _p(u), nranks, rank), "comm_init")

    def comm_destroy(self):
        return abi.check(self.lib.emurx_comm_destroy(self.h), "comm_destroy")

    def comm_info(self):
        """(nranks, rank) of the handle's communicator, or None."""
        a, b = C.c_uint32(), C.c_uint32()
        rc = self.lib.emurx_comm_info(self.h, C.byref(a), C.byref(b))
        if rc == abi.EMURX_ENOENT:
            return None
        abi.check(rc, "comm_info")
        return a.value, b.value

    def exchange_dev(self, send, send_count, recv, recv_count, cap: int, tail_cap=None, payload: bool = False,
                     route: bool = False, stream=None) -> int:
        """One exchange of the owners' regions over the handle's communicator (RCCL): region r
        of every rank's send into region s of rank r's recv, counts alongside.  Lookup regions
        (parse_route_dev) unless route (classify_route_dev's route records).  Returns the bytes
        sent to other ranks."""
        tail_cap = (self.default_tail_cap(cap) if tail_cap is None else tail_cap) if not route else 0
        moved = C.c_uint64()
        flags = (abi.XCH_PAYLOAD if payload else abi.XCH_EQUAL) | (abi.XCH_ROUTE if route else 0)
        abi.check(self.lib.emurx_exchange_dev(self.h, _addr(send), _addr(send_count), _addr(recv), _addr(recv_count),
                                              cap, tail_cap, flags, C.byref(moved), _stream(stream)), "exchange_dev")
        return moved.value

    # ---- table generations / image diagnostics -------------------------------------------------
    def table_gen(self) -> int:
        return int(self.lib.emurx_table_gen(self.h))

    def recs_stale(self, rec: np.ndarray, gen: int) -> np.ndarray:
        """emurx_recs_stale: 1 where a record may differ from the live tables' answer."""
        r = np.ascontiguousarray(rec, dtype=abi.REC_DTYPE)
        out = np.zeros(max(len(r), 1), np.uint8)
        abi.check(self.lib.emurx_recs_stale(self.h, _p(r) if len(r) else None, len(r), gen, _p(out)),
                  "recs_stale")
        return out[: len(r)]

    def image_lookup(self, table: int, key) -> int | None:
        k = np.ascontiguousarray(key, dtype=np.uint32)
        v = C.c_uint32()
        rc = self.lib.emurx_image_lookup(self.h, table, _p(k), C.byref(v))
        if rc == abi.EMURX_ENOENT:
            return None
        abi.check(rc, "image_lookup")
        return v.value

    def image_probe(self, table: int, key) -> dict:
        """emurx_image_probe: image_lookup's walk with its trace.  value None when absent;
        buckets 0 where the walk read nothing (a client key of a dead Namespace)."""
        k = np.ascontiguousarray(key, dtype=np.uint32)
        out = np.zeros(6, np.uint32)
        rc = self.lib.emurx_image_probe(self.h, table, _p(k), _p(out))
        if rc != abi.EMURX_ENOENT:
            abi.check(rc, "image_probe")
        v, nb, home, reads, wrapped, tombs = (int(x) for x in out)
        return dict(value=None if rc == abi.EMURX_ENOENT else v, buckets=nb, home=home, reads=reads,
                    wrapped=bool(wrapped), tombstones=tombs)

    def image_check(self) -> int:
        """32-bit words where the device tables differ from the host image (0 = in sync)."""
        v = C.c_uint64()
        abi.check(self.lib.emurx_image_check(self.h, C.byref(v)), "image_check")
        return v.value

    def table_stats(self) -> dict:
        """Blocks shipped as deltas, whole tables uploaded, bytes of the device tables."""
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        abi.check(self.lib.emurx_table_stats(self.h, C.byref(a), C.byref(b), C.byref(c)), "table_stats")
        return dict(delta_blocks=a.value, whole_tables=b.value, table_bytes=c.value)


def comm_library():
    """Path of the RCCL the library's communicators use (emurx_comm_library: bound at the first
    call), or None when none loads."""
    _torch_first()
    b = C.create_string_buffer(1024)
    rc = abi.load().emurx_comm_library(b, 1024)
    return b.value.decode() if rc == abi.EMURX_OK else None


def _torch_first():
    """Before the library binds RCCL (its first communicator call): torch, when installed, is
    imported first, so that the process has one ROCm runtime and one RCCL (torch's bundled
    ones).  The system's RCCL bound ahead of a later torch import mixes two copies of ROCm's
    libraries, and such a process aborts at exit."""
    try:
        import torch  # noqa: F401
    except ImportError:
        pass


def comm_unique_id() -> bytes:
    """A fresh communicator id (emurx_comm_unique_id, ncclGetUniqueId): one rank makes it, every
    rank passes it to RxPath.comm_init."""
    _torch_first()
    b = np.zeros(abi.COMM_ID_BYTES, np.uint8)
    abi.check(abi.load().emurx_comm_unique_id(_p(b)), "comm_unique_id")
    return b.tobytes()


def comm_init_all(paths) -> None:
    """One communicator over several handles of this process, one GPU each (emurx_comm_init_all):
    handle k is rank k."""
    _torch_first()
    hs = (C.c_void_p * len(paths))(*[p.h.value for p in paths])
    abi.check(abi.load().emurx_comm_init_all(hs, len(paths)), "comm_init_all")


def group_start():
    _torch_first()
    abi.check(abi.load().emurx_group_start(), "group_start")


def group_end():
    abi.check(abi.load().emurx_group_end(), "group_end")


def owner_key(key: bytes) -> int:
    """The descriptor owner key of a 12-byte CTunnelKey (EMURX_DESC_KEYED | 7-bit digest)."""
    return int(abi.load().emurx_owner_key(_p(_u8(key, 12))))


def ns_owner(key: bytes, n_parts: int) -> int:
    """Partition (GPU) owning the Namespace with this 12-byte CTunnelKey."""
    k = np.frombuffer(bytes(key), np.uint8).copy()
    assert k.size == 12
    return int(abi.load().emurx_ns_owner(_p(k), n_parts))


def _addr(x):
    if x is None:
        return None
    if isinstance(x, int):
        return x
    return x.data_ptr()


def _stream(s):
    if s is None:
        return None
    if isinstance(s, int):
        return s
    return s.cuda_stream


def zmq_descriptors(msg: bytes, cap: int = 1 << 16):
    lib = abi.load()
    m = np.frombuffer(bytes(msg), dtype=np.uint8).copy() if len(msg) else np.zeros(1, np.uint8)
    d = np.zeros(cap, dtype=abi.DESC_DTYPE)
    n, e = C.c_uint32(), C.c_int()
    rc = lib.emurx_zmq_descriptors(_p(m), len(msg), _p(d), cap, C.byref(n), C.byref(e))
    return rc, d[:n.value], e.value


def hist_fold(shards: np.ndarray) -> np.ndarray:
    """[HIST_SHARDS * 2 * HIST_BINS] device histogram copies -> [2 * HIST_BINS] (C-ABI)."""
    lib = abi.load()
    s = np.ascontiguousarray(shards, dtype=np.uint64).reshape(-1)
    assert s.size == abi.HIST_SHARDS * 2 * abi.HIST_BINS
    out = np.zeros(2 * abi.HIST_BINS, np.uint64)
    lib.emurx_hist_fold(_p(s), _p(out))
    return out


def pack_queues(qlist: np.ndarray, qcap: int, tile_cnt: np.ndarray, n: int):
    """Per-tile queue segments -> (frame indices in queue order, qoff[NUM_QUEUES + 1]):
    queue q = qlist_packed[qoff[q]:qoff[q+1]], frames in order (the host side of
    emurx_rx_stream's packing)."""
    nt = abi.ntiles(n)
    ql = np.asarray(qlist).view(np.uint32).reshape(abi.NUM_QUEUES, -1)[:, : nt * abi.QUEUE_TILE]
    cnt = np.asarray(tile_cnt).view(np.uint32).reshape(-1, 16)[:nt, : abi.NUM_QUEUES].astype(np.int64)
    assert (cnt <= abi.QUEUE_TILE).all()
    seg = ql.reshape(abi.NUM_QUEUES, nt, abi.QUEUE_TILE)
    keep = np.arange(abi.QUEUE_TILE)[None, None, :] < cnt.T[:, :, None]
    packed = seg[keep].astype(np.uint32)  # C order: queue, tile, slot
    qoff = np.zeros(abi.NUM_QUEUES + 1, np.uint32)
    qoff[1:] = np.cumsum(cnt.sum(0))
    return packed, qoff


def hist_to_counters(hist: np.ndarray) -> dict:
    lib = abi.load()
    h = np.ascontiguousarray(hist, dtype=np.uint64)
    cnt = abi.Counters()
    lib.emurx_hist_to_counters(_p(h), C.byref(cnt))
    return cnt.as_dict()

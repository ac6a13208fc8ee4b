"""Python restatement, frame by frame, of what the ICMPv4 and ICMPv6 handlers and Ping do with an
echo reply or a destination-unreachable message, of the fold emurx_ping_dev makes of a batch of
them, and of the replay of its events.

    ping_ref(frame, rec, env, fams, now, hole) -> Item (outcome, key, seq, cls, lat)
    handle(item, state)          one frame the way Go handles it
    fold(items) -> events        emurx_ping_dev's events of a batch, in ascending `last`
    replay(events, state)        INTEGRATION.md's loop

rec: the frame's record (emurx.abi.REC_DTYPE, from the oracle or emurx_classify_dev); env: Env, the
MAC map of the handle.  The rule, with the reference's lines (paths relative to src/emu/plugins):

  considered only if status OK, the descriptor no hole, callback icmp / icmpv6 as fams selects;
  header offsets that do not fit the frame (emurx_nsstat_dev's tests) -> HOST
  icmp    HandleRxIcmpPacket icmp/icmp.go:396-462: the classifier has done CLookupByIPv4(dst) and
          IsUnicastToMe (:417-427); lookup other than CLIENT / CLIENT_NO_PLUGIN -> NONE; type, code
          other than (0,0), (3,0..4) -> NONE (:438-456); source neither loopback nor global unicast
          -> MCAST (:433-436); l4 != l3 + 20 -> HOST (IPv4.DecodeFromBytes over 20 bytes fails for
          IHL > 5, gopacket layers/ip4.go:336-343; icmp.go:336-340, :369-373); client without the
          plugin -> NO_CLIENT (GetIcmpClientByMac :349-351, :384-386; the record says CLIENT); HandleEchoReply :328-358 -> handleEchoReply
          :180-193 (payload < 16 -> HOST); HandleDestinationUnreachable :361-393 (the nested header
          at l4 + 28 needs 8 bytes, :378 -> HOST), identifier p[l4+32:l4+34]
  icmpv6  HandleRxIpv6Packet ipv6/ipv6.go:517-532, Namespace level: HandleEchoReply :359-406 (len <
          24 -> HOST :389), HandleDestinationUnreachable :408-462 (len < 72 -> HOST :445; the nested
          echo's identifier p[l4+52:l4+54], where ICMPv6Echo.DecodeFromBytes of p[l4+52:] reads
          it); GetIcmpClientByMac(dst MAC) :559-573, no client or none with the ipv6 plugin ->
          NO_CLIENT (:397-399, :453-455); CLookupByMac finds no zero MAC (core/ns_ctx.go:262-265)
  Ping.HandleEchoReply ping/ping.go:246-295, HandleDestinationUnreachable :298-304; the magic :198,
  the simulation's identifier 0x1234, sequence number 0xabcd (:195-196) and now 128 + 1 ms (:263-265)

No text of the reference is restated here.
"""
from dataclasses import dataclass, field

import numpy as np

from emurx import abi, frames as F

CB_ICMP, CB_ICMPV6 = 1, 9
CLS_NONE, CLS_MALFORMED, CLS_BAD_LATENCY, CLS_OK = range(4)
PLUG_ICMP, PLUG_IPV6 = 1, 8  # enum emurx_plugin: the bits of the icmp and ipv6 plugins
SIM_IDENT, SIM_SEQ, SIM_NOW, SIM_TS = 0x1234, 0xABCD, 128 + 1_000_000, 128


class Env:
    """CLookupByMac of the handle: (vport, vlan0, vlan1, mac bytes) -> (client id, plugin mask)."""

    def __init__(self):
        self.mac, self.plugins = {}, {}

    def add(self, vport, v0, v1, mac, cid, plugins):
        self.mac[(vport, v0, v1, bytes(mac))] = (cid, plugins)
        self.plugins[cid] = plugins


@dataclass
class Item:
    outcome: int
    key: tuple = None  # (ns_id, client_id, family, ident)
    seq: int = 0
    cls: int = CLS_NONE
    lat: int = 0
    why: str = ""


def ip4_src_ok(ip: bytes) -> bool:
    """net.IP.IsLoopback() || IsGlobalUnicast() of Go 1.18 for an IPv4 address (respond_ref's)."""
    if ip == bytes(4) or ip == b"\xff" * 4:
        return False
    return not (ip[0] & 0xF0 == 0xE0 or (ip[0] == 169 and ip[1] == 254))


def _reply(e: bytes, ns, cid, fam, now) -> Item:
    """e: the 24 bytes from l4 (ping.go:246-295)."""
    ident, seq = int.from_bytes(e[4:6], "big"), int.from_bytes(e[6:8], "big")
    key = (ns, cid, fam, ident)
    if int.from_bytes(e[8:16], "big") != abi.PING_MAGIC:
        return Item(abi.PNG_REPLY, key, seq, CLS_MALFORMED, 0, "reply-magic")
    ts = int.from_bytes(e[16:24], "big", signed=True)
    # latency < 0 || latency > 5 s, Time.Sub saturating: exact in Python's integers
    if ts > now or now - ts > abi.PING_TIMEOUT_NS:
        return Item(abi.PNG_REPLY, key, seq, CLS_BAD_LATENCY, 0, "reply-latency")
    return Item(abi.PNG_REPLY, key, seq, CLS_OK, now - ts, "reply-ok")


def ping_ref(frame: bytes, rec, env: Env, fams: int = abi.PNGK_ALL, now: int = SIM_NOW, hole: bool = False) -> Item:
    p, n = bytes(frame), len(frame)
    proto, lk = int(rec["proto"]), (int(rec["flags"]) >> 4) & 7
    l3, l4, ns = int(rec["l3"]), int(rec["l4"]), int(rec["ns_id"])
    if int(rec["status"]) != 0 or hole:
        return Item(abi.PNG_NONE, why="not-candidate")
    if proto == CB_ICMP and fams & abi.PNGK_V4:
        if l3 < 14 or l3 + 20 > n or l4 + 8 > n:
            return Item(abi.PNG_HOST, why="v4-bounds")
        if lk not in (abi.LK["CLIENT"], abi.LK["CLIENT_NO_PLUGIN"]):
            return Item(abi.PNG_NONE, why="v4-lookup")
        typ, code = p[l4], p[l4 + 1]
        reply = (typ, code) == (0, 0)
        if not reply and not (typ == 3 and code <= 4):
            return Item(abi.PNG_NONE, why="v4-type")
        if not ip4_src_ok(p[l3 + 12:l3 + 16]):
            return Item(abi.PNG_MCAST, (ns, abi.PING_NS_LEVEL, 4, 0), why="v4-mcast")
        if l4 != l3 + 20:
            return Item(abi.PNG_HOST, why="v4-ihl")
        cid = int(rec["client_id"])
        # the classifier gives the icmp callback CLIENT whatever the client's plugins are
        if lk == abi.LK["CLIENT_NO_PLUGIN"] or not env.plugins.get(cid, 0) & (1 << PLUG_ICMP):
            return Item(abi.PNG_NO_CLIENT, (ns, abi.PING_NS_LEVEL, 4, 0), why="v4-no-plugin")
        if reply:
            if n - (l4 + 8) < 16:
                return Item(abi.PNG_HOST, why="v4-reply-short")
            return _reply(p[l4:l4 + 24], ns, cid, 4, now)
        if n < l4 + 36:
            return Item(abi.PNG_HOST, why="v4-unreach-short")
        return Item(abi.PNG_UNREACH, (ns, cid, 4, int.from_bytes(p[l4 + 32:l4 + 34], "big")), why="v4-unreach")
    if proto == CB_ICMPV6 and fams & abi.PNGK_V6:
        if l3 < 14 or l3 + 40 > l4 or l4 + 4 > n:
            return Item(abi.PNG_HOST, why="v6-bounds")
        typ, code = p[l4], p[l4 + 1]
        reply = (typ, code) == (129, 0)
        if (not reply and not (typ == 1 and code <= 6)) or lk != abi.LK["NS_LEVEL"]:
            return Item(abi.PNG_NONE, why="v6-type-or-lookup")
        if n - l4 < (24 if reply else 72):
            return Item(abi.PNG_HOST, why="v6-short")
        hit = env.mac.get((int(rec["vport"]), int(rec["vlan0"]), int(rec["vlan1"]), p[0:6])) if p[0:6] != bytes(6) else None
        if hit is None or not hit[1] & (1 << PLUG_IPV6):
            return Item(abi.PNG_NO_CLIENT, (ns, abi.PING_NS_LEVEL, 6, 0), why="v6-no-client")
        if reply:
            return _reply(p[l4:l4 + 24], ns, hit[0], 6, now)
        return Item(abi.PNG_UNREACH, (ns, hit[0], 6, int.from_bytes(p[l4 + 52:l4 + 54], "big")), why="v6-unreach")
    return Item(abi.PNG_NONE, why="not-candidate")


def batch_items(buf, desc, rec, env, fams=abi.PNGK_ALL, now=SIM_NOW):
    out = []
    for i in range(len(desc)):
        d = desc[i]
        f = bytes(buf[int(d["off"]):int(d["off"]) + int(d["len"])])
        out.append(ping_ref(f, rec[i], env, fams, now, hole=int(d["pad"]) == abi.DESC_HOLE))
    return out


# ---- the Go state ------------------------------------------------------------------------
@dataclass
class Ping:
    """Ping's fields that a received frame touches (ping.go:139-167) and its PingStats."""
    identifier: int = SIM_IDENT
    startingSeq: int = SIM_SEQ
    firstReplyReceived: bool = False
    lastSeqReceived: int = 0
    latencySum: int = 0
    minLatency: int = 0
    maxLatency: int = 0
    repliesInOrder: int = 0
    repliesOutOfOrder: int = 0
    repliesBadIdentifier: int = 0
    repliesMalformedPkt: int = 0
    repliesBadLatency: int = 0
    dstUnreachable: int = 0


NS_COUNTERS = ("pktRxIcmpResponse", "pktRxIcmpDstUnreachable", "pktRxErrUnhandled", "pktRxNoClientUnhandled",
               "pktRxErrMulticastB")


@dataclass
class State:
    """pings: (client_id, family) -> Ping, absent = no ping running (pl.ping == nil); ns: (ns_id,
    family) -> the Namespace plugin's counters."""
    pings: dict = field(default_factory=dict)
    ns: dict = field(default_factory=dict)

    def cnt(self, ns, fam):
        return self.ns.setdefault((ns, fam), dict.fromkeys(NS_COUNTERS, 0))


def handle(it: Item, st: State):
    """One frame, as the Go handlers and Ping treat it."""
    if it.outcome in (abi.PNG_NONE, abi.PNG_HOST):
        return
    ns, cid, fam, ident = it.key
    c = st.cnt(ns, fam)
    if it.outcome == abi.PNG_NO_CLIENT:
        c["pktRxNoClientUnhandled"] += 1
        return
    if it.outcome == abi.PNG_MCAST:
        c["pktRxErrMulticastB"] += 1
        return
    pg = st.pings.get((cid, fam))
    if pg is None:  # icmp.go:186-192, :196-202
        c["pktRxErrUnhandled"] += 1
        return
    if it.outcome == abi.PNG_UNREACH:
        c["pktRxIcmpDstUnreachable"] += 1
        if ident != pg.identifier:  # ping.go:298-304
            pg.repliesBadIdentifier += 1
        else:
            pg.dstUnreachable += 1
        return
    c["pktRxIcmpResponse"] += 1
    if ident != pg.identifier:  # ping.go:247-250
        pg.repliesBadIdentifier += 1
    elif it.cls == CLS_MALFORMED:
        pg.repliesMalformedPkt += 1
    elif it.cls == CLS_BAD_LATENCY:
        pg.repliesBadLatency += 1
    else:
        if not pg.firstReplyReceived:  # :271-286
            ok = it.seq == pg.startingSeq
            pg.firstReplyReceived = True
        else:
            ok = (pg.lastSeqReceived + 1) & 0xFFFF == it.seq
        if ok:
            pg.repliesInOrder += 1
        else:
            pg.repliesOutOfOrder += 1
        pg.lastSeqReceived = it.seq
        pg.latencySum += it.lat
        if pg.minLatency == 0:  # :290-294
            pg.minLatency = it.lat
        pg.minLatency = min(pg.minLatency, it.lat)
        pg.maxLatency = max(pg.maxLatency, it.lat)


def stats(pg: Ping) -> dict:
    """updateStats ping.go:345-355, in the recorded JSON's names (microseconds)."""
    tot = pg.repliesInOrder + pg.repliesOutOfOrder
    avg = pg.latencySum // tot if tot else 0
    return dict(repliesInOrder=pg.repliesInOrder, minLatency=pg.minLatency // 1000, maxLatency=pg.maxLatency // 1000,
                avgLatency=avg // 1000)


# ---- the fold and its replay -------------------------------------------------------------
EV_FIELDS = ("first", "last", "n_reply", "n_unreach", "n_malformed", "n_bad_latency", "n_ok", "n_succ", "seq_first",
             "seq_last", "lat_sum", "lat_min_tail", "lat_max", "n_no_client", "n_mcast", "flags")


def fold(items, base: int = 0):
    """emurx_ping_dev's events for the batch `items` (frame i has index base + i): dicts in
    ascending `last`."""
    evs = {}
    for j, it in enumerate(items):
        if it.outcome in (abi.PNG_NONE, abi.PNG_HOST):
            continue
        i = base + j
        e = evs.get(it.key)
        if e is None:
            e = evs[it.key] = dict.fromkeys(EV_FIELDS, 0)
            e.update(key=it.key, first=i, prev=None)
        e["last"] = i
        if it.outcome == abi.PNG_NO_CLIENT:
            e["n_no_client"] += 1
        elif it.outcome == abi.PNG_MCAST:
            e["n_mcast"] += 1
        elif it.outcome == abi.PNG_UNREACH:
            e["n_unreach"] += 1
        else:
            e["n_reply"] += 1
            if it.cls == CLS_MALFORMED:
                e["n_malformed"] += 1
            elif it.cls == CLS_BAD_LATENCY:
                e["n_bad_latency"] += 1
            else:
                if e["n_ok"] == 0:
                    e["seq_first"] = it.seq
                elif (e["prev"] + 1) & 0xFFFF == it.seq:
                    e["n_succ"] += 1
                e["n_ok"] += 1
                e["prev"] = e["seq_last"] = it.seq
                e["lat_sum"] += it.lat
                e["lat_max"] = max(e["lat_max"], it.lat)
                if it.lat == 0:
                    e["flags"] |= 1
                    e["lat_min_tail"] = 0
                elif e["lat_min_tail"] == 0 or it.lat < e["lat_min_tail"]:
                    e["lat_min_tail"] = it.lat
    return sorted(evs.values(), key=lambda e: e["last"])


def events_array(evs):
    a = np.zeros(len(evs), abi.PING_EV_DTYPE)
    for k, e in enumerate(evs):
        a[k]["ns_id"], a[k]["client_id"], a[k]["family"], a[k]["ident"] = e["key"]
        for f in EV_FIELDS:
            a[k][f] = e[f]
    return a


def events_from_array(a):
    return [dict({f: int(e[f]) for f in EV_FIELDS},
                 key=(int(e["ns_id"]), int(e["client_id"]), int(e["family"]), int(e["ident"]))) for e in a]


def replay(evs, st: State):
    """INTEGRATION.md's loop over a batch's events."""
    for e in evs:
        ns, cid, fam, ident = e["key"]
        c = st.cnt(ns, fam)
        if cid == abi.PING_NS_LEVEL:
            c["pktRxNoClientUnhandled"] += e["n_no_client"]
            c["pktRxErrMulticastB"] += e["n_mcast"]
            continue
        pg = st.pings.get((cid, fam))
        if pg is None:
            c["pktRxErrUnhandled"] += e["n_reply"] + e["n_unreach"]
            continue
        c["pktRxIcmpResponse"] += e["n_reply"]
        c["pktRxIcmpDstUnreachable"] += e["n_unreach"]
        if ident != pg.identifier:
            pg.repliesBadIdentifier += e["n_reply"] + e["n_unreach"]
            continue
        pg.dstUnreachable += e["n_unreach"]
        pg.repliesMalformedPkt += e["n_malformed"]
        pg.repliesBadLatency += e["n_bad_latency"]
        if e["n_ok"] == 0:
            continue
        if not pg.firstReplyReceived:
            first_ok = e["seq_first"] == pg.startingSeq
        else:
            first_ok = (pg.lastSeqReceived + 1) & 0xFFFF == e["seq_first"]
        in_order = int(first_ok) + e["n_succ"]
        pg.repliesInOrder += in_order
        pg.repliesOutOfOrder += e["n_ok"] - in_order
        pg.firstReplyReceived = True
        pg.lastSeqReceived = e["seq_last"]
        pg.latencySum += e["lat_sum"]
        pg.maxLatency = max(pg.maxLatency, e["lat_max"])
        if e["flags"] & 1 or pg.minLatency == 0:
            pg.minLatency = e["lat_min_tail"]
        else:
            pg.minLatency = min(pg.minLatency, e["lat_min_tail"])


def ping_batch(buf, desc, rec, env, fams=abi.PNGK_ALL, now=SIM_NOW, ev_cap=None, items=None):
    """emurx_ping_dev's outputs for a batch: outcome u8 [n], the events (abi.PING_EV_DTYPE) and info."""
    items = batch_items(buf, desc, rec, env, fams, now) if items is None else items
    return batch_of_items(items, ev_cap)


def batch_of_items(items, ev_cap=None):
    outcome = np.array([it.outcome for it in items], np.uint8)
    ev = events_array(fold(items))
    over = ev_cap is not None and len(ev) > ev_cap
    info = np.zeros(abi.PNG_INFO_WORDS, np.uint64)
    info[0], info[1], info[2] = 0 if over else len(ev), len(ev), int(over)
    for k in range(1, 6):
        info[2 + k] = int((outcome == k).sum())
    return outcome, ev[:0] if over else ev, info


# ---- frames ------------------------------------------------------------------------------
def eth(dst: bytes, src: bytes, tags=((0x8100, 1), (0x8100, 2)), etype=0x0800) -> bytes:
    t = b"".join(tp.to_bytes(2, "big") + vid.to_bytes(2, "big") for tp, vid in tags)
    return bytes(dst) + bytes(src) + t + etype.to_bytes(2, "big")


def echo_body(ident, seq, ts, magic=abi.PING_MAGIC, extra=0) -> bytes:
    return (ident.to_bytes(2, "big") + seq.to_bytes(2, "big") + magic.to_bytes(8, "big") +
            (ts & (2 ** 64 - 1)).to_bytes(8, "big") + bytes(extra))


def _with_csum(b: bytes, at: int, init: int = 0) -> bytes:
    """b with the Internet checksum of b (its field at `at` zero) stored at b[at:at+2]."""
    return b[:at] + F.csum_fold(b, init).to_bytes(2, "big") + b[at + 2:]


def v4(dst_mac, src_ip, dst_ip, icmp: bytes, tags=((0x8100, 1), (0x8100, 2)), ihl=5) -> bytes:
    """An ICMPv4 frame with valid checksums (the parser verifies both); ihl > 5 pads options."""
    ip = bytes([0x40 | ihl, 0]) + (4 * ihl + len(icmp)).to_bytes(2, "big") + bytes([0, 0xCC, 0, 0, 64, 1, 0, 0]) + \
        bytes(src_ip) + bytes(dst_ip) + bytes(4 * (ihl - 5))
    icmp = _with_csum(icmp, 2) if len(icmp) >= 4 else icmp
    return eth(dst_mac, bytes([0, 0, 0, 2, 0, 0]), tags, 0x0800) + _with_csum(ip, 10) + icmp


def v4_reply(dst_mac, src_ip, dst_ip, ident, seq, ts, **kw) -> bytes:
    body = echo_body(ident, seq, ts, kw.pop("magic", abi.PING_MAGIC), kw.pop("extra", 4))
    body = body[:kw.pop("cut", len(body))]
    return v4(dst_mac, src_ip, dst_ip, bytes([0, 0, 0, 0]) + body, **kw)


def v4_unreach(dst_mac, src_ip, dst_ip, ident, code=1, cut=None, **kw) -> bytes:
    inner = bytes([0x45, 0]) + (48).to_bytes(2, "big") + bytes([0, 0, 0, 0, 64, 1, 0, 0]) + bytes(dst_ip) + bytes(src_ip) + \
        bytes([8, 0, 0, 0]) + ident.to_bytes(2, "big") + bytes(2)
    icmp = bytes([3, code, 0, 0, 0, 0, 0, 0]) + inner
    return v4(dst_mac, src_ip, dst_ip, icmp[:cut], **kw)


def v6(dst_mac, src_ip, dst_ip, icmp: bytes, tags=((0x8100, 1), (0x8100, 2))) -> bytes:
    ip = bytes([0x60, 0, 0, 0]) + len(icmp).to_bytes(2, "big") + bytes([58, 64]) + bytes(src_ip) + bytes(dst_ip)
    icmp = _with_csum(icmp, 2, F.ipv6_pseudo(bytes(src_ip), bytes(dst_ip), len(icmp), 58)) if len(icmp) >= 4 else icmp
    return eth(dst_mac, bytes([0, 0, 0, 2, 0, 0]), tags, 0x86DD) + ip + icmp


def v6_reply(dst_mac, src_ip, dst_ip, ident, seq, ts, **kw) -> bytes:
    body = echo_body(ident, seq, ts, kw.pop("magic", abi.PING_MAGIC), 0)
    body = body[:kw.pop("cut", len(body))]
    return v6(dst_mac, src_ip, dst_ip, bytes([129, kw.pop("code", 0), 0, 0]) + body, **kw)


def v6_unreach(dst_mac, src_ip, dst_ip, ident, code=0, cut=None, **kw) -> bytes:
    inner = bytes([0x60, 0, 0, 0, 0, 24, 58, 64]) + bytes(dst_ip) + bytes(src_ip) + bytes([128, 0, 0, 0]) + \
        echo_body(ident, 0, 0)
    icmp = bytes([1, code, 0, 0, 0, 0, 0, 0]) + inner
    return v6(dst_mac, src_ip, dst_ip, icmp[:cut], **kw)

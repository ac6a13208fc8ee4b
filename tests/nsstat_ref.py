"""Python restatement of the per-frame rule of emurx_nsstat_dev and of its fold into one event per
Namespace: which of the ARP, ICMPv4, ICMPv6 and ND handlers' counters a frame bumps, and whether
its Go handler still has to run.

    nsstat_ref(frame, rec, kinds, rsp, lrn, hole=False, max_ns=None) -> (done, [counter indices])

frame: the rx frame; rec: its record (emurx.abi.REC_DTYPE); kinds: abi.RSPK_* bits; rsp: the
frame's outcome of respond_ref / nd_ref (emurx_respond_kinds_dev), lrn: its outcome of learn_ref
(emurx_learn_dev).  The rule, with the reference's lines (paths relative to src/emu/plugins; the type
and code constants are gopacket's, src/external/google/gopacket/layers/icmp4.go:20-43 and
icmp6.go:21-52):

  candidate: status OK, the descriptor no hole, callback arp / icmp / icmpv6 selected by kinds
      (icmpv6 by ICMPV6 or ND); everything else done 0
  lookup NO_NS / NS_NO_PLUGIN: done 2, the handler only returns PARSER_ERR
      (arp/arp.go:958-965, icmp/icmp.go:486-493, ipv6/ipv6.go:546-553); lookup NONE: done 0
  header offsets that do not fit the frame (no record of a classify has them): done 0
  a Namespace id at or above max_ns: done 0
  arp     PluginArpNs.HandleRxArpPacket arp/arp.go:904-946; learn outcome HOST -> done 0
      operation 1 (:915): pktRxArpQuery :916; CLookupByIPv4 nil (NO_CLIENT): pktRxArpQueryNotForUs
          :932; a client without the arp plugin (CLIENT_NO_PLUGIN): nothing more :926-927; CLIENT:
          Respond counts pktTxReply :778, so done 1 only if the device wrote the reply (RSP_ARP),
          else done 0 with no counter at all
      operation 2 (:935): broadcast destination: pktRxErrNoBroadcast :937; else pktRxArpReply :940
      any other (:943): pktRxErrWrongOp :944
  icmp    PluginIcmpNs.HandleRxIcmpPacket icmp/icmp.go:396-462
      NO_CLIENT (CLookupByIPv4 nil :418 or !IsUnicastToMe :424): pktRxNoClientUnhandled :419, :425
      CLIENT: responder DROP_MCAST (the source test :433 or HandleEcho's swapped destination :295):
          pktRxErrMulticastB :434, :296; RSP_ICMP: HandleEcho's pktRxIcmpQuery, pktTxIcmpResponse
          :322-323; else the switch :438-459: (8,0) ICMPv4TypeEchoRequest, (13,0)
          ICMPv4TypeTimestampRequest, (0,0) ICMPv4TypeEchoReply, (3, 0..4)
          ICMPv4TypeDestinationUnreachable with ICMPv4CodeNet, Host, Protocol, Port,
          FragmentationNeeded stay with the handler (done 0); default: pktRxErrUnhandled :458
  icmpv6  PluginIpv6Ns.HandleRxIpv6Packet ipv6/ipv6.go:465-539
      (128,0) ICMPv6TypeEchoRequest :480: NO_CLIENT (:487, :493; the classifier also folds the
          multicast source test :499 into it, so a source that starts 0xff is done 0):
          pktRxNoClientUnhandled :488, :494; CLIENT: RSP_ICMPV6: HandleEcho's pktRxIcmpQuery,
          pktTxIcmpResponse :354-355; DROP_MCAST: pktRxErrMulticastB :322; else done 0
      (135,0) ICMPv6TypeNeighborSolicitation -> nd.go: answered (RSP_ND) and learn NONE or ND_NS:
          pktRxNeighborSolicitation nd.go:1547, and Respond's pktTxNeighborDADError :1240 for an
          unspecified source, pktTxNeighborAdvUnicast :1246 otherwise; else done 0
      (136,0) ICMPv6TypeNeighborAdvertisement: learn ND_NA: pktRxNeighborAdvertisement nd.go:1688 and
          pktRxNeighborAdvLearn :1758, :1768; else done 0
      (130,0), (131,0), (132,0), (143,0) MLD :505-509; (133,0), (134,0), (137,0) router
          solicitation, advertisement, redirect :511-516; (129,0) ICMPv6TypeEchoReply :517;
          (1, 0..6) ICMPv6TypeDestinationUnreachable with ICMPv6CodeNoRouteToDst ..
          ICMPv6CodeRejectRouteToDst :522-528: done 0
      default: pktRxErrUnhandled :535

No text of the reference is restated here."""
import numpy as np

import learn_ref as L
import nd_ref as N
import respond_ref as R
from emurx import abi, frames as F

CB_ARP, CB_ICMP, CB_ICMPV6 = 0, 1, 9
BCAST = b"\xff" * 6
LK = abi.LK
# the counter every done-1 frame bumps exactly one of
FIRST = (abi.NSC_ARP_QUERY, abi.NSC_ARP_REPLY, abi.NSC_ARP_ERR_NO_BROADCAST, abi.NSC_ARP_ERR_WRONG_OP, abi.NSC_ICMP_ECHO,
         abi.NSC_ICMP_NO_CLIENT, abi.NSC_ICMP_ERR_MCAST, abi.NSC_ICMP_ERR_UNHANDLED, abi.NSC_V6_ECHO, abi.NSC_V6_NO_CLIENT,
         abi.NSC_V6_ERR_MCAST, abi.NSC_V6_ERR_UNHANDLED, abi.NSC_ND_RX_NS, abi.NSC_ND_RX_NA)


def _decide(p: bytes, rec, kinds: int, rsp: int, lrn: int, hole: bool):
    """-> (done, counters, branch, candidate)"""
    proto, lk = int(rec["proto"]), (int(rec["flags"]) >> 4) & 7
    l3, l4, n = int(rec["l3"]), int(rec["l4"]), len(p)
    sel = {CB_ARP: abi.RSPK_ARP, CB_ICMP: abi.RSPK_ICMP, CB_ICMPV6: abi.RSPK_ICMPV6 | abi.RSPK_ND}.get(proto, 0)
    if int(rec["status"]) != 0 or not kinds & sel or hole:
        return 0, [], "not-candidate", False
    if lk in (LK["NO_NS"], LK["NS_NO_PLUGIN"]):
        return 2, [], "parser-err", True
    if lk < LK["NS_LEVEL"]:
        return 0, [], "no-lookup", True
    if proto == CB_ARP:
        if l3 < 14 or l3 + 28 > n:
            return 0, [], "arp-bounds", True
        if lrn == abi.LRN_HOST:
            return 0, [], "arp-learn-host", True
        op = (p[l3 + 6] << 8) | p[l3 + 7]
        if op == 1:
            if lk == LK["NO_CLIENT"]:
                return 1, [abi.NSC_ARP_QUERY, abi.NSC_ARP_QUERY_NOT_FOR_US], "arp-not-for-us", True
            if lk == LK["CLIENT_NO_PLUGIN"]:
                return 1, [abi.NSC_ARP_QUERY], "arp-client-no-plugin", True
            if lk == LK["CLIENT"] and rsp == abi.RSP_ARP:
                return 1, [abi.NSC_ARP_QUERY, abi.NSC_ARP_TX_REPLY], "arp-answered", True
            return 0, [], "arp-request-host", True
        if op == 2:
            if p[0:6] == BCAST:
                return 1, [abi.NSC_ARP_ERR_NO_BROADCAST], "arp-reply-broadcast", True
            return 1, [abi.NSC_ARP_REPLY], "arp-reply", True
        return 1, [abi.NSC_ARP_ERR_WRONG_OP], "arp-wrong-op", True
    if proto == CB_ICMP:
        if l3 < 14 or l3 + 20 > n or l4 + 8 > n:
            return 0, [], "icmp-bounds", True
        if lk == LK["NO_CLIENT"]:
            return 1, [abi.NSC_ICMP_NO_CLIENT], "icmp-no-client", True
        if lk != LK["CLIENT"]:
            return 0, [], "icmp-other-lookup", True
        if rsp == abi.RSP_DROP_MCAST:
            return 1, [abi.NSC_ICMP_ERR_MCAST], "icmp-mcast", True
        if rsp == abi.RSP_ICMP:
            return 1, [abi.NSC_ICMP_ECHO], "icmp-echo", True
        t, c = p[l4], p[l4 + 1]
        if (t, c) == (8, 0):
            return 0, [], "icmp-echo-host", True
        if (t, c) in ((13, 0), (0, 0)) or (t == 3 and c <= 4):
            return 0, [], "icmp-handler-type", True
        return 1, [abi.NSC_ICMP_ERR_UNHANDLED], "icmp-unhandled", True
    if l3 < 14 or l3 + 40 > l4 or l4 + 4 > n:
        return 0, [], "v6-bounds", True
    t, c = p[l4], p[l4 + 1]
    if (t, c) == (128, 0):
        if not kinds & abi.RSPK_ICMPV6:
            return 0, [], "v6-echo-not-selected", True
        if lk == LK["NO_CLIENT"]:
            if p[l3 + 8] == 0xFF:
                return 0, [], "v6-echo-mcast-source", True
            return 1, [abi.NSC_V6_NO_CLIENT], "v6-no-client", True
        if lk != LK["CLIENT"]:
            return 0, [], "v6-echo-other-lookup", True
        if rsp == abi.RSP_ICMPV6:
            return 1, [abi.NSC_V6_ECHO], "v6-echo", True
        if rsp == abi.RSP_DROP_MCAST:
            return 1, [abi.NSC_V6_ERR_MCAST], "v6-mcast", True
        return 0, [], "v6-echo-host", True
    if lk != LK["NS_LEVEL"]:
        return 0, [], "v6-other-lookup", True
    if (t, c) in ((135, 0), (136, 0)):
        if not kinds & abi.RSPK_ND:
            return 0, [], "nd-not-selected", True
        if t == 136:
            if lrn == abi.LRN_ND_NA:
                return 1, [abi.NSC_ND_RX_NA, abi.NSC_ND_RX_NA_LEARN], "na-learned", True
            return 0, [], "na-host", True
        if rsp != abi.RSP_ND or lrn not in (abi.LRN_NONE, abi.LRN_ND_NS):
            return 0, [], "ns-host", True
        if N.is_unspecified(p[l3 + 8:l3 + 24]):
            return 1, [abi.NSC_ND_RX_NS, abi.NSC_ND_TX_DAD_ERROR], "ns-answered-dad", True
        return 1, [abi.NSC_ND_RX_NS, abi.NSC_ND_TX_ADV_UNICAST], "ns-answered-unicast", True
    if (c == 0 and (129 <= t <= 134 or t in (137, 143))) or (t == 1 and c <= 6):
        return 0, [], "v6-handler-type", True
    if not kinds & abi.RSPK_ICMPV6:
        return 0, [], "v6-unhandled-not-selected", True
    return 1, [abi.NSC_V6_ERR_UNHANDLED], "v6-unhandled", True


def _decide_ns(p, rec, kinds, rsp, lrn, hole, max_ns):
    done, cnt, why, cand = _decide(bytes(p), rec, kinds, int(rsp), int(lrn), hole)
    if done == 1 and max_ns is not None and int(rec["ns_id"]) >= max_ns:
        return 0, [], "ns-out-of-range", True
    return done, cnt, why, cand


def nsstat_ref(frame, rec, kinds: int, rsp: int, lrn: int = 0, hole: bool = False, max_ns=None):
    return _decide_ns(frame, rec, kinds, rsp, lrn, hole, max_ns)[:2]


def nsstat_branch(frame, rec, kinds: int, rsp: int, lrn: int = 0, hole: bool = False, max_ns=None) -> str:
    return _decide_ns(frame, rec, kinds, rsp, lrn, hole, max_ns)[2]


def nsstat_frames(buf, desc, rec, kinds: int, rsp, lrn=None, max_ns=None):
    """Per frame -> done u8 [n], the counters each frame bumps (a list of lists), candidate bool [n]"""
    n = len(desc)
    done, cnts, cand = np.zeros(n, np.uint8), [], np.zeros(n, bool)
    for i in range(n):
        d = desc[i]
        f = bytes(buf[int(d["off"]):int(d["off"]) + int(d["len"])])
        o, c, _, k = _decide_ns(f, rec[i], kinds, rsp[i], 0 if lrn is None else lrn[i], int(d["pad"]) == abi.DESC_HOLE, max_ns)
        done[i], cand[i] = o, k
        cnts.append(c)
    return done, cnts, cand


def fold(ns_ids, done, cnts, cand, ev_cap=None):
    """The per-frame decisions of a batch (or of a prefix of one) -> the events written
    (abi.NSSTAT_EV_DTYPE, ascending ns_id) and info u64 [8]; ev_cap None = room for everything."""
    acc = {}
    for i in np.nonzero(done == 1)[0]:
        row = acc.setdefault(int(ns_ids[i]), np.zeros(1 + abi.NSC_WORDS, np.uint64))
        row[0] += 1
        for c in cnts[i]:
            row[1 + c] += 1
    ev = np.zeros(len(acc), abi.NSSTAT_EV_DTYPE)
    for j, ns in enumerate(sorted(acc)):
        ev[j] = (ns, acc[ns][0], acc[ns][1:])
    over = ev_cap is not None and len(ev) > ev_cap
    info = np.zeros(abi.NSS_INFO_WORDS, np.uint64)
    info[0], info[1], info[2] = 0 if over else len(ev), len(ev), int(over)
    info[3], info[4], info[5] = int((done == 1).sum()), int((done == 2).sum()), int((cand & (done == 0)).sum())
    return ev[:0] if over else ev, info


def nsstat_batch(buf, desc, rec, kinds: int, rsp, lrn=None, ev_cap=None, max_ns=None):
    """emurx_nsstat_dev's outputs for a batch: done u8 [n], the events written, info u64 [8]."""
    done, cnts, cand = nsstat_frames(buf, desc, rec, kinds, rsp, lrn, max_ns)
    ev, info = fold(rec["ns_id"], done, cnts, cand, ev_cap)
    return done, ev, info


def replay(events, stats=None):
    """INTEGRATION.md's replay loop: stats[(ns, plugin stats, Go counter)] += cnt; words 6 and 10 add
    to two Go counters each."""
    stats = {} if stats is None else stats
    for e in events:
        for idx, (plug, names) in enumerate(abi.NSC_GO):
            v = int(e["cnt"][idx])
            for name in names if v else ():
                k = (int(e["ns_id"]), plug, name)
                stats[k] = stats.get(k, 0) + v
    return stats


# ---- the mixed batch --------------------------------------------------------------------------------
# respond_ref.mixed_batch (even slots) and learn_ref.learning_batch (odd slots) interleaved, with
# every 128th slot replaced by an entry of EXTRA: the frames whose handler is one counter and
# nothing else, which neither of the two batches has a reason to hold.
def _extra():
    def echo4(typ=8, dmac=None):
        def make(ns, c):
            mac, ip4, _ = R._client(ns, c)
            ip = F.ipv4(bytes([48, 0, 0, 9]), ip4, 1, F.icmp4(typ, 0, 7, c, bytes(20)))
            f = R._eth(dmac if dmac is not None else mac, R.DUT_MAC, R._NS[ns], 0x0800, ip, c)
            return f + bytes(max(60 - len(f), 0))
        return make

    def echo6(esrc=R.DUT_MAC, known=True):
        def make(ns, c):
            mac, _, ip6 = R._client(ns, c)
            dst = ip6 if known else ip6[:15] + b"\x77"
            src, body = bytes([0x20, 1, 0x0D, 0xB8] + [0] * 10 + [1, 9]), bytes(12)
            ic = F.icmp6(128, 0, body, pseudo=F.ipv6_pseudo(src, dst, 4 + len(body), 58))
            return R._eth(mac, esrc, R._NS[ns], 0x86DD, F.ipv6(src, dst, 58, ic), c)
        return make

    return [echo4(dmac=bytes([0, 0, 9, 9, 9, 9])),  # the client's IP behind another MAC: !IsUnicastToMe
            echo4(typ=11),                           # time exceeded: no case of the handler's switch
            echo6(known=False),                      # no client has the address
            echo6(esrc=bytes([0x33, 0x33, 0, 0, 0, 9]))]  # a group source: HandleEcho drops it


EXTRA = _extra()
EXTRA_EVERY, EXTRA_AT = 128, 126


def mixed_batch(n: int, seed: int = 7):
    """-> (frames, vports)"""
    a, va = R.mixed_batch((n + 1) // 2, seed)
    b, vb = L.learning_batch(n // 2)
    frames = [(a if i % 2 == 0 else b)[i // 2] for i in range(n)]
    vports = [(va if i % 2 == 0 else vb)[i // 2] for i in range(n)]
    for j, i in enumerate(range(EXTRA_AT, n, EXTRA_EVERY)):
        frames[i], vports[i] = EXTRA[j % len(EXTRA)](j % len(R._NS), (j // len(EXTRA)) % R.N_CLIENTS), 1
    return frames, vports

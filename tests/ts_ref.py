"""Python restatement of the ICMPv4 timestamp reply emurx_respond_ts_dev builds on the device, of
the two outcomes it adds to emurx_nsstat_ts_dev's rule, and the frames that exercise them.  It
wraps respond_ref, nd_ref and nsstat_ref, which stay as they are.

    ts_ref(frame, rec, kinds, ip_time, env4, env6=None, hole=False) -> (outcome, reply bytes or None)

The rules, with the reference's lines (paths relative to src/emu/plugins; gopacket under
src/external/google/gopacket):

  an icmp frame is considered if status OK, lookup CLIENT, callback icmp, no hole and kinds has ICMP
  or TS (the client lookup and IsUnicastToMe, icmp/icmp.go:417-427, are the classifier's)
  offsets that do not fit (l3 < 14, l3 + 20 > len, l4 + 8 > len): HOST
  the source-IP rule icmp.go:429-436: DROP_MCAST, for every type
  (8, 0): respond_ref's echo rule if kinds has ICMP, else NONE
  (13, 0) -> HandleEcho(ps, true) :289-325; without TS in kinds: HOST
      the swapped Ethernet destination (the request's source p[6:12]) broadcast or multicast
          :293-299: DROP_MCAST (pktRxErrMulticastB)
      len(icmp) = len - l4 < 20 :312-316, behind the multicast test: DROP_SHORT (pktRxErrTooShort)
      an odd l4 (no parse produces one): HOST
      else the whole frame with the Ethernet addresses swapped :293-294, the IPv4 addresses swapped
          :301-302, type and code 14, 0 :310-311, ipt = iptime() :281-287 (milliseconds since
          midnight UTC; here the caller's ip_time) big-endian in icmp[12:16] and icmp[16:20]
          :317-319, and icmp.UpdateChecksum() :320 (layers/icmp4.go:252-256: the checksum field
          zeroed, then tcpipChecksum(icmp, 0), layers/tcpip.go:76-94, over p[l4:len], the rest of
          the frame): pktRxIcmpQuery, pktTxIcmpResponse :322-323
  any other type: NONE
  nsstat, with TS and ICMP in kinds, an icmp frame with lookup CLIENT: responder outcome TS:
      NSC_ICMP_ECHO, done 1; DROP_SHORT: NSC_ICMP_ERR_TOO_SHORT, done 1; everything else is
      nsstat_ref's rule (DROP_MCAST counts pktRxErrMulticastB; a timestamp request left at HOST,
      NOSPC or NONE stays at done 0)

No text of the reference is restated here."""
import struct

import numpy as np

import nd_ref as N
import nsstat_ref as NS
import respond_ref as R
from emurx import abi, frames as F

CB_ICMP = R.CB_ICMP
FIRST = NS.FIRST + (abi.NSC_ICMP_ERR_TOO_SHORT,)


def tcpip_checksum(data: bytes, csum: int = 0) -> int:
    """tcpipChecksum (layers/tcpip.go:76-94): big-endian byte pairs, an odd last byte << 8, folded
    while above 0xffff, complemented."""
    length = len(data) - 1
    for i in range(0, length, 2):
        csum += data[i] << 8
        csum += data[i + 1]
    if len(data) % 2 == 1:
        csum += data[length] << 8
    while csum > 0xFFFF:
        csum = (csum >> 16) + (csum & 0xFFFF)
    return ~csum & 0xFFFF


def span_sum(data: bytes) -> int:
    """The folded sum of a span with its checksum in place: 0xffff if and only if it verifies."""
    return ~tcpip_checksum(data) & 0xFFFF


def ts_ref(frame: bytes, rec, kinds: int, ip_time: int, env4=None, env6=None, hole: bool = False):
    p = bytearray(frame)
    lk = (int(rec["flags"]) >> 4) & 7
    proto, l3, l4, n = int(rec["proto"]), int(rec["l3"]), int(rec["l4"]), len(p)
    if not (int(rec["status"]) == 0 and lk == abi.LK["CLIENT"] and proto == CB_ICMP and not hole):
        # every other kind: nd_ref.respond_batch's rule for one frame
        o, r = abi.RSP_NONE, None
        if kinds & 7 and env4 is not None:
            o, r = R.respond_ref(frame, rec, env4, hole=hole)
            sel = {R.CB_ARP: abi.RSPK_ARP, R.CB_ICMP: abi.RSPK_ICMP, R.CB_ICMPV6: abi.RSPK_ICMPV6}.get(proto, 0)
            if not kinds & sel:
                o, r = abi.RSP_NONE, None
        if o == abi.RSP_NONE and kinds & abi.RSPK_ND and env6 is not None:
            o, r = N.nd_ref(frame, rec, env6, hole=hole)
        return o, r
    if not kinds & (abi.RSPK_ICMP | abi.RSPK_TS):
        return abi.RSP_NONE, None
    if l3 < 14 or l3 + 20 > n or l4 + 8 > n:
        return abi.RSP_HOST, None
    if not R.ip4_src_ok(bytes(p[l3 + 12:l3 + 16])):
        return abi.RSP_DROP_MCAST, None
    tc = (p[l4] << 8) | p[l4 + 1]
    if tc == 0x0800:
        return R.respond_ref(frame, rec, env4, hole=hole) if kinds & abi.RSPK_ICMP else (abi.RSP_NONE, None)
    if tc != 0x0D00:
        return abi.RSP_NONE, None
    if not kinds & abi.RSPK_TS:
        return abi.RSP_HOST, None
    if p[6] & 1:
        return abi.RSP_DROP_MCAST, None
    if n - l4 < 20:
        return abi.RSP_DROP_SHORT, None
    if l4 & 1:
        return abi.RSP_HOST, None
    p[0:6], p[6:12] = p[6:12], p[0:6]
    p[l3 + 12:l3 + 16], p[l3 + 16:l3 + 20] = p[l3 + 16:l3 + 20], p[l3 + 12:l3 + 16]
    p[l4], p[l4 + 1] = 14, 0
    p[l4 + 12:l4 + 20] = struct.pack(">II", ip_time & 0xFFFFFFFF, ip_time & 0xFFFFFFFF)
    p[l4 + 2:l4 + 4] = b"\0\0"
    p[l4 + 2:l4 + 4] = struct.pack(">H", tcpip_checksum(bytes(p[l4:])))
    return abi.RSP_TS, bytes(p)


def respond_batch(buf, desc, rec, kinds: int, ip_time: int, env4=None, env6=None, out_cap=None):
    """emurx_respond_ts_dev's outputs for a batch -> outcome u8 [n], out_desc, out_src, the replies,
    info u64 [16] = {replies, bytes needed, frames with outcome 1..9, zeros}."""
    n = len(desc)
    outcome = np.zeros(n, np.uint8)
    replies, src, od = [], [], []
    off = 0
    for i in range(n):
        d = desc[i]
        f = bytes(buf[int(d["off"]):int(d["off"]) + int(d["len"])])
        o, r = ts_ref(f, rec[i], kinds, ip_time, env4, env6, hole=int(d["pad"]) == abi.DESC_HOLE)
        if r is not None:
            end = off + R.align16(len(r))
            if out_cap is not None and end > out_cap:
                o = abi.RSP_NOSPC
            else:
                replies.append(r)
                src.append(i)
                od.append((off, len(r), int(rec[i]["vport"]) & 0xFF, 0))
            off = end
        outcome[i] = o
    info = np.zeros(abi.RSP_INFO_WORDS, np.uint64)
    info[0], info[1] = len(replies), off
    for k in range(1, 10):
        info[1 + k] = int((outcome == k).sum())
    return outcome, np.array(od, abi.DESC_DTYPE), np.array(src, np.uint32), replies, info


# ---- nsstat ------------------------------------------------------------------------------------
def nsstat_decide(p: bytes, rec, kinds: int, rsp: int, lrn: int = 0, hole: bool = False, max_ns=None):
    """-> (done, counters, candidate): nsstat_ref's rule, refined for the two timestamp outcomes"""
    assert not kinds & abi.RSPK_TS or kinds & abi.RSPK_ICMP  # the entry point refuses TS without ICMP
    lk = (int(rec["flags"]) >> 4) & 7
    l3, l4, n = int(rec["l3"]), int(rec["l4"]), len(p)
    if (kinds & abi.RSPK_TS and int(rec["status"]) == 0 and not hole and int(rec["proto"]) == CB_ICMP and lk == abi.LK["CLIENT"]
            and not (l3 < 14 or l3 + 20 > n or l4 + 8 > n) and int(rsp) in (abi.RSP_TS, abi.RSP_DROP_SHORT)):
        if max_ns is not None and int(rec["ns_id"]) >= max_ns:
            return 0, [], True
        return 1, [abi.NSC_ICMP_ECHO if int(rsp) == abi.RSP_TS else abi.NSC_ICMP_ERR_TOO_SHORT], True
    done, cnt, _, cand = NS._decide_ns(bytes(p), rec, kinds & abi.RSPK_ALL, rsp, lrn, hole, max_ns)
    return done, cnt, cand


def nsstat_frames(buf, desc, rec, kinds: int, rsp, lrn=None, max_ns=None):
    n = len(desc)
    done, cnts, cand = np.zeros(n, np.uint8), [], np.zeros(n, bool)
    for i in range(n):
        d = desc[i]
        f = bytes(buf[int(d["off"]):int(d["off"]) + int(d["len"])])
        o, c, k = nsstat_decide(f, rec[i], kinds, rsp[i], 0 if lrn is None else lrn[i], int(d["pad"]) == abi.DESC_HOLE, max_ns)
        done[i], cand[i] = o, k
        cnts.append(c)
    return done, cnts, cand


def nsstat_batch(buf, desc, rec, kinds: int, rsp, lrn=None, ev_cap=None, max_ns=None):
    """emurx_nsstat_ts_dev's outputs for a batch: done u8 [n], the events written, info u64 [8]."""
    done, cnts, cand = nsstat_frames(buf, desc, rec, kinds, rsp, lrn, max_ns)
    ev, info = NS.fold(rec["ns_id"], done, cnts, cand, ev_cap)
    return done, ev, info


def replay(events, stats=None):
    """nsstat_ref.replay with the word emurx_nsstat_ts_dev adds (abi.NSC_GO_TS): stats[(ns, plugin
    stats, Go counter)] += cnt."""
    stats = {} if stats is None else stats
    for e in events:
        for idx, (plug, names) in enumerate(abi.NSC_GO_TS):
            v = int(e["cnt"][idx])
            for name in names if v else ():
                k = (int(e["ns_id"]), plug, name)
                stats[k] = stats.get(k, 0) + v
    return stats


# ---- frames ------------------------------------------------------------------------------------
SIX_SEQ = range(0xABCD, 0xABD3)


def six_requests():
    """The six timestamp requests of the reference's TestPluginIcmp2 (icmp/icmp_test.go:221-250),
    for the "icmp" environment of sim_envs: 62 bytes each."""
    out = []
    for seq in SIX_SEQ:
        ic = F.icmp4(13, 0, 1, seq, bytes(12))
        ip = F.ipv4(bytes([16, 0, 0, 2]), bytes([16, 0, 0, 0]), 1, ic, ttl=128, ident=0xCC)
        out.append(bytes([0, 0, 1, 0, 0, 0]) + bytes([0, 0, 0, 2, 0, 0]) + struct.pack(">HHHHH", 0x8100, 1, 0x8100, 2, 0x0800) + ip)
    assert all(len(f) == 62 for f in out)
    return out


def ts_frame(ns: int, c: int, *, opts: int = 0, span: int = 20, icmp_len=None, typ: int = 13, orig: bytes = bytes(4),
             fill: int = 0, esrc: bytes = R.DUT_MAC, src: bytes = bytes([48, 0, 0, 7]), pcp: int = 0, ident: int = 1, seq: int = 2):
    """A timestamp request to client c of respond_ref's Namespace ns (0, 1 or 2 tags for ns 0, 1, 2):
    IHL 5 + opts words, len - l4 = span; the ICMP message is icmp_len bytes (default min(span, 20):
    the IPv4 total length ends there) = header, originate timestamp `orig`, then `fill`; the bytes
    behind it up to span are a trailer of 0xa5, 0xa6, ...  l4 = 14 + 4 * tags + 20 + 4 * opts."""
    mac, ip4, _ = R._client(ns, c)
    icmp_len = min(span, 20) if icmp_len is None else icmp_len
    body = (orig + bytes([fill]) * max(icmp_len - 12, 0))[: icmp_len - 8]
    ic = F.icmp4(typ, 0, ident, seq, body)
    ip = F.ipv4(src, ip4, 1, ic, options=bytes([1] * (4 * opts - 1) + [0]) if opts else b"")
    f = R._eth(mac, esrc, R._NS[ns], 0x0800, ip, pcp)
    return f + bytes((0xA5 + j) & 0xFF for j in range(span - icmp_len))


def l4_of(ns: int, opts: int) -> int:
    return 14 + 4 * len(R._NS[ns]) + 20 + 4 * opts


def ffff_frame(ns: int, c: int, ip_time: int, **kw):
    """A request whose reply's span sums to 0xffff with the checksum field zero, so that the reply
    stores 0x0000: the originate timestamp is chosen for it."""
    f0 = ts_frame(ns, c, orig=bytes(4), **kw)
    span = bytearray(f0[l4_of(ns, kw.get("opts", 0)):])
    span[0], span[2:4], span[12:20] = 14, b"\0\0", struct.pack(">II", ip_time, ip_time)
    s = span_sum(bytes(span))
    assert 0 < s <= 0xFFFF
    return ts_frame(ns, c, orig=struct.pack(">HH", 0, 0xFFFF - s), **kw)

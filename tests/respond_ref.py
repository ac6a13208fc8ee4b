"""Python restatement of the three stateless answers emurx_respond_dev builds on the device, and
a seeded mixed batch that exercises every branch of them.

    respond_ref(frame, rec, env) -> (outcome, reply bytes or None)

frame: the rx frame; rec: its record (emurx.abi.REC_DTYPE, from the oracle or emurx_classify_dev);
env: Env, the IPv4 client map of the handle that answers.  The rules, with the reference's lines
(paths relative to src/emu/plugins):

  considered only if status OK, lookup CLIENT, callback arp / icmp / icmpv6 (the record carries the
  decision "request, client found, plugin present, unicast to me": arp/arp.go:914-930,
  icmp/icmp.go:413-427, ipv6/ipv6.go:465-504)
  arp     PluginArpClient.Respond arp/arp.go:776-790 on the template of arp.go:621-636 (Ethernet
          from ns_ctx.go:634-653: dst, client MAC, the Namespace key's tags, EtherType)
  icmp    HandleRxIcmpPacket icmp/icmp.go:429-461 -> HandleEcho :289-325; the source-IP rule is Go
          1.18 net.IP.IsLoopback / IsGlobalUnicast (the standard library, not the reference tree)
  icmpv6  HandleEcho ipv6/ipv6.go:315-357
  UpdateInetChecksum: external/google/gopacket/layers/icmp4.go:238-250
"""
import struct

import numpy as np

from emurx import abi, frames as F

CB_ARP, CB_ICMP, CB_ICMPV6 = 0, 1, 9


class Env:
    """CLookupByIPv4 of the answering handle: (vport, vlan0, vlan1, ipv4 bytes) -> (client id, MAC)."""

    def __init__(self):
        self.ip4 = {}

    def add(self, key: bytes, cid: int, mac: bytes, ipv4):
        if ipv4 is not None and bytes(ipv4) != bytes(4):
            vport, _, v0, v1 = struct.unpack("<HHII", key)
            self.ip4[(vport, v0, v1, bytes(ipv4))] = (cid, bytes(mac))

    def remove(self, key: bytes, ipv4):
        vport, _, v0, v1 = struct.unpack("<HHII", key)
        self.ip4.pop((vport, v0, v1, bytes(ipv4)), None)


def update_inet_checksum(cs: int, old: int, new: int) -> int:
    s = (~cs & 0xFFFF) + (~old & 0xFFFF) + new
    while s > 0xFFFF:
        s = (s >> 16) + (s & 0xFFFF)
    return ~s & 0xFFFF


def ip4_src_ok(ip: bytes) -> bool:
    """net.IP.IsLoopback() || IsGlobalUnicast() of Go 1.18 for an IPv4 address."""
    if ip == bytes(4) or ip == b"\xff" * 4:
        return False
    if ip[0] & 0xF0 == 0xE0 or (ip[0] == 169 and ip[1] == 254):
        return False
    return True


def respond_ref(frame: bytes, rec, env: Env, hole: bool = False):
    p = bytearray(frame)
    lk = (int(rec["flags"]) >> 4) & 7
    proto, l3, l4 = int(rec["proto"]), int(rec["l3"]), int(rec["l4"])
    if hole or int(rec["status"]) != 0 or lk != abi.LK["CLIENT"] or proto not in (CB_ARP, CB_ICMP, CB_ICMPV6):
        return abi.RSP_NONE, None
    if l3 < 14 or l3 > len(p):  # offsets that do not fit the frame: no record of a classify has them
        return abi.RSP_HOST, None
    if proto == CB_ARP:
        if l3 + 28 > len(p):
            return abi.RSP_HOST, None
        sha, spa, tpa = bytes(p[l3 + 8:l3 + 14]), bytes(p[l3 + 14:l3 + 18]), bytes(p[l3 + 24:l3 + 28])
        hit = env.ip4.get((int(rec["vport"]), int(rec["vlan0"]), int(rec["vlan1"]), tpa))
        if hit is None or hit[0] != int(rec["client_id"]):
            return abi.RSP_HOST, None
        mac = hit[1]
        tags = b"".join(struct.pack(">I", int(v)) for v in (rec["vlan0"], rec["vlan1"]) if int(v))
        return abi.RSP_ARP, (sha + mac + tags + b"\x08\x06" + bytes([0, 1, 8, 0, 6, 4, 0, 2]) + mac + tpa + sha + spa)
    group_src = bool(p[6] & 1)  # eth.SwapSrcDst(); eth.IsBroadcast() || eth.IsMcast()
    if proto == CB_ICMP:
        if l3 + 20 > len(p) or l4 + 8 > len(p):
            return abi.RSP_HOST, None
        if not ip4_src_ok(bytes(p[l3 + 12:l3 + 16])):
            return abi.RSP_DROP_MCAST, None
        tc = (p[l4] << 8) | p[l4 + 1]
        if tc == 0x0D00:
            return abi.RSP_HOST, None
        if tc != 0x0800:
            return abi.RSP_NONE, None
        if group_src:
            return abi.RSP_DROP_MCAST, None
        p[0:6], p[6:12] = p[6:12], p[0:6]
        p[l3 + 12:l3 + 16], p[l3 + 16:l3 + 20] = p[l3 + 16:l3 + 20], p[l3 + 12:l3 + 16]
        cs = (p[l4 + 2] << 8) | p[l4 + 3]
        p[l4], p[l4 + 1] = 0, 0
        p[l4 + 2:l4 + 4] = struct.pack(">H", update_inet_checksum(cs, 0x0800, 0x0000))
        return abi.RSP_ICMP, bytes(p)
    if l3 + 40 > l4 or l4 + 8 > len(p):
        return abi.RSP_HOST, None
    if group_src:
        return abi.RSP_DROP_MCAST, None
    strip = l4 - l3 - 40
    if (p[l3 + 6] != 58) != (strip != 0):  # ipv6.go:340-344, or a next header that disagrees with l4
        return abi.RSP_HOST, None
    p[0:6], p[6:12] = p[6:12], p[0:6]
    p[l3 + 8:l3 + 24], p[l3 + 24:l3 + 40] = p[l3 + 24:l3 + 40], p[l3 + 8:l3 + 24]
    p[l4] = 129
    if strip:
        p[l3 + 6] = 58
        plen = ((p[l3 + 4] << 8) | p[l3 + 5]) - strip
        p[l3 + 4:l3 + 6] = struct.pack(">H", plen & 0xFFFF)
        del p[l3 + 40:l4]
        l4 = l3 + 40
    cs = (p[l4 + 2] << 8) | p[l4 + 3]
    p[l4 + 2:l4 + 4] = struct.pack(">H", update_inet_checksum(cs, 0x8000, 0x8100))
    return abi.RSP_ICMPV6, bytes(p)


def align16(x: int) -> int:
    return (x + 15) & ~15


def respond_batch(buf, desc, rec, env: Env, out_cap=None):
    """emurx_respond_dev's outputs for a batch: outcome u8 [n], out_desc, out_src, the replies
    (list of bytes, in order) and info u64 [8]; out_cap None = room for everything."""
    n = len(desc)
    outcome = np.zeros(n, np.uint8)
    replies, src, od = [], [], []
    off = 0
    for i in range(n):
        d = desc[i]
        f = bytes(buf[int(d["off"]):int(d["off"]) + int(d["len"])])
        o, r = respond_ref(f, rec[i], env, hole=int(d["pad"]) == abi.DESC_HOLE)
        if r is not None:
            end = off + align16(len(r))
            if out_cap is not None and end > out_cap:
                o = abi.RSP_NOSPC
            else:
                replies.append(r)
                src.append(i)
                od.append((off, len(r), int(rec[i]["vport"]) & 0xFF, 0))
            off = end
        outcome[i] = o
    info = np.zeros(8, np.uint64)
    info[0], info[1] = len(replies), off
    for k in range(1, 7):
        info[1 + k] = int((outcome == k).sum())
    return outcome, np.array(od, abi.DESC_DTYPE), np.array(src, np.uint32), replies, info


# ---- the mixed batch ---------------------------------------------------------------------
# Namespaces (vport 1): untagged, dot1q, QinQ with an 0x8100 and with an 0x88a8 outer tag, and
# one that is never added (unknown).  Every frame's tags carry PCP != 0 where it has tags.
_NS = [(), ((0x8100, 7),), ((0x8100, 5), (0x8100, 6)), ((0x88A8, 9), (0x8100, 10))]
_UNKNOWN_NS = ((0x8100, 99),)
DUT_MAC = bytes([0x00, 0x10, 0x94, 0, 0, 0x02])


def _key(tags):
    v = [(t << 16) | vid for t, vid in tags] + [0, 0]
    return F.tunnel_key(1, v[0], v[1])


def _client(ns: int, c: int):
    """Client c of Namespace ns: MAC, IPv4, static IPv6; odd clients answer on an EUI-64
    link-local address (fe80::/64 needs no RA prefix, client_ctx.go:279-295)."""
    mac = bytes([0, 0, 1, ns, 0, c])
    return mac, bytes([16, ns, 0, c + 1]), bytes([0x20, 1, 0x0D, 0xB8, 0, ns] + [0] * 9 + [c + 1])


def _eui(mac: bytes) -> bytes:
    return bytes([0xFE, 0x80] + [0] * 6 + [mac[0] ^ 2, mac[1], mac[2], 0xFF, 0xFE, mac[3], mac[4], mac[5]])


N_CLIENTS = 4


def load_tables(target, env: Env | None = None):
    """The batch's Namespaces and clients into an Oracle / RxPath (and the Env twin)."""
    cid = 0
    for ns, tags in enumerate(_NS):
        assert target.ns_add(_key(tags), ns, abi.PLUG_ALL) == 0
        for c in range(N_CLIENTS):
            mac, ip4, ip6 = _client(ns, c)
            assert target.client_add(ns, cid, mac, ip4, ip6, None, abi.PLUG_ALL) == 0
            if env is not None:
                env.add(_key(tags), cid, mac, ip4)
            cid += 1


def _eth(dst, src, tags, etype, payload, pcp):
    tg = b""
    for k, (tpid, vid) in enumerate(tags):
        tg += struct.pack(">HH", tpid, (((pcp + k) % 7 + 1) << 13) | vid)
    return F.mac(dst) + F.mac(src) + tg + struct.pack(">H", etype) + payload


def mixed_batch(n: int, seed: int = 7):
    """n frames cycling through the kinds below (frame i is kind i % len(kinds), so every prefix
    longer than the list holds every kind), each with a seeded Namespace / client / payload.
    -> (frames, vports)"""
    rng = np.random.default_rng([seed, 0x727370])
    frames = []

    def echo4(size, ihl=5, typ=8, code=0, src=None, esrc=DUT_MAC, bad=False):
        def make(ns, c, tags, pcp):
            mac, ip4, _ = _client(ns, c)
            room = size - 14 - 4 * len(tags) - 4 * ihl - 8
            body = rng.integers(0, 256, max(room, 0), dtype=np.uint8).tobytes()
            ic = F.icmp4(typ, code, int(rng.integers(0, 65536)), int(rng.integers(0, 65536)), body)
            if bad:
                ic = ic[:2] + struct.pack(">H", (struct.unpack(">H", ic[2:4])[0] + 1) & 0xFFFF) + ic[4:]
            s = src if src is not None else bytes([48, 0, int(rng.integers(0, 256)), int(rng.integers(1, 255))])
            ip = F.ipv4(s, ip4, 1, ic, options=bytes([1, 1, 1, 0]) if ihl == 6 else b"")
            f = _eth(mac, esrc, tags, 0x0800, ip, pcp)
            return f + bytes(max(60 - len(f), 0))  # Ethernet padding: trailing bytes the reply keeps
        return make

    def echo6(ext=0, eui=False, size=0):
        def make(ns, c, tags, pcp):
            mac, _, ip6 = _client(ns, c)
            dst = _eui(mac) if eui else ip6
            src = bytes([0x20, 1, 0x0D, 0xB8] + [0] * 10 + [1, int(rng.integers(1, 255))])
            body = struct.pack(">HH", int(rng.integers(0, 65536)), int(rng.integers(0, 65536))) + \
                rng.integers(0, 256, int(rng.integers(4, 64)) if not size else size, dtype=np.uint8).tobytes()
            ic = F.icmp6(128, 0, body, pseudo=F.ipv6_pseudo(src, dst, 4 + len(body), 58))
            # extension headers: hop-by-hop (PadN) and / or destination options, 8 bytes each or 16
            hdrs, nh = b"", 58
            chain = {0: [], 8: [(0, 6)], 16: [(0, 14)], 24: [(0, 6), (60, 14)]}[ext]
            for k in range(len(chain) - 1, -1, -1):
                kind, blen = chain[k]
                hdrs = F.ipv6_ext(nh, bytes([1, blen - 2]) + bytes(blen - 2)) + hdrs
                nh = kind
            assert len(hdrs) == ext
            return _eth(mac, DUT_MAC, tags, 0x86DD, F.ipv6(src, dst, nh, hdrs + ic), pcp)
        return make

    def arp(op=1, known=True):
        def make(ns, c, tags, pcp):
            mac, ip4, _ = _client(ns, c)
            tpa = ip4 if known else bytes([16, ns, 9, c + 1])
            spa = bytes([48, 0, 0, int(rng.integers(1, 255))])
            sha = bytes([0x00, 0x10, 0x94, int(rng.integers(0, 256)), 0, 3])  # not the Ethernet source
            a = F.arp(op, sha, spa, bytes(6) if op == 1 else mac, tpa)
            dst = b"\xff" * 6 if op == 1 else mac
            f = _eth(dst, DUT_MAC, tags, 0x0806, a, pcp)
            return f + bytes(max(60 - len(f), 0))
        return make

    def l4(proto):
        def make(ns, c, tags, pcp):
            mac, ip4, _ = _client(ns, c)
            src = bytes([48, 0, 0, 7])
            body = rng.integers(0, 256, 26, dtype=np.uint8).tobytes()
            ps = F.ipv4_pseudo(src, ip4, proto, (8 if proto == 17 else 20) + len(body))
            seg = F.udp(1025, 4000, body, csum="auto", pseudo=ps) if proto == 17 else F.tcp(1025, 80, body, pseudo=ps)
            return _eth(mac, DUT_MAC, tags, 0x0800, F.ipv4(src, ip4, proto, seg), pcp)
        return make

    kinds = [
        echo4(60), arp(), echo6(), echo4(594), l4(17), echo6(8), arp(known=False), echo4(1518, ihl=6),
        echo6(16, eui=True), arp(op=2), echo4(64, typ=13), echo6(24), l4(6), echo4(9216), echo4(60, src=bytes(4)),
        echo6(0, eui=True), echo4(98, src=bytes([224, 0, 0, 5])), arp(), echo4(77, src=bytes([169, 254, 3, 4])),
        echo4(60, src=bytes([127, 0, 0, 1])), echo4(60, esrc=bytes([1, 0, 0x5E, 0, 0, 1])),
        echo4(61, esrc=b"\xff" * 6), echo4(90, bad=True), echo4(60, ihl=6), echo4(60, typ=0), echo6(8, size=1400),
        echo6(0, eui=True, size=3), "unknown_ns", echo4(1518), echo4(594, ihl=6),
    ]
    jumbo = 0
    for i in range(n):
        k = kinds[i % len(kinds)]
        ns = int(rng.integers(0, len(_NS)))
        c = int(rng.integers(0, N_CLIENTS))
        pcp = int(rng.integers(0, 7))
        if k == "unknown_ns":
            frames.append(echo4(60)(0, c, _UNKNOWN_NS, pcp))
            continue
        if i % len(kinds) == 13:  # the 9216 B echo: a few per batch are enough
            jumbo += 1
            if jumbo > 3:
                k = echo4(125)
        frames.append(k(ns, c, _NS[ns], pcp))
    return frames, [1] * n


def pack_with_holes(frames, vports, every: int = 37):
    """pack_frames, with every `every`-th descriptor turned into a hole (its frame stays in the
    buffer, unreferenced)."""
    buf, desc = F.pack_frames(frames, vports)
    if every:
        desc["pad"][every - 1::every] = abi.DESC_HOLE
    return buf, desc

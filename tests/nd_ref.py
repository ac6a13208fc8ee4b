"""Python restatement of the fourth stateless answer of the device responder, the neighbour
advertisement (NA) that answers a neighbour solicitation (NS), and a seeded batch that reaches
every branch of it.

    nd_ref(frame, rec, env) -> (outcome, reply bytes or None)

frame: the rx frame; rec: its record (emurx.abi.REC_DTYPE, from the oracle or emurx_classify_dev);
env: Env, the MAC map, the IPv6 map and the clients of the handle that answers.  The rule, with the
reference's lines (paths relative to src/emu unless they start with external/):

  considered only if status OK, callback icmpv6, lookup NS_LEVEL, no hole, p[l4] == 135 and
  p[l4 + 1] == 0 (plugins/ipv6/nd.go:1546; the parser has checked the ICMPv6 checksum)
  header offsets that do not fit the frame (no record of a classify has them) -> HOST, before the
  type byte is read
  len(nd) < 20 -> NONE                                                    nd.go:1550-1553
  options = p[l4 + 24:], the rest of the frame (not the IPv6 payload length):
      external/google/gopacket/layers/icmp6msg.go:299-312, 497-529
      empty: no source link-layer address (SLLA); 1..7 bytes: a decode error -> NONE; 8 bytes:
      {type 1, length 1} is the SLLA, anything else (another type, length 0, a truncated option)
      ends in an error -> NONE                                           nd.go:1555-1587
      more than 8 bytes -> HOST (the device does not walk an option chain)
  hop limit != 255 -> NONE                                                nd.go:1561-1564
  SLLA all zero; source unspecified with an SLLA; source unspecified and destination not
  multicast; target unspecified or multicast -> NONE                      nd.go:1589-1609
  NdLearn nd.go:1611-1620 stays on the host and does not change the answer
  target neither link-local unicast nor global unicast -> NONE            nd.go:1622-1624, 1680-1683
  EUI-64 target (core/client_ctx.go:314-329): CLookupByMac of the extracted MAC (a zero MAC never
      matches), IsValidPrefix core/client_ctx.go:279-295 (fe80::/64, or the client's RA prefix of
      length 64), the client's ipv6 plugin; else NONE                     nd.go:1626-1652
  other target: global -> CLookupByIPv6, the client's ipv6 plugin; else NONE   nd.go:1653-1678
  the reply: NdClientCtx.Respond nd.go:1220-1253 on the template of nd.go:835-865; checksum
      FixIcmpL4Checksum external/google/gopacket/layers/ip6.go:54-56

net.IP.IsUnspecified / IsMulticast / IsLinkLocalUnicast / IsGlobalUnicast are Go 1.18's, on a
16-byte slice, with their IPv4-mapped readings (::ffff:0.0.0.0 is unspecified, ::ffff:224.x is
multicast, ::ffff:169.254.x is link-local).  They are Go's standard library (net/ip.go), not the
reference tree, and no capture pins them: like the ICMPv4 source rule of respond_ref.
"""
import struct

import numpy as np

import respond_ref as R
from emurx import abi, frames as F

CB_ICMPV6 = 9
PLUG_IPV6 = 1 << 8
ALL_NODES = bytes([0xFF, 2] + [0] * 13 + [1])
V4MAPPED = bytes(10) + b"\xff\xff"


# ---- Go 1.18 net.IP predicates on a 16-byte address -----------------------------------------
def _to4(ip: bytes):
    return ip[12:16] if ip[:12] == V4MAPPED else None


def is_unspecified(ip: bytes) -> bool:
    return ip == bytes(16) or ip == V4MAPPED + bytes(4)


def is_multicast(ip: bytes) -> bool:
    v4 = _to4(ip)
    return (v4[0] & 0xF0) == 0xE0 if v4 is not None else ip[0] == 0xFF


def is_link_local_unicast(ip: bytes) -> bool:
    v4 = _to4(ip)
    return (v4[0] == 169 and v4[1] == 254) if v4 is not None else (ip[0] == 0xFE and ip[1] & 0xC0 == 0x80)


def is_loopback(ip: bytes) -> bool:
    v4 = _to4(ip)
    return v4[0] == 127 if v4 is not None else ip == bytes(15) + b"\x01"


def is_global_unicast(ip: bytes) -> bool:
    return not (ip == V4MAPPED + b"\xff" * 4 or is_unspecified(ip) or is_loopback(ip) or is_multicast(ip) or
                is_link_local_unicast(ip))


def eui_of(mac: bytes, prefix: bytes = bytes([0xFE, 0x80] + [0] * 6)) -> bytes:
    return prefix[:8] + bytes([mac[0] ^ 2, mac[1], mac[2], 0xFF, 0xFE, mac[3], mac[4], mac[5]])


class Env:
    """CLookupByMac / CLookupByIPv6 of the answering handle, keyed by the tunnel key, and per
    client its MAC, plugin mask and RA prefix (prefix bytes, length) or None."""

    def __init__(self):
        self.mac, self.ip6, self.clients = {}, {}, {}

    @staticmethod
    def _k(key: bytes):
        vport, _, v0, v1 = struct.unpack("<HHII", key)
        return vport, v0, v1

    def add(self, key: bytes, cid: int, mac: bytes, ipv6=None, dhcpv6=None, plugins=abi.PLUG_ALL, ra=None):
        k = self._k(key)
        self.mac[k + (bytes(mac),)] = cid
        ips = [bytes(a) for a in (ipv6, dhcpv6) if a is not None and bytes(a) != bytes(16)]
        for a in ips:
            self.ip6[k + (a,)] = cid
        self.clients[cid] = dict(key=k, mac=bytes(mac), plugins=plugins, ra=ra, ips=ips)

    def remove(self, cid: int):
        c = self.clients.pop(cid)
        self.mac.pop(c["key"] + (c["mac"],), None)
        for a in c["ips"]:
            self.ip6.pop(c["key"] + (a,), None)


def _decide(frame: bytes, rec, env: Env, hole: bool):
    """-> (outcome, reply or None, the branch that decided)"""
    p = bytes(frame)
    n = len(p)
    lk = (int(rec["flags"]) >> 4) & 7
    l3, l4 = int(rec["l3"]), int(rec["l4"])
    if hole or int(rec["status"]) != 0 or int(rec["proto"]) != CB_ICMPV6 or lk != abi.LK["NS_LEVEL"]:
        return abi.RSP_NONE, None, "not-candidate"
    if l3 < 14 or l3 + 40 > l4 or l4 + 4 > n:
        return abi.RSP_HOST, None, "bounds"
    if p[l4] != 135 or p[l4 + 1] != 0:
        return abi.RSP_NONE, None, "not-ns"
    if n - (l4 + 4) < 20:
        return abi.RSP_NONE, None, "too-short"
    opts, slla = p[l4 + 24:], None
    if len(opts) > 8:
        return abi.RSP_HOST, None, "options-long"
    if 0 < len(opts) < 8:
        return abi.RSP_NONE, None, "options-1-7"
    if len(opts) == 8:
        if opts[0] != 1 or opts[1] != 1:
            return abi.RSP_NONE, None, "options-8-wrong"
        slla = opts[2:8]
    if p[l3 + 7] != 255:
        return abi.RSP_NONE, None, "hop-limit"
    src, dst, tgt = p[l3 + 8:l3 + 24], p[l3 + 24:l3 + 40], p[l4 + 8:l4 + 24]
    if slla == bytes(6):
        return abi.RSP_NONE, None, "slla-zero"
    dad = is_unspecified(src)
    if dad and slla is not None:
        return abi.RSP_NONE, None, "dad-with-slla"
    if dad and not is_multicast(dst):
        return abi.RSP_NONE, None, "dad-unicast-dst"
    if is_unspecified(tgt) or is_multicast(tgt):
        return abi.RSP_NONE, None, "target-unspec-mcast"
    glob = is_global_unicast(tgt)
    if not (is_link_local_unicast(tgt) or glob):
        return abi.RSP_NONE, None, "target-not-local-global"
    key = (int(rec["vport"]), int(rec["vlan0"]), int(rec["vlan1"]))
    if tgt[11] == 0xFF and tgt[12] == 0xFE:
        mac = bytes([tgt[8] ^ 2, tgt[9], tgt[10], tgt[13], tgt[14], tgt[15]])
        cid = env.mac.get(key + (mac,)) if mac != bytes(6) else None
        if cid is None:
            return abi.RSP_NONE, None, "eui-mac-miss"
        c = env.clients[cid]
        ra = c["ra"]
        if not (tgt[:8] == bytes([0xFE, 0x80] + [0] * 6) or (ra is not None and ra[1] == 64 and ra[0][:8] == tgt[:8])):
            return abi.RSP_NONE, None, "eui-prefix"
        if not c["plugins"] & PLUG_IPV6:
            return abi.RSP_NONE, None, "eui-no-plugin"
        why = "eui-local" if tgt[:2] == b"\xfe\x80" else "eui-ra"
    else:
        if not glob:
            return abi.RSP_NONE, None, "plain-not-global"
        cid = env.ip6.get(key + (tgt,))
        if cid is None:
            return abi.RSP_NONE, None, "ip6-miss"
        c = env.clients[cid]
        if not c["plugins"] & PLUG_IPV6:
            return abi.RSP_NONE, None, "ip6-no-plugin"
        mac, why = c["mac"], "ip6"
    tags = b"".join(struct.pack(">I", int(v)) for v in (rec["vlan0"], rec["vlan1"]) if int(v))
    if dad:
        edst, ipsrc, ipdst, fl = bytes([0x33, 0x33, 0, 0, 0, 1]), eui_of(mac), ALL_NODES, 0
    else:
        edst, ipsrc, ipdst, fl = p[6:12], tgt, src, 0x60
    icmp = bytes([0x88, 0, 0, 0, fl, 0, 0, 0]) + tgt + b"\x02\x01" + mac
    cs = F.csum_fold(icmp, F.ipv6_pseudo(ipsrc, ipdst, 32, 58))
    icmp = icmp[:2] + struct.pack(">H", cs) + icmp[4:]
    reply = edst + mac + tags + b"\x86\xdd" + bytes([0x60, 0, 0, 0, 0, 0x20, 0x3A, 0xFF]) + ipsrc + ipdst + icmp
    return abi.RSP_ND, reply, why + ("-dad" if dad else "-unicast")


def nd_ref(frame: bytes, rec, env: Env, hole: bool = False):
    o, r, _ = _decide(frame, rec, env, hole)
    return o, r


def nd_branch(frame: bytes, rec, env: Env, hole: bool = False) -> str:
    return _decide(frame, rec, env, hole)[2]


def respond_batch(buf, desc, rec, kinds: int, env4=None, env6: Env | None = None, out_cap=None, info_words=None):
    """emurx_respond_kinds_dev's outputs for a batch: respond_ref for the kinds 1-3 that `kinds`
    selects, nd_ref for ND.  -> outcome u8 [n], out_desc, out_src, the replies, info u64 [16]
    (u64 [8], emurx_respond_dev's, when info_words == 8)."""
    n = len(desc)
    outcome = np.zeros(n, np.uint8)
    replies, src, od = [], [], []
    off = 0
    for i in range(n):
        d = desc[i]
        f = bytes(buf[int(d["off"]):int(d["off"]) + int(d["len"])])
        hole = int(d["pad"]) == abi.DESC_HOLE
        o, r = abi.RSP_NONE, None
        if kinds & 7 and env4 is not None:
            o, r = R.respond_ref(f, rec[i], env4, hole=hole)
            sel = {R.CB_ARP: abi.RSPK_ARP, R.CB_ICMP: abi.RSPK_ICMP, R.CB_ICMPV6: abi.RSPK_ICMPV6}.get(int(rec[i]["proto"]), 0)
            if not kinds & sel:
                o, r = abi.RSP_NONE, None
        if o == abi.RSP_NONE and kinds & abi.RSPK_ND and env6 is not None:
            o, r = nd_ref(f, rec[i], env6, hole=hole)
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
    words = info_words or abi.RSP_INFO_WORDS
    info = np.zeros(words, np.uint64)
    info[0], info[1] = len(replies), off
    for k in range(1, 8 if words > 8 else 7):
        info[1 + k] = int((outcome == k).sum())
    return outcome, np.array(od, abi.DESC_DTYPE), np.array(src, np.uint32), replies, info


# ---- the ND batch ------------------------------------------------------------------------------
# Namespaces on vport 2 (respond_ref's are on vport 1): untagged, dot1q, QinQ; ids behind
# respond_ref's.  Client c of a Namespace:
#   0  static global IPv6, a DHCPv6 address that is IPv4-mapped (::ffff:10.ns.0.9), no RA prefix
#   1  RA prefix 2001:db8:aa:ns::/64, a DHCPv6 address
#   2  like 1, without the ipv6 plugin
#   3  an RA prefix of length 48: IsValidPrefix takes only 64
_NS = [(), ((0x8100, 21),), ((0x88A8, 22), (0x8100, 23))]
NS_BASE, CID_BASE, N_CLIENTS, VPORT = 8, 32, 4, 2
PEER_MAC = bytes([0x00, 0x10, 0x94, 0, 0, 0x09])


def _key(tags):
    v = [(t << 16) | vid for t, vid in tags] + [0, 0]
    return F.tunnel_key(VPORT, v[0], v[1])


def _client(ns: int, c: int):
    """-> mac, static IPv6, DHCPv6 address, plugins, RA (prefix, length) or None"""
    mac = bytes([0, 0, 2, ns, 0, c])
    ip6 = bytes([0x20, 1, 0x0D, 0xB8, 0, ns] + [0] * 9 + [c + 1])
    d6 = V4MAPPED + bytes([10, ns, 0, 9]) if c == 0 else bytes([0x20, 1, 0x0D, 0xB8, 0xD, ns] + [0] * 9 + [c + 1])
    plugins = abi.PLUG_ALL & ~PLUG_IPV6 if c == 2 else abi.PLUG_ALL
    prefix = bytes([0x20, 1, 0x0D, 0xB8, 0, 0xAA, c, ns] + [0] * 8)
    ra = None if c == 0 else (prefix, 48 if c == 3 else 64)
    return mac, ip6, d6, plugins, ra


def load_tables(target, env: Env | None = None):
    """The ND batch's Namespaces and clients into an Oracle / RxPath (and the Env twin)."""
    for ns, tags in enumerate(_NS):
        assert target.ns_add(_key(tags), NS_BASE + ns, abi.PLUG_ALL) == 0
        for c in range(N_CLIENTS):
            mac, ip6, d6, plugins, ra = _client(ns, c)
            cid = CID_BASE + ns * N_CLIENTS + c
            assert target.client_add(NS_BASE + ns, cid, mac, None, ip6, d6, plugins) == 0
            if ra is not None:
                assert target.client_set_ra(cid, ra[0], ra[1]) == 0
            if env is not None:
                env.add(_key(tags), cid, mac, ip6, d6, plugins, ra)


def _solicited(tgt: bytes):
    return bytes([0xFF, 2] + [0] * 9 + [1, 0xFF]) + tgt[13:], bytes([0x33, 0x33, 0xFF]) + tgt[13:]


def slla(mac: bytes) -> bytes:
    return b"\x01\x01" + mac


def ns_frame(tags, pcp, tgt, *, src=None, dst=None, edst=None, esrc=PEER_MAC, opts=None, hop=255, ext=0, trail=b"",
             typ=135, code=0, body=None):
    """A neighbour solicitation (or, with typ / body, another ICMPv6 message) with a valid checksum.
    src None: the unspecified address (duplicate address detection)."""
    dad = src is None
    src = bytes(16) if dad else src
    mdst, medst = _solicited(tgt)
    dst, edst = dst if dst is not None else mdst, edst if edst is not None else medst
    if opts is None:
        opts = b"" if dad else slla(esrc)
    if body is None:
        body = bytes(4) + tgt + opts
    ic = F.icmp6(typ, code, body, pseudo=F.ipv6_pseudo(src, dst, 4 + len(body), 58))
    hdrs, nh = b"", 58
    chain = {0: [], 8: [(0, 6)], 24: [(0, 6), (60, 14)]}[ext]
    for k in range(len(chain) - 1, -1, -1):
        kind, blen = chain[k]
        hdrs = F.ipv6_ext(nh, bytes([1, blen - 2]) + bytes(blen - 2)) + hdrs
        nh = kind
    assert len(hdrs) == ext
    return R._eth(edst, esrc, tags, 0x86DD, F.ipv6(src, dst, nh, hdrs + ic, hop=hop), pcp) + trail


# (label, the outcome the rule gives it, builder(ns, tags, pcp, rng)); frame i of nd_batch is entry
# i % len(KINDS), so every prefix longer than the list holds every entry
def _kinds():
    peer = bytes([0x20, 1, 0x0D, 0xB8, 0, 0xEE] + [0] * 9 + [7])
    peer_ll = eui_of(PEER_MAC)
    ND, NONE, HOST = abi.RSP_ND, abi.RSP_NONE, abi.RSP_HOST

    def tgt(kind, c):
        def f(ns):
            mac, ip6, d6, _, ra = _client(ns, c)
            return {"ll": eui_of(mac), "ra": eui_of(mac, ra[0]) if ra else None, "ip6": ip6, "d6": d6}[kind]
        return f

    def fixed(a):
        return lambda ns: a

    def mk(label, want, target, **kw):
        def make(ns, tags, pcp, rng):
            k = dict(kw)
            if k.get("src") == "peer":
                k["src"] = peer[:15] + bytes([int(rng.integers(1, 255))])
            t = target(ns)
            if k.pop("unicast", False):  # a unicast probe to the target (neighbour unreachability detection)
                k["dst"], k["edst"] = t, bytes([0, 0, 2, ns, 0, 0])
            if callable(k.get("opts")):
                k["opts"] = k["opts"](rng)
            if callable(k.get("trail")):
                k["trail"] = k["trail"](rng)
            return ns_frame(tags, pcp, t, **k)
        return label, want, make

    rnd = lambda n: (lambda rng: rng.integers(0, 256, n, dtype=np.uint8).tobytes())  # noqa: E731
    nonce = bytes([14, 1, 1, 2, 3, 4, 5, 6])
    unknown_eui = eui_of(bytes([0, 0, 2, 0x77, 0, 1]))
    zero_mac_eui = bytes([0xFE, 0x80] + [0] * 6 + [2, 0, 0, 0xFF, 0xFE, 0, 0, 0])
    return [
        mk("ll-eui unicast", ND, tgt("ll", 0), src="peer"),
        mk("ll-eui dad", ND, tgt("ll", 1)),
        mk("ra-eui unicast", ND, tgt("ra", 1), src="peer"),
        mk("ip6 unicast", ND, tgt("ip6", 0), src="peer"),
        mk("hop-limit", NONE, tgt("ll", 0), src="peer", hop=64),
        mk("slla-zero", NONE, tgt("ll", 0), src="peer", opts=slla(bytes(6))),
        mk("dad-with-slla", NONE, tgt("ll", 0), opts=slla(PEER_MAC)),
        mk("ip6 dad dhcpv6", ND, tgt("d6", 1)),
        mk("dad-unicast-dst", NONE, tgt("ll", 0), unicast=True),
        mk("target-unspecified", NONE, fixed(bytes(16)), src="peer"),
        mk("target-multicast", NONE, fixed(ALL_NODES), src="peer"),
        mk("ext8", ND, tgt("ll", 3), src="peer", ext=8),
        mk("target-loopback", NONE, fixed(bytes(15) + b"\x01"), src="peer"),
        mk("eui-mac-unknown", NONE, fixed(unknown_eui), src="peer"),
        mk("eui-mac-zero", NONE, fixed(zero_mac_eui), src="peer"),
        mk("no-slla unicast", ND, tgt("ip6", 1), src="peer", opts=b""),
        mk("eui-prefix-none", NONE, lambda ns: eui_of(_client(ns, 0)[0], peer), src="peer"),
        mk("eui-prefix-len48", NONE, tgt("ra", 3), src="peer"),
        mk("eui-no-plugin", NONE, tgt("ll", 2), src="peer"),
        mk("ext24 dad", ND, tgt("ra", 1), ext=24),
        mk("ip6-no-plugin", NONE, tgt("ip6", 2), src="peer"),
        mk("plain-link-local", NONE, fixed(bytes([0xFE, 0x80] + [0] * 12 + [0x12, 0x34])), src="peer"),
        mk("ip6-unknown", NONE, fixed(peer), src="peer"),
        mk("probe unicast", ND, tgt("ll", 1), src=peer_ll, unicast=True),
        mk("options-3", NONE, tgt("ll", 0), opts=b"\x01\x01\x00"),
        mk("options-7", NONE, tgt("ll", 0), src="peer", opts=slla(PEER_MAC)[:7]),
        mk("options-8-type", NONE, tgt("ll", 0), src="peer", opts=nonce),
        mk("options-8-len0", NONE, tgt("ll", 0), src="peer", opts=b"\x01\x00" + PEER_MAC),
        mk("v4mapped-src dad", ND, tgt("ll", 0), src=V4MAPPED + bytes(4), opts=b""),
        mk("options-8-truncated", NONE, tgt("ll", 0), src="peer", opts=b"\x01\x02" + PEER_MAC),
        mk("options-16", HOST, tgt("ll", 0), src="peer", opts=slla(PEER_MAC) + nonce),
        mk("v4mapped-target ip6", ND, tgt("d6", 0), src="peer"),
        mk("v4mapped-target-multicast", NONE, fixed(V4MAPPED + bytes([224, 0, 0, 1])), src="peer"),
        mk("v4mapped-target-link-local", NONE, fixed(V4MAPPED + bytes([169, 254, 1, 2])), src="peer"),
        mk("v4mapped-target-unknown", NONE, fixed(V4MAPPED + bytes([10, 99, 0, 1])), src="peer"),
        mk("ip6 dad", ND, tgt("ip6", 3)),
        mk("v4mapped-dst-multicast dad", ND, tgt("ll", 3), dst=V4MAPPED + bytes([224, 0, 0, 1])),
        mk("trail-becomes-slla", ND, tgt("ll", 1), src="peer", opts=b"", trail=slla(PEER_MAC)),
        mk("trail-2", NONE, tgt("ll", 1), src="peer", opts=b"", trail=rnd(2)),
        mk("trail-after-slla", HOST, tgt("ll", 1), src="peer", trail=rnd(4)),
        mk("ra-eui dad", ND, tgt("ra", 1)),
        mk("rs", NONE, tgt("ll", 0), src="peer", typ=133, body=bytes(4) + slla(PEER_MAC)),
        mk("ra", NONE, tgt("ll", 0), src=peer_ll, dst=ALL_NODES, typ=134, body=bytes([64, 0, 7, 8]) + bytes(8)),
        mk("na", NONE, tgt("ll", 0), src="peer", typ=136, body=bytes([0x60, 0, 0, 0]) + peer + b"\x02\x01" + PEER_MAC),
        mk("code-1", NONE, tgt("ll", 0), src="peer", code=1),
        mk("too-short", NONE, tgt("ll", 0), src="peer", body=bytes(4) + bytes(12)),
        mk("ll-eui unicast 2", ND, tgt("ll", 3), src=peer_ll),
    ]


KINDS = _kinds()
# respond_ref.pack_with_holes(every=HOLE_EVERY) puts holes over answered and unanswered entries alike
HOLE_EVERY = 29


def nd_batch(n: int, seed: int = 11):
    """n frames cycling through KINDS, each in a seeded Namespace (0, 1 or 2 tags).
    -> (frames, vports, labels)"""
    rng = np.random.default_rng([seed, 0x6E64])
    frames, labels = [], []
    for i in range(n):
        label, _, make = KINDS[i % len(KINDS)]
        ns = int(rng.integers(0, len(_NS)))
        frames.append(make(ns, _NS[ns], int(rng.integers(0, 7)), rng))
        labels.append(label)
    return frames, [VPORT] * n, labels


def combined_batch(n: int, seed: int = 5):
    """respond_ref.mixed_batch frames and nd_batch frames interleaved (even slots the former, odd
    slots the latter).  -> (frames, vports)"""
    a, va = R.mixed_batch((n + 1) // 2, seed)
    b, vb, _ = nd_batch(n // 2, seed)
    frames, vports = [], []
    for i in range(n):
        src, vs = (a, va) if i % 2 == 0 else (b, vb)
        frames.append(src[i // 2])
        vports.append(vs[i // 2])
    return frames, vports


def load_combined(target, env4=None, env6=None):
    """The union of the two batches' tables: respond_ref's Namespaces 0-3 / clients 0-15 on vport 1,
    the ND batch's Namespaces 8-10 / clients 32-43 on vport 2."""
    R.load_tables(target, env4)
    load_tables(target, env6)


def answered_batch(n: int, seed: int = 3):
    """n solicitations that are all answered (the entries of KINDS built for a reply, in turn)."""
    rng = np.random.default_rng([seed, 0x6E65])
    makers = [make for _, want, make in KINDS if want == abi.RSP_ND]
    frames = []
    for i in range(n):
        ns = int(rng.integers(0, len(_NS)))
        frames.append(makers[i % len(makers)](ns, _NS[ns], int(rng.integers(0, 7)), rng))
    return frames, [VPORT] * n

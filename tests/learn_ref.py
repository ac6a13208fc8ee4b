"""Python restatement of the ARP / ND cache learning that emurx_learn_dev folds on the device, a
model of the two resolution tables the events are replayed into, and seeded batches that reach
every branch of the rule.

    learn_ref(frame, rec, env6, kinds) -> (outcome, key or None)

frame: the rx frame; rec: its record (emurx.abi.REC_DTYPE, from the oracle or emurx_classify_dev);
env6: nd_ref.Env, the MAC map, the IPv6 map and the clients of the handle; key = (ns_id, kind,
16 IP bytes, 6 MAC bytes).  The rule, with the reference's lines (paths relative to
src/emu/plugins):

  considered only if status OK and the descriptor is no hole; header offsets that do not fit the
  frame (no record of a classify has them) -> HOST
  arp     callback arp, lookup NS_LEVEL or above: the Namespace exists and has the arp plugin
          (arp/arp.go:956-969).  HandleRxArpPacket arp.go:904-946:
          operation 1 -> ARP_REQ whatever the target resolves to: ArpLearn runs first (:915-918)
          operation 2 -> ARP_REPLY unless the Ethernet destination is broadcast (:936-941), then NONE
          any other operation -> NONE (:943-944)
          key: sender IP p[l3+14:l3+18], sender MAC p[l3+8:l3+14]   PluginArpNs.ArpLearn :886-901
          (0.0.0.0 is learned like any other address: there is no test for it)
  nd      callback icmpv6, lookup NS_LEVEL, code 0
          type 135: nd_ref's checks (ipv6/nd.go:1550-1609, options of more than 8 bytes -> HOST);
              then :1611-1620: source IsGlobalUnicast, an SLLA present, CLookupByIPv6(source) nil
              -> ND_NS with key (source, SLLA); else NONE
          type 136 (:1687-1776): len(nd) < 20 -> NONE (:1691-1694); options p[l4+24:]: none ->
              NONE (no target MAC, :1733), {2, 1, mac} -> the target MAC, any other 8 bytes or
              1..7 bytes -> NONE (:1696-1724, decode errors included), more than 8 -> HOST; hop
              limit != 255 -> NONE (:1702-1705); flags & 0x20 clear -> NONE (:1726-1733); target
              neither link-local nor global unicast -> NONE (:1735-1736); EUI-64 target: learned
              unless CLookupByMac of the extracted MAC gives a client with IsValidPrefix
              (:1740-1756); any other target: learned unless CLookupByIPv6 finds it (:1758-1770);
              key (target, target MAC); a zero target MAC is learned (only solicitations test it)

An event is the fold of all frames with one key: count, first and last frame index; events are
ordered by ascending last.  ArpFlowTable.ArpLearn (arp.go:435-451) and
Ipv6NsCacheFlowTable.NdLearn (nd.go:608-624) write the MAC, then MoveToComplete from Incomplete /
Refresh and otherwise set touch: idempotent after the second application, so applying an event
once, and once more if count > 1, leaves the table as its frames one by one would (FlowTable
below, the model the tests replay both ways).  No text of the reference is restated here.
"""
import numpy as np

import nd_ref as N
import respond_ref as R
from emurx import abi, frames as F

CB_ARP, CB_ICMPV6 = 0, 9
BCAST = b"\xff" * 6


def _arp(p: bytes, rec, hole: bool):
    l3, n = int(rec["l3"]), len(p)
    if hole:
        return abi.LRN_NONE, None, "arp-hole"
    if l3 < 14 or l3 + 28 > n:
        return abi.LRN_HOST, None, "arp-bounds"
    op = (p[l3 + 6] << 8) | p[l3 + 7]
    if op == 1:
        kind = abi.LRN_ARP_REQ
    elif op == 2:
        if p[0:6] == BCAST:
            return abi.LRN_NONE, None, "arp-reply-broadcast"
        kind = abi.LRN_ARP_REPLY
    else:
        return abi.LRN_NONE, None, "arp-wrong-op"
    key = (int(rec["ns_id"]), kind, p[l3 + 14:l3 + 18] + bytes(12), p[l3 + 8:l3 + 14])
    return kind, key, "arp-request" if op == 1 else "arp-reply"


def _nd(p: bytes, rec, env: N.Env, hole: bool):
    l3, l4, n = int(rec["l3"]), int(rec["l4"]), len(p)
    if hole:
        return abi.LRN_NONE, None, "nd-hole"
    if l3 < 14 or l3 + 40 > l4 or l4 + 4 > n:
        return abi.LRN_HOST, None, "nd-bounds"
    typ = p[l4]
    if p[l4 + 1] != 0 or typ not in (135, 136):
        return abi.LRN_NONE, None, "nd-other-type"
    ns = int(rec["ns_id"])
    tk = (int(rec["vport"]), int(rec["vlan0"]), int(rec["vlan1"]))
    if typ == 135:
        # the responder's checks decide first; where they pass, its answer does not matter here
        why = N.nd_branch(p, rec, env)
        if why in ("options-long", "bounds"):
            return abi.LRN_HOST, None, "ns-" + why
        if why in ("too-short", "options-1-7", "options-8-wrong", "hop-limit", "slla-zero", "dad-with-slla",
                   "dad-unicast-dst", "target-unspec-mcast"):
            return abi.LRN_NONE, None, "ns-" + why
        assert why not in ("not-candidate", "not-ns"), why
        opts, src = p[l4 + 24:], p[l3 + 8:l3 + 24]
        if len(opts) != 8:
            return abi.LRN_NONE, None, "ns-no-slla"
        if not N.is_global_unicast(src):
            return abi.LRN_NONE, None, "ns-src-not-global"
        if env.ip6.get(tk + (src,)) is not None:
            return abi.LRN_NONE, None, "ns-src-ours"
        return abi.LRN_ND_NS, (ns, abi.LRN_ND_NS, src, opts[2:8]), "ns-learn"
    if n - (l4 + 4) < 20:
        return abi.LRN_NONE, None, "na-too-short"
    opts = p[l4 + 24:]
    if len(opts) > 8:
        return abi.LRN_HOST, None, "na-options-long"
    if len(opts) == 0:
        return abi.LRN_NONE, None, "na-no-option"
    if len(opts) < 8:
        return abi.LRN_NONE, None, "na-options-1-7"
    if opts[0] != 2 or opts[1] != 1:
        return abi.LRN_NONE, None, "na-options-8-wrong"
    mac = opts[2:8]
    if p[l3 + 7] != 255:
        return abi.LRN_NONE, None, "na-hop-limit"
    if not p[l4 + 4] & 0x20:
        return abi.LRN_NONE, None, "na-no-override"
    tgt = p[l4 + 8:l4 + 24]
    if not (N.is_link_local_unicast(tgt) or N.is_global_unicast(tgt)):
        return abi.LRN_NONE, None, "na-target-not-local-global"
    if tgt[11] == 0xFF and tgt[12] == 0xFE:
        emac = bytes([tgt[8] ^ 2, tgt[9], tgt[10], tgt[13], tgt[14], tgt[15]])
        cid = env.mac.get(tk + (emac,)) if emac != bytes(6) else None
        if cid is not None:
            ra = env.clients[cid]["ra"]
            if tgt[:8] == bytes([0xFE, 0x80] + [0] * 6) or (ra is not None and ra[1] == 64 and ra[0][:8] == tgt[:8]):
                return abi.LRN_NONE, None, "na-eui-ours"
        why = "na-learn-eui"
    else:
        if env.ip6.get(tk + (tgt,)) is not None:
            return abi.LRN_NONE, None, "na-ip6-ours"
        why = "na-learn-ip6"
    return abi.LRN_ND_NA, (ns, abi.LRN_ND_NA, tgt, mac), why


def _decide(frame: bytes, rec, env6, kinds: int, hole: bool):
    lk = (int(rec["flags"]) >> 4) & 7
    proto = int(rec["proto"])
    if int(rec["status"]) != 0:
        return abi.LRN_NONE, None, "not-candidate"
    if proto == CB_ARP and kinds & abi.LRNK_ARP and lk >= abi.LK["NS_LEVEL"]:
        return _arp(bytes(frame), rec, hole)
    if proto == CB_ICMPV6 and kinds & abi.LRNK_ND and lk == abi.LK["NS_LEVEL"]:
        return _nd(bytes(frame), rec, env6 if env6 is not None else N.Env(), hole)
    return abi.LRN_NONE, None, "not-candidate"


def learn_ref(frame: bytes, rec, env6=None, kinds: int = abi.LRNK_ALL, hole: bool = False):
    o, k, _ = _decide(frame, rec, env6, kinds, hole)
    return o, k


def learn_branch(frame: bytes, rec, env6=None, kinds: int = abi.LRNK_ALL, hole: bool = False) -> str:
    return _decide(frame, rec, env6, kinds, hole)[2]


# every branch of the rule a record of a classify can reach ("arp-bounds" and "nd-bounds" need a
# record that does not belong to its frame: test_learn_ref builds those by hand)
BRANCHES = ["not-candidate", "arp-hole", "arp-request", "arp-reply", "arp-reply-broadcast", "arp-wrong-op", "nd-hole",
            "nd-other-type", "ns-options-long", "ns-too-short", "ns-options-1-7", "ns-options-8-wrong", "ns-hop-limit",
            "ns-slla-zero", "ns-dad-with-slla", "ns-dad-unicast-dst", "ns-target-unspec-mcast", "ns-no-slla",
            "ns-src-not-global", "ns-src-ours", "ns-learn", "na-too-short", "na-options-long", "na-no-option",
            "na-options-1-7", "na-options-8-wrong", "na-hop-limit", "na-no-override", "na-target-not-local-global",
            "na-eui-ours", "na-ip6-ours", "na-learn-eui", "na-learn-ip6"]


def fold(keys):
    """keys: per frame a key or None -> the events [(key, count, first, last)] in ascending last."""
    acc = {}
    for i, k in enumerate(keys):
        if k is None:
            continue
        c = acc.get(k)
        acc[k] = (1, i, i) if c is None else (c[0] + 1, c[1], i)
    return sorted(((k, c, f, l) for k, (c, f, l) in acc.items()), key=lambda e: e[3])


def events_array(events) -> np.ndarray:
    ev = np.zeros(len(events), abi.LEARN_EV_DTYPE)
    for j, ((ns, kind, ip, mac), c, f, l) in enumerate(events):
        ev[j] = (ns, c, f, l, np.frombuffer(ip, np.uint8), np.frombuffer(mac, np.uint8), kind, 0)
    return ev


def learn_keys(buf, desc, rec, kinds: int = abi.LRNK_ALL, env6=None):
    """-> outcome u8 [n], the per-frame keys"""
    n = len(desc)
    outcome, keys = np.zeros(n, np.uint8), []
    for i in range(n):
        d = desc[i]
        f = bytes(buf[int(d["off"]):int(d["off"]) + int(d["len"])])
        o, k = learn_ref(f, rec[i], env6, kinds, hole=int(d["pad"]) == abi.DESC_HOLE)
        outcome[i] = o
        keys.append(k)
    return outcome, keys


def learn_batch(buf, desc, rec, kinds: int = abi.LRNK_ALL, env6=None, ev_cap=None):
    """emurx_learn_dev's outputs for a batch: outcome u8 [n], the events written
    (abi.LEARN_EV_DTYPE), info u64 [8]; ev_cap None = room for everything."""
    outcome, keys = learn_keys(buf, desc, rec, kinds, env6)
    ev = events_array(fold(keys))
    info = np.zeros(abi.LRN_INFO_WORDS, np.uint64)
    over = ev_cap is not None and len(ev) > ev_cap
    info[0], info[1], info[2] = 0 if over else len(ev), len(ev), int(over)
    for k in range(1, 6):
        info[2 + k] = int((outcome == k).sum())
    return outcome, ev[:0] if over else ev, info


# ---- the resolution table the events are replayed into --------------------------------------------
LEARNED, INCOMPLETE, COMPLETE, REFRESH = "learned", "incomplete", "complete", "refresh"


class FlowTable:
    """ArpFlowTable / Ipv6NsCacheFlowTable as far as learning touches them: the flows' state, MAC
    and touch flag, and the counters tblAdd, tblActive, addLearn, addIncomplete, moveComplete
    (AddNew arp.go:370-408, MoveToComplete :421-433, ArpLearn :435-451; nd.go:543-624 is the same
    code for IPv6).  Timers are not modelled: learning only restarts them."""

    def __init__(self):
        self.flows = {}
        self.c = dict(tblAdd=0, tblActive=0, addLearn=0, addIncomplete=0, moveComplete=0)

    def add_new(self, ip, mac, state):
        assert ip not in self.flows and state in (LEARNED, INCOMPLETE)
        self.c["tblAdd"] += 1
        self.c["tblActive"] += 1
        self.flows[ip] = dict(state=state, mac=mac, resolved=mac is not None, touch=False)
        self.c["addLearn" if state == LEARNED else "addIncomplete"] += 1

    def learn(self, ip, mac):
        """PluginArpNs.ArpLearn arp.go:886-901 / PluginIpv6Ns NdLearn: Lookup, then the table's
        learn or AddNew as Learned."""
        f = self.flows.get(ip)
        if f is None:
            self.add_new(ip, mac, LEARNED)
            return
        f["resolved"], f["mac"] = True, mac
        if f["state"] in (INCOMPLETE, REFRESH):
            f["touch"], f["state"] = False, COMPLETE
            self.c["moveComplete"] += 1
        else:
            f["touch"] = True

    def snapshot(self):
        return {k: dict(v) for k, v in self.flows.items()}, dict(self.c)


RX_COUNTER = {abi.LRN_ARP_REQ: "pktRxArpQuery", abi.LRN_ARP_REPLY: "pktRxArpReply",
              abi.LRN_ND_NS: "pktRxNeighborSolicitation", abi.LRN_ND_NA: "pktRxNeighborAdvLearn"}


class Caches:
    """Per Namespace an ARP table and an ND table, and the handlers' rx counters the events carry."""

    def __init__(self):
        self.tables, self.rx = {}, {}

    def table(self, ns, kind):
        return self.tables.setdefault((ns, "arp" if kind <= abi.LRN_ARP_REPLY else "nd"), FlowTable())

    def _count(self, ns, kind, n):
        k = (ns, RX_COUNTER[kind])
        self.rx[k] = self.rx.get(k, 0) + n

    def apply_frames(self, keys):
        """The Go handler's learning, frame by frame."""
        for k in keys:
            if k is not None:
                ns, kind, ip, mac = k
                self.table(ns, kind).learn(ip, mac)
                self._count(ns, kind, 1)

    def apply_events(self, events):
        """INTEGRATION.md's replay loop: each event in order, its learn call once, and once more if
        count > 1; count added to the kind's rx counter."""
        for (ns, kind, ip, mac), count, _, _ in events:
            t = self.table(ns, kind)
            t.learn(ip, mac)
            if count > 1:
                t.learn(ip, mac)
            self._count(ns, kind, count)

    def snapshot(self):
        return {k: t.snapshot() for k, t in self.tables.items()}, dict(self.rx)


# ---- the learning batch -----------------------------------------------------------------------
# nd_ref.combined_batch (respond_ref's mixed batch on vport 1, the ND batch on vport 2) with every
# fourth slot replaced by an entry of EXTRA below: ARP replies, advertisements and the
# solicitations the responder's batch has no reason to hold.  Few senders, so keys repeat.
def _extra():
    peer = bytes([0x20, 1, 0x0D, 0xB8, 0, 0xEE] + [0] * 9 + [7])
    tlla = lambda mac: b"\x02\x01" + mac  # noqa: E731

    def arp(op, dst=None, spa=None, sha=None):
        def make(ns, rng):
            tags = R._NS[ns]
            mac, ip4, _ = R._client(ns, int(rng.integers(0, R.N_CLIENTS)))
            s_ip = spa if spa is not None else bytes([16, ns, 0, 200 + int(rng.integers(0, 3))])
            s_mac = sha if sha is not None else bytes([0, 0x10, 0x94, 0, int(rng.integers(0, 2)), 2])
            f = R._eth(dst if dst is not None else mac, R.DUT_MAC, tags, 0x0806, F.arp(op, s_mac, s_ip, mac, ip4),
                       int(rng.integers(0, 7)))
            return f + bytes(max(60 - len(f), 0)), 1
        return make

    def na(target, flags=0x60, opts="tlla", mac=None, **kw):
        def make(ns, rng):
            ns %= len(N._NS)
            t = target(ns, rng) if callable(target) else target
            m = mac if mac is not None else bytes([0, 0x10, 0x94, 0, int(rng.integers(0, 2)), 9])
            o = tlla(m) if opts == "tlla" else opts
            src = peer[:15] + bytes([int(rng.integers(1, 4))])
            return N.ns_frame(N._NS[ns], int(rng.integers(0, 7)), t, src=src, dst=N.ALL_NODES,
                              edst=bytes([0x33, 0x33, 0, 0, 0, 1]), typ=136, body=bytes([flags, 0, 0, 0]) + t + o, **kw), N.VPORT
        return make

    def ns_(src, **kw):
        def make(ns, rng):
            ns %= len(N._NS)
            return N.ns_frame(N._NS[ns], int(rng.integers(0, 7)), N.eui_of(N._client(ns, 0)[0]), src=src(ns, rng), **kw), N.VPORT
        return make

    few = lambda ns, rng: peer[:14] + bytes([ns, int(rng.integers(1, 4))])  # noqa: E731
    return [
        arp(2), arp(2, dst=BCAST), arp(3), arp(1, dst=BCAST, spa=bytes(4)), arp(2, spa=bytes([16, 0, 0, 2]), sha=bytes([0, 0, 0, 2, 0, 0])),
        na(few), na(lambda ns, rng: N.eui_of(bytes([0, 0, 9, ns, 0, int(rng.integers(1, 3))]))),
        na(few, flags=0x40), na(few, opts=b""), na(few, opts=N.slla(N.PEER_MAC)), na(few, opts=tlla(N.PEER_MAC) + bytes([14, 1, 1, 2, 3, 4, 5, 6])),
        na(few, opts=tlla(N.PEER_MAC)[:7]), na(few, hop=64), na(N.ALL_NODES), na(bytes(15) + b"\x01"),
        na(lambda ns, rng: N.eui_of(N._client(ns, 0)[0])), na(lambda ns, rng: N._client(ns, 1)[1]),
        na(lambda ns, rng: N.eui_of(N._client(ns, 1)[0], N._client(ns, 1)[4][0])),
        na(lambda ns, rng: N.eui_of(N._client(ns, 0)[0], peer)), na(lambda ns, rng: N.eui_of(N._client(ns, 3)[0], N._client(ns, 3)[4][0])),
        na(few, mac=bytes(6)), na(few, opts=b"\x02\x00" + N.PEER_MAC),
        na(bytes([0xFE, 0x80] + [0] * 12 + [0x12, 0x34])), na(few, ext=8), na(few, code=1),
        na(bytes([0xFE, 0x80] + [0] * 6 + [2, 0, 0, 0xFF, 0xFE, 0, 0, 0])),
        ns_(lambda ns, rng: N._client(ns, 1)[1]), ns_(lambda ns, rng: N._client(ns, 0)[2]), ns_(few),
        ns_(few, opts=N.slla(N.PEER_MAC) + bytes([14, 1, 1, 2, 3, 4, 5, 6])), ns_(few, opts=b""),
    ]


def na_short(ns: int):
    """An advertisement whose ICMPv6 body is 16 bytes: len(nd) < 20."""
    return N.ns_frame(N._NS[ns], 0, bytes(16), src=bytes([0x20, 1, 0x0D, 0xB8] + [0] * 11 + [9]), dst=N.ALL_NODES,
                      edst=bytes([0x33, 0x33, 0, 0, 0, 1]), typ=136, body=bytes([0x60, 0, 0, 0]) + bytes(12))


EXTRA = _extra() + [lambda ns, rng: (na_short(ns % len(N._NS)), N.VPORT)]
HOLE_EVERY = 37  # coprime to the period of EXTRA's entries, so holes fall on each of them in turn


def learning_batch(n: int, seed: int = 5):
    """-> (frames, vports): N.combined_batch(n) with slot 4j + 3 replaced by EXTRA[j % len(EXTRA)]."""
    frames, vports = N.combined_batch(n, seed)
    rng = np.random.default_rng([seed, 0x6C726E])
    for j, i in enumerate(range(3, n, 4)):
        frames[i], vports[i] = EXTRA[j % len(EXTRA)](int(rng.integers(0, len(R._NS))), rng)
    return frames, vports


def pack(frames, vports, every: int = HOLE_EVERY):
    return R.pack_with_holes(frames, vports, every)


def arp_requests(n: int, senders: int, ns: int = 0, seed: int = 1):
    """n ARP requests for client 0 of respond_ref's Namespace ns from `senders` distinct senders
    (IP and MAC both count up), sender j at every frame i with i % senders == j."""
    mac, ip4, _ = R._client(ns, 0)
    out = []
    for i in range(n):
        j = i % senders
        sha = bytes([0, 0x10, 0x94, (j >> 16) & 0xFF, (j >> 8) & 0xFF, j & 0xFF])
        spa = bytes([48, (j >> 16) & 0xFF, (j >> 8) & 0xFF, j & 0xFF])
        f = R._eth(BCAST, sha, R._NS[ns], 0x0806, F.arp(1, sha, spa, bytes(6), ip4), 0)
        out.append(f + bytes(max(60 - len(f), 0)))
    return out, [1] * n

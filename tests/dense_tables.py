"""Dense tables: Namespaces, clients, flows and listeners placed so that the device's bucket walks
(csrc/emurx_parse.h resolve_ns / resolve_mac / resolve_ip4 / resolve_ip6 / client_info / flow_probe)
meet long chains, the step from the last bucket to bucket 0, tombstones, removed keys and keys put
back into a tombstone's slot, and a batch whose frames drive each of those lookups.

The tables are at spread 2 (EMURX_TABLE_SPREAD=2,2,2,2, read once per process: every user of this
module runs in a child process started with ENV) on a handle of CFG.  build() works on a host-only
handle: it draws candidate keys from a seeded generator, learns each one's home bucket from
emurx_image_probe, keeps those that fall where a cluster needs them and records every table call
in an ordered list (Scenario.ops) that replay() applies to any target: an RxPath, the oracle, the
Model below, the responder's and learner's Env twins.  The coverage the batch reaches is computed
by probing the final image; a condition that is not met is an error, not a skip.

Cluster layout (buckets of S slots; `last` = the table's last bucket).  Keys homed at `last` are
inserted in order, so they fill last, 0, 1, ...; then (phase B) key 1 is removed and put back (it
lands in its own tombstone), key 2 is removed (a tombstone in the home bucket), for the 4-slot
tables key 5 too (a tombstone in bucket 0); `unknown` keys homed at `last` are never inserted.

No torch at module level; the GPU drivers at the end import it inside.
"""
import struct

import numpy as np

import learn_ref as L
import nd_ref as N
import respond_ref as R
from emurx import abi, frames as F

NS, MAC, IP4, IP6, CI, FT4, FT6, SRV = range(8)
TNAME = ["ns", "mac", "ip4", "ip6", "ci", "flow4", "flow6", "listener"]
ENV = {"EMURX_TABLE_SPREAD": "2,2,2,2"}
CFG = dict(max_ns=16, max_clients=64, max_frames=1024)
# bucket counts at ENV / CFG, and live + tombstone slots above which a table is rebuilt
# (Mirror::set_partition, Hash::full)
BUCKETS = {NS: 8, MAC: 32, IP4: 64, IP6: 64, CI: 64, FT4: 64, FT6: 256, SRV: 32}
REBUILD_ABOVE = {NS: 24, MAC: 96, IP4: 96, IP6: 96, CI: 96, FT4: 16, FT6: 16, SRV: 32}
CONDITIONS = ["hit3", "hit_wrap", "hit_tomb", "miss3_tomb", "miss_wrap", "miss_removed", "hit_readded"]
WALKED = [NS, MAC, IP4, IP6, FT4, FT6, SRV]  # every condition is required of these
SIZES = [1, 64, 65, 257, None]  # None: the full batch
PEER_MAC = bytes([0x00, 0x10, 0x94, 0, 0, 0x09])
BCAST = b"\xff" * 6
PLUG_ARP, PLUG_TRANSPORT, PLUG_IPV6 = 1 << 0, 1 << 7, 1 << 8


def le32(b):
    return int.from_bytes(bytes(b[:4]), "little")


def ns_words(nsk):
    vport, tags = nsk
    v = [(t << 16) | vid for t, vid in tags] + [0, 0]
    return (vport, v[0], v[1])


def ns_key(nsk):
    return F.tunnel_key(*ns_words(nsk))


def mac_words(ns, mac):
    return (ns, le32(mac), mac[4] | (mac[5] << 8))


def ip4_words(ns, ip):
    return (ns, le32(ip))


def ip6_words(ns, ip):
    return (ns,) + tuple(le32(ip[4 * k:4 * k + 4]) for k in range(4))


def ft_words(cid, t):
    """(table, key words) of a c5tuplekey: 13 bytes over IPv4, 37 over IPv6."""
    if len(t) == 13:
        return FT4, (cid, le32(t[0:4]), le32(t[4:8]), le32(t[8:12]), t[12])
    return FT6, (cid,) + tuple(le32(t[4 * k:4 * k + 4]) for k in range(9)) + (t[36],)


def srv_words(cid, port, proto):
    return (cid, port | (proto << 16))


# ---- the Python truth of the tables ---------------------------------------------------------------
class Model:
    """The tables as dicts, kept by the same calls as an RxPath: keys[table][key words] = the value
    the device image answers; `removed` / `readded`: (table, key) ever removed / put back after."""

    def __init__(self):
        self.keys = [dict() for _ in range(8)]
        self.removed, self.readded = set(), set()
        self.ns, self.cl = {}, {}  # ns id -> dict(nsk-independent key bytes, order); cid -> client

    def _put(self, t, k, v):
        self.keys[t][k] = v
        if (t, k) in self.removed:
            self.readded.add((t, k))

    def _del(self, t, k):
        del self.keys[t][k]
        self.removed.add((t, k))
        self.readded.discard((t, k))

    def ns_add(self, key, ns_id, plugins):
        self.ns[ns_id] = dict(key=bytes(key), plugins=plugins, order=[])
        v, _, a, b = struct.unpack("<HHII", key)
        self._put(NS, (v, a, b), ns_id)
        return 0

    def ns_remove(self, key):
        v, _, a, b = struct.unpack("<HHII", key)
        ns_id = self.keys[NS][(v, a, b)]
        assert not self.ns[ns_id]["order"]
        self._del(NS, (v, a, b))
        del self.ns[ns_id]
        return 0

    def client_add(self, ns, cid, mac, ip4=None, ip6=None, d6=None, plugins=abi.PLUG_ALL):
        c = dict(ns=ns, mac=bytes(mac), ip4=ip4 and bytes(ip4), ip6=ip6 and bytes(ip6), d6=d6 and bytes(d6),
                 plugins=plugins, ra=None, ctx=False)
        self.cl[cid] = c
        self.ns[ns]["order"].append(cid)
        self._put(MAC, mac_words(ns, c["mac"]), cid)
        if c["ip4"]:
            self._put(IP4, ip4_words(ns, c["ip4"]), cid)
        for a in (c["ip6"], c["d6"]):
            if a:
                self._put(IP6, ip6_words(ns, a), cid)
        self._put(CI, (cid,), plugins)
        return 0

    def client_remove(self, ns, mac):
        cid = self.keys[MAC][mac_words(ns, bytes(mac))]
        c = self.cl.pop(cid)
        self.ns[ns]["order"].remove(cid)
        self._del(MAC, mac_words(ns, c["mac"]))
        if c["ip4"]:
            self._del(IP4, ip4_words(ns, c["ip4"]))
        for a in (c["ip6"], c["d6"]):
            if a:
                self._del(IP6, ip6_words(ns, a))
        self._del(CI, (cid,))
        for t in (FT4, FT6, SRV):
            for k in [k for k in self.keys[t] if k[0] == cid]:
                self._del(t, k)
        return 0

    def _update(self, cid, field, table, words, ip):
        c = self.cl[cid]
        if c[field]:
            self._del(table, words(c["ns"], c[field]))
        c[field] = bytes(ip)
        self._put(table, words(c["ns"], c[field]), cid)
        return 0

    def client_update_ipv4(self, cid, ip):
        return self._update(cid, "ip4", IP4, ip4_words, ip)

    def client_update_ipv6(self, cid, ip):
        return self._update(cid, "ip6", IP6, ip6_words, ip)

    def client_update_dipv6(self, cid, ip):
        return self._update(cid, "d6", IP6, ip6_words, ip)

    def client_set_ra(self, cid, prefix, plen):
        self.cl[cid]["ra"] = (bytes(prefix), plen)
        return 0

    def client_set_transport(self, cid, has):
        self.cl[cid]["ctx"] = bool(has)
        return 0

    def flow_add(self, cid, t, fid):
        self._put(*ft_words(cid, bytes(t)), fid)
        self.cl[cid]["ctx"] = True
        return 0

    def flow_remove(self, cid, t):
        self._del(*ft_words(cid, bytes(t)))
        return 0

    def server_add(self, cid, port, proto):
        self._put(SRV, srv_words(cid, port, proto), 1)
        self.cl[cid]["ctx"] = True
        return 0

    def server_remove(self, cid, port, proto):
        self._del(SRV, srv_words(cid, port, proto))
        return 0

    def envs(self):
        """The responder's and the learner's views (respond_ref.Env, nd_ref.Env) of these tables."""
        e4, e6 = R.Env(), N.Env()
        for cid, c in self.cl.items():
            key = self.ns[c["ns"]]["key"]
            e4.add(key, cid, c["mac"], c["ip4"])
            e6.add(key, cid, c["mac"], c["ip6"], c["d6"], c["plugins"], c["ra"])
        return e4, e6


PHASES = ("A", "B", "C")  # additions; removals and re-additions; one more removal mid-chain


def replay(ops, target, phases=PHASES):
    """Apply the recorded table calls of `phases`, in order, to an RxPath / Oracle / Model."""
    for ph, name, args in ops:
        if ph in phases:
            rc = getattr(target, name)(*args)
            assert rc == 0, (ph, name, args, rc)


# ---- frames ---------------------------------------------------------------------------------------
def _eth(nsk, dst, src, etype, payload, pcp=0):
    f = R._eth(dst, src, nsk[1], etype, payload, pcp)
    return f + bytes(max(60 - len(f), 0))


def f_l4(nsk, dmac, t, syn=False, pcp=0):
    """tcp / udp carrying the c5tuplekey t (13 bytes: IPv4, 37: IPv6) to dmac."""
    v6 = len(t) == 37
    n = 16 if v6 else 4
    src, dst, (sport, dport), proto = t[:n], t[n:2 * n], struct.unpack(">HH", t[2 * n:2 * n + 4]), t[-1]
    body = bytes(range(12))
    ln = (8 if proto == 17 else 20) + len(body)
    ps = F.ipv6_pseudo(src, dst, ln, proto) if v6 else F.ipv4_pseudo(src, dst, proto, ln)
    seg = F.udp(sport, dport, body, csum="auto", pseudo=ps) if proto == 17 else \
        F.tcp(sport, dport, body, flags=0x02 if syn else 0x18, pseudo=ps)
    ip = F.ipv6(src, dst, proto, seg) if v6 else F.ipv4(src, dst, proto, seg)
    return _eth(nsk, dmac, PEER_MAC, 0x86DD if v6 else 0x0800, ip, pcp)


def f_arp(nsk, tpa, spa, pcp=0):
    return _eth(nsk, BCAST, PEER_MAC, 0x0806, F.arp(1, PEER_MAC, spa, bytes(6), tpa), pcp)


def f_echo4(nsk, dmac, dst, src, pcp=0):
    return _eth(nsk, dmac, PEER_MAC, 0x0800, F.ipv4(src, dst, 1, F.icmp4(8, 0, 7, 9, b"dense-tables")), pcp)


def f_echo6(nsk, dmac, dst, src, pcp=0):
    body = struct.pack(">HH", 7, 9) + b"dense-tables"
    ic = F.icmp6(128, 0, body, pseudo=F.ipv6_pseudo(src, dst, 4 + len(body), 58))
    return _eth(nsk, dmac, PEER_MAC, 0x86DD, F.ipv6(src, dst, 58, ic), pcp)


def f_dhcpsrv(nsk, pcp=0):
    src, dst = bytes(4), b"\xff" * 4
    u = F.udp(68, 67, b"abcd", csum="auto", pseudo=F.ipv4_pseudo(src, dst, 17, 12))
    return _eth(nsk, BCAST, PEER_MAC, 0x0800, F.ipv4(src, dst, 17, u), pcp)


def f_dhcp(nsk, dmac, pcp=0):
    src, dst = bytes([48, 0, 0, 1]), bytes([16, 0, 0, 9])
    u = F.udp(67, 68, b"abcd", csum="auto", pseudo=F.ipv4_pseudo(src, dst, 17, 12))
    return _eth(nsk, dmac, PEER_MAC, 0x0800, F.ipv4(src, dst, 17, u), pcp)


def f_eapol(nsk, pcp=0):
    return _eth(nsk, bytes([1, 0x80, 0xC2, 0, 0, 3]), PEER_MAC, F.ETH_EAPOL, b"\x01\x00\x00\x05", pcp)


def f_nsol(nsk, tgt, src, pcp=0):
    """A neighbour solicitation for tgt from src (global, with its link-layer address)."""
    return N.ns_frame(nsk[1], pcp, tgt, src=src)


def f_nadv(nsk, tgt, src, mac, pcp=0):
    """An overriding neighbour advertisement of tgt with the target link-layer address mac."""
    return N.ns_frame(nsk[1], pcp, tgt, src=src, dst=N.ALL_NODES, edst=bytes([0x33, 0x33, 0, 0, 0, 1]), typ=136,
                      body=bytes([0x60, 0, 0, 0]) + tgt + b"\x02\x01" + mac)


class Scenario:
    """ops: [(phase, call, args)] (model_of replays them into a Model); frames: [dict(f, vport, kind,
    lookups [(table, key words)], want (ns id or None, client id or None))], built against the tables
    after phases A + B; orders: name -> frame indices of a batch ("grouped": every walking frame, 64
    plain ones, the walking frames backwards; "interleaved": per table its longest hit and miss, each
    alone among 63 plain frames at lane 0 or 63 of its wave; `lone` lists them); coverage: table name
    -> condition -> frame indices; trace: (table, key) -> emurx_image_probe's dict on the image after
    A + B; chain: table name -> longest walk of the batch; buckets: table name -> bucket count."""


def batch(sc, order, n=None):
    idx = sc.orders[order][:n]
    return F.pack_frames([sc.frames[i]["f"] for i in idx], [sc.frames[i]["vport"] for i in idx])


def carried(sc, order, pos):
    """What frame `pos` of a batch is there for: its kind and the coverage conditions it carries."""
    i = (sc.orders[order] if isinstance(order, str) else order[1])[pos]
    order = order if isinstance(order, str) else order[0]
    conds = [f"{t}:{c}" for t, cs in sc.coverage.items() for c, fr in cs.items() if i in fr]
    return f"frame {pos} of order {order} (scenario frame {i}, {sc.frames[i]['kind']}) carries {conds or 'no condition'}"


# ---- the builder ------------------------------------------------------------------------------------
class _Builder:
    def __init__(self):
        from emurx.rx import RxPath
        self.rx = RxPath(-1, **CFG)
        self.model = Model()
        self.ops, self.phase = [], "A"
        self.rng = np.random.default_rng([2024, 0x64656E73])
        self.used = set()
        self.nb = {}
        for t in range(8):
            self.nb[t] = self.rx.image_probe(t, [0] * 11)["buckets"] if t in (NS, CI, FT4, FT6, SRV) else None

    def op(self, name, *args):
        self.ops.append((self.phase, name, args))
        for t in (self.rx, self.model):
            rc = getattr(t, name)(*args)
            assert rc == 0, (self.phase, name, args, rc)

    def home(self, table, words):
        p = self.rx.image_probe(table, list(words))
        assert p["buckets"], (TNAME[table], words)  # a client key needs its Namespace alive
        self.nb[table] = p["buckets"]
        return p["home"]

    def rnd(self, n):
        return self.rng.integers(0, 256, n, dtype=np.uint8).tobytes()

    def draw(self, table, gen, words, where, count, limit=200000):
        """`count` fresh candidates gen() whose home bucket satisfies where(home, buckets)."""
        out = []
        for _ in range(limit):
            c = gen()
            w = (table, tuple(words(c)))
            if w in self.used:
                continue
            h = self.home(table, w[1])
            if where(h, self.nb[table]):
                self.used.add(w)
                out.append(c)
                if len(out) == count:
                    return out
        raise AssertionError(f"no {count} candidates for {TNAME[table]}")

    # candidate generators
    def g_nsk(self):
        r = self.rng
        kind = int(r.integers(0, 3))
        vid = lambda: int(r.integers(1, 4095))  # noqa: E731
        tags = [((0x8100, vid()),), ((0x8100, vid()), (0x8100, vid())), ((0x88A8, vid()), (0x8100, vid()))][kind]
        return (int(r.integers(1, 7)), tags)

    def g_mac(self):
        return bytes([0x00, 0x1B]) + self.rnd(4)

    def g_ip4(self):
        return bytes([16]) + self.rnd(2) + bytes([int(self.rng.integers(1, 255))])

    def g_ip6(self):  # global, not of the EUI-64 form (bytes 11, 12 = ff fe)
        a = bytearray(bytes([0x20, 1, 0x0D, 0xB8]) + self.rnd(12))
        a[11] = 0
        return bytes(a)

    def g_t4(self, proto=None):
        p = proto or (6 if self.rng.integers(0, 2) else 17)
        return bytes([48]) + self.rnd(3) + bytes([16]) + self.rnd(3) + \
            struct.pack(">HH", int(self.rng.integers(1024, 65536)), int(self.rng.integers(1, 1024))) + bytes([p])

    def g_t6(self):
        p = 6 if self.rng.integers(0, 2) else 17
        return self.g_ip6() + self.g_ip6() + \
            struct.pack(">HH", int(self.rng.integers(1024, 65536)), int(self.rng.integers(1, 1024))) + bytes([p])


def at_last(h, nb):
    return h == nb - 1


def away(h, nb):  # clear of a cluster at the last bucket and of its overflow
    return 4 <= h < nb - 2


def build():
    """-> Scenario.  Everything is seeded: two calls give the same scenario."""
    b = _Builder()
    rx, m = b.rx, b.model
    sc = Scenario()

    # ---- Namespaces: 11 homed at the last bucket (ids 0..10), 2 unknown there, 2 elsewhere ----------
    kc = b.draw(NS, b.g_nsk, ns_words, at_last, 11)
    ku = b.draw(NS, b.g_nsk, ns_words, at_last, 2)
    kp = b.draw(NS, b.g_nsk, ns_words, lambda h, nb: 2 <= h < nb - 2, 2)
    # ids in insertion order, but cluster keys 3 and 5 swapped: the Namespaces removed in phase B
    # (keys 1, 2, 5) then have ids 1, 2, 3, one 64-byte block of the dense ns-info array, so that its
    # edits travel as a delta block too (a quarter of an array edited ships the whole array)
    ids = list(range(13))
    ids[3], ids[5] = 5, 3
    for i, k in zip(ids, kc + kp):
        b.op("ns_add", ns_key(k), i, abi.PLUG_ALL)
    A, Bn, Cn, P = 0, 8, 9, 11  # nsA: home bucket, first slot; nsB, nsC: three buckets deep; P: elsewhere
    nsk = {i: k for i, k in zip(ids, kc + kp)}

    # ---- client ids: two triples of ids that share a client-info home bucket -------------------------
    by_home = {}
    for cid in range(CFG["max_clients"]):
        by_home.setdefault(b.home(CI, (cid,)), []).append(cid)
    triples = sorted((v for v in by_home.values() if len(v) >= 3), key=lambda v: v[0])
    assert len(triples) >= 2, "no two client-info buckets with three ids: use max_clients=128"
    (ci_a, ci_b, ci_first), (ci_d, ci_e, ci_ra) = triples[0][:3], triples[1][:3]
    special = {ci_a, ci_b, ci_first, ci_d, ci_e, ci_ra}
    pool = [c for c in range(CFG["max_clients"]) if c not in special]
    take = lambda: pool.pop(0)  # noqa: E731

    def mac_away(ns):
        return b.draw(MAC, b.g_mac, lambda x: mac_words(ns, x), away, 1)[0]

    # ---- MAC cluster in nsA: M0..M10, 2 unknown -------------------------------------------------------
    M = b.draw(MAC, b.g_mac, lambda x: mac_words(A, x), at_last, 11)
    MU = b.draw(MAC, b.g_mac, lambda x: mac_words(A, x), at_last, 2)
    mcid = {0: ci_b, 1: ci_a, 2: ci_d, 3: ci_e, 8: ci_ra}
    mcid = [mcid.get(i, None) for i in range(11)]
    mcid = [c if c is not None else take() for c in mcid]
    ra_prefix = bytes([0x20, 1, 0x0D, 0xB8, 0, 0xAA, 0, 1]) + bytes(8)
    for i in range(11):
        plug = abi.PLUG_ALL & ~PLUG_IPV6 if i == 10 else abi.PLUG_ALL
        b.op("client_add", A, mcid[i], M[i], None, None, None, plug)
    b.op("client_set_ra", mcid[8], ra_prefix, 64)
    b.op("client_set_ra", mcid[3], ra_prefix, 48)  # IsValidPrefix takes only 64

    # ---- IPv4 cluster in nsB: X0..X6 (two per bucket), 2 unknown ---------------------------------------
    X = b.draw(IP4, b.g_ip4, lambda x: ip4_words(Bn, x), at_last, 7)
    XU = b.draw(IP4, b.g_ip4, lambda x: ip4_words(Bn, x), at_last, 2)
    x_else = b.draw(IP4, b.g_ip4, lambda x: ip4_words(Bn, x), away, 1)[0]
    xmac, xcid = [mac_away(Bn) for _ in X], [take() for _ in X]
    for i in range(7):
        plug = abi.PLUG_ALL & ~PLUG_ARP if i == 5 else abi.PLUG_ALL
        b.op("client_add", Bn, xcid[i], xmac[i], X[i], None, None, plug)

    # ---- IPv6 cluster in nsC: V0..V6 over four clients (ipv6, dhcpv6), 2 unknown; the Namespace's first
    # client has the id whose client-info slot lies past its home bucket -------------------------------
    first_mac = mac_away(Cn)
    b.op("client_add", Cn, ci_first, first_mac, None, None, None, abi.PLUG_ALL)
    V = b.draw(IP6, b.g_ip6, lambda x: ip6_words(Cn, x), at_last, 7)
    VU = b.draw(IP6, b.g_ip6, lambda x: ip6_words(Cn, x), at_last, 2)
    v_else = b.draw(IP6, b.g_ip6, lambda x: ip6_words(Cn, x), away, 2)
    ymac, ycid = [mac_away(Cn) for _ in range(4)], [take() for _ in range(4)]
    vown = {}
    for j in range(4):
        a6, d6 = V[2 * j], V[2 * j + 1] if 2 * j + 1 < 7 else None
        plug = abi.PLUG_ALL & ~PLUG_IPV6 if j == 3 else abi.PLUG_ALL
        b.op("client_add", Cn, ycid[j], ymac[j], None, a6, d6, plug)
        vown[2 * j], vown[2 * j + 1] = j, j

    # ---- plain clients (every lookup ends in its home bucket): the 63 other lanes of a wave ---------
    pl = []
    for j in range(3):
        mac = mac_away(P)
        ip = b.draw(IP4, b.g_ip4, lambda x: ip4_words(P, x), away, 1)[0]
        cid = take()
        b.op("client_add", P, cid, mac, ip, None, None, abi.PLUG_ALL)
        pl.append((cid, mac, ip))

    # ---- flows and listeners: flow4 of client G (nsA, plain MAC), flow6 of M9 (three buckets deep),
    # listeners of both --------------------------------------------------------------------------------
    G, gmac = take(), mac_away(A)
    b.op("client_add", A, G, gmac, None, None, None, abi.PLUG_ALL)
    H = mcid[9]
    T4 = b.draw(FT4, b.g_t4, lambda t: ft_words(G, t)[1], at_last, 7)
    T4U = b.draw(FT4, b.g_t4, lambda t: ft_words(G, t)[1], at_last, 2)
    T6 = b.draw(FT6, b.g_t6, lambda t: ft_words(H, t)[1], at_last, 5)
    T6U = b.draw(FT6, b.g_t6, lambda t: ft_words(H, t)[1], at_last, 2)
    g_srv = lambda: ((G, H)[int(b.rng.integers(0, 2))], int(b.rng.integers(1, 65536)), (6, 17)[int(b.rng.integers(0, 2))])  # noqa: E731
    S = b.draw(SRV, g_srv, lambda s: srv_words(*s), at_last, 11)
    SU = b.draw(SRV, g_srv, lambda s: srv_words(*s), at_last, 2)
    for i, t in enumerate(T4):
        b.op("flow_add", G, t, 100 + i)
    for i, t in enumerate(T6):
        b.op("flow_add", H, t, 200 + i)
    for s in S:
        b.op("server_add", *s)
    noctx = take()  # transport plugin, no TransportCtx
    noctx_mac = mac_away(A)
    b.op("client_add", A, noctx, noctx_mac, None, None, None, abi.PLUG_ALL)

    # ---- phase B: tombstones, and keys put back into them -----------------------------------------------
    b.phase = "B"
    for k in (1, 2, 5):
        b.op("ns_remove", ns_key(kc[k]))
    b.op("ns_add", ns_key(kc[1]), 1, abi.PLUG_ALL)
    for k in (1, 2, 5):
        b.op("client_remove", A, M[k])
    m1 = take()
    b.op("client_add", A, m1, M[1], None, None, None, abi.PLUG_ALL)
    b.op("client_update_ipv4", xcid[1], x_else)
    b.op("client_update_ipv4", xcid[1], X[1])
    b.op("client_remove", Bn, xmac[2])
    b.op("client_update_dipv6", ycid[0], v_else[0])
    b.op("client_update_dipv6", ycid[0], V[1])
    b.op("client_update_ipv6", ycid[1], v_else[1])
    b.op("flow_remove", G, T4[1])
    b.op("flow_add", G, T4[1], 150)
    b.op("flow_remove", G, T4[2])
    b.op("flow_remove", H, T6[1])
    b.op("flow_add", H, T6[1], 250)
    b.op("flow_remove", H, T6[2])
    for k in (1, 2, 5):
        b.op("server_remove", *S[k])
    b.op("server_add", *S[1])

    # ---- the frames, against the tables after A + B -------------------------------------------------------
    frames = []
    peer4 = bytes([48, 0, 0, 7])
    peer6 = bytes([0x20, 1, 0x0D, 0xB8, 0, 0xEE] + [0] * 9 + [7])

    def ns_of(k):
        return m.keys[NS].get(ns_words(k))

    def add(kind, k, f, lookups, cid=None):
        """lookups: the (table, key) pairs behind the Namespace's; cid: the client the record names."""
        ns = ns_of(k)
        lk = [(NS, ns_words(k))] + (list(lookups) if ns is not None else [])
        frames.append(dict(f=f, vport=k[0], kind=kind, lookups=lk, want=(ns, cid if ns is not None else None)))
        return len(frames) - 1

    def l4(kind, k, dmac, t, syn=False, pcp=0):
        ns = ns_of(k)
        lk, cid = [], None
        if ns is not None:
            lk.append((MAC, mac_words(ns, dmac)))
            cid = m.keys[MAC].get(mac_words(ns, dmac))
            c = m.cl.get(cid)
            if c is not None and c["plugins"] & PLUG_TRANSPORT and c["ctx"]:
                ft = ft_words(cid, t)
                lk.append(ft)
                if ft[1] not in m.keys[ft[0]] and (t[-1] == 17 or syn):
                    lk.append((SRV, srv_words(cid, struct.unpack(">H", t[-3:-1])[0], t[-1])))
        return add(kind, k, f_l4(k, dmac, t, syn, pcp), lk, cid)

    def eui_lookups(ns, tgt):
        mac = bytes([tgt[8] ^ 2, tgt[9], tgt[10], tgt[13], tgt[14], tgt[15]])
        lk = [(MAC, mac_words(ns, mac))]
        cid = m.keys[MAC].get(mac_words(ns, mac))
        if cid is not None and tgt[:8] != bytes([0xFE, 0x80] + [0] * 6):
            lk.append((CI, (cid,)))
            ra = m.cl[cid]["ra"]
            if not (ra and ra[1] == 64 and ra[0][:8] == tgt[:8]):
                cid = None
        return lk, cid, mac

    kA, kB, kC, kP = nsk[A], nsk[Bn], nsk[Cn], nsk[P]
    # Namespaces: every cluster key (the removed ones and the one put back among them) and the unknown
    for i, k in enumerate(kc + ku):
        l4(f"ns{i} tcp to an unknown MAC", k, b.g_mac(), b.g_t4(6), pcp=i % 7)
    # MAC: tcp / udp / dhcp to every cluster MAC and the unknown
    for i, mac in enumerate(M + MU):
        if i % 4 == 3:
            ns, cid = A, m.keys[MAC].get(mac_words(A, mac))
            add(f"mac{i} dhcp", kA, f_dhcp(kA, mac, i % 7), [(MAC, mac_words(ns, mac))], cid)
        else:
            l4(f"mac{i} {'tcp' if i % 2 else 'udp'}", kA, mac, b.g_t4(6 if i % 2 else 17), pcp=i % 7)
    # IPv4: an ARP request for, and an ICMP echo to, every cluster address and the unknown
    for i, ip in enumerate(X + XU):
        cid = m.keys[IP4].get(ip4_words(Bn, ip))
        c = m.cl.get(cid)
        add(f"ip4-{i} arp request", kB, f_arp(kB, ip, peer4, i % 7), [(IP4, ip4_words(Bn, ip))],
            cid if c and c["plugins"] & PLUG_ARP else None)
        add(f"ip4-{i} echo", kB, f_echo4(kB, c["mac"] if c else xmac[0], ip, peer4, i % 7), [(IP4, ip4_words(Bn, ip))], cid)
    # IPv6: an echo to every cluster address and the unknown
    for i, ip in enumerate(V + VU):
        cid = m.keys[IP6].get(ip6_words(Cn, ip))
        add(f"ip6-{i} echo", kC, f_echo6(kC, m.cl[cid]["mac"] if cid is not None else ymac[0], ip, peer6, i % 7),
            [(IP6, ip6_words(Cn, ip))], cid)
    # EUI-64: link-local echoes to every cluster MAC, RA-prefix echoes to the RA clients and one without
    for i, mac in enumerate(M + MU):
        tgt = N.eui_of(mac)
        lk, cid, _ = eui_lookups(A, tgt)
        add(f"eui-ll mac{i} echo", kA, f_echo6(kA, mac, tgt, peer6, i % 7), lk, cid)
    for i in (8, 3, 0, 9):
        tgt = N.eui_of(M[i], ra_prefix)
        lk, cid, _ = eui_lookups(A, tgt)
        add(f"eui-ra mac{i} echo", kA, f_echo6(kA, M[i], tgt, peer6, i % 7), lk, cid)
    # GetFirstClient: dhcpsrv broadcast and eapol in nsC (its first client's info lies past the home
    # bucket), nsA and nsB
    for k, ns in ((kC, Cn), (kA, A), (kB, Bn)):
        first = m.ns[ns]["order"][0]
        add(f"dhcpsrv ns{ns}", k, f_dhcpsrv(k, 1), [(CI, (first,))], first)
        add(f"eapol ns{ns}", k, f_eapol(k, 2), [(CI, (first,))], first)
    # flows: every cluster tuple and the unknown (tcp without SYN, with SYN, udp), listeners
    for i, t in enumerate(T4 + T4U):
        l4(f"flow4-{i}", kA, gmac, t, syn=i % 2 == 0, pcp=i % 7)
    for i, t in enumerate(T6 + T6U):
        l4(f"flow6-{i}", kA, M[9], t, syn=i % 2 == 0, pcp=i % 7)
    for i, (cid, port, proto) in enumerate(S + SU):
        mac = gmac if cid == G else M[9]
        t = (b.g_t4(proto)[:10] if i % 3 else b.g_t6()[:34]) + struct.pack(">H", port) + bytes([proto])
        l4(f"listener-{i} {'syn' if proto == 6 else 'udp'}", kA, mac, t, syn=True, pcp=i % 7)
    l4("tcp to a client without TransportCtx", kA, noctx_mac, b.g_t4(6), syn=True)
    l4("tcp without SYN, no flow", kA, gmac, b.g_t4(6))
    # neighbour solicitations: the responder's MAC / client-info / IPv6 probes, the learner's source probe
    for i, mac in enumerate(M + MU):
        tgt = N.eui_of(mac)
        src = peer6[:15] + bytes([i + 1])
        add(f"nsol eui-ll mac{i}", kA, f_nsol(kA, tgt, src, i % 7), eui_lookups(A, tgt)[0] + [(IP6, ip6_words(A, src))])
    for i in (8, 3, 9):
        tgt = N.eui_of(M[i], ra_prefix)
        add(f"nsol eui-ra mac{i}", kA, f_nsol(kA, tgt, peer6, i % 7), eui_lookups(A, tgt)[0])
    for i, ip in enumerate(V + VU):
        add(f"nsol ip6-{i}", kC, f_nsol(kC, ip, peer6[:15] + bytes([i + 1]), i % 7),
            [(IP6, ip6_words(Cn, ip)), (IP6, ip6_words(Cn, peer6[:15] + bytes([i + 1])))])
    sol_src = [V[4], V[6], V[2], VU[0], VU[1]]  # ours through a chain; removed; never there
    for i, src in enumerate(sol_src):
        add(f"nsol from ip6 src {i}", kC, f_nsol(kC, N.eui_of(first_mac), src, i % 7),
            [(MAC, mac_words(Cn, first_mac)), (IP6, ip6_words(Cn, src))])
    # neighbour advertisements: the learner's target probes
    for i, ip in enumerate(V + VU):
        add(f"nadv ip6-{i}", kC, f_nadv(kC, ip, peer6, PEER_MAC, i % 7), [(IP6, ip6_words(Cn, ip))])
    for i, mac in enumerate(M + MU):
        tgt = N.eui_of(mac)
        add(f"nadv eui-ll mac{i}", kA, f_nadv(kA, tgt, peer6, PEER_MAC, i % 7), eui_lookups(A, tgt)[0])
    add("nadv eui-ra mac8", kA, f_nadv(kA, N.eui_of(M[8], ra_prefix), peer6, PEER_MAC), eui_lookups(A, N.eui_of(M[8], ra_prefix))[0])
    n_walk = len(frames)
    # home-bucket hits in Namespace P
    for j, (cid, mac, ip) in enumerate(pl):
        add(f"plain echo {j}", kP, f_echo4(kP, mac, ip, peer4, j), [(IP4, ip4_words(P, ip))], cid)
        add(f"plain arp {j}", kP, f_arp(kP, ip, peer4, j), [(IP4, ip4_words(P, ip))], cid)
        l4(f"plain tcp {j}", kP, mac, b.g_t4(6), pcp=j)
    plain = list(range(n_walk, len(frames)))

    # ---- traces and coverage on the final image ---------------------------------------------------------
    sc.trace = {}
    for fr in frames:
        for t, k in fr["lookups"]:
            if (t, k) not in sc.trace:
                sc.trace[(t, k)] = rx.image_probe(t, list(k))
    for i in plain:
        assert all(sc.trace[lk]["reads"] == 1 and sc.trace[lk]["value"] is not None for lk in frames[i]["lookups"][:2]), frames[i]["kind"]
    cov = {TNAME[t]: {c: [] for c in CONDITIONS} for t in WALKED}
    cov["ci"] = dict(first2=[], eui_prefix2=[])
    chain = {TNAME[t]: 0 for t in range(8)}
    for i, fr in enumerate(frames):
        for t, k in fr["lookups"]:
            p = sc.trace[(t, k)]
            chain[TNAME[t]] = max(chain[TNAME[t]], p["reads"])
            hit = p["value"] is not None
            if t == CI:
                if p["reads"] >= 2 and hit:
                    cov["ci"]["first2" if fr["kind"].startswith(("dhcpsrv", "eapol")) else "eui_prefix2"].append(i)
                continue
            got = dict(hit3=hit and p["reads"] >= 3, hit_wrap=hit and p["wrapped"], hit_tomb=hit and p["tombstones"] >= 1,
                       miss3_tomb=not hit and p["reads"] >= 3 and p["tombstones"] >= 1, miss_wrap=not hit and p["wrapped"],
                       miss_removed=not hit and (t, k) in m.removed, hit_readded=hit and (t, k) in m.readded)
            for c, yes in got.items():
                if yes and i not in cov[TNAME[t]][c]:
                    cov[TNAME[t]][c].append(i)
    missing = [f"{t}:{c}" for t, cs in cov.items() for c, fr in cs.items() if not fr]
    assert not missing, f"coverage conditions not met: {missing}"
    assert any(frames[i]["want"][1] is not None for i in cov["ci"]["eui_prefix2"]), "no IsValidPrefix hit past the home bucket"

    # ---- phase C: a client leaves from the middle of each client chain ----------------------------------
    b.phase = "C"
    b.op("client_remove", A, M[4])
    b.op("client_remove", Bn, xmac[3])
    b.op("client_remove", Cn, ymac[1])

    # ---- orders ---------------------------------------------------------------------------------------------
    walkers = list(range(n_walk))
    filler = [plain[j % len(plain)] for j in range(64)]
    grouped = walkers + filler + walkers[::-1]
    # interleaved: per table its longest hit and its longest miss alone in a wave of plain frames, at
    # lane 0 and at lane 63 in turn
    lone = []
    for t in WALKED:
        for want_hit in (True, False):
            best = max((i for i in walkers for lk in frames[i]["lookups"] if lk[0] == t and (sc.trace[lk]["value"] is not None) == want_hit),
                       key=lambda i: max(sc.trace[lk]["reads"] for lk in frames[i]["lookups"] if lk[0] == t))
            lone.append(best)
    inter = []
    for j, i in enumerate(lone):
        wave = [plain[(j + q) % len(plain)] for q in range(63)]
        inter += ([i] + wave) if j % 4 in (0, 3) else (wave + [i])
    sc.ops, sc.frames, sc.coverage, sc.chain = b.ops, frames, cov, chain
    sc.orders = dict(grouped=grouped, interleaved=inter)
    sc.lone = lone
    sc.buckets = {TNAME[t]: b.nb[t] for t in range(8)}
    assert len(inter) <= CFG["max_frames"] and len(grouped) <= CFG["max_frames"]
    return sc


def model_of(sc, phases=("A", "B")):
    m = Model()
    replay(sc.ops, m, phases)
    return m


def walk(sc, i, table):
    """emurx_image_probe's trace (after A + B) of scenario frame i's first lookup in `table`."""
    return sc.trace[next(lk for lk in sc.frames[i]["lookups"] if lk[0] == table)]


def oracles(sc):
    """The oracle after phase A and after phases A + B."""
    import pyoracle
    oa, ob = pyoracle.Oracle(), pyoracle.Oracle()
    replay(sc.ops, oa, ("A",))
    replay(sc.ops, ob, ("A", "B"))
    return oa, ob


def want_classify(sc, o, order, n=None):
    import pyoracle
    buf, desc = batch(sc, order, n)
    rec, ql, qoff, cnt = o.rx_batch(buf, desc)
    return dict(buf=buf, desc=desc, rec=rec, qlist=ql, qoff=qoff, counters=pyoracle.counters_dict(cnt),
                flows=o.flows(buf, desc, rec))


def messages(sc, order, per=64):
    idx = sc.orders[order]
    return [F.zmq_pack([sc.frames[i]["f"] for i in idx[a:a + per]], [sc.frames[i]["vport"] for i in idx[a:a + per]])
            for a in range(0, len(idx), per)]


# ---- the host-only check (tests/test_dense_tables.py) ---------------------------------------------------
def check_host():
    """Everything the GPU tests rely on, without a GPU -> one summary line."""
    from emurx.rx import RxPath
    sc = build()
    assert sc.buckets == {TNAME[t]: n for t, n in BUCKETS.items()}, sc.buckets
    rx = RxPath(-1, **CFG)
    counts = lambda: {TNAME[t]: rx.image_probe(t, [0] * 11)["buckets"] for t in (NS, CI, FT4, FT6, SRV)}  # noqa: E731
    c0 = counts()
    replay(sc.ops, rx, ("A",))
    assert counts() == c0
    replay(sc.ops, rx, ("B",))
    m = model_of(sc)
    nk = 0
    for (t, k), tr in sc.trace.items():  # every key the batch looks up
        p = rx.image_probe(t, list(k))
        assert p == tr, (TNAME[t], k, p, tr)  # a replay gives the image the builder probed
        assert p["buckets"] == BUCKETS[t] and p["home"] < p["buckets"] and 1 <= p["reads"] <= p["buckets"]
        assert p["wrapped"] == (p["home"] + p["reads"] - 1 >= p["buckets"])
        assert p["value"] == rx.image_lookup(t, list(k)) == m.keys[t].get(k), (TNAME[t], k, p)
        nk += 1
    for t in range(8):  # every live key hits, every removed key that did not come back misses
        for k, v in m.keys[t].items():
            assert rx.image_lookup(t, list(k)) == v, (TNAME[t], k)
        for tt, k in m.removed - m.readded:
            if tt == t and k not in m.keys[t] and (t in (NS, CI, FT4, FT6, SRV) or k[0] in m.ns):
                assert rx.image_lookup(t, list(k)) is None, (TNAME[t], k)
    assert counts() == c0
    for t in range(8):  # live + tombstone slots stay below the rebuild limit: no rebuild dropped the tombstones
        tombs = sum(1 for tt, k in m.removed - m.readded if tt == t)
        assert len(m.keys[t]) + tombs + 3 <= REBUILD_ABOVE[t], (TNAME[t], len(m.keys[t]), tombs)
    replay(sc.ops, rx, ("C",))
    assert counts() == c0 and rx.image_probe(MAC, [0, 1, 1])["buckets"] == BUCKETS[MAC]
    oa, ob = oracles(sc)
    for order in sc.orders:
        w = want_classify(sc, ob, order)
        want_classify(sc, oa, order)
        lk = (w["rec"]["flags"] >> 4) & 7
        for pos, i in enumerate(sc.orders[order]):  # the oracle's record names what the builder meant
            ns, cid = sc.frames[i]["want"]
            r = w["rec"][pos]
            assert r["status"] == 0, carried(sc, order, pos)
            assert (lk[pos] == abi.LK["NO_NS"]) == (ns is None) and (ns is None or r["ns_id"] == ns), carried(sc, order, pos)
            assert (lk[pos] == abi.LK["CLIENT"] and r["client_id"] == cid) if cid is not None else lk[pos] != abi.LK["CLIENT"], \
                carried(sc, order, pos)
        fl = w["flows"]
        assert order != "grouped" or all((fl == v).any() for v in (abi.FLOW_NO_CTX, abi.FLOW_NO_SYN, abi.FLOW_NO_SERVER, abi.FLOW_NEW, 150, 250, 106, 204))
    return f"ok frames={len(sc.frames)} keys={nk} chain={sc.chain} coverage=" + \
        str({t: {c: len(f) for c, f in cs.items()} for t, cs in sc.coverage.items()})


# ---- the GPU drivers (tests/test_gpu_dense_tables.py: one child process each) ---------------------------
def _open(sc, oa, stage=None, ingest_small=None):
    """A GPU handle with the scenario's tables: phase A shipped whole and one batch run, then phase
    B shipped as delta blocks."""
    import os
    from emurx.rx import RxPath
    from gpu_util import rec_diff, run_dev
    for name, v in (("EMURX_STAGE", stage), ("EMURX_INGEST_SMALL", ingest_small)):  # read by emurx_open
        os.environ.pop(name, None)
        if v is not None:
            os.environ[name] = v
    rx = RxPath(0, **CFG)
    rx.register_all()
    replay(sc.ops, rx, ("A",))
    rx.sync()
    w = want_classify(sc, oa, "grouped")
    got = run_dev(rx, w["buf"], w["desc"])[0]
    assert got.tobytes() == w["rec"].tobytes(), "phase A: " + rec_diff(got, w["rec"])
    st = rx.table_stats()
    replay(sc.ops, rx, ("B",))
    rx.sync()
    st2 = rx.table_stats()
    assert rx.image_check() == 0
    assert st2["whole_tables"] == st["whole_tables"] and st2["delta_blocks"] > st["delta_blocks"], (st, st2)
    return rx


def _same(sc, order, what, got, want):
    got, want = np.asarray(got), np.asarray(want)
    if got.shape == want.shape and got.tobytes() == want.tobytes():
        return
    if got.shape != want.shape:
        raise AssertionError(f"{what}: shape {got.shape} != {want.shape}")
    a = got.view(np.uint8).reshape(len(got), -1)
    bad = np.nonzero((a != want.view(np.uint8).reshape(len(want), -1)).any(1))[0]
    raise AssertionError(f"{what}: {len(bad)} differ; " + "; ".join(
        f"{carried(sc, order, int(p))}: got {got[p]}, want {want[p]}" for p in bad[:4]))


def _check_classify(sc, order, w, rec, ql, qoff, counters, flows=None):
    _same(sc, order, "records", rec, w["rec"])
    if flows is not None:
        _same(sc, order, "flow decisions", flows, w["flows"])
    name = order if isinstance(order, str) else order[0]
    assert np.array_equal(qoff, w["qoff"]) and np.array_equal(ql, w["qlist"]), f"queues ({name}, n={len(rec)})"
    assert counters == w["counters"], f"counters ({name}, n={len(rec)})"


def gpu_startup():
    import time
    t0 = time.time()
    import torch  # noqa: F401
    from emurx.rx import RxPath
    rx = RxPath(0, **CFG)
    rx.sync()
    rx.close()
    return f"ok startup {time.time() - t0:.2f}s"


def gpu_classify():
    import time
    t0 = time.time()
    from emurx.rx import hist_to_counters
    from gpu_util import run_dev
    import pyoracle
    import test_gpu_parity as P
    marks0 = time.time() - t0
    sc = build()
    oa, ob = oracles(sc)
    wants = {(o, n): want_classify(sc, ob, o, n) for o in sc.orders for n in SIZES}
    runs, marks = 0, [round(marks0, 2), round(time.time() - t0, 2)]
    for stage in ("tight", "narrow", "wide"):
        rx = _open(sc, oa, stage=stage)
        marks.append(round(time.time() - t0, 2))
        for (order, n), w in wants.items():
            rec, ql, qoff, hist, fl = run_dev(rx, w["buf"], w["desc"], flows=True)
            _check_classify(sc, order, w, rec, ql, qoff, hist_to_counters(hist), fl)
            runs += 1
        rx.close()
    marks.append(round(time.time() - t0, 2))
    rx = _open(sc, oa)
    for order in sc.orders:  # emurx_rx_stream, one ZMQ message per 64 frames
        for j, msg in enumerate(messages(sc, order)):
            rec, ql, qoff, cnt = rx.on_rx_stream(msg)
            orec, oq, oqoff, ocnt = ob.rx_stream(msg)
            sub = dict(rec=orec, qlist=oq, qoff=oqoff, counters=pyoracle.counters_dict(ocnt))
            part = (f"{order}, message {j}", sc.orders[order][64 * j:64 * j + 64])
            _check_classify(sc, part, sub, rec, ql, qoff, cnt.as_dict())
            runs += 1
    rx.close()
    marks.append(round(time.time() - t0, 2))
    for small in ("1", "0"):  # one ingest batch on each path
        rx = _open(sc, oa, ingest_small=small)
        for order in sc.orders:
            msgs = messages(sc, order)
            tab = P.place_messages(rx, 0, msgs, np.random.default_rng(3))
            rx.ingest_submit(0, tab)
            res = rx.ingest_wait(0)
            assert res["one_launch"] == (small == "1")
            P.check_ingest(res, ob, msgs, tab)
            runs += 1
        rx.close()
    return f"ok classify runs={runs} frames={len(sc.frames)} marks={marks} {time.time() - t0:.2f}s"


def gpu_owner_lookup():
    import time
    t0 = time.time()
    import torch
    from emurx import exchange as X
    from gpu_util import to_dev
    from test_gpu_tables import tail_cap_max
    sc = build()
    oa, ob = oracles(sc)
    src, own = _open(sc, oa), _open(sc, oa)
    runs = 0
    for order in sc.orders:
        for n in SIZES:
            w = want_classify(sc, ob, order, n)
            n = len(w["desc"])
            cap, tcap = n, tail_cap_max(n)
            rb = abi.lookup_region_bytes(cap, tcap)
            buf, desc = to_dev(w["buf"]), to_dev(w["desc"])
            qcap = max(abi.queue_cap(n), abi.QUEUE_TILE)
            ql = torch.empty(abi.NUM_QUEUES * qcap, dtype=torch.int32, device="cuda")
            tc = torch.empty(max(abi.ntiles(n), 1) * 16, dtype=torch.int32, device="cuda")
            hi = torch.zeros(abi.HIST_SHARDS * 2 * abi.HIST_BINS, dtype=torch.int64, device="cuda")
            sd = torch.full((rb,), 0xEE, dtype=torch.uint8, device="cuda")
            scnt = torch.full((2,), -1, dtype=torch.int32, device="cuda")
            src.parse_route_dev(buf, desc, n, None, ql, qcap, tc, hi, 1, 0, cap, sd, scnt, tail_cap=tcap)
            out = torch.full((cap * X.REC_BYTES,), 0xEE, dtype=torch.uint8, device="cuda")
            flow = torch.full((cap,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
            own.lookup_dev(sd, scnt, 1, cap, out, flow, tail_cap=tcap)
            torch.cuda.synchronize()
            assert scnt.cpu().numpy().tolist() == [n, 0], scnt
            got = out.cpu().numpy().view(abi.ROUTE_REC_DTYPE)[:n]
            _same(sc, order, "owner records", np.ascontiguousarray(got["rec"]), w["rec"])
            _same(sc, order, "owner flow decisions", flow.cpu().numpy().view(np.uint32)[:n], w["flows"])
            runs += 1
    src.close()
    own.close()
    return f"ok owner runs={runs} {time.time() - t0:.2f}s"


def _classified(sc, rx, ob, order):
    from test_gpu_respond import classify
    w = want_classify(sc, ob, order)
    tb, td, trec, rec = classify(rx, w["buf"], w["desc"])
    _same(sc, order, "records", rec, w["rec"])
    return w, tb, td, trec, rec


def gpu_respond():
    import time
    t0 = time.time()
    from test_gpu_respond import check
    from test_gpu_respond_nd import respond
    sc = build()
    oa, ob = oracles(sc)
    rx = _open(sc, oa)
    e4, e6 = model_of(sc).envs()
    e4c, e6c = model_of(sc, PHASES).envs()
    runs = 0
    kind = lambda i: sc.frames[i]["kind"]  # noqa: E731
    for order in sc.orders:
        w, tb, td, trec, rec = _classified(sc, rx, ob, order)
        idx = sc.orders[order]
        full = N.respond_batch(w["buf"], w["desc"], rec, abi.RSPK_ALL, e4, e6)
        oc = {i: int(full[0][p]) for p, i in enumerate(idx)}
        # the three probes of the responder each meet a long hit, a wrapped hit and a miss past tombstones
        for table, prefix, yes, no in ((IP4, "ip4-", abi.RSP_ARP, None), (MAC, "nsol eui-", abi.RSP_ND, abi.RSP_NONE),
                                       (IP6, "nsol ip6-", abi.RSP_ND, abi.RSP_NONE)):
            mine = [i for i in oc if kind(i).startswith(prefix) and (table != IP4 or "arp" in kind(i))]
            if order == "grouped":
                assert any(walk(sc, i, table)["reads"] >= 3 and oc[i] == yes for i in mine), (prefix, "long hit")
                assert any(walk(sc, i, table)["wrapped"] and oc[i] == yes for i in mine), (prefix, "wrapped hit")
                if no is not None:
                    assert any(walk(sc, i, table)["value"] is None and walk(sc, i, table)["reads"] >= 3 and
                               walk(sc, i, table)["tombstones"] and oc[i] == no for i in mine), (prefix, "miss past tombstones")
        for n in SIZES:
            n = len(idx) if n is None else n
            want = N.respond_batch(w["buf"], w["desc"][:n], rec[:n], abi.RSPK_ALL, e4, e6)
            cap = int(want[4][1])
            check(respond(rx, tb, td, trec, n, cap, abi.RSPK_ALL), want, n, cap)
            runs += 1
        if order == "grouped":
            keep = (w, tb, td, trec, rec, full, idx)
    # a client leaves from the middle of each chain: the frames behind it still answer, and the ARP
    # re-probe of the one that left walks past its tombstone to a miss
    replay(sc.ops, rx, ("C",))
    rx.sync()
    assert rx.image_check() == 0
    w, tb, td, trec, rec, full, idx = keep
    want = N.respond_batch(w["buf"], w["desc"], rec, abi.RSPK_ALL, e4c, e6c)
    lost = {kind(i) for p, i in enumerate(idx) if full[0][p] != want[0][p]}
    assert {"ip4-3 arp request", "nsol eui-ll mac4", "nsol ip6-3"} <= lost, lost
    still = {kind(i) for p, i in enumerate(idx) if want[0][p] in (abi.RSP_ARP, abi.RSP_ND)}
    assert {"ip4-4 arp request", "ip4-6 arp request", "nsol eui-ll mac6", "nsol eui-ll mac9", "nsol ip6-4", "nsol ip6-5"} <= still, still
    gone = next(i for i in idx if kind(i) == "ip4-3 arp request")
    p = rx.image_probe(*next(lk for lk in sc.frames[gone]["lookups"] if lk[0] == IP4))
    assert p["value"] is None and p["reads"] >= 3 and p["tombstones"] >= 1, p
    cap = int(want[4][1])
    check(respond(rx, tb, td, trec, len(idx), cap, abi.RSPK_ALL), want, len(idx), cap)
    rx.close()
    return f"ok respond runs={runs + 1} {time.time() - t0:.2f}s"


def gpu_learn():
    import time
    t0 = time.time()
    from test_gpu_learn import check, learn
    sc = build()
    oa, ob = oracles(sc)
    rx = _open(sc, oa)
    e6 = model_of(sc).envs()[1]
    runs = 0
    for order in sc.orders:
        w, tb, td, trec, rec = _classified(sc, rx, ob, order)
        idx = sc.orders[order]
        if order == "grouped":
            # the two "the table already holds this address" probes: a hit and a miss through a chain each
            br = {sc.frames[i]["kind"]: L.learn_branch(sc.frames[i]["f"], rec[p], e6) for p, i in enumerate(idx)}
            deep = lambda k: walk(sc, next(i for i in idx if sc.frames[i]["kind"] == k), IP6)  # noqa: E731
            assert br["nsol from ip6 src 0"] == "ns-src-ours" and deep("nsol from ip6 src 0")["reads"] >= 3
            assert br["nsol from ip6 src 3"] == "ns-learn" and deep("nsol from ip6 src 3")["reads"] >= 3
            assert br["nsol from ip6 src 2"] == "ns-learn"  # the address was there and was removed
            assert br["nadv ip6-4"] == "na-ip6-ours" and deep("nadv ip6-4")["reads"] >= 3
            assert br["nadv ip6-7"] == "na-learn-ip6" and deep("nadv ip6-7")["reads"] >= 3
            assert br["nadv ip6-2"] == "na-learn-ip6"
            assert br["nadv eui-ll mac9"] == "na-eui-ours" and br["nadv eui-ll mac11"] == "na-learn-eui"
            assert br["nadv eui-ra mac8"] == "na-eui-ours"
        for n in SIZES:
            n = len(idx) if n is None else n
            want = L.learn_batch(w["buf"], w["desc"][:n], rec[:n], abi.LRNK_ALL, e6)
            ev_cap = min(rx.learn_max_events(), max(n, 1))
            assert int(want[2][2]) == 0
            check(learn(rx, tb, td, trec, n, ev_cap), want)
            runs += 1
    rx.close()
    return f"ok learn runs={runs} {time.time() - t0:.2f}s"

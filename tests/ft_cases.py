"""Tables and TCP / UDP frames for the tests of emurx_ftstat_dev and the ingest flow stage: every
branch of the rule in include/emu_rx.h, both families and both protocols.  TEST INFRASTRUCTURE ONLY.

Namespaces (vport 1): 0 untagged, 1 tag 0x8100/5, 2 tag 0x8100/6 without the transport plugin; tag
0x8100/99 is no Namespace.  N_CLIENTS clients in Namespace 0 (client i: MAC 00:00:02:00:hi:lo) and
eight in Namespace 1 (ids N_CLIENTS ..).  A client whose id is 5 mod 8 has no TransportCtx, one
whose id is 6 mod 8 no transport plugin; every other client listens on tcp :80 and udp :53."""
import struct

import numpy as np

from emurx import abi
from emurx import frames as F

N_CLIENTS = 1000
MAX_NS, MAX_CLIENTS = 8, 1024
DUT = bytes([0x00, 0x10, 0x94, 0, 0, 2])
TAGS = {0: (), 1: ((0x8100, 5),), 2: ((0x8100, 6),), 99: ((0x8100, 99),)}
TRANSPORT = 1 << abi.PLUG_NAMES.index("transport")
TCP_PORT, UDP_PORT = 80, 53
SYN, ACK = 0x02, 0x10


def ns_key(ns):
    v = [(t << 16) | vid for t, vid in TAGS[ns]] + [0, 0]
    return F.tunnel_key(1, v[0], v[1])


def client(cid):
    """-> (ns, mac, ipv4, ipv6)"""
    ns = 0 if cid < N_CLIENTS else 1
    return (ns, bytes([0, 0, 2, ns, cid >> 8, cid & 255]), bytes([16, ns, cid >> 8, cid & 255]),
            bytes([0x20, 1, 0x0D, 0xB8, 0, ns] + [0] * 8 + [cid >> 8, cid & 255]))


def has_ctx(cid):
    return cid % 8 not in (5, 6)


def load_tables(t):
    """The Namespaces, clients, TransportCtx marks and listeners into an RxPath or an Oracle."""
    for ns in (0, 1, 2):
        assert t.ns_add(ns_key(ns), ns, abi.PLUG_ALL & ~TRANSPORT if ns == 2 else abi.PLUG_ALL) == 0
    for cid in range(N_CLIENTS + 8):
        ns, mac, ip4, ip6 = client(cid)
        assert t.client_add(ns, cid, mac, ip4, ip6, None, abi.PLUG_ALL & ~TRANSPORT if cid % 8 == 6 else abi.PLUG_ALL) == 0
        if has_ctx(cid):
            assert t.client_set_transport(cid, 1) == 0
            assert t.server_add(cid, TCP_PORT, 6) == 0 and t.server_add(cid, UDP_PORT, 17) == 0
    # a client of the Namespace without the plugin (its frames never reach it: NS_NO_PLUGIN)
    assert t.client_add(2, N_CLIENTS + 8, bytes([0, 0, 2, 2, 0, 1]), bytes([16, 2, 0, 1]), None, None, abi.PLUG_ALL) == 0


def l4(cid, proto=6, v6=False, dport=None, flags=ACK, sport=1025, ns=None, mac=None, size=0):
    """A tcp (proto 6) or udp (17) frame to client cid; ns / mac override where it is sent."""
    cns, cmac, ip4, ip6 = client(cid)
    ns = cns if ns is None else ns
    dport = (TCP_PORT if proto == 6 else UDP_PORT) if dport is None else dport
    body = bytes((cid + k) & 255 for k in range(size))
    if v6:
        src = bytes([0x20, 1, 0x0D, 0xB8] + [0] * 10 + [0x30, 7])
        ps = F.ipv6_pseudo(src, ip6, (20 if proto == 6 else 8) + len(body), proto)
    else:
        src = bytes([48, 0, 0, 7])
        ps = F.ipv4_pseudo(src, ip4, proto, (20 if proto == 6 else 8) + len(body))
    seg = F.tcp(sport, dport, body, flags=flags, pseudo=ps) if proto == 6 else F.udp(sport, dport, body, csum="auto", pseudo=ps)
    ip = F.ipv6(src, ip6, proto, seg) if v6 else F.ipv4(src, ip4, proto, seg)
    tg = b"".join(struct.pack(">HH", tpid, vid) for tpid, vid in TAGS[ns])
    f = (cmac if mac is None else mac) + DUT + tg + struct.pack(">H", 0x86DD if v6 else 0x0800) + ip
    return f + bytes(max(60 - len(f), 0))


def tuple_of(f, ns=0):
    """The c5tuplekey of a frame built by l4 (client_ctx.go:720-765)."""
    l3 = 14 + 4 * len(TAGS[ns])
    if f[l3] >> 4 == 6:
        return f[l3 + 8:l3 + 40] + f[l3 + 40:l3 + 44] + bytes([f[l3 + 6]])
    return f[l3 + 12:l3 + 20] + f[l3 + 20:l3 + 24] + bytes([f[l3 + 9]])


def arp(cid):
    _, mac, ip4, _ = client(cid)
    f = b"\xff" * 6 + DUT + struct.pack(">H", 0x0806) + F.arp(1, DUT, bytes([48, 0, 0, 7]), bytes(6), ip4)
    return f + bytes(60 - len(f))


# one frame per branch of the rule x {tcp, udp} x {IPv4, IPv6}: (name, frame, outcome & 7)
def matrix():
    out = []
    for v6 in (False, True):
        fam = "v6" if v6 else "v4"
        out += [
            (f"tcp-no-syn-{fam}", l4(1, 6, v6, flags=ACK), abi.FT_NO_SYN),
            (f"tcp-synack-no-flow-{fam}", l4(2, 6, v6, flags=SYN | ACK), abi.FT_NO_SYN),
            (f"tcp-no-server-{fam}", l4(1, 6, v6, dport=81, flags=SYN), abi.FT_NO_SRV_TCP),
            (f"udp-no-server-{fam}", l4(3, 17, v6, dport=54), abi.FT_NO_SRV_UDP),
            (f"tcp-new-{fam}", l4(1, 6, v6, flags=SYN), abi.FT_NONE),
            (f"udp-new-{fam}", l4(1, 17, v6), abi.FT_NONE),
            (f"tcp-flow-{fam}", l4(4, 6, v6, sport=FLOW_SPORT), abi.FT_NONE),
            (f"udp-flow-{fam}", l4(4, 17, v6, sport=FLOW_SPORT), abi.FT_NONE),
            (f"tcp-no-ctx-{fam}", l4(5, 6, v6), abi.FT_ERR),
            (f"udp-no-ctx-{fam}", l4(13, 17, v6), abi.FT_ERR),
            (f"tcp-client-no-plugin-{fam}", l4(6, 6, v6), abi.FT_ERR),
            (f"udp-no-client-{fam}", l4(1, 17, v6, mac=bytes([0, 0, 2, 0, 0xEE, 0xEE])), abi.FT_ERR),
            (f"tcp-no-ns-{fam}", l4(1, 6, v6, ns=99), abi.FT_ERR),
            (f"udp-ns-no-plugin-{fam}", l4(1, 17, v6, ns=2, mac=bytes([0, 0, 2, 2, 0, 1])), abi.FT_ERR),
            (f"tcp-ns1-{fam}", l4(N_CLIENTS + 1, 6, v6, flags=ACK), abi.FT_NO_SYN),
        ]
    out.append(("arp", arp(1), abi.FT_NONE))
    return out


FLOW_SPORT = 4000
FLOW_CLIENTS = (4, 12)


def flow_keys():
    """(cid, tuple, flow id) of the established flows: clients 4 and 12, both protocols and families."""
    out = []
    for cid in FLOW_CLIENTS:
        for proto in (6, 17):
            for v6 in (False, True):
                out.append((cid, tuple_of(l4(cid, proto, v6, sport=FLOW_SPORT)), 1000 + len(out)))
    return out


def load_flows(t):
    for cid, tup, fid in flow_keys():
        assert t.flow_add(cid, tup, fid) == 0


def stream(n, seed=11):
    """n frames cycling through the matrix's kinds with seeded clients: all five outcomes, flows
    found and NEW in between, other protocols."""
    rng = np.random.default_rng([seed, 0x6674])
    ok = [c for c in range(64) if has_ctx(c) and c not in FLOW_CLIENTS]
    out = []
    for i in range(n):
        k, v6 = i % 13, bool((i // 13) & 1)
        c = int(rng.choice(ok[:6] if i % 3 else ok))
        if k == 0:
            f = l4(c, 6, v6, flags=ACK, size=int(rng.integers(0, 40)))
        elif k == 1:
            f = l4(c, 6, v6, dport=81, flags=SYN)
        elif k == 2:
            f = l4(c, 17, v6, dport=54, size=int(rng.integers(0, 300)))
        elif k == 3:
            f = l4(c, 6, v6, flags=SYN)
        elif k == 4:
            f = l4(FLOW_CLIENTS[i & 1], 6 if i & 2 else 17, v6, sport=FLOW_SPORT, size=9)
        elif k == 5:
            f = l4(5 + 8 * int(rng.integers(0, 3)), 6 if i & 1 else 17, v6)
        elif k == 6:
            f = l4(6, 17, v6)
        elif k == 7:
            f = l4(c, 6, v6, ns=99)
        elif k == 8:
            f = arp(c)
        elif k == 9:
            f = l4(c, 17, v6)
        elif k == 10:
            f = l4(N_CLIENTS + 1 + (i & 2), 6, v6, flags=ACK | 0x01)
        elif k == 11:
            f = l4(c, 17, v6, mac=bytes([0, 0, 2, 0, 0xEE, c]))
        else:
            f = l4(c, 6, v6, flags=0x04)
        out.append(f)
    return out


def one_client(n, cid=9):
    """n refused frames of one client, the kinds and families mixed."""
    return [l4(cid, 17, bool(i & 4), dport=54) if i % 3 == 2 else l4(cid, 6, bool(i & 4), dport=81 if i % 3 else None,
                                                                      flags=SYN if i % 3 else ACK) for i in range(n)]


def interleaved(n, k):
    """k clients taking turns frame by frame."""
    cids = (9, 10, 11)[:k]
    return [l4(cids[i % k], 6, bool(i & 8), flags=ACK) if i % 5 else l4(cids[i % k], 17, False, dport=54) for i in range(n)]


def near_clients():
    """Client ids that differ in one bit, three frames each."""
    cids = [8, 9, 8 ^ 2, 8 ^ 16, 8 ^ 64, 8 ^ 512]
    return [l4(c, 6, bool(r & 1), flags=ACK) for r in range(3) for c in cids], cids


def distinct(n, first=0):
    """One refused frame for each of n distinct clients with a TransportCtx."""
    cids = [c for c in range(first, N_CLIENTS) if has_ctx(c) and c not in FLOW_CLIENTS][:n]
    assert len(cids) == n
    return [l4(c, 6 if c & 1 else 17, bool(c & 2), dport=99, flags=SYN) for c in cids]

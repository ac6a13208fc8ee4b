"""The tables and the batches of the ping tests: what tests/test_ping_ref.py classifies with the
oracle and tests/test_gpu_ping.py with emurx_classify_dev."""
import json
from pathlib import Path

import numpy as np

import ping_ref as P
from emurx import abi, frames as F

FIXTURE = json.loads((Path(__file__).resolve().parent / "golden" / "ping_fixture.json").read_text())

NOW = 1_700_000_000_123_456_789  # a time.Now().UnixNano(), below 2^63
TIMEOUT = abi.PING_TIMEOUT_NS
TAGS = [((0x8100, 1), (0x8100, 2)), ((0x8100, 7),)]  # the Namespaces' tags (vport 1)
N_CLIENTS = 6  # per Namespace; client 4 has no icmp plugin, client 5 no ipv6 plugin
REMOTE4, REMOTE6 = bytes([48, 0, 0, 1]), bytes([0x20, 1, 0x0D, 0xB8, 0xFF] + [0] * 10 + [9])


def _vlans(tags):
    v = [(t << 16) | vid for t, vid in tags] + [0, 0]
    return v[0], v[1]


def client(ns: int, c: int):
    """-> client id, MAC, IPv4, IPv6, plugin mask"""
    mask = abi.PLUG_ALL
    if c == 4:
        mask &= ~(1 << abi.PLUG_NAMES.index("icmp"))
    if c == 5:
        mask &= ~(1 << abi.PLUG_NAMES.index("ipv6"))
    return (ns * N_CLIENTS + c, bytes([0, 0, 1, ns, 0, c + 1]), bytes([16, ns, 0, c + 1]),
            bytes([0x20, 1, 0x0D, 0xB8, 0, ns] + [0] * 9 + [c + 1]), mask)


def load_tables(target, env: P.Env | None = None):
    """Two Namespaces with N_CLIENTS clients each into an Oracle / RxPath (and the Env twin)."""
    for ns, tags in enumerate(TAGS):
        v0, v1 = _vlans(tags)
        assert target.ns_add(F.tunnel_key(1, v0, v1), ns, abi.PLUG_ALL) == 0
        for c in range(N_CLIENTS):
            cid, mac, ip4, ip6, mask = client(ns, c)
            assert target.client_add(ns, cid, mac, ip4, ip6, None, mask) == 0
            if env is not None:
                env.add(1, v0, v1, mac, cid, mask)


def sim_env(name: str) -> P.Env:
    """The Env twin of tests/sim_envs.py load_env(name): one client, id 0, with the one plugin."""
    import sim_envs as S
    e = S.ENVS[name]
    env = P.Env()
    env.add(1, 0x81000001, 0x81000002, e["mac"], 0, 1 << S.PLUG.index(e["plugin"]))
    return env


def fixture_frames(capture: str):
    return [bytes.fromhex(h) for h in FIXTURE[capture]["rx"]]


# ---- frames to the clients above ---------------------------------------------------------
def r4(ns, c, ident, seq, ts, **kw):
    _, mac, ip4, _, _ = client(ns, c)
    return P.v4_reply(kw.pop("dst_mac", mac), kw.pop("src", REMOTE4), kw.pop("dst", ip4), ident, seq, ts, tags=TAGS[ns], **kw)


def u4(ns, c, ident, **kw):
    _, mac, ip4, _, _ = client(ns, c)
    return P.v4_unreach(mac, kw.pop("src", REMOTE4), ip4, ident, tags=TAGS[ns], **kw)


def r6(ns, c, ident, seq, ts, **kw):
    _, mac, _, ip6, _ = client(ns, c)
    return P.v6_reply(kw.pop("dst_mac", mac), REMOTE6, ip6, ident, seq, ts, tags=TAGS[ns], **kw)


def u6(ns, c, ident, **kw):
    _, mac, _, ip6, _ = client(ns, c)
    return P.v6_unreach(kw.pop("dst_mac", mac), REMOTE6, ip6, ident, tags=TAGS[ns], **kw)


def arp_request(ns=0):
    return P.eth(b"\xff" * 6, bytes([0, 0, 0, 2, 0, 0]), TAGS[ns], 0x0806) + bytes([0, 1, 8, 0, 6, 4, 0, 1]) + \
        bytes([0, 0, 0, 2, 0, 0]) + REMOTE4 + bytes(6) + bytes([16, ns, 0, 1])


def matrix():
    """One frame per branch of the rule: [(name, frame, expected outcome, expected class or None)]."""
    ok = NOW - 1000
    m = [
        # ---- ICMPv4
        ("v4-ok", r4(0, 0, 0x1234, 1, ok), abi.PNG_REPLY, P.CLS_OK),
        ("v4-magic", r4(0, 0, 0x1234, 2, ok, magic=abi.PING_MAGIC ^ 1), abi.PNG_REPLY, P.CLS_MALFORMED),
        ("v4-ts-now", r4(0, 0, 0x1234, 3, NOW), abi.PNG_REPLY, P.CLS_OK),
        ("v4-ts-5s", r4(0, 0, 0x1234, 4, NOW - TIMEOUT), abi.PNG_REPLY, P.CLS_OK),
        ("v4-ts-5s-1", r4(0, 0, 0x1234, 5, NOW - TIMEOUT - 1), abi.PNG_REPLY, P.CLS_BAD_LATENCY),
        ("v4-ts-future", r4(0, 0, 0x1234, 6, NOW + 1), abi.PNG_REPLY, P.CLS_BAD_LATENCY),
        ("v4-ts-2^63", r4(0, 0, 0x1234, 7, 1 << 63), abi.PNG_REPLY, P.CLS_BAD_LATENCY),
        ("v4-ts-2^64-1", r4(0, 0, 0x1234, 8, (1 << 64) - 1), abi.PNG_REPLY, P.CLS_BAD_LATENCY),
        ("v4-payload-16", r4(0, 0, 0x1234, 9, ok, extra=0), abi.PNG_REPLY, P.CLS_OK),
        ("v4-payload-15", r4(0, 0, 0x1234, 10, ok, cut=19), abi.PNG_HOST, None),
        ("v4-payload-0", r4(0, 0, 0x1234, 11, ok, cut=4), abi.PNG_HOST, None),
        ("v4-ihl-6", r4(0, 0, 0x1234, 12, ok, ihl=6), abi.PNG_HOST, None),
        ("v4-src-mcast", r4(0, 0, 0x1234, 13, ok, src=bytes([224, 0, 0, 1])), abi.PNG_MCAST, None),
        ("v4-src-zero", r4(0, 0, 0x1234, 14, ok, src=bytes(4)), abi.PNG_MCAST, None),
        ("v4-src-linklocal", u4(0, 0, 0x1234, src=bytes([169, 254, 1, 1])), abi.PNG_MCAST, None),
        ("v4-src-loopback", r4(0, 0, 0x1234, 15, ok, src=bytes([127, 0, 0, 1])), abi.PNG_REPLY, P.CLS_OK),
        ("v4-no-plugin", r4(0, 4, 0x1234, 16, ok), abi.PNG_NO_CLIENT, None),
        ("v4-no-plugin-unreach", u4(0, 4, 0x1234), abi.PNG_NO_CLIENT, None),
        ("v4-no-client", r4(0, 0, 0x1234, 17, ok, dst=bytes([16, 0, 0, 99])), abi.PNG_NONE, None),
        ("v4-not-to-me", r4(0, 0, 0x1234, 18, ok, dst_mac=bytes([0, 0, 1, 0, 0, 77])), abi.PNG_NONE, None),
        ("v4-echo-request", P.v4(client(0, 0)[1], REMOTE4, client(0, 0)[2], bytes([8, 0, 0, 0]) + P.echo_body(1, 1, ok), TAGS[0]),
         abi.PNG_NONE, None),
        ("v4-reply-code-1", P.v4(client(0, 0)[1], REMOTE4, client(0, 0)[2], bytes([0, 1, 0, 0]) + P.echo_body(1, 1, ok), TAGS[0]),
         abi.PNG_NONE, None),
        ("v4-unknown-ns", P.v4_reply(client(0, 0)[1], REMOTE4, client(0, 0)[2], 1, 1, ok, tags=((0x8100, 99),)), abi.PNG_NONE, None),
        ("arp", arp_request(), abi.PNG_NONE, None),
    ]
    m += [(f"v4-unreach-{c}", u4(1, 1, 0x2000 + c, code=c), abi.PNG_UNREACH if c <= 4 else abi.PNG_NONE, None) for c in range(6)]
    m += [("v4-unreach-35", u4(1, 1, 0x2000, cut=35), abi.PNG_HOST, None),
          ("v4-unreach-36", u4(1, 1, 0x2000, cut=36), abi.PNG_UNREACH, None)]
    m += [
        # ---- ICMPv6
        ("v6-ok", r6(0, 0, 0x1234, 1, ok), abi.PNG_REPLY, P.CLS_OK),
        ("v6-magic", r6(0, 0, 0x1234, 2, ok, magic=0), abi.PNG_REPLY, P.CLS_MALFORMED),
        ("v6-ts-now", r6(0, 0, 0x1234, 3, NOW), abi.PNG_REPLY, P.CLS_OK),
        ("v6-ts-5s-1", r6(0, 0, 0x1234, 4, NOW - TIMEOUT - 1), abi.PNG_REPLY, P.CLS_BAD_LATENCY),
        ("v6-ts-2^63", r6(0, 0, 0x1234, 5, 1 << 63), abi.PNG_REPLY, P.CLS_BAD_LATENCY),
        ("v6-len-23", r6(0, 0, 0x1234, 6, ok, cut=19), abi.PNG_HOST, None),
        ("v6-reply-code-1", r6(0, 0, 0x1234, 7, ok, code=1), abi.PNG_NONE, None),
        ("v6-no-client", r6(0, 0, 0x1234, 8, ok, dst_mac=bytes([0, 0, 1, 0, 0, 77])), abi.PNG_NO_CLIENT, None),
        ("v6-zero-mac", r6(0, 0, 0x1234, 9, ok, dst_mac=bytes(6)), abi.PNG_NO_CLIENT, None),
        ("v6-no-plugin", r6(0, 5, 0x1234, 10, ok), abi.PNG_NO_CLIENT, None),
        ("v6-no-plugin-unreach", u6(0, 5, 0x1234), abi.PNG_NO_CLIENT, None),
        ("v6-echo-request", P.v6(client(0, 0)[1], REMOTE6, client(0, 0)[3], bytes([128, 0, 0, 0]) + P.echo_body(1, 1, ok), TAGS[0]),
         abi.PNG_NONE, None),
    ]
    m += [(f"v6-unreach-{c}", u6(1, 2, 0x3000 + c, code=c), abi.PNG_UNREACH if c <= 6 else abi.PNG_NONE, None) for c in range(8)]
    m += [("v6-unreach-71", u6(1, 2, 0x3000, cut=71), abi.PNG_HOST, None)]
    return m


def stream(n: int, seed: int = 11):
    """A seeded stream of n frames over a few pings: runs of in-order replies with jumps, repeats
    and wraps of the sequence number, every class of timestamp (zero latencies included), both
    families, unreachables, Namespace-level outcomes and frames that are not the fold's."""
    rng = np.random.default_rng(seed)
    pings = [(0, 0, 4, 0x1234), (0, 0, 6, 0x1234), (0, 1, 4, 0x1234), (1, 2, 6, 0x1234), (0, 0, 4, 0x4321), (1, 3, 4, 0x1234)]
    seq = {p: int(rng.integers(0xFFF0, 0x10000)) for p in pings}
    out = []
    for _ in range(n):
        k = int(rng.integers(0, 20))
        ns, c, fam, ident = pings[int(rng.integers(0, len(pings)))]
        key = (ns, c, fam, ident)
        if k < 12:  # a reply
            j = int(rng.integers(0, 10))
            if j == 0:
                seq[key] = int(rng.integers(0, 0x10000))  # a jump
            elif j != 1:  # j == 1: the same number again
                seq[key] = (seq[key] + 1) & 0xFFFF
            t = int(rng.integers(0, 12))
            ts = (NOW if t < 2 else NOW - TIMEOUT - 1 if t == 2 else NOW + 5 if t == 3 else
                  NOW - int(rng.integers(1, 2_000_000_000)))
            magic = abi.PING_MAGIC if rng.integers(0, 12) else 0x1122334455667788
            out.append((r4 if fam == 4 else r6)(ns, c, ident, seq[key], ts, magic=magic))
        elif k < 14:
            out.append((u4 if fam == 4 else u6)(ns, c, ident))
        elif k == 14:
            out.append(r4(ns, 4, ident, 1, NOW) if fam == 4 else r6(ns, 5, ident, 1, NOW))  # NO_CLIENT
        elif k == 15:
            out.append(r4(ns, c, ident, 1, NOW, src=bytes([224, 0, 0, 5])))  # MCAST
        elif k == 16:
            out.append(r4(ns, c, ident, 1, NOW, cut=10) if fam == 4 else r6(ns, c, ident, 1, NOW, cut=12))  # HOST
        elif k == 17:
            out.append(arp_request(ns))
        elif k == 18:
            out.append(r4(ns, c, ident, 1, NOW, dst=bytes([16, ns, 0, 200])))  # v4 NO_CLIENT: NONE
        else:
            out.append(bytes(rng.integers(0, 256, int(rng.integers(10, 60)), dtype=np.uint8)))  # no parse
    return out


def one_key(n: int, first_seq: int = 0xFFF0):
    """n accepted replies of one ping, sequence numbers first_seq, first_seq + 1, ... (across the
    wrap): n_succ = n - 1, and any other order of the frames gives less.  Latencies differ, one is 0."""
    return [r4(0, 0, 0x1234, (first_seq + i) & 0xFFFF, NOW - (0 if i == n // 3 else 1000 + 7 * i)) for i in range(n)]


def interleaved(n: int, k: int):
    """k pings lane by lane: frame i belongs to ping i % k; ping j skips a number every j + 2 frames."""
    pings = [(0, 0, 4), (0, 1, 6), (1, 2, 4)][:k]
    out = []
    for i in range(n):
        ns, c, fam = pings[i % k]
        t = i // k
        s = (0xFF00 + t + t // (i % k + 2)) & 0xFFFF
        ts = NOW - (0 if t % 97 == 5 else 500 + (i * 37) % 1000)
        out.append((r4 if fam == 4 else r6)(ns, c, 0x1234, s, ts))
    return out


def near_keys():
    """Keys that differ only in ident, only in family, only in client: six pings, three frames each."""
    fr = []
    for rep in range(3):
        fr += [r4(0, 0, 0x1234, rep, NOW - 100), r4(0, 0, 0x1235, rep, NOW - 100), r6(0, 0, 0x1234, rep, NOW - 100),
               r4(0, 1, 0x1234, rep, NOW - 100), r6(0, 1, 0x1234, rep, NOW - 100), u4(0, 0, 0x1236)]
    return fr


def distinct_keys(n: int):
    """n frames, n keys: the identifier counts up."""
    return [(r4 if i % 2 else r6)(i % 2, i % 4, 0x100 + i, i, NOW - 1 - i) for i in range(n)]


def stale_marks():
    """Three batches of 1,024 frames for one handle, one after the other: replies of one ping fill
    the second tile; then that tile holds no candidate while the first and third tiles of the same
    step of the ordered pass hold four accepted replies of another ping; then the first batch
    again.  What the first call left in the second tile's per-frame words must not reach the second
    call, and nothing of the second may reach the third."""
    arp = [arp_request(i % 2) for i in range(1024)]
    b1 = arp[:256] + one_key(256) + arp[512:]
    b2 = list(arp)
    for j, i in enumerate((10, 20, 600, 700)):
        b2[i] = r4(0, 1, 0x1234, 0x100 + j, NOW - 50 - j)
    return b1, b2, list(b1)

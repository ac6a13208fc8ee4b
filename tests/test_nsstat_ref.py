"""The per-Namespace counter rule of emurx_nsstat_dev against the counters the reference's own
captures recorded, its branches on hand-built frames, and the C-ABI of the call (no GPU).

nsstat_ref (tests/nsstat_ref.py) applied to the rx frames of a capture, with records from the
oracle, the environment of the capture's Go test (tests/sim_envs.py) and the outcomes of
respond_ref / nd_ref and learn_ref, must give every frame done 1 and, replayed as INTEGRATION.md
says, exactly the handler counters the capture's Go test dumped
(tests/golden/nsstat_counters.json, extracted by tests/golden/make_nsstat_counters.py).

ipv6nd_2 and ipv6nd_3 recorded no ND counters: they are pinned to the reply counts test_nd_ref.py
pins (six unicast advertisements, six duplicate-address-detection answers).  The other ND counters
(pktRxNeighborAdvertisement, pktRxNeighborAdvLearn) and the error counters (pktRxErrNoBroadcast,
pktRxErrWrongOp, pktRxNoClientUnhandled, pktRxErrMulticastB, pktRxErrUnhandled) are recorded by no
capture: they rest on the Go lines nsstat_ref cites alone, exercised here on hand-built frames."""
import ctypes as C
import json
from pathlib import Path

import numpy as np
import pytest

import learn_ref as L
import nd_ref as N
import nsstat_ref as NS
import respond_ref as R
import sim_envs as S
from emurx import abi, frames as F
from test_oracle_corpus import GOLD

COUNTERS = json.loads((Path(__file__).parent / "golden" / "nsstat_counters.json").read_text())
# the client's own transmissions (its gateway resolution, its gratuitous ARP): no rx handler counts them
NOT_A_HANDLER_COUNTER = {"pktTxArpQuery", "pktTxGArp"}

# capture, environment, frames, the counter words and their values
CAPTURES = [
    ("arp4.json", "arp", 6, {abi.NSC_ARP_QUERY: 6, abi.NSC_ARP_TX_REPLY: 6}),
    ("arp5.json", "arp", 6, {abi.NSC_ARP_QUERY: 6, abi.NSC_ARP_QUERY_NOT_FOR_US: 6}),
    ("arp2.json", "arp", 57, {abi.NSC_ARP_REPLY: 57}),
    ("icmp1.json", "icmp", 6, {abi.NSC_ICMP_ECHO: 6}),
    ("icmpv6_1.json", "ipv6", 6, {abi.NSC_V6_ECHO: 6}),
    ("icmpv6_2.json", "ipv6", 6, {abi.NSC_V6_ECHO: 6}),
    ("ipv6nd_2.json", "ipv6", 6, {abi.NSC_ND_RX_NS: 6, abi.NSC_ND_TX_ADV_UNICAST: 6}),
    ("ipv6nd_3.json", "ipv6", 6, {abi.NSC_ND_RX_NS: 6, abi.NSC_ND_TX_DAD_ERROR: 6}),
]


def sim_envs(name):
    """The capture's environment as respond_ref's and nd_ref's lookups."""
    e = S.ENVS[name]
    env4, env6 = R.Env(), N.Env()
    env4.add(e.get("key", S.NS_KEY), 0, e["mac"], e["ipv4"])
    env6.add(e.get("key", S.NS_KEY), 0, e["mac"], e["ipv6"], None, 1 << S.PLUG.index(e["plugin"]))
    return env4, env6


def capture_case(capture, envname):
    """-> buf, desc, the oracle's records, env4, env6"""
    import pyoracle
    z = np.load(GOLD, allow_pickle=False)
    fr = S.rx_frames(z, capture)
    o = pyoracle.Oracle()
    S.load_env(o, envname)
    buf, desc = F.pack_frames(fr, [1] * len(fr))
    rec, _, _, _ = o.rx_batch(buf, desc)
    return (buf, desc, rec) + sim_envs(envname)


def outcomes(buf, desc, rec, env4, env6, kinds=abi.RSPK_ALL):
    """The responder's outcomes for `kinds` and the learner's for the ARP / ND of them."""
    rsp = N.respond_batch(buf, desc, rec, kinds, env4, env6)[0]
    lk = (abi.LRNK_ARP if kinds & abi.RSPK_ARP else 0) | (abi.LRNK_ND if kinds & abi.RSPK_ND else 0)
    lrn = L.learn_keys(buf, desc, rec, lk, env6)[0] if lk else np.zeros(len(desc), np.uint8)
    return rsp, lrn


@pytest.mark.parametrize("capture,envname,n,words", CAPTURES, ids=[c[0] for c in CAPTURES])
def test_capture_counters(oracle_built, capture, envname, n, words):
    buf, desc, rec, env4, env6 = capture_case(capture, envname)
    assert len(desc) == n
    rsp, lrn = outcomes(buf, desc, rec, env4, env6)
    done, ev, info = NS.nsstat_batch(buf, desc, rec, abi.RSPK_ALL, rsp, lrn)
    assert (done == 1).all()  # no frame of the capture needs its Go handler
    assert tuple(int(x) for x in info) == (1, 1, 0, n, 0, 0, 0, 0)
    assert len(ev) == 1 and int(ev[0]["ns_id"]) == 0 and int(ev[0]["frames"]) == n
    want = np.zeros(abi.NSC_WORDS, np.uint32)
    for k, v in words.items():
        want[k] = v
    assert np.array_equal(ev[0]["cnt"], want), ev[0]["cnt"]  # no other counter is non-zero
    # the replay loop against what the capture's Go test dumped
    stats = NS.replay(ev)
    got = {name: v for (_, _, name), v in stats.items()}
    assert len(got) == len(stats)  # one plugin per capture: no name twice
    recorded = {k: v for k, v in COUNTERS[capture].items() if k not in NOT_A_HANDLER_COUNTER}
    if capture.startswith("ipv6nd"):
        assert recorded == {}  # the capture recorded no ND counter: the reply counts of test_nd_ref stand in
        reply = N.respond_batch(buf, desc, rec, abi.RSPK_ND, env6=env6)
        assert len(reply[3]) == n and all((r[:6] == bytes([0x33, 0x33, 0, 0, 0, 1])) == (capture == "ipv6nd_3.json") for r in reply[3])
    else:
        assert got == recorded, (got, recorded)


def test_capture_kinds_select(oracle_built):
    """A kind that is not selected leaves its frames to the handler: done 0, not even a candidate."""
    for capture, envname, n, _ in CAPTURES:
        buf, desc, rec, env4, env6 = capture_case(capture, envname)
        own = {"arp": abi.RSPK_ARP, "icmp": abi.RSPK_ICMP}.get(envname, abi.RSPK_ND if "nd" in capture else abi.RSPK_ICMPV6)
        rsp, lrn = outcomes(buf, desc, rec, env4, env6, abi.RSPK_ALL & ~own)
        done, ev, info = NS.nsstat_batch(buf, desc, rec, abi.RSPK_ALL & ~own, rsp, lrn)
        assert not done.any() and len(ev) == 0 and int(info[3]) == 0
        # an icmpv6 frame stays a candidate while either of its two kinds is selected
        assert int(info[5]) == (n if envname == "ipv6" else 0)
        rsp, lrn = outcomes(buf, desc, rec, env4, env6, own)
        done, ev, info = NS.nsstat_batch(buf, desc, rec, own, rsp, lrn)
        assert (done == 1).all() and len(ev) == 1


# ---- hand-built frames: the branches no capture reaches -------------------------------------------
MAC_A, MAC_B = bytes([0, 0, 1, 0, 0, 0]), bytes([0, 0x10, 0x94, 0, 0, 2])
IP6_A = bytes([0x20, 1, 0x0D, 0xB8] + [0] * 11 + [2])
IP6_B = bytes([0x20, 1, 0x0D, 0xB8] + [0] * 11 + [1])


def record(proto, lk, l3=14, l4=0, ns=3, status=0):
    r = np.zeros(1, abi.REC_DTYPE)
    r["ns_id"], r["client_id"], r["vport"], r["l3"], r["l4"] = ns, 0, 1, l3, l4
    r["proto"], r["status"], r["flags"] = proto, status, abi.LK[lk] << 4
    return r[0]


def arp_frame(op, dst=MAC_A):
    return dst + MAC_B + b"\x08\x06" + F.arp(op, MAC_B, bytes([16, 0, 0, 2]), bytes(6), bytes([16, 0, 0, 0])) + bytes(18)


def icmp4_frame(t, c, src=bytes([16, 0, 0, 2])):
    ip = bytes([0x45, 0, 0, 36, 0, 0, 0, 0, 64, 1, 0, 0]) + src + bytes([16, 0, 0, 0])
    return MAC_A + MAC_B + b"\x08\x00" + ip + bytes([t, c, 0, 0, 0, 1, 0, 1]) + bytes(8)


def icmp6_frame(t, c, src=IP6_B):
    ip = bytes([0x60, 0, 0, 0, 0, 24, 58, 255]) + src + IP6_A
    return MAC_A + MAC_B + b"\x86\xdd" + ip + bytes([t, c, 0, 0]) + bytes(20)


A, I4, I6 = NS.CB_ARP, NS.CB_ICMP, NS.CB_ICMPV6
# (branch, frame, record, rsp, lrn) -> (done, counters)
HAND = [
    ("arp-not-for-us", arp_frame(1), record(A, "NO_CLIENT"), 0, 1, 1, [0, 1]),
    ("arp-client-no-plugin", arp_frame(1), record(A, "CLIENT_NO_PLUGIN"), 0, 1, 1, [0]),
    ("arp-answered", arp_frame(1), record(A, "CLIENT"), abi.RSP_ARP, 1, 1, [0, 5]),
    ("arp-request-host", arp_frame(1), record(A, "CLIENT"), abi.RSP_NOSPC, 1, 0, []),
    ("arp-request-host", arp_frame(1), record(A, "CLIENT"), abi.RSP_HOST, 1, 0, []),
    ("arp-request-host", arp_frame(1), record(A, "CLIENT"), abi.RSP_NONE, 1, 0, []),
    ("arp-request-host", arp_frame(1), record(A, "NS_LEVEL"), 0, 1, 0, []),
    ("arp-learn-host", arp_frame(1), record(A, "CLIENT"), abi.RSP_ARP, abi.LRN_HOST, 0, []),
    ("arp-learn-host", arp_frame(2), record(A, "NS_LEVEL"), 0, abi.LRN_HOST, 0, []),
    ("arp-reply", arp_frame(2), record(A, "NS_LEVEL"), 0, 2, 1, [2]),
    ("arp-reply-broadcast", arp_frame(2, b"\xff" * 6), record(A, "NS_LEVEL"), 0, 0, 1, [3]),
    ("arp-reply", arp_frame(2, b"\xff" * 5 + b"\xfe"), record(A, "NS_LEVEL"), 0, 2, 1, [2]),
    ("arp-wrong-op", arp_frame(3), record(A, "NS_LEVEL"), 0, 0, 1, [4]),
    ("arp-wrong-op", arp_frame(0x0101), record(A, "NO_CLIENT"), 0, 0, 1, [4]),
    ("arp-bounds", arp_frame(1), record(A, "CLIENT", l3=13), abi.RSP_ARP, 1, 0, []),
    ("arp-bounds", arp_frame(1)[:41], record(A, "CLIENT"), abi.RSP_ARP, 1, 0, []),
    ("parser-err", arp_frame(1), record(A, "NO_NS"), 0, 0, 2, []),
    ("parser-err", arp_frame(2), record(A, "NS_NO_PLUGIN"), 0, 0, 2, []),
    ("parser-err", icmp4_frame(8, 0), record(I4, "NO_NS", l4=34), 0, 0, 2, []),
    ("parser-err", icmp4_frame(8, 0), record(I4, "NS_NO_PLUGIN", l4=34), 0, 0, 2, []),
    ("parser-err", icmp6_frame(128, 0), record(I6, "NO_NS", l4=54), 0, 0, 2, []),
    ("parser-err", icmp6_frame(135, 0), record(I6, "NS_NO_PLUGIN", l4=54), 0, 0, 2, []),
    ("no-lookup", arp_frame(1), record(A, "NONE"), 0, 0, 0, []),
    ("not-candidate", arp_frame(1), record(A, "CLIENT", status=4), abi.RSP_ARP, 1, 0, []),
    ("not-candidate", arp_frame(1), record(8, "CLIENT"), 0, 0, 0, []),
    ("icmp-no-client", icmp4_frame(8, 0), record(I4, "NO_CLIENT", l4=34), 0, 0, 1, [7]),
    ("icmp-no-client", icmp4_frame(3, 1), record(I4, "NO_CLIENT", l4=34), 0, 0, 1, [7]),
    ("icmp-other-lookup", icmp4_frame(8, 0), record(I4, "CLIENT_NO_PLUGIN", l4=34), 0, 0, 0, []),
    ("icmp-mcast", icmp4_frame(8, 0), record(I4, "CLIENT", l4=34), abi.RSP_DROP_MCAST, 0, 1, [8]),
    ("icmp-echo", icmp4_frame(8, 0), record(I4, "CLIENT", l4=34), abi.RSP_ICMP, 0, 1, [6]),
    ("icmp-echo-host", icmp4_frame(8, 0), record(I4, "CLIENT", l4=34), abi.RSP_NOSPC, 0, 0, []),
    ("icmp-echo-host", icmp4_frame(8, 0), record(I4, "CLIENT", l4=34), abi.RSP_NONE, 0, 0, []),
    ("icmp-handler-type", icmp4_frame(13, 0), record(I4, "CLIENT", l4=34), abi.RSP_HOST, 0, 0, []),
    ("icmp-handler-type", icmp4_frame(0, 0), record(I4, "CLIENT", l4=34), 0, 0, 0, []),
] + [("icmp-handler-type", icmp4_frame(3, c), record(I4, "CLIENT", l4=34), 0, 0, 0, []) for c in range(5)] + [
    ("icmp-unhandled", icmp4_frame(t, c), record(I4, "CLIENT", l4=34), 0, 0, 1, [9])
    for t, c in ((3, 5), (8, 1), (13, 1), (0, 1), (14, 0), (11, 0), (5, 0), (255, 255))
] + [
    ("icmp-bounds", icmp4_frame(9, 0), record(I4, "CLIENT", l4=43), 0, 0, 0, []),
    ("icmp-bounds", icmp4_frame(9, 0), record(I4, "NO_CLIENT", l3=13, l4=34), 0, 0, 0, []),
    ("v6-no-client", icmp6_frame(128, 0), record(I6, "NO_CLIENT", l4=54), 0, 0, 1, [11]),
    ("v6-echo-mcast-source", icmp6_frame(128, 0, bytes([0xFF, 2] + [0] * 13 + [1])), record(I6, "NO_CLIENT", l4=54), 0, 0, 0, []),
    ("v6-echo", icmp6_frame(128, 0), record(I6, "CLIENT", l4=54), abi.RSP_ICMPV6, 0, 1, [10]),
    ("v6-mcast", icmp6_frame(128, 0), record(I6, "CLIENT", l4=54), abi.RSP_DROP_MCAST, 0, 1, [12]),
    ("v6-echo-host", icmp6_frame(128, 0), record(I6, "CLIENT", l4=54), abi.RSP_NOSPC, 0, 0, []),
    ("v6-echo-host", icmp6_frame(128, 0), record(I6, "CLIENT", l4=54), abi.RSP_HOST, 0, 0, []),
    ("v6-echo-other-lookup", icmp6_frame(128, 0), record(I6, "NS_LEVEL", l4=54), 0, 0, 0, []),
    ("v6-other-lookup", icmp6_frame(2, 0), record(I6, "CLIENT", l4=54), 0, 0, 0, []),
    ("ns-answered-unicast", icmp6_frame(135, 0), record(I6, "NS_LEVEL", l4=54), abi.RSP_ND, abi.LRN_ND_NS, 1, [14, 15]),
    ("ns-answered-unicast", icmp6_frame(135, 0), record(I6, "NS_LEVEL", l4=54), abi.RSP_ND, abi.LRN_NONE, 1, [14, 15]),
    ("ns-answered-dad", icmp6_frame(135, 0, bytes(16)), record(I6, "NS_LEVEL", l4=54), abi.RSP_ND, 0, 1, [14, 16]),
    # ::ffff:0.0.0.0 is unspecified to net.IP.IsUnspecified, the responder's reading
    ("ns-answered-dad", icmp6_frame(135, 0, bytes(10) + b"\xff\xff" + bytes(4)), record(I6, "NS_LEVEL", l4=54), abi.RSP_ND, 0, 1, [14, 16]),
    ("ns-host", icmp6_frame(135, 0), record(I6, "NS_LEVEL", l4=54), abi.RSP_NONE, 0, 0, []),
    ("ns-host", icmp6_frame(135, 0), record(I6, "NS_LEVEL", l4=54), abi.RSP_HOST, 0, 0, []),
    ("ns-host", icmp6_frame(135, 0), record(I6, "NS_LEVEL", l4=54), abi.RSP_NOSPC, abi.LRN_ND_NS, 0, []),
    ("ns-host", icmp6_frame(135, 0), record(I6, "NS_LEVEL", l4=54), abi.RSP_ND, abi.LRN_HOST, 0, []),
    ("na-learned", icmp6_frame(136, 0), record(I6, "NS_LEVEL", l4=54), 0, abi.LRN_ND_NA, 1, [17, 18]),
    ("na-host", icmp6_frame(136, 0), record(I6, "NS_LEVEL", l4=54), 0, abi.LRN_NONE, 0, []),
    ("na-host", icmp6_frame(136, 0), record(I6, "NS_LEVEL", l4=54), 0, abi.LRN_HOST, 0, []),
] + [("v6-handler-type", icmp6_frame(t, 0), record(I6, "NS_LEVEL", l4=54), 0, 0, 0, []) for t in (129, 130, 131, 132, 133, 134, 137, 143)] + [
    ("v6-handler-type", icmp6_frame(1, c), record(I6, "NS_LEVEL", l4=54), 0, 0, 0, []) for c in range(7)
] + [
    ("v6-unhandled", icmp6_frame(t, c), record(I6, "NS_LEVEL", l4=54), 0, 0, 1, [13])
    for t, c in ((1, 7), (2, 0), (3, 0), (3, 1), (4, 0), (128, 1), (129, 1), (130, 1), (133, 2), (135, 1), (136, 1))
] + [
    ("v6-bounds", icmp6_frame(2, 0), record(I6, "NS_LEVEL", l4=53), 0, 0, 0, []),
    ("v6-bounds", icmp6_frame(2, 0), record(I6, "NS_LEVEL", l4=75), 0, 0, 0, []),
    ("v6-bounds", icmp6_frame(2, 0), record(I6, "NS_LEVEL", l3=13, l4=54), 0, 0, 0, []),
]


@pytest.mark.parametrize("case", HAND, ids=[f"{i}-{c[0]}" for i, c in enumerate(HAND)])
def test_hand_built_branches(case):
    why, frame, rec, rsp, lrn, done, cnt = case
    assert NS.nsstat_branch(frame, rec, abi.RSPK_ALL, rsp, lrn) == why
    assert NS.nsstat_ref(frame, rec, abi.RSPK_ALL, rsp, lrn) == (done, cnt)
    if why != "not-candidate":
        assert NS.nsstat_ref(frame, rec, abi.RSPK_ALL, rsp, lrn, hole=True) == (0, [])  # a hole is nothing
    if done == 1:  # every done-1 frame bumps exactly one of the counters `frames` is the sum of
        assert sum(c in NS.FIRST for c in cnt) == 1 and len(cnt) <= 2
        assert NS.nsstat_ref(frame, rec, abi.RSPK_ALL, rsp, lrn, max_ns=3) == (0, [])
        assert NS.nsstat_ref(frame, rec, abi.RSPK_ALL, rsp, lrn, max_ns=4) == (done, cnt)


def test_hand_built_reach_every_branch_and_counter():
    seen = {c[0] for c in HAND}
    # the two "not selected" branches are reached through `kinds` below
    want = {"not-candidate", "parser-err", "no-lookup", "arp-bounds", "arp-learn-host", "arp-not-for-us",
            "arp-client-no-plugin", "arp-answered", "arp-request-host", "arp-reply-broadcast", "arp-reply", "arp-wrong-op",
            "icmp-bounds", "icmp-no-client", "icmp-other-lookup", "icmp-mcast", "icmp-echo", "icmp-echo-host",
            "icmp-handler-type", "icmp-unhandled", "v6-bounds", "v6-no-client", "v6-echo-mcast-source",
            "v6-echo-other-lookup", "v6-echo", "v6-mcast", "v6-echo-host", "v6-other-lookup", "na-learned", "na-host",
            "ns-host", "ns-answered-dad", "ns-answered-unicast", "v6-handler-type", "v6-unhandled"}
    assert seen == want, seen ^ want
    assert {k for c in HAND for k in c[6]} == set(range(19))
    echo, ns, unh = icmp6_frame(128, 0), icmp6_frame(135, 0), icmp6_frame(2, 0)
    r = record(I6, "CLIENT", l4=54)
    assert NS.nsstat_branch(echo, r, abi.RSPK_ND, abi.RSP_ICMPV6) == "v6-echo-not-selected"
    r = record(I6, "NS_LEVEL", l4=54)
    assert NS.nsstat_branch(ns, r, abi.RSPK_ICMPV6, abi.RSP_ND) == "nd-not-selected"
    assert NS.nsstat_branch(unh, r, abi.RSPK_ND, 0) == "v6-unhandled-not-selected"
    assert NS.nsstat_branch(unh, r, abi.RSPK_ARP | abi.RSPK_ICMP, 0) == "not-candidate"


def test_fold_and_replay():
    """Events in ascending ns_id, frames = the done-1 frames of the Namespace, words 6 and 10 replayed
    into two Go counters each; overflow writes nothing and keeps the rest of info."""
    ns_ids = np.array([5, 2, 5, 9, 2, 7, 5], np.uint32)
    done = np.array([1, 1, 0, 2, 1, 1, 1], np.uint8)
    cnts = [[6], [0, 5], [], [], [10], [14, 15], [6]]
    cand = np.array([1, 1, 1, 1, 1, 1, 1], bool)
    ev, info = NS.fold(ns_ids, done, cnts, cand)
    assert [int(e["ns_id"]) for e in ev] == [2, 5, 7] and [int(e["frames"]) for e in ev] == [2, 2, 1]
    assert tuple(int(x) for x in info) == (3, 3, 0, 5, 1, 1, 0, 0)
    assert int(ev[1]["cnt"][6]) == 2 and int(ev[0]["cnt"][10]) == 1 and int(ev["cnt"].sum()) == 7
    stats = NS.replay(ev)
    assert stats[(5, "icmp", "pktRxIcmpQuery")] == 2 and stats[(5, "icmp", "pktTxIcmpResponse")] == 2
    assert stats[(2, "ipv6", "pktRxIcmpQuery")] == 1 and stats[(2, "ipv6", "pktTxIcmpResponse")] == 1
    assert stats[(2, "arp", "pktTxReply")] == 1 and stats[(7, "nd", "pktTxNeighborAdvUnicast")] == 1 and len(stats) == 8
    ev2, info2 = NS.fold(ns_ids, done, cnts, cand, ev_cap=2)
    assert len(ev2) == 0 and tuple(int(x) for x in info2) == (0, 3, 1, 5, 1, 1, 0, 0)
    ev3, info3 = NS.fold(ns_ids, done, cnts, cand, ev_cap=3)
    assert ev3.tobytes() == ev.tobytes() and np.array_equal(info3, info)


# ---- the mixed batch's coverage -------------------------------------------------------------------
def mixed_case(n):
    import pyoracle
    fr, vp = NS.mixed_batch(n)
    o = pyoracle.Oracle()
    env4, env6 = R.Env(), N.Env()
    N.load_combined(o, env4, env6)
    buf, desc = R.pack_with_holes(fr, vp, L.HOLE_EVERY)
    rec, _, _, _ = o.rx_batch(buf, desc)
    return buf, desc, rec, env4, env6


def test_mixed_batch_reaches_every_counter(oracle_built):
    """A condition on the inputs: a comparison against nsstat_ref cannot pass on an empty set."""
    buf, desc, rec, env4, env6 = mixed_case(4096)
    rsp, lrn = outcomes(buf, desc, rec, env4, env6)
    done, cnts, cand = NS.nsstat_frames(buf, desc, rec, abi.RSPK_ALL, rsp, lrn)
    assert all((done == k).sum() >= 64 for k in (0, 1, 2)) and (cand & (done == 0)).sum() >= 64
    hits = {k: sum(k in c for c in cnts) for k in range(abi.NSC_WORDS)}
    assert all(hits[k] >= 4 for k in range(19)) and not any(hits[k] for k in range(19, abi.NSC_WORDS)), hits
    assert set(rsp) == {0, 1, 2, 3, 4, 5, 7} and set(lrn) == set(range(6))
    ev, info = NS.fold(rec["ns_id"], done, cnts, cand)
    assert len(ev) == 7 and (ev["frames"] > 16).all() and int(info[0]) == 7 and int(info[2]) == 0
    # every prefix the device test takes has frames of all three values of done
    for n in (63, 64, 65, 255, 256, 257):
        assert all((done[:n] == k).any() for k in (0, 1, 2))
    # the kinds alone: done under all kinds is the one value among them that is not 0, the counters add up
    alone = [NS.nsstat_frames(buf, desc, rec, k, rsp, lrn) for k in (1, 2, 4, 8)]
    assert np.array_equal(np.maximum.reduce([a[0] for a in alone]), done)
    for i in range(len(desc)):
        assert sorted(c for a in alone for c in a[1][i]) == sorted(cnts[i])


# ---- the C-ABI -----------------------------------------------------------------------------------
@pytest.fixture()
def host_handle(lib):
    cfg = abi.Cfg(-1, 16, 16, 1000, 1 << 16)
    h = C.c_void_p()
    assert lib.emurx_open(C.byref(cfg), C.byref(h)) == 0
    yield lib, h
    lib.emurx_close(h)


def test_nsstat_abi(lib):
    """The new symbols are exported, the event is 96 bytes, and abi.py mirrors the header."""
    assert hasattr(lib, "emurx_nsstat_dev") and hasattr(lib, "emurx_nsstat_max_events")
    assert {"emurx_nsstat_dev", "emurx_nsstat_max_events"} <= {s[0] for s in abi.SIGNATURES}
    dt = abi.NSSTAT_EV_DTYPE
    assert dt.itemsize == 96 and [dt.fields[k][1] for k in ("ns_id", "frames", "cnt")] == [0, 4, 8]
    assert dt.fields["cnt"][0].shape == (22,) and (abi.NSC_WORDS, abi.NSS_INFO_WORDS) == (22, 8)
    header = (abi.REPO_ROOT / "include" / "emu_rx.h").read_text()
    for text in ("#define EMURX_NSC_WORDS 22", "#define EMURX_NSS_INFO_WORDS 8", "uint32_t cnt[EMURX_NSC_WORDS];",
                 "} emurx_nsstat_ev;", "EMURX_NSC_ARP_QUERY = 0", "EMURX_NSC_ARP_TX_REPLY = 5", "EMURX_NSC_ICMP_ECHO = 6",
                 "EMURX_NSC_V6_ECHO = 10", "EMURX_NSC_ND_RX_NS = 14", "EMURX_NSC_ND_RX_NA_LEARN = 18"):
        assert text in header, text
    # the enum's names in the header, in order, are abi.py's
    import re
    names = re.findall(r"EMURX_(NSC_[A-Z0-9_]+) = (\d+)", header)
    assert [int(v) for _, v in names] == list(range(19)) and all(getattr(abi, n) == int(v) for n, v in names)
    assert len(abi.NSC_GO) == 19
    # sizeof(emurx_nsstat_ev) as the C compiler lays it out: two u32 and 22 u32, no padding
    class Ev(C.Structure):
        _fields_ = [("ns_id", C.c_uint32), ("frames", C.c_uint32), ("cnt", C.c_uint32 * 22)]
    assert C.sizeof(Ev) == 96
    assert lib.emurx_abi_version() == 6  # the call is additive


def test_nsstat_argument_checks(host_handle):
    lib, h = host_handle
    EINVAL, EDEVICE = -22, -5
    cap = lib.emurx_nsstat_max_events(h)
    assert cap == 16  # min(max_frames 1000, max_ns 16)
    assert lib.emurx_nsstat_max_events(None) == 0
    a = 0x10000  # stand-ins for device pointers: the checks come before anything is dereferenced

    def call(frames=a, desc=a, rec=a, n=4, kinds=abi.RSPK_ALL, rsp=a, lrn=a, ev=a, ev_cap=16, done=a, info=a, handle=h):
        return lib.emurx_nsstat_dev(handle, frames, desc, rec, n, kinds, rsp, lrn, ev, ev_cap, done, info, None)

    for kw in (dict(handle=None), dict(frames=None), dict(desc=None), dict(rec=None), dict(rsp=None), dict(lrn=None),
               dict(lrn=None, kinds=abi.RSPK_ARP), dict(lrn=None, kinds=abi.RSPK_ND | abi.RSPK_ICMP), dict(ev=None),
               dict(info=None), dict(info=None, n=0), dict(ev=None, n=0), dict(kinds=0), dict(kinds=16), dict(kinds=31),
               dict(ev_cap=0), dict(ev_cap=cap + 1), dict(rec=a + 8), dict(desc=a + 4), dict(ev=a + 4), dict(info=a + 4)):
        assert call(**kw) == EINVAL, kw
    # valid arguments reach the handle: a host-only one has no device
    for kw in (dict(), dict(done=None), dict(kinds=abi.RSPK_ARP), dict(kinds=abi.RSPK_ND), dict(ev_cap=1), dict(ev_cap=cap),
               dict(lrn=None, kinds=abi.RSPK_ICMP | abi.RSPK_ICMPV6), dict(n=1 << 20),
               dict(frames=None, desc=None, rec=None, rsp=None, lrn=None, n=0, done=None)):
        assert call(**kw) == EDEVICE, kw

"""The learning rule and its fold against the reference's captures and against a model of the Go
resolution tables, the learning batch's coverage, and the argument checks of emurx_learn_dev on a
host-only handle (no GPU).

learn_ref (tests/learn_ref.py) applied to the rx frames of arp4, arp5 (six requests each) and arp2
(57 unicast replies), with records from the oracle and the environment of the capture's Go test
(tests/sim_envs.py), folds each capture into one event; replayed into a table that holds the one
Incomplete flow the environment's client created for its gateway (addIncomplete 1 in the capture),
the event reproduces the capture's recorded pktRxArpQuery / pktRxArpReply and moveComplete
(tests/golden/learn_counters.json).

No capture of the reference records the ND cache counters: the ND half of the rule is pinned by
its citations (learn_ref's docstring, include/emu_rx.h) and by the learning batch reaching every
branch of it at least twice, HOST included (test_learning_batch_reaches_every_branch)."""
import ctypes as C
import json
from collections import Counter
from pathlib import Path

import numpy as np
import pytest

import learn_ref as L
import nd_ref as N
import respond_ref as R
import sim_envs as S
from emurx import abi, frames as F
from test_oracle_corpus import GOLD

COUNTERS = json.loads((Path(__file__).parent / "golden" / "learn_counters.json").read_text())
GATEWAY = bytes([16, 0, 0, 2])  # arp_test.go:87-89, the client's default gateway


def capture_case(capture):
    """-> buf, desc, the oracle's records"""
    import pyoracle
    z = np.load(GOLD, allow_pickle=False)
    fr = S.rx_frames(z, capture)
    o = pyoracle.Oracle()
    S.load_env(o, "arp")
    buf, desc = F.pack_frames(fr, [1] * len(fr))
    rec, _, _, _ = o.rx_batch(buf, desc)
    return buf, desc, rec


@pytest.mark.parametrize("capture,kind,rx_counter,count", [("arp4.json", abi.LRN_ARP_REQ, "pktRxArpQuery", 6),
                                                           ("arp5.json", abi.LRN_ARP_REQ, "pktRxArpQuery", 6),
                                                           ("arp2.json", abi.LRN_ARP_REPLY, "pktRxArpReply", 57)])
def test_capture_counters(oracle_built, capture, kind, rx_counter, count):
    want = COUNTERS[capture]
    assert want[rx_counter] == count and want["moveComplete"] == 1 and want["addIncomplete"] == 1
    buf, desc, rec = capture_case(capture)
    outcome, ev, info = L.learn_batch(buf, desc, rec)
    assert len(desc) == count and (outcome == kind).all()
    assert len(ev) == 1 and tuple(int(x) for x in info) == (1, 1, 0) + tuple(count if k == kind else 0 for k in range(1, 6))
    e = ev[0]
    assert (int(e["ns_id"]), int(e["count"]), int(e["first"]), int(e["last"]), int(e["kind"])) == (0, count, 0, count - 1, kind)
    assert e["ip"].tobytes() == GATEWAY + bytes(12)
    for replay in ("events", "frames"):
        c = L.Caches()
        c.table(0, kind).add_new(GATEWAY + bytes(12), None, L.INCOMPLETE)  # the client's gateway, unresolved
        if replay == "events":
            c.apply_events(L.fold(L.learn_keys(buf, desc, rec)[1]))
        else:
            c.apply_frames(L.learn_keys(buf, desc, rec)[1])
        t = c.table(0, kind)
        got = dict(t.c, **{rx_counter: c.rx[(0, rx_counter)]})
        for k, v in want.items():
            if k != "pktRxArpQueryNotForUs":  # the client lookup's counter, not the cache's
                assert got[k] == v, (replay, k)
        f = t.flows[GATEWAY + bytes(12)]
        assert f["state"] == L.COMPLETE and f["mac"] == e["mac"].tobytes() and f["touch"] and got["addLearn"] == 0


# ---- the fold against frame-by-frame handling -----------------------------------------------------
A, B = bytes([0, 0x10, 0x94, 0, 0, 0xA]), bytes([0, 0x10, 0x94, 0, 0, 0xB])
IP1, IP2 = bytes([48, 0, 0, 1]), bytes([48, 0, 0, 2])


def arp_frame(ns, op, spa, sha):
    mac, ip4, _ = R._client(ns, 0)
    f = R._eth(L.BCAST if op == 1 else mac, sha, R._NS[ns], 0x0806, F.arp(op, sha, spa, bytes(6) if op == 1 else mac, ip4), 0)
    return f + bytes(max(60 - len(f), 0))


def seeded_sequence(seed, n=120):
    """Holds, whatever the seed: MAC A, B, A for one IP; that IP in two Namespaces; one (IP, MAC)
    pair as request and as reply; then a seeded walk over a small pool, so keys repeat."""
    rng = np.random.default_rng([seed, 0x736571])
    head = [(0, 1, IP1, A), (0, 1, IP1, B), (0, 1, IP1, A), (1, 1, IP1, A), (0, 2, IP2, A), (0, 1, IP2, A)]
    pool = [(ns, op, ip, mac) for ns in (0, 1, 2) for op in (1, 2) for ip in (IP1, IP2) for mac in (A, B)]
    return head + [pool[int(rng.integers(0, len(pool)))] for _ in range(n - len(head))]


def keys_of(seq):
    import pyoracle
    o = pyoracle.Oracle()
    R.load_tables(o)
    buf, desc = F.pack_frames([arp_frame(*s) for s in seq], [1] * len(seq))
    rec, _, _, _ = o.rx_batch(buf, desc)
    outcome, keys = L.learn_keys(buf, desc, rec)
    assert all(k == (ns, op, ip + bytes(12), mac) for k, (ns, op, ip, mac) in zip(keys, seq))
    return keys


def preset(c: L.Caches, state):
    """IP1 of Namespace 0 already in the ARP table: Incomplete (a client waits for it), Refresh
    (resolved before, being re-queried), or absent."""
    if state is not None:
        t = c.table(0, abi.LRN_ARP_REQ)
        t.add_new(IP1 + bytes(12), None, L.INCOMPLETE)
        if state == L.REFRESH:
            t.learn(IP1 + bytes(12), B)
            t.flows[IP1 + bytes(12)]["state"] = L.REFRESH
        t.c.update(dict.fromkeys(t.c, 0))


@pytest.mark.parametrize("state", [None, L.INCOMPLETE, L.REFRESH])
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_events_replay_equals_frames(oracle_built, seed, state):
    keys = keys_of(seeded_sequence(seed))
    events = L.fold(keys)
    assert [e[3] for e in events] == sorted(e[3] for e in events) and sum(e[1] for e in events) == len(keys)
    assert len({e[0] for e in events}) == len(events) == len(set(keys))
    by_frame, by_event = L.Caches(), L.Caches()
    preset(by_frame, state)
    preset(by_event, state)
    by_frame.apply_frames(keys)
    by_event.apply_events(events)
    assert by_frame.snapshot() == by_event.snapshot()
    t = by_frame.table(0, abi.LRN_ARP_REQ)
    assert t.c["moveComplete"] == (0 if state is None else 1) and t.c["tblAdd"] == (2 if state is None else 1)
    # every prefix too: a batch boundary may fall anywhere
    for cut in (1, 2, 3, 4, 6, 17):
        a, b = L.Caches(), L.Caches()
        preset(a, state)
        preset(b, state)
        a.apply_frames(keys[:cut])
        b.apply_events(L.fold(keys[:cut]))
        b.apply_events([(k, c, f + cut, l + cut) for k, c, f, l in L.fold(keys[cut:])])
        a.apply_frames(keys[cut:])
        assert a.snapshot() == b.snapshot() == by_frame.snapshot(), cut


def test_one_key_batch(oracle_built):
    keys = keys_of([(0, 1, IP1, A)] * 50)
    (k, count, first, last), = L.fold(keys)
    assert (count, first, last) == (50, 0, 49)
    a, b = L.Caches(), L.Caches()
    a.apply_frames(keys)
    b.apply_events(L.fold(keys))
    assert a.snapshot() == b.snapshot()
    f = a.table(0, 1).flows[IP1 + bytes(12)]
    assert f["state"] == L.LEARNED and f["touch"] and a.table(0, 1).c["addLearn"] == 1 and a.rx[(0, "pktRxArpQuery")] == 50
    # a single frame leaves touch clear: the second application is what sets it
    c = L.Caches()
    c.apply_events(L.fold(keys[:1]))
    assert not c.table(0, 1).flows[IP1 + bytes(12)]["touch"]


# ---- the learning batch's coverage ----------------------------------------------------------------
def learning_case(n, seed=5):
    import pyoracle
    fr, vp = L.learning_batch(n, seed)
    o = pyoracle.Oracle()
    env6 = N.Env()
    N.load_combined(o, None, env6)
    buf, desc = L.pack(fr, vp)
    rec, _, _, _ = o.rx_batch(buf, desc)
    return buf, desc, rec, env6


def test_learning_batch_reaches_every_branch(oracle_built):
    """A condition on the inputs: a comparison against learn_ref cannot pass on an empty set."""
    buf, desc, rec, env6 = learning_case(4096)
    hits = Counter()
    for i in range(len(desc)):
        d = desc[i]
        f = bytes(buf[int(d["off"]):int(d["off"]) + int(d["len"])])
        hits[L.learn_branch(f, rec[i], env6, hole=int(d["pad"]) == abi.DESC_HOLE)] += 1
    assert not set(hits) - set(L.BRANCHES), set(hits) - set(L.BRANCHES)
    for b in L.BRANCHES:
        assert hits[b] >= 2, (b, hits[b])
    outcome, ev, info = L.learn_batch(buf, desc, rec, env6=env6)
    for k in range(6):
        assert (outcome == k).sum() >= 8, k
    # keys repeat and keys stand alone: the fold has both to get right
    assert 4 <= len(ev) < int(info[3:7].sum()) and (ev["count"] > 1).sum() >= 32 and (ev["count"] == 1).sum() >= 32
    assert {int(k) for k in ev["kind"]} == {1, 2, 3, 4} and int(ev["count"].max()) >= 8
    assert any(bytes(e["mac"]) == bytes(6) for e in ev) and any(bytes(e["ip"][:4]) == bytes(4) and e["kind"] == 1 for e in ev)
    # the kinds alone: their union is the whole
    oa, ea, ia = L.learn_batch(buf, desc, rec, abi.LRNK_ARP, env6)
    on, en, i_n = L.learn_batch(buf, desc, rec, abi.LRNK_ND, env6)
    assert np.array_equal(np.maximum(oa, on), outcome) and not (oa & on).any() and len(ea) + len(en) == len(ev)


def test_offsets_that_do_not_fit_give_host(oracle_built):
    buf, desc, rec, env6 = learning_case(256)
    outcome, keys = L.learn_keys(buf, desc, rec, env6=env6)
    seen = set()
    for i in np.nonzero(outcome != 0)[0]:
        r = rec[i:i + 1].copy()
        f = bytes(buf[int(desc[i]["off"]):int(desc[i]["off"]) + int(desc[i]["len"])])
        arp = int(r["proto"][0]) == L.CB_ARP
        for field, v in (("l3", 13), ("l3", len(f) - 27)) if arp else (("l3", 13), ("l4", len(f) - 3), ("l4", int(r["l3"][0]) + 39)):
            r2 = r.copy()
            r2[field] = v
            assert L.learn_ref(f, r2[0], env6) == (abi.LRN_HOST, None)
            seen.add(L.learn_branch(f, r2[0], env6))
    assert seen == {"arp-bounds", "nd-bounds"}


# ---- the C-ABI -----------------------------------------------------------------------------------
@pytest.fixture()
def host_handle(lib):
    cfg = abi.Cfg(-1, 16, 16, 1000, 1 << 16)
    h = C.c_void_p()
    assert lib.emurx_open(C.byref(cfg), C.byref(h)) == 0
    yield lib, h
    lib.emurx_close(h)


def test_learn_abi_constants():
    assert (abi.LRN_NONE, abi.LRN_ARP_REQ, abi.LRN_ARP_REPLY, abi.LRN_ND_NS, abi.LRN_ND_NA, abi.LRN_HOST) == (0, 1, 2, 3, 4, 5)
    assert (abi.LRNK_ARP, abi.LRNK_ND, abi.LRNK_ALL, abi.LRN_INFO_WORDS) == (1, 2, 3, 8)
    dt = abi.LEARN_EV_DTYPE
    assert dt.itemsize == 40
    assert [dt.fields[k][1] for k in ("ns_id", "count", "first", "last", "ip", "mac", "kind", "pad")] == [0, 4, 8, 12, 16, 32, 38, 39]
    names = {s[0] for s in abi.SIGNATURES}
    assert {"emurx_learn_dev", "emurx_learn_max_events"} <= names
    header = (abi.REPO_ROOT / "include" / "emu_rx.h").read_text()
    for text in ("EMURX_LRN_NONE = 0", "EMURX_LRN_ARP_REQ = 1, EMURX_LRN_ARP_REPLY = 2, EMURX_LRN_ND_NS = 3, EMURX_LRN_ND_NA = 4",
                 "EMURX_LRN_HOST = 5", "#define EMURX_LRNK_ARP 1u", "#define EMURX_LRNK_ND  2u", "#define EMURX_LRNK_ALL 3u",
                 "#define EMURX_LRN_INFO_WORDS 8"):
        assert text in header, text


def test_learn_argument_checks(host_handle):
    lib, h = host_handle
    EINVAL, EDEVICE = -22, -5
    cap = lib.emurx_learn_max_events(h)
    assert cap == 1024  # half of the 2048 slots that hold twice max_frames = 1000
    assert lib.emurx_learn_max_events(None) == 0
    a = 0x10000  # stand-ins for device pointers: the checks come before anything is dereferenced

    def call(frames=a, desc=a, rec=a, n=4, kinds=abi.LRNK_ALL, ev=a, ev_cap=16, outcome=a, info=a, handle=h):
        return lib.emurx_learn_dev(handle, frames, desc, rec, n, kinds, ev, ev_cap, outcome, info, None)

    for kw in (dict(handle=None), dict(frames=None), dict(desc=None), dict(rec=None), dict(ev=None), dict(info=None),
               dict(info=None, n=0), dict(kinds=0), dict(kinds=4), dict(kinds=7), dict(ev_cap=0), dict(ev_cap=cap + 1),
               dict(rec=a + 8), dict(desc=a + 4), dict(ev=a + 4), dict(info=a + 4), dict(n=abi.TX_ZMQ_MAX_FRAMES)):
        assert call(**kw) == EINVAL, kw
    # valid arguments reach the handle: a host-only one has no device
    for kw in (dict(), dict(outcome=None), dict(kinds=abi.LRNK_ARP), dict(kinds=abi.LRNK_ND), dict(ev_cap=1), dict(ev_cap=cap),
               dict(n=abi.TX_ZMQ_MAX_FRAMES - 1), dict(frames=None, desc=None, rec=None, n=0, outcome=None)):
        assert call(**kw) == EDEVICE, kw

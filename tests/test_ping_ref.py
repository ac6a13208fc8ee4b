"""ping_ref against the reference's own ping simulations, and the fold + replay against the frame
by frame handling it restates (CPU; records from the oracle)."""
import copy

import numpy as np
import pytest

import ping_cases as K
import ping_ref as P
import sim_envs as S
from emurx import abi, frames as F


def classify_with(load, frames):
    import pyoracle
    o = pyoracle.Oracle()
    load(o)
    buf, desc = F.pack_frames(frames, [1] * len(frames))
    rec, _, _, _ = o.rx_batch(buf, desc)
    return buf, desc, rec


def items_of(frames, now=K.NOW, fams=abi.PNGK_ALL):
    env = P.Env()
    buf, desc, rec = classify_with(lambda o: K.load_tables(o, env), frames)
    return P.batch_items(buf, desc, rec, env, fams, now), rec


def states():
    """The ping running on every client, on none, and running with a foreign identifier."""
    cids = [K.client(ns, c)[0] for ns in range(2) for c in range(K.N_CLIENTS)]
    run = P.State(pings={(cid, fam): P.Ping() for cid in cids for fam in (4, 6)})
    foreign = P.State(pings={(cid, fam): P.Ping(identifier=0x7777) for cid in cids for fam in (4, 6)})
    mixed = P.State(pings={(cid, fam): P.Ping(startingSeq=0xFFF3) for cid in cids[::2] for fam in (4, 6)})
    return dict(running=run, absent=P.State(), foreign=foreign, mixed=mixed)


def by_frame(items, st):
    st = copy.deepcopy(st)
    for it in items:
        P.handle(it, st)
    return st


def by_events(batches, st):
    st = copy.deepcopy(st)
    base = 0
    for b in batches:
        evs = P.fold(b, base)
        # through the event's bytes: what a caller of emurx_ping_dev gets
        P.replay(P.events_from_array(P.events_array(evs)), st)
        base += len(b)
    return st


def drop_empty(st):
    """Counter rows a frame-by-frame run never touched and a replay created (or the reverse) hold zeros."""
    return {k: v for k, v in st.ns.items() if any(v.values())}, st.pings


@pytest.mark.parametrize("capture", sorted(K.FIXTURE))
def test_captures_give_the_recorded_stats(oracle_built, capture):
    fx = K.FIXTURE[capture]
    fam, envname = fx["family"], fx["env"]
    frames = K.fixture_frames(capture)
    buf, desc, rec = classify_with(lambda o: S.load_env(o, envname), frames)
    assert (rec["status"] == 0).all() and (rec["proto"] == (P.CB_ICMP if fam == 4 else P.CB_ICMPV6)).all()
    items = P.batch_items(buf, desc, rec, K.sim_env(envname), abi.PNGK_ALL, P.SIM_NOW)
    assert [it.outcome for it in items] == [abi.PNG_REPLY] * 5 and all(it.cls == P.CLS_OK for it in items)
    assert [it.key for it in items] == [(0, 0, fam, P.SIM_IDENT)] * 5
    assert [it.seq for it in items] == [P.SIM_SEQ + i for i in range(5)] and all(it.lat == 1_000_000 for it in items)
    want = {k: fx["stats"][k] for k in ("repliesInOrder", "minLatency", "maxLatency", "avgLatency")}
    assert want == dict(repliesInOrder=5, minLatency=1000, maxLatency=1000, avgLatency=1000)
    st0 = P.State(pings={(0, fam): P.Ping()})
    a = by_frame(items, st0)
    assert P.stats(a.pings[(0, fam)]) == want
    assert a.ns[(0, fam)]["pktRxIcmpResponse"] == fx["counters"]["pktRxIcmpResponse"] == 5
    assert sum(a.ns[(0, fam)].values()) == 5
    evs = P.fold(items)
    assert len(evs) == 1 and (evs[0]["n_ok"], evs[0]["n_succ"], evs[0]["seq_first"], evs[0]["seq_last"]) == \
        (5, 4, P.SIM_SEQ, P.SIM_SEQ + 4)
    for cut in range(6):
        b = by_events([items[:cut], items[cut:]], st0)
        assert b == a, cut


def test_matrix(oracle_built):
    m = K.matrix()
    items, rec = items_of([f for _, f, _, _ in m])
    for (name, _, outcome, cls), it, r in zip(m, items, rec):
        assert it.outcome == outcome, (name, it, r)
        if cls is not None:
            assert it.cls == cls, (name, it)
    lk = {name: (int(r["flags"]) >> 4) & 7 for (name, _, _, _), r in zip(m, rec)}
    assert lk["v4-no-client"] == abi.LK["NO_CLIENT"] and lk["v4-no-plugin"] == abi.LK["CLIENT"]
    assert lk["v6-ok"] == abi.LK["NS_LEVEL"] and lk["v6-echo-request"] != abi.LK["NS_LEVEL"]
    byname = {name: it for (name, _, _, _), it in zip(m, items)}
    assert byname["v4-ts-now"].lat == 0 and byname["v4-ts-5s"].lat == abi.PING_TIMEOUT_NS
    assert byname["v4-unreach-3"].key == (1, K.client(1, 1)[0], 4, 0x2003)
    assert byname["v6-unreach-6"].key == (1, K.client(1, 2)[0], 6, 0x3006)
    assert byname["v6-ok"].key == (0, K.client(0, 0)[0], 6, 0x1234) and byname["v6-ok"].seq == 1
    assert byname["v4-src-mcast"].key == (0, abi.PING_NS_LEVEL, 4, 0) and byname["v6-no-client"].key == (0, abi.PING_NS_LEVEL, 6, 0)
    # the families alone: the other family's frames are NONE
    for fams, keep in ((abi.PNGK_V4, 4), (abi.PNGK_V6, 6)):
        alone, _ = items_of([f for _, f, _, _ in m], fams=fams)
        for it, both in zip(alone, items):
            mine = both.key[2] == keep if both.key else both.why.startswith("v%d" % keep)
            assert it.outcome == (both.outcome if mine else abi.PNG_NONE)


@pytest.fixture(scope="module")
def stream_items(oracle_built):
    items, _ = items_of(K.stream(300))
    oc = [it.outcome for it in items]
    assert all(oc.count(k) >= 5 for k in range(6))
    assert {it.cls for it in items} == {0, 1, 2, 3} and sum(it.cls == P.CLS_OK and it.lat == 0 for it in items) >= 10
    return items


@pytest.mark.parametrize("which", ["running", "absent", "foreign", "mixed"])
def test_replay_of_fold_equals_frame_by_frame_at_every_cut(stream_items, which):
    st0 = states()[which]
    want = drop_empty(by_frame(stream_items, st0))
    if which == "running":
        pg = want[1][(K.client(0, 0)[0], 4)]
        assert pg.repliesInOrder > 5 and pg.repliesOutOfOrder > 2 and pg.repliesBadIdentifier > 5 and pg.repliesBadLatency and \
            pg.repliesMalformedPkt and pg.dstUnreachable
    for cut in range(len(stream_items) + 1):
        got = drop_empty(by_events([stream_items[:cut], stream_items[cut:]], st0))
        assert got == want, cut


def _ok(seq, lat, key=(0, 0, 4, P.SIM_IDENT)):
    return P.Item(abi.PNG_REPLY, key, seq, P.CLS_OK, lat)


@pytest.mark.parametrize("lats", [[0, 5, 3], [5, 0, 3, 9], [5, 3, 0], [0], [0, 0, 7], [4, 6, 2], [7, 0, 0]])
def test_zero_latency_first_middle_last(lats):
    items = [_ok(P.SIM_SEQ + i, lat) for i, lat in enumerate(lats)]
    e = P.fold(items)[0]
    tail = lats[len(lats) - lats[::-1].index(0):] if 0 in lats else lats
    assert e["lat_min_tail"] == (min(tail) if tail else 0) and e["flags"] == int(0 in lats)
    assert e["lat_sum"] == sum(lats) and e["lat_max"] == max(lats)
    for prior in (0, 1, 100):
        st0 = P.State(pings={(0, 4): P.Ping(minLatency=prior, firstReplyReceived=prior != 0, lastSeqReceived=P.SIM_SEQ - 1)})
        for cut in range(len(items) + 1):
            assert by_events([items[:cut], items[cut:]], st0) == by_frame(items, st0)


def test_sequence_wrap_and_order():
    items = [_ok(s, 10) for s in (0xFFFE, 0xFFFF, 0, 1, 1, 3, 2, 3)]
    e = P.fold(items)[0]
    assert (e["n_ok"], e["n_succ"], e["seq_first"], e["seq_last"]) == (8, 4, 0xFFFE, 3)
    st0 = P.State(pings={(0, 4): P.Ping(startingSeq=0xFFFE)})
    a = by_frame(items, st0).pings[(0, 4)]
    assert (a.repliesInOrder, a.repliesOutOfOrder, a.lastSeqReceived) == (5, 3, 3)
    assert by_events([items[:2], items[2:]], st0).pings[(0, 4)] == a
    # every other order of a strictly ascending run has fewer successors
    asc = [_ok((0xFFF0 + i) & 0xFFFF, 10) for i in range(40)]
    assert P.fold(asc)[0]["n_succ"] == 39
    rng = np.random.default_rng(3)
    for _ in range(20):
        perm = rng.permutation(40)
        if (perm == np.arange(40)).all():
            continue
        assert P.fold([asc[j] for j in perm])[0]["n_succ"] < 39


def test_events_are_in_ascending_last_and_cover_every_folded_frame(stream_items):
    evs = P.fold(stream_items)
    assert [e["last"] for e in evs] == sorted(e["last"] for e in evs) and len({e["key"] for e in evs}) == len(evs)
    n = sum(e["n_reply"] + e["n_unreach"] + e["n_no_client"] + e["n_mcast"] for e in evs)
    assert n == sum(1 <= it.outcome <= 4 for it in stream_items)
    for e in evs:
        assert e["n_reply"] == e["n_malformed"] + e["n_bad_latency"] + e["n_ok"]
        assert (e["key"][1] == abi.PING_NS_LEVEL) == bool(e["n_no_client"] + e["n_mcast"])
    outcome, ev, info = P.batch_of_items(stream_items, ev_cap=len(evs) - 1)
    assert len(ev) == 0 and tuple(int(x) for x in info[:3]) == (0, len(evs), 1) and int(info[3:].sum()) == \
        sum(it.outcome != 0 for it in stream_items)

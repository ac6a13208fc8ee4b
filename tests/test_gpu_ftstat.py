"""GPU parity of emurx_ftstat_dev against ft_ref: d_ev[:info[0]], d_outcome and d_info byte-equal
through the C-ABI; nothing written before d_ev, past the events written or behind d_info.  Records
and flow words come from emurx_classify_dev on the same handle (and equal the oracle's), except
where a test hands the device records it has edited."""
import numpy as np
import pytest

import ft_cases as K
import ft_ref as R
from emurx import abi
from emurx import frames as F
from test_gpu_respond import SENTINEL

pytestmark = pytest.mark.gpu

GUARD = 96  # bytes before and behind d_ev (two events), and 4 words behind d_info, that must stay untouched
EV = abi.FT_EV_DTYPE.itemsize
MAX_FRAMES = 1 << 12


def ftstat(rx, c, n, ev_cap, outcome=True, sync=True):
    """One emurx_ftstat_dev call into sentinel-filled buffers -> dict (numpy after finish())."""
    import torch
    ev = torch.full((GUARD + ev_cap * EV + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    oc = torch.full((max(n, 1),), SENTINEL, dtype=torch.uint8, device="cuda") if outcome else None
    info = torch.full((abi.FT_INFO_WORDS + 4,), -1, dtype=torch.int64, device="cuda")
    rx.ftstat_dev(c["tb"], c["td"], c["trec"], c["tflow"], n, ev[GUARD:], ev_cap, oc, info)
    got = dict(ev=ev, oc=oc, info=info, n=n)
    return finish(got) if sync else got


def finish(got):
    import torch
    torch.cuda.synchronize()
    raw = got["ev"].cpu().numpy()
    iw = got["info"].cpu().numpy().view(np.uint64)
    assert (iw[abi.FT_INFO_WORDS:] == 0xFFFFFFFFFFFFFFFF).all(), iw
    assert (raw[:GUARD] == SENTINEL).all() and (raw[-GUARD:] == SENTINEL).all()  # nothing before d_ev, nothing past ev_cap
    return dict(ev=raw[GUARD:-GUARD], outcome=None if got["oc"] is None else got["oc"].cpu().numpy()[: got["n"]],
                info=iw[: abi.FT_INFO_WORDS])


def want_of(c, n, ev_cap=None):
    return (c["oc"][:n],) + R.fold(c["oc"][:n], c["cand"][:n], c["rec"][:n], ev_cap)


def check(got, want):
    w_outcome, w_ev, w_info = want
    assert np.array_equal(got["info"], w_info), (got["info"], w_info)
    if got["outcome"] is not None:
        assert np.array_equal(got["outcome"], w_outcome), np.nonzero(got["outcome"] != w_outcome)[0][:10]
    k = int(w_info[0])
    assert k == len(w_ev)
    g = got["ev"][: k * EV].view(abi.FT_EV_DTYPE)
    assert g.tobytes() == w_ev.tobytes(), next((j, g[j], w_ev[j]) for j in range(k) if g[j] != w_ev[j])
    assert (got["ev"][k * EV:] == SENTINEL).all()  # entries past the events written are untouched
    return g


def upload(buf, desc, rec, flow, tb=None, td=None):
    """A case from host arrays: the device copies and ft_ref's outcomes for them."""
    from gpu_util import to_dev
    oc, cand = R.outcomes(buf, desc, rec, flow, K.MAX_NS, K.MAX_CLIENTS)
    return dict(tb=to_dev(buf) if tb is None else tb, td=to_dev(desc) if td is None else td, trec=to_dev(rec), tflow=to_dev(flow),
                rec=rec, desc=desc, flow=flow, buf=buf, oc=oc, cand=cand, n=len(desc))


def make_case(h, frames, holes=0):
    """The frames classified on the device, flow words included; both equal the oracle's."""
    from gpu_util import run_dev
    buf, desc = F.pack_frames(frames, [1] * len(frames))
    if holes:
        desc["pad"][holes - 1::holes] = abi.DESC_HOLE
    rec, _, _, _, flow = run_dev(h["rx"], buf, desc, flows=True)
    orec, _, _, _ = h["orc"].rx_batch(buf, desc)
    live = desc["pad"] != abi.DESC_HOLE  # the oracle knows no holes: the device's records of them say ST_HOLE
    assert rec[live].tobytes() == orec[live].tobytes() and (rec["status"][~live] == abi.ST_HOLE).all()
    assert np.array_equal(flow[live], h["orc"].flows(buf, desc, orec)[live])
    return upload(buf, desc, rec.copy(), flow.copy())


def run(h, c, n=None, ev_cap=None, **kw):
    """The first n frames of case c through the device, checked against ft_ref -> the events."""
    n = c["n"] if n is None else n
    want = want_of(c, n, ev_cap)
    cap = max(len(want[1]), 1) if ev_cap is None else ev_cap
    return check(ftstat(h["rx"], c, n, cap, **kw), want), want


@pytest.fixture(scope="module")
def h(gpu_ok, oracle_built):
    from emurx.rx import RxPath
    rx = RxPath(0, max_ns=K.MAX_NS, max_clients=K.MAX_CLIENTS, max_frames=MAX_FRAMES)
    rx.register_all()
    orc = oracle_built.Oracle()
    for t in (rx, orc):
        K.load_tables(t)
        K.load_flows(t)
    h = dict(rx=rx, orc=orc)
    near, near_cids = K.near_clients()
    h.update(stream=make_case(h, K.stream(700), holes=37), matrix=make_case(h, [f for _, f, _ in K.matrix()]),
             none=make_case(h, [K.arp(i % 5) if i % 3 else K.l4(K.FLOW_CLIENTS[i & 1], 17, bool(i & 2), sport=K.FLOW_SPORT)
                                for i in range(300)]),
             arp=make_case(h, [K.arp(i % 9) for i in range(300)]),
             one1025=make_case(h, K.one_client(1025)), one2049=make_case(h, K.one_client(2049)),
             two=make_case(h, K.interleaved(1100, 2)), three=make_case(h, K.interleaved(1100, 3)),
             near=make_case(h, near), near_cids=near_cids, d600=make_case(h, K.distinct(600)), d300=make_case(h, K.distinct(300)))
    yield h
    rx.close()


def test_rule_matrix(h):
    c = h["matrix"]
    m = K.matrix()
    assert [int(o) & 7 for o in c["oc"]] == [w for _, _, w in m]  # the device's records and flow words give every branch
    ev, want = run(h, c)
    assert {int(e["client_id"]) for e in ev} == {1, 2, 3, K.N_CLIENTS + 1} and int(want[2][6]) == 12 and int(want[2][7]) == 8
    e1 = ev[ev["client_id"] == 1][0]  # client 1: NO_SYN and NO_SRV_TCP in both families
    assert list(map(int, e1["cnt"])) == [2, 2, 4, 2, 0, 2, 0] and int(e1["frames"]) == 4 and int(e1["ns_id"]) == 0
    assert int(ev[ev["client_id"] == K.N_CLIENTS + 1][0]["ns_id"]) == 1


def test_no_candidate_then_a_batch(h):
    """A batch without a refused frame (found flows and ARP): an all-zero outcome, no event, info
    counts the candidates alone; the call behind it is unaffected."""
    c, s = h["none"], h["stream"]
    got = ftstat(h["rx"], c, 300, 8, sync=False)
    nxt = ftstat(h["rx"], s, 700, len(want_of(s, 700)[1]), sync=False)
    got = finish(got)
    assert list(map(int, got["info"])) == [0] * 7 + [100] and not got["outcome"].any() and (got["ev"] == SENTINEL).all()
    check(got, want_of(c, 300))
    check(finish(nxt), want_of(s, 700))


def test_no_candidate_at_all(h):
    """300 ARP requests: no frame is a candidate, every word of d_info and every outcome is zero, no
    event; the fold behind it on the same handle is unaffected."""
    c = h["arp"]
    assert not c["cand"].any() and (c["rec"]["proto"] == abi.CB_ARP).all()
    for n in (300, 256, 1):
        got = ftstat(h["rx"], c, n, 4)
        assert not got["info"].any() and not got["outcome"].any() and (got["ev"] == SENTINEL).all()
        check(got, want_of(c, n))
    run(h, h["stream"])


def test_holes_and_every_outcome(h):
    c = h["stream"]
    hole = c["desc"]["pad"] == abi.DESC_HOLE
    assert hole.sum() >= 15 and not c["oc"][hole].any() and not c["cand"][hole].any()
    ev, want = run(h, c)
    assert all(((want[0] & 7) == k).sum() >= 30 for k in range(5)) and len(ev) >= 8 and (want[0] & abi.FT_V6).sum() >= 100


def test_bad_records(h):
    """Records and flow words the classifier never writes: a client_id or ns_id out of range, l3 at
    or past the frame's end or inside the Ethernet header, NO_SYN on a udp record, refusing flow
    words on records whose lookup is not CLIENT, holes whose records look alive, FLOW_UNKNOWN."""
    s = h["stream"]
    rec, flow, desc = s["rec"].copy(), s["flow"].copy(), s["desc"].copy()
    folds = np.nonzero((s["oc"] & 7 >= 1) & (s["oc"] & 7 <= 3))[0]
    assert len(folds) >= 120
    f = iter(folds)
    edits = {}
    for name in ("cid", "cid_edge", "ns", "l3_end", "l3_past", "l3_low", "udp_no_syn", "lk_ns_level", "lk_none", "lk_no_client",
                 "hole", "unknown", "flow_none", "flow_id", "status"):
        for _ in range(4):
            i = int(next(f))
            edits.setdefault(name, []).append(i)
            lkbits = int(rec[i]["flags"]) & ~0x70  # EMURX_FLAG_LK_MASK
            if name == "cid":
                rec[i]["client_id"] = 0xFFFFFFF0
            elif name == "cid_edge":
                rec[i]["client_id"] = K.MAX_CLIENTS
            elif name == "ns":
                rec[i]["ns_id"] = K.MAX_NS
            elif name == "l3_end":
                rec[i]["l3"] = desc[i]["len"]
            elif name == "l3_past":
                rec[i]["l3"] = 0xFFFF
            elif name == "l3_low":
                rec[i]["l3"] = 13
            elif name == "udp_no_syn":
                rec[i]["proto"], flow[i] = abi.CB_UDP, abi.FLOW_NO_SYN
            elif name == "lk_ns_level":
                rec[i]["flags"] = lkbits | abi.LK["NS_LEVEL"] << 4
            elif name == "lk_none":
                rec[i]["flags"] = lkbits | abi.LK["NONE"] << 4
            elif name == "lk_no_client":
                rec[i]["flags"] = lkbits | abi.LK["NO_CLIENT"] << 4
            elif name == "hole":
                desc[i]["pad"] = abi.DESC_HOLE
            elif name == "unknown":
                flow[i] = abi.FLOW_UNKNOWN
            elif name == "flow_none":
                flow[i] = abi.FLOW_NONE
            elif name == "flow_id":
                flow[i] = 7
            else:
                rec[i]["status"] = 1
    c = upload(s["buf"], desc, rec, flow, tb=s["tb"])
    for name, idx in edits.items():
        w = abi.FT_ERR if name == "lk_no_client" else abi.FT_NONE
        assert (c["oc"][idx] == w).all(), name
        assert c["cand"][idx].all() != (name in ("hole", "status")), name
    # l3 one below the end still reads its byte, the frame's last
    i = int(next(f))
    c["rec"][i]["l3"] = int(desc[i]["len"]) - 1
    c = upload(s["buf"], desc, c["rec"], flow, tb=s["tb"])
    assert 1 <= c["oc"][i] & 7 <= 3
    ev, want = run(h, c)
    assert len(ev) >= 6 and int(want[2][7]) > int(want_of(s, 700)[2][7])


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257])
def test_sizes(h, n):
    run(h, h["stream"], n=n)
    run(h, h["two"], n=n)
    run(h, h["d300"], n=n)


@pytest.mark.parametrize("case,n", [("one1025", 1025), ("one2049", 2049)])
def test_one_client_in_every_frame(h, case, n):
    ev, want = run(h, h[case], ev_cap=1)
    e = ev[0]
    assert (int(e["frames"]), int(e["first"]), int(e["last"]), int(e["client_id"])) == (n, 0, n - 1, 9)
    assert int(e["cnt"][0]) + int(e["cnt"][1]) == n and int(e["cnt"][2]) + int(e["cnt"][4]) == n and min(map(int, e["cnt"][:6])) > 100


@pytest.mark.parametrize("case", ["two", "three"])
def test_clients_interleaved_lane_by_lane(h, case):
    k = 2 if case == "two" else 3
    ev, _ = run(h, h[case], n=1024)
    assert len(ev) == k and (ev["frames"] >= 1024 // k).all() and sorted(map(int, ev["last"])) == list(range(1024 - k, 1024))
    for n in (1023, 1025, 1100):
        run(h, h[case], n=n)


def test_client_ids_that_differ_in_one_bit(h):
    ev, _ = run(h, h["near"])
    assert len(ev) == 6 and (ev["frames"] == 3).all() and {int(e["client_id"]) for e in ev} == set(h["near_cids"])
    assert [int(e["cnt"][0]) for e in ev] == [2] * 6 and [int(e["cnt"][1]) for e in ev] == [1] * 6


def test_600_distinct_clients_in_consecutive_frames(h):
    ev, _ = run(h, h["d600"])
    assert len(ev) == 600 and (ev["frames"] == 1).all() and (ev["first"] == ev["last"]).all() and (ev["last"] == np.arange(600)).all()


@pytest.mark.parametrize("short", [0, 1], ids=["exact", "one-below"])
def test_distinct_clients_and_overflow(h, short):
    """ev_cap equal to the 300 distinct clients: every event; 299: overflow, info[0] 0, nothing
    written (d_ev and the guard bytes around it keep their fill), outcomes and counts valid."""
    c = h["d300"]
    want = want_of(c, 300, 300 - short)
    assert tuple(int(x) for x in want[2][:3]) == (0 if short else 300, 300, short) and int(want[2][3:6].sum()) == 300
    got = ftstat(h["rx"], c, 300, 300 - short)
    check(got, want)
    if short:
        assert (got["ev"] == SENTINEL).all()
        run(h, c)  # the overflowing call left no residue
        run(h, h["stream"])


def test_same_call_twice_and_without_outcome(h):
    c = h["stream"]
    cap = len(want_of(c, 700)[1])
    a = ftstat(h["rx"], c, 700, cap, sync=False)
    b = ftstat(h["rx"], c, 700, cap, sync=False)
    o = ftstat(h["rx"], c, 700, cap, outcome=False, sync=False)
    a, b, o = finish(a), finish(b), finish(o)
    assert a["ev"].tobytes() == b["ev"].tobytes() == o["ev"].tobytes() and a["outcome"].tobytes() == b["outcome"].tobytes()
    assert np.array_equal(a["info"], b["info"]) and np.array_equal(a["info"], o["info"]) and o["outcome"] is None
    check(a, want_of(c, 700))


def test_rows_of_an_earlier_call_are_not_read(h):
    """Three calls; in the second, the tile of frames 256..511 folds nothing and sits between tiles
    that fold, while the first call folded in all of them: its row indices are still there."""
    full = [K.l4(9 + (i & 1), 6, False, flags=K.ACK) for i in range(768)]
    gap = list(full)
    gap[256:512] = [K.l4(K.FLOW_CLIENTS[i & 1], 17, False, sport=K.FLOW_SPORT) for i in range(256)]
    b1, b2 = make_case(h, full), make_case(h, gap)
    e1, _ = run(h, b1)
    e2, _ = run(h, b2)
    e3, _ = run(h, b1)
    assert [int(e["frames"]) for e in e1] == [384, 384] and e3.tobytes() == e1.tobytes()
    assert [(int(e["frames"]), int(e["first"]), int(e["last"])) for e in e2] == [(256, 0, 766), (256, 1, 767)]
    run(h, h["stream"])  # and a batch of another shape behind them


def test_arguments(h):
    import torch
    c = h["near"]
    rx = h["rx"]
    ev = torch.zeros(EV * 8, dtype=torch.uint8, device="cuda")
    info = torch.zeros(abi.FT_INFO_WORDS, dtype=torch.int64, device="cuda")
    lib, P_ = rx.lib, abi.ptr
    assert rx.ftstat_max_events() == min(MAX_FRAMES, K.MAX_CLIENTS)

    def call(n=c["n"], cap=8, stream=None, fl=c["tflow"]):
        return lib.emurx_ftstat_dev(rx.h, P_(c["tb"]), P_(c["td"]), P_(c["trec"]), P_(fl), n, P_(ev), cap, None, P_(info), stream)

    assert call(n=MAX_FRAMES + 1) == abi.EMURX_ENOMEM
    assert call(cap=0) == abi.EMURX_EINVAL and call(cap=rx.ftstat_max_events() + 1) == abi.EMURX_EINVAL
    assert call(fl=None) == abi.EMURX_EINVAL
    info.fill_(-1)
    assert call(n=0) == 0
    torch.cuda.synchronize()
    assert not info.cpu().numpy().any()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        rc = call(stream=s.cuda_stream)  # a capturing stream: refused before anything is enqueued
    assert rc == abi.EMURX_EINVAL
    run(h, c)

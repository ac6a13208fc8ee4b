"""GPU parity of emurx_ping_dev against ping_ref.fold, and through it against the reference's ping
simulations: d_ev[:info[0]], d_outcome and d_info byte-equal through the C-ABI; nothing written
before d_ev, past the events written or behind d_info.  Records come from emurx_classify_dev on
the same handle."""
import numpy as np
import pytest

import ping_cases as K
import ping_ref as P
import respond_ref as R
import sim_envs as S
from emurx import abi
from test_gpu_respond import SENTINEL, classify

pytestmark = pytest.mark.gpu

GUARD = 160  # bytes before and behind d_ev (two events), and 4 words behind d_info, that must stay untouched
EV = abi.PING_EV_DTYPE.itemsize


def ping(rx, tb, td, trec, n, ev_cap, now=K.NOW, fams=abi.PNGK_ALL, outcome=True, sync=True):
    """One emurx_ping_dev call into sentinel-filled buffers -> dict (numpy after finish())."""
    import torch
    ev = torch.full((GUARD + ev_cap * EV + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    oc = torch.full((max(n, 1),), SENTINEL, dtype=torch.uint8, device="cuda") if outcome else None
    info = torch.full((abi.PNG_INFO_WORDS + 4,), -1, dtype=torch.int64, device="cuda")
    rx.ping_dev(tb, td, trec, n, now, ev[GUARD:], ev_cap, oc, info, fams=fams)
    got = dict(ev=ev, oc=oc, info=info, n=n)
    return finish(got) if sync else got


def finish(got):
    import torch
    torch.cuda.synchronize()
    raw = got["ev"].cpu().numpy()
    iw = got["info"].cpu().numpy().view(np.uint64)
    assert (iw[abi.PNG_INFO_WORDS:] == 0xFFFFFFFFFFFFFFFF).all(), iw
    assert (raw[:GUARD] == SENTINEL).all() and (raw[-GUARD:] == SENTINEL).all()  # nothing before d_ev, nothing past ev_cap
    return dict(ev=raw[GUARD:-GUARD], outcome=None if got["oc"] is None else got["oc"].cpu().numpy()[: got["n"]],
                info=iw[: abi.PNG_INFO_WORDS])


def check(got, want):
    """got: ping(); want: ping_ref.batch_of_items() for the same ev_cap."""
    w_outcome, w_ev, w_info = want
    assert np.array_equal(got["info"], w_info), (got["info"], w_info)
    if got["outcome"] is not None:
        assert np.array_equal(got["outcome"], w_outcome), np.nonzero(got["outcome"] != w_outcome)[0][:10]
    k = int(w_info[0])
    assert k == len(w_ev)
    g = got["ev"][: k * EV].view(abi.PING_EV_DTYPE)
    assert g.tobytes() == w_ev.tobytes(), next((j, g[j], w_ev[j]) for j in range(k) if g[j] != w_ev[j])
    assert (got["ev"][k * EV:] == SENTINEL).all()  # entries past the events written are untouched
    return g


def make_case(rx, env, frames, holes=0, now=K.NOW):
    buf, desc = R.pack_with_holes(frames, [1] * len(frames), holes)
    tb, td, trec, rec = classify(rx, buf, desc)
    items = {f: P.batch_items(buf, desc, rec, env, f, now) for f in (1, 2, 3)}
    return dict(rx=rx, tb=tb, td=td, trec=trec, rec=rec, desc=desc, items=items, n=len(desc), now=now)


def run(c, n=None, ev_cap=None, fams=abi.PNGK_ALL, **kw):
    """The first n frames of case c through the device, checked against the reference -> the events."""
    n = c["n"] if n is None else n
    want = P.batch_of_items(c["items"][fams][:n], ev_cap)
    cap = max(len(want[1]), 1) if ev_cap is None else ev_cap
    return check(ping(c["rx"], c["tb"], c["td"], c["trec"], n, cap, c["now"], fams, **kw), want), want


@pytest.fixture(scope="module")
def h(gpu_ok, oracle_built):
    """The handle with ping_cases' tables, its Env twin and the cases classified once."""
    from emurx.rx import RxPath
    rx = RxPath(0, max_ns=16, max_clients=64, max_frames=1 << 12)
    rx.register_all()
    env = P.Env()
    K.load_tables(rx, env)
    cases = dict(stream=make_case(rx, env, K.stream(600), holes=37), matrix=make_case(rx, env, [f for _, f, _, _ in K.matrix()]),
                 none=make_case(rx, env, [K.arp_request(i % 2) for i in range(300)]),
                 one1025=make_case(rx, env, K.one_key(1025)), one2049=make_case(rx, env, K.one_key(2049, 0xF900)),
                 two=make_case(rx, env, K.interleaved(1100, 2)), three=make_case(rx, env, K.interleaved(2100, 3)),
                 near=make_case(rx, env, K.near_keys()), distinct=make_case(rx, env, K.distinct_keys(300)))
    yield dict(rx=rx, env=env, **cases)
    rx.close()


@pytest.mark.parametrize("capture", sorted(K.FIXTURE))
def test_ping_captures_fold_and_replay_to_the_recorded_stats(gpu_ok, oracle_built, capture):
    from emurx.rx import RxPath
    fx = K.FIXTURE[capture]
    fam = fx["family"]
    rx = RxPath(0, max_ns=16, max_clients=16, max_frames=1 << 10)
    rx.register_all()
    S.load_env(rx, fx["env"])
    c = make_case(rx, K.sim_env(fx["env"]), K.fixture_frames(capture), now=P.SIM_NOW)
    ev, want = run(c, ev_cap=4)
    assert len(ev) == 1 and int(ev[0]["n_ok"]) == 5 and int(ev[0]["n_succ"]) == 4 and int(ev[0]["family"]) == fam
    st = P.State(pings={(0, fam): P.Ping()})
    P.replay(P.events_from_array(ev), st)
    assert P.stats(st.pings[(0, fam)]) == {k: fx["stats"][k] for k in ("repliesInOrder", "minLatency", "maxLatency", "avgLatency")}
    assert st.ns[(0, fam)]["pktRxIcmpResponse"] == fx["counters"]["pktRxIcmpResponse"] == 5
    rx.close()


def test_ping_rule_matrix(h):
    c = h["matrix"]
    m = K.matrix()
    assert [it.outcome for it in c["items"][3]] == [o for _, _, o, _ in m]  # the device's records give the oracle's outcomes
    for fams in (3, 1, 2):
        run(c, fams=fams)


def test_ping_no_candidate_then_a_batch(h):
    """A batch without candidates: an all-zero info and outcome, no event; the call behind it is unaffected."""
    got = ping(h["rx"], h["none"]["tb"], h["none"]["td"], h["none"]["trec"], 300, 8, sync=False)
    nxt = ping(h["rx"], h["stream"]["tb"], h["stream"]["td"], h["stream"]["trec"], 600,
               len(P.fold(h["stream"]["items"][3])), sync=False)
    got = finish(got)
    assert not got["info"].any() and not got["outcome"].any() and (got["ev"] == SENTINEL).all()
    check(finish(nxt), P.batch_of_items(h["stream"]["items"][3]))


def test_ping_holes_and_bad_records_are_skipped(h):
    c = h["stream"]
    hole = c["desc"]["pad"] == abi.DESC_HOLE
    bad = c["rec"]["status"] != 0
    oc = np.array([it.outcome for it in c["items"][3]])
    assert hole.sum() >= 10 and (bad & ~hole).sum() >= 10 and not oc[hole | bad].any()
    ev, want = run(c)
    assert all((want[0] == k).sum() >= 5 for k in range(6)) and len(ev) >= 8


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_ping_sizes(h, n):
    run(h["stream"], n=n)
    run(h["two"], n=n)


@pytest.mark.parametrize("case,n", [("one1025", 1025), ("one2049", 2049)])
def test_ping_one_key_in_every_frame(h, case, n):
    """One ping's replies in ascending sequence across the wrap: n_succ = n - 1, which no other
    order of the frames gives; 2,049 is one frame past two steps of the ordered pass."""
    ev, _ = run(h[case], ev_cap=1)
    e = ev[0]
    assert (int(e["n_ok"]), int(e["n_succ"]), int(e["first"]), int(e["last"])) == (n, n - 1, 0, n - 1) and int(e["flags"]) == 1
    assert int(e["lat_min_tail"]) == 1000 + 7 * (n // 3 + 1)  # the minimum behind the zero latency


@pytest.mark.parametrize("case", ["two", "three"])
def test_ping_keys_interleaved_lane_by_lane(h, case):
    k = 2 if case == "two" else 3
    ev, _ = run(h[case])
    assert len(ev) == k and (ev["n_succ"] > 100).all() and (ev["n_succ"] < ev["n_ok"] - 10).all() and (ev["flags"] == 1).all()
    for n in (1023, 1024, 1025):
        run(h[case], n=n)


def test_ping_keys_that_differ_in_one_field(h):
    ev, _ = run(h["near"])
    assert len(ev) == 6 and (ev["n_reply"] + ev["n_unreach"] == 3).all()
    keys = {(int(e["client_id"]), int(e["family"]), int(e["ident"])) for e in ev}
    c0, c1 = K.client(0, 0)[0], K.client(0, 1)[0]
    assert keys == {(c0, 4, 0x1234), (c0, 4, 0x1235), (c0, 6, 0x1234), (c1, 4, 0x1234), (c1, 6, 0x1234), (c0, 4, 0x1236)}


@pytest.mark.parametrize("short", [0, 1], ids=["exact", "one-below"])
def test_ping_distinct_keys_and_overflow(h, short):
    """ev_cap equal to the 300 distinct keys: every event; 299: overflow, info[0] 0, nothing written
    (d_ev and the guard bytes around it keep their fill), outcomes and the rest of d_info valid."""
    c = h["distinct"]
    want = P.batch_of_items(c["items"][3], 300 - short)
    assert tuple(int(x) for x in want[2][:4]) == (0 if short else 300, 300, short, 300)
    got = ping(h["rx"], c["tb"], c["td"], c["trec"], 300, 300 - short)
    check(got, want)
    if short:
        assert (got["ev"] == SENTINEL).all()
        run(c)  # the overflowing call left no residue


def test_ping_same_call_twice_and_without_outcome(h):
    c = h["stream"]
    cap = len(P.fold(c["items"][3]))
    a = ping(h["rx"], c["tb"], c["td"], c["trec"], 600, cap, sync=False)
    b = ping(h["rx"], c["tb"], c["td"], c["trec"], 600, cap, sync=False)
    o = ping(h["rx"], c["tb"], c["td"], c["trec"], 600, cap, outcome=False, sync=False)
    a, b, o = finish(a), finish(b), finish(o)
    assert a["ev"].tobytes() == b["ev"].tobytes() == o["ev"].tobytes() and a["outcome"].tobytes() == b["outcome"].tobytes()
    assert np.array_equal(a["info"], b["info"]) and o["outcome"] is None
    check(a, P.batch_of_items(c["items"][3]))


def test_ping_marks_of_an_earlier_call_are_not_read(h):
    """The ordered pass walks 1,024 frames a step; a tile of a step that folds nothing in this
    call still holds the row indices and marks of an earlier one."""
    b1, b2, b3 = (make_case(h["rx"], h["env"], fr) for fr in K.stale_marks())
    e1, _ = run(b1)
    e2, _ = run(b2)
    e3, _ = run(b3)
    assert [(int(e["n_ok"]), int(e["n_succ"])) for e in e1] == [(256, 255)] and e3.tobytes() == e1.tobytes()
    assert [(int(e["n_ok"]), int(e["n_succ"]), int(e["first"]), int(e["last"])) for e in e2] == [(4, 3, 10, 700)]
    run(h["stream"])  # and a batch of another shape behind them


def test_ping_arguments(h):
    import torch
    c = h["near"]
    rx = h["rx"]
    ev = torch.zeros(EV * 8, dtype=torch.uint8, device="cuda")
    info = torch.zeros(abi.PNG_INFO_WORDS, dtype=torch.int64, device="cuda")
    lib, P_ = rx.lib, abi.ptr

    def call(n=c["n"], fams=3, now=K.NOW, cap=8, stream=None):
        return lib.emurx_ping_dev(rx.h, P_(c["tb"]), P_(c["td"]), P_(c["trec"]), n, fams, now, P_(ev), cap, None, P_(info), stream)

    assert call(n=(1 << 12) + 1) == abi.EMURX_ENOMEM
    assert call(fams=0) == abi.EMURX_EINVAL and call(now=1 << 63) == abi.EMURX_EINVAL and call(cap=0) == abi.EMURX_EINVAL
    assert call(cap=rx.ping_max_events() + 1) == abi.EMURX_EINVAL
    info.fill_(-1)
    assert call(n=0) == 0
    torch.cuda.synchronize()
    assert not info.cpu().numpy().any()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        rc = call(stream=s.cuda_stream)  # a capturing stream: refused before anything is enqueued
    assert rc == abi.EMURX_EINVAL
    run(c)

"""GPU parity of emurx_learn_dev against learn_ref, and through it against the reference's
captures: d_ev[:info[0]], d_outcome and d_info bit-exact; nothing written before d_ev, past the
events written or behind d_info.  Records come from emurx_classify_dev on the same handle."""
import numpy as np
import pytest

import learn_ref as L
import nd_ref as N
import respond_ref as R
import sim_envs as S
from emurx import abi, frames as F
from test_gpu_respond import SENTINEL, classify
from test_learn_ref import A, B, IP1, arp_frame, capture_case

pytestmark = pytest.mark.gpu

GUARD = 64  # bytes before and behind d_ev, and 4 words behind d_info, that must stay untouched


def learn(rx, tb, td, trec, n, ev_cap, kinds=abi.LRNK_ALL, outcome=True, sync=True):
    """One emurx_learn_dev call into sentinel-filled buffers -> dict (numpy after finish())."""
    import torch
    ev = torch.full((GUARD + ev_cap * 40 + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    oc = torch.full((max(n, 1),), SENTINEL, dtype=torch.uint8, device="cuda") if outcome else None
    info = torch.full((abi.LRN_INFO_WORDS + 4,), -1, dtype=torch.int64, device="cuda")
    rx.learn_dev(tb, td, trec, n, ev[GUARD:], ev_cap, oc, info, kinds=kinds)
    got = dict(ev=ev, oc=oc, info=info, n=n, ev_cap=ev_cap)
    return finish(got) if sync else got


def finish(got):
    import torch
    torch.cuda.synchronize()
    raw = got["ev"].cpu().numpy()
    iw = got["info"].cpu().numpy().view(np.uint64)
    assert (iw[abi.LRN_INFO_WORDS:] == 0xFFFFFFFFFFFFFFFF).all(), iw
    assert (raw[:GUARD] == SENTINEL).all() and (raw[-GUARD:] == SENTINEL).all()  # nothing before d_ev, nothing past ev_cap
    return dict(ev=raw[GUARD:-GUARD], outcome=None if got["oc"] is None else got["oc"].cpu().numpy()[: got["n"]],
                info=iw[: abi.LRN_INFO_WORDS])


def check(got, want):
    """got: learn(); want: learn_ref.learn_batch() for the same ev_cap."""
    w_outcome, w_ev, w_info = want
    assert np.array_equal(got["info"], w_info), (got["info"], w_info)
    if got["outcome"] is not None:
        assert np.array_equal(got["outcome"], w_outcome), np.nonzero(got["outcome"] != w_outcome)[0][:10]
    k = int(w_info[0])
    assert k == len(w_ev)
    g = got["ev"][: k * 40].view(abi.LEARN_EV_DTYPE)
    assert g.tobytes() == w_ev.tobytes(), next((j, g[j], w_ev[j]) for j in range(k) if g[j] != w_ev[j])
    assert (got["ev"][k * 40:] == SENTINEL).all()  # entries past the events written are untouched


def want_prefix(m, n, kinds=abi.LRNK_ALL, ev_cap=None):
    """learn_batch of the first n frames from the per-frame reference computed once for the batch."""
    outcome, keys = m["ref"][kinds]
    ev = L.events_array(L.fold(keys[:n]))
    over = ev_cap is not None and len(ev) > ev_cap
    info = np.zeros(abi.LRN_INFO_WORDS, np.uint64)
    info[0], info[1], info[2] = 0 if over else len(ev), len(ev), int(over)
    for k in range(1, 6):
        info[2 + k] = int((outcome[:n] == k).sum())
    return outcome[:n], ev[:0] if over else ev, info


def make_case(rx, frames, vports, env6=None, holes=0, kinds=(abi.LRNK_ALL,)):
    buf, desc = R.pack_with_holes(frames, vports, holes)
    tb, td, trec, rec = classify(rx, buf, desc)
    ref = {k: L.learn_keys(buf, desc, rec, k, env6) for k in kinds}
    return dict(rx=rx, buf=buf, desc=desc, tb=tb, td=td, trec=trec, rec=rec, env6=env6, ref=ref, n=len(desc))


@pytest.fixture(scope="module")
def mixed(gpu_ok, oracle_built):
    """The learning batch's handle and its classified 4,096 frames; smaller n are prefixes."""
    from emurx.rx import RxPath
    rx = RxPath(0, max_ns=16, max_clients=64, max_frames=1 << 12)
    rx.register_all()
    env4, env6 = R.Env(), N.Env()
    N.load_combined(rx, env4, env6)
    fr, vp = L.learning_batch(4096)
    m = make_case(rx, fr, vp, env6, L.HOLE_EVERY, kinds=(1, 2, 3))
    m["env4"] = env4
    yield m
    rx.close()


@pytest.fixture(scope="module")
def arp(gpu_ok, oracle_built):
    """A handle with respond_ref's tables and the ARP-only batches of 4,096 frames."""
    from emurx.rx import RxPath
    rx = RxPath(0, max_ns=16, max_clients=64, max_frames=1 << 12)
    rx.register_all()
    R.load_tables(rx)
    one = make_case(rx, *L.arp_requests(4096, 1))
    distinct = make_case(rx, *L.arp_requests(4096, 4096))
    yield dict(rx=rx, one=one, distinct=distinct)
    rx.close()


@pytest.mark.parametrize("capture,count", [("arp4.json", 6), ("arp5.json", 6), ("arp2.json", 57)])
def test_learn_captures(gpu_ok, oracle_built, capture, count):
    from emurx.rx import RxPath
    buf, desc, orec = capture_case(capture)
    rx = RxPath(0, max_ns=16, max_clients=16, max_frames=1 << 10)
    rx.register_all()
    S.load_env(rx, "arp")
    tb, td, trec, rec = classify(rx, buf, desc)
    assert rec.tobytes() == orec.tobytes()
    want = L.learn_batch(buf, desc, rec)
    assert len(want[1]) == 1 and int(want[1][0]["count"]) == count  # learn_ref = the capture (test_learn_ref)
    check(learn(rx, tb, td, trec, len(desc), 8), want)
    rx.close()


@pytest.mark.parametrize("n", [63, 64, 65, 255, 256, 257, 4096])
def test_learn_mixed(mixed, n):
    m = mixed
    want = want_prefix(m, n, 3)
    if n >= 255:
        assert all((want[0] == k).any() for k in range(6)) and (want[1]["count"] > 1).any()
    check(learn(m["rx"], m["tb"], m["td"], m["trec"], n, max(len(want[1]), 1)), want)


def test_learn_kinds_alone_and_union(mixed):
    m, n = mixed, 4096
    a, d = want_prefix(m, n, abi.LRNK_ARP), want_prefix(m, n, abi.LRNK_ND)
    both = want_prefix(m, n, abi.LRNK_ALL)
    assert len(a[1]) > 8 and len(d[1]) > 8 and len(a[1]) + len(d[1]) == len(both[1])
    ga = learn(m["rx"], m["tb"], m["td"], m["trec"], n, len(both[1]), abi.LRNK_ARP)
    gd = learn(m["rx"], m["tb"], m["td"], m["trec"], n, len(both[1]), abi.LRNK_ND)
    gb = learn(m["rx"], m["tb"], m["td"], m["trec"], n, len(both[1]), abi.LRNK_ALL)
    check(ga, a)
    check(gd, d)
    check(gb, both)
    # the union: per frame the one outcome that is not NONE; the events merged by `last`
    assert np.array_equal(np.maximum(ga["outcome"], gd["outcome"]), gb["outcome"])
    ea = ga["ev"][: len(a[1]) * 40].view(abi.LEARN_EV_DTYPE)
    ed = gd["ev"][: len(d[1]) * 40].view(abi.LEARN_EV_DTYPE)
    merged = np.concatenate([ea, ed])
    merged = merged[np.argsort(merged["last"], kind="stable")]
    assert merged.tobytes() == gb["ev"][: len(both[1]) * 40].tobytes()
    assert np.array_equal(ga["info"][3:] + gd["info"][3:], gb["info"][3:])


def test_learn_one_key(arp):
    m = arp["one"]
    want = want_prefix(m, 4096)
    assert len(want[1]) == 1 and tuple(int(want[1][0][k]) for k in ("count", "first", "last")) == (4096, 0, 4095)
    check(learn(arp["rx"], m["tb"], m["td"], m["trec"], 4096, 1), want)


@pytest.mark.parametrize("short", [0, 1], ids=["exact", "one-below"])
def test_learn_all_distinct_and_overflow(arp, short):
    """ev_cap equal to the distinct count: every event; one below: overflow, nothing written (the
    guard bytes before and behind d_ev, and d_ev itself, keep their fill), the rest of d_info valid."""
    m = arp["distinct"]
    cap = 4096 - short
    want = want_prefix(m, 4096, ev_cap=cap)
    assert int(want[2][1]) == 4096 and int(want[2][2]) == short and int(want[2][0]) == (0 if short else 4096)
    assert int(want[2][3]) == 4096
    got = learn(arp["rx"], m["tb"], m["td"], m["trec"], 4096, cap)
    check(got, want)
    if short:
        assert (got["ev"] == SENTINEL).all()


def test_learn_small_cap_four_keys(arp):
    """ev_cap = 4 and exactly four keys among 1,024 frames."""
    from emurx.rx import RxPath  # noqa: F401
    rx = arp["rx"]
    m = make_case(rx, *L.arp_requests(1024, 4))
    want = want_prefix(m, 1024, ev_cap=4)
    assert len(want[1]) == 4 and (want[1]["count"] == 256).all() and int(want[2][2]) == 0
    check(learn(rx, m["tb"], m["td"], m["trec"], 1024, 4), want)
    over = want_prefix(m, 1024, ev_cap=3)
    assert int(over[2][2]) == 1
    check(learn(rx, m["tb"], m["td"], m["trec"], 1024, 3), over)


def test_learn_mac_change_across_tile_edge(arp):
    """MAC A, B, A for one IP at frames 255, 256, 257: two events, B's before A's, A's first = 255."""
    rx = arp["rx"]
    C_ = bytes([0, 0x10, 0x94, 0, 0, 0xC])
    seq = [(0, 1, bytes([48, 0, 0, 9]), C_)] * 300
    seq[255], seq[256], seq[257] = (0, 1, IP1, A), (0, 1, IP1, B), (0, 1, IP1, A)
    m = make_case(rx, [arp_frame(*s) for s in seq], [1] * len(seq))
    want = want_prefix(m, 300)
    ev = want[1]
    assert [(bytes(e["mac"]), int(e["count"]), int(e["first"]), int(e["last"])) for e in ev] == \
        [(B, 1, 256, 256), (A, 2, 255, 257), (C_, 297, 0, 299)]
    check(learn(rx, m["tb"], m["td"], m["trec"], 300, 3), want)


def test_learn_without_outcome(mixed):
    m, n = mixed, 1000
    want = want_prefix(m, n, 3)
    got = learn(m["rx"], m["tb"], m["td"], m["trec"], n, len(want[1]), outcome=False)
    assert got["outcome"] is None
    check(got, want)


def test_learn_back_to_back_leaves_no_residue(arp):
    """Two calls on one stream, no synchronisation between them, with different batches: the
    first call's set is empty again when the second starts."""
    rx, d, o = arp["rx"], arp["distinct"], arp["one"]
    g1 = learn(rx, d["tb"], d["td"], d["trec"], 4096, 4096, sync=False)
    g2 = learn(rx, o["tb"], o["td"], o["trec"], 4096, 16, sync=False)
    g3 = learn(rx, d["tb"], d["td"], d["trec"], 1000, 100, sync=False)  # overflows: its slots are cleared all the same
    g4 = learn(rx, d["tb"], d["td"], d["trec"], 4096, 4096, sync=False)
    check(finish(g1), want_prefix(d, 4096))
    check(finish(g2), want_prefix(o, 4096))
    check(finish(g3), want_prefix(d, 1000, ev_cap=100))
    check(finish(g4), want_prefix(d, 4096))


def test_learn_client_removed_before_learn(gpu_ok, oracle_built):
    """Tables changed between classify and learn: solicitations from, and advertisements for, a
    client's address are not learned while the client exists, and are once it is gone."""
    from emurx.rx import RxPath
    rx = RxPath(0, max_ns=16, max_clients=64, max_frames=1 << 11)
    rx.register_all()
    env6 = N.Env()
    N.load_combined(rx, None, env6)
    fr, vp = L.learning_batch(2048)
    m = make_case(rx, fr, vp, env6)
    before = want_prefix(m, 2048)
    check(learn(rx, m["tb"], m["td"], m["trec"], 2048, len(before[1])), before)
    for ns in range(len(N._NS)):  # client 1 of every Namespace leaves
        cid = N.CID_BASE + ns * N.N_CLIENTS + 1
        assert rx.client_remove(N.NS_BASE + ns, env6.clients[cid]["mac"]) == 0
        env6.remove(cid)
    rx.sync()
    want = L.learn_batch(m["buf"], m["desc"], m["rec"], abi.LRNK_ALL, env6)
    flipped = np.nonzero(before[0] != want[0])[0]
    assert {(int(before[0][i]), int(want[0][i])) for i in flipped} == {(0, abi.LRN_ND_NS), (0, abi.LRN_ND_NA)}
    assert len(want[1]) > len(before[1])
    check(learn(rx, m["tb"], m["td"], m["trec"], 2048, len(want[1])), want)
    rx.close()


def test_respond_and_learn_account_for_every_arp_request(mixed):
    """emurx_respond_kinds_dev and emurx_learn_dev on one batch: every ARP request that reaches a
    Namespace with the arp plugin is folded into an ARP_REQ event, every one for a client's address
    is answered, and those need no Go handler."""
    import torch
    m, n = mixed, 4096
    rec, desc, buf = m["rec"], m["desc"], m["buf"]
    lk = (rec["flags"] >> 4) & 7
    is_req = np.zeros(n, bool)
    for i in np.nonzero((rec["status"] == 0) & (rec["proto"] == abi.CB_ARP) & (lk >= abi.LK["NS_LEVEL"]) &
                        (desc["pad"] != abi.DESC_HOLE))[0]:
        p = int(desc["off"][i]) + int(rec["l3"][i])
        is_req[i] = bytes(buf[p + 6:p + 8]) == b"\x00\x01"
    assert is_req.sum() >= 100
    want = want_prefix(m, n, 3)
    got = learn(m["rx"], m["tb"], m["td"], m["trec"], n, len(want[1]))
    check(got, want)
    rwant = N.respond_batch(buf, desc, rec, abi.RSPK_ARP, m["env4"], None)
    cap = int(rwant[4][1])
    out = torch.zeros(cap + 64, dtype=torch.uint8, device="cuda")
    od = torch.zeros(n * 8, dtype=torch.uint8, device="cuda")
    src = torch.zeros(n, dtype=torch.int32, device="cuda")
    oc = torch.zeros(n, dtype=torch.uint8, device="cuda")
    info = torch.zeros(abi.RSP_INFO_WORDS, dtype=torch.int64, device="cuda")
    m["rx"].respond_dev(m["tb"], m["td"], m["trec"], n, out, cap, od, src, oc, info, kinds=abi.RSPK_ARP)
    torch.cuda.synchronize()
    rsp = oc.cpu().numpy()
    assert np.array_equal(rsp, rwant[0])
    lrn = got["outcome"]
    assert np.array_equal(lrn == abi.LRN_ARP_REQ, is_req)                    # every request is folded, nothing else is
    assert np.array_equal(rsp == abi.RSP_ARP, is_req & (lk == abi.LK["CLIENT"]))  # every request for a client is answered
    ev = got["ev"][: int(got["info"][0]) * 40].view(abi.LEARN_EV_DTYPE)
    assert int(ev["count"][ev["kind"] == abi.LRN_ARP_REQ].sum()) == int(is_req.sum()) == int(got["info"][3])
    no_go = (rsp == abi.RSP_ARP) & (lrn != abi.LRN_HOST) & (got["info"][2] == 0)
    assert no_go.sum() == (rsp == abi.RSP_ARP).sum() >= 50

"""The device answers of an ingest slot (emurx_ingest_set_answers / emurx_ingest_answers): every
batch is compared (a) byte for byte with the direct chain on the same handle -- the slot's buffer
uploaded, res.desc as the descriptors, then classify_dev, respond_dev(kinds), tx_zmq_dev(n =
replies), learn_dev, nsstat_dev -- and (b) with the Python references of the stage tests
(respond_ref / nd_ref, the oracle's tx framing, learn_ref, nsstat_ref) and, for the reference's
captures, with the replies and counters those tests pin."""
import ctypes as C
import struct

import numpy as np
import pytest

import learn_ref as L
import nd_ref as N
import nsstat_ref as NS
import respond_ref as R
import sim_envs as S
from emurx import abi, frames as F

pytestmark = pytest.mark.gpu

KEYS = ["tx", "tx_msg_off", "reply_src", "rsp_outcome", "lrn_outcome", "done", "learn_ev", "ns_ev", "rsp_info",
        "lrn_info", "nss_info"]


# ---- helpers ---------------------------------------------------------------------------------------
def messages(frames, vports, per=64, limit=60000):
    """Consecutive frames as ZMQ messages of at most `per` frames and `limit` bytes."""
    msgs, cur, size = [], [], 4
    for i, f in enumerate(frames):
        if cur and (len(cur) == per or size + 4 + len(f) > limit):
            msgs.append(F.zmq_pack([frames[k] for k in cur], [vports[k] for k in cur]))
            cur, size = [], 4
        cur.append(i)
        size += 4 + len(f)
    if cur:
        msgs.append(F.zmq_pack([frames[k] for k in cur], [vports[k] for k in cur]))
    return msgs


def place(rx, slot, msgs, gap=3):
    """The messages into the slot's buffer, `gap` bytes apart (unaligned) -> the table and a copy of the buffer."""
    buf = rx.ingest_buffer(slot, sum(len(m) + gap for m in msgs) + 16)
    buf[:] = 0
    tab, at = np.zeros(len(msgs), abi.MSG_DTYPE), 0
    for i, m in enumerate(msgs):
        at += gap
        buf[at:at + len(m)] = np.frombuffer(m, np.uint8)
        tab[i] = (at, len(m))
        at += len(m)
    return tab, np.array(buf)


def run_slot(rx, slot, msgs, kinds=None):
    """One batch on the slot -> the ingest result, its answers, the buffer's bytes."""
    if kinds is not None:
        rx.ingest_set_answers(slot, kinds)
    tab, buf = place(rx, slot, msgs)
    rx.ingest_submit(slot, tab)
    res = rx.ingest_wait(slot)
    return res, rx.ingest_answers(slot, res["n"]), buf


def direct(rx, buf, desc, kinds):
    """The chain through the device entry points, on the closed batch -> the answers' dict, and the records."""
    import torch
    from gpu_util import to_dev
    n = len(desc)
    m1 = max(n, 1)
    tb, td = to_dev(buf), to_dev(desc)
    trec = torch.zeros(m1 * 32, dtype=torch.uint8, device="cuda")
    if n:
        hist = torch.zeros(abi.HIST_SHARDS * 2 * abi.HIST_BINS, dtype=torch.int64, device="cuda")
        rx.classify_dev(tb, td, n, trec, None, 0, None, hist)
    cap = int(sum(max((int(x) + 15) & ~15, 96) for x in desc["len"])) + 64
    out = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    od = torch.zeros(m1 * 8, dtype=torch.uint8, device="cuda")
    src = torch.zeros(m1, dtype=torch.int32, device="cuda")
    rsp = torch.zeros(m1, dtype=torch.uint8, device="cuda")
    rinfo = torch.zeros(abi.RSP_INFO_WORDS, dtype=torch.int64, device="cuda")
    rx.respond_dev(tb, td, trec, n, out, cap, od, src, rsp, rinfo, kinds=kinds)
    torch.cuda.synchronize()
    k = int(rinfo[0])
    zcap = 8 * k + cap
    zout = torch.zeros(zcap, dtype=torch.uint8, device="cuda")
    zoff = torch.zeros(k + 1, dtype=torch.int64, device="cuda")
    zinfo = torch.zeros(2, dtype=torch.int64, device="cuda")
    rx.tx_zmq_dev(out, od, k, zout, zcap, zoff, zinfo)
    lk = (abi.LRNK_ARP if kinds & abi.RSPK_ARP else 0) | (abi.LRNK_ND if kinds & abi.RSPK_ND else 0)
    lrn = torch.zeros(m1, dtype=torch.uint8, device="cuda")
    linfo = torch.zeros(abi.LRN_INFO_WORDS, dtype=torch.int64, device="cuda")
    lcap = rx.learn_max_events()
    lev = torch.zeros(lcap * 40, dtype=torch.uint8, device="cuda")
    if lk:
        rx.learn_dev(tb, td, trec, n, lev, lcap, lrn, linfo, kinds=lk)
    ncap = rx.nsstat_max_events()
    nev = torch.zeros(ncap * 96, dtype=torch.uint8, device="cuda")
    dn = torch.zeros(m1, dtype=torch.uint8, device="cuda")
    ninfo = torch.zeros(abi.NSS_INFO_WORDS, dtype=torch.int64, device="cuda")
    rx.nsstat_dev(tb, td, trec, n, rsp, lrn, nev, ncap, dn, ninfo, kinds=kinds)
    torch.cuda.synchronize()
    u64 = lambda t: t.cpu().numpy().view(np.uint64)  # noqa: E731
    nm, total = (int(x) for x in zinfo.cpu().numpy())
    ans = dict(tx=zout.cpu().numpy()[:total], tx_msg_off=u64(zoff)[: nm + 1], reply_src=src.cpu().numpy().view(np.uint32)[:k],
               rsp_outcome=rsp.cpu().numpy()[:n], lrn_outcome=lrn.cpu().numpy()[:n], done=dn.cpu().numpy()[:n],
               learn_ev=lev.cpu().numpy()[: int(linfo[0]) * 40].view(abi.LEARN_EV_DTYPE),
               ns_ev=nev.cpu().numpy()[: int(ninfo[0]) * 96].view(abi.NSSTAT_EV_DTYPE),
               rsp_info=u64(rinfo), lrn_info=u64(linfo), nss_info=u64(ninfo), n_replies=k, n_tx_msgs=nm, tx_bytes=total)
    return ans, trec.cpu().numpy()[: n * 32].view(abi.REC_DTYPE)


def same(got, want, tag=None):
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), (tag, k, got[k][:8], want[k][:8])
    for k in ("n_replies", "n_tx_msgs", "tx_bytes"):
        assert got[k] == want[k], (tag, k)


def check_direct(rx, res, ans, buf, kinds, tag=None):
    """(a): the answers equal the direct chain's on the closed batch; -> the direct records."""
    want, rec = direct(rx, buf, res["desc"], kinds)
    assert res["rec"].tobytes() == rec.tobytes(), tag
    assert not res["one_launch"], tag
    same(ans, want, tag)
    return rec


def unframe(tx, off):
    """The frames of back-to-back ZMQ messages (veth_zmq.go:8-22), each message checked whole."""
    out = []
    for m in range(len(off) - 1):
        b = tx[int(off[m]):int(off[m + 1])].tobytes()
        magic, cnt = struct.unpack(">HH", b[:4])
        assert magic == 0xBEEF and 1 <= cnt <= abi.ZMQ_TX_BURST
        at = 4
        for _ in range(cnt):
            h = struct.unpack(">I", b[at:at + 4])[0]
            assert h >> 24 == abi.ZMQ_PKT_MAGIC
            out.append(b[at + 4:at + 4 + (h & 0xFFFF)])
            at += 4 + (h & 0xFFFF)
        assert at == len(b)
    return out


def check_refs(res, ans, buf, kinds, env4, env6):
    """(b): the Python references of the stage tests on the result's records."""
    import pyoracle
    desc, rec = res["desc"], res["rec"]
    outcome, od, src, replies, info = N.respond_batch(buf, desc, rec, kinds, env4, env6)
    assert np.array_equal(ans["rsp_outcome"], outcome) and np.array_equal(ans["rsp_info"], info)
    assert np.array_equal(ans["reply_src"], src) and unframe(ans["tx"], ans["tx_msg_off"]) == replies
    if replies:
        rbuf, rdesc = F.pack_frames(replies, [int(v) for v in od["vport"]], header=0)
        wmsg, woff, wtotal = pyoracle.tx_zmq(rbuf, rdesc)
        assert ans["tx_bytes"] == wtotal and np.array_equal(ans["tx_msg_off"], woff) and ans["tx"].tobytes() == wmsg.tobytes()
    else:
        assert ans["tx_bytes"] == 0 and ans["n_tx_msgs"] == 0 and ans["tx_msg_off"].tolist() == [0]
    lk = (abi.LRNK_ARP if kinds & abi.RSPK_ARP else 0) | (abi.LRNK_ND if kinds & abi.RSPK_ND else 0)
    if lk:
        lo, lev, linfo = L.learn_batch(buf, desc, rec, lk, env6)
        assert np.array_equal(ans["lrn_outcome"], lo) and np.array_equal(ans["lrn_info"], linfo)
        assert ans["learn_ev"].tobytes() == lev.tobytes()
    else:
        assert not ans["lrn_outcome"].any() and not ans["lrn_info"].any() and len(ans["learn_ev"]) == 0
    done, nev, ninfo = NS.nsstat_batch(buf, desc, rec, kinds, ans["rsp_outcome"], ans["lrn_outcome"])
    assert np.array_equal(ans["done"], done) and np.array_equal(ans["nss_info"], ninfo)
    assert ans["ns_ev"].tobytes() == nev.tobytes()


# ---- the reference's captures ------------------------------------------------------------------------
def _capture_params():
    from test_nsstat_ref import CAPTURES
    return [c for c in CAPTURES if c[0] != "arp2.json"]


@pytest.mark.parametrize("capture,envname,n,words", _capture_params(), ids=[c[0] for c in _capture_params()])
def test_answers_captures(gpu_ok, oracle_built, capture, envname, n, words):
    """arp4, arp5, icmp1, icmpv6_1, icmpv6_2, ipv6nd_2, ipv6nd_3 as messages of 1, 7 and 64 frames, every
    kind on: the replies unframed from tx are the capture's (test_respond_ref / test_nd_ref pin them),
    every frame is done 1 and the one Namespace event carries the capture's counters (test_nsstat_ref)."""
    from emurx.rx import RxPath
    from test_oracle_corpus import GOLD
    import test_nd_ref
    import test_respond_ref
    z = np.load(GOLD, allow_pickle=False)
    fr = S.rx_frames(z, capture)
    assert len(fr) == n
    if capture.startswith("ipv6nd"):
        cbuf, cdesc, crec, env6, tx = test_nd_ref.capture_case(capture)
        want = N.respond_batch(cbuf, cdesc, crec, abi.RSPK_ND, env6=env6)[3]
        assert test_nd_ref.capture_replies(tx, want) == want and len(want) == n
    else:
        want = test_respond_ref.capture_case(capture, envname)[4]
    rx = RxPath(0, max_ns=16, max_clients=16, max_frames=1 << 10)
    rx.register_all()
    S.load_env(rx, envname)
    try:
        for per in (1, 7, 64):
            res, ans, buf = run_slot(rx, 0, messages(fr, [1] * n, per), abi.RSPK_ALL)
            assert res["n"] == n and res["counters"]["rx_batch"] == -(-n // per)
            check_direct(rx, res, ans, buf, abi.RSPK_ALL, per)
            assert unframe(ans["tx"], ans["tx_msg_off"]) == want, per
            assert ans["n_replies"] == len(want) and ans["n_tx_msgs"] == (1 if want else 0)
            assert (ans["done"] == 1).all() and len(ans["ns_ev"]) == 1 and int(ans["ns_ev"][0]["frames"]) == n
            assert {k: int(v) for k, v in enumerate(ans["ns_ev"][0]["cnt"]) if v} == words
    finally:
        rx.close()


# ---- the mixed batches ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed(gpu_ok, oracle_built):
    """test_gpu_respond's mixed batch (respond_ref.mixed_batch(4099), its tables) on a handle with
    room for it, and the frames of its first run with every kind on."""
    from emurx.rx import RxPath
    rx = RxPath(0, max_ns=16, max_clients=64, max_frames=1 << 13, max_bytes=4 << 20)
    rx.register_all()
    env = R.Env()
    R.load_tables(rx, env)
    fr, vp = R.mixed_batch(4099)
    m = dict(rx=rx, env=env, fr=fr, vp=vp, msgs=messages(fr, vp))
    yield m
    rx.close()


@pytest.fixture(scope="module")
def picks(mixed):
    """Indices of the mixed batch's answered ARP requests, answered echo requests and plain UDP frames."""
    res, ans, _ = run_slot(mixed["rx"], 0, mixed["msgs"], abi.RSPK_ALL)
    assert res["n"] == 4099
    o = ans["rsp_outcome"]
    udp = np.nonzero((res["rec"]["proto"] == abi.CB_UDP) & (res["rec"]["status"] == 0))[0]
    return dict(arp=np.nonzero(o == abi.RSP_ARP)[0], echo=np.nonzero((o == abi.RSP_ICMP) | (o == abi.RSP_ICMPV6))[0], udp=udp)


@pytest.mark.parametrize("kinds", [abi.RSPK_ARP, abi.RSPK_ICMP, abi.RSPK_ICMPV6, abi.RSPK_ND, abi.RSPK_ARP | abi.RSPK_ND,
                                   abi.RSPK_ALL])
def test_answers_mixed_kinds(mixed, kinds):
    m = mixed
    res, ans, buf = run_slot(m["rx"], 0, m["msgs"], kinds)
    assert res["n"] == 4099
    check_direct(m["rx"], res, ans, buf, kinds)
    check_refs(res, ans, buf, kinds, m["env"], N.Env())
    if kinds & (abi.RSPK_ARP | abi.RSPK_ICMP | abi.RSPK_ICMPV6):
        assert ans["n_replies"] > 100 and ans["n_tx_msgs"] >= 2 and (ans["done"] == 1).sum() > 100
    if kinds & abi.RSPK_ARP:
        assert len(ans["learn_ev"]) > 50


@pytest.mark.parametrize("kinds", [abi.RSPK_ALL, abi.RSPK_ARP | abi.RSPK_ND, abi.RSPK_ND])
def test_answers_combined_batch(gpu_ok, oracle_built, kinds):
    """test_gpu_nsstat's batch (respond_ref's mixed frames and learn_ref's learning frames interleaved,
    neighbour solicitations and advertisements among them): every stage has work, ND included."""
    from emurx.rx import RxPath
    rx = RxPath(0, max_ns=16, max_clients=64, max_frames=1 << 12, max_bytes=4 << 20)
    rx.register_all()
    env4, env6 = R.Env(), N.Env()
    N.load_combined(rx, env4, env6)
    fr, vp = NS.mixed_batch(2048)
    try:
        res, ans, buf = run_slot(rx, 1, messages(fr, vp), kinds)
        assert res["n"] == 2048
        check_direct(rx, res, ans, buf, kinds)
        check_refs(res, ans, buf, kinds, env4, env6)
        assert (ans["rsp_outcome"] == abi.RSP_ND).sum() > 8 and {abi.LRN_ND_NS, abi.LRN_ND_NA} <= set(ans["lrn_outcome"])
        assert len(ans["learn_ev"]) > 8 and len(ans["ns_ev"]) >= 3
    finally:
        rx.close()


# ---- sizes ---------------------------------------------------------------------------------------------
def test_answers_no_message_and_empty_message(mixed):
    rx = mixed["rx"]
    for msgs in ([], [F.zmq_pack([])], [b"", F.zmq_pack([])]):
        res, ans, buf = run_slot(rx, 0, msgs, abi.RSPK_ALL)
        assert res["n"] == 0 and ans["n_replies"] == 0 and ans["n_tx_msgs"] == 0 and ans["tx_bytes"] == 0
        assert ans["tx_msg_off"].tolist() == [0] and len(ans["learn_ev"]) == 0 and len(ans["ns_ev"]) == 0
        assert not ans["rsp_info"].any() and not ans["lrn_info"].any() and not ans["nss_info"].any()
        check_direct(rx, res, ans, buf, abi.RSPK_ALL, len(msgs))


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_answers_tile_edges(mixed, n):
    """1 frame, and the k_rx tile edge: the mixed batch's frames 1 .. n + 1 (frame 1 is an answered ARP request)."""
    m = mixed
    fr, vp = m["fr"][1:n + 1], m["vp"][1:n + 1]
    res, ans, buf = run_slot(m["rx"], 0, messages(fr, vp), abi.RSPK_ALL)
    assert res["n"] == n and ans["n_replies"] >= 1
    check_direct(m["rx"], res, ans, buf, abi.RSPK_ALL)
    check_refs(res, ans, buf, abi.RSPK_ALL, m["env"], N.Env())


def test_answers_130_arp_requests(mixed, picks):
    """130 answered ARP requests in one message: three tx messages (64 + 64 + 2, EMURX_ZMQ_TX_BURST)."""
    m = mixed
    idx = picks["arp"][:130]
    assert len(idx) == 130
    fr = [m["fr"][i] for i in idx]
    res, ans, buf = run_slot(m["rx"], 0, [F.zmq_pack(fr, [1] * 130)], abi.RSPK_ALL)
    assert res["n"] == 130 and ans["n_replies"] == 130 and ans["n_tx_msgs"] == 3
    assert (ans["rsp_outcome"] == abi.RSP_ARP).all() and (ans["done"] == 1).all()
    assert ans["reply_src"].tolist() == list(range(130))
    assert [struct.unpack(">HH", ans["tx"][int(o):int(o) + 4].tobytes())[1] for o in ans["tx_msg_off"][:-1]] == [64, 64, 2]
    check_direct(m["rx"], res, ans, buf, abi.RSPK_ALL)
    check_refs(res, ans, buf, abi.RSPK_ALL, m["env"], N.Env())


def test_answers_udp_only(mixed, picks):
    """Plain UDP alone: no candidate for any stage, everything zero."""
    m = mixed
    fr = [m["fr"][i] for i in picks["udp"]]
    assert len(fr) > 100
    res, ans, buf = run_slot(m["rx"], 0, messages(fr, [1] * len(fr)), abi.RSPK_ALL)
    assert res["n"] == len(fr) and ans["n_tx_msgs"] == 0 and ans["tx_bytes"] == 0 and ans["n_replies"] == 0
    assert not ans["rsp_outcome"].any() and not ans["lrn_outcome"].any() and not ans["done"].any()
    assert len(ans["learn_ev"]) == 0 and len(ans["ns_ev"]) == 0
    assert not ans["rsp_info"].any() and not ans["lrn_info"].any() and not ans["nss_info"][[0, 1, 2, 3, 4]].any()
    check_direct(m["rx"], res, ans, buf, abi.RSPK_ALL)


# ---- holes ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["first", "middle", "last", "all"])
def test_answers_holes(mixed, where):
    """Messages whose header announces 3 frames more than they carry leave hole slots: the per-frame
    arrays line up with res.rec, reply_src and the learn events' first / last are in the closed
    numbering, and everything equals the direct chain on the closed batch."""
    m = mixed
    fr, vp = m["fr"][:700], m["vp"][:700]
    msgs = messages(fr, vp, per=40)
    short = {"first": [0], "middle": [len(msgs) // 2], "last": [len(msgs) - 1], "all": [0, len(msgs) // 2, len(msgs) - 1]}[where]
    carried = []
    for k in short:
        b = bytearray(msgs[k])
        carried.append(struct.unpack(">H", b[2:4])[0])
        b[2:4] = struct.pack(">H", carried[-1] + 3)
        msgs[k] = bytes(b)
    res, ans, buf = run_slot(m["rx"], 0, msgs, abi.RSPK_ALL)
    assert res["n"] == 700 and [int(res["msg_frames"][k]) for k in short] == carried
    assert all(int(res["msg_status"][k]) == abi.MSG_PARSE_ERR for k in short)
    assert len(ans["rsp_outcome"]) == len(ans["lrn_outcome"]) == len(ans["done"]) == 700
    assert ans["n_replies"] > 100 and ans["reply_src"].max() < 700 and (np.diff(ans["reply_src"].astype(np.int64)) > 0).all()
    ev = ans["learn_ev"]
    assert len(ev) > 10 and ev["last"].max() < 700 and (ev["first"] <= ev["last"]).all()
    assert (np.diff(ev["last"].astype(np.int64)) > 0).all()
    # the frames themselves: every reply's source is a frame the responder's outcome says it answered
    assert (ans["rsp_outcome"][ans["reply_src"]] != 0).all()
    check_direct(m["rx"], res, ans, buf, abi.RSPK_ALL, where)
    check_refs(res, ans, buf, abi.RSPK_ALL, m["env"], N.Env())


# ---- slots ---------------------------------------------------------------------------------------------
def test_answers_two_slots_in_flight(mixed, picks):
    """Two slots submitted before either is waited for, one ARP-heavy and one echo-heavy, then both
    reused for three more rounds of other content: each batch equals its own sequential result (the
    shared scratch is handed over by an event; learn sets, nsstat rows, the framing's arrival
    counters and k_ans_out's counts are clean between batches)."""
    m, rx = mixed, mixed["rx"]
    arp, echo = picks["arp"], picks["echo"]
    rx.ingest_set_answers(0, abi.RSPK_ALL)
    rx.ingest_set_answers(1, abi.RSPK_ALL)
    for rnd in range(4):
        a = [int(i) for i in arp[40 * rnd:40 * rnd + 150 - 30 * rnd]] + list(range(rnd, 60 + 20 * rnd))
        e = [int(i) for i in echo[100 * rnd:100 * rnd + 400 + 50 * rnd]] + list(range(5 * rnd, 30))
        if rnd == 3:
            a, e = e, a[:7]  # the slots change roles, and a small batch follows a large one
        sets = [a, e]
        tabs, bufs = [], []
        for s in (0, 1):
            fr = [m["fr"][i] for i in sets[s]]
            t, b = place(rx, s, messages(fr, [1] * len(fr), per=33 + 31 * s))
            tabs.append(t)
            bufs.append(b)
        rx.ingest_submit(0, tabs[0])
        rx.ingest_submit(1, tabs[1])
        out = []
        for s in (1, 0):  # waited for in the other order
            res = rx.ingest_wait(s)
            out.append((s, res, rx.ingest_answers(s, res["n"])))
        for s, res, ans in out:
            assert res["n"] == len(sets[s])
            check_direct(rx, res, ans, bufs[s], abi.RSPK_ALL, (rnd, s))
        if rnd == 0:
            a0, e0 = (o[2] for o in sorted(out, key=lambda o: o[0]))
            assert (a0["rsp_outcome"] == abi.RSP_ARP).sum() >= 150 and len(a0["learn_ev"]) >= 100
            assert ((e0["rsp_outcome"] == abi.RSP_ICMP) | (e0["rsp_outcome"] == abi.RSP_ICMPV6)).sum() >= 400
            assert a0["tx"].tobytes() != e0["tx"].tobytes()


def test_answers_off_by_default_and_switch(mixed):
    """A slot that never called set_answers: ENOENT, and a small batch still runs as one launch; the
    same batch with answers on takes the pipeline with identical results; kinds 0 turns them off again."""
    m, rx = mixed, mixed["rx"]
    short = [f for f in m["fr"] if len(f) <= 80][:300]  # a tile's messages within the one-launch path's LDS budget
    assert len(short) == 300
    msgs = messages(short, [1] * 300)
    a = abi.Answers()

    def plain(slot):
        tab, _ = place(rx, slot, msgs)
        rx.ingest_submit(slot, tab)
        res = rx.ingest_wait(slot)
        assert rx.lib.emurx_ingest_answers(rx.h, slot, C.byref(a)) == abi.EMURX_ENOENT
        return res
    assert rx.lib.emurx_ingest_answers(rx.h, 3, C.byref(a)) == abi.EMURX_EINVAL  # before any wait
    off = plain(3)
    assert off["one_launch"]
    on, ans, buf = run_slot(rx, 2, msgs, abi.RSPK_ALL)
    assert not on["one_launch"] and ans["n_replies"] > 50
    for k in ("rec", "desc", "qlist", "qoff", "msg_frames", "msg_status"):
        assert on[k].tobytes() == off[k].tobytes(), k
    assert on["counters"] == off["counters"] and on["n"] == off["n"] == 300
    rx.ingest_set_answers(2, 0)
    again = plain(2)
    assert again["one_launch"] and again["rec"].tobytes() == off["rec"].tobytes()


def test_set_answers_in_flight_and_arguments(mixed):
    rx = mixed["rx"]
    f = rx.lib.emurx_ingest_set_answers
    assert f(rx.h, abi.INGEST_SLOTS, abi.RSPK_ALL) == abi.EMURX_EINVAL
    assert f(rx.h, 0, abi.RSPK_ALL + 1) == abi.EMURX_EINVAL
    tab, _ = place(rx, 0, messages(mixed["fr"][:64], mixed["vp"][:64]))
    rx.ingest_submit(0, tab)
    assert f(rx.h, 0, abi.RSPK_ARP) == abi.EMURX_EINVAL
    assert f(rx.h, 0, 0) == abi.EMURX_EINVAL
    a = abi.Answers()
    assert rx.lib.emurx_ingest_answers(rx.h, 0, C.byref(a)) == abi.EMURX_EINVAL  # a batch in flight
    assert rx.ingest_wait(0)["n"] == 64
    assert f(rx.h, 0, abi.RSPK_ARP) == abi.EMURX_OK


def test_answers_past_max_bytes(gpu_ok, oracle_built):
    """With answers on, messages that end past cfg.max_bytes are refused (the answer buffers are sized for it)."""
    from emurx.rx import RxPath
    rx = RxPath(0, max_ns=16, max_clients=16, max_frames=1 << 10, max_bytes=4096)
    try:
        msgs = [F.zmq_pack([bytes(60)] * 64)] * 2
        rx.ingest_set_answers(0, abi.RSPK_ALL)
        tab, _ = place(rx, 0, msgs)
        with pytest.raises(RuntimeError, match=f"emurx error {abi.EMURX_ENOSPC}"):
            rx.ingest_submit(0, tab)
        rx.ingest_set_answers(0, 0)
        rx.ingest_submit(0, tab)
        assert rx.ingest_wait(0)["n"] == 128
    finally:
        rx.close()

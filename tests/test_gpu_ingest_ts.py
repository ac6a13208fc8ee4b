"""The timestamp reply on an ingest slot (emurx_ingest_set_answers_ts, emurx_ingest_set_time): every
batch is compared (a) byte for byte with the direct chain on the same handle -- classify_dev,
emurx_respond_ts_dev with the slot's time, tx_zmq_dev, learn_dev, emurx_nsstat_ts_dev -- and (b)
with ts_ref, and for the reference's six requests with the counters its simulation recorded."""
import json
import struct
from pathlib import Path

import numpy as np
import pytest

import learn_ref as L
import nd_ref as N
import nsstat_ref as NS
import respond_ref as R
import sim_envs as S
import ts_ref as T
from emurx import abi, frames as F
from test_gpu_ingest_answers import check_direct, messages, place, same, unframe
from test_nsstat_ref import sim_envs

pytestmark = pytest.mark.gpu

COUNTERS = json.loads((Path(__file__).parent / "golden" / "icmp2_counters.json").read_text())
ALL = abi.RSPK_ALL_TS


def submit(rx, slot, msgs):
    tab, buf = place(rx, slot, msgs)
    rx.ingest_submit(slot, tab)
    return buf


def collect(rx, slot):
    res = rx.ingest_wait(slot)
    return res, rx.ingest_answers(slot, res["n"])


def direct(rx, buf, desc, kinds, ip_time):
    """The chain through the device entry points on the closed batch -> the answers' dict, the records."""
    import torch
    from gpu_util import to_dev
    n = len(desc)
    m1 = max(n, 1)
    tb, td = to_dev(buf), to_dev(desc)
    trec = torch.zeros(m1 * 32, dtype=torch.uint8, device="cuda")
    hist = torch.zeros(abi.HIST_SHARDS * 2 * abi.HIST_BINS, dtype=torch.int64, device="cuda")
    rx.classify_dev(tb, td, n, trec, None, 0, None, hist)
    cap = int(sum(max((int(x) + 15) & ~15, 96) for x in desc["len"])) + 64
    out = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    od = torch.zeros(m1 * 8, dtype=torch.uint8, device="cuda")
    src = torch.zeros(m1, dtype=torch.int32, device="cuda")
    rsp = torch.zeros(m1, dtype=torch.uint8, device="cuda")
    rinfo = torch.zeros(abi.RSP_INFO_WORDS, dtype=torch.int64, device="cuda")
    rx.respond_dev(tb, td, trec, n, out, cap, od, src, rsp, rinfo, kinds=kinds, ip_time=ip_time)
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


def check_chain(rx, res, ans, buf, kinds, ip_time, tag=None):
    want, rec = direct(rx, buf, res["desc"], kinds, ip_time)
    assert res["rec"].tobytes() == rec.tobytes() and not res["one_launch"], tag
    same(ans, want, tag)


def check_refs(res, ans, buf, kinds, ip_time, env4, env6=None):
    desc, rec = res["desc"], res["rec"]
    outcome, od, src, replies, info = T.respond_batch(buf, desc, rec, kinds, ip_time, env4, env6)
    assert np.array_equal(ans["rsp_outcome"], outcome) and np.array_equal(ans["rsp_info"], info)
    assert np.array_equal(ans["reply_src"], src) and unframe(ans["tx"], ans["tx_msg_off"]) == replies
    done, nev, ninfo = T.nsstat_batch(buf, desc, rec, kinds, ans["rsp_outcome"], ans["lrn_outcome"])
    assert np.array_equal(ans["done"], done) and np.array_equal(ans["nss_info"], ninfo)
    assert ans["ns_ev"].tobytes() == nev.tobytes()
    return replies


@pytest.fixture(scope="module")
def six(gpu_ok, oracle_built):
    from emurx.rx import RxPath
    rx = RxPath(0, max_ns=16, max_clients=16, max_frames=1 << 10)
    rx.register_all()
    S.load_env(rx, "icmp")
    yield dict(rx=rx, fr=T.six_requests(), env4=sim_envs("icmp")[0])
    rx.close()


def times_of(replies, l4=42):
    return [struct.unpack(">II", r[l4 + 12:l4 + 20]) for r in replies]


@pytest.mark.parametrize("per", [1, 7, 64])
def test_ingest_ts_six_requests(six, per):
    rx, fr = six["rx"], six["fr"]
    ip_time = 86_399_999 - per
    rx.ingest_set_answers(0, ALL)
    rx.ingest_set_time(0, ip_time)
    buf = submit(rx, 0, messages(fr, [1] * 6, per))
    res, ans = collect(rx, 0)
    assert res["n"] == 6 and res["counters"]["rx_batch"] == -(-6 // per)
    check_chain(rx, res, ans, buf, ALL, ip_time, per)
    replies = check_refs(res, ans, buf, ALL, ip_time, six["env4"])
    assert len(replies) == 6 and times_of(replies) == [(ip_time, ip_time)] * 6
    assert all(T.span_sum(r[42:]) == 0xFFFF for r in replies)
    assert (ans["rsp_outcome"] == abi.RSP_TS).all() and (ans["done"] == 1).all() and ans["n_tx_msgs"] == 1
    assert len(ans["ns_ev"]) == 1 and int(ans["ns_ev"][0]["frames"]) == 6
    assert {name: v for (ns, plug, name), v in NS.replay(ans["ns_ev"]).items()} == COUNTERS


def test_ingest_ts_two_slots_in_flight(six):
    """Two slots in flight with different times, three rounds: each slot's replies carry its own."""
    rx, fr = six["rx"], six["fr"]
    msgs = messages(fr, [1] * 6, 7)
    for slot in (1, 2):
        rx.ingest_set_answers(slot, ALL)
    for rnd in range(3):
        t = {1: 1000 * rnd + 1, 2: 0xFFFFFFFF - rnd}
        bufs = {}
        for slot in (1, 2):
            rx.ingest_set_time(slot, t[slot])
            bufs[slot] = submit(rx, slot, msgs)
        for slot in (2, 1):
            res, ans = collect(rx, slot)
            replies = check_refs(res, ans, bufs[slot], ALL, t[slot], six["env4"])
            assert times_of(replies) == [(t[slot], t[slot])] * 6, (rnd, slot)


def test_ingest_ts_set_time_rules(six):
    """A time set once holds for the next submits; with a batch in flight the call is refused and the
    batch keeps the time it was submitted with."""
    rx, fr = six["rx"], six["fr"]
    msgs = messages(fr, [1] * 6, 64)
    rx.ingest_set_answers(3, ALL)
    rx.ingest_set_time(3, 777)
    for _ in range(2):
        buf = submit(rx, 3, msgs)
        res, ans = collect(rx, 3)
        assert times_of(check_refs(res, ans, buf, ALL, 777, six["env4"])) == [(777, 777)] * 6
    buf = submit(rx, 3, msgs)
    assert rx.lib.emurx_ingest_set_time(rx.h, 3, 888) == abi.EMURX_EINVAL
    assert rx.lib.emurx_ingest_set_answers_ts(rx.h, 3, ALL) == abi.EMURX_EINVAL
    res, ans = collect(rx, 3)
    assert times_of(check_refs(res, ans, buf, ALL, 777, six["env4"])) == [(777, 777)] * 6
    assert rx.lib.emurx_ingest_set_time(rx.h, abi.INGEST_SLOTS, 1) == abi.EMURX_EINVAL
    for kinds in (32, 16, 16 | 13):
        assert rx.lib.emurx_ingest_set_answers_ts(rx.h, 3, kinds) == abi.EMURX_EINVAL
    assert rx.lib.emurx_ingest_set_answers(rx.h, 3, 16) == abi.EMURX_EINVAL
    rx.ingest_set_time(3, 888)
    buf = submit(rx, 3, msgs)
    res, ans = collect(rx, 3)
    assert times_of(check_refs(res, ans, buf, ALL, 888, six["env4"])) == [(888, 888)] * 6


def test_ingest_ts_off_and_old_kinds(six):
    """Answers off: no answers; kinds <= 15 through either entry point: emurx_ingest_set_answers' results
    (the timestamp requests stay with the Go handler), whatever time the slot holds."""
    rx, fr = six["rx"], six["fr"]
    echo = [f[:42] + F.icmp4(8, 0, 1, 9, bytes(12)) for f in fr[:3]]
    msgs = messages(fr + echo, [1] * 9, 64)
    rx.ingest_set_time(0, 4242)
    got = []
    for setter in (rx.lib.emurx_ingest_set_answers_ts, rx.lib.emurx_ingest_set_answers):
        assert setter(rx.h, 0, abi.RSPK_ALL) == 0
        buf = submit(rx, 0, msgs)
        res, ans = collect(rx, 0)
        assert res["n"] == 9 and ans["rsp_outcome"].tolist() == [abi.RSP_HOST] * 6 + [abi.RSP_ICMP] * 3
        assert ans["done"].tolist() == [0] * 6 + [1] * 3
        check_direct(rx, res, ans, buf, abi.RSPK_ALL)  # test_gpu_ingest_answers' chain: the old entry points
        got.append(ans)
    same(got[0], got[1])
    assert rx.lib.emurx_ingest_set_answers_ts(rx.h, 0, 0) == 0
    submit(rx, 0, msgs)
    res = rx.ingest_wait(0)
    assert res["n"] == 9
    assert rx.lib.emurx_ingest_answers(rx.h, 0, __import__("ctypes").byref(abi.Answers())) == abi.EMURX_ENOENT


def test_ingest_ts_mixed_batch(gpu_ok, oracle_built):
    """respond_ref's mixed batch with every kind and the timestamp reply on."""
    from emurx.rx import RxPath
    rx = RxPath(0, max_ns=16, max_clients=64, max_frames=1 << 13, max_bytes=4 << 20)
    rx.register_all()
    env = R.Env()
    R.load_tables(rx, env)
    fr, vp = R.mixed_batch(4099)
    try:
        rx.ingest_set_answers(0, ALL)
        rx.ingest_set_time(0, 12_345_678)
        buf = submit(rx, 0, messages(fr, vp))
        res, ans = collect(rx, 0)
        assert res["n"] == 4099
        check_chain(rx, res, ans, buf, ALL, 12_345_678)
        check_refs(res, ans, buf, ALL, 12_345_678, env, N.Env())
        o = ans["rsp_outcome"]
        assert (o == abi.RSP_TS).sum() >= 100 and (ans["done"][o == abi.RSP_TS] == 1).all()
        assert int(ans["rsp_info"][1 + abi.RSP_TS]) == (o == abi.RSP_TS).sum() and ans["n_replies"] == int(ans["rsp_info"][0])
        lo, lev, linfo = L.learn_batch(buf, res["desc"], res["rec"], abi.LRNK_ALL, N.Env())
        assert np.array_equal(ans["lrn_outcome"], lo) and ans["learn_ev"].tobytes() == lev.tobytes()
    finally:
        rx.close()

"""The flow stage on an ingest slot (emurx_ingest_set_flows / emurx_ingest_flows): every batch is
compared byte for byte with the direct chain on the same handle -- the slot's buffer uploaded,
res.desc as the descriptors, classify_dev with a flow array, then ftstat_dev -- and with ft_ref on
the oracle's flow words; emurx_ingest_result, emurx_answers and emurx_ping_out do not change with
the stage on."""
import ctypes as C
import struct

import numpy as np
import pytest

import ft_cases as K
import ft_ref as R
from emurx import abi
from test_gpu_ingest_answers import messages, place, same

pytestmark = pytest.mark.gpu

NOW = 1_700_000_000_000_000_000
RES_KEYS = ("rec", "desc", "qlist", "qoff", "msg_frames", "msg_status")


def direct(rx, buf, desc):
    """classify_dev (flow words) + ftstat_dev on the closed batch -> dict(flow, outcome, ev, info), the records."""
    import torch
    from gpu_util import to_dev
    n = len(desc)
    tb, td = to_dev(buf), to_dev(desc)
    trec = torch.zeros(max(n, 1) * 32, dtype=torch.uint8, device="cuda")
    tflow = torch.zeros(max(n, 1), dtype=torch.int32, device="cuda")
    hist = torch.zeros(abi.HIST_SHARDS * 2 * abi.HIST_BINS, dtype=torch.int64, device="cuda")
    rx.classify_dev(tb, td, n, trec, None, 0, None, hist, flow=tflow)
    cap = rx.ftstat_max_events()
    ev = torch.zeros(cap * 48, dtype=torch.uint8, device="cuda")
    oc = torch.zeros(max(n, 1), dtype=torch.uint8, device="cuda")
    info = torch.zeros(abi.FT_INFO_WORDS, dtype=torch.int64, device="cuda")
    rx.ftstat_dev(tb, td, trec, tflow, n, ev, cap, oc, info)
    torch.cuda.synchronize()
    iw = info.cpu().numpy().view(np.uint64)
    return dict(flow=tflow.cpu().numpy().view(np.uint32)[:n], outcome=oc.cpu().numpy()[:n],
                ev=ev.cpu().numpy()[: int(iw[0]) * 48].view(abi.FT_EV_DTYPE), info=iw), \
        trec.cpu().numpy()[: n * 32].view(abi.REC_DTYPE)


def equal(got, want, tag=None):
    for k in ("flow", "outcome", "ev", "info"):
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), (tag, k, got[k][:4], want[k][:4])


def check(m, res, flw, buf, tag=None):
    """The slot's stage equals the direct chain's and ft_ref's on the closed batch."""
    want, rec = direct(m["rx"], buf, res["desc"])
    assert res["rec"].tobytes() == rec.tobytes() and not res["one_launch"], tag
    equal(flw, want, tag)
    oflow = m["orc"].flows(buf, res["desc"], res["rec"])
    assert np.array_equal(flw["flow"], oflow), tag
    oc, cand = R.outcomes(buf, res["desc"], res["rec"], oflow, K.MAX_NS, K.MAX_CLIENTS)
    ev, info = R.fold(oc, cand, res["rec"])
    assert np.array_equal(flw["outcome"], oc) and flw["ev"].tobytes() == ev.tobytes() and np.array_equal(flw["info"], info), tag
    return oc


@pytest.fixture(scope="module")
def m(gpu_ok, oracle_built):
    from emurx.rx import RxPath
    rx = RxPath(0, max_ns=K.MAX_NS, max_clients=K.MAX_CLIENTS, max_frames=1 << 12, max_bytes=1 << 20)
    rx.register_all()
    orc = oracle_built.Oracle()
    for t in (rx, orc):
        K.load_tables(t)
        K.load_flows(t)
    yield dict(rx=rx, orc=orc, fr=K.stream(700, seed=5))
    rx.close()


def run_slot(rx, slot, msgs, flows=True, kinds=0, fams=0):
    rx.ingest_set_answers(slot, kinds)
    if kinds:
        rx.ingest_set_ping(slot, fams)
        rx.ingest_set_now(slot, NOW)
    rx.ingest_set_flows(slot, flows)
    tab, buf = place(rx, slot, msgs)
    rx.ingest_submit(slot, tab)
    res = rx.ingest_wait(slot)
    return res, (rx.ingest_flows(slot, res["n"]) if flows else None), buf


def fall_short(msgs):
    """Three messages announce 3 frames more than they carry: hole slots, closed by the wait."""
    msgs = list(msgs)
    for k in (0, len(msgs) // 2, len(msgs) - 1):
        b = bytearray(msgs[k])
        b[2:4] = struct.pack(">H", struct.unpack(">H", b[2:4])[0] + 3)
        msgs[k] = bytes(b)
    return msgs


@pytest.mark.parametrize("short", [False, True], ids=["whole", "messages-fall-short"])
def test_slot_returns_the_direct_chain(m, short):
    fr = m["fr"]
    msgs = messages(fr, [1] * len(fr), per=40)
    res, flw, buf = run_slot(m["rx"], 0, fall_short(msgs) if short else msgs)
    assert res["n"] == len(fr) and len(flw["outcome"]) == len(flw["flow"]) == len(fr)
    oc = check(m, res, flw, buf, tag=short)
    ev = flw["ev"]
    assert len(ev) >= 8 and all(((oc & 7) == k).sum() >= 30 for k in range(5)) and int(flw["info"][2]) == 0
    assert ev["last"].max() < len(fr) and (ev["first"] <= ev["last"]).all() and (np.diff(ev["last"].astype(np.int64)) > 0).all()
    # the renumbering: the events' frames are frames the outcome array says were folded, of the event's client
    for e in ev:
        for j in (int(e["first"]), int(e["last"])):
            assert 1 <= flw["outcome"][j] & 7 <= 3 and int(res["rec"][j]["client_id"]) == int(e["client_id"])
    assert (flw["flow"] <= abi.FLOW_ID_MAX).sum() >= 30 and (flw["flow"] == abi.FLOW_NEW).sum() >= 30
    # res.* is what the same batch gives with flows off, except one_launch
    off, none, _ = run_slot(m["rx"], 0, fall_short(msgs) if short else msgs, flows=False)
    assert none is None and not res["one_launch"]
    for k in RES_KEYS:
        assert res[k].tobytes() == off[k].tobytes(), k
    assert res["counters"] == off["counters"] and res["n"] == off["n"] and not res["degraded"]


def test_two_slots_in_flight(m):
    rx, fr = m["rx"], m["fr"]
    sets = [fr[:400], fr[150:700]]
    for rnd in range(2):
        tabs, bufs = [], []
        for s in (0, 1):
            rx.ingest_set_answers(s, 0)
            rx.ingest_set_flows(s, True)
            t, b = place(rx, s, messages(sets[s], [1] * len(sets[s]), per=33 + 31 * s))
            tabs.append(t)
            bufs.append(b)
        rx.ingest_submit(0, tabs[0])
        rx.ingest_submit(1, tabs[1])
        out = {}
        for s in (1, 0):  # waited for in the other order
            res = rx.ingest_wait(s)
            out[s] = (res, rx.ingest_flows(s, res["n"]))
        for s in (0, 1):
            check(m, out[s][0], out[s][1], bufs[s], tag=(rnd, s))
        assert out[0][1]["ev"].tobytes() != out[1][1]["ev"].tobytes()
        sets.reverse()  # the slots change roles


def test_flows_beside_answers_and_ping(m):
    """Flows with answers and ping on: emurx_answers and emurx_ping_out as without the stage; flows
    without answers on the same slot: the same flow results."""
    rx = m["rx"]
    fr = list(m["fr"][:500])
    fr[7::10] = [K.arp(i % 7) for i in range(len(fr[7::10]))]  # requests the responder answers
    msgs = messages(fr, [1] * len(fr))

    def batch(slot, flows):
        res, flw, buf = run_slot(rx, slot, msgs, flows=flows, kinds=abi.RSPK_ALL, fams=abi.PNGK_ALL)
        return res, flw, buf, rx.ingest_answers(slot, res["n"]), rx.ingest_ping(slot, res["n"])

    res0, none, _, ans0, png0 = batch(2, False)
    res1, flw1, buf, ans1, png1 = batch(2, True)
    same(ans1, ans0, "answers")
    assert ans1["n_replies"] >= 40
    for k in ("ev", "outcome", "info"):
        assert png1[k].tobytes() == png0[k].tobytes(), k
    for k in RES_KEYS:
        assert res1[k].tobytes() == res0[k].tobytes(), k
    check(m, res1, flw1, buf, tag="with answers")
    res2, flw2, buf2 = run_slot(rx, 2, msgs, flows=True, kinds=0)
    equal(flw2, flw1, "without answers")
    o = abi.Answers()
    assert rx.lib.emurx_ingest_answers(rx.h, 2, C.byref(o)) == abi.EMURX_ENOENT


def test_enoent_and_einval(m):
    rx, lib = m["rx"], m["rx"].lib
    o = abi.FlowsOut()
    f = lib.emurx_ingest_flows
    msgs = messages(m["fr"][:100], [1] * 100)
    assert f(rx.h, 3, C.byref(o)) == abi.EMURX_EINVAL  # before any wait
    assert f(rx.h, abi.INGEST_SLOTS, C.byref(o)) == abi.EMURX_EINVAL and f(rx.h, 3, None) == abi.EMURX_EINVAL
    assert lib.emurx_ingest_set_flows(rx.h, abi.INGEST_SLOTS, 1) == abi.EMURX_EINVAL
    res, none, _ = run_slot(rx, 3, msgs, flows=False)
    assert f(rx.h, 3, C.byref(o)) == abi.EMURX_ENOENT  # the last batch ran without flows
    rx.ingest_set_flows(3, True)
    tab, buf = place(rx, 3, msgs)
    rx.ingest_submit(3, tab)
    assert f(rx.h, 3, C.byref(o)) == abi.EMURX_EINVAL  # a batch in flight
    assert lib.emurx_ingest_set_flows(rx.h, 3, 0) == abi.EMURX_EINVAL
    res = rx.ingest_wait(3)
    check(m, res, rx.ingest_flows(3, res["n"]), buf)
    rx.ingest_set_flows(3, False)
    run_slot(rx, 3, msgs, flows=False)
    assert f(rx.h, 3, C.byref(o)) == abi.EMURX_ENOENT


def test_flows_past_max_bytes(gpu_ok, oracle_built):
    """With flows on, messages that end past cfg.max_bytes are refused (the stage's buffers are sized for it)."""
    from emurx import frames as F
    from emurx.rx import RxPath
    rx = RxPath(0, max_ns=16, max_clients=16, max_frames=1 << 10, max_bytes=4096)
    try:
        msgs = [F.zmq_pack([bytes(60)] * 64)] * 2
        rx.ingest_set_flows(0, True)
        tab, _ = place(rx, 0, msgs)
        with pytest.raises(RuntimeError, match=f"emurx error {abi.EMURX_ENOSPC}"):
            rx.ingest_submit(0, tab)
        rx.ingest_set_flows(0, False)
        rx.ingest_submit(0, tab)
        assert rx.ingest_wait(0)["n"] == 128
        one = [F.zmq_pack([bytes(60)] * 32)]  # within max_bytes: taken, at most max_bytes / 42 + 1 events
        rx.ingest_set_flows(0, True)
        tab, _ = place(rx, 0, one)
        rx.ingest_submit(0, tab)
        res = rx.ingest_wait(0)
        flw = rx.ingest_flows(0, res["n"])
        assert res["n"] == 32 and not flw["info"].any() and not flw["outcome"].any() and len(flw["ev"]) == 0
    finally:
        rx.close()

"""Egress slots (emurx_egress_buffer / _submit / _wait): a slot's msgs, msg_off, plan, status and
plan_info byte for byte against (a) the direct chain on the same batch through the device entry
points, emurx_tx_plan_dev -> emurx_tx_checksum_dev -> emurx_tx_zmq_dev, and (b) the CPU chain
txplan_ref -> tx_ref.tx_checksum -> the oracle's tx framing."""
import ctypes as C

import numpy as np
import pytest

import tx_ref
import txplan_cases
import txplan_ref
import txzmq_util
from emurx import abi

pytestmark = pytest.mark.gpu
KEYS = ["msgs", "msg_off", "plan", "status", "plan_info"]
MAX_FRAMES, MAX_BYTES = 1 << 14, 4 << 20


@pytest.fixture(scope="module")
def rx(gpu_ok, oracle_built):
    from emurx.rx import RxPath
    r = RxPath(0, max_ns=16, max_clients=16, max_frames=MAX_FRAMES, max_bytes=MAX_BYTES)
    yield r
    r.close()


def fill(rx, slot, buf, desc):
    frames, d = rx.egress_buffer(slot)
    assert len(frames) == MAX_BYTES and len(d) == MAX_FRAMES
    frames[:len(buf)] = buf
    d[:len(desc)] = desc
    return len(desc), len(buf)


def slot_run(rx, slot, buf, desc, flags):
    n, nb = fill(rx, slot, buf, desc)
    rx.egress_submit(slot, n, nb, flags)
    return rx.egress_wait(slot)


def direct(rx, buf, desc, flags):
    """(a): the three device entry points on the batch -> the slot result's dict."""
    import torch
    from gpu_util import to_dev
    n, m1 = len(desc), max(len(desc), 1)
    tb, td = to_dev(buf), to_dev(desc)
    txd = torch.zeros(m1 * 16, dtype=torch.uint8, device="cuda")
    plan = torch.zeros(m1, dtype=torch.uint8, device="cuda")
    status = torch.zeros(m1, dtype=torch.uint8, device="cuda")
    pinfo = torch.zeros(abi.TXP_INFO_WORDS, dtype=torch.int64, device="cuda")
    cap = 8 * n + len(buf)
    out = torch.zeros(cap + 16, dtype=torch.uint8, device="cuda")
    off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    zinfo = torch.zeros(2, dtype=torch.int64, device="cuda")
    rx.tx_plan_dev(tb, td, n, txd, plan, pinfo, flags)
    rx.tx_checksum_dev(tb, txd, n, status)
    rx.tx_zmq_dev(tb, td, n, out, cap, off, zinfo)
    torch.cuda.synchronize()
    nm, total = (int(x) for x in zinfo.cpu().numpy())
    return dict(msgs=out.cpu().numpy()[:total], msg_off=off.cpu().numpy().view(np.uint64)[:nm + 1], plan=plan.cpu().numpy()[:n],
                status=status.cpu().numpy()[:n], plan_info=pinfo.cpu().numpy().view(np.uint64), n_msgs=nm, n_frames=n, bytes=total)


def cpu_chain(buf, desc, flags):
    """(b): the Python plan, the Python checksums, the oracle's framing."""
    import pyoracle
    txd, oc, info = txplan_ref.plan(buf, desc, flags)
    out, st = tx_ref.tx_checksum(buf, txd)
    msgs, off, total = pyoracle.tx_zmq(out, desc)
    return dict(msgs=msgs[:total], msg_off=off, plan=oc, status=st, plan_info=info, n_msgs=len(off) - 1, n_frames=len(desc),
                bytes=total)


def same(got, want, tag=None):
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), (tag, k, got[k][:16], want[k][:16])
    for k in ("n_msgs", "n_frames", "bytes"):
        assert got[k] == want[k], (tag, k, got[k], want[k])


_memo = {}


def batch(name):
    """-> (buf, desc, flags, the CPU chain's result), built once and left unchanged."""
    if name not in _memo:
        if name == "corpus":
            # the captures with every checksum field their producers computed cleared (a captured
            # UDP field of 00 00 was not computed: the plan with UDP0_KEEP), sent by a caller who
            # stubbed its checksum calls out: flags 0
            from test_oracle_corpus import corpus_batch
            cbuf, desc, _ = corpus_batch()
            keep = txplan_ref.plan(cbuf, desc, abi.TXP_UDP0_KEEP)[0]
            buf, flags = txplan_ref.clear_fields(cbuf, keep), 0
            _memo["captured"] = cbuf
            _memo["udp0"] = np.nonzero(keep["ops"] != txplan_ref.plan(cbuf, desc, 0)[0]["ops"])[0]
        elif name == "threshold":
            buf, desc = txzmq_util.threshold_batch()
            flags = 0
        elif name == "cases":
            buf, desc, _, _ = txplan_cases.batch(0)
            flags = 0
        elif name == "small":
            buf, desc = txzmq_util.batch(70, 0, seed=3)
            flags = abi.TXP_UDP0_KEEP
        want = cpu_chain(buf, desc, flags)
        for a in (buf, desc, *[want[k] for k in KEYS]):
            a.setflags(write=False)
        _memo[name] = (buf, desc, flags, want)
    return _memo[name]


def test_zeroed_captures_come_back_framed(rx):
    """The capture frames with their checksum fields cleared: the slot's messages carry the captured
    bytes (the frames the captures sent with a UDP field of 00 00 under UDP0_KEEP, where that means
    "not used"; without the flag it is computed), and they parse as the captures do."""
    import pyoracle
    from emurx.rx import zmq_descriptors
    from test_gpu_ingest_answers import unframe
    buf, desc, flags, want = batch("corpus")
    got = slot_run(rx, 0, buf, desc, flags)
    same(got, want, "cpu")
    same(got, direct(rx, buf, desc, flags), "direct")
    assert not got["status"].any() and got["n_frames"] == len(desc)
    assert all(got["plan_info"][o] > 0 for o in (abi.TXP_NONE, abi.TXP_HDR, abi.TXP_L4, abi.TXP_LENGTH))
    captured, udp0 = _memo["captured"], _memo["udp0"]
    frames = [captured[int(d["off"]):int(d["off"]) + int(d["len"])].tobytes() for d in desc]
    sent = unframe(got["msgs"], got["msg_off"])
    assert len(sent) == len(frames) and 0 < len(udp0) < 200
    # a captured UDP field of 00 00 is computed without the flag; every other frame is the capture's
    assert [i for i in range(len(frames)) if sent[i] != frames[i]] == udp0.tolist()
    # those frames from a caller whose plugins left the field unused on purpose: UDP0_KEEP
    sub = np.ascontiguousarray(desc[udp0])
    kept = slot_run(rx, 1, buf, sub, abi.TXP_UDP0_KEEP)
    same(kept, cpu_chain(buf, sub, abi.TXP_UDP0_KEEP), "udp0 cpu")
    assert unframe(kept["msgs"], kept["msg_off"]) == [frames[i] for i in udp0]
    assert kept["plan_info"][abi.TXP_HDR] + kept["plan_info"][abi.TXP_NONE] == len(udp0)
    # the messages through the library's own walk, then the rx oracle over what it found
    walked = []
    for m in range(got["n_msgs"]):
        a, b = int(got["msg_off"][m]), int(got["msg_off"][m + 1])
        rc, d, err = zmq_descriptors(got["msgs"][a:b].tobytes())
        assert rc == 0 and err == 0
        d = d.copy()
        d["off"] += a
        walked.append(d)
    walked = np.concatenate(walked)
    assert len(walked) == len(desc) and np.array_equal(walked["len"], desc["len"]) and np.array_equal(walked["vport"], desc["vport"])
    o = pyoracle.Oracle()
    was = o.rx_batch(captured, desc)[0]
    now = o.rx_batch(got["msgs"], walked)[0]
    assert (was["status"] == 0).sum() > 7000 and np.array_equal(now["status"], was["status"])
    assert np.array_equal(now["proto"], was["proto"])


@pytest.mark.parametrize("name", ["threshold", "cases"])
def test_batches_against_both_chains(rx, name):
    """threshold: frames exactly at the 32 KiB rule and the 64-frame burst, random bytes (mostly
    NONE and BAD plans, lengths up to 65535); cases: every branch of the planner."""
    buf, desc, flags, want = batch(name)
    got = slot_run(rx, 1, buf, desc, flags)
    same(got, want, "cpu")
    same(got, direct(rx, buf, desc, flags), "direct")
    if name == "threshold":
        assert got["n_msgs"] > 8 and int(desc["len"].max()) == 65535


def test_n_zero(rx):
    got = slot_run(rx, 0, np.zeros(0, np.uint8), np.zeros(0, abi.DESC_DTYPE), 0)
    assert got["n_msgs"] == 0 and got["n_frames"] == 0 and got["bytes"] == 0
    assert got["msg_off"].tolist() == [0] and not got["plan_info"].any() and len(got["msgs"]) == 0
    same(got, direct(rx, np.zeros(0, np.uint8), np.zeros(0, abi.DESC_DTYPE), 0), "direct")


def test_large_then_small_on_one_slot(rx):
    """Nothing of the larger batch shows in the smaller one's result."""
    buf, desc, flags, want = batch("corpus")
    same(slot_run(rx, 1, buf, desc, flags), want, "large")
    sbuf, sdesc, sflags, swant = batch("small")
    got = slot_run(rx, 1, sbuf, sdesc, sflags)
    same(got, swant, "small")
    same(got, direct(rx, sbuf, sdesc, sflags), "small direct")
    same(slot_run(rx, 1, buf, desc, flags), want, "large again")


def test_both_slots_in_flight(rx):
    b0, b1 = batch("corpus"), batch("cases")
    n0, nb0 = fill(rx, 0, b0[0], b0[1])
    n1, nb1 = fill(rx, 1, b1[0], b1[1])
    rx.egress_submit(0, n0, nb0, b0[2])
    rx.egress_submit(1, n1, nb1, b1[2])
    got1 = rx.egress_wait(1)
    got0 = rx.egress_wait(0)
    same(got0, b0[3], "slot 0")
    same(got1, b1[3], "slot 1")
    # the other order of submits, the slots swapped
    n0, nb0 = fill(rx, 0, b1[0], b1[1])
    n1, nb1 = fill(rx, 1, b0[0], b0[1])
    rx.egress_submit(1, n1, nb1, b0[2])
    rx.egress_submit(0, n0, nb0, b1[2])
    same(rx.egress_wait(0), b1[3], "slot 0 swapped")
    same(rx.egress_wait(1), b0[3], "slot 1 swapped")


def test_beside_an_ingest_slot_with_answers(gpu_ok, oracle_built):
    """An egress batch in flight beside an ingest slot whose answer stages frame their replies with
    the same scratch: each equals its solo result, in both submit orders."""
    import sim_envs as S
    import test_gpu_ingest_answers as A
    from emurx.rx import RxPath
    from test_oracle_corpus import GOLD
    z = np.load(GOLD, allow_pickle=False)
    fr = S.rx_frames(z, "icmp1.json") * 40  # echo requests: every one gets a framed reply
    msgs = A.messages(fr, [1] * len(fr), 64)
    buf, desc, flags, want = batch("corpus")
    rx = RxPath(0, max_ns=16, max_clients=16, max_frames=MAX_FRAMES, max_bytes=MAX_BYTES)
    try:
        rx.register_all()
        S.load_env(rx, next(c[1] for c in A._capture_params() if c[0] == "icmp1.json"))
        n, nb = fill(rx, 0, buf, desc)
        res, solo, _ = A.run_slot(rx, 0, msgs, abi.RSPK_ALL)
        assert solo["n_replies"] == len(fr) and solo["n_tx_msgs"] >= 2
        same(slot_run(rx, 0, buf, desc, flags), want, "egress solo")
        for order in (0, 1):
            tab, _ = A.place(rx, 0, msgs)
            if order == 0:
                rx.ingest_submit(0, tab)
                rx.egress_submit(0, n, nb, flags)
            else:
                rx.egress_submit(0, n, nb, flags)
                rx.ingest_submit(0, tab)
            got = rx.egress_wait(0)
            r2 = rx.ingest_wait(0)
            a2 = rx.ingest_answers(0, r2["n"])
            same(got, want, ("egress", order))
            A.same(a2, solo, ("ingest", order))
            assert r2["rec"].tobytes() == res["rec"].tobytes()
    finally:
        rx.close()


def test_return_codes(gpu_ok):
    from emurx.rx import RxPath
    rx = RxPath(0, max_ns=16, max_clients=16, max_frames=256, max_bytes=1 << 16)
    lib, h = rx.lib, rx.h
    try:
        r = abi.EgressResult()
        f, d = C.c_void_p(), C.c_void_p()
        assert lib.emurx_egress_wait(h, 0, C.byref(r)) == abi.EMURX_EINVAL            # nothing submitted
        assert lib.emurx_egress_submit(h, 0, 0, 0, 0) == abi.EMURX_EINVAL             # no buffer yet
        assert lib.emurx_egress_buffer(h, abi.EGRESS_SLOTS, C.byref(f), C.byref(d)) == abi.EMURX_EINVAL
        frames, desc = rx.egress_buffer(0)
        assert lib.emurx_egress_wait(h, 0, C.byref(r)) == abi.EMURX_EINVAL            # still nothing submitted
        desc[0] = (0, 100, 1, 0)
        desc[1] = (100, 101, 1, 0)
        assert lib.emurx_egress_submit(h, 0, 2, 200, 0) == abi.EMURX_EINVAL           # desc[1] ends past bytes
        assert lib.emurx_egress_submit(h, 0, 2, 201, 2) == abi.EMURX_EINVAL           # unknown flag
        assert lib.emurx_egress_submit(h, 0, 257, 201, 0) == abi.EMURX_ENOMEM         # n > cfg.max_frames
        assert lib.emurx_egress_submit(h, 0, 2, (1 << 16) + 1, 0) == abi.EMURX_ENOSPC  # bytes > cfg.max_bytes
        assert lib.emurx_egress_submit(h, abi.EGRESS_SLOTS, 2, 201, 0) == abi.EMURX_EINVAL
        assert lib.emurx_egress_wait(h, 0, C.byref(r)) == abi.EMURX_EINVAL            # none of them submitted anything
        assert lib.emurx_egress_submit(h, 0, 2, 201, 0) == 0
        assert lib.emurx_egress_submit(h, 0, 2, 201, 0) == abi.EMURX_EINVAL           # still in flight
        assert lib.emurx_egress_buffer(h, 0, C.byref(f), C.byref(d)) == abi.EMURX_EINVAL
        assert lib.emurx_egress_wait(h, 0, C.byref(r)) == 0 and r.n_frames == 2 and r.n_msgs == 1
        assert r.bytes == 4 + 4 + 100 + 4 + 101
        assert lib.emurx_egress_wait(h, 0, C.byref(r)) == 0 and r.n_frames == 2       # the result stays until the next submit
        assert lib.emurx_egress_wait(h, 1, C.byref(r)) == abi.EMURX_EINVAL            # the other slot has nothing
        assert lib.emurx_egress_buffer(h, 0, C.byref(f), C.byref(d)) == 0 and f.value == frames.ctypes.data
    finally:
        rx.close()

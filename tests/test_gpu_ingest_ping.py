"""The ping fold on an ingest slot (emurx_ingest_set_ping / emurx_ingest_set_now / emurx_ingest_ping):
every batch is compared byte for byte with the direct chain on the same handle -- the slot's buffer
uploaded, res.desc as the descriptors, classify_dev, then ping_dev with the slot's now -- and with
ping_ref; the answers of emurx_ingest_answers do not change with the stage on."""
import ctypes as C
import struct

import numpy as np
import pytest

import ping_cases as K
import ping_ref as P
from emurx import abi
from test_gpu_ingest_answers import messages, place, same

pytestmark = pytest.mark.gpu

LATER = K.NOW + 3_000_000_000  # a second slot's time: three seconds on, other latencies and classes


def direct(rx, buf, desc, now, fams=abi.PNGK_ALL):
    """classify_dev + ping_dev on the closed batch -> dict(ev, outcome, info), the records."""
    import torch
    from gpu_util import to_dev
    n = len(desc)
    tb, td = to_dev(buf), to_dev(desc)
    trec = torch.zeros(max(n, 1) * 32, dtype=torch.uint8, device="cuda")
    hist = torch.zeros(abi.HIST_SHARDS * 2 * abi.HIST_BINS, dtype=torch.int64, device="cuda")
    rx.classify_dev(tb, td, n, trec, None, 0, None, hist)
    cap = rx.ping_max_events()
    ev = torch.zeros(cap * 80, dtype=torch.uint8, device="cuda")
    oc = torch.zeros(max(n, 1), dtype=torch.uint8, device="cuda")
    info = torch.zeros(abi.PNG_INFO_WORDS, dtype=torch.int64, device="cuda")
    rx.ping_dev(tb, td, trec, n, now, ev, cap, oc, info, fams=fams)
    torch.cuda.synchronize()
    iw = info.cpu().numpy().view(np.uint64)
    return dict(ev=ev.cpu().numpy()[: int(iw[0]) * 80].view(abi.PING_EV_DTYPE), outcome=oc.cpu().numpy()[:n], info=iw), \
        trec.cpu().numpy()[: n * 32].view(abi.REC_DTYPE)


def equal(got, want, tag=None):
    for k in ("ev", "outcome", "info"):
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), (tag, k, got[k][:4], want[k][:4])


def check(m, res, png, buf, now, fams=abi.PNGK_ALL, tag=None):
    """The slot's fold equals the direct chain's and ping_ref's on the closed batch."""
    want, rec = direct(m["rx"], buf, res["desc"], now, fams)
    assert res["rec"].tobytes() == rec.tobytes(), tag
    equal(png, want, tag)
    ref = P.ping_batch(buf, res["desc"], res["rec"], m["env"], fams, now)
    assert np.array_equal(png["outcome"], ref[0]) and png["ev"].tobytes() == ref[1].tobytes() and \
        np.array_equal(png["info"], ref[2]), tag
    return ref


@pytest.fixture(scope="module")
def m(gpu_ok, oracle_built):
    from emurx.rx import RxPath
    rx = RxPath(0, max_ns=16, max_clients=64, max_frames=1 << 12, max_bytes=1 << 20)
    rx.register_all()
    env = P.Env()
    K.load_tables(rx, env)
    yield dict(rx=rx, env=env, fr=K.stream(700, seed=5))
    rx.close()


def run_slot(rx, slot, msgs, now, fams=abi.PNGK_ALL, kinds=abi.RSPK_ALL):
    rx.ingest_set_answers(slot, kinds)
    rx.ingest_set_ping(slot, fams)
    rx.ingest_set_now(slot, now)
    tab, buf = place(rx, slot, msgs)
    rx.ingest_submit(slot, tab)
    res = rx.ingest_wait(slot)
    return res, rx.ingest_answers(slot, res["n"]), rx.ingest_ping(slot, res["n"]), buf


@pytest.mark.parametrize("short", [False, True], ids=["whole", "messages-fall-short"])
def test_slot_returns_the_direct_chain(m, short):
    fr = m["fr"]
    msgs = messages(fr, [1] * len(fr), per=40)
    if short:  # three messages announce 3 frames more than they carry: hole slots, closed by the wait
        for k in (0, len(msgs) // 2, len(msgs) - 1):
            b = bytearray(msgs[k])
            b[2:4] = struct.pack(">H", struct.unpack(">H", b[2:4])[0] + 3)
            msgs[k] = bytes(b)
    res, ans, png, buf = run_slot(m["rx"], 0, msgs, K.NOW)
    assert res["n"] == len(fr) and len(png["outcome"]) == len(fr)
    ref = check(m, res, png, buf, K.NOW, tag=short)
    ev = png["ev"]
    assert len(ev) >= 8 and all((ref[0] == k).sum() >= 5 for k in range(6)) and int(png["info"][2]) == 0
    assert ev["last"].max() < len(fr) and (ev["first"] <= ev["last"]).all() and (np.diff(ev["last"].astype(np.int64)) > 0).all()
    # the events' frames are frames the outcome array says were folded
    assert (png["outcome"][ev["last"]] != 0).all() and (png["outcome"][ev["first"]] != 0).all()
    # one family alone on the same slot
    res4, _, png4, buf4 = run_slot(m["rx"], 0, msgs, K.NOW, fams=abi.PNGK_V4)
    check(m, res4, png4, buf4, K.NOW, abi.PNGK_V4, tag=(short, 4))
    assert 0 < len(png4["ev"]) < len(ev)


def test_two_slots_in_flight_carry_their_own_now(m):
    rx, fr = m["rx"], m["fr"]
    sets = [fr[:400], fr[150:700]]
    nows = [K.NOW, LATER]
    for rnd in range(2):
        tabs, bufs = [], []
        for s in (0, 1):
            rx.ingest_set_answers(s, abi.RSPK_ALL)
            rx.ingest_set_ping(s, abi.PNGK_ALL)
            rx.ingest_set_now(s, nows[s])
            t, b = place(rx, s, messages(sets[s], [1] * len(sets[s]), per=33 + 31 * s))
            tabs.append(t)
            bufs.append(b)
        rx.ingest_submit(0, tabs[0])
        rx.ingest_set_now(1, nows[1])  # a store between the submits: slot 0's batch keeps its own
        rx.ingest_submit(1, tabs[1])
        out = {}
        for s in (1, 0):  # waited for in the other order
            res = rx.ingest_wait(s)
            out[s] = (res, rx.ingest_ping(s, res["n"]))
        for s in (0, 1):
            check(m, out[s][0], out[s][1], bufs[s], nows[s], tag=(rnd, s))
        sets.reverse()  # the slots change roles
    # the time matters: the same frames under the other slot's now fold differently
    other, _ = direct(rx, bufs[0], out[0][0]["desc"], nows[1])
    assert other["ev"].tobytes() != out[0][1]["ev"].tobytes()


def test_ping_off_leaves_the_answers_alone(m):
    """ENOENT without the stage; emurx_ingest_answers is byte-identical with ping on, off again,
    and on a slot that never saw a ping call."""
    rx, fr = m["rx"], m["fr"][:500]
    msgs = messages(fr, [1] * len(fr))
    o = abi.PingOut()
    f = rx.lib.emurx_ingest_ping

    def answers_only(slot):
        rx.ingest_set_answers(slot, abi.RSPK_ALL)
        tab, _ = place(rx, slot, msgs)
        rx.ingest_submit(slot, tab)
        res = rx.ingest_wait(slot)
        assert f(rx.h, slot, C.byref(o)) == abi.EMURX_ENOENT
        return res, rx.ingest_answers(slot, res["n"])

    assert f(rx.h, 3, C.byref(o)) == abi.EMURX_EINVAL  # before any wait
    assert rx.lib.emurx_ingest_set_ping(rx.h, 3, abi.PNGK_ALL) == abi.EMURX_EINVAL  # answers are off on slot 3
    never_res, never = answers_only(2)  # no ping call on slot 2, ever
    on_res, on, png, _ = run_slot(rx, 0, msgs, K.NOW)
    assert len(png["ev"]) >= 6
    same(on, never, "on")
    assert on_res["rec"].tobytes() == never_res["rec"].tobytes() and on_res["qlist"].tobytes() == never_res["qlist"].tobytes()
    rx.ingest_set_ping(0, 0)
    _, off = answers_only(0)
    same(off, never, "off")
    # turning answers off turns ping off: answers on again, and still no ping
    rx.ingest_set_ping(0, abi.PNGK_ALL)
    rx.ingest_set_answers(0, 0)
    _, again = answers_only(0)
    same(again, never, "again")


def test_ping_in_flight_and_arguments(m):
    rx = m["rx"]
    lib = rx.lib
    msgs = messages(m["fr"][:100], [1] * 100)
    rx.ingest_set_answers(1, abi.RSPK_ICMP)  # any kinds will do
    rx.ingest_set_ping(1, abi.PNGK_V6)
    assert lib.emurx_ingest_set_ping(rx.h, 1, 4) == abi.EMURX_EINVAL
    assert lib.emurx_ingest_set_ping(rx.h, abi.INGEST_SLOTS, 1) == abi.EMURX_EINVAL
    assert lib.emurx_ingest_set_now(rx.h, 1, 1 << 63) == abi.EMURX_EINVAL
    assert lib.emurx_ingest_set_now(rx.h, abi.INGEST_SLOTS, 1) == abi.EMURX_EINVAL
    assert lib.emurx_ingest_ping(rx.h, 1, None) == abi.EMURX_EINVAL
    rx.ingest_set_now(1, K.NOW)
    tab, buf = place(rx, 1, msgs)
    rx.ingest_submit(1, tab)
    o = abi.PingOut()
    assert lib.emurx_ingest_ping(rx.h, 1, C.byref(o)) == abi.EMURX_EINVAL  # a batch in flight
    assert lib.emurx_ingest_set_ping(rx.h, 1, 0) == abi.EMURX_EINVAL
    assert lib.emurx_ingest_set_now(rx.h, 1, 5) == abi.EMURX_EINVAL
    res = rx.ingest_wait(1)
    check(m, res, rx.ingest_ping(1, res["n"]), buf, K.NOW, abi.PNGK_V6)

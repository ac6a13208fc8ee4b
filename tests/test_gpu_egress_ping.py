"""Echo requests on an egress slot (emurx_egress_ping_buffer / _submit_ping): the slot's result
against the CPU chain, txplan_ref -> tx_ref.tx_checksum on the plain frames, pingtx_ref.generate's
frames behind them, the oracle's tx framing over all of them; the submit's errors; and the
lifetime of a removed template id."""
import ctypes as C
import random
from pathlib import Path

import numpy as np
import pytest

import pingtx_ref as R
import pingtx_util as U
import tx_ref
import txplan_cases
import txplan_ref
from emurx import abi
from test_gpu_ingest_answers import unframe

pytestmark = pytest.mark.gpu
KEYS = ["msgs", "msg_off", "plan", "status", "plan_info"]
MAX_FRAMES, MAX_BYTES, MAX_PINGS = 2048, 1 << 20, 64
TS = 0x1122334455667788
GOLDEN = Path(__file__).parent / "golden" / "corpus_frames.npz"


@pytest.fixture(scope="module")
def env(gpu_ok, oracle_built):
    from emurx.rx import RxPath
    rx = RxPath(0, max_ns=16, max_clients=16, max_frames=MAX_FRAMES, max_bytes=MAX_BYTES)
    st = U.Store(rx, MAX_PINGS)
    for s in range(abi.EGRESS_SLOTS):
        rx.egress_buffer(s)
        assert len(rx.egress_ping_buffer(s)) == MAX_FRAMES
    yield rx, st
    rx.close()


@pytest.fixture(scope="module")
def pool(env):
    """The two simulations' templates and six more of other lengths; ids 0..7, never removed."""
    rx, st = env
    rng = random.Random(3)
    ids = [st.add(t, off, vport=1) for off, t in U.capture_templates()]
    for k in range(6):
        off = 34 + 3 * k
        ids.append(st.add(U.raw_template(rng, off + 24 + 9 * k, off), off, vport=10 + k))
    assert ids == list(range(8))
    return ids


_plain = {}


def plain(name):
    """-> (buf, desc, flags), built once and left unchanged."""
    if name not in _plain:
        if name == "none":
            buf, desc = np.zeros(0, np.uint8), np.zeros(0, abi.DESC_DTYPE)
        else:  # a small batch of the planner's cases: every branch, odd offsets
            buf, desc, _, _ = txplan_cases.batch(0)
            buf, desc = buf[:int(desc["off"][39]) + int(desc["len"][39])].copy(), desc[:40].copy()
        for a in (buf, desc):
            a.setflags(write=False)
        _plain[name] = (buf, desc, 0)
    return _plain[name]


def cpu_chain(buf, desc, flags, mirror, reqs):
    import pyoracle
    txd, oc, info = txplan_ref.plan(buf, desc, flags)
    out, st = tx_ref.tx_checksum(buf, txd)
    gf, gd, _, gi = R.generate(mirror, reqs, U.HUGE, U.HUGE)
    base = R.align16(len(buf))
    area = np.zeros(base + int(gi[1]) + 16, np.uint8)
    area[:len(out)] = out
    gd = gd.copy()
    gd["off"] += base
    for f, d in zip(gf, gd):
        area[int(d["off"]):int(d["off"]) + len(f)] = np.frombuffer(f, np.uint8)
    alld = np.concatenate([np.asarray(desc), gd]) if len(gd) else np.asarray(desc)
    msgs, off, total = pyoracle.tx_zmq(area, alld)
    g = len(gf)
    return dict(msgs=msgs[:total], msg_off=off, plan=np.concatenate([oc, np.zeros(g, np.uint8)]),
                status=np.concatenate([st, np.zeros(g, np.uint8)]), plan_info=info, n_msgs=len(off) - 1, n_frames=len(alld),
                bytes=total, frames=gf)


def same(got, want, tag=None):
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), (tag, k, got[k][:16], want[k][:16])
    for k in ("n_msgs", "n_frames", "bytes"):
        assert got[k] == want[k], (tag, k, got[k], want[k])


def fill(rx, slot, buf, desc, reqs):
    frames, d = rx.egress_buffer(slot)
    frames[:len(buf)] = buf
    d[:len(desc)] = desc
    rx.egress_ping_buffer(slot)[:len(reqs)] = U.reqs_array(reqs)
    return len(desc), len(buf), len(reqs)


def slot_run(rx, slot, buf, desc, flags, reqs):
    n, nb, nr = fill(rx, slot, buf, desc, reqs)
    assert rx.egress_submit_ping(slot, n, nb, nr, flags) == 0
    return rx.egress_wait(slot)


@pytest.mark.parametrize("name", ["cases", "none"])
def test_plain_frames_and_requests_equal_the_cpu_chain(env, pool, name):
    rx, st = env
    buf, desc, flags = plain(name)
    reqs = [(pool[k % 8], 0xFFF0 + k, [1, 3, 0, 2][k % 4], TS + k) for k in range(12)]
    want = cpu_chain(buf, desc, flags, st.m, reqs)
    got = slot_run(rx, 0, buf, desc, flags, reqs)
    same(got, want, name)
    n = len(desc)
    assert got["n_frames"] == n + 18 and not got["plan"][n:].any() and not got["status"][n:].any()
    assert int(got["plan_info"].sum()) == n  # the plain frames only
    assert unframe(got["msgs"], got["msg_off"])[n:] == want["frames"]


def test_the_captured_requests_come_out_framed(env, pool):
    rx, st = env
    z = np.load(GOLDEN)
    caps = (U.capture_frames(z, "icmp3.json", (1824, 1826, 1828, 1830, 1832)) +
            U.capture_frames(z, "ipv6ping_rpc.json", (6854, 6857, 6860, 6863, 6866)))
    got = slot_run(rx, 1, *plain("none"), [(pool[0], R.SIM_SEQ, 5, R.SIM_TS), (pool[1], R.SIM_SEQ, 5, R.SIM_TS)])
    assert unframe(got["msgs"], got["msg_off"]) == caps and got["n_msgs"] == 1


def test_no_requests_is_the_plain_submit(env, pool):
    rx, st = env
    buf, desc, flags = plain("cases")
    got = slot_run(rx, 0, buf, desc, flags, [])
    n, nb, _ = fill(rx, 1, buf, desc, [])
    rx.egress_submit(1, n, nb, flags)
    same(got, rx.egress_wait(1), "plain")
    same(got, cpu_chain(buf, desc, flags, st.m, []), "cpu")


@pytest.mark.parametrize("g", [64, 65])
def test_the_framing_burst_edge(env, pool, g):
    rx, st = env
    reqs = [(pool[0], 7, g - 1, TS), (pool[1], 9, 1, TS)]
    got = slot_run(rx, 0, *plain("none"), reqs)
    same(got, cpu_chain(*plain("none"), st.m, reqs), g)
    assert got["n_msgs"] == (1 if g == 64 else 2) and got["n_frames"] == g


def test_generated_bytes_close_a_message_at_32768(env, pool):
    """A frame that would bring the open message's frame bytes to 32,768 or more closes it first
    (veth_zmq.go:186-188).  Behind a plain frame of P bytes the k-th generated 70-byte frame does so
    when P + 70 k >= 32768: with P = 32768 - 70 * 40 the 40th meets the bound exactly and the first
    message has 40 frames; one byte less and it has 41."""
    rx, st = env
    rng = np.random.default_rng(1)
    assert len(st.m[pool[0]][0]) == 70
    for plain_len, first_msg in ((32768 - 70 * 40, 40), (32768 - 70 * 40 - 1, 41)):
        buf = rng.integers(0, 256, plain_len, dtype=np.uint8)
        desc = np.zeros(1, abi.DESC_DTYPE)
        desc[0] = (0, plain_len, 1, 0)
        reqs = [(pool[0], 0, 100, TS)]
        want = cpu_chain(buf, desc, 0, st.m, reqs)
        got = slot_run(rx, 1, buf, desc, 0, reqs)
        same(got, want, plain_len)
        b = got["msgs"]
        assert (int(b[2]) << 8 | int(b[3])) == first_msg and got["n_msgs"] == 2, plain_len


def test_submit_errors_enqueue_nothing(env, pool):
    rx, st = env
    lib, h = rx.lib, rx.h
    r = abi.EgressResult()
    buf, desc, flags = plain("cases")
    good = [(pool[0], 1, 2, TS)]
    want = cpu_chain(buf, desc, flags, st.m, good)
    same(slot_run(rx, 0, buf, desc, flags, good), want, "before")
    seen = rx.egress_wait(0)
    L = len(st.m[pool[0]][0])
    a16 = R.align16(L)
    for reqs, n, nb, code in (
            ([(pool[0], 1, 2, TS), (50, 1, 0, TS)], None, None, abi.EMURX_EINVAL),            # a free id, even with count 0
            ([(MAX_PINGS, 1, 1, TS)], None, None, abi.EMURX_EINVAL),                          # an id out of range
            ([(pool[0], 1, MAX_FRAMES - len(desc) + 1, TS)], None, None, abi.EMURX_ENOMEM),   # n + G > cfg.max_frames
            ([(pool[0], 1, 65535, TS)] * 3, None, None, abi.EMURX_ENOMEM),
            ([(pool[0], 1, 2, TS)], None, MAX_BYTES - 2 * a16 + 1, abi.EMURX_ENOSPC),         # align16(bytes) + B > cfg.max_bytes
            ([(pool[0], 1, 2, TS)], len(desc) + 1, None, abi.EMURX_EINVAL)):                  # a descriptor past `bytes`
        nn, nbb, nr = fill(rx, 0, buf, desc, reqs)
        rx.egress_buffer(0)[1][len(desc)] = (len(buf), 1, 0, 0)
        assert rx.egress_submit_ping(0, nn if n is None else n, nbb if nb is None else nb, nr, flags) == code, (reqs[0], code)
        # nothing was enqueued: the slot is not in flight and still holds the last result
        same(rx.egress_wait(0), seen, "after an error")
    assert rx.egress_submit_ping(0, 0, 0, MAX_FRAMES + 1, 0) == abi.EMURX_ENOMEM
    assert lib.emurx_egress_submit_ping(h, 0, 0, 0, 2, 1) == abi.EMURX_EINVAL
    # the largest batch that fits, to the byte, and the slot is as usable as before
    nb_max = MAX_BYTES - 2 * a16
    assert nb_max % 16 == 0
    big = np.zeros(nb_max, np.uint8)
    d1 = np.zeros(1, abi.DESC_DTYPE)
    d1[0] = (nb_max - 60, 60, 3, 0)
    got = slot_run(rx, 0, big, d1, 0, good)
    same(got, cpu_chain(big, d1, 0, st.m, good), "to the byte")
    same(slot_run(rx, 0, buf, desc, flags, good), want, "after")
    assert lib.emurx_egress_wait(h, 0, C.byref(r)) == 0 and r.n_frames == len(desc) + 2


def test_two_slots_pipelined(env, pool):
    rx, st = env
    buf, desc, flags = plain("cases")
    r0 = [(pool[k % 8], k, 1 + k % 3, TS) for k in range(30)]
    r1 = [(pool[(k + 3) % 8], 0xFFFF, 70, TS + 1) for k in range(4)]
    w0, w1 = cpu_chain(buf, desc, flags, st.m, r0), cpu_chain(*plain("none"), st.m, r1)
    for order in (0, 1):
        a = fill(rx, 0, buf, desc, r0)
        b = fill(rx, 1, *plain("none")[:2], r1)
        for s in ((0, 1) if order == 0 else (1, 0)):
            n, nb, nr = (a, b)[s]
            assert rx.egress_submit_ping(s, n, nb, nr, flags) == 0
        same(rx.egress_wait(1), w1, ("slot 1", order))
        same(rx.egress_wait(0), w0, ("slot 0", order))


def test_a_removed_id_is_not_reused_while_a_batch_may_read_it(env, pool):
    rx, st = env
    rng = random.Random(21)
    tx, ty = U.raw_template(rng, 120, 50), U.raw_template(rng, 77, 40)
    x = st.add(tx, 50, 5)
    rx0 = [(x, 0xFFFE, 300, TS), (pool[2], 1, 1, TS)]
    w0 = cpu_chain(*plain("none"), st.m, rx0)
    n, nb, nr = fill(rx, 0, *plain("none")[:2], rx0)
    assert rx.egress_submit_ping(0, n, nb, nr, 0) == 0               # 1. in flight with X
    st.remove(x)                                                      # 2.
    y = st.add(ty, 40, 6)                                             # 3. a different template: not X's id
    assert y != x
    ry = [(y, 3, 4, TS), (pool[3], 1, 1, TS)]
    w1 = cpu_chain(*plain("none"), st.m, ry)
    n, nb, nr = fill(rx, 1, *plain("none")[:2], ry)
    assert rx.egress_submit_ping(1, n, nb, nr, 0) == 0               # 4.
    same(rx.egress_wait(1), w1, "slot 1")                             # 5. both as submitted: slot 0 carries X's bytes
    same(rx.egress_wait(0), w0, "slot 0")
    z = st.add(ty, 40, 7)                                             # 6. after the waits the id may come back
    assert z == x
    got = slot_run(rx, 0, *plain("none"), [(z, 3, 2, TS)])
    same(got, cpu_chain(*plain("none"), st.m, [(z, 3, 2, TS)]), "X's id with its next template")
    st.remove(y)
    st.remove(z)

"""The responder and the learning fold on batches of more than 1,024 tiles: k_rsp_scan and
k_lrn_scan are one workgroup of 1,024 lanes that loops over the tiles 1,024 at a time and carries
the replies, rows and emitters of a round into the next, so up to 262,144 frames the loop runs once
and every carry is added to zero.  The sizes here are the smallest with one full round (262,144),
one frame in a second round (262,145), 16 full tiles in it (266,240) and a third round (528,384).

A large batch is a unit of 4,096 frames whose descriptors are repeated over one frame buffer.  The
references (nd_ref, learn_ref) run on the unit once; what the device must give for the large batch
follows from the unit's reference by rule on the host: outcomes tiled, reply bytes repeated in
order, out_desc.off the running sum of the rows, out_src shifted by 4,096 per repetition, the
counts of d_info as multiples plus the prefix of a ragged end; events folded by learn_ref.fold over
the unit's keys repeated.  Checked with the checks of test_gpu_respond and test_gpu_learn as they
are: bit-exact, nothing before the outputs, nothing past the bytes or entries written."""
import numpy as np
import pytest

import learn_ref as L
import nd_ref as N
import respond_ref as R
from emurx import abi
from test_gpu_learn import check as check_learn, learn
from test_gpu_respond import check as check_respond, classify
from test_gpu_respond_nd import respond

pytestmark = pytest.mark.gpu

UNIT, TILE, ROUND = 4096, 256, 1024 * 256  # frames: the unit, a tile, one round of either scan
MAX_FRAMES = 129 * UNIT
SIZES = [ROUND, ROUND + 1, 65 * UNIT, 129 * UNIT]


@pytest.fixture(scope="module")
def big(gpu_ok, oracle_built):
    """One handle for every batch of this module (the handle's open and first classify at 528,384
    frames are most of the module's time), the responder's unit classified, and its references."""
    from emurx.rx import RxPath
    rx = RxPath(0, max_ns=16, max_clients=64, max_frames=MAX_FRAMES)
    rx.register_all()
    env4, env6 = R.Env(), N.Env()
    N.load_combined(rx, env4, env6)
    buf, desc = R.pack_with_holes(*N.combined_batch(UNIT), N.HOLE_EVERY)
    _, _, _, rec = classify(rx, buf, desc)
    m = dict(rx=rx, env4=env4, env6=env6, buf=buf, desc=desc, rec=rec, ref={}, dev={})
    yield m
    rx.close()


def unit_ref(m, kinds, words, r=UNIT):
    """nd_ref.respond_batch of the unit's first r frames, computed once."""
    k = (kinds, words, r)
    if k not in m["ref"]:
        m["ref"][k] = N.respond_batch(m["buf"], m["desc"][:r], m["rec"][:r], kinds, m["env4"], m["env6"], info_words=words)
    return m["ref"][k]


def on_device(m, n):
    """The unit's descriptors repeated and cut to n, classified on the device, once per n."""
    if n not in m["dev"]:
        desc = np.tile(m["desc"], -(-n // UNIT))[:n]
        tb, td, trec, rec = classify(m["rx"], m["buf"], desc)
        assert rec.tobytes() == np.tile(m["rec"], -(-n // UNIT))[:n].tobytes()
        m["dev"][n] = (tb, td, trec)
    return m["dev"][n]


def tiled_want(unit, prefix, n):
    """The large batch's outputs from the references of the unit and of its first n % UNIT frames."""
    q = n // UNIT
    (u_out, u_desc, u_src, u_rep, u_info), (p_out, p_desc, p_src, p_rep, p_info) = unit, prefix
    rows = int(u_info[1])
    assert rows % 16 == 0 and len(p_out) == n % UNIT
    outcome = np.concatenate([np.tile(u_out, q), p_out])
    desc = np.concatenate([np.tile(u_desc, q), p_desc])
    desc["off"] = np.concatenate([u_desc["off"].astype(np.int64) + j * rows for j in range(q)] +
                                 [p_desc["off"].astype(np.int64) + q * rows])
    src = np.concatenate([u_src.astype(np.int64) + j * UNIT for j in range(q)] + [p_src.astype(np.int64) + q * UNIT])
    info = u_info * np.uint64(q) + p_info
    assert int(info[0]) == len(desc) and int(info[1]) == q * rows + int(p_info[1])
    return outcome, desc, src.astype(np.uint32), u_rep * q + p_rep, info


def want_at(m, n, kinds, words):
    return tiled_want(unit_ref(m, kinds, words), unit_ref(m, kinds, words, n % UNIT), n)


def test_unit_is_not_trivial(big):
    """A scan that lost a carry would go unnoticed only if the carry were zero: every tile of the
    unit has replies, so tord and trow of every tile behind the first are non-zero, those of tile
    1,024 among them."""
    outcome, desc, src, replies, info = unit_ref(big, abi.RSPK_ALL, None)
    per_tile = np.bincount(src // TILE, minlength=UNIT // TILE)
    assert (per_tile > 0).all() and 4 * len(replies) >= UNIT
    assert all((outcome == k).any() for k in (abi.RSP_ARP, abi.RSP_ICMP, abi.RSP_ICMPV6, abi.RSP_ND, abi.RSP_HOST))
    before = want_at(big, ROUND, abi.RSPK_ALL, None)  # what precedes frame 262,144
    assert int(before[4][0]) > 0 and int(before[4][1]) // 16 > 0
    assert int(before[4][1]) < 1 << 32  # out_desc.off is 32 bits: the largest batch's last offset fits
    assert int(want_at(big, SIZES[-1], abi.RSPK_ALL, None)[4][1]) < 1 << 32


@pytest.mark.parametrize("n", SIZES)
def test_respond_kinds_past_one_round(big, n):
    want = want_at(big, n, abi.RSPK_ALL, None)
    assert len(want[0]) == n and -(-n // TILE) == {SIZES[0]: 1024, SIZES[1]: 1025, SIZES[2]: 1040, SIZES[3]: 2064}[n]
    tb, td, trec = on_device(big, n)
    cap = int(want[4][1])
    check_respond(respond(big["rx"], tb, td, trec, n, cap, abi.RSPK_ALL), want, n, cap)


def test_respond_dev_past_one_round(big):
    """emurx_respond_dev: eight info words, the instantiation without the solicitation path."""
    n = SIZES[2]
    want = want_at(big, n, 7, 8)
    assert abi.RSP_ND not in want[0] and len(want[4]) == 8 and int(want[4][0]) > n // 8
    tb, td, trec = on_device(big, n)
    cap = int(want[4][1])
    check_respond(respond(big["rx"], tb, td, trec, n, cap, None), want, n, cap)


def test_respond_capacity_ends_in_round_two(big):
    """out_cap 16 bytes short of the end of a reply of tile 1,025: the replies before it are
    written, it and every later reply are NOSPC, d_info[1] is the need all the same."""
    n = SIZES[2]
    outcome, desc, src, replies, info = want_at(big, n, abi.RSPK_ALL, None)
    j = int(np.searchsorted(src, ROUND + TILE + 40))  # the first reply from frame 262,440 on
    assert j < len(src) - 1000 and src[j] // TILE >= 1024
    cap = int(desc["off"][j]) + R.align16(int(desc["len"][j])) - 16
    outcome = outcome.copy()
    outcome[src[j:]] = abi.RSP_NOSPC
    winfo = np.zeros(abi.RSP_INFO_WORDS, np.uint64)
    winfo[0], winfo[1] = j, info[1]
    for k in range(1, 8):
        winfo[1 + k] = int((outcome == k).sum())
    assert int(winfo[1 + abi.RSP_NOSPC]) == len(src) - j
    tb, td, trec = on_device(big, n)
    check_respond(respond(big["rx"], tb, td, trec, n, cap, abi.RSPK_ALL), (outcome, desc[:j], src[:j], replies[:j], winfo), n, cap)


# ---- the learning fold ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hot(big):
    """learn_ref's learning batch of 4,096 frames, classified on the module's handle, with its
    per-frame reference."""
    buf, desc = L.pack(*L.learning_batch(UNIT))
    tb, td, trec, rec = classify(big["rx"], buf, desc)
    outcome, keys = L.learn_keys(buf, desc, rec, abi.LRNK_ALL, big["env6"])
    return dict(buf=buf, desc=desc, rec=rec, outcome=outcome, keys=keys, unit=(tb, td, trec))


def learn_info(outcome, distinct, over=False):
    info = np.zeros(abi.LRN_INFO_WORDS, np.uint64)
    info[0], info[1], info[2] = 0 if over else distinct, distinct, int(over)
    for k in range(1, 6):
        info[2 + k] = int((outcome == k).sum())
    return info


def check_hot_unit(big, hot):
    ev = L.events_array(L.fold(hot["keys"]))
    tb, td, trec = hot["unit"]
    check_learn(learn(big["rx"], tb, td, trec, UNIT, len(ev)), (hot["outcome"], ev, learn_info(hot["outcome"], len(ev))))


@pytest.mark.parametrize("n", SIZES[2:])
def test_learn_hot_keys_past_one_round(big, hot, n):
    """65 and 129 repetitions of the learning batch: count, first and last of every key summed over
    more than 1,024 tiles.  Every key's last frame is in the final repetition, so the emitters sit
    in the last 16 tiles: this batch says nothing about the carry of k_lrn_scan
    (test_learn_emitters_on_both_sides_of_the_round does)."""
    q = n // UNIT
    ev = L.events_array(L.fold(hot["keys"] * q))
    unit_ev = L.events_array(L.fold(hot["keys"]))
    assert len(ev) == len(unit_ev) > 50 and (ev["count"] == q * unit_ev["count"]).all() and (ev["last"] >= n - UNIT).all()
    assert (ev["first"] < UNIT).all()
    outcome = np.tile(hot["outcome"], q)
    desc = np.tile(hot["desc"], q)
    tb, td, trec, _ = classify(big["rx"], hot["buf"], desc)
    check_learn(learn(big["rx"], tb, td, trec, n, len(ev)), (outcome, ev, learn_info(outcome, len(ev))))


SENDERS = 65 * UNIT // 2


def stamped_requests(n, senders):
    """n ARP requests as learn_ref.arp_requests(n, senders) builds them, stamped with numpy from
    its 60-byte frame -> buf, desc (the layout of frames.pack_frames), the keys in closed form."""
    (tmpl,), _ = L.arp_requests(1, 1)
    assert len(tmpl) == 60
    j = np.arange(n) % senders
    b = np.zeros((n, 64), np.uint8)
    b[:, 4:] = np.frombuffer(tmpl, np.uint8)
    for k, sh in enumerate((16, 8, 0)):
        v = ((j >> sh) & 0xFF).astype(np.uint8)
        b[:, 4 + 9 + k] = v    # the Ethernet source
        b[:, 4 + 25 + k] = v   # the sender's hardware address
        b[:, 4 + 29 + k] = v   # the sender's IP
    desc = np.zeros(n, abi.DESC_DTYPE)
    desc["off"], desc["len"], desc["vport"] = 4 + 64 * np.arange(n), 60, 1
    buf = np.concatenate([b.reshape(-1), np.zeros(16, np.uint8)])
    one = [(0, abi.LRN_ARP_REQ, bytes([48, (s >> 16) & 255, (s >> 8) & 255, s & 255]) + bytes(12),
            bytes([0, 0x10, 0x94, (s >> 16) & 255, (s >> 8) & 255, s & 255])) for s in range(senders)]
    return buf, desc, (one * -(-n // senders))[:n]


@pytest.fixture(scope="module")
def spread(big, hot):
    """266,240 requests, every sender twice: first = j, last = j + 133,120, so the emitters fill
    tiles 520 to 1,039, on both sides of the scan's round.  The closed-form keys are held against
    learn_ref.learn_keys on the oracle's records before the batch goes to the device."""
    import pyoracle
    n = SIZES[2]
    buf, desc, keys = stamped_requests(n, SENDERS)
    o = pyoracle.Oracle()
    R.load_tables(o)
    rng = np.random.default_rng(0x1A26E)
    for idx in (np.arange(UNIT), np.arange(n - UNIT, n), np.sort(rng.choice(n, UNIT, replace=False))):
        rec = o.rx_batch(buf, desc[idx])[0]
        outcome, got = L.learn_keys(buf, desc[idx], rec)
        assert (outcome == abi.LRN_ARP_REQ).all() and got == [keys[i] for i in idx]
    fr, _ = L.arp_requests(300, 7)
    fb, fd, _ = stamped_requests(300, 7)
    assert [fb[d["off"]:d["off"] + d["len"]].tobytes() for d in fd] == fr
    events = L.fold(keys)
    assert len(events) == SENDERS and all(e[1:] == (2, s, s + SENDERS) for s, e in enumerate(events))
    assert SENDERS // TILE == 520 and (n - 1) // TILE == 1039  # the emitters' tiles
    tb, td, trec, rec = classify(big["rx"], buf, desc)
    return dict(n=n, dev=(tb, td, trec), ev=L.events_array(events), outcome=np.full(n, abi.LRN_ARP_REQ, np.uint8))


@pytest.mark.parametrize("short", [0, 1], ids=["exact", "one-below"])
def test_learn_emitters_on_both_sides_of_the_round(big, hot, spread, short):
    """ev_cap equal to the distinct count: every event, in ascending last, those of tiles 1,024 to
    1,039 behind the carry of round one; one below: overflow, nothing written, the rest of d_info
    valid.  Then the learning batch on the same handle: the set is empty again."""
    s = spread
    cap = SENDERS - short
    tb, td, trec = s["dev"]
    got = learn(big["rx"], tb, td, trec, s["n"], cap)
    check_learn(got, (s["outcome"], s["ev"][:0] if short else s["ev"], learn_info(s["outcome"], SENDERS, over=bool(short))))
    if short:
        assert (got["ev"] == 0xEE).all()
    check_hot_unit(big, hot)

"""emurx_pingtx_dev through the C-ABI: frames, descriptors, outcomes and info byte for byte against
tests/pingtx_ref.py generate(), which is sendPing's chain request by request; the two ping
simulations' captured echo requests; and the shipment of store edits ahead of the calls that read
them."""
import random
from pathlib import Path

import numpy as np
import pytest

import pingtx_ref as R
import pingtx_util as U
from emurx import abi

pytestmark = pytest.mark.gpu
GOLDEN = Path(__file__).parent / "golden" / "corpus_frames.npz"
MAX_PINGS, MAX_FRAMES = 1024, 640
TS = 0x0123456789ABCDEF


@pytest.fixture(scope="module")
def env(gpu_ok):
    from emurx.rx import RxPath
    rx = RxPath(0, max_ns=16, max_clients=16, max_frames=MAX_FRAMES, max_bytes=1 << 20)
    st = U.Store(rx, MAX_PINGS)
    yield rx, st
    rx.close()


@pytest.fixture(scope="module")
def pool(env):
    """Templates the tests below share: every length residue and every icmp_off residue mod 16,
    seq_t 0 / 0xffff / random, timestamps of their own; ids 0..39, never removed."""
    rx, st = env
    rng = random.Random(5)
    ids = []
    for k in range(40):
        icmp_off = 30 + k % 16 + 4 * (k // 16)
        length = icmp_off + 24 + (k * 11 - icmp_off - 24) % 16 + 16 * (k % 2)  # length % 16 == 11 k % 16
        ids.append(st.add(U.raw_template(rng, length, icmp_off, seq_t=[0, 0xFFFF, None][k % 3],
                                         ts_t=[0, (1 << 64) - 1, None][k % 3]), icmp_off, vport=k))
    assert ids == list(range(40))
    assert {len(st.m[i][0]) % 16 for i in ids} == set(range(16)) and {st.m[i][1] % 16 for i in ids} == set(range(16))
    return ids


def test_the_captured_echo_requests(env):
    rx, st = env
    z = np.load(GOLDEN)
    caps = [U.capture_frames(z, "icmp3.json", (1824, 1826, 1828, 1830, 1832)),
            U.capture_frames(z, "ipv6ping_rpc.json", (6854, 6857, 6860, 6863, 6866))]
    ids = [st.add(t, off, vport=1) for off, t in U.capture_templates()]
    try:
        for i, want in zip(ids, caps):
            assert st.m[i][1] == {70: 42, 86: 62}[len(want[0])]
            got = U.run(rx, st.m, [(i, R.SIM_SEQ + k, 1, R.SIM_TS) for k in range(5)], tag="five of one")
            assert got["frames"] == want
            got = U.run(rx, st.m, [(i, R.SIM_SEQ, 5, R.SIM_TS)], tag="one of five")
            assert got["frames"] == want and (got["desc"]["vport"] == 1).all()
        # both families in one call, interleaved
        got = U.run(rx, st.m, [(ids[k % 2], R.SIM_SEQ + k // 2, 1, R.SIM_TS) for k in range(10)])
        assert got["frames"][0::2] == caps[0] and got["frames"][1::2] == caps[1]
    finally:
        for i in ids:
            st.remove(i)


def test_sequence_wrap_and_timestamp_words(env, pool):
    rx, st = env
    got = U.run(rx, st.m, [(pool[3], 0xFFFE, 4, TS)])
    off = st.m[pool[3]][1]
    assert [R.be16(f, off + 6) for f in got["frames"]] == [0xFFFE, 0xFFFF, 0, 1]
    ts = [0, (1 << 64) - 1, 0xFFFF0000FFFF0000, 0x0000FFFF0000FFFF, 0xFFFF, 0xFFFF << 48, 1]
    U.run(rx, st.m, [(pool[k % 6], 0xFFFF, 2, t) for k, t in enumerate(ts)])


def test_counts(env, pool):
    rx, st = env
    got = U.run(rx, st.m, [(pool[k], 100 * k, c, TS + k) for k, c in enumerate([0, 1, 63, 64, 65, 257, 0])])
    assert got["info"][0] == 1 + 63 + 64 + 65 + 257 and got["outcome"].tolist() == [0] * 7


@pytest.mark.parametrize("n_req", [0, 1, 64, 65, 300])
def test_request_counts(env, pool, n_req):
    """300 requests: two tiles of requests, an output of several workgroups of chunks."""
    rx, st = env
    rng = random.Random(n_req)
    reqs = [(rng.choice(pool), rng.randrange(1 << 16), rng.choice([0, 1, 1, 2, 3]), rng.getrandbits(64)) for _ in range(n_req)]
    got = U.run(rx, st.m, reqs)
    if n_req == 300:
        assert int(got["info"][1]) // 16 > 2 * 1024
    if n_req == 0:
        assert not got["info"].any()


def test_template_lengths(env):
    """icmp_off + 24 (the shortest), 63, 64, 65 and 248, the longest: its last chunk ends the slot."""
    rx, st = env
    rng = random.Random(9)
    shapes = [(30 + 24, 30), (63, 34), (64, 40), (65, 41), (248, 224), (248, 42), (24, 0)]
    ids = [st.add(U.raw_template(rng, ln, off), off, vport=200 + k) for k, (ln, off) in enumerate(shapes)]
    try:
        U.run(rx, st.m, [(i, 0xFFFD, 5, TS) for i in ids] + [(i, 7, 1, 0) for i in reversed(ids)])
    finally:
        for i in ids:
            st.remove(i)


def test_patched_fields_across_chunk_edges(env, pool):
    """icmp_off alone decides where the fields fall in the 16-byte output chunks: the seq field
    ending a chunk ((icmp_off + 6) % 16 == 14), split over two (== 15), the timestamp split at every
    byte ((icmp_off + 16) % 16 in 9..15), the checksum split (icmp_off % 16 == 13)."""
    rx, st = env
    by_res = {}
    for i in pool:
        by_res.setdefault(st.m[i][1] % 16, i)
    assert {(8 + 6) % 16, (9 + 6) % 16} == {14, 15} and set(by_res) == set(range(16))
    U.run(rx, st.m, [(by_res[r], 0xA1B2 + r, 3, 0x1122334455667788 + r) for r in range(16)])


def test_bad_ids_among_good_ones(env, pool):
    rx, st = env
    rng = random.Random(2)
    gone = st.add(U.raw_template(rng, 80, 34), 34)
    st.remove(gone)
    reqs = [(pool[0], 1, 2, TS), (gone, 1, 2, TS), (pool[1], 1, 2, TS), (MAX_PINGS, 1, 2, TS), (0xFFFFFFFF, 1, 65535, TS),
            (pool[2], 1, 2, TS), (MAX_PINGS - 1, 0, 0, 0), (pool[3], 9, 1, 3)]
    got = U.run(rx, st.m, reqs)
    assert got["outcome"].tolist() == [0, 1, 0, 1, 1, 0, 1, 0] and got["info"].tolist()[:6] == [7, got["info"][1], 7, 4, 4, 0]


def test_600_templates_interleaved(env, pool):
    rx, st = env
    rng = random.Random(600)
    ids = []
    for k in range(600):
        off = 34 + rng.randrange(12)
        ids.append(st.add(U.raw_template(rng, off + 24 + rng.randrange(40), off), off, vport=k % 256))
    try:
        assert len(set(ids)) == 600
        order = ids[:]
        rng.shuffle(order)
        # one call over all 600, each template twice, the second round in another order
        reqs = [(i, rng.randrange(1 << 16), 1 + (k % 3 == 0), rng.getrandbits(64)) for k, i in enumerate(order)]
        U.run(rx, st.m, reqs, tag="600 templates")
        rng.shuffle(order)
        U.run(rx, st.m, [(i, 5, 1, 6) for i in order] + reqs[:40], tag="again, with repeats")
    finally:
        for i in ids:
            st.remove(i)


@pytest.mark.parametrize("short", ["bytes", "desc", "both", "first"])
def test_too_little_room_gives_a_prefix(env, pool, short):
    rx, st = env
    reqs = [(pool[k % len(pool)], k, 1 + k % 4, TS) for k in range(70)] + [(MAX_PINGS, 0, 3, 0), (pool[0], 0, 0, 0)]
    full = R.generate(st.m, reqs, U.HUGE, U.HUGE)
    cut = 0 if short == "first" else 41  # the first request that does not fit: one short of its end
    nf = sum(r[2] for r in reqs[:cut + 1])
    end = int(full[1]["off"][nf - 1]) + R.align16(int(full[1]["len"][nf - 1]))
    caps = {"bytes": (end - 1, nf + 100), "desc": (end + 1000, nf - 1), "both": (end - 1, nf - 1), "first": (end - 1, nf)}[short]
    got = U.run(rx, st.m, reqs, *caps)
    assert got["outcome"].tolist() == [0] * cut + [2] * (70 - cut) + [1, 0]
    assert got["info"].tolist() == [nf - reqs[cut][2], int(full[3][1]), int(full[3][2]), cut + 1, 1, 70 - cut, 0, 0]
    # nothing at all fits
    got = U.run(rx, st.m, reqs, 0, 0)
    assert got["info"][0] == 0 and got["outcome"].tolist() == [2] * 70 + [1, 0]


def test_an_add_between_two_calls_is_seen_by_the_second(env, pool):
    rx, st = env
    rng = random.Random(4)
    t1, t2 = U.raw_template(rng, 90, 42), U.raw_template(rng, 75, 37)
    a = st.add(t1, 42, 3)
    U.run(rx, st.m, [(a, 1, 3, TS), (a + 1, 1, 3, TS)])      # a + 1 is still free
    b = st.add(t2, 37, 4)
    assert b == a + 1
    U.run(rx, st.m, [(a, 1, 3, TS), (b, 1, 3, TS)])
    st.remove(a)                                                 # and a remove, and the id's next template
    U.run(rx, st.m, [(a, 1, 3, TS), (b, 1, 3, TS)])
    assert st.add(t2, 37, 9) == a
    U.run(rx, st.m, [(a, 1, 3, TS), (b, 1, 3, TS)])
    st.remove(a)
    st.remove(b)


def test_two_streams_after_one_edit(env, pool):
    """The edit is shipped on the first call's stream; the second stream waits for it by event.
    No host synchronisation between the two calls."""
    import torch
    rx, st = env
    rng = random.Random(8)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    ids = [st.add(U.raw_template(rng, 100 + k, 40 + k), 40 + k, k) for k in range(8)]
    try:
        reqs = [(i, 0xFFF0, 40, TS) for i in ids]
        c1 = U.Call(rx, st.m, reqs, tag="stream 1")
        c2 = U.Call(rx, st.m, list(reversed(reqs)), tag="stream 2")
        torch.cuda.synchronize()  # the buffers' fills; nothing between the two launches
        c1.launch(s1)
        c2.launch(s2)
        c1.finish()
        c2.finish()
    finally:
        for i in ids:
            st.remove(i)

"""The send side of ping on the CPU (tests/pingtx_ref.py): the two templates and sendPing's chain
against the echo requests the reference's own ping simulations sent, the closed form of the
checksum against the chain and the full recompute, and the batch semantics against the chain
applied request by request."""
import random
import struct
from pathlib import Path

import numpy as np
import pytest

import pingtx_ref as R
import sim_envs

GOLDEN = Path(__file__).parent / "golden" / "corpus_frames.npz"
NS_VLANS = struct.unpack_from("<II", sim_envs.NS_KEY, 4)
TS_EDGE = [0, (1 << 64) - 1, 0xFFFF0000FFFF0000, 0x0000FFFF0000FFFF]

# (capture, its tx frames that are echo requests, the template of the capture's Ping)
CAPTURES = [
    # icmp_test.go:133 icmp3: dst 16.0.0.1, payloadSize 20, no gateway MAC resolved
    ("icmp3.json", (1824, 1826, 1828, 1830, 1832), 42,
     lambda: R.template4(sim_envs.ENVS["icmp"]["mac"], NS_VLANS, sim_envs.ENVS["icmp"]["ipv4"], bytes([16, 0, 0, 1]),
                         R.SIM_IDENT, R.SIM_SEQ, payload_size=20)),
    # ipv6ping_rpc: 2001:db8::2 -> 2001:db8::1, the default payload of 16
    ("ipv6ping_rpc.json", (6854, 6857, 6860, 6863, 6866), 62,
     lambda: R.template6(sim_envs.ENVS["ipv6"]["mac"], NS_VLANS, sim_envs.ENVS["ipv6"]["ipv6"],
                         sim_envs.ENVS["ipv6"]["ipv6"][:15] + b"\x01", R.SIM_IDENT, R.SIM_SEQ)),
]


def captured(z, capture, ids):
    files = [str(x) for x in z["files"]]
    for i in ids:
        assert z["src"][i] == files.index(capture) and z["meta"][i] == 0  # a tx frame of that capture
    return [z["data"][z["off"][i]:z["off"][i] + z["len"][i]].tobytes() for i in ids]


def full_recompute(frame, icmp_off, v6):
    """The checksum PreparePingPacketTemplate would give the patched frame."""
    f = bytearray(frame)
    f[icmp_off + 2:icmp_off + 4] = b"\0\0"
    if not v6:
        return R.tcpip_checksum(f[icmp_off:])
    l3 = icmp_off - 40
    ph = R.tcpip_checksum(f[l3 + 8:l3 + 40] + struct.pack(">II", len(f) - icmp_off, 58))
    return R.tcpip_checksum(f[icmp_off:], ~ph & 0xFFFF)


@pytest.mark.parametrize("capture,ids,off,make", CAPTURES, ids=[c[0] for c in CAPTURES])
def test_templates_and_chain_reproduce_the_captures(capture, ids, off, make):
    want = captured(np.load(GOLDEN), capture, ids)
    icmp_off, tmpl = make()
    assert icmp_off == off and len(tmpl) == len(want[0])
    # the template is the first captured frame with a zero timestamp and its checksum recomputed
    assert struct.unpack_from(">Q", tmpl, icmp_off + 16)[0] == 0
    frames, live = R.send(tmpl, icmp_off, R.SIM_SEQ, 5, R.SIM_TS)
    assert frames == want
    assert bytes(live) == want[-1]
    # five calls of one frame each, as the simulation's timer made them, leave the same frames
    live, out = tmpl, []
    for k in range(5):
        f, live = R.send(live, icmp_off, R.SIM_SEQ + k, 1, R.SIM_TS)
        out += f
    assert out == want
    assert [R.patch(tmpl, icmp_off, R.SIM_SEQ + k, R.SIM_TS) for k in range(5)] == want


def random_template(rng, length=None, seq_t=None, v6=None):
    """A template of either family with random addresses; length: the frame's, if given."""
    v6 = rng.random() < 0.5 if v6 is None else v6
    tags = rng.choice([(0, 0), (0x81000005, 0), (0x81000001, 0x81000002)])
    mac = bytes(rng.randrange(256) for _ in range(6))
    seq_t = rng.randrange(1 << 16) if seq_t is None else seq_t
    head = 14 + 4 * sum(1 for t in tags if t) + (40 if v6 else 20) + 8
    size = rng.randrange(16, 64) if length is None else length - head
    assert size >= 16
    mk, alen = (R.template6, 16) if v6 else (R.template4, 4)
    src, dst = (bytes(rng.randrange(256) for _ in range(alen)) for _ in range(2))
    icmp_off, pkt = mk(mac, tags, src, dst, rng.randrange(1 << 16), seq_t, payload_size=size)
    # a payload that is not all zero behind the magic, the template's own timestamp field included
    if rng.random() < 0.5:
        for i in range(icmp_off + 16, len(pkt)):
            pkt[i] = rng.randrange(256)
        struct.pack_into(">H", pkt, icmp_off + 2, full_recompute(pkt, icmp_off, v6))
    return icmp_off, pkt, v6


def test_closed_form_is_the_chain_is_the_full_recompute():
    rng = random.Random(7)
    frames = 0
    for t in range(300):
        icmp_off, tmpl, v6 = random_template(rng, seq_t=[0, 0xFFFF, None][t % 3])
        if R.be16(tmpl, icmp_off + 2) == 0xFFFF:
            continue  # emurx_pingtx_add refuses it: the chain is path dependent there
        live = tmpl
        for call in range(4):  # the live packet goes on from call to call, as Ping's does
            seq = rng.choice([0xFFFE, 0, rng.randrange(1 << 16)])
            ts = rng.choice(TS_EDGE + [rng.getrandbits(64)])
            count = rng.randrange(1, 6)
            out, live = R.send(live, icmp_off, seq, count, ts)
            for k, f in enumerate(out):
                s = (seq + k) & 0xFFFF
                cs = R.closed_form(tmpl, icmp_off, s, ts)
                assert R.be16(f, icmp_off + 2) == cs == full_recompute(f, icmp_off, v6), (t, call, k)
                assert f == R.patch(tmpl, icmp_off, s, ts)
                frames += 1
    assert frames > 2000


def fuzz_store(rng, n=48):
    store = {}
    for i in range(n):
        # every length residue mod 16 (the lengths 96..111 and then random ones)
        icmp_off, tmpl, _ = random_template(rng, length=96 + i if i < 16 else None, seq_t=[0, 0xFFFF, None][i % 3])
        if R.be16(tmpl, icmp_off + 2) != 0xFFFF:
            store[2 * i] = (bytes(tmpl), icmp_off, rng.randrange(256))  # odd ids stay free
    return store


def by_request(store, reqs):
    frames, desc, off = [], [], 0
    for rid, seq, count, ts in reqs:
        if rid not in store:
            continue
        tmpl, icmp_off, vport = store[rid]
        for f in R.send(tmpl, icmp_off, seq, count, ts)[0]:
            frames.append(f)
            desc.append((off, len(f), vport, 0))
            off += R.align16(len(f))
    return frames, np.array(desc, R.DESC_DTYPE), off


def test_generate_is_send_request_by_request():
    rng = random.Random(11)
    store = fuzz_store(rng)
    assert {len(v[0]) % 16 for v in store.values()} == set(range(16))
    reqs = []
    for _ in range(400):
        rid = rng.choice(list(store) + [1, 3, 4096])
        seq = rng.choice([0xFFFE, 0xFFFF, 0, rng.randrange(1 << 16)])
        reqs.append((rid, seq, rng.choice([0, 1, 2, 5, 70]), rng.choice(TS_EDGE + [rng.getrandbits(64)])))
    want_f, want_d, total = by_request(store, reqs)
    frames, desc, outcome, info = R.generate(store, reqs, 1 << 40, 1 << 30)
    assert frames == want_f and desc.tobytes() == want_d.tobytes()
    assert list(outcome) == [R.PTX_OK if r[0] in store else R.PTX_BAD_ID for r in reqs]
    bad = sum(1 for r in reqs if r[0] not in store)
    assert list(info) == [len(want_f), total, len(want_f), len(reqs) - bad, bad, 0, 0, 0]
    # bursts across the wrap: the frames behind seq 0xfffe carry 0xffff, 0, 1
    tmpl, icmp_off, _ = store[0]
    f = R.generate(store, [(0, 0xFFFE, 4, 5)], 1 << 20, 100)[0]
    assert [R.be16(x, icmp_off + 6) for x in f] == [0xFFFE, 0xFFFF, 0, 1]


@pytest.mark.parametrize("short", ["bytes", "desc"])
def test_generate_writes_a_prefix_of_whole_requests(short):
    rng = random.Random(13)
    store = fuzz_store(rng)
    ids = list(store)
    reqs = [(ids[i % len(ids)], i, 1 + i % 4, i) for i in range(40)] + [(1, 0, 3, 0), (ids[0], 0, 0, 0)]
    all_f, all_d, outcome, info = R.generate(store, reqs, 1 << 40, 1 << 30)
    cut = 25  # request 25 is the first that does not fit: one byte / one descriptor short of its end
    n_before = sum(r[2] for r in reqs[:cut])
    end = int(all_d["off"][n_before + reqs[cut][2] - 1]) + R.align16(int(all_d["len"][n_before + reqs[cut][2] - 1]))
    caps = (end - 1, 1 << 30) if short == "bytes" else (1 << 40, n_before + reqs[cut][2] - 1)
    f, d, o, i2 = R.generate(store, reqs, *caps)
    assert f == all_f[:n_before] and d.tobytes() == all_d[:n_before].tobytes()
    assert list(o[:cut]) == [R.PTX_OK] * cut and list(o[cut:40]) == [R.PTX_NOSPC] * (40 - cut)
    assert list(o[40:]) == [R.PTX_BAD_ID, R.PTX_OK]  # a free id and an empty request need no room
    assert list(i2) == [n_before, int(info[1]), int(info[2]), cut + 1, 1, 40 - cut, 0, 0]

"""The fixed per-wave work of k_rx around the uniform-wave path (csrc/emurx_kernels.hip): the
wave's byte range read off its end lanes when the descriptors are dense, the tight slab's park
through LDS and the checksum verdicts of parse_uniform without byte swaps, and the tail (queue
ranks, counts, histogram bytes) of waves that took the uniform-wave path.  Every batch is checked
bit-exact against the CPU oracle (records, queues, tile counts, counters) on all three slabs; the
second witness (emurx_last_trim: RANGE per wave of tile 0) tells the range shortcut from its
fall-back.  The cases are the smallest shapes at which each shortcut can go wrong.
"""
import struct

import numpy as np
import pytest

import edge_frames as E
from emurx import abi
from emurx import frames as F
from emurx import synth
from gpu_util import frame_tuples, rec_diff, run_dev
from test_gpu_uniform_waves import (CM, DIP, SIP, _l2, batch, check, pair_b, pair_frames, plain256, tcpf, tile0,
                                    udpf)

pytestmark = pytest.mark.gpu
S, P, L = abi.UNI_SAMPLED, abi.UNI_PARSE, abi.UNI_LOOKUP
R = abi.TRIM_RANGE
FULL = S | R
SLABS = {"tight": 5120, "narrow": 6144, "wide": 7168}


@pytest.fixture(scope="module")
def rxmod(gpu_ok, oracle_built):
    from emurx.rx import RxPath
    return RxPath


@pytest.fixture(params=list(SLABS))
def stage(request, monkeypatch):
    monkeypatch.setenv("EMURX_STAGE", request.param)  # read by emurx_open
    return request.param


def trim0(rx):
    """The second witness words of tile 0's four waves."""
    return [int(x) for x in rx.last_trim()[:4]]


# ---- the range from the end lanes ---------------------------------------------------------------
def test_range_dense(rxmod, stage):
    w, _ = plain256()
    rx, o = pair_b(rxmod, w)
    check(rx, o, w["buf"], w["desc"])
    assert rx.last_stage() == SLABS[stage]
    assert trim0(rx) == [FULL] * 4 and tile0(rx) == [S | P | L] * 4


def test_range_swapped_pair(rxmod, stage):
    """Two descriptors of wave 1 swapped: that wave alone reduces; its lookups stay uniform."""
    w, _ = plain256()
    desc = w["desc"].copy()
    desc[[64 + 10, 64 + 11]] = desc[[64 + 11, 64 + 10]]
    rx, o = pair_b(rxmod, w)
    check(rx, o, w["buf"], desc)
    assert trim0(rx) == [FULL, S, FULL, FULL]


@pytest.mark.parametrize("lane", [0, 63, 31])
def test_range_hole(rxmod, stage, lane):
    w, frames = plain256()
    rx, o = pair_b(rxmod, w)
    check(rx, o, *batch(frames, holes=[128 + lane]))
    assert trim0(rx) == [FULL, FULL, S, FULL]


def test_range_aliased_descriptors(rxmod, stage):
    """Two descriptors naming one frame.  Next to each other neither the offsets nor the ends
    fall, and lane 0 / lane 63 still bound the range: the shortcut holds.  Apart, the second one
    steps back: the reductions."""
    w, _ = plain256()
    desc = w["desc"].copy()
    desc[70] = desc[69]
    desc[192 + 40] = desc[192 + 3]
    rx, o = pair_b(rxmod, w)
    check(rx, o, w["buf"], desc)
    assert trim0(rx) == [FULL, FULL, FULL, S]
    desc[0] = desc[63]  # lane 0 no longer holds the least offset
    check(rx, o, w["buf"], desc)
    assert trim0(rx) == [S, FULL, FULL, S]


def test_range_end_not_monotone(rxmod, stage):
    """Increasing offsets, but a long frame's descriptor is followed by a short frame that lies
    inside it: lane 63's end is still the greatest, the rule does not hold, the wave reduces.  In
    wave 1 the long frame is the last descriptor but one, so lane 63 does not hold the greatest
    end at all."""
    _, frames = plain256()
    inner = udpf(sp=77)
    for at in (20, 64 + 62):
        frames[at] = udpf(payload=bytes(10) + inner + bytes(30))
    buf, desc = batch(frames)
    for at in (20, 64 + 62):
        desc[at + 1]["off"], desc[at + 1]["len"] = int(desc[at]["off"]) + 42 + 10, len(inner)
    assert desc[64 + 63]["off"] + desc[64 + 63]["len"] < desc[64 + 62]["off"] + desc[64 + 62]["len"]
    rx, o = pair_b(rxmod, plain256()[0])
    rec = check(rx, o, buf, desc)
    assert (rec["status"] == 0).all()
    assert [x & R for x in trim0(rx)] == [0, 0, R, R]


@pytest.mark.parametrize("n", [1, 63, 65, 255, 257])
def test_range_ragged_batches(rxmod, stage, n):
    """A partial last wave and a partial last tile: the wave with empty slots reduces."""
    w = synth.config_b(n)
    rx, o = pair_b(rxmod, w)
    check(rx, o, w["buf"], w["desc"])
    assert trim0(rx) == [FULL if n >= 64 * (k + 1) else S for k in range(4)]
    check(rx, o, w["buf"], w["desc"], classify=False)
    assert trim0(rx) == [S | R if n >= 64 * (k + 1) else S for k in range(4)]


def test_range_wider_than_the_slab(rxmod, stage):
    """Wave 0: 64 frames of 100 bytes, a monotone range of 6.5 KiB.  It fits the wide slab only;
    on the others the shortcut hands the window path the same vector count the reductions do
    (wave 1: the same frames with two descriptors swapped)."""
    _, plain = plain256()
    big = [udpf(sp=2000 + i, payload=bytes((i + k) & 0xFF for k in range(58))) for i in range(64)]
    buf, desc = batch(big + big + plain[:128])
    desc[[64 + 5, 64 + 6]] = desc[[64 + 6, 64 + 5]]
    rx, o = pair_b(rxmod, plain256()[0])
    check(rx, o, buf, desc)
    staged = S | P | L if stage == "wide" else S
    assert tile0(rx) == [staged, staged, S | P | L, S | P | L]
    assert [x & R for x in trim0(rx)] == [R, 0, R, R]


@pytest.mark.parametrize("extra", [0, 1])
def test_range_tight_boundary(rxmod, stage, extra):
    """Wave 0's range is 320 vectors (the whole tight slab) or 321 (the window path there)."""
    _, plain = plain256()
    first = [udpf(sp=3000 + i, payload=bytes(34 + (extra if i == 63 else 0))) for i in range(64)]
    buf, desc = batch(first + plain[:192])
    assert int(desc[0]["off"]) == 4 and int(desc[63]["off"]) + int(desc[63]["len"]) == 5120 + extra
    rx, o = pair_b(rxmod, plain256()[0])
    check(rx, o, buf, desc)
    assert trim0(rx) == [FULL if not (stage == "tight" and extra) else S | R] + [FULL] * 3
    assert tile0(rx)[0] == (S if stage == "tight" and extra else S | P | L)


# ---- the park of the tight slab: general lookups with non-trivial parked fields -------------------
ODD_MAC = bytes([2, 0, 0, 0, 9, 9])  # no client: the wave leaves the uniform lookups


def _park_waves():
    """name -> wave 0's 64 frames (the lane that sends the wave to the general lookups is 9)."""
    tag = ((F.ETH_DOT1Q, 7),)
    opt = bytes([1, 1, 1, 0])
    out = {
        "tcp_options": [tcpf(bytes(range(i % 13)), doff=6, options=opt, dmac=ODD_MAC if i == 9 else CM) for i in range(64)],
        "tagged": [udpf(sp=100 + i, tags=tag, dmac=ODD_MAC if i == 9 else CM) for i in range(64)],
        "rtalert": [udpf(sp=100 + i) for i in range(64)],
        "bad_status": [udpf(sp=100 + i, csum=0x1357 if i in (9, 40) else "auto") for i in range(64)],
    }
    out["rtalert"][9] = E.udp6(9, 10, exts=F.ipv6_ext(17, bytes([5, 2, 0, 0, 1, 0])), ext_nh=0)
    return out


@pytest.mark.parametrize("name", list(_park_waves()))
def test_park_general_lookups(rxmod, stage, name):
    frames = _park_waves()[name] + plain256()[1][:192]
    rx, o = pair_frames(rxmod, [f for f in frames if f[:6] != ODD_MAC])  # no client for lane 9's MAC
    rec = check(rx, o, *batch(frames))
    assert not tile0(rx)[0] & L
    if name == "tcp_options":
        assert (rec["l7"][:64] == rec["l4"][:64] + 24).all() and rec["l7_len"][12] == 12
    if name == "tagged":
        assert (rec["vlan0"][:64] != 0).all()
    if name == "rtalert":
        assert rec["flags"][9] & abi.FLAG_RTALERT
    if name == "bad_status":
        assert rec["status"][9] == abi.ST["UDP_CS"] and rec["status"][10] == 0


def test_park_flow_probe(rxmod, stage):
    """Flows on: the clients have a TransportCtx, so every wave runs the general lookups and the
    flow probe reads the tuple through the parked words."""
    macs = [CM] + [bytes([2, 0, 0, 0, 1, k]) for k in range(3)]  # frames_tables: client 0 has no transport plugin
    frames = [udpf(sp=4000 + i, dmac=macs[i % 4]) if i % 3 else tcpf(bytes(i % 11), dmac=macs[i % 4]) for i in range(256)]
    rx, o = pair_frames(rxmod, frames)
    buf, desc = batch(frames)
    orec = o.rx_batch(buf, desc)[0]
    tup = frame_tuples(buf, desc, orec)
    for c in np.unique(orec["client_id"]):
        assert rx.client_set_transport(int(c), 1) == o.client_set_transport(int(c), 1) == 0
    for i in range(0, 256, 3):
        if tup[i] is not None:
            cid = int(orec[i]["client_id"])
            assert rx.flow_add(cid, tup[i], i) == o.flow_add(cid, tup[i], i)
    rec, _, _, _, flow = run_dev(rx, buf, desc, flows=True)
    orec = o.rx_batch(buf, desc)[0]
    assert rec.tobytes() == orec.tobytes(), rec_diff(rec, orec)
    want = o.flows(buf, desc, orec)
    assert np.array_equal(flow, want) and (want <= abi.FLOW_ID_MAX).sum() > 20
    assert not any(x & L for x in tile0(rx))
    check(rx, o, buf, desc)


# ---- the checksum verdicts of parse_uniform ---------------------------------------------------
def _ip_frame(proto, l4, tags, **kw):
    return _l2(CM, tags, F.ipv4(SIP, DIP, proto, l4, **kw))


def _csum_variants(proto, tags):
    """The odd lanes, one to a wave: (name, frame).  Every base frame is 64 bytes + 4 per tag, so
    a buffer of them keeps the alignment of its first frame."""
    if proto == "udp":
        pay = bytes(range(22))
        ps = F.ipv4_pseudo(F.ip4(SIP), F.ip4(DIP), 17, 8 + len(pay))
        l4 = F.udp(1234, 5000, pay, csum="auto", pseudo=ps)
        bad = F.udp(1234, 5000, pay, csum=0x2468)
        pid, base = 17, udpf(tags=tags)
    else:
        pay = b"hello tcp!"
        ps = F.ipv4_pseudo(F.ip4(SIP), F.ip4(DIP), 6, 20 + len(pay))
        l4 = F.tcp(1000, 80, pay, csum="auto", pseudo=ps)
        bad = F.tcp(1000, 80, pay, csum=0x2468)
        pid, base = 6, tcpf(tags=tags)
    assert _ip_frame(pid, l4, tags) == base and len(base) == 64 + 4 * len(tags)
    # the identification that makes the header's checksum field 0: the other words sum to 0xffff
    hdr0 = F.ipv4(SIP, DIP, pid, l4)[:20]
    ident = struct.unpack(">H", hdr0[10:12])[0]
    zero_cs = F.ipv4(SIP, DIP, pid, l4, ident=ident)
    assert zero_cs[10:12] == b"\x00\x00"
    v = [("base", base),
         ("bad_ip_cs", _ip_frame(pid, l4, tags, csum=0x1234)),
         ("ip_cs_zero", _l2(CM, tags, zero_cs)),                              # the sum is 0xffff, the field 0
         ("ip_cs_ffff", _ip_frame(pid, l4, tags, ident=ident, csum=0xFFFF)),  # the same header, the field -0
         ("bad_l4_cs", _ip_frame(pid, bad, tags))]
    if proto == "udp":
        odd, even = udpf(payload=bytes(range(23)), tags=tags), udpf(payload=bytes(range(24)), tags=tags)
        # a datagram whose checksum computes to 0: sent as 0xffff it verifies, sent as 0 it is "absent"
        body = bytearray(22)
        c0 = struct.unpack(">H", F.udp(1234, 5000, bytes(body), csum="auto", pseudo=ps)[6:8])[0]
        body[20:22] = struct.pack(">H", c0)
        assert F.udp(1234, 5000, bytes(body), csum="auto", pseudo=ps)[6:8] in (b"\x00\x00", b"\xff\xff")
        v += [("udp_cs_absent", udpf(csum=0, tags=tags)),
              ("udp_cs_ffff_wrong", udpf(csum=0xFFFF, tags=tags)),
              ("udp_cs_ffff_right", _ip_frame(17, F.udp(1234, 5000, bytes(body), csum=0xFFFF), tags)),
              ("udp_cs_zero_sum_absent", _ip_frame(17, F.udp(1234, 5000, bytes(body), csum=0), tags))]
    else:
        odd, even = tcpf(b"hello tcp!!", tags=tags), tcpf(b"hello tcp!!!", tags=tags)
    # an all-zero L4 span under a zero pseudo sum (csum_ok's T == 0 && pcs == 0) cannot be framed:
    # the IPv4 pseudo header holds the protocol, 6 or 17
    return v + [("odd_l4_len", odd), ("even_l4_len", even)]


@pytest.mark.parametrize("uniform", ["1", "0"])
@pytest.mark.parametrize("proto", ["udp", "tcp"])
@pytest.mark.parametrize("ntags", [0, 1, 2])
def test_checksum_verdicts(rxmod, monkeypatch, stage, ntags, proto, uniform):
    monkeypatch.setenv("EMURX_UNIFORM", uniform)
    tags = (((F.ETH_QINQ, 5), (F.ETH_DOT1Q, 6)), ((F.ETH_DOT1Q, 7),), ())[2 - ntags]
    variants = _csum_variants(proto, tags)
    frames = []
    for k, (_, f) in enumerate(variants):  # a wave per variant, at a lane that moves with it
        wave = [variants[0][1]] * 64
        wave[(11 * k + 3) % 64] = f
        frames += wave
    assert len(frames) <= 1024
    rx, o = pair_frames(rxmod, frames)
    buf, desc = batch(frames)
    for shift in range(4):  # off mod 4 of every base frame
        b2, d2 = np.concatenate([np.zeros(shift, np.uint8), buf]), desc.copy()
        d2["off"] += shift
        assert int(d2[0]["off"]) % 4 == shift
        rec = check(rx, o, b2, d2)
        st = {name: int(rec["status"][64 * k + (11 * k + 3) % 64]) for k, (name, _) in enumerate(variants)}
        assert st["bad_ip_cs"] == abi.ST["IPV4_CS"] and st["ip_cs_zero"] == st["ip_cs_ffff"] == 0
        assert st["bad_l4_cs"] == abi.ST["UDP_CS" if proto == "udp" else "TCP_CS"]
        assert st["odd_l4_len"] == st["even_l4_len"] == 0
        if proto == "udp":
            assert st["udp_cs_absent"] == st["udp_cs_ffff_right"] == st["udp_cs_zero_sum_absent"] == 0
            assert st["udp_cs_ffff_wrong"] == abi.ST["UDP_CS"]
        assert [x & P for x in tile0(rx)] == [P * int(uniform)] * 4
        check(rx, o, b2, d2, classify=False)


# ---- the tail of uniform waves ------------------------------------------------------------------
def _tail_lanes():
    """name -> (frame, vport) of the one lane that takes wave 2 off the uniform lookups."""
    return {"mdns": (udpf(dp=5353), 0), "bad_udp_cs": (udpf(csum=0xABCD), 0), "unknown_client": (udpf(dmac=ODD_MAC), 0),
            "unknown_ns": (udpf(), 5)}


@pytest.mark.parametrize("name", list(_tail_lanes()))
def test_tail_one_lane_off(rxmod, stage, name):
    w, frames = plain256()
    vports = [0] * 256
    frames[128 + 17], vports[128 + 17] = _tail_lanes()[name]
    rx, o = pair_b(rxmod, w)
    check(rx, o, *batch(frames, vports))
    assert trim0(rx) == [FULL, FULL, S | R, FULL]
    assert tile0(rx)[2] == S | P


def _udp_tcp_tile():
    """Waves 0 and 2 udp, 1 and 3 tcp (64 bytes each): two queues whose ranks cross the waves; wave
    3's frames differ in length."""
    u = [udpf(sp=5000 + i) for i in range(64)]
    t = [tcpf(bytes(10)) for _ in range(64)]
    return u + t + u + [tcpf(bytes(3 + i % 9)) for i in range(64)]


def _bin_bytes(rec, desc):
    """Bytes per histogram bin (EMURX_HIST_BIN) from the records."""
    want = np.zeros(abi.HIST_BINS, np.uint64)
    for r, d in zip(rec, desc):
        s, p = int(r["status"]), int(r["proto"])
        want[s * abi.NUM_CB + p if s <= abi.ST["NOT_SUPPORTED"] else 2 * abi.NUM_CB + s - 2] += int(d["len"])
    return want


def test_tail_two_queues_and_lengths(rxmod, stage):
    frames = _udp_tcp_tile()
    rx, o = pair_frames(rxmod, frames)
    buf, desc = batch(frames)
    rec = check(rx, o, buf, desc)
    assert trim0(rx) == [FULL] * 4 and tile0(rx) == [S | P | L] * 4
    assert (rec["proto"][64:128] == abi.CB_TCP).all() and (rec["proto"][:64] == abi.CB_UDP).all()
    # the bytes of wave 3 are summed per lane, not 64 x the first lane's length
    hist = run_dev(rx, buf, desc)[3]
    assert np.array_equal(hist[1::2], _bin_bytes(rec, desc))
    assert len(set(desc["len"][192:])) > 1


def test_tail_switch_off(rxmod, monkeypatch, stage):
    monkeypatch.setenv("EMURX_UNIFORM", "0")
    frames = _udp_tcp_tile()
    rx, o = pair_frames(rxmod, frames)
    check(rx, o, *batch(frames))
    assert trim0(rx) == [S | R] * 4 and tile0(rx) == [S] * 4


def test_tail_kind0(rxmod, stage):
    """The parse alone (kind 0)."""
    frames = _udp_tcp_tile()
    rx, o = pair_frames(rxmod, frames)
    check(rx, o, *batch(frames), classify=False)
    assert trim0(rx) == [S | R] * 4 and tile0(rx) == [S | P] * 4
    w, plain = plain256()
    rx, o = pair_b(rxmod, w)
    for name, (f, vp) in _tail_lanes().items():
        fr, vports = list(plain), [0] * 256
        fr[128 + 17], vports[128 + 17] = f, vp
        check(rx, o, *batch(fr, vports), classify=False)
        assert trim0(rx) == [S | R] * 4, name


def test_tail_kind2_two_owners(rxmod, stage):
    """The same batches through parse_route_dev at 2 owners (k_rx kind 2) and lookup_dev."""
    from test_gpu_tables import partitioned_vs_oracle
    w, plain = plain256()
    made = []

    def factory(*a, **k):
        made.append(rxmod(*a, **k))
        return made[-1]

    todo = [(plain, [0] * 256)]
    for f, vp in _tail_lanes().values():
        fr, vports = list(plain), [0] * 256
        fr[128 + 17], vports[128 + 17] = f, vp
        todo.append((fr, vports))
    for fr, vports in todo:
        del made[:]
        buf, desc = batch(fr, vports)
        partitioned_vs_oracle(factory, [dict(buf=buf, desc=desc), dict(buf=w["buf"], desc=w["desc"])],
                              lambda t: synth.load_tables(w, t), 2)
        assert [x & R for x in trim0(made[1])] == [R] * 4
        for h in made:
            h.close()

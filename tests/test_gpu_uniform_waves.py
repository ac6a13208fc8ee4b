"""The uniform-wave path of k_rx (csrc/emurx_parse.h uniform_shape / parse_uniform /
classify_uniform): a staged wave whose 64 frames share one plain shape is parsed, and where its
home slots hit looked up, by straight-line code; any other wave runs the general code.  Every
batch here is checked bit-exact against the CPU oracle (records, queues, counters), and the
witness (emurx_last_uniform: one word per wave of every 64th tile) says which path the waves of
tile 0 took, so that a fall-back that should happen and a wave that should stay are both seen.
"""
import numpy as np
import pytest

import edge_frames as E
from emurx import abi
from emurx import frames as F
from emurx import synth
from gpu_util import frames_tables, load_frame_tables, rec_diff, run_dev
from test_gpu_parity import _hole_rec, check_batch, new_pair

pytestmark = pytest.mark.gpu
S, P, L = abi.UNI_SAMPLED, abi.UNI_PARSE, abi.UNI_LOOKUP
ALL = S | P | L

# config B's one Namespace and client (synth.config_b)
CM, SM = bytes([2, 0, 0, 0, 0, 0]), bytes([0, 0x11, 0x22, 0x33, 0x44, 0x55])
SIP, DIP = "16.0.1.2", "10.0.0.1"


@pytest.fixture(scope="module")
def rxmod(gpu_ok, oracle_built):
    from emurx.rx import RxPath
    return RxPath


# ---- frames ---------------------------------------------------------------------------------
def _l2(dmac, tags, ip):
    """Ethernet with 802.1Q / QinQ tags [(tpid, vid), ...] around an IPv4 packet, unpadded."""
    et = [t for t, _ in tags] + [F.ETH_IPV4]
    body = b"".join(F.dot1q(vid, et[k + 1]) for k, (_, vid) in enumerate(tags)) + ip
    return F.ethernet(dmac, SM, et[0], body, pad=False)


def udpf(sp=1234, dp=5000, payload=bytes(range(22)), csum="auto", dmac=CM, tags=(), **ipkw):
    u = F.udp(sp, dp, payload, csum=csum, pseudo=F.ipv4_pseudo(F.ip4(SIP), F.ip4(DIP), 17, 8 + len(payload)))
    return _l2(dmac, tags, F.ipv4(SIP, DIP, 17, u, **ipkw))


def tcpf(payload=b"hello tcp!", doff=5, options=b"", csum="auto", dmac=CM, tags=(), **ipkw):
    n = 20 + len(options) + len(payload)
    t = F.tcp(1000, 80, payload, doff=doff, options=options, csum=csum, pseudo=F.ipv4_pseudo(F.ip4(SIP), F.ip4(DIP), 6, n))
    return _l2(dmac, tags, F.ipv4(SIP, DIP, 6, t, **ipkw))


def _frames_of(w):
    return [bytes(w["buf"][int(d["off"]):int(d["off"]) + int(d["len"])]) for d in w["desc"]]


_B256 = {}


def plain256():
    """config B's first 256 frames (computed once): untagged IPv4 / UDP, 64 bytes each."""
    if not _B256:
        w = synth.config_b(256)
        _B256["w"], _B256["frames"] = w, _frames_of(w)
    return _B256["w"], list(_B256["frames"])


def batch(frames, vports=None, holes=()):
    buf, desc = F.pack_frames(frames, vports)
    for h in holes:
        desc["pad"][h] = abi.DESC_HOLE
    return buf, desc


# ---- checks -----------------------------------------------------------------------------------
def check(rx, o, buf, desc, classify=True):
    """check_batch; a batch with empty descriptor slots against the oracle's outputs for the
    other descriptors, with a hole record spliced in for each slot (no queue entry, no count)."""
    holes = np.nonzero(desc["pad"] == abi.DESC_HOLE)[0]
    if not len(holes):
        return check_batch(rx, o, buf, desc, classify)
    import pyoracle
    from emurx.rx import hist_to_counters
    assert classify
    keep = np.setdiff1d(np.arange(len(desc)), holes)
    orec, oq, oqoff, ocnt = o.rx_batch(buf, desc[keep])
    want = np.zeros(len(desc), abi.REC_DTYPE)
    want[keep] = orec
    want[holes] = _hole_rec()
    rec, qlist, qoff, hist = run_dev(rx, buf, desc)
    assert rec.tobytes() == want.tobytes(), rec_diff(rec, want)
    assert np.array_equal(qlist, keep[oq].astype(np.uint32)) and np.array_equal(qoff, oqoff)
    got, cnt = hist_to_counters(hist), pyoracle.counters_dict(ocnt)
    for k in abi.PARSER_COUNTER_NAMES + ["ref_panic"]:
        assert got[k] == cnt[k], k
    assert int(hist[0::2].sum()) == len(keep)
    return rec


def tile0(rx):
    """The witness words of tile 0's four waves."""
    return [int(x) for x in rx.last_uniform()[:4]]


def pair_b(rxmod, w):
    rx, o = new_pair(rxmod)
    synth.load_tables(w, rx)
    synth.load_tables(w, o)
    return rx, o


def pair_frames(rxmod, frames):
    rx, o = new_pair(rxmod)
    ns, cl = frames_tables(frames, vport=0)
    load_frame_tables([rx, o], ns, cl)
    return rx, o


# ---- all-plain batches ------------------------------------------------------------------------
def _plain_want(n, bits):
    """Tile 0's words for a dense batch of n plain frames: full waves on the path (bits), the
    wave holding the ragged end and the waves past it sampled but not on it."""
    return [bits if n >= 64 * (k + 1) else S for k in range(4)]


# 100: the ragged end (36 frames in wave 1) lies in the sampled tile
@pytest.mark.parametrize("n", [64, 100, 256, 257, 4099])
def test_plain_batches(rxmod, n):
    w = synth.config_b(n)
    rx, o = pair_b(rxmod, w)
    rec = check(rx, o, w["buf"], w["desc"])
    assert (rec["status"] == 0).all() and (rec["client_id"] == 0).all()
    assert tile0(rx) == _plain_want(n, ALL)
    check(rx, o, w["buf"], w["desc"], classify=False)  # kind 0: the parse alone
    assert tile0(rx) == _plain_want(n, S | P)


# ---- one odd lane: the wave falls back --------------------------------------------------------
def _odd_lane_cases():
    """name -> (frame or None for a hole).  Each differs from the plain shape in one fact the
    straight-line parse assumes."""
    return {
        "tag": udpf(tags=((F.ETH_DOT1Q, 7),)),
        "ipv6": E.udp6(1234, 5000),
        "arp": E.eth(F.ETH_ARP, F.arp(1, SM, "1.1.1.1", bytes(6), DIP)),
        "ihl6": udpf(options=bytes([0x94, 0x04, 0x00, 0x00])),
        "fragment": udpf(flags=1),
        "totlen_lt_28": udpf(payload=b"", length=27),
        "cut_short": udpf()[:-3],
        "padded": udpf() + bytes(5),
        "hole": None,
    }


@pytest.mark.parametrize("wave,lane", [(0, 0), (0, 31), (3, 63), (3, 0), (0, 63), (3, 31)])
@pytest.mark.parametrize("name", list(_odd_lane_cases()))
def test_one_odd_lane_falls_back(rxmod, name, wave, lane):
    w, frames = plain256()
    f, at = _odd_lane_cases()[name], wave * 64 + lane
    if f is not None:
        frames[at] = f
    buf, desc = batch(frames, holes=[at] if f is None else ())
    rx, o = pair_b(rxmod, w)
    check(rx, o, buf, desc)
    assert tile0(rx) == [S if k == wave else ALL for k in range(4)]


# ---- a failure or a special rule in one lane: the parse stays straight-line ---------------------
def _staying_cases():
    """name -> (frame, vport, the lookups stay on the path too)."""
    return {
        "bad_ipv4_cs": (_bad_ip_cs(), 0, False),
        "bad_udp_cs": (udpf(csum=0xABCD), 0, False),
        "zero_udp_cs": (udpf(csum=0), 0, True),
        "mdns": (udpf(dp=5353), 0, False),
        "dhcp": (udpf(sp=67, dp=68), 0, False),
        "dhcpsrv": (udpf(sp=68, dp=67), 0, False),
        "bcast_mac": (udpf(dmac=bytes([0xFF] * 6)), 0, False),
        "zero_mac": (udpf(dmac=bytes(6)), 0, False),
        "unknown_mac": (udpf(dmac=bytes([2, 0, 0, 0, 9, 9])), 0, False),
        "unknown_ns": (udpf(), 5, False),
    }


def _bad_ip_cs():
    u = F.udp(1234, 5000, bytes(22), csum=0, pseudo=None)
    return _l2(CM, (), F.ipv4(SIP, DIP, 17, u, csum=0x1234))


@pytest.mark.parametrize("wave,lane", [(0, 0), (3, 63), (0, 31)])
@pytest.mark.parametrize("name", list(_staying_cases()))
def test_one_lane_stays_straight_line(rxmod, name, wave, lane):
    w, frames = plain256()
    f, vport, lookups = _staying_cases()[name]
    at = wave * 64 + lane
    frames[at] = f
    vports = [0] * 256
    vports[at] = vport
    buf, desc = batch(frames, vports)
    rx, o = pair_b(rxmod, w)
    rec = check(rx, o, buf, desc)
    if name.startswith("bad_"):
        assert rec["status"][at] != 0
    assert tile0(rx) == [(ALL if lookups else S | P) if k == wave else ALL for k in range(4)]


# ---- uniformly tagged waves, TCP ---------------------------------------------------------------
@pytest.mark.parametrize("proto", ["udp", "tcp"])
@pytest.mark.parametrize("tags", [((F.ETH_DOT1Q, 7),), ((F.ETH_QINQ, 5), (F.ETH_DOT1Q, 6)), ()])
def test_uniformly_tagged_waves(rxmod, tags, proto):
    """256 frames with the same tags, distinct payload lengths and source ports (the L4 sums
    differ in length and alignment from lane to lane).  TCP: lane 5 has data offset 6, lane 70
    a data offset past its segment (TCP_TOO_SHORT by select), lane 130 a bad checksum."""
    frames = []
    for i in range(256):
        pay = bytes((i + k) & 0xFF for k in range(4 + i % 29))
        if proto == "udp":
            frames.append(udpf(sp=1024 + i, payload=pay, tags=tags, csum=0 if i == 9 else "auto"))
        elif i == 5:
            frames.append(tcpf(pay, doff=6, options=bytes([1, 1, 1, 0]), tags=tags))
        elif i == 70:
            frames.append(tcpf(b"", doff=15, tags=tags))
        else:
            frames.append(tcpf(pay, tags=tags, csum=0xBEEF if i == 130 else "auto"))
    rx, o = pair_frames(rxmod, frames)
    buf, desc = batch(frames)
    rec = check(rx, o, buf, desc)
    if proto == "tcp":
        assert rec["status"][70] == abi.ST["TCP_TOO_SHORT"] and rec["status"][130] == abi.ST["TCP_CS"]
        assert rec["l7"][5] == rec["l4"][5] + 24
    w = tile0(rx)
    assert all(x & P for x in w), w
    check(rx, o, buf, desc, classify=False)
    assert tile0(rx) == [S | P] * 4


def test_mixed_tag_counts_fall_back(rxmod):
    """Wave 0 half untagged, half tagged; wave 1 UDP with one TCP lane; waves 2, 3 plain."""
    _, frames = plain256()
    for i in range(32, 64):
        frames[i] = udpf(tags=((F.ETH_DOT1Q, 7),))
    frames[64 + 17] = tcpf()
    rx, o = pair_frames(rxmod, frames)
    check(rx, o, *batch(frames))
    w = tile0(rx)
    assert w[0] == S and w[1] == S and w[2] & P and w[3] & P


# ---- every edge case in an otherwise plain wave -------------------------------------------------
@pytest.mark.parametrize("classify", [True, False])
def test_edge_cases_in_plain_waves(rxmod, classify):
    """One wave per case of edge_frames.cases(): 63 plain frames and the case, at a lane that
    moves with the case."""
    w, plain = plain256()
    cases = E.cases()
    frames, vports = [], []
    for k, c in enumerate(cases):
        wave = plain[:64]
        vp = [0] * 64
        wave[(7 * k) % 64], vp[(7 * k) % 64] = c[1], c[2]
        frames += wave
        vports += vp
    assert 6000 < len(frames) < 7000
    rx, o = pair_b(rxmod, w)
    buf, desc = batch(frames, vports)
    rec = check(rx, o, buf, desc, classify)
    got = {abi.STATUS_NAMES[s] for s in rec["status"]}
    assert {c[3] for c in cases} <= got


# ---- the three slabs, and kind 2 ----------------------------------------------------------------
def _odd_batches():
    """(name, buf, desc, tile 0's parse bits) of an all-plain batch and of one-odd-lane batches
    without holes (the oracle takes no holes; kind 2 is checked against it whole)."""
    w, plain = plain256()
    out = [("plain", w["buf"], w["desc"], [1, 1, 1, 1])]
    odd = _odd_lane_cases()
    for name, at in (("tag", 0), ("ipv6", 31), ("ihl6", 3 * 64 + 63), ("padded", 3 * 64), ("cut_short", 63)):
        frames = list(plain)
        frames[at] = odd[name]
        buf, desc = batch(frames)
        out.append((name, buf, desc, [int(k != at // 64) for k in range(4)]))
    return w, out


@pytest.mark.parametrize("stage,bytes_", [("tight", 5120), ("narrow", 6144), ("wide", 7168)])
def test_slabs(rxmod, monkeypatch, stage, bytes_):
    monkeypatch.setenv("EMURX_STAGE", stage)  # read by emurx_open
    w, batches = _odd_batches()
    rx, o = pair_b(rxmod, w)
    for name, buf, desc, want in batches:
        check(rx, o, buf, desc)
        assert rx.last_stage() == bytes_
        assert [x & P for x in tile0(rx)] == want, name
        assert [bool(x & L) for x in tile0(rx)] == [bool(x) for x in want], name
        check(rx, o, buf, desc, classify=False)
        assert [x & P for x in tile0(rx)] == want, name
    hole = batch(plain256()[1], holes=[64 + 31])
    check(rx, o, *hole)
    assert tile0(rx) == [ALL, S, ALL, ALL]


@pytest.mark.parametrize("stage", ["tight", "narrow", "wide"])
def test_kind2_two_parts(rxmod, monkeypatch, stage):
    """parse_route_dev (k_rx kind 2) with 2 partitions, lookup_dev on the owners, against the
    oracle (test_gpu_tables.partitioned_vs_oracle); the sources' witness shows the parse on the
    path and, kind 2 doing no lookups, never the lookups."""
    from test_gpu_tables import partitioned_vs_oracle
    monkeypatch.setenv("EMURX_STAGE", stage)
    w, batches = _odd_batches()
    made = []

    def factory(*a, **k):
        made.append(rxmod(*a, **k))
        return made[-1]

    for name, buf, desc, want in batches[:4]:
        del made[:]
        shards = [dict(buf=buf, desc=desc), dict(buf=w["buf"], desc=w["desc"])]
        partitioned_vs_oracle(factory, shards, lambda t: synth.load_tables(w, t), 2)
        full, src0, src1 = made
        assert [x & (P | L) for x in tile0(src0)] == want, name
        assert [x & (P | L) for x in tile0(src1)] == [1, 1, 1, 1], name
        for h in made:
            h.close()


# ---- the switch ---------------------------------------------------------------------------------
def test_switch_off(rxmod, monkeypatch):
    """EMURX_UNIFORM=0: no sampled wave on the path, outputs byte-identical to the default."""
    w, batches = _odd_batches()
    cases = E.cases()
    mixed = batch([c[1] for c in cases] + plain256()[1], [c[2] for c in cases] + [0] * 256)
    todo = [(b, d) for _, b, d, _ in batches] + [mixed]
    outs = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("EMURX_UNIFORM", mode)
        rx, _ = pair_b(rxmod, w)
        outs[mode] = []
        for buf, desc in todo:
            for classify in (True, False):
                rec, ql, qoff, hist = run_dev(rx, buf, desc, classify)
                outs[mode].append((rec.tobytes(), ql.tobytes(), qoff.tobytes(), hist.tobytes()))
                words = rx.last_uniform()
                assert (words[:4] & S).all()
                if mode == "0":
                    assert not (words & (P | L)).any()
        rx.close()
    assert outs["1"] == outs["0"]
    monkeypatch.delenv("EMURX_UNIFORM")
    rx, o = pair_b(rxmod, w)
    check(rx, o, *todo[0])
    assert tile0(rx) == [ALL] * 4  # the default is on

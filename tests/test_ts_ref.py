"""The timestamp reply's rule (tests/ts_ref.py) against what the reference recorded and on every
branch, without a GPU.

The reference's TestPluginIcmp2 sends six timestamp requests; its capture holds no packets, because
the replies carry the clock, only the counters: pktRxIcmpQuery 6, pktTxIcmpResponse 6
(tests/golden/icmp2_counters.json, extracted by tests/golden/make_icmp2_counters.py).  The requests
are rebuilt from the Go test's source (icmp_test.go:221-250) and classified by the oracle in the
"icmp" environment of sim_envs."""
import json
import struct
from pathlib import Path

import numpy as np
import pytest

import nsstat_ref as NS
import respond_ref as R
import sim_envs as S
import ts_ref as T
from emurx import abi, frames as F
from test_nsstat_ref import sim_envs

COUNTERS = json.loads((Path(__file__).parent / "golden" / "icmp2_counters.json").read_text())
TIMES = [0, 1, 86_399_999, 0xFFFFFFFF]
ALL = abi.RSPK_ALL_TS


@pytest.fixture(scope="module")
def six(oracle_built):
    o = oracle_built.Oracle()
    S.load_env(o, "icmp")
    fr = T.six_requests()
    buf, desc = F.pack_frames(fr, [1] * len(fr))
    rec = o.rx_batch(buf, desc)[0]
    return dict(fr=fr, buf=buf, desc=desc, rec=rec, env4=sim_envs("icmp")[0])


@pytest.fixture(scope="module")
def tables(oracle_built):
    o, env = oracle_built.Oracle(), R.Env()
    R.load_tables(o, env)
    return o, env


def classify(tables, frames):
    buf, desc = F.pack_frames(frames, [1] * len(frames))
    return tables[0].rx_batch(buf, desc)[0]


def one(tables, frame, kinds=ALL, ip_time=0x01020304, rec=None):
    rec = classify(tables, [frame])[0] if rec is None else rec
    assert int(rec["status"]) == 0 and (int(rec["flags"]) >> 4) & 7 == abi.LK["CLIENT"] and int(rec["proto"]) == T.CB_ICMP
    return T.ts_ref(frame, rec, kinds, ip_time, tables[1]), rec


def test_tcpip_checksum_is_the_fold_of_frames():
    rng = np.random.default_rng(3)
    for n in (0, 1, 2, 3, 20, 21, 1501):
        d = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        assert T.tcpip_checksum(d) == F.csum_fold(d)
    assert T.tcpip_checksum(b"\xff\xff") == 0 and T.tcpip_checksum(b"\xff" * 9216) == 0
    assert T.tcpip_checksum(b"\x01") == 0xFEFF  # an odd last byte counts as its pair's high byte


@pytest.mark.parametrize("ip_time", TIMES)
def test_six_requests(six, ip_time):
    m = six
    outcome, od, src, replies, info = T.respond_batch(m["buf"], m["desc"], m["rec"], ALL, ip_time, m["env4"])
    assert (outcome == abi.RSP_TS).all() and len(replies) == 6 and list(src) == list(range(6))
    assert int(info[0]) == 6 and int(info[1]) == 6 * 64 and int(info[1 + abi.RSP_TS]) == 6 and int(info[2:].sum()) == 6
    for f, r, seq in zip(m["fr"], replies, T.SIX_SEQ):
        l4 = 42
        assert len(r) == len(f) == 62 and r[:6] == f[6:12] and r[6:12] == f[:6] and r[12:22] == f[12:22]
        assert r[22:34] == f[22:34] and r[34:38] == f[38:42] and r[38:42] == f[34:38]  # the header checksum holds
        assert F.csum_fold(r[22:42]) == 0
        assert r[l4] == 14 and r[l4 + 1] == 0 and r[l4 + 4:l4 + 8] == struct.pack(">HH", 1, seq)
        assert r[l4 + 8:l4 + 12] == f[l4 + 8:l4 + 12]  # the originate timestamp stays
        assert r[l4 + 12:l4 + 16] == r[l4 + 16:l4 + 20] == struct.pack(">I", ip_time)
        assert T.span_sum(r[l4:]) == 0xFFFF  # the reply verifies
    rsp = outcome
    done, ev, ninfo = T.nsstat_batch(m["buf"], m["desc"], m["rec"], ALL, rsp, np.zeros(6, np.uint8))
    assert (done == 1).all() and tuple(int(x) for x in ninfo) == (1, 1, 0, 6, 0, 0, 0, 0)
    assert int(ev[0]["frames"]) == 6
    got = {name: v for (ns, plug, name), v in NS.replay(ev).items() if plug == "icmp"}
    assert got == COUNTERS and len(NS.replay(ev)) == 2


def test_six_requests_without_ts_stay_with_the_handler(six):
    m = six
    outcome = T.respond_batch(m["buf"], m["desc"], m["rec"], abi.RSPK_ALL, 5, m["env4"])[0]
    assert (outcome == abi.RSP_HOST).all()
    assert np.array_equal(outcome, R.respond_batch(m["buf"], m["desc"], m["rec"], m["env4"])[0])
    done, ev, _ = T.nsstat_batch(m["buf"], m["desc"], m["rec"], abi.RSPK_ALL, outcome, np.zeros(6, np.uint8))
    assert not done.any() and len(ev) == 0
    # outcomes of a call with more kinds than nsstat is asked for: the timestamp rule is not applied
    ts = np.full(6, abi.RSP_TS, np.uint8)
    assert not T.nsstat_batch(m["buf"], m["desc"], m["rec"], abi.RSPK_ALL, ts, np.zeros(6, np.uint8))[0].any()


def test_bad_source_ip(tables):
    for src in (bytes(4), bytes([224, 0, 0, 5]), bytes([169, 254, 1, 1]), b"\xff" * 4):
        for kinds in (ALL, abi.RSPK_TS, abi.RSPK_ICMP):
            (o, r), _ = one(tables, T.ts_frame(1, 2, src=src), kinds)
            assert (o, r) == (abi.RSP_DROP_MCAST, None)
    (o, r), _ = one(tables, T.ts_frame(1, 2, src=bytes([127, 0, 0, 1])))
    assert o == abi.RSP_TS


def test_multicast_comes_before_too_short(tables):
    group = bytes([1, 0, 0x5E, 0, 0, 1])
    (o, _), rec = one(tables, T.ts_frame(0, 1, span=19, esrc=group))
    assert o == abi.RSP_DROP_MCAST
    assert T.nsstat_decide(T.ts_frame(0, 1, span=19, esrc=group), rec, ALL, o)[:2] == (1, [abi.NSC_ICMP_ERR_MCAST])
    assert one(tables, T.ts_frame(0, 1, span=19, esrc=b"\xff" * 6))[0][0] == abi.RSP_DROP_MCAST
    assert one(tables, T.ts_frame(0, 1, span=20, esrc=group))[0][0] == abi.RSP_DROP_MCAST


@pytest.mark.parametrize("span,want", [(8, abi.RSP_DROP_SHORT), (19, abi.RSP_DROP_SHORT), (20, abi.RSP_TS)])
def test_span_lengths(tables, span, want):
    f = T.ts_frame(2, 3, span=span)
    (o, r), rec = one(tables, f)
    assert o == want and (r is None) == (want != abi.RSP_TS)
    done, cnt, cand = T.nsstat_decide(f, rec, ALL, o)
    assert (done, cand) == (1, True)
    assert cnt == [abi.NSC_ICMP_ERR_TOO_SHORT if want == abi.RSP_DROP_SHORT else abi.NSC_ICMP_ECHO]
    ev, info = NS.fold(np.array([rec["ns_id"]]), np.array([done], np.uint8), [cnt], np.array([cand]))
    names = {name for (_, plug, name) in T.replay(ev) if plug == "icmp"}
    assert names == ({"pktRxErrTooShort"} if want == abi.RSP_DROP_SHORT else {"pktRxIcmpQuery", "pktTxIcmpResponse"})
    assert int(ev[0]["frames"]) == 1  # the too-short counter is one a frame bumps alone: it adds to `frames`
    # left with the handler: done 0
    for host in (abi.RSP_HOST, abi.RSP_NOSPC, abi.RSP_NONE):
        assert T.nsstat_decide(f, rec, ALL, host)[:2] == (0, [])


def test_trailing_bytes_are_summed(tables):
    """The span is the rest of the frame, not the IPv4 total length."""
    f = T.ts_frame(1, 0, span=36)  # 20 bytes of ICMP, 16 of trailer
    (o, r), rec = one(tables, f)
    l4 = int(rec["l4"])
    assert o == abi.RSP_TS and any(f[l4 + 20:]) and r[l4 + 20:] == f[l4 + 20:]
    assert T.span_sum(r[l4:]) == 0xFFFF and T.span_sum(r[l4:l4 + 20]) != 0xFFFF
    g = f[:-1] + bytes([f[-1] ^ 0x40])
    (o2, r2), _ = one(tables, g)
    assert o2 == abi.RSP_TS and r2[l4 + 2:l4 + 4] != r[l4 + 2:l4 + 4] and T.span_sum(r2[l4:]) == 0xFFFF


@pytest.mark.parametrize("span", [21, 37])
def test_odd_frame_length(tables, span):
    f = T.ts_frame(0, 0, span=span)
    (o, r), rec = one(tables, f)
    l4 = int(rec["l4"])
    assert o == abi.RSP_TS and len(r) % 2 == 1 and r[-1] == f[-1] != 0
    assert T.span_sum(r[l4:]) == 0xFFFF
    # the last byte counts as a high byte: the same byte as a low byte gives another checksum
    assert T.tcpip_checksum(r[l4:l4 + 2] + b"\0\0" + r[l4 + 4:]) == struct.unpack(">H", r[l4 + 2:l4 + 4])[0]


def test_sum_ffff_stores_zero(tables):
    ip_time = 0x0123ABCD
    f = T.ffff_frame(1, 1, ip_time, span=36)
    (o, r), rec = one(tables, f, ip_time=ip_time)
    l4 = int(rec["l4"])
    assert o == abi.RSP_TS and r[l4 + 2:l4 + 4] == b"\0\0" and T.span_sum(r[l4:]) == 0xFFFF


def test_kinds(tables):
    ts, echo = T.ts_frame(1, 1), R.mixed_batch(1)[0][0]
    for kinds in range(1, 16):
        want = abi.RSP_HOST if kinds & abi.RSPK_ICMP else abi.RSP_NONE
        assert one(tables, ts, kinds)[0] == (want, None)
    rec = classify(tables, [echo])[0]
    assert T.ts_ref(echo, rec, abi.RSPK_TS, 0, tables[1]) == (abi.RSP_NONE, None)  # TS alone: no echo reply
    assert T.ts_ref(echo, rec, ALL, 0, tables[1]) == R.respond_ref(echo, rec, tables[1])
    assert T.ts_ref(echo, rec, ALL, 0, tables[1])[0] == abi.RSP_ICMP
    assert one(tables, ts, abi.RSPK_TS)[0][0] == abi.RSP_TS
    (o, _), _ = one(tables, T.ts_frame(1, 1, typ=17), ALL)  # address mask request: no case of the switch
    assert o == abi.RSP_NONE


def test_odd_l4_and_offsets_that_do_not_fit(tables):
    f = T.ts_frame(0, 0, span=24)
    rec = classify(tables, [f])[0].copy()
    l4 = int(rec["l4"])
    rec["l4"] = l4 + 1  # a record no parse writes: the message one byte further on
    g = f[:l4] + b"\0" + f[l4:]
    assert g[l4 + 1] == 13 and T.ts_ref(g, rec, ALL, 0, tables[1]) == (abi.RSP_HOST, None)
    assert T.ts_ref(g[:l4 + 20], rec, ALL, 0, tables[1]) == (abi.RSP_DROP_SHORT, None)  # the length test comes first
    rec["l4"] = len(f) - 7
    assert T.ts_ref(f, rec, ALL, 0, tables[1]) == (abi.RSP_HOST, None)
    assert T.ts_ref(f, classify(tables, [f])[0], ALL, 0, tables[1], hole=True) == (abi.RSP_NONE, None)


def test_mixed_batch_keeps_every_other_answer(tables):
    """With TS added, every frame that is no timestamp request gets respond_ref's answer."""
    fr, vp = R.mixed_batch(300)
    buf, desc = R.pack_with_holes(fr, vp)
    rec = tables[0].rx_batch(buf, desc)[0]
    old = R.respond_batch(buf, desc, rec, tables[1])
    new = T.respond_batch(buf, desc, rec, 7 | abi.RSPK_TS, 77, tables[1])
    same = T.respond_batch(buf, desc, rec, 7, 77, tables[1])
    assert np.array_equal(same[0], old[0]) and same[3] == old[3] and np.array_equal(same[4][:8], old[4])
    diff = np.nonzero(new[0] != old[0])[0]
    assert len(diff) >= 5 and (old[0][diff] == abi.RSP_HOST).all() and (new[0][diff] == abi.RSP_TS).all()
    assert all(fr[i][int(rec[i]["l4"])] == 13 for i in diff)

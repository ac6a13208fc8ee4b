"""The neighbour-advertisement rule against the reference's own captures, the ND batch's coverage,
and the argument checks of emurx_respond_kinds_dev on a host-only handle (no GPU).

nd_ref (tests/nd_ref.py) applied to the rx frames of ipv6nd_2 (six unicast solicitations) and
ipv6nd_3 (six duplicate-address-detection probes), with records from the oracle and the
environment of the capture's Go test (tests/sim_envs.py), must give the capture's six answering
tx frames byte for byte, in order."""
import ctypes as C
import struct
from collections import Counter

import numpy as np
import pytest

import nd_ref as N
import respond_ref as R
import sim_envs as S
from emurx import abi, frames as F
from test_oracle_corpus import GOLD

CAPTURES = [("ipv6nd_2.json", 6, "unicast"), ("ipv6nd_3.json", 6, "dad")]
NOT_NS = ["ipv6nd_1.json", "ipv6nd_4.json", "ipv6nd_rpc.json"]


def sim_env():
    e = S.ENVS["ipv6"]
    env = N.Env()
    env.add(S.NS_KEY, 0, e["mac"], e["ipv6"], None, 1 << S.PLUG.index("ipv6"))
    return env


def capture_tx(z, capture):
    files = [str(x) for x in z["files"]]
    idx = np.nonzero((z["src"] == files.index(capture)) & (z["meta"] == 0))[0]
    return [z["data"][z["off"][i]:z["off"][i] + z["len"][i]].tobytes() for i in idx]


def capture_case(capture):
    """-> buf, desc, the oracle's records, the Env, the capture's tx frames"""
    import pyoracle
    z = np.load(GOLD, allow_pickle=False)
    fr = S.rx_frames(z, capture)
    o = pyoracle.Oracle()
    S.load_env(o, "ipv6")
    buf, desc = F.pack_frames(fr, [1] * len(fr))
    rec, _, _, _ = o.rx_batch(buf, desc)
    return buf, desc, rec, sim_env(), capture_tx(z, capture)


def capture_replies(tx, replies):
    """The capture's tx frames that answer its rx frames: the capture's other advertisements are
    unsolicited, so the answers are selected by matching the rule's output, in order."""
    out, k = [], 0
    for r in replies:
        while k < len(tx) and tx[k] != r:
            k += 1
        if k == len(tx):
            return out
        out.append(tx[k])
        k += 1
    return out


def rfc1071(data: bytes) -> int:
    """A plain RFC 1071 sum, independent of the helpers the rule is built with."""
    if len(data) % 2:
        data += b"\x00"
    s = 0
    for i in range(0, len(data), 2):
        s += (data[i] << 8) | data[i + 1]
    while s >> 16:
        s = (s & 0xFFFF) + (s >> 16)
    return s


def icmp6_checksum_ok(reply: bytes) -> bool:
    l3 = 14
    while reply[l3 - 2:l3] in (b"\x81\x00", b"\x88\xa8"):
        l3 += 4
    assert reply[l3 - 2:l3] == b"\x86\xdd" and reply[l3 + 6] == 58
    plen = struct.unpack(">H", reply[l3 + 4:l3 + 6])[0]
    assert l3 + 40 + plen == len(reply)
    pseudo = reply[l3 + 8:l3 + 40] + struct.pack(">I", plen) + bytes([0, 0, 0, 58])
    return rfc1071(pseudo + reply[l3 + 40:]) == 0xFFFF


@pytest.mark.parametrize("capture,n_replies,form", CAPTURES, ids=[c[0] for c in CAPTURES])
def test_capture_replies(oracle_built, capture, n_replies, form):
    buf, desc, rec, env, tx = capture_case(capture)
    assert len(desc) == n_replies
    outcome, od, src, got, info = N.respond_batch(buf, desc, rec, abi.RSPK_ND, env6=env)
    assert (outcome == abi.RSP_ND).all() and len(got) == n_replies and int(info[0]) == n_replies
    assert int(info[1 + abi.RSP_ND]) == n_replies and (info[9:] == 0).all()
    want = capture_replies(tx, got)
    assert len(want) == n_replies
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, (k, g.hex(), w.hex())
        assert len(g) == 94 and icmp6_checksum_ok(g)
        assert (g[:6] == bytes([0x33, 0x33, 0, 0, 0, 1])) == (form == "dad")
    # the same records give nothing when ND is not asked for
    o7, _, _, r7, _ = N.respond_batch(buf, desc, rec, 7, env4=R.Env(), env6=env)
    assert not r7 and (o7 == abi.RSP_NONE).all()


@pytest.mark.parametrize("capture", NOT_NS)
def test_capture_not_a_solicitation(oracle_built, capture):
    buf, desc, rec, env, _ = capture_case(capture)
    assert len(desc) > 0
    outcome, _, _, got, info = N.respond_batch(buf, desc, rec, abi.RSPK_ALL, env4=R.Env(), env6=env)
    assert not got and (outcome == abi.RSP_NONE).all() and (info == 0).all()


def nd_case(n, seed=11):
    import pyoracle
    fr, vp, labels = N.nd_batch(n, seed)
    o = pyoracle.Oracle()
    env = N.Env()
    N.load_tables(o, env)
    buf, desc = R.pack_with_holes(fr, vp, every=N.HOLE_EVERY)
    rec, _, _, _ = o.rx_batch(buf, desc)
    return fr, buf, desc, rec, env, labels


# the branches of the rule a classified frame can reach
BRANCHES = ["not-ns", "too-short", "options-long", "options-1-7", "options-8-wrong", "hop-limit", "slla-zero",
            "dad-with-slla", "dad-unicast-dst", "target-unspec-mcast", "target-not-local-global", "eui-mac-miss",
            "eui-prefix", "eui-no-plugin", "plain-not-global", "ip6-miss", "ip6-no-plugin", "eui-local-unicast",
            "eui-local-dad", "eui-ra-unicast", "eui-ra-dad", "ip6-unicast", "ip6-dad"]


def test_nd_batch_reaches_every_branch(oracle_built):
    """Conditions on the inputs: a comparison against nd_ref cannot pass on an empty set."""
    fr, buf, desc, rec, env, labels = nd_case(257)
    n = len(desc)
    outcome, od, src, replies, info = N.respond_batch(buf, desc, rec, abi.RSPK_ND, env6=env)
    hole = desc["pad"] == abi.DESC_HOLE
    why = [N.nd_branch(fr[i], rec[i], env, hole=bool(hole[i])) for i in range(n)]
    seen = Counter(why)
    for b in BRANCHES:
        assert seen[b] >= 2, (b, seen)
    # every entry of the generator's list occurs at least twice, and the rule gives it the outcome
    # it was built for (holes apart)
    want = {label: o for label, o, _ in N.KINDS}
    count = Counter(l for i, l in enumerate(labels) if not hole[i])
    for label in want:
        assert count[label] >= 2, label
    for i in range(n):
        if not hole[i]:
            assert outcome[i] == want[labels[i]], (i, labels[i], why[i], int(outcome[i]))
    # every candidate is an icmpv6 NS_LEVEL record with status OK: the frames are valid for the parser
    ns = [i for i in range(n) if why[i] != "not-candidate"]
    assert all(int(rec[i]["status"]) == 0 and int(rec[i]["proto"]) == N.CB_ICMPV6 for i in ns)
    assert {labels[i] for i in range(n) if why[i] == "not-candidate" and not hole[i]} == set()
    # holes over frames that would otherwise be answered
    assert hole.sum() >= 2 and (outcome[hole] == abi.RSP_NONE).all()
    assert sum(N.nd_ref(fr[i], rec[i], env)[1] is not None for i in np.nonzero(hole)[0]) >= 2
    # the shapes: a quarter of the frames answered, every tag count, both forms, extension headers
    assert 4 * len(replies) >= n
    assert {len(r) for r in replies} == {86, 90, 94}
    dad = [r[:6] == bytes([0x33, 0x33, 0, 0, 0, 1]) for r in replies]
    assert sum(dad) >= 8 and len(dad) - sum(dad) >= 8
    assert {int(rec[s]["l4"]) - int(rec[s]["l3"]) - 40 for s in src} == {0, 8, 24}
    slla = [int(desc["len"][s]) - int(rec[s]["l4"]) - 24 for s in src]
    assert set(slla) == {0, 8}
    n_ns = sum(1 for i in range(n) if why[i] not in ("not-candidate", "not-ns"))
    n_host = int((outcome == abi.RSP_HOST).sum())
    assert 1 <= n_host <= 0.05 * n_ns, (n_host, n_ns)
    assert int(info[1]) == 96 * len(replies) and int(info[1 + abi.RSP_ND]) == len(replies)
    # with a buffer one row short the last reply alone is refused
    o2, _, _, r2, i2 = N.respond_batch(buf, desc, rec, abi.RSPK_ND, env6=env, out_cap=int(info[1]) - 16)
    assert len(r2) == len(replies) - 1 and (o2 == abi.RSP_NOSPC).sum() == 1 and i2[1] == info[1]


def test_nd_reply_checksums(oracle_built):
    fr, buf, desc, rec, env, labels = nd_case(257)
    replies = N.respond_batch(buf, desc, rec, abi.RSPK_ND, env6=env)[3]
    assert len(replies) > 60
    for r in replies:
        assert icmp6_checksum_ok(r), r.hex()


def combined_case(n, seed=5):
    import pyoracle
    fr, vp = N.combined_batch(n, seed)
    o = pyoracle.Oracle()
    env4, env6 = R.Env(), N.Env()
    N.load_combined(o, env4, env6)
    buf, desc = R.pack_with_holes(fr, vp)
    rec, _, _, _ = o.rx_batch(buf, desc)
    return buf, desc, rec, env4, env6


def test_combined_batch_holds_all_four_answers(oracle_built):
    buf, desc, rec, env4, env6 = combined_case(257)
    outcome, od, src, replies, info = N.respond_batch(buf, desc, rec, abi.RSPK_ALL, env4, env6)
    for k in range(8):
        if k != abi.RSP_NOSPC:
            assert (outcome == k).sum() >= 2, k
    # kinds select: ND alone leaves the other answers' frames NONE, and the other way round
    o8 = N.respond_batch(buf, desc, rec, abi.RSPK_ND, env4, env6)[0]
    o7, _, _, _, i7 = N.respond_batch(buf, desc, rec, 7, env4, env6, info_words=8)
    assert set(np.unique(o8)) == {abi.RSP_NONE, abi.RSP_HOST, abi.RSP_ND}
    assert abi.RSP_ND not in o7 and len(i7) == 8
    both = np.where(o8 != abi.RSP_NONE, o8, o7)
    assert np.array_equal(both, outcome)
    # kinds = 7 is emurx_respond_dev: respond_ref's own batch function agrees
    w = R.respond_batch(buf, desc, rec, env4)
    assert np.array_equal(w[0], o7) and np.array_equal(w[4], i7)


# ---- the C-ABI's argument checks (host-only handle: no device is touched) -----------------
@pytest.fixture()
def host_handle(lib):
    cfg = abi.Cfg(-1, 16, 16, 1 << 10, 1 << 16)
    h = C.c_void_p()
    assert lib.emurx_open(C.byref(cfg), C.byref(h)) == 0
    yield lib, h
    lib.emurx_close(h)


def test_respond_kinds_abi_constants(lib):
    assert abi.RSP_ND == 7 and abi.RSP_INFO_WORDS == 16
    assert (abi.RSPK_ARP, abi.RSPK_ICMP, abi.RSPK_ICMPV6, abi.RSPK_ND, abi.RSPK_ALL) == (1, 2, 4, 8, 15)
    assert any(s[0] == "emurx_respond_kinds_dev" for s in abi.SIGNATURES)
    assert hasattr(lib, "emurx_respond_kinds_dev")


def test_respond_kinds_argument_checks(host_handle):
    lib, h = host_handle
    EINVAL, EDEVICE = -22, -5
    a = 0x10000  # stand-ins for device pointers: the checks come before anything is dereferenced

    def call(frames=a, desc=a, rec=a, n=4, kinds=abi.RSPK_ALL, out=a, cap=1024, odesc=a, osrc=a, outcome=a, info=a,
             handle=h):
        return lib.emurx_respond_kinds_dev(handle, frames, desc, rec, n, kinds, out, cap, odesc, osrc, outcome, info, None)

    assert call(kinds=0) == EINVAL
    assert call(kinds=16) == EINVAL
    assert call(kinds=abi.RSPK_ND | 32) == EINVAL
    for kw in (dict(handle=None), dict(frames=None), dict(desc=None), dict(rec=None), dict(out=None),
               dict(odesc=None), dict(osrc=None), dict(info=None), dict(info=None, n=0)):
        assert call(**kw) == EINVAL, kw
    assert call(out=a + 8) == EINVAL   # d_out is written in 16-byte rows
    assert call(rec=a + 8) == EINVAL   # d_rec is read in 16-byte halves
    assert call(n=abi.TX_ZMQ_MAX_FRAMES) == EINVAL
    # valid arguments reach the handle: a host-only one has no device
    for k in (abi.RSPK_ND, abi.RSPK_ARP, 7, abi.RSPK_ALL):
        assert call(kinds=k) == EDEVICE, k
    assert call(outcome=None) == EDEVICE
    assert call(out=None, cap=0) == EDEVICE
    assert call(frames=None, desc=None, rec=None, n=0, out=None, cap=0, odesc=None, osrc=None, outcome=None) == EDEVICE

"""The responder's rules against the reference's own captures, the mixed batch's coverage, and the
argument checks of emurx_respond_dev on a host-only handle (no GPU).

respond_ref (tests/respond_ref.py) applied to the rx frames of icmp1, arp4, arp5, icmpv6_1 and
icmpv6_2, with records from the oracle and the environment of the capture's Go test
(tests/sim_envs.py), must give the capture's tx replies byte for byte, in order."""
import ctypes as C
import struct

import numpy as np
import pytest

import respond_ref as R
import sim_envs as S
from emurx import abi, frames as F
from test_oracle_corpus import GOLD

CAPTURES = [("icmp1.json", "icmp", 6), ("arp4.json", "arp", 6), ("arp5.json", "arp", 0),
            ("icmpv6_1.json", "ipv6", 6), ("icmpv6_2.json", "ipv6", 6)]


def capture_replies(z, capture):
    """The capture's tx frames that are an ARP op 2, an ICMP type 0 or an ICMPv6 type 129, in order."""
    files = [str(x) for x in z["files"]]
    idx = np.nonzero((z["src"] == files.index(capture)) & (z["meta"] == 0))[0]
    out = []
    for i in idx:
        f = z["data"][z["off"][i]:z["off"][i] + z["len"][i]].tobytes()
        et, l3 = struct.unpack(">H", f[12:14])[0], 14
        while et in (0x8100, 0x88A8):
            et, l3 = struct.unpack(">H", f[l3 + 2:l3 + 4])[0], l3 + 4
        if et == 0x0806 and f[l3 + 6:l3 + 8] == b"\x00\x02":
            out.append(f)
        elif et == 0x0800 and f[l3 + 9] == 1 and f[l3 + 4 * (f[l3] & 15)] == 0:
            out.append(f)
        elif et == 0x86DD and f[l3 + 6] == 58 and f[l3 + 40] == 129:
            out.append(f)
    return out


def sim_env(name):
    e = S.ENVS[name]
    env = R.Env()
    env.add(e.get("key", S.NS_KEY), 0, e["mac"], e["ipv4"])
    return env


def capture_case(capture, envname):
    """-> buf, desc, the oracle's records, the Env, the capture's replies"""
    import pyoracle
    z = np.load(GOLD, allow_pickle=False)
    fr = S.rx_frames(z, capture)
    o = pyoracle.Oracle()
    S.load_env(o, envname)
    buf, desc = F.pack_frames(fr, [1] * len(fr))
    rec, _, _, _ = o.rx_batch(buf, desc)
    return buf, desc, rec, sim_env(envname), capture_replies(z, capture)


@pytest.mark.parametrize("capture,envname,n_replies", CAPTURES, ids=[c[0] for c in CAPTURES])
def test_capture_replies(oracle_built, capture, envname, n_replies):
    buf, desc, rec, env, want = capture_case(capture, envname)
    assert len(want) == n_replies
    outcome, od, src, got, info = R.respond_batch(buf, desc, rec, env)
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, (k, g.hex(), w.hex())
    assert int(info[0]) == n_replies
    if capture == "arp4.json":
        assert all(len(r) == 50 for r in got) and (desc["len"][src] == 60).all()
    if capture == "icmpv6_2.json":  # the hop-by-hop header is stripped
        assert all(len(r) == 80 for r in got) and (desc["len"][src] == 88).all()


def mixed_case(n, seed=7):
    import pyoracle
    fr, vp = R.mixed_batch(n, seed)
    o = pyoracle.Oracle()
    env = R.Env()
    R.load_tables(o, env)
    buf, desc = R.pack_with_holes(fr, vp)
    rec, _, _, _ = o.rx_batch(buf, desc)
    return buf, desc, rec, env


def test_mixed_batch_covers_every_outcome(oracle_built):
    """A condition on the inputs: a comparison against respond_ref cannot pass on an empty set."""
    buf, desc, rec, env = mixed_case(257)
    outcome, od, src, replies, info = R.respond_batch(buf, desc, rec, env)
    for k in range(6):
        assert (outcome == k).any(), k
    assert 4 * len(replies) >= len(desc)
    for k in (abi.RSP_ARP, abi.RSP_ICMP, abi.RSP_ICMPV6):
        assert (outcome == k).sum() >= 8
    # the shapes the emit pass has to get right: every tag count of an ARP reply, stripped
    # extension headers of 8, 16 and 24 bytes, a 9216 B and an IHL 6 echo, holes
    assert {len(r) for r, s in zip(replies, src) if outcome[s] == abi.RSP_ARP} == {42, 46, 50}
    strips = {int(desc["len"][s]) - len(r) for r, s in zip(replies, src) if outcome[s] == abi.RSP_ICMPV6}
    assert strips == {0, 8, 16, 24}
    assert max(len(r) for r in replies) == abi.MAX_FRAME
    assert any(outcome[i] == abi.RSP_ICMP and rec[i]["l4"] - rec[i]["l3"] == 24 for i in range(len(desc)))
    # holes over frames that would otherwise be answered (the oracle parses the bytes regardless)
    holes = np.nonzero(desc["pad"] == abi.DESC_HOLE)[0]
    assert len(holes) and (outcome[holes] == abi.RSP_NONE).all()
    assert any(R.respond_ref(bytes(buf[desc["off"][i]:desc["off"][i] + desc["len"][i]]), rec[i], env)[1] for i in holes)
    assert int(info[1]) == sum(R.align16(len(r)) for r in replies)
    # with a buffer one row short the last reply alone is refused
    o2, _, _, r2, i2 = R.respond_batch(buf, desc, rec, env, out_cap=int(info[1]) - 16)
    assert len(r2) == len(replies) - 1 and (o2 == abi.RSP_NOSPC).sum() == 1 and i2[1] == info[1]


def test_update_inet_checksum_is_incremental():
    """UpdateInetChecksum of a valid checksum equals the checksum recomputed over the rewritten bytes."""
    rng = np.random.default_rng(3)
    for _ in range(200):
        body = rng.integers(0, 256, int(rng.integers(0, 40)) * 2, dtype=np.uint8).tobytes()
        req = F.icmp4(8, 0, 1, 2, body)
        cs = struct.unpack(">H", req[2:4])[0]
        rep = F.icmp4(0, 0, 1, 2, body)
        new = R.update_inet_checksum(cs, 0x0800, 0x0000)
        # one's complement: 0x0000 and 0xffff are the same sum
        assert new == struct.unpack(">H", rep[2:4])[0] or {new, struct.unpack(">H", rep[2:4])[0]} == {0, 0xFFFF}


# ---- the C-ABI's argument checks (host-only handle: no device is touched) -----------------
@pytest.fixture()
def host_handle(lib):
    cfg = abi.Cfg(-1, 16, 16, 1 << 10, 1 << 16)
    h = C.c_void_p()
    assert lib.emurx_open(C.byref(cfg), C.byref(h)) == 0
    yield lib, h
    lib.emurx_close(h)


def test_respond_abi_constants():
    assert (abi.RSP_NONE, abi.RSP_ARP, abi.RSP_ICMP, abi.RSP_ICMPV6, abi.RSP_DROP_MCAST, abi.RSP_HOST,
            abi.RSP_NOSPC) == (0, 1, 2, 3, 4, 5, 6)
    assert any(s[0] == "emurx_respond_dev" for s in abi.SIGNATURES)


def test_respond_argument_checks(host_handle):
    lib, h = host_handle
    assert hasattr(lib, "emurx_respond_dev")
    EINVAL, EDEVICE = -22, -5
    # stand-ins for device pointers: the checks come before anything is dereferenced
    a = 0x10000

    def call(frames=a, desc=a, rec=a, n=4, out=a, cap=1024, odesc=a, osrc=a, outcome=a, info=a, handle=h):
        return lib.emurx_respond_dev(handle, frames, desc, rec, n, out, cap, odesc, osrc, outcome, info, None)

    for kw in (dict(handle=None), dict(frames=None), dict(desc=None), dict(rec=None), dict(out=None),
               dict(odesc=None), dict(osrc=None), dict(info=None), dict(info=None, n=0)):
        assert call(**kw) == EINVAL, kw
    assert call(out=a + 8) == EINVAL                       # d_out is written in 16-byte rows
    assert call(n=abi.TX_ZMQ_MAX_FRAMES) == EINVAL
    assert call(n=abi.TX_ZMQ_MAX_FRAMES - 1) == EDEVICE    # the largest n passes the checks
    # valid arguments reach the handle: a host-only one has no device
    assert call() == EDEVICE
    assert call(outcome=None) == EDEVICE                   # d_outcome is optional
    assert call(out=None, cap=0) == EDEVICE                # no buffer: the sizing call
    # n == 0 is valid (no array is required but d_info, which gets zeros on a device handle)
    assert call(frames=None, desc=None, rec=None, n=0, out=None, cap=0, odesc=None, osrc=None, outcome=None) == EDEVICE

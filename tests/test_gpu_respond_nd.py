"""GPU parity of emurx_respond_kinds_dev against nd_ref / respond_ref, and through them against the
reference's captures: outcome, descriptors, source indices, reply bytes and d_info bit-exact;
nothing written outside the replies' rows or past out_cap.  Records come from emurx_classify_dev
on the same handle."""
import numpy as np
import pytest

import nd_ref as N
import respond_ref as R
import sim_envs as S
from emurx import abi, frames as F
from test_gpu_respond import SENTINEL, check, classify
from test_nd_ref import CAPTURES, capture_case, capture_replies

pytestmark = pytest.mark.gpu

GUARD = 4  # words behind d_info that must stay untouched


def respond(rx, tb, td, trec, n, cap, kinds, tail=4096):
    """One call into sentinel-filled buffers -> dict of numpy outputs.  kinds None: emurx_respond_dev
    (eight info words), else emurx_respond_kinds_dev; GUARD words follow d_info."""
    import torch
    words = 8 if kinds is None else abi.RSP_INFO_WORDS
    out = torch.full((cap + tail,), SENTINEL, dtype=torch.uint8, device="cuda")
    od = torch.full((max(n, 1) * 8,), SENTINEL, dtype=torch.uint8, device="cuda")
    src = torch.full((max(n, 1),), -1, dtype=torch.int32, device="cuda")
    oc = torch.full((max(n, 1),), SENTINEL, dtype=torch.uint8, device="cuda")
    info = torch.full((words + GUARD,), -1, dtype=torch.int64, device="cuda")
    rx.respond_dev(tb, td, trec, n, out, cap, od, src, oc, info, kinds=kinds)
    torch.cuda.synchronize()
    iw = info.cpu().numpy().view(np.uint64)
    assert (iw[words:] == 0xFFFFFFFFFFFFFFFF).all(), iw  # nothing behind the info words
    return dict(out=out.cpu().numpy(), desc=od.cpu().numpy()[: n * 8].view(abi.DESC_DTYPE),
                src=src.cpu().numpy().view(np.uint32)[:n], outcome=oc.cpu().numpy()[:n], info=iw[:words], tout=out, tdesc=od)


@pytest.fixture(scope="module")
def combined(gpu_ok, oracle_built):
    """The combined batch's handle and its largest classified batch; smaller n are prefixes."""
    from emurx.rx import RxPath
    rx = RxPath(0, max_ns=16, max_clients=64, max_frames=1 << 12)
    rx.register_all()
    env4, env6 = R.Env(), N.Env()
    N.load_combined(rx, env4, env6)
    fr, vp = N.combined_batch(1025)
    buf, desc = R.pack_with_holes(fr, vp)
    tb, td, trec, rec = classify(rx, buf, desc)
    yield dict(rx=rx, env4=env4, env6=env6, buf=buf, desc=desc, tb=tb, td=td, trec=trec, rec=rec)
    rx.close()


def want_of(m, n, kinds, cap=None, words=None):
    return N.respond_batch(m["buf"], m["desc"][:n], m["rec"][:n], kinds, m["env4"], m["env6"], out_cap=cap, info_words=words)


@pytest.mark.parametrize("capture,n_replies,form", CAPTURES, ids=[c[0] for c in CAPTURES])
def test_nd_captures(gpu_ok, oracle_built, capture, n_replies, form):
    from emurx.rx import RxPath
    buf, desc, orec, env, tx = capture_case(capture)
    rx = RxPath(0, max_ns=16, max_clients=16, max_frames=1 << 10)
    rx.register_all()
    S.load_env(rx, "ipv6")
    tb, td, trec, rec = classify(rx, buf, desc)
    assert rec.tobytes() == orec.tobytes()
    want = N.respond_batch(buf, desc, rec, abi.RSPK_ND, env6=env)
    assert len(want[3]) == n_replies and capture_replies(tx, want[3]) == want[3]  # nd_ref = the capture
    cap = int(want[4][1])
    check(respond(rx, tb, td, trec, len(desc), cap, abi.RSPK_ND), want, len(desc), cap)
    rx.close()


@pytest.mark.parametrize("n", [1, 64, 65, 255, 256, 257, 1025])
def test_nd_combined(combined, n):
    m = combined
    want = want_of(m, n, abi.RSPK_ALL)
    if n >= 255:
        assert all((want[0] == k).any() for k in (0, 1, 2, 3, 4, 5, 7)) and 4 * len(want[3]) >= n
    cap = int(want[4][1])
    check(respond(m["rx"], m["tb"], m["td"], m["trec"], n, cap, abi.RSPK_ALL), want, n, cap)


def test_nd_full_tile_then_jumbo_echo(gpu_ok, oracle_built):
    """A tile of 256 solicitations, all answered (1536 rows written by their own lanes), then a tile
    that holds one 9216 B echo (576 rows dealt over the lanes)."""
    from emurx.rx import RxPath
    rx = RxPath(0, max_ns=16, max_clients=64, max_frames=1 << 10)
    rx.register_all()
    env4, env6 = R.Env(), N.Env()
    N.load_combined(rx, env4, env6)
    fr, vp = N.answered_batch(256)
    jumbo = R.mixed_batch(14)[0][13]
    assert len(jumbo) == abi.MAX_FRAME
    buf, desc = F.pack_frames(fr + [jumbo], vp + [1])
    tb, td, trec, rec = classify(rx, buf, desc)
    want = N.respond_batch(buf, desc, rec, abi.RSPK_ALL, env4, env6)
    assert (want[0][:256] == abi.RSP_ND).all() and want[0][256] == abi.RSP_ICMP
    assert int(want[4][1]) == 256 * 96 + abi.MAX_FRAME
    cap = int(want[4][1])
    check(respond(rx, tb, td, trec, 257, cap, abi.RSPK_ALL), want, 257, cap)
    rx.close()


def test_nd_alone(combined):
    m, n = combined, 600
    want = want_of(m, n, abi.RSPK_ND)
    assert set(np.unique(want[0])) == {abi.RSP_NONE, abi.RSP_HOST, abi.RSP_ND} and len(want[3]) > 60
    cap = int(want[4][1])
    check(respond(m["rx"], m["tb"], m["td"], m["trec"], n, cap, abi.RSPK_ND), want, n, cap)


def test_kinds_7_is_respond_dev(combined):
    """kinds = ARP | ICMP | ICMPV6 and emurx_respond_dev give the same outputs word for word; the
    eight-word form leaves a guard behind d_info[7] untouched (respond() checks it)."""
    m, n = combined, 600
    want = want_of(m, n, 7)
    assert abi.RSP_ND not in want[0] and len(want[3]) > 60 and int(want[4][8]) == 0
    cap = int(want[4][1])
    got = respond(m["rx"], m["tb"], m["td"], m["trec"], n, cap, 7)
    old = respond(m["rx"], m["tb"], m["td"], m["trec"], n, cap, None)
    check(got, want, n, cap)
    check(old, want_of(m, n, 7, words=8), n, cap)
    assert len(old["info"]) == 8 and np.array_equal(got["info"][:8], old["info"]) and (got["info"][8:] == 0).all()
    for k in ("out", "desc", "src", "outcome"):
        assert np.array_equal(got[k], old[k]), k


@pytest.mark.parametrize("short", [0, 16, None], ids=["exact", "minus16", "zero"])
def test_nd_capacity(combined, short):
    m, n = combined, 700
    full = want_of(m, n, abi.RSPK_ALL)
    need = int(full[4][1])
    cap = 0 if short is None else need - short
    want = want_of(m, n, abi.RSPK_ALL, cap=cap)
    assert int(want[4][1]) == need  # d_info[1] does not depend on the capacity
    assert int((want[0] == abi.RSP_NOSPC).sum()) == {0: 0, 16: 1, None: len(full[3])}[short]
    check(respond(m["rx"], m["tb"], m["td"], m["trec"], n, cap, abi.RSPK_ALL), want, n, cap)


def test_nd_capacity_last_reply_is_nd(gpu_ok, oracle_built):
    """A buffer 16 bytes short of a batch that ends in an advertisement: that reply is NOSPC and
    nothing is written behind the replies before it."""
    from emurx.rx import RxPath
    rx = RxPath(0, max_ns=16, max_clients=64, max_frames=1 << 10)
    rx.register_all()
    env6 = N.Env()
    N.load_tables(rx, env6)
    fr, vp = N.answered_batch(70)
    buf, desc = F.pack_frames(fr, vp)
    tb, td, trec, rec = classify(rx, buf, desc)
    cap = 70 * 96 - 16
    want = N.respond_batch(buf, desc, rec, abi.RSPK_ND, env6=env6, out_cap=cap)
    assert want[0][69] == abi.RSP_NOSPC and len(want[3]) == 69
    check(respond(rx, tb, td, trec, 70, cap, abi.RSPK_ND), want, 70, cap)
    rx.close()


def test_nd_client_removed_before_respond(gpu_ok, oracle_built):
    """Tables changed between classify and respond: the targets' client is gone, so its
    solicitations get NONE, no reply, nothing written."""
    from emurx.rx import RxPath
    rx = RxPath(0, max_ns=16, max_clients=64, max_frames=1 << 10)
    rx.register_all()
    env6 = N.Env()
    N.load_tables(rx, env6)
    fr, vp, labels = N.nd_batch(300)
    buf, desc = F.pack_frames(fr, vp)
    tb, td, trec, rec = classify(rx, buf, desc)
    before = N.respond_batch(buf, desc, rec, abi.RSPK_ND, env6=env6)
    # client 1 of every Namespace leaves: EUI-64 targets (MAC table) and plain ones (IPv6 table)
    for ns in range(len(N._NS)):
        cid = N.CID_BASE + ns * N.N_CLIENTS + 1
        assert rx.client_remove(N.NS_BASE + ns, env6.clients[cid]["mac"]) == 0
        env6.remove(cid)
    rx.sync()
    want = N.respond_batch(buf, desc, rec, abi.RSPK_ND, env6=env6)
    gone = np.nonzero((before[0] == abi.RSP_ND) & (want[0] == abi.RSP_NONE))[0]
    assert len(gone) >= 20 and {"ll-eui dad", "ip6 dad dhcpv6", "no-slla unicast"} <= {labels[i] for i in gone}
    assert (want[0] == abi.RSP_ND).sum() >= 20 and not set(gone) & set(want[2])
    cap = int(want[4][1])
    check(respond(rx, tb, td, trec, len(desc), cap, abi.RSPK_ND), want, len(desc), cap)
    rx.close()


def test_nd_then_tx_zmq(combined):
    """The responder's output is emurx_tx_zmq_dev's input: the messages equal the oracle's
    VethIFZmq.Send / FlushTx packing of the reference replies."""
    import pyoracle
    import torch
    m, n = combined, 1000
    want = want_of(m, n, abi.RSPK_ALL)
    cap = int(want[4][1])
    got = respond(m["rx"], m["tb"], m["td"], m["trec"], n, cap, abi.RSPK_ALL)
    k = int(got["info"][0])
    assert k == len(want[3]) > 250 and int(got["info"][1 + abi.RSP_ND]) > 100
    rbuf, rdesc = F.pack_frames(want[3], [int(v) for v in want[1]["vport"]], header=0)
    wmsg, woff, wtotal = pyoracle.tx_zmq(rbuf, rdesc)
    zcap = 8 * k + int(rdesc["len"].astype(np.int64).sum())
    zout = torch.full((zcap + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    zoff = torch.full((k + 1,), -1, dtype=torch.int64, device="cuda")
    zinfo = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    m["rx"].tx_zmq_dev(got["tout"], got["tdesc"], k, zout, zcap, zoff, zinfo)
    torch.cuda.synchronize()
    nm, total = (int(x) for x in zinfo.cpu().numpy())
    assert total == wtotal and nm == len(woff) - 1
    assert np.array_equal(zoff.cpu().numpy()[: nm + 1].astype(np.uint64), woff)
    assert zout.cpu().numpy()[:total].tobytes() == wmsg.tobytes()

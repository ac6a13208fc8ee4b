"""GPU parity of the device responder (emurx_respond_dev) against respond_ref, and through it
against the reference's captures: outcome, descriptors, source indices, reply bytes and d_info
bit-exact; nothing written outside the replies' rows or past out_cap.  Records come from
emurx_classify_dev on the same handle."""
import numpy as np
import pytest

import respond_ref as R
import sim_envs as S
from emurx import abi, frames as F
from test_respond_ref import CAPTURES, capture_case, capture_replies

pytestmark = pytest.mark.gpu

SENTINEL = 0xEE


def classify(rx, buf, desc):
    """-> device frames, descriptors, records (torch) and the records as numpy"""
    import torch
    from gpu_util import to_dev
    n = len(desc)
    tb, td = to_dev(buf), to_dev(desc)
    rec = torch.zeros(max(n, 1) * 32, dtype=torch.uint8, device="cuda")
    hist = torch.zeros(abi.HIST_SHARDS * 2 * abi.HIST_BINS, dtype=torch.int64, device="cuda")
    rx.classify_dev(tb, td, n, rec, None, 0, None, hist)
    torch.cuda.synchronize()
    return tb, td, rec, rec.cpu().numpy()[: n * 32].view(abi.REC_DTYPE)


def respond(rx, tb, td, trec, n, cap, outcome=True, tail=4096):
    """One emurx_respond_dev call into sentinel-filled buffers -> dict of numpy outputs."""
    import torch
    out = torch.full((cap + tail,), SENTINEL, dtype=torch.uint8, device="cuda")
    od = torch.full((max(n, 1) * 8,), SENTINEL, dtype=torch.uint8, device="cuda")
    src = torch.full((max(n, 1),), -1, dtype=torch.int32, device="cuda")
    oc = torch.full((max(n, 1),), SENTINEL, dtype=torch.uint8, device="cuda") if outcome else None
    info = torch.full((8,), -1, dtype=torch.int64, device="cuda")
    rx.respond_dev(tb, td, trec, n, out, cap, od, src, oc, info)
    torch.cuda.synchronize()
    return dict(out=out.cpu().numpy(), desc=od.cpu().numpy()[: n * 8].view(abi.DESC_DTYPE),
                src=src.cpu().numpy().view(np.uint32)[:n], outcome=None if oc is None else oc.cpu().numpy()[:n],
                info=info.cpu().numpy().view(np.uint64), tout=out, tdesc=od)


def check(got, want, n, cap):
    """got: respond(); want: respond_batch() for the same cap."""
    w_outcome, w_desc, w_src, w_replies, w_info = want
    k = len(w_replies)
    assert np.array_equal(got["info"], w_info), (got["info"], w_info)
    if got["outcome"] is not None:
        assert np.array_equal(got["outcome"], w_outcome), np.nonzero(got["outcome"] != w_outcome)[0][:10]
    assert got["desc"][:k].tobytes() == w_desc.tobytes()
    assert np.array_equal(got["src"][:k], w_src)
    # entries past the replies written are untouched
    assert (got["desc"][k:].view(np.uint8) == SENTINEL).all() and (got["src"][k:] == 0xFFFFFFFF).all()
    out = got["out"]
    end = 0
    for j, r in enumerate(w_replies):
        off = int(w_desc["off"][j])
        assert off == end and off % 16 == 0
        assert out[off:off + len(r)].tobytes() == r, (j, int(w_src[j]), len(r))
        end = off + R.align16(len(r))
    assert end <= cap
    assert (out[end:] == SENTINEL).all(), np.nonzero(out[end:] != SENTINEL)[0][:10] + end


@pytest.fixture(scope="module")
def mixed(gpu_ok, oracle_built):
    """The mixed batch's handle and its largest classified batch; smaller n are prefixes."""
    from emurx.rx import RxPath
    rx = RxPath(0, max_ns=16, max_clients=64, max_frames=1 << 13)
    rx.register_all()
    env = R.Env()
    R.load_tables(rx, env)
    fr, vp = R.mixed_batch(4099)
    buf, desc = R.pack_with_holes(fr, vp)
    tb, td, trec, rec = classify(rx, buf, desc)
    yield dict(rx=rx, env=env, buf=buf, desc=desc, tb=tb, td=td, trec=trec, rec=rec)
    rx.close()


@pytest.mark.parametrize("capture,envname,n_replies", CAPTURES, ids=[c[0] for c in CAPTURES])
def test_respond_captures(gpu_ok, oracle_built, capture, envname, n_replies):
    from emurx.rx import RxPath
    buf, desc, orec, env, replies = capture_case(capture, envname)
    rx = RxPath(0, max_ns=16, max_clients=16, max_frames=1 << 10)
    rx.register_all()
    S.load_env(rx, envname)
    tb, td, trec, rec = classify(rx, buf, desc)
    assert rec.tobytes() == orec.tobytes()
    want = R.respond_batch(buf, desc, rec, env)
    assert want[3] == replies and len(replies) == n_replies  # respond_ref = the capture
    cap = int(want[4][1])
    check(respond(rx, tb, td, trec, len(desc), cap), want, len(desc), cap)
    rx.close()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 4099])
def test_respond_mixed(mixed, n):
    m = mixed
    want = R.respond_batch(m["buf"], m["desc"][:n], m["rec"][:n], m["env"])
    if n >= 255:
        assert 4 * len(want[3]) >= n and all((want[0] == k).any() for k in range(6))
    cap = int(want[4][1])
    check(respond(m["rx"], m["tb"], m["td"], m["trec"], n, cap), want, n, cap)


def test_respond_without_outcome_array(mixed):
    m, n = mixed, 300
    want = R.respond_batch(m["buf"], m["desc"][:n], m["rec"][:n], m["env"])
    cap = int(want[4][1])
    check(respond(m["rx"], m["tb"], m["td"], m["trec"], n, cap, outcome=False), want, n, cap)


@pytest.mark.parametrize("short", [0, 16, None], ids=["exact", "minus16", "zero"])
def test_respond_capacity(mixed, short):
    m, n = mixed, 700
    need = int(R.respond_batch(m["buf"], m["desc"][:n], m["rec"][:n], m["env"])[4][1])
    cap = 0 if short is None else need - short
    want = R.respond_batch(m["buf"], m["desc"][:n], m["rec"][:n], m["env"], out_cap=cap)
    assert int(want[4][1]) == need  # d_info[1] does not depend on the capacity
    nospc = int((want[0] == abi.RSP_NOSPC).sum())
    assert nospc == {0: 0, 16: 1, None: len(R.respond_batch(m["buf"], m["desc"][:n], m["rec"][:n], m["env"])[3])}[short]
    check(respond(m["rx"], m["tb"], m["td"], m["trec"], n, cap), want, n, cap)


def test_respond_capacity_mid_batch(mixed):
    """A capacity that ends inside the batch: the prefix that fits, NOSPC on every later reply."""
    m, n = mixed, 700
    need = int(R.respond_batch(m["buf"], m["desc"][:n], m["rec"][:n], m["env"])[4][1])
    cap = (need // 3) & ~15
    want = R.respond_batch(m["buf"], m["desc"][:n], m["rec"][:n], m["env"], out_cap=cap)
    assert 0 < len(want[3]) and (want[0] == abi.RSP_NOSPC).sum() > 100
    check(respond(m["rx"], m["tb"], m["td"], m["trec"], n, cap), want, n, cap)


def test_respond_arp_client_not_in_tables(gpu_ok, oracle_built):
    """Classified on handle A, answered on handle B whose tables lost the client: RSP_HOST."""
    from emurx.rx import RxPath
    a = RxPath(0, max_ns=16, max_clients=64, max_frames=1 << 10)
    b = RxPath(0, max_ns=16, max_clients=64, max_frames=1 << 10)
    env = R.Env()
    for h in (a, b):
        h.register_all()
        R.load_tables(h, env if h is a else None)
    fr, vp = R.mixed_batch(120)
    buf, desc = F.pack_frames(fr, vp)
    tb, td, trec, rec = classify(a, buf, desc)
    arps = [i for i in range(len(fr)) if R.respond_ref(fr[i], rec[i], env)[0] == abi.RSP_ARP]
    assert len(arps) >= 4
    i0 = arps[0]  # the client this request asks for leaves B
    ns, tpa = int(rec[i0]["ns_id"]), fr[i0][rec[i0]["l3"] + 24:rec[i0]["l3"] + 28]
    cid, mac = env.ip4[(1, int(rec[i0]["vlan0"]), int(rec[i0]["vlan1"]), tpa)]
    assert b.client_remove(ns, mac) == 0
    b.sync()
    env.remove(F.tunnel_key(1, int(rec[i0]["vlan0"]), int(rec[i0]["vlan1"])), tpa)
    want = R.respond_batch(buf, desc, rec, env)
    assert want[0][i0] == abi.RSP_HOST and i0 not in want[2] and (want[0] == abi.RSP_ARP).any()
    cap = int(want[4][1])
    check(respond(b, tb, td, trec, len(desc), cap), want, len(desc), cap)
    a.close()
    b.close()


def test_respond_then_tx_zmq(mixed):
    """The responder's output is emurx_tx_zmq_dev's input: the messages equal the oracle's
    VethIFZmq.Send / FlushTx packing of respond_ref's replies."""
    import pyoracle
    import torch
    m, n = mixed, 1000
    want = R.respond_batch(m["buf"], m["desc"][:n], m["rec"][:n], m["env"])
    cap = int(want[4][1])
    got = respond(m["rx"], m["tb"], m["td"], m["trec"], n, cap)
    k = int(got["info"][0])
    assert k == len(want[3]) > 250
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


def test_respond_no_responders(gpu_ok, oracle_built):
    """65,536 config-B frames, all UDP: no reply, every outcome NONE, nothing written."""
    from emurx import synth
    from emurx.rx import RxPath
    n = 1 << 16
    w = synth.config_b(n)
    rx = RxPath(0, max_ns=16, max_clients=16, max_frames=n)
    rx.register_all()
    synth.load_tables(w, rx)
    tb, td, trec, rec = classify(rx, w["buf"], w["desc"])
    assert (rec["proto"] == abi.CB_NAMES.index("udp")).all()
    got = respond(rx, tb, td, trec, n, 1 << 16)
    assert (got["info"] == 0).all() and (got["outcome"] == abi.RSP_NONE).all()
    assert (got["out"] == SENTINEL).all() and (got["src"] == 0xFFFFFFFF).all()
    rx.close()

"""GPU parity of emurx_nsstat_ts_dev against ts_ref's refinement of nsstat_ref, and through it against
the counters the reference's timestamp simulation recorded: d_ev[:info[0]], d_done and d_info
bit-exact, nothing written around them.  Records and outcomes come from emurx_classify_dev,
emurx_respond_ts_dev and emurx_learn_dev on the same handle."""
import json
from pathlib import Path

import numpy as np
import pytest

import learn_ref as L
import nd_ref as N
import nsstat_ref as NS
import respond_ref as R
import sim_envs as S
import ts_ref as T
from emurx import abi, frames as F
from test_gpu_nsstat import EV, GUARD, check, finish
from test_gpu_respond import SENTINEL, classify

pytestmark = pytest.mark.gpu

COUNTERS = json.loads((Path(__file__).parent / "golden" / "icmp2_counters.json").read_text())
ALL = abi.RSPK_ALL_TS
TIME = 43_200_123


def prepare(rx, buf, desc, kinds=ALL):
    """classify, respond (emurx_respond_ts_dev) and learn on the device -> the batch's device arrays
    and their numpy copies"""
    import torch
    n = len(desc)
    tb, td, trec, rec = classify(rx, buf, desc)
    cap = int(sum((int(x) + 15) & ~15 for x in desc["len"])) + 96 * n + 64
    out = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    od = torch.zeros(max(n, 1) * 8, dtype=torch.uint8, device="cuda")
    src = torch.zeros(max(n, 1), dtype=torch.int32, device="cuda")
    rsp = torch.zeros(max(n, 1), dtype=torch.uint8, device="cuda")
    rinfo = torch.zeros(abi.RSP_INFO_WORDS, dtype=torch.int64, device="cuda")
    rx.respond_dev(tb, td, trec, n, out, cap, od, src, rsp, rinfo, kinds=kinds, ip_time=TIME)
    lcap = rx.learn_max_events()
    lev = torch.zeros(lcap * 40, dtype=torch.uint8, device="cuda")
    lrn = torch.zeros(max(n, 1), dtype=torch.uint8, device="cuda")
    linfo = torch.zeros(abi.LRN_INFO_WORDS, dtype=torch.int64, device="cuda")
    rx.learn_dev(tb, td, trec, n, lev, lcap, lrn, linfo, kinds=abi.LRNK_ALL)
    torch.cuda.synchronize()
    assert int(linfo[2]) == 0 and int(rinfo[1 + abi.RSP_NOSPC]) == 0
    return dict(rx=rx, buf=buf, desc=desc, n=n, tb=tb, td=td, trec=trec, rec=rec, t_rsp=rsp, t_lrn=lrn,
                rsp=rsp.cpu().numpy()[:n], lrn=lrn.cpu().numpy()[:n], ref={})


def nsstat(m, n, ev_cap, kinds=ALL, ts=True):
    """One emurx_nsstat_ts_dev (ts False: emurx_nsstat_dev) call into sentinel-filled buffers."""
    import torch
    rx = m["rx"]
    ev = torch.full((GUARD + ev_cap * EV + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    dn = torch.full((max(n, 1) + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    info = torch.full((abi.NSS_INFO_WORDS + 4,), -1, dtype=torch.int64, device="cuda")
    fn = rx.lib.emurx_nsstat_ts_dev if ts else rx.lib.emurx_nsstat_dev
    rc = fn(rx.h, m["tb"].data_ptr(), m["td"].data_ptr(), m["trec"].data_ptr(), n, kinds, m["t_rsp"].data_ptr(),
            m["t_lrn"].data_ptr(), ev[GUARD:].data_ptr(), ev_cap, dn.data_ptr(), info.data_ptr(), None)
    assert rc == 0, rc
    return finish(dict(ev=ev, dn=dn, info=info, n=n))


def want_prefix(m, n, kinds=ALL, ev_cap=None, max_ns=None):
    if kinds not in m["ref"]:
        m["ref"][kinds] = T.nsstat_frames(m["buf"], m["desc"], m["rec"], kinds, m["rsp"], m["lrn"], max_ns)
    done, cnts, cand = m["ref"][kinds]
    ev, info = NS.fold(m["rec"]["ns_id"][:n], done[:n], cnts[:n], cand[:n], ev_cap)
    return done[:n], ev, info


def test_nsstat_ts_six_requests(gpu_ok, oracle_built):
    from emurx.rx import RxPath
    rx = RxPath(0, max_ns=16, max_clients=16, max_frames=1 << 10)
    rx.register_all()
    S.load_env(rx, "icmp")
    fr = T.six_requests()
    buf, desc = F.pack_frames(fr, [1] * 6)
    m = prepare(rx, buf, desc)
    assert (m["rsp"] == abi.RSP_TS).all()
    want = want_prefix(m, 6)
    assert (want[0] == 1).all() and len(want[1]) == 1 and int(want[1][0]["frames"]) == 6
    got = nsstat(m, 6, 16)
    check(got, want)
    ev = got["ev"][:EV].view(abi.NSSTAT_EV_DTYPE)
    assert {name: v for (ns, plug, name), v in NS.replay(ev).items()} == COUNTERS
    rx.close()


@pytest.fixture(scope="module")
def mixed(gpu_ok, oracle_built):
    """nsstat_ref.mixed_batch (it holds respond_ref's timestamp requests), 4,096 frames with holes,
    answered with every kind and the timestamp reply."""
    from emurx.rx import RxPath
    rx = RxPath(0, max_ns=16, max_clients=64, max_frames=1 << 12)
    rx.register_all()
    N.load_combined(rx, R.Env(), N.Env())
    fr, vp = NS.mixed_batch(4096)
    buf, desc = R.pack_with_holes(fr, vp, L.HOLE_EVERY)
    m = prepare(rx, buf, desc)
    yield m
    rx.close()


@pytest.mark.parametrize("kinds", [k for k in range(17, 32) if k & abi.RSPK_ICMP])
def test_nsstat_ts_kinds(mixed, kinds):
    want = want_prefix(mixed, 4096, kinds)
    ts = (mixed["rsp"] == abi.RSP_TS)
    assert ts.sum() >= 50 and (want[0][ts] == 1).all()  # every answered timestamp request is done
    old = NS.nsstat_frames(mixed["buf"], mixed["desc"], mixed["rec"], kinds & 15, mixed["rsp"], mixed["lrn"])[0]
    assert not old[ts].any() and np.array_equal(old[~ts], want[0][~ts])
    check(nsstat(mixed, 4096, 16, kinds), want)


@pytest.mark.parametrize("n", [65, 255, 256, 257])
def test_nsstat_ts_prefixes(mixed, n):
    want = want_prefix(mixed, n)
    check(nsstat(mixed, n, max(len(want[1]), 1)), want)


def test_nsstat_ts_equals_nsstat_dev(mixed):
    """For kinds <= 15 the two entry points write the same bytes (the outcomes are those of a
    responder call with more kinds: the timestamp outcomes then count for nothing)."""
    for kinds in range(1, 16):
        a, b = nsstat(mixed, 4096, 16, kinds), nsstat(mixed, 4096, 16, kinds, ts=False)
        for k in ("ev", "done", "info"):
            assert np.array_equal(a[k], b[k]), (kinds, k)
        if kinds in (2, 15):
            check(a, want_prefix(mixed, 4096, kinds))


def test_nsstat_ts_drops_of_three_namespaces(mixed):
    """Too-short and multicast-source timestamp requests in three Namespaces: pktRxErrTooShort is a
    counter a frame bumps alone, so the events' `frames` include it."""
    group = bytes([1, 0, 0x5E, 0, 0, 7])
    fr, kind = [], []
    for i in range(330):
        ns, c = i % 3, i % R.N_CLIENTS
        k = (i // 3) % 5
        if k in (0, 1):
            fr.append(T.ts_frame(ns, c, span=8 + (i % 12), opts=i % 2, seq=i))
        elif k == 2:
            fr.append(T.ts_frame(ns, c, span=12 + (i % 20), esrc=group, seq=i))
        elif k == 3:
            fr.append(T.ts_frame(ns, c, span=20 + (i % 9), seq=i))
        else:
            fr.append(T.ts_frame(ns, c, span=19, src=bytes([224, 0, 0, 1]), seq=i))
        kind.append(k)
    buf, desc = F.pack_frames(fr, [1] * len(fr))
    m = prepare(mixed["rx"], buf, desc)
    kind = np.array(kind)
    assert (m["rsp"][kind <= 1] == abi.RSP_DROP_SHORT).all() and (m["rsp"][kind == 3] == abi.RSP_TS).all()
    assert (m["rsp"][(kind == 2) | (kind == 4)] == abi.RSP_DROP_MCAST).all()
    want = want_prefix(m, len(fr))
    assert (want[0] == 1).all() and len(want[1]) == 3
    for e in want[1]:
        c = e["cnt"]
        assert int(c[abi.NSC_ICMP_ERR_TOO_SHORT]) == 44 and int(c[abi.NSC_ICMP_ERR_MCAST]) == 44 and int(c[abi.NSC_ICMP_ECHO]) == 22
        assert int(e["frames"]) == 110 == int(c.sum())
    stats = T.replay(want[1])
    assert all(stats[(ns, "icmp", "pktRxErrTooShort")] == 44 and stats[(ns, "icmp", "pktTxIcmpResponse")] == 22 for ns in range(3))
    check(nsstat(m, len(fr), 3), want)
    # without the timestamp kind the two outcomes count for nothing: only the multicast drops are done
    want15 = want_prefix(m, len(fr), abi.RSPK_ALL)
    assert (want15[0] == 1).sum() == 132
    check(nsstat(m, len(fr), 3, abi.RSPK_ALL), want15)


def test_nsstat_ts_argument_checks(mixed):
    import torch
    m, rx = mixed, mixed["rx"]
    cap = rx.nsstat_max_events()
    ev = torch.full((cap * EV + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
    dn = torch.full((4096,), SENTINEL, dtype=torch.uint8, device="cuda")
    info = torch.full((abi.NSS_INFO_WORDS + 1,), -1, dtype=torch.int64, device="cuda")
    a = dict(frames=m["tb"], desc=m["td"], rec=m["trec"], n=64, rsp=m["t_rsp"], lrn=m["t_lrn"], ev=ev, ev_cap=cap, done=dn,
             info=info, kinds=ALL)

    def rc(**kw):
        p = dict(a, **kw)
        ad = lambda x: 0 if x is None else x if isinstance(x, int) else x.data_ptr()  # noqa: E731
        return rx.lib.emurx_nsstat_ts_dev(rx.h, ad(p["frames"]), ad(p["desc"]), ad(p["rec"]), p["n"], p["kinds"], ad(p["rsp"]),
                                          ad(p["lrn"]), ad(p["ev"]), p["ev_cap"], ad(p["done"]), ad(p["info"]), None)

    for kw in (dict(kinds=0), dict(kinds=32), dict(kinds=16), dict(kinds=16 | 13), dict(ev_cap=0), dict(ev_cap=cap + 1),
               dict(frames=None), dict(desc=None), dict(rec=None), dict(rsp=None), dict(lrn=None), dict(ev=None), dict(info=None),
               dict(rec=m["trec"].data_ptr() + 8), dict(desc=m["td"].data_ptr() + 4), dict(ev=ev.data_ptr() + 4),
               dict(info=info.data_ptr() + 4)):
        assert rc(**kw) == abi.EMURX_EINVAL, kw
    assert rc(n=4097) == abi.EMURX_ENOMEM
    torch.cuda.synchronize()
    assert (ev == SENTINEL).all() and (dn == SENTINEL).all() and (info == -1).all()  # none of them wrote anything
    assert rc(lrn=None, kinds=abi.RSPK_ICMP | abi.RSPK_TS) == 0  # without ARP and ND the learn outcomes are not read
    torch.cuda.synchronize()
    want = want_prefix(m, 64, abi.RSPK_ICMP | abi.RSPK_TS)
    assert np.array_equal(info.cpu().numpy().view(np.uint64)[: abi.NSS_INFO_WORDS], want[2]) and int(info[-1]) == -1
    assert np.array_equal(dn.cpu().numpy()[:64], want[0])

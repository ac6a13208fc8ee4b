"""GPU parity of emurx_nsstat_dev against nsstat_ref, and through it against the counters the
reference's captures recorded: d_ev[:info[0]], d_done and d_info bit-exact; nothing written before
d_ev, past the events written, behind d_done or behind d_info.  Records and outcomes come from
emurx_classify_dev, emurx_respond_kinds_dev and emurx_learn_dev on the same handle."""
import numpy as np
import pytest

import learn_ref as L
import nd_ref as N
import nsstat_ref as NS
import respond_ref as R
import sim_envs as S
from emurx import abi, frames as F
from test_gpu_respond import SENTINEL, classify
from test_nsstat_ref import CAPTURES, HAND, capture_case

pytestmark = pytest.mark.gpu

GUARD = 96  # bytes before and behind d_ev and behind d_done, and 4 words behind d_info, that must stay untouched
EV = 96


def prepare(rx, buf, desc, kinds=abi.RSPK_ALL):
    """classify, respond and learn on the device -> the batch's device arrays and their numpy copies"""
    import torch
    n = len(desc)
    tb, td, trec, rec = classify(rx, buf, desc)
    cap = int(sum((int(x) + 15) & ~15 for x in desc["len"])) + 64
    out = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    od = torch.zeros(max(n, 1) * 8, dtype=torch.uint8, device="cuda")
    src = torch.zeros(max(n, 1), dtype=torch.int32, device="cuda")
    rsp = torch.zeros(max(n, 1), dtype=torch.uint8, device="cuda")
    rinfo = torch.zeros(abi.RSP_INFO_WORDS, dtype=torch.int64, device="cuda")
    rx.respond_dev(tb, td, trec, n, out, cap, od, src, rsp, rinfo, kinds=kinds)
    lk = (abi.LRNK_ARP if kinds & abi.RSPK_ARP else 0) | (abi.LRNK_ND if kinds & abi.RSPK_ND else 0)
    lrn = None
    if lk:
        lcap = rx.learn_max_events()
        lev = torch.zeros(lcap * 40, dtype=torch.uint8, device="cuda")
        lrn = torch.zeros(max(n, 1), dtype=torch.uint8, device="cuda")
        linfo = torch.zeros(abi.LRN_INFO_WORDS, dtype=torch.int64, device="cuda")
        rx.learn_dev(tb, td, trec, n, lev, lcap, lrn, linfo, kinds=lk)
    torch.cuda.synchronize()
    if lk:
        assert int(linfo[2]) == 0  # the learn call did not overflow: its outcomes stand
    return dict(rx=rx, buf=buf, desc=desc, n=n, tb=tb, td=td, trec=trec, rec=rec, t_rsp=rsp, t_lrn=lrn,
                rsp=rsp.cpu().numpy()[:n], lrn=None if lrn is None else lrn.cpu().numpy()[:n])


def nsstat(m, n, ev_cap, kinds=abi.RSPK_ALL, done=True, sync=True):
    """One emurx_nsstat_dev call into sentinel-filled buffers -> dict (numpy after finish())."""
    import torch
    ev = torch.full((GUARD + ev_cap * EV + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    dn = torch.full((max(n, 1) + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda") if done else None
    info = torch.full((abi.NSS_INFO_WORDS + 4,), -1, dtype=torch.int64, device="cuda")
    m["rx"].nsstat_dev(m["tb"], m["td"], m["trec"], n, m["t_rsp"], m["t_lrn"], ev[GUARD:], ev_cap, dn, info, kinds=kinds)
    got = dict(ev=ev, dn=dn, info=info, n=n)
    return finish(got) if sync else got


def finish(got):
    import torch
    torch.cuda.synchronize()
    raw = got["ev"].cpu().numpy()
    iw = got["info"].cpu().numpy().view(np.uint64)
    assert (iw[abi.NSS_INFO_WORDS:] == 0xFFFFFFFFFFFFFFFF).all(), iw  # nothing behind d_info
    assert (raw[:GUARD] == SENTINEL).all() and (raw[-GUARD:] == SENTINEL).all()  # nothing before d_ev, nothing past ev_cap
    done = None
    if got["dn"] is not None:
        d = got["dn"].cpu().numpy()
        assert (d[got["n"]:] == SENTINEL).all()  # nothing behind d_done[n]
        done = d[: got["n"]]
    return dict(ev=raw[GUARD:-GUARD], done=done, info=iw[: abi.NSS_INFO_WORDS])


def check(got, want):
    """got: nsstat(); want: (done, events, info) of nsstat_ref for the same ev_cap."""
    w_done, w_ev, w_info = want
    assert np.array_equal(got["info"], w_info), (got["info"], w_info)
    if got["done"] is not None:
        assert np.array_equal(got["done"], w_done), np.nonzero(got["done"] != w_done)[0][:10]
    k = int(w_info[0])
    assert k == len(w_ev)
    g = got["ev"][: k * EV].view(abi.NSSTAT_EV_DTYPE)
    assert g.tobytes() == w_ev.tobytes(), next((j, g[j], w_ev[j]) for j in range(k) if g[j] != w_ev[j])
    assert (got["ev"][k * EV:] == SENTINEL).all()  # entries past the events written are untouched


def reference(m, kinds=abi.RSPK_ALL, max_ns=None):
    """The per-frame reference of the whole batch for `kinds`, computed once and kept."""
    ref = m.setdefault("ref", {})
    if kinds not in ref:
        ref[kinds] = NS.nsstat_frames(m["buf"], m["desc"], m["rec"], kinds, m["rsp"], m["lrn"], max_ns)
    return ref[kinds]


def want_prefix(m, n, kinds=abi.RSPK_ALL, ev_cap=None, max_ns=None):
    done, cnts, cand = reference(m, kinds, max_ns)
    ev, info = NS.fold(m["rec"]["ns_id"][:n], done[:n], cnts[:n], cand[:n], ev_cap)
    return done[:n], ev, info


# ---- the captures ----------------------------------------------------------------------------------
@pytest.mark.parametrize("capture,envname,n,words", CAPTURES, ids=[c[0] for c in CAPTURES])
def test_nsstat_captures(gpu_ok, oracle_built, capture, envname, n, words):
    from emurx.rx import RxPath
    buf, desc, orec, env4, env6 = capture_case(capture, envname)
    rx = RxPath(0, max_ns=16, max_clients=16, max_frames=1 << 10)
    rx.register_all()
    S.load_env(rx, envname)
    m = prepare(rx, buf, desc)
    assert m["rec"].tobytes() == orec.tobytes()
    want = want_prefix(m, n)
    # nsstat_ref on the device's outcomes = the capture's counters (test_nsstat_ref pins them)
    assert (want[0] == 1).all() and len(want[1]) == 1 and int(want[1][0]["frames"]) == n
    assert {k: int(v) for k, v in enumerate(want[1][0]["cnt"]) if v} == words
    check(nsstat(m, n, 16), want)
    rx.close()


# ---- the mixed batch ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed(gpu_ok, oracle_built):
    """nsstat_ref.mixed_batch: respond_ref's mixed batch and learn_ref's learning batch interleaved,
    4,096 frames with holes, classified, answered and learned once; smaller n are prefixes."""
    from emurx.rx import RxPath
    rx = RxPath(0, max_ns=16, max_clients=64, max_frames=1 << 12)
    rx.register_all()
    N.load_combined(rx, R.Env(), N.Env())
    fr, vp = NS.mixed_batch(4096)
    buf, desc = R.pack_with_holes(fr, vp, L.HOLE_EVERY)
    m = prepare(rx, buf, desc)
    yield m
    rx.close()


def test_nsstat_mixed_batch_reaches_the_rule(mixed):
    """A condition on the inputs: a comparison against nsstat_ref cannot pass on an empty set."""
    m = mixed
    done, cnts, cand = reference(m)
    assert all((done == k).sum() >= 16 for k in (0, 1, 2)) and (cand & (done == 0)).sum() >= 16
    assert {c for cs in cnts for c in cs} == set(range(19))  # every counter of the call
    ev, info = NS.fold(m["rec"]["ns_id"], done, cnts, cand)
    assert len(ev) >= 6 and (ev["frames"] > 1).all()
    assert set(m["rsp"]) >= {0, 1, 2, 3, 4, 5, 7} and set(m["lrn"]) == set(range(6))


@pytest.mark.parametrize("n", [63, 64, 65, 255, 256, 257, 4096])
def test_nsstat_mixed(mixed, n):
    want = want_prefix(mixed, n)
    assert int(want[2][3]) > 0
    check(nsstat(mixed, n, max(len(want[1]), 1)), want)


@pytest.mark.parametrize("kinds", list(range(1, 16)))
def test_nsstat_kinds(mixed, kinds):
    """Every subset of kinds, with the outcomes of the calls made with all of them."""
    want = want_prefix(mixed, 4096, kinds)
    assert int(want[2][3]) > 0
    check(nsstat(mixed, 4096, 16, kinds), want)


def test_nsstat_kinds_add_up(mixed):
    """A frame's decision depends on its own kind alone: per frame, done under all kinds is the
    one value that is not 0 among the single kinds (ICMPV6 and ND share the icmpv6 callback but
    never the same type); the counters add up."""
    alone = [want_prefix(mixed, 4096, k) for k in (1, 2, 4, 8)]
    both = want_prefix(mixed, 4096, 15)
    assert np.array_equal(np.maximum.reduce([a[0] for a in alone]), both[0])
    tot = np.zeros(abi.NSC_WORDS, np.uint64)
    for a in alone:
        tot += a[1]["cnt"].sum(axis=0).astype(np.uint64)
    assert np.array_equal(tot, both[1]["cnt"].sum(axis=0).astype(np.uint64))


def test_nsstat_without_done(mixed):
    want = want_prefix(mixed, 1000)
    got = nsstat(mixed, 1000, len(want[1]), done=False)
    assert got["done"] is None
    check(got, want)


def test_nsstat_twice_in_a_row(mixed):
    """The same call twice, no synchronisation between them: identical results (the accumulator
    rows are zero again when a call ends)."""
    want = want_prefix(mixed, 4096)
    g1 = nsstat(mixed, 4096, len(want[1]), sync=False)
    g2 = nsstat(mixed, 4096, len(want[1]), sync=False)
    g1, g2 = finish(g1), finish(g2)
    check(g1, want)
    check(g2, want)
    assert g1["ev"].tobytes() == g2["ev"].tobytes() and np.array_equal(g1["done"], g2["done"])


def test_nsstat_overflow_then_exact(mixed):
    """ev_cap equal to the distinct Namespaces: every event; one less: overflow, nothing written,
    the rest of d_info and d_done valid; the next call on the handle is exact again (the rows an
    overflowing call touched are zeroed all the same)."""
    full = want_prefix(mixed, 4096)
    k = len(full[1])
    assert k >= 2
    check(nsstat(mixed, 4096, k), full)
    over = want_prefix(mixed, 4096, ev_cap=k - 1)
    assert tuple(int(x) for x in over[2][:3]) == (0, k, 1) and np.array_equal(over[2][3:], full[2][3:])
    got = nsstat(mixed, 4096, k - 1)
    check(got, over)
    assert (got["ev"] == SENTINEL).all()
    check(nsstat(mixed, 4096, k), full)
    # and behind an overflowing call without a synchronisation in between
    g1 = nsstat(mixed, 4096, 1, sync=False)
    g2 = nsstat(mixed, 300, k, sync=False)
    check(finish(g1), want_prefix(mixed, 4096, ev_cap=1))
    check(finish(g2), want_prefix(mixed, 300))


def test_nsstat_no_counted_frame(mixed):
    """A batch with candidates but no frame with done 1 (the ND kind alone, with outcome arrays that
    say nothing was answered or learned): no event, the counts of d_info valid; the calls before and
    behind it on the handle are exact."""
    import torch
    n = 4096
    z = torch.zeros(n, dtype=torch.uint8, device="cuda")
    m0 = dict(mixed, t_rsp=z, t_lrn=z, rsp=np.zeros(n, np.uint8), lrn=np.zeros(n, np.uint8), ref={})
    want = want_prefix(m0, n, abi.RSPK_ND)
    assert tuple(int(x) for x in want[2][:4]) == (0, 0, 0, 0) and int(want[2][5]) > 100 and not (want[0] == 1).any()
    full = want_prefix(mixed, n)
    g1 = nsstat(mixed, n, len(full[1]), sync=False)
    g2 = nsstat(m0, n, 4, abi.RSPK_ND, sync=False)
    g3 = nsstat(mixed, n, len(full[1]), sync=False)
    check(finish(g1), full)
    got = finish(g2)
    check(got, want)
    assert (got["ev"] == SENTINEL).all()
    check(finish(g3), full)


def test_nsstat_n_zero(mixed):
    got = nsstat(mixed, 0, 4)
    assert (got["info"] == 0).all() and (got["ev"] == SENTINEL).all()


# ---- hand-built records: every branch of the rule ----------------------------------------------------
def test_nsstat_hand_built(mixed):
    """The hand-built frames, records and outcomes of test_nsstat_ref (records no classify writes
    among them), each also as a hole, on the device."""
    import torch
    from gpu_util import to_dev
    frames = [c[1] for c in HAND] * 2
    buf, desc = F.pack_frames(frames, [1] * len(frames))
    desc["pad"][len(HAND):] = abi.DESC_HOLE
    rec = np.array([c[2] for c in HAND] * 2, abi.REC_DTYPE)
    rsp = np.array([c[3] for c in HAND] * 2, np.uint8)
    lrn = np.array([c[4] for c in HAND] * 2, np.uint8)
    m = dict(rx=mixed["rx"], buf=buf, desc=desc, rec=rec, rsp=rsp, lrn=lrn, tb=to_dev(buf), td=to_dev(desc),
             trec=to_dev(rec.view(np.uint8)), t_rsp=to_dev(rsp), t_lrn=to_dev(lrn))
    torch.cuda.synchronize()
    want = want_prefix(m, len(frames), max_ns=16)
    assert [int(x) for x in want[0][: len(HAND)]] == [c[5] for c in HAND] and not want[0][len(HAND):].any()
    check(nsstat(m, len(frames), 4), want)
    # a handle whose max_ns the records' Namespace (3) is not below: no row, done 0
    from emurx.rx import RxPath
    rx3 = RxPath(0, max_ns=3, max_clients=16, max_frames=1 << 10)
    m3 = dict(m, rx=rx3, ref={})
    want3 = want_prefix(m3, len(frames), max_ns=3)
    assert not (want3[0] == 1).any() and (want3[0] == 2).sum() == (want[0] == 2).sum() and len(want3[1]) == 0
    check(nsstat(m3, len(frames), 3), want3)
    rx3.close()


# ---- one key, and all keys distinct -----------------------------------------------------------------
SCAN_ROUND = 8192  # rows per round of k_nss_scan
WIDE_NS = 3 * SCAN_ROUND + 100
WIDE_EDGES = (0, 255, 256, 8191, 8192, 8193, 16383, 16384, 24575, 24576, WIDE_NS - 1)


@pytest.fixture(scope="module")
def wide(gpu_ok, oracle_built):
    """A handle with max_ns = WIDE_NS and 1,024 Namespaces of one client each.  The scan of the row
    flags takes 8,192 rows a round (1,024 lanes x 8 flags): WIDE_NS makes it four rounds, the last
    one partial and no multiple of 8, and the ids lie in every round, on both sides of every round's
    edge (8191, 8192, 16383, 16384, 24575, 24576) and at 0, 255, 256 and WIDE_NS - 1."""
    from emurx.rx import RxPath
    rx = RxPath(0, max_ns=WIDE_NS, max_clients=2048, max_frames=1 << 12)
    rx.register_all()
    ids = list(WIDE_EDGES)
    ids += [j for j in range(1, WIDE_NS - 1) if j % 24 == 7 and j not in WIDE_EDGES][: 1024 - len(ids)]
    assert len(ids) == 1024 and len(set(ids)) == 1024
    rng = np.random.default_rng(11)
    rng.shuffle(ids)
    ids = [int(x) for x in ids]
    nss = []
    for k, ns in enumerate(ids):
        tags = ((0x8100, k + 1),)
        mac, ip4 = bytes([0, 0, 2, k >> 8, k & 0xFF, 1]), bytes([16, 1 + (k >> 8), k & 0xFF, 1])
        assert rx.ns_add(R._key(tags), ns, abi.PLUG_ALL) == 0
        assert rx.client_add(ns, k, mac, ip4, None, None, abi.PLUG_ALL) == 0
        nss.append((ns, tags, mac, ip4))
    yield dict(rx=rx, nss=nss)
    rx.close()


def test_nsstat_one_namespace_echo(wide):
    """4,096 echo requests to one client of one Namespace: every lane hits one key."""
    ns, tags, mac, ip4 = wide["nss"][5]
    fr = []
    for i in range(4096):
        ic = F.icmp4(8, 0, 0x1234, i, bytes(18))
        fr.append(R._eth(mac, R.DUT_MAC, tags, 0x0800, F.ipv4(bytes([48, 0, 0, 7]), ip4, 1, ic), 0))
    buf, desc = F.pack_frames(fr, [1] * len(fr))
    m = prepare(wide["rx"], buf, desc)
    want = want_prefix(m, 4096, max_ns=WIDE_NS)
    assert (want[0] == 1).all() and len(want[1]) == 1
    e = want[1][0]
    assert (int(e["ns_id"]), int(e["frames"]), int(e["cnt"][abi.NSC_ICMP_ECHO]), int(e["cnt"].sum())) == (ns, 4096, 4096, 4096)
    check(nsstat(m, 4096, 1), want)


@pytest.mark.parametrize("short", [0, 1], ids=["exact", "one-below"])
def test_nsstat_distinct_namespaces(wide, short):
    """1,024 answered ARP requests in 1,024 Namespaces: every workgroup holds 512 distinct (ns,
    counter) keys.  The Namespace ids lie in all four rounds of the flag scan (WIDE_NS rows, 8,192 a
    round), so the ordinals carry from round to round and the events come out in ascending ns_id
    across them; ev_cap one below the distinct count overflows, and a normal call behind it is exact."""
    if "distinct" not in wide:
        fr = []
        for k, (ns, tags, mac, ip4) in enumerate(wide["nss"]):
            sha = bytes([0, 0x10, 0x94, 0, k >> 8, k & 0xFF])
            f = R._eth(b"\xff" * 6, sha, tags, 0x0806, F.arp(1, sha, bytes([48, 0, k >> 8, k & 0xFF]), bytes(6), ip4), 0)
            fr.append(f + bytes(max(60 - len(f), 0)))
        buf, desc = F.pack_frames(fr, [1] * len(fr))
        wide["distinct"] = prepare(wide["rx"], buf, desc)
    m = wide["distinct"]
    assert (m["rsp"] == abi.RSP_ARP).all() and (m["lrn"] == abi.LRN_ARP_REQ).all()
    full = want_prefix(m, 1024, max_ns=WIDE_NS)
    ev = full[1]
    assert (full[0] == 1).all() and len(ev) == 1024 and (ev["frames"] == 1).all()
    assert [int(x) for x in ev["ns_id"]] == sorted(ns for ns, _, _, _ in wide["nss"])
    got_ids = [int(x) for x in ev["ns_id"]]
    assert set(WIDE_EDGES) <= set(got_ids) and got_ids == sorted(got_ids)
    per_round = np.bincount(np.array(got_ids) // SCAN_ROUND, minlength=4)
    assert len(per_round) == 4 and (per_round >= 2).all(), per_round  # every round of the scan holds flagged rows
    assert (ev["cnt"][:, abi.NSC_ARP_QUERY] == 1).all() and (ev["cnt"][:, abi.NSC_ARP_TX_REPLY] == 1).all()
    cap = 1024 - short
    want = want_prefix(m, 1024, ev_cap=cap, max_ns=WIDE_NS)
    assert tuple(int(x) for x in want[2]) == (0 if short else 1024, 1024, short, 1024, 0, 0, 0, 0)
    got = nsstat(m, 1024, cap)
    check(got, want)
    if short:
        assert (got["ev"] == SENTINEL).all()
        check(nsstat(m, 1024, 1024), full)  # the scratch is zero again
        check(nsstat(m, 300, 1024), want_prefix(m, 300, max_ns=WIDE_NS))


# ---- the argument checks on a device handle -----------------------------------------------------------
def test_nsstat_argument_checks(mixed):
    import torch
    m, rx = mixed, mixed["rx"]
    cap = rx.nsstat_max_events()
    assert cap == 16  # min(max_frames 4096, max_ns 16)
    ev = torch.full((cap * EV + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
    dn = torch.full((4096,), SENTINEL, dtype=torch.uint8, device="cuda")
    info = torch.full((abi.NSS_INFO_WORDS + 1,), -1, dtype=torch.int64, device="cuda")
    a = dict(frames=m["tb"], desc=m["td"], rec=m["trec"], n=64, rsp=m["t_rsp"], lrn=m["t_lrn"], ev=ev, ev_cap=cap, done=dn,
             info=info, kinds=abi.RSPK_ALL, stream=None)

    def rc(**kw):
        p = dict(a, **kw)
        ad = lambda x: 0 if x is None else x if isinstance(x, int) else x.data_ptr()  # noqa: E731
        s = p["stream"]
        return rx.lib.emurx_nsstat_dev(rx.h, ad(p["frames"]), ad(p["desc"]), ad(p["rec"]), p["n"], p["kinds"], ad(p["rsp"]),
                                       ad(p["lrn"]), ad(p["ev"]), p["ev_cap"], ad(p["done"]), ad(p["info"]),
                                       None if s is None else s.cuda_stream)

    EINVAL, ENOMEM = -22, -12
    for kw in (dict(kinds=0), dict(kinds=16), dict(ev_cap=0), dict(ev_cap=cap + 1), dict(frames=None), dict(desc=None),
               dict(rec=None), dict(rsp=None), dict(lrn=None), dict(lrn=None, kinds=abi.RSPK_ND), dict(ev=None), dict(info=None),
               dict(rec=m["trec"].data_ptr() + 8), dict(desc=m["td"].data_ptr() + 4), dict(ev=ev.data_ptr() + 4),
               dict(info=info.data_ptr() + 4)):
        assert rc(**kw) == EINVAL, kw
    assert rc(n=4097) == ENOMEM
    # a capturing stream is refused before anything is enqueued
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        refused = rc(stream=s)
    assert refused == EINVAL
    torch.cuda.synchronize()
    assert (ev == SENTINEL).all() and (dn == SENTINEL).all() and (info == -1).all()  # none of them wrote anything
    # without ARP and ND the learn outcomes are not needed, and the call works
    assert rc(lrn=None, kinds=abi.RSPK_ICMP | abi.RSPK_ICMPV6) == 0
    torch.cuda.synchronize()
    want = want_prefix(m, 64, abi.RSPK_ICMP | abi.RSPK_ICMPV6)
    assert np.array_equal(info.cpu().numpy().view(np.uint64)[: abi.NSS_INFO_WORDS], want[2]) and int(info[-1]) == -1
    assert np.array_equal(dn.cpu().numpy()[:64], want[0])

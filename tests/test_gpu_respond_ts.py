"""GPU parity of emurx_respond_ts_dev against ts_ref: outcome, descriptors, source indices, reply
bytes and d_info bit-exact; nothing written outside the replies' rows, past out_cap or behind
d_info.  Records come from emurx_classify_dev on the same handle."""
import numpy as np
import pytest

import respond_ref as R
import sim_envs as S
import ts_ref as T
from emurx import abi, frames as F
from test_gpu_respond import SENTINEL, check, classify
from test_nsstat_ref import sim_envs

pytestmark = pytest.mark.gpu

GUARD = 4  # words behind d_info that must stay untouched
ALL = abi.RSPK_ALL_TS
TIME = 0x0123ABCD


def respond(rx, tb, td, trec, n, cap, kinds, ip_time=TIME, outcome=True, tail=4096, sync=True):
    """One emurx_respond_ts_dev call (emurx_respond_kinds_dev with ip_time None) into sentinel-filled
    buffers -> dict of numpy outputs after finish()."""
    import torch
    out = torch.full((cap + tail,), SENTINEL, dtype=torch.uint8, device="cuda")
    od = torch.full((max(n, 1) * 8,), SENTINEL, dtype=torch.uint8, device="cuda")
    src = torch.full((max(n, 1),), -1, dtype=torch.int32, device="cuda")
    oc = torch.full((max(n, 1) + 64,), SENTINEL, dtype=torch.uint8, device="cuda") if outcome else None
    info = torch.full((abi.RSP_INFO_WORDS + GUARD,), -1, dtype=torch.int64, device="cuda")
    rx.respond_dev(tb, td, trec, n, out, cap, od, src, oc, info, kinds=kinds, ip_time=ip_time)
    got = dict(out=out, od=od, src=src, oc=oc, info=info, n=n)
    return finish(got) if sync else got


def finish(g):
    import torch
    torch.cuda.synchronize()
    n = g["n"]
    iw = g["info"].cpu().numpy().view(np.uint64)
    assert (iw[abi.RSP_INFO_WORDS:] == 0xFFFFFFFFFFFFFFFF).all(), iw  # nothing behind the info words
    oc = None
    if g["oc"] is not None:
        oc = g["oc"].cpu().numpy()
        assert (oc[n:] == SENTINEL).all()
        oc = oc[:n]
    return dict(out=g["out"].cpu().numpy(), desc=g["od"].cpu().numpy()[: n * 8].view(abi.DESC_DTYPE),
                src=g["src"].cpu().numpy().view(np.uint32)[:n], outcome=oc, info=iw[: abi.RSP_INFO_WORDS])


def handle(max_frames=1 << 13):
    from emurx.rx import RxPath
    rx = RxPath(0, max_ns=16, max_clients=64, max_frames=max_frames)
    rx.register_all()
    env = R.Env()
    R.load_tables(rx, env)
    return rx, env


def batch(rx, env, frames, holes=()):
    buf, desc = F.pack_frames(frames, [1] * len(frames))
    for i in holes:
        desc["pad"][i] = abi.DESC_HOLE
    tb, td, trec, rec = classify(rx, buf, desc)
    return dict(rx=rx, env=env, buf=buf, desc=desc, tb=tb, td=td, trec=trec, rec=rec, n=len(desc))


def want_of(m, n, kinds, ip_time=TIME, cap=None):
    return T.respond_batch(m["buf"], m["desc"][:n], m["rec"][:n], kinds, ip_time, m["env"], out_cap=cap)


def run(m, n, kinds, ip_time=TIME, cap=None, **kw):
    want = want_of(m, n, kinds, ip_time, cap)
    c = int(want[4][1]) if cap is None else cap
    check(respond(m["rx"], m["tb"], m["td"], m["trec"], n, c, kinds, ip_time, **kw), want, n, c)
    return want


@pytest.fixture(scope="module")
def mixed(gpu_ok, oracle_built):
    """respond_ref's mixed batch (it holds timestamp requests), with holes; smaller n are prefixes."""
    rx, env = handle()
    fr, vp = R.mixed_batch(4099)
    buf, desc = R.pack_with_holes(fr, vp)
    tb, td, trec, rec = classify(rx, buf, desc)
    yield dict(rx=rx, env=env, buf=buf, desc=desc, tb=tb, td=td, trec=trec, rec=rec, n=4099, kept={})
    rx.close()


def shapes_frames():
    """Every l4 (34, 38, 42, 46: 0 to 2 tags, IHL 5 to 7) with ICMP spans of 20, 21, 36 and 37 bytes
    (the time bytes at 14, 2, 6 and 10 mod 16: inside one row and across two), the short and the
    multicast drops, a 9,216-byte request of 0xff (a sum that folds more than once) and a span
    whose sum is 0xffff."""
    fr = []
    for ns, opts in ((0, 0), (1, 0), (0, 1), (2, 0), (1, 1), (3, 0), (2, 1), (1, 2), (0, 2), (3, 1)):
        for span in (20, 21, 36, 37):
            fr.append(T.ts_frame(ns, (ns + span) % R.N_CLIENTS, opts=opts, span=span, orig=bytes([span, ns, opts, 0xFE]),
                                 ident=0xFFFF - span, seq=0xFF00 | opts))
    assert {T.l4_of(ns, o) for ns, o in ((0, 0), (1, 0), (2, 0), (2, 1))} == {34, 38, 42, 46}
    fr += [T.ts_frame(0, 1, span=8), T.ts_frame(1, 1, span=19), T.ts_frame(2, 1, opts=1, span=19),
           T.ts_frame(0, 2, span=19, esrc=bytes([1, 0, 0x5E, 0, 0, 1])), T.ts_frame(1, 2, span=40, esrc=b"\xff" * 6),
           T.ts_frame(1, 3, span=24, src=bytes([224, 0, 0, 9]))]
    jumbo = T.ts_frame(0, 0, span=abi.MAX_FRAME - 34, icmp_len=abi.MAX_FRAME - 34, orig=b"\xff" * 4, fill=0xFF, ident=0xFFFF,
                       seq=0xFFFF)
    assert len(jumbo) == abi.MAX_FRAME and jumbo[46:] == b"\xff" * (abi.MAX_FRAME - 46)
    fr += [jumbo, T.ffff_frame(1, 1, TIME, span=36), T.ffff_frame(2, 0, TIME, span=21, opts=1),
           T.ts_frame(3, 3, span=1500, icmp_len=1500, fill=0xFF)]
    return fr


@pytest.fixture(scope="module")
def shapes(gpu_ok, oracle_built):
    rx, env = handle(1 << 10)
    fr = shapes_frames()
    m = batch(rx, env, fr, holes=(5, 17))
    yield dict(m, frames=fr)
    rx.close()


# ---- the reference's six requests -----------------------------------------------------------------
@pytest.mark.parametrize("ip_time", [0, 86_399_999, 0xFFFFFFFF])
def test_ts_six_requests(gpu_ok, oracle_built, ip_time):
    from emurx.rx import RxPath
    rx = RxPath(0, max_ns=16, max_clients=16, max_frames=1 << 10)
    rx.register_all()
    S.load_env(rx, "icmp")
    m = batch(rx, sim_envs("icmp")[0], T.six_requests())
    want = run(m, 6, ALL, ip_time)
    assert (want[0] == abi.RSP_TS).all() and int(want[4][0]) == 6 and int(want[4][1 + abi.RSP_TS]) == 6
    rx.close()


# ---- the mixed batch ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kinds", [16, 18, 31])
def test_ts_mixed(mixed, kinds):
    want = run(mixed, 4099, kinds)
    o = want[0]
    assert (o == abi.RSP_TS).sum() >= 100 and (o == abi.RSP_DROP_MCAST).any()
    if kinds == 16:
        assert set(np.unique(o)) == {abi.RSP_NONE, abi.RSP_DROP_MCAST, abi.RSP_TS}
    else:
        assert (o == abi.RSP_ICMP).sum() >= 100 and int(want[4][0]) == len(want[3]) > (o == abi.RSP_TS).sum()


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_ts_mixed_prefixes(mixed, n):
    run(mixed, n, ALL)


@pytest.mark.parametrize("kinds", list(range(1, 16)))
def test_ts_entry_point_equals_kinds_dev(mixed, kinds):
    """Without the timestamp kind the new entry point is emurx_respond_kinds_dev byte for byte."""
    m, n = mixed, 4099
    if "cap" not in m["kept"]:
        m["kept"]["cap"] = int(want_of(m, n, abi.RSPK_ALL)[4][1])
    cap = m["kept"]["cap"]
    new = respond(m["rx"], m["tb"], m["td"], m["trec"], n, cap, kinds, ip_time=0xDEADBEEF)
    old = respond(m["rx"], m["tb"], m["td"], m["trec"], n, cap, kinds, ip_time=None)
    for k in ("out", "desc", "src", "outcome", "info"):
        assert np.array_equal(new[k], old[k]), k
    assert int(old["info"][0]) > 0 or kinds == abi.RSPK_ND
    assert (old["info"][1 + abi.RSP_TS:] == 0).all() and abi.RSP_TS not in old["outcome"]


# ---- the shapes ----------------------------------------------------------------------------------------
def test_ts_shapes(shapes):
    m = shapes
    want = run(m, m["n"], ALL)
    o = want[0]
    assert (o == abi.RSP_TS).sum() == 40 - 2 + 4 and (o == abi.RSP_DROP_SHORT).sum() == 3 and (o == abi.RSP_DROP_MCAST).sum() == 3
    assert int(want[4][1 + abi.RSP_DROP_SHORT]) == 3 and (o == abi.RSP_NONE).sum() == 2  # the holes
    l4s = {int(m["rec"][i]["l4"]) for i in want[2]}
    assert l4s == {34, 38, 42, 46}
    by_src = dict(zip((int(i) for i in want[2]), want[3]))
    n = m["n"]
    jumbo = by_src[n - 4]
    assert len(jumbo) == abi.MAX_FRAME and T.span_sum(jumbo[34:]) == 0xFFFF
    for i in (n - 3, n - 2):  # a span that sums to 0xffff stores 0x0000
        z, l4 = by_src[i], int(m["rec"][i]["l4"])
        assert z[l4 + 2:l4 + 4] == b"\0\0" and T.span_sum(z[l4:]) == 0xFFFF


def test_ts_shapes_other_time_and_kinds(shapes):
    m = shapes
    run(m, m["n"], abi.RSPK_TS, 0xFFFFFFFF)
    want = run(m, m["n"], abi.RSPK_ALL)  # kinds <= 15 through the new entry point: every request stays with Go
    assert set(np.unique(want[0])) == {abi.RSP_NONE, abi.RSP_DROP_MCAST, abi.RSP_HOST}


@pytest.mark.parametrize("short", [0, 16], ids=["exact", "minus16"])
def test_ts_capacity(shapes, short):
    m = shapes
    n = m["n"] - 1  # the batch then ends in a timestamp reply
    need = int(want_of(m, n, ALL)[4][1])
    cap = need - short
    want = run(m, n, ALL, cap=cap)
    assert int(want[4][1]) == need and int((want[0] == abi.RSP_NOSPC).sum()) == (1 if short else 0)
    if short:
        assert want[0][n - 1] == abi.RSP_NOSPC and int(want[4][1 + abi.RSP_NOSPC]) == 1


def test_ts_capacity_mid_batch(shapes):
    m = shapes
    cap = (int(want_of(m, m["n"], ALL)[4][1]) // 3) & ~15
    want = run(m, m["n"], ALL, cap=cap)
    assert 0 < len(want[3]) and (want[0] == abi.RSP_NOSPC).sum() >= 3


def test_ts_without_outcome_array(shapes):
    run(shapes, shapes["n"], ALL, outcome=False)


def test_ts_n_zero(shapes):
    m = shapes
    got = respond(m["rx"], m["tb"], m["td"], m["trec"], 0, 64, ALL)
    assert (got["info"] == 0).all() and (got["out"] == SENTINEL).all()


def test_ts_twice_without_synchronisation(shapes):
    """Two calls back to back on the handle's stream with different times: each reply carries the
    time of its call (the time rides the launch, the shared scratch is reused in stream order)."""
    m, n = shapes, shapes["n"]
    w1, w2 = want_of(m, n, ALL, 1), want_of(m, n, ALL, 0xFFFFFFFE)
    cap = int(w1[4][1])
    g1 = respond(m["rx"], m["tb"], m["td"], m["trec"], n, cap, ALL, 1, sync=False)
    g2 = respond(m["rx"], m["tb"], m["td"], m["trec"], n, cap, ALL, 0xFFFFFFFE, sync=False)
    check(finish(g1), w1, n, cap)
    check(finish(g2), w2, n, cap)
    assert w1[3] != w2[3]


# ---- which lane owns the reply -----------------------------------------------------------------------
def test_ts_reply_owners(shapes):
    """Replies owned by lanes 0, 63, 64 and 255 of the first tile, by lane 0 of the second and by
    the batch's last lane in a partial last tile; every other frame gets no reply."""
    n = 300
    own = {0: 20, 63: 21, 64: 36, 255: 37, 256: 52, n - 1: 53}
    fr = [T.ts_frame(i % 4, i % R.N_CLIENTS, span=own[i], opts=i % 3, seq=i) if i in own else T.ts_frame(i % 4, 1, typ=17, seq=i)
          for i in range(n)]
    m = batch(shapes["rx"], shapes["env"], fr)
    want = run(m, n, ALL)
    assert sorted(int(i) for i in want[2]) == sorted(own) and (want[0] == abi.RSP_TS).sum() == len(own)
    want = run(m, 257, abi.RSPK_TS | abi.RSPK_ICMP)
    assert int(want[2][-1]) == 256


def test_ts_full_tiles(shapes):
    """Two full tiles and a partial one of timestamp requests of every span from 20 to 83 bytes: up
    to eight rows a reply, all 256 accumulators of a tile in use."""
    n = 600
    fr = [T.ts_frame(i % 4, i % R.N_CLIENTS, span=20 + (i * 7) % 64, opts=(i // 4) % 3, seq=i, orig=bytes([i & 0xFF, i >> 8, 0xFF, 0xFF]))
          for i in range(n)]
    m = batch(shapes["rx"], shapes["env"], fr, holes=(255, 256))
    want = run(m, n, ALL)
    assert (want[0] == abi.RSP_TS).sum() == n - 2


# ---- the argument checks on a device handle --------------------------------------------------------------
def test_ts_argument_checks(shapes):
    import torch
    m, rx = shapes, shapes["rx"]
    out = torch.full((1 << 16,), SENTINEL, dtype=torch.uint8, device="cuda")
    od = torch.full((m["n"] * 8 + 8,), SENTINEL, dtype=torch.uint8, device="cuda")
    src = torch.full((m["n"] + 2,), -1, dtype=torch.int32, device="cuda")
    oc = torch.full((m["n"],), SENTINEL, dtype=torch.uint8, device="cuda")
    info = torch.full((abi.RSP_INFO_WORDS + 1,), -1, dtype=torch.int64, device="cuda")
    a = dict(frames=m["tb"], desc=m["td"], rec=m["trec"], n=m["n"], kinds=ALL, time=TIME, out=out, cap=1 << 16, od=od, src=src,
             oc=oc, info=info, stream=None)

    def rc(**kw):
        p = dict(a, **kw)
        ad = lambda x: 0 if x is None else x if isinstance(x, int) else x.data_ptr()  # noqa: E731
        s = p["stream"]
        return rx.lib.emurx_respond_ts_dev(rx.h, ad(p["frames"]), ad(p["desc"]), ad(p["rec"]), p["n"], p["kinds"], p["time"],
                                           ad(p["out"]), p["cap"], ad(p["od"]), ad(p["src"]), ad(p["oc"]), ad(p["info"]),
                                           None if s is None else s.cuda_stream)

    for kw in (dict(kinds=0), dict(kinds=32), dict(kinds=33), dict(frames=None), dict(desc=None), dict(rec=None), dict(od=None),
               dict(src=None), dict(out=None), dict(info=None), dict(n=abi.TX_ZMQ_MAX_FRAMES), dict(out=out.data_ptr() + 8),
               dict(rec=m["trec"].data_ptr() + 8), dict(desc=m["td"].data_ptr() + 4), dict(od=od.data_ptr() + 4),
               dict(info=info.data_ptr() + 4)):
        assert rc(**kw) == abi.EMURX_EINVAL, kw
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        refused = rc(stream=s)
    assert refused == abi.EMURX_EINVAL  # a capturing stream is refused before anything is enqueued
    torch.cuda.synchronize()
    assert (out == SENTINEL).all() and (od == SENTINEL).all() and (oc == SENTINEL).all() and (info == -1).all()
    assert rc(out=None, cap=0) == 0  # no buffer and no capacity: every reply NOSPC, the size needed in d_info[1]
    torch.cuda.synchronize()
    want = want_of(m, m["n"], ALL, cap=0)
    assert np.array_equal(info.cpu().numpy().view(np.uint64)[: abi.RSP_INFO_WORDS], want[4]) and int(info[-1]) == -1
    assert np.array_equal(oc.cpu().numpy(), want[0])

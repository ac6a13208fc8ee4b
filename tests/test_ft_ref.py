"""CPU checks of ft_ref: replaying the per-client fold of the refused TCP / UDP frames leaves every
ftStats counter and errParser as frame-by-frame handling does (records and flow words from the
oracle), on a mixed stream at every cut, on the reference's 17 transport captures, and with the
tables moved mid-batch (the stale rule)."""
import numpy as np
import pytest

import ft_cases as K
import ft_ref as R
import transport_sims as T
from emurx import abi
from emurx import frames as F


def classified(o, frames, vports=None):
    buf, desc = F.pack_frames(frames, vports or [1] * len(frames))
    rec, _, _, _ = o.rx_batch(buf, desc)
    return buf, desc, rec, o.flows(buf, desc, rec)


def folded(buf, desc, rec, flow, n, max_ns=K.MAX_NS, max_clients=K.MAX_CLIENTS):
    oc, cand = R.outcomes(buf, desc[:n], rec[:n], flow[:n], max_ns, max_clients)
    return (oc,) + R.fold(oc, cand, rec[:n])


@pytest.fixture(scope="module")
def orc(oracle_built):
    o = oracle_built.Oracle()
    K.load_tables(o)
    K.load_flows(o)
    return o


def test_matrix_outcomes(orc):
    m = K.matrix()
    buf, desc, rec, flow = classified(orc, [f for _, f, _ in m])
    oc, cand = R.outcomes(buf, desc, rec, flow, K.MAX_NS, K.MAX_CLIENTS)
    assert [(n, int(o) & 7) for (n, _, _), o in zip(m, oc)] == [(n, w) for n, _, w in m]
    assert [bool(o & abi.FT_V6) for (n, _, w), o in zip(m, oc) if 1 <= w <= 3] == [n.endswith("v6") for n, _, w in m if 1 <= w <= 3]
    assert cand.sum() == len(m) - 1 and not cand[-1]
    # the flow words behind the outcomes 0: found flows and NEW, which stay with the handler
    byname = {n: int(fw) for (n, _, _), fw in zip(m, flow)}
    assert byname["tcp-new-v4"] == byname["udp-new-v6"] == abi.FLOW_NEW and byname["tcp-flow-v6"] <= abi.FLOW_ID_MAX


def test_replay_equals_frame_by_frame_at_every_cut(orc):
    buf, desc, rec, flow = classified(orc, K.stream(300))
    oc_all, _ = R.outcomes(buf, desc, rec, flow, K.MAX_NS, K.MAX_CLIENTS)
    assert all(((oc_all & 7) == k).sum() >= 15 for k in range(5)) and (oc_all & abi.FT_V6).sum() >= 40
    assert (flow == abi.FLOW_NEW).sum() >= 20 and (flow <= abi.FLOW_ID_MAX).sum() >= 20
    for cut in range(301):
        oc, ev, info = folded(buf, desc, rec, flow, cut)
        got = R.replay(ev, info, oc, buf, desc, rec, flow)
        want = R.by_frame(buf, desc, rec, flow, upto=cut)
        assert R.clean(got[0]) == R.clean(want[0]) and got[1] == want[1], cut
        assert int(info[0]) == len(ev) == len({int(rec[i]["client_id"]) for i in range(cut) if 1 <= oc[i] & 7 <= 3})
        assert (np.diff(ev["last"].astype(np.int64)) > 0).all()


@pytest.mark.parametrize("capture", T.CAPTURES)
def test_transport_captures(oracle_built, capture):
    """The capture's frames as their receivers' rx frames, with no flow loaded (the listener alone),
    with the listener removed, and with both flows loaded: the folded counters per client equal the
    restatement's; frames with a found flow or NEW stay at outcome 0."""
    from test_reference_transport_sims import corpus
    fr = T.frames(corpus(), capture)
    proto, ckey, skey, accept, _ = T.plan(capture, fr)
    buf, desc = F.pack_frames(fr, [1] * len(fr))

    def state(listener, flows):
        o = oracle_built.Oracle()
        T.load(o, proto, ckey, abi.PLUG_ALL)
        if not flows:
            assert o.flow_remove(T.CLIENT["cid"], ckey) == 0
        else:
            assert o.flow_add(T.SERVER["cid"], skey, T.SERVER_FLOW) == 0
        if not listener:
            assert o.server_remove(T.SERVER["cid"], T.PORT, proto) == 0
        rec, _, _, _ = o.rx_batch(buf, desc)
        flow = o.flows(buf, desc, rec)
        oc, cand = R.outcomes(buf, desc, rec, flow, 16, 16)
        ev, info = R.fold(oc, cand, rec)
        assert cand.all() and not oc[(flow <= abi.FLOW_ID_MAX) | (flow == abi.FLOW_NEW)].any()
        got = R.replay(ev, info, oc, buf, desc, rec, flow)
        want = R.by_frame(buf, desc, rec, flow)
        assert R.clean(got[0]) == R.clean(want[0]) and got[1] == want[1] == 0
        # the events alone against the refused frames alone
        refused = [i for i in range(len(fr)) if oc[i]]
        only = R.by_frame(buf, desc, rec, flow, only=refused)[0]
        assert R.clean({int(e["client_id"]): dict(zip(R.FTC, map(int, e["cnt"]))) for e in ev}) == R.clean(only)
        assert int(ev["frames"].sum()) == len(refused) if len(ev) else not refused
        return oc, flow

    oc, flow = state(True, False)   # no flow: the accepted frame is NEW, what follows it is refused
    assert flow[accept] == abi.FLOW_NEW and oc.any()
    oc, flow = state(False, False)  # and no listener
    assert flow[accept] == abi.FLOW_NO_SERVER and (oc[accept] & 7) == (abi.FT_NO_SRV_TCP if proto == 6 else abi.FT_NO_SRV_UDP)
    assert bool(oc[accept] & abi.FT_V6) == T.l3l4(fr[accept])[0]
    oc, flow = state(True, True)    # both flows: only frames before the accept can be refused
    assert not oc[accept + 1:].any()


@pytest.mark.parametrize("k", [0, 97, 250])
def test_stale_subtraction(oracle_built, k):
    """The tables move behind frame k (a flow is added for client 1, as a FLOW_NEW frame's OnAccept
    would, client 2 loses its listener and client 5 gets its TransportCtx): the frames behind k are
    stale, run their handlers against the tables as they are, and their contributions leave the
    events first, client 5's EMURX_FT_ERR frames leaving errParser.  The final counters equal
    frame-by-frame handling, frames [0, k] against the old tables and the rest against the new ones."""
    o = oracle_built.Oracle()
    K.load_tables(o)
    K.load_flows(o)
    fr = K.stream(300)
    for i in range(0, 300, 4):  # client 1's refused flow, and new flows at client 2's listener
        fr[i] = K.l4(1, 6, bool(i & 8), flags=K.ACK, sport=2000) if i & 4 else K.l4(2, 6, bool(i & 8), flags=K.SYN)
    for i in range(2, 300, 8):  # client 5 has no TransportCtx yet: PARSER_ERR
        fr[i] = K.l4(5, 6 if i & 16 else 17, bool(i & 32))
    buf, desc, rec, flow = classified(o, fr)
    oc, ev, info = folded(buf, desc, rec, flow, 300)
    assert o.client_set_transport(5, 1) == 0
    for v6 in (False, True):
        assert o.flow_add(1, K.tuple_of(K.l4(1, 6, v6, flags=K.ACK, sport=2000)), 77 + v6) == 0
    assert o.server_remove(2, K.TCP_PORT, 6) == 0
    flow_now = o.flows(buf, desc, rec)
    moved = np.nonzero(flow_now != flow)[0]
    assert (moved > k).sum() >= 10 and {int(rec[i]["client_id"]) for i in moved} == {1, 2, 5}
    stale = [i for i in range(k + 1, 300) if int(rec[i]["client_id"]) in (1, 2, 5)]  # what emurx_recs_stale flags
    n_err = sum(int(oc[i]) == abi.FT_ERR for i in stale)  # outcome 4: one errParser each comes out of info[6]
    assert n_err >= 5 and all(flow_now[i] in (abi.FLOW_NO_SYN, abi.FLOW_NO_SERVER) for i in stale if oc[i] == abi.FT_ERR)
    got = R.replay(ev, info, oc, buf, desc, rec, flow, stale=stale, flow_now=flow_now)
    mixed = np.where(np.arange(300) <= k, flow, flow_now)
    want = R.by_frame(buf, desc, rec, mixed)
    assert R.clean(got[0]) == R.clean(want[0]) and got[1] == want[1]
    old = R.by_frame(buf, desc, rec, flow)
    assert R.clean(got[0]) != R.clean(old[0]) and got[1] == old[1] - n_err  # the move shows in the counters and in errParser

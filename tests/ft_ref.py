"""What the transport plugin does with a TCP / UDP frame that reaches no socket, restated from the
reference (src/emu/plugins/transport/), the per-client fold of emurx_ftstat_dev and the Go side's
replay of its events.  TEST INFRASTRUCTURE ONLY.

Per frame, in the order the reference runs (HandleRxPacket core/thread_ctx.go:365-372 counts a
callback's negative return as errParser):
  HandleRxTransPacket      plugin_transport.go:116-127   GetNs nil (:118-120) or the Namespace without
                                                         the plugin (:121-124) -> PARSER_ERR
  PluginTransNs.handle..   plugin_transport.go:82-114    CLookupByMac nil (:95-97) or the client without
                                                         the plugin (:109-112) -> PARSER_ERR
  PluginTransClient.hand.. plugin_transport.go:74-80     no TransportCtx (:75-78) -> -1
  TransportCtx.handleRx..  client_ctx.go:912-969         version = p[L3] >> 4 (:918-920); ft_lookupv4 (:927) /
                                                         ft_lookupv6 (:951); found: ft_lookup_found* and the
                                                         socket's input; else handleRx{Tcp,Udp}NewFlow, whose
                                                         return value is dropped (:936-942, :960-966): returns 0
  handleRxTcpNewFlow       client_ctx.go:829-864         ft_new_tcp (:837); no bare SYN: ft_new_tcp_no_syn (:842);
                                                         no listener: ft_new_no_cb (:851); else OnAccept
  handleRxUdpNewFlow       client_ctx.go:866-903         ft_new_udp (:878); no listener: ft_new_no_cb (:886)
The flow word per frame (EMURX_FLOW_*) is the oracle's (pyoracle.Oracle.flows), which restates the
probe and the listener lookup; this module takes it as given."""
from collections import Counter

import numpy as np

from emurx import abi

LK_ERR = (abi.LK["NO_NS"], abi.LK["NS_NO_PLUGIN"], abi.LK["NO_CLIENT"], abi.LK["CLIENT_NO_PLUGIN"])
FTC = abi.FTC_GO  # the six folded counters, in enum emurx_ftc order


# ---- the handler, frame by frame ------------------------------------------------------------
def handle(frame: bytes, rec, flow: int, stats: dict) -> int:
    """HandleRxTransPacket for one classified tcp / udp frame: adds to stats[client_id] (a Counter
    of ftStats names) what the reference adds and returns what it returns.  A found flow and a new
    flow with a listener reach socket code, of which only the flow table's own counters are kept."""
    lk = (int(rec["flags"]) >> 4) & 7
    if lk in LK_ERR:
        return -1  # plugin_transport.go:118-124, :95-97, :109-112
    assert lk == abi.LK["CLIENT"], lk
    if flow == abi.FLOW_NO_CTX:
        return -1  # :75-78
    st = stats.setdefault(int(rec["client_id"]), Counter())
    v6 = frame[int(rec["l3"])] >> 4 != 4  # client_ctx.go:918-920
    st["ft_lookupv6" if v6 else "ft_lookupv4"] += 1  # :927 / :951
    if flow <= abi.FLOW_ID_MAX:
        st["ft_lookup_foundv6" if v6 else "ft_lookup_foundv4"] += 1  # :929 / :953
        return 0  # the socket's input decides; not modelled
    tcp = int(rec["proto"]) == abi.CB_TCP
    st["ft_new_tcp" if tcp else "ft_new_udp"] += 1  # :837 / :878
    if flow == abi.FLOW_NO_SYN:
        assert tcp
        st["ft_new_tcp_no_syn"] += 1  # :842
    elif flow == abi.FLOW_NO_SERVER:
        st["ft_new_no_cb"] += 1  # :851 / :886
    else:
        assert flow == abi.FLOW_NEW, hex(flow)  # OnAccept and the socket: not modelled
    return 0  # :968: the new-flow functions' return values are dropped (:936-942, :960-966)


def is_candidate(desc, rec) -> bool:
    return (int(rec["status"]) == 0 and int(desc["pad"]) != abi.DESC_HOLE
            and int(rec["proto"]) in (abi.CB_TCP, abi.CB_UDP))


def by_frame(buf, desc, rec, flow, upto=None, only=None):
    """Every candidate frame [0, upto) (or the indices `only`) through handle() -> (stats, errParser)."""
    stats, err = {}, 0
    idx = range(len(desc) if upto is None else upto) if only is None else only
    for i in idx:
        if not is_candidate(desc[i], rec[i]) or (int(rec[i]["flags"]) >> 4) & 7 in (abi.LK["NONE"], abi.LK["NS_LEVEL"]):
            continue
        f = buf[int(desc[i]["off"]):int(desc[i]["off"]) + int(desc[i]["len"])].tobytes()
        if handle(f, rec[i], int(flow[i]), stats) < 0:
            err += 1  # thread_ctx.go:365-372
    return stats, err


# ---- the device's rule per frame (include/emu_rx.h emurx_ftstat_dev) ---------------------------
def outcome_of(buf, d, r, flow: int, max_ns: int, max_clients: int):
    """-> (outcome byte, candidate)"""
    if not is_candidate(d, r):
        return abi.FT_NONE, False
    lk = (int(r["flags"]) >> 4) & 7
    if lk in LK_ERR:
        return abi.FT_ERR, True
    if lk != abi.LK["CLIENT"] or int(r["client_id"]) >= max_clients or int(r["ns_id"]) >= max_ns:
        return abi.FT_NONE, True
    tcp = int(r["proto"]) == abi.CB_TCP
    if flow == abi.FLOW_NO_CTX:
        return abi.FT_ERR, True
    if flow == abi.FLOW_NO_SYN and tcp:
        o = abi.FT_NO_SYN
    elif flow == abi.FLOW_NO_SERVER:
        o = abi.FT_NO_SRV_TCP if tcp else abi.FT_NO_SRV_UDP
    else:
        return abi.FT_NONE, True
    l3 = int(r["l3"])
    if l3 < 14 or l3 >= int(d["len"]):
        return abi.FT_NONE, True
    return (o if int(buf[int(d["off"]) + l3]) >> 4 == 4 else o | abi.FT_V6), True


def outcomes(buf, desc, rec, flow, max_ns, max_clients):
    """-> (outcome u8 [n], candidate bool [n])"""
    n = len(desc)
    oc, cand = np.zeros(n, np.uint8), np.zeros(n, bool)
    for i in range(n):
        oc[i], cand[i] = outcome_of(buf, desc[i], rec[i], int(flow[i]), max_ns, max_clients)
    return oc, cand


def contribution(ob: int) -> Counter:
    """The ftStats words a frame with outcome byte ob contributed to its client's event."""
    o, c = ob & 7, Counter()
    if o in (abi.FT_NO_SYN, abi.FT_NO_SRV_TCP, abi.FT_NO_SRV_UDP):
        c["ft_lookupv6" if ob & abi.FT_V6 else "ft_lookupv4"] += 1
        c["ft_new_udp" if o == abi.FT_NO_SRV_UDP else "ft_new_tcp"] += 1
        c["ft_new_tcp_no_syn" if o == abi.FT_NO_SYN else "ft_new_no_cb"] += 1
    return c


# ---- the fold -----------------------------------------------------------------------------------
def fold(oc, cand, rec, ev_cap=None):
    """-> (events abi.FT_EV_DTYPE in ascending `last`, info u64[8]) of the first len(oc) frames."""
    rows = {}
    for i, ob in enumerate(oc):
        if 1 <= (int(ob) & 7) <= 3:
            e = rows.setdefault(int(rec[i]["client_id"]), dict(first=i, frames=0, cnt=Counter()))
            e["last"], e["ns_id"] = i, int(rec[i]["ns_id"])
            e["frames"] += 1
            e["cnt"] += contribution(int(ob))
    order = sorted(rows, key=lambda c: rows[c]["last"])
    over = ev_cap is not None and len(order) > ev_cap
    ev = np.zeros(0 if over else len(order), abi.FT_EV_DTYPE)
    for k, c in enumerate(order if not over else []):
        e = rows[c]
        ev[k] = (e["ns_id"], c, e["first"], e["last"], e["frames"], [e["cnt"][n] for n in FTC] + [0])
    o7 = np.asarray(oc) & 7
    info = np.array([len(ev), len(order), int(over), (o7 == 1).sum(), (o7 == 2).sum(), (o7 == 3).sum(), (o7 == 4).sum(),
                     (np.asarray(cand) & (np.asarray(oc) == 0)).sum()], np.uint64)
    return ev, info


# ---- the Go side's replay ----------------------------------------------------------
def replay(ev, info, oc, buf, desc, rec, flow, stale=(), flow_now=None):
    """What the caller does with a batch's events: per event tx.flowTableStats.ft_* += ev.cnt[*] and
    errParser += info[6]; the transport handler runs for the candidates with outcome 0 alone.  A
    frame in `stale` (emurx_recs_stale flagged it: the tables moved after the batch was classified)
    runs its handler against the tables as they are now (flow_now; the other frames' handlers saw
    the tables the batch was classified against, flow), and its contribution, read off its outcome
    byte, is taken out of its client's event first.  -> (stats, errParser)"""
    assert int(info[2]) == 0, "an overflowing batch has no events: every frame runs its handler"
    stale = set(stale)
    stats, err = {}, int(info[6])
    cnt = {int(e["client_id"]): Counter({n: int(e["cnt"][k]) for k, n in enumerate(FTC)}) for e in ev}
    for i in stale:
        ob = int(oc[i])
        if 1 <= (ob & 7) <= 3:
            cnt[int(rec[i]["client_id"])].subtract(contribution(ob))
        elif ob == abi.FT_ERR:
            err -= 1
    for c, k in cnt.items():
        assert min(k.values(), default=0) >= 0
        stats.setdefault(c, Counter()).update(k)
    run = [i for i in range(len(oc)) if int(oc[i]) == 0 or i in stale]
    live = np.array([flow_now[i] if i in stale else flow[i] for i in range(len(oc))], np.uint32)
    s2, e2 = by_frame(buf, desc, rec, live, only=run)
    for c, k in s2.items():
        stats.setdefault(c, Counter()).update(k)
    return stats, err + e2


def clean(stats):
    """Counters without zero entries and clients without counters, for comparison."""
    out = {c: {n: v for n, v in k.items() if v} for c, k in stats.items()}
    return {c: k for c, k in out.items() if k}

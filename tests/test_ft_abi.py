"""C-ABI checks of emurx_ftstat_dev and the ingest flow stage that need no GPU: the exports, the
structs' layouts, the enums, and the argument checks on a host-only handle (EMURX_ENOMEM, which
comes behind the device check, is exercised on a small device handle in test_gpu_ftstat.py)."""
import ctypes as C
import re
from pathlib import Path

import numpy as np

from emurx import abi

HEADER = (Path(__file__).resolve().parent.parent / "include" / "emu_rx.h").read_text()


def test_exports_and_signatures(lib):
    for name in ("emurx_ftstat_dev", "emurx_ftstat_max_events", "emurx_ingest_set_flows", "emurx_ingest_flows"):
        assert hasattr(lib, name), name
        assert name in {s[0] for s in abi.SIGNATURES}
    assert lib.emurx_abi_version() == 6  # added entry points, nothing changed


def test_layouts_match_the_header():
    d = abi.FT_EV_DTYPE
    assert d.itemsize == 48 and abi.FT_INFO_WORDS == 8 and abi.FTC_WORDS == 7
    assert {n: d.fields[n][1] for n in d.names} == dict(ns_id=0, client_id=4, first=8, last=12, frames=16, cnt=20)
    body = re.search(r"typedef struct emurx_ft_ev \{(.*?)\} emurx_ft_ev;", HEADER, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"\b([a-z_0-9]+)\s*(?:\[\w+\])?[,;]", body) == list(d.names)
    assert C.sizeof(abi.FlowsOut) == 32 + 8 * abi.FT_INFO_WORDS
    body = re.search(r"typedef struct emurx_flows_out \{(.*?)\} emurx_flows_out;", HEADER, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"\b([a-z_0-9]+)\s*(?:\[\w+\])?[,;]", body) == [f[0] for f in abi.FlowsOut._fields_]
    # emurx_ingest_result, emurx_answers and emurx_ping_out keep their sizes
    assert C.sizeof(abi.Answers) == 352 and C.sizeof(abi.PingOut) == 24 + 8 * abi.PNG_INFO_WORDS


def test_enums_and_constants():
    assert (abi.FT_NONE, abi.FT_NO_SYN, abi.FT_NO_SRV_TCP, abi.FT_NO_SRV_UDP, abi.FT_ERR, abi.FT_V6) == (0, 1, 2, 3, 4, 8)
    for name, val in (("EMURX_FT_NONE", 0), ("EMURX_FT_NO_SYN", 1), ("EMURX_FT_NO_SRV_TCP", 2), ("EMURX_FT_NO_SRV_UDP", 3),
                      ("EMURX_FT_ERR", 4), ("EMURX_FTC_LOOKUP_V4", 0)):
        assert re.search(r"\b%s = %d\b" % (name, val), HEADER), name
    for name, val in (("EMURX_FT_V6", "0x08u"), ("EMURX_FTC_WORDS", "7"), ("EMURX_FT_INFO_WORDS", "8")):
        assert re.search(r"#define %s %s\b" % (name, val), HEADER), name
    order = re.search(r"enum emurx_ftc \{(.*?)\};", HEADER, re.S).group(1)
    order = re.findall(r"EMURX_FTC_([A-Z0-9_]+)", re.sub(r"/\*.*?\*/", "", order, flags=re.S))
    assert order == ["LOOKUP_V4", "LOOKUP_V6", "NEW_TCP", "NEW_TCP_NO_SYN", "NEW_UDP", "NEW_NO_CB"]
    assert abi.FTC_GO == ["ft_lookupv4", "ft_lookupv6", "ft_new_tcp", "ft_new_tcp_no_syn", "ft_new_udp", "ft_new_no_cb"]


def test_host_only_handle_and_bad_arguments(lib):
    cfg = abi.Cfg(-1, 16, 48, 64, 0)  # host-only handle: no device
    h = C.c_void_p()
    assert lib.emurx_open(C.byref(cfg), C.byref(h)) == 0
    try:
        cap = lib.emurx_ftstat_max_events(h)
        assert cap == 48 and lib.emurx_ftstat_max_events(None) == 0  # min(max_frames, max_clients)
        buf = np.zeros(4096, np.uint8)
        p = (buf.ctypes.data + 63) & ~63

        def call(hh=h, fr=p, de=p, re_=p, fl=p, n=4, ev=p, ev_cap=4, oc=p, info=p):
            return lib.emurx_ftstat_dev(hh, fr, de, re_, fl, n, ev, ev_cap, oc, info, None)

        assert call() == abi.EMURX_EDEVICE and call(oc=None) == abi.EMURX_EDEVICE and call(n=0) == abi.EMURX_EDEVICE
        assert call(hh=None) == abi.EMURX_EINVAL
        assert call(ev_cap=0) == abi.EMURX_EINVAL and call(ev_cap=cap + 1) == abi.EMURX_EINVAL and call(ev_cap=cap) == abi.EMURX_EDEVICE
        assert call(ev=None) == abi.EMURX_EINVAL and call(info=None) == abi.EMURX_EINVAL
        assert call(fr=None) == abi.EMURX_EINVAL and call(de=None) == abi.EMURX_EINVAL and call(re_=None) == abi.EMURX_EINVAL
        assert call(fl=None) == abi.EMURX_EINVAL
        assert call(fr=None, de=None, re_=None, fl=None, n=0) == abi.EMURX_EDEVICE  # n == 0 needs none of them
        assert call(re_=p + 8) == abi.EMURX_EINVAL and call(de=p + 4) == abi.EMURX_EINVAL and call(fl=p + 2) == abi.EMURX_EINVAL
        assert call(ev=p + 4) == abi.EMURX_EINVAL and call(info=p + 4) == abi.EMURX_EINVAL
        assert call(n=abi.TX_ZMQ_MAX_FRAMES) == abi.EMURX_EINVAL
        # the stage on an ingest slot: arguments first, then the device
        sf, fl = lib.emurx_ingest_set_flows, lib.emurx_ingest_flows
        o = abi.FlowsOut()
        assert sf(None, 0, 1) == abi.EMURX_EINVAL and sf(h, abi.INGEST_SLOTS, 1) == abi.EMURX_EINVAL
        assert sf(h, 0, 1) == abi.EMURX_EDEVICE and sf(h, 0, 0) == abi.EMURX_EDEVICE  # a host-only handle
        assert fl(None, 0, C.byref(o)) == abi.EMURX_EINVAL and fl(h, abi.INGEST_SLOTS, C.byref(o)) == abi.EMURX_EINVAL
        assert fl(h, 0, None) == abi.EMURX_EINVAL and fl(h, 0, C.byref(o)) == abi.EMURX_EINVAL  # no batch was waited for
    finally:
        lib.emurx_close(h)

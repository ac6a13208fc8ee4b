"""C-ABI checks of emurx_ping_dev that need no GPU: the exports, the event's layout, the enums,
and the argument checks on a host-only handle."""
import ctypes as C
import re
from pathlib import Path

import numpy as np

from emurx import abi

HEADER = (Path(__file__).resolve().parent.parent / "include" / "emu_rx.h").read_text()


def test_exports_and_signatures(lib):
    for name in ("emurx_ping_dev", "emurx_ping_max_events", "emurx_ingest_set_ping", "emurx_ingest_set_now", "emurx_ingest_ping"):
        assert hasattr(lib, name), name
        assert name in {s[0] for s in abi.SIGNATURES}
    assert lib.emurx_abi_version() == 6  # added entry points, nothing changed


def test_event_layout_matches_the_header():
    d = abi.PING_EV_DTYPE
    assert d.itemsize == 80
    off = {n: d.fields[n][1] for n in d.names}
    assert off == dict(ns_id=0, client_id=4, ident=8, family=10, flags=11, first=12, last=16, n_reply=20, n_unreach=24,
                       n_malformed=28, n_bad_latency=32, n_ok=36, n_succ=40, seq_first=44, seq_last=46, lat_sum=48,
                       lat_min_tail=56, lat_max=64, n_no_client=72, n_mcast=76)
    # the header declares the fields in this order
    body = re.search(r"typedef struct emurx_ping_ev \{(.*?)\} emurx_ping_ev;", HEADER, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"\b([a-z_0-9]+)\s*[,;]", body)
    assert names == list(d.names)


def test_enums_and_constants():
    assert (abi.PNG_NONE, abi.PNG_REPLY, abi.PNG_UNREACH, abi.PNG_NO_CLIENT, abi.PNG_MCAST, abi.PNG_HOST) == tuple(range(6))
    assert (abi.PNGK_V4, abi.PNGK_V6, abi.PNGK_ALL, abi.PNG_INFO_WORDS) == (1, 2, 3, 8)
    for name, val in (("EMURX_PNG_NONE", 0), ("EMURX_PNG_REPLY", 1), ("EMURX_PNG_UNREACH", 2), ("EMURX_PNG_NO_CLIENT", 3),
                      ("EMURX_PNG_MCAST", 4), ("EMURX_PNG_HOST", 5)):
        assert re.search(r"\b%s = %d\b" % (name, val), HEADER), name
    for name, val in (("EMURX_PNGK_V4", "1u"), ("EMURX_PNGK_V6", "2u"), ("EMURX_PNGK_ALL", "3u"), ("EMURX_PNG_INFO_WORDS", "8"),
                      ("EMURX_PING_MAGIC", "0xc15c0c15c0be5be5ull"), ("EMURX_PING_TIMEOUT_NS", "5000000000ull")):
        assert re.search(r"#define %s %s\b" % (name, val), HEADER), name
    assert abi.PING_MAGIC == 0xC15C0C15C0BE5BE5 and abi.PING_TIMEOUT_NS == 5 * 10 ** 9


def test_host_only_handle_and_bad_arguments(lib):
    cfg = abi.Cfg(-1, 16, 16, 64, 0)  # host-only handle: no device
    h = C.c_void_p()
    assert lib.emurx_open(C.byref(cfg), C.byref(h)) == 0
    try:
        cap = lib.emurx_ping_max_events(h)
        assert cap == lib.emurx_learn_max_events(h) >= 64 and lib.emurx_ping_max_events(None) == 0
        buf = np.zeros(4096, np.uint8)
        p = (buf.ctypes.data + 63) & ~63
        now = 1 << 62

        def call(hh=h, fr=p, de=p, re_=p, n=4, fams=abi.PNGK_ALL, t=now, ev=p, ev_cap=4, oc=p, info=p):
            return lib.emurx_ping_dev(hh, fr, de, re_, n, fams, t, ev, ev_cap, oc, info, None)

        assert call() == abi.EMURX_EDEVICE and call(oc=None) == abi.EMURX_EDEVICE and call(n=0) == abi.EMURX_EDEVICE
        assert call(hh=None) == abi.EMURX_EINVAL
        assert call(fams=0) == abi.EMURX_EINVAL and call(fams=4) == abi.EMURX_EINVAL
        assert call(t=1 << 63) == abi.EMURX_EINVAL and call(t=(1 << 63) - 1) == abi.EMURX_EDEVICE
        assert call(ev_cap=0) == abi.EMURX_EINVAL and call(ev_cap=cap + 1) == abi.EMURX_EINVAL and call(ev_cap=cap) == abi.EMURX_EDEVICE
        assert call(ev=None) == abi.EMURX_EINVAL and call(info=None) == abi.EMURX_EINVAL
        assert call(fr=None) == abi.EMURX_EINVAL and call(de=None) == abi.EMURX_EINVAL and call(re_=None) == abi.EMURX_EINVAL
        assert call(fr=None, de=None, re_=None, n=0) == abi.EMURX_EDEVICE  # n == 0 needs none of them
        assert call(re_=p + 8) == abi.EMURX_EINVAL and call(de=p + 4) == abi.EMURX_EINVAL
        assert call(ev=p + 4) == abi.EMURX_EINVAL and call(info=p + 4) == abi.EMURX_EINVAL
        assert call(n=abi.TX_ZMQ_MAX_FRAMES) == abi.EMURX_EINVAL
        # the stage on an ingest slot: arguments first, then the device
        sp, sn, ip = lib.emurx_ingest_set_ping, lib.emurx_ingest_set_now, lib.emurx_ingest_ping
        o = abi.PingOut()
        assert C.sizeof(abi.PingOut) == 24 + 8 * abi.PNG_INFO_WORDS
        assert sp(None, 0, 1) == abi.EMURX_EINVAL and sp(h, abi.INGEST_SLOTS, 1) == abi.EMURX_EINVAL and sp(h, 0, 4) == abi.EMURX_EINVAL
        assert sp(h, 0, abi.PNGK_ALL) == abi.EMURX_EDEVICE and sp(h, 0, 0) == abi.EMURX_EDEVICE  # a host-only handle
        assert sn(None, 0, 1) == abi.EMURX_EINVAL and sn(h, abi.INGEST_SLOTS, 1) == abi.EMURX_EINVAL
        assert sn(h, 0, 1 << 63) == abi.EMURX_EINVAL and sn(h, 0, (1 << 63) - 1) == abi.EMURX_OK  # a host store
        assert ip(None, 0, C.byref(o)) == abi.EMURX_EINVAL and ip(h, abi.INGEST_SLOTS, C.byref(o)) == abi.EMURX_EINVAL
        assert ip(h, 0, None) == abi.EMURX_EINVAL and ip(h, 0, C.byref(o)) == abi.EMURX_EINVAL  # no batch was waited for
    finally:
        lib.emurx_close(h)

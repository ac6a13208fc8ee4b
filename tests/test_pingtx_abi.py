"""C-ABI checks of the resident ping templates (emurx_pingtx_*): the exports, the layouts and the
argument checks on a host-only handle, which need no GPU; and the store's bookkeeping (ids, the
fill, reuse after a remove), which needs a handle with a device because emurx_pingtx_reserve
allocates the device image (a host-only handle gets EMURX_EDEVICE) and is marked gpu."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import pingtx_ref as R
from emurx import abi

HEADER = (Path(__file__).resolve().parent.parent / "include" / "emu_rx.h").read_text()
NAMES = ("emurx_pingtx_reserve", "emurx_pingtx_add", "emurx_pingtx_remove", "emurx_pingtx_dev", "emurx_egress_ping_buffer",
         "emurx_egress_submit_ping")


def template(seq=0x0102, size=16, vlans=(0, 0)):
    return R.template4(bytes([0, 0, 1, 0, 0, 7]), vlans, bytes([16, 0, 0, 7]), bytes([48, 0, 0, 1]), 0x4242, seq,
                       payload_size=size)


def test_exports_layouts_and_constants(lib):
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in {s[0] for s in abi.SIGNATURES}
    assert lib.emurx_abi_version() == 6  # added entry points, nothing changed
    assert abi.PINGTX_REQ_DTYPE.itemsize == 16 and abi.DESC_DTYPE.itemsize == 8
    d = abi.PINGTX_REQ_DTYPE
    assert {n: d.fields[n][1] for n in d.names} == dict(id=0, seq=4, count=6, ts=8)
    assert d == R.REQ_DTYPE and abi.DESC_DTYPE == R.DESC_DTYPE
    body = re.search(r"typedef struct emurx_pingtx_req \{(.*?)\} emurx_pingtx_req;", HEADER, re.S).group(1)
    assert re.findall(r"\b([a-z_0-9]+)\s*;", body) == list(d.names)
    assert (abi.PTX_OK, abi.PTX_BAD_ID, abi.PTX_NOSPC, abi.PTX_INFO_WORDS) == (0, 1, 2, 8)
    assert (abi.PINGTX_SLOT, abi.PINGTX_MAX_LEN) == (256, 248) == (R.SLOT, R.MAX_LEN)
    for name, val in (("EMURX_PTX_OK", 0), ("EMURX_PTX_BAD_ID", 1), ("EMURX_PTX_NOSPC", 2)):
        assert re.search(r"\b%s = %d\b" % (name, val), HEADER), name
    for name, val in (("EMURX_PINGTX_SLOT", "256u"), ("EMURX_PINGTX_MAX_LEN", "248u"), ("EMURX_PTX_INFO_WORDS", "8")):
        assert re.search(r"#define %s %s\b" % (name, val), HEADER), name


def test_host_only_handle(lib):
    cfg = abi.Cfg(-1, 16, 16, 64, 0)  # host-only handle: no device
    h = C.c_void_p()
    assert lib.emurx_open(C.byref(cfg), C.byref(h)) == 0
    try:
        icmp_off, t = template()
        t = bytes(t)
        i = C.c_uint32(77)
        assert lib.emurx_pingtx_reserve(h, 8) == abi.EMURX_EDEVICE
        assert lib.emurx_pingtx_reserve(None, 8) == abi.EMURX_EINVAL and lib.emurx_pingtx_reserve(h, 0) == abi.EMURX_EINVAL
        # no reserve before it
        assert lib.emurx_pingtx_add(h, t, len(t), icmp_off, 1, C.byref(i)) == abi.EMURX_EINVAL and i.value == 77
        assert lib.emurx_pingtx_add(None, t, len(t), icmp_off, 1, C.byref(i)) == abi.EMURX_EINVAL
        assert lib.emurx_pingtx_remove(h, 0) == abi.EMURX_ENOENT and lib.emurx_pingtx_remove(None, 0) == abi.EMURX_EINVAL
        buf = np.zeros(4096, np.uint8)
        p = (buf.ctypes.data + 63) & ~63

        def call(hh=h, req=p, n=4, out=p, cap=1024, de=p, dcap=16, oc=p, info=p):
            return lib.emurx_pingtx_dev(hh, req, n, out, cap, de, dcap, oc, info, None)

        assert call() == abi.EMURX_EDEVICE and call(oc=None) == abi.EMURX_EDEVICE and call(n=0) == abi.EMURX_EDEVICE
        assert call(hh=None) == abi.EMURX_EINVAL and call(info=None) == abi.EMURX_EINVAL
        assert call(req=None) == abi.EMURX_EINVAL and call(de=None) == abi.EMURX_EINVAL and call(out=None) == abi.EMURX_EINVAL
        assert call(out=None, cap=0) == abi.EMURX_EDEVICE and call(req=None, de=None, out=None, n=0) == abi.EMURX_EDEVICE
        assert call(out=p + 8) == abi.EMURX_EINVAL and call(req=p + 4) == abi.EMURX_EINVAL
        assert call(de=p + 4) == abi.EMURX_EINVAL and call(info=p + 4) == abi.EMURX_EINVAL
        q = C.c_void_p()
        assert lib.emurx_egress_ping_buffer(h, 0, C.byref(q)) == abi.EMURX_EDEVICE
        assert lib.emurx_egress_ping_buffer(h, abi.EGRESS_SLOTS, C.byref(q)) == abi.EMURX_EINVAL
        assert lib.emurx_egress_ping_buffer(h, 0, None) == abi.EMURX_EINVAL
        assert lib.emurx_egress_submit_ping(h, 0, 0, 0, 0, 1) == abi.EMURX_EDEVICE
        assert lib.emurx_egress_submit_ping(h, abi.EGRESS_SLOTS, 0, 0, 0, 1) == abi.EMURX_EINVAL
        assert lib.emurx_egress_submit_ping(h, 0, 0, 0, 2, 1) == abi.EMURX_EINVAL  # unknown flag
    finally:
        lib.emurx_close(h)


@pytest.fixture()
def rx(gpu_ok):
    from emurx.rx import RxPath
    r = RxPath(0, max_ns=16, max_clients=16, max_frames=256, max_bytes=1 << 16)
    yield r
    r.close()


@pytest.mark.gpu
def test_add_remove_reserve_errors(rx):
    icmp_off, t = template()
    assert rx.pingtx_add(t, icmp_off, 1)[0] == abi.EMURX_EINVAL            # no reserve before it
    assert rx.pingtx_remove(0) == abi.EMURX_ENOENT
    assert rx.pingtx_reserve(4) == 0
    assert rx.pingtx_reserve(4) == abi.EMURX_EEXIST and rx.pingtx_reserve(8) == abi.EMURX_EEXIST
    assert rx.pingtx_add(t, icmp_off, 256)[0] == abi.EMURX_EINVAL          # vport > 255
    assert rx.pingtx_add(t[:icmp_off + 23], icmp_off, 1)[0] == abi.EMURX_EINVAL   # icmp_off + 24 > len
    assert rx.pingtx_add(t, len(t) - 23, 1)[0] == abi.EMURX_EINVAL
    assert rx.pingtx_add(t, 0xFFFFFFF0, 1)[0] == abi.EMURX_EINVAL          # no wrap in icmp_off + 24
    big_off, big = template(size=abi.PINGTX_MAX_LEN + 1 - icmp_off - 8)
    assert len(big) == abi.PINGTX_MAX_LEN + 1 and rx.pingtx_add(big, big_off, 1)[0] == abi.EMURX_EINVAL
    ffff = bytearray(t)
    ffff[icmp_off + 2:icmp_off + 4] = b"\xff\xff"
    assert rx.pingtx_add(ffff, icmp_off, 1)[0] == abi.EMURX_EINVAL         # a checksum field of 0xffff
    assert rx.pingtx_add(t, icmp_off, 255) == (0, 0)                       # none of them took an id
    assert rx.pingtx_add(big[:-1], big_off, 0) == (0, 1)                   # the longest template
    assert rx.pingtx_add(t[:icmp_off + 24], icmp_off, 0) == (0, 2)         # the shortest for its icmp_off
    assert rx.pingtx_remove(3) == abi.EMURX_ENOENT and rx.pingtx_remove(4) == abi.EMURX_ENOENT
    assert rx.pingtx_remove(0xFFFFFFFF) == abi.EMURX_ENOENT
    assert rx.pingtx_remove(1) == 0 and rx.pingtx_remove(1) == abi.EMURX_ENOENT


@pytest.mark.gpu
def test_store_fills_exactly_and_ids_come_back_only_after_remove(rx):
    n = 37
    assert rx.pingtx_reserve(n) == 0
    icmp_off, t = template()
    assert [rx.pingtx_add(t, icmp_off, i) for i in range(n)] == [(0, i) for i in range(n)]
    assert rx.pingtx_add(t, icmp_off, 0)[0] == abi.EMURX_ENOSPC
    assert rx.pingtx_add(t, icmp_off, 0)[0] == abi.EMURX_ENOSPC
    for i in (30, 5, 17):
        assert rx.pingtx_remove(i) == 0
    # no egress batch is in flight: the removed ids may be handed out at once, the lowest first
    assert [rx.pingtx_add(t, icmp_off, 0) for _ in range(3)] == [(0, 5), (0, 17), (0, 30)]
    assert rx.pingtx_add(t, icmp_off, 0)[0] == abi.EMURX_ENOSPC
    assert rx.pingtx_remove(5) == 0 and rx.pingtx_remove(5) == abi.EMURX_ENOENT
    assert rx.pingtx_add(t, icmp_off, 0) == (0, 5)
    for i in range(n):
        assert rx.pingtx_remove(i) == 0
    assert [rx.pingtx_add(t, icmp_off, 0)[1] for _ in range(n)] == list(range(n))

"""The C-ABI of the timestamp reply (emurx_respond_ts_dev, emurx_nsstat_ts_dev,
emurx_ingest_set_answers_ts, emurx_ingest_set_time) without a GPU: the symbols, the constants of
include/emu_rx.h and the argument checks a host-only handle can reach."""
import ctypes as C
import re

import numpy as np
import pytest

from emurx import abi

NEW = ["emurx_respond_ts_dev", "emurx_nsstat_ts_dev", "emurx_ingest_set_answers_ts", "emurx_ingest_set_time"]
HEADER = (abi.REPO_ROOT / "include" / "emu_rx.h").read_text()


def header_value(name):
    m = re.search(r"\b%s\s*=\s*(\d+)" % name, HEADER) or re.search(r"#define\s+%s\s+(\d+)u?\b" % name, HEADER)
    assert m, name
    return int(m.group(1))


@pytest.fixture()
def host_handle(lib):
    cfg = abi.Cfg(-1, 16, 16, 16, 0)  # host-only handle: no device
    h = C.c_void_p()
    assert lib.emurx_open(C.byref(cfg), C.byref(h)) == 0
    yield h
    lib.emurx_close(h)


def test_symbols_are_exported_and_declared(lib):
    for name in NEW:
        assert getattr(lib, name) is not None
        assert re.search(r"\bint\s+%s\s*\(" % name, HEADER), name


def test_constants(lib):
    assert header_value("EMURX_RSPK_TS") == abi.RSPK_TS == 16
    assert header_value("EMURX_RSPK_ALL_TS") == abi.RSPK_ALL_TS == 31
    assert header_value("EMURX_RSPK_ALL") == abi.RSPK_ALL == 15
    assert header_value("EMURX_RSP_TS") == abi.RSP_TS == 8
    assert header_value("EMURX_RSP_DROP_SHORT") == abi.RSP_DROP_SHORT == 9
    # the new word follows the enum's last one
    assert "EMURX_NSC_ICMP_ERR_TOO_SHORT = EMURX_NSC_ND_RX_NA_LEARN + 1" in HEADER
    assert header_value("EMURX_NSC_ND_RX_NA_LEARN") + 1 == abi.NSC_ICMP_ERR_TOO_SHORT == 19 < abi.NSC_WORDS
    assert header_value("EMURX_RSP_INFO_WORDS") == abi.RSP_INFO_WORDS == 16 and 1 + abi.RSP_DROP_SHORT < abi.RSP_INFO_WORDS
    assert header_value("EMURX_NSC_WORDS") == abi.NSC_WORDS == 22
    assert abi.NSC_GO_TS[abi.NSC_ICMP_ERR_TOO_SHORT] == ("icmp", ("pktRxErrTooShort",)) and abi.NSC_GO_TS[:19] == abi.NSC_GO
    assert lib.emurx_abi_version() == 6
    assert C.sizeof(abi.Answers) == 352


def test_respond_ts_argument_checks(lib, host_handle):
    h = host_handle
    buf = np.zeros(256, np.uint64)
    p = buf.ctypes.data

    def rc(kinds, n=1, time=5):
        return lib.emurx_respond_ts_dev(h, p, p, p, n, kinds, time, p, 64, p, p, p, p, None)
    assert rc(0) == abi.EMURX_EINVAL and rc(32) == abi.EMURX_EINVAL and rc(64 | 16) == abi.EMURX_EINVAL
    for kinds in (1, 15, 16, 18, 31):  # a valid call reaches the device binding: a host-only handle has none
        assert rc(kinds) == abi.EMURX_EDEVICE, kinds
        assert rc(kinds, time=0xFFFFFFFF) == abi.EMURX_EDEVICE
    assert lib.emurx_respond_kinds_dev(h, p, p, p, 1, 15, p, 64, p, p, p, p, None) == abi.EMURX_EDEVICE
    assert lib.emurx_respond_kinds_dev(h, p, p, p, 1, 16, p, 64, p, p, p, p, None) == abi.EMURX_EINVAL
    assert lib.emurx_respond_kinds_dev(h, p, p, p, 1, 31, p, 64, p, p, p, p, None) == abi.EMURX_EINVAL
    assert lib.emurx_respond_ts_dev(h, p, p, p, 1, 31, 5, p, 64, p, p, p, None, None) == abi.EMURX_EINVAL  # no d_info
    assert lib.emurx_respond_ts_dev(None, p, p, p, 1, 31, 5, p, 64, p, p, p, p, None) == abi.EMURX_EINVAL


def test_nsstat_ts_argument_checks(lib, host_handle):
    h = host_handle
    buf = np.zeros(256, np.uint64)
    p = buf.ctypes.data

    def rc(kinds, fn=lib.emurx_nsstat_ts_dev):
        return fn(h, p, p, p, 1, kinds, p, p, p, 1, p, p, None)
    assert rc(0) == abi.EMURX_EINVAL and rc(32) == abi.EMURX_EINVAL
    for kinds in (16, 16 | 1, 16 | 4 | 8, 16 | 13):  # TS without ICMP
        assert rc(kinds) == abi.EMURX_EINVAL, kinds
    for kinds in (2, 15, 18, 31):
        assert rc(kinds) == abi.EMURX_EDEVICE, kinds
    assert rc(15, lib.emurx_nsstat_dev) == abi.EMURX_EDEVICE
    assert rc(16, lib.emurx_nsstat_dev) == abi.EMURX_EINVAL and rc(31, lib.emurx_nsstat_dev) == abi.EMURX_EINVAL
    assert rc(18, lib.emurx_nsstat_dev) == abi.EMURX_EINVAL


def test_ingest_ts_argument_checks(lib, host_handle):
    h = host_handle
    assert lib.emurx_ingest_set_answers(h, 0, 16) == abi.EMURX_EINVAL  # the old entry point keeps rejecting it
    assert lib.emurx_ingest_set_answers(h, 0, 31) == abi.EMURX_EINVAL
    assert lib.emurx_ingest_set_answers(h, 0, 15) == abi.EMURX_EDEVICE
    assert lib.emurx_ingest_set_answers_ts(h, 0, 32) == abi.EMURX_EINVAL
    assert lib.emurx_ingest_set_answers_ts(h, abi.INGEST_SLOTS, 31) == abi.EMURX_EINVAL
    for kinds in (16, 17, 29):  # TS without ICMP
        assert lib.emurx_ingest_set_answers_ts(h, 0, kinds) == abi.EMURX_EINVAL, kinds
    for kinds in (0, 15, 18, 31):
        assert lib.emurx_ingest_set_answers_ts(h, 0, kinds) == abi.EMURX_EDEVICE, kinds
    assert lib.emurx_ingest_set_time(h, abi.INGEST_SLOTS, 1) == abi.EMURX_EINVAL
    assert lib.emurx_ingest_set_time(None, 0, 1) == abi.EMURX_EINVAL
    for t in (0, 86_399_999, 0xFFFFFFFF):  # a host store: any u32, no device needed
        assert lib.emurx_ingest_set_time(h, abi.INGEST_SLOTS - 1, t) == abi.EMURX_OK

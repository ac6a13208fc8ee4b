"""The tx planner's and the egress slots' C-ABI without a GPU: the exports, the result struct,
the constants against emurx/abi.py and every argument error on a host-only handle."""
import ctypes as C
import re

import numpy as np
import pytest

from emurx import abi

NEW = ["emurx_tx_plan_dev", "emurx_egress_buffer", "emurx_egress_submit", "emurx_egress_wait"]


@pytest.fixture()
def host_only(lib):
    cfg = abi.Cfg(-1, 16, 16, 64, 4096)  # host-only handle: the table mirror alone
    h = C.c_void_p()
    assert lib.emurx_open(C.byref(cfg), C.byref(h)) == 0
    yield h
    lib.emurx_close(h)


def test_exports_and_version(lib):
    bound = {s[0] for s in abi.SIGNATURES}
    for name in NEW:
        assert hasattr(lib, name) and name in bound and name in abi.OPTIONAL, name
    assert lib.emurx_abi_version() == 6


def test_struct_and_constants_match_the_header():
    txt = (abi.REPO_ROOT / "include" / "emu_rx.h").read_text()
    assert C.sizeof(abi.EgressResult) == 112
    body = re.search(r"typedef struct emurx_egress_result \{(.*?)\} emurx_egress_result;", txt, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.findall(r"\w+", re.sub(r"\[.*?\]", "", part))[-1] for decl in body.split(";") if decl.strip()
             for part in decl.split(",")]
    assert names == ["msgs", "msg_off", "n_msgs", "n_frames", "bytes", "plan", "status", "plan_info"]
    assert [f[0] for f in abi.EgressResult._fields_] == names
    assert abi.EgressResult.plan_info.offset == 48 and abi.EgressResult.bytes.offset == 24
    for name, val in (("EGRESS_SLOTS", abi.EGRESS_SLOTS), ("TXP_INFO_WORDS", abi.TXP_INFO_WORDS),
                      ("TXP_UDP0_KEEP", abi.TXP_UDP0_KEEP)):
        assert int(re.search(r"#define EMURX_%s (\d+)" % name, txt).group(1)) == val
    assert (abi.TXP_NONE, abi.TXP_HDR, abi.TXP_L4, abi.TXP_LENGTH, abi.TXP_BAD) == (0, 1, 2, 3, 4)


def test_tx_plan_argument_errors(lib, host_only):
    h = host_only
    a = np.zeros(256, np.uint64)  # 16-byte aligned scratch for every pointer
    p = a.ctypes.data
    p += -p % 16
    plan = lib.emurx_tx_plan_dev
    assert plan(None, p, p, 1, 0, p, p, p, None) == abi.EMURX_EINVAL
    assert plan(h, None, p, 1, 0, p, p, p, None) == abi.EMURX_EINVAL
    assert plan(h, p, None, 1, 0, p, p, p, None) == abi.EMURX_EINVAL
    assert plan(h, p, p, 1, 0, None, p, p, None) == abi.EMURX_EINVAL
    assert plan(h, p, p, 1, 0, p, p, None, None) == abi.EMURX_EINVAL
    assert plan(h, p, p, 0, 0, p, p, None, None) == abi.EMURX_EINVAL       # d_info is written for n == 0 too
    assert plan(h, p, p, 1, 2, p, p, p, None) == abi.EMURX_EINVAL          # unknown flag bit
    assert plan(h, p, p, 1, 0x80000000, p, p, p, None) == abi.EMURX_EINVAL
    assert plan(h, p, p + 4, 1, 0, p, p, p, None) == abi.EMURX_EINVAL      # descriptor alignment
    assert plan(h, p, p, 1, 0, p + 8, p, p, None) == abi.EMURX_EINVAL      # tx descriptor alignment
    assert plan(h, p, p, 65, 0, p, p, p, None) == abi.EMURX_ENOMEM         # n > cfg.max_frames
    assert plan(h, p, p, 1, 0, p, None, p, None) == abi.EMURX_EDEVICE      # valid (outcome may be NULL): host-only
    assert plan(h, None, None, 0, 1, None, None, p, None) == abi.EMURX_EDEVICE


def test_egress_argument_errors(lib, host_only):
    h = host_only
    f, d = C.c_void_p(), C.c_void_p()
    r = abi.EgressResult()
    assert lib.emurx_egress_buffer(None, 0, C.byref(f), C.byref(d)) == abi.EMURX_EINVAL
    assert lib.emurx_egress_buffer(h, abi.EGRESS_SLOTS, C.byref(f), C.byref(d)) == abi.EMURX_EINVAL
    assert lib.emurx_egress_buffer(h, 0, None, C.byref(d)) == abi.EMURX_EINVAL
    assert lib.emurx_egress_buffer(h, 0, C.byref(f), None) == abi.EMURX_EINVAL
    assert lib.emurx_egress_buffer(h, 0, C.byref(f), C.byref(d)) == abi.EMURX_EDEVICE
    assert lib.emurx_egress_submit(None, 0, 0, 0, 0) == abi.EMURX_EINVAL
    assert lib.emurx_egress_submit(h, abi.EGRESS_SLOTS, 0, 0, 0) == abi.EMURX_EINVAL
    assert lib.emurx_egress_submit(h, 0, 0, 0, 2) == abi.EMURX_EINVAL      # unknown flag bit
    assert lib.emurx_egress_submit(h, 1, 0, 0, abi.TXP_UDP0_KEEP) == abi.EMURX_EDEVICE
    assert lib.emurx_egress_wait(None, 0, C.byref(r)) == abi.EMURX_EINVAL
    assert lib.emurx_egress_wait(h, abi.EGRESS_SLOTS, C.byref(r)) == abi.EMURX_EINVAL
    assert lib.emurx_egress_wait(h, 0, None) == abi.EMURX_EINVAL
    assert lib.emurx_egress_wait(h, 0, C.byref(r)) == abi.EMURX_EDEVICE

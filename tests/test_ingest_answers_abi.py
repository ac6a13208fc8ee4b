"""The answers of an ingest slot and the counted tx framing, as far as they go without a GPU: the
layout of emurx_answers (the ctypes mirror against the header, compiled) and the argument checks
of the three new entry points on a host-only handle."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from emurx import abi

FIELDS = ["tx", "tx_msg_off", "n_tx_msgs", "n_replies", "tx_bytes", "reply_src", "rsp_outcome", "lrn_outcome", "done",
          "learn_ev", "n_learn", "ns_ev", "n_ns", "rsp_info", "lrn_info", "nss_info"]
OFFSETS = [0, 8, 16, 20, 24, 32, 40, 48, 56, 64, 72, 80, 88, 96, 224, 288]


def test_answers_layout_mirror():
    assert [f[0] for f in abi.Answers._fields_] == FIELDS
    assert [getattr(abi.Answers, f).offset for f in FIELDS] == OFFSETS
    assert C.sizeof(abi.Answers) == 352


def test_answers_layout_header(tmp_path):
    """The same offsets from the header itself, through the C compiler."""
    src = tmp_path / "off.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "emu_rx.h"\nint main(void) {\n' +
                   "".join(f'    printf("%zu\\n", offsetof(emurx_answers, {f}));\n' for f in FIELDS) +
                   '    printf("%zu\\n", sizeof(emurx_answers));\n    return 0;\n}\n')
    exe = tmp_path / "off"
    subprocess.run(["cc", "-I", str(abi.REPO_ROOT / "include"), "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert [int(x) for x in out] == OFFSETS + [352]


@pytest.fixture(scope="module")
def host(lib):
    from emurx.rx import RxPath
    r = RxPath(-1, max_ns=16, max_clients=16, max_frames=1 << 10)
    yield r
    r.close()


def test_set_answers_host_only(host):
    f = host.lib.emurx_ingest_set_answers
    assert f(host.h, 0, abi.RSPK_ALL) == abi.EMURX_EDEVICE
    assert f(host.h, 0, 0) == abi.EMURX_EDEVICE
    assert f(host.h, abi.INGEST_SLOTS, abi.RSPK_ALL) == abi.EMURX_EINVAL   # the private slot is not addressable
    assert f(host.h, 0, abi.RSPK_ALL + 1) == abi.EMURX_EINVAL
    assert f(host.h, 0, 1 << 31) == abi.EMURX_EINVAL
    assert f(None, 0, abi.RSPK_ARP) == abi.EMURX_EINVAL


def test_answers_before_any_wait(host):
    a = abi.Answers()
    f = host.lib.emurx_ingest_answers
    for slot in range(abi.INGEST_SLOTS):
        assert f(host.h, slot, C.byref(a)) == abi.EMURX_EINVAL
    assert f(host.h, abi.INGEST_SLOTS, C.byref(a)) == abi.EMURX_EINVAL
    assert f(host.h, 0, None) == abi.EMURX_EINVAL


def test_counted_framing_arguments(host):
    """Refused before the device is looked for: the arguments are checked first."""
    f = host.lib.emurx_tx_zmq_counted_dev
    buf = np.zeros(256, np.uint8)
    p = (buf.ctypes.data + 15) & ~15
    good = dict(frames=p, desc=p + 16, n=4, count=p + 32, out=p + 48, cap=64, off=p + 128, info=p + 192)

    def call(**kw):
        a = {**good, **kw}
        return f(host.h, a["frames"], a["desc"], a["n"], a["count"], a["out"], a["cap"], a["off"], a["info"], None)
    assert call(count=None) == abi.EMURX_EINVAL
    assert call(out=good["out"] + 8) == abi.EMURX_EINVAL                # d_out 16-byte aligned
    assert call(desc=good["desc"] + 4) == abi.EMURX_EINVAL              # descriptors 8-byte aligned
    assert call(count=good["count"] + 4) == abi.EMURX_EINVAL            # a u64 count
    assert call(n=abi.TX_ZMQ_MAX_FRAMES) == abi.EMURX_EINVAL
    assert call(off=None) == abi.EMURX_EINVAL and call(info=None) == abi.EMURX_EINVAL
    assert call(n=abi.TX_ZMQ_MAX_FRAMES - 1) == abi.EMURX_EDEVICE       # accepted: only the device is missing
    assert call() == abi.EMURX_EDEVICE

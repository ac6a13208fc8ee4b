"""emurx_tx_plan_dev (k_tx_plan, csrc/emurx_txplan.hip) against tests/txplan_ref.py: the tx
descriptors (all 16 bytes of each), the outcomes and the info words byte for byte, every output
between sentinel guards.  The batches: the capture corpus, the hand-built branch frames
(txplan_cases) at every skew of the buffer, n around the wave and workgroup sizes, extension
chains that leave the 96-byte header window, more tiles than the grid has workgroups."""
import numpy as np
import pytest

import txplan_cases
import txplan_ref
from emurx import abi

pytestmark = pytest.mark.gpu
GUARD = 64
FLAGS = [0, abi.TXP_UDP0_KEEP]


@pytest.fixture(scope="module")
def rx(gpu_ok):
    from emurx.rx import RxPath
    r = RxPath(0, max_ns=16, max_clients=16, max_frames=1 << 20)
    yield r
    r.close()


_ref = {}


def reference(key, buf, desc, flags):
    """txplan_ref over a batch, computed once and left unchanged."""
    if (key, flags) not in _ref:
        out = txplan_ref.plan(buf, desc, flags)
        for a in out:
            a.setflags(write=False)
        _ref[(key, flags)] = out
    return _ref[(key, flags)]


def corpus():
    if "corpus" not in _ref:
        from test_oracle_corpus import corpus_batch
        buf, desc, _ = corpus_batch()
        _ref["corpus"] = (buf, desc)
    return _ref["corpus"]


class Run:
    """A batch on the device: d_frames `skew` bytes past a 16-byte boundary; the tx descriptors, the
    outcomes and the info words each inside an array filled with 0xEE."""

    def __init__(self, buf, desc, skew=0, outcome=True):
        import torch
        self.n = n = len(desc)
        t = torch.zeros(32 + len(buf) + 64, dtype=torch.uint8, device="cuda")
        at = (skew - t.data_ptr()) % 16
        if len(buf):
            t[at:at + len(buf)] = torch.from_numpy(np.ascontiguousarray(buf))
        self.t, self.frames = t, t[at:]
        assert self.frames.data_ptr() % 16 == skew
        dd = np.ascontiguousarray(desc).view(np.uint8).reshape(-1)
        self.desc = torch.zeros(dd.size + 16, dtype=torch.uint8, device="cuda")
        if dd.size:
            self.desc[:dd.size] = torch.from_numpy(dd.copy())
        self.txd = torch.full((GUARD + 16 * n + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
        self.oc = torch.full((GUARD + n + GUARD,), 0xEE, dtype=torch.uint8, device="cuda") if outcome else None
        self.info = torch.full((GUARD + 8 * abi.TXP_INFO_WORDS + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")

    def call(self, rx, flags, n=None, sync=True):
        import torch
        rx.tx_plan_dev(self.frames, self.desc, self.n if n is None else n, self.txd[GUARD:],
                       None if self.oc is None else self.oc[GUARD:], self.info[GUARD:], flags)
        if sync:
            torch.cuda.synchronize()

    def check(self, want, n=None):
        n = self.n if n is None else n
        wd, wo, wi = (np.ascontiguousarray(a[:n] if k < 2 else a).view(np.uint8).reshape(-1) for k, a in enumerate(want))
        txd, info = self.txd.cpu().numpy(), self.info.cpu().numpy()
        got = txd[GUARD:GUARD + 16 * n]
        bad = np.nonzero((got.reshape(-1, 16) != wd.reshape(-1, 16)).any(1))[0]
        assert len(bad) == 0, (len(bad), bad[:8], got.reshape(-1, 16)[bad[:4]], wd.reshape(-1, 16)[bad[:4]])
        assert (txd[:GUARD] == 0xEE).all() and (txd[GUARD + 16 * n:] == 0xEE).all()
        if self.oc is not None:
            oc = self.oc.cpu().numpy()
            assert np.array_equal(oc[GUARD:GUARD + n], wo), np.nonzero(oc[GUARD:GUARD + n] != wo)[0][:8]
            assert (oc[:GUARD] == 0xEE).all() and (oc[GUARD + n:] == 0xEE).all()
        assert info[GUARD:-GUARD].tobytes() == wi.tobytes(), (info[GUARD:-GUARD].view(np.uint64), wi.view(np.uint64))
        assert (info[:GUARD] == 0xEE).all() and (info[-GUARD:] == 0xEE).all()


def prefix(want, n):
    """The reference of a batch's first n frames from the reference of the whole batch."""
    d, oc, _ = want
    info = np.zeros(abi.TXP_INFO_WORDS, np.uint64)
    info[:5] = np.bincount(oc[:n], minlength=5)
    return d[:n], oc[:n], info


@pytest.mark.parametrize("flags", FLAGS)
def test_capture_corpus(rx, flags):
    buf, desc = corpus()
    want = reference("corpus", buf, desc, flags)
    assert all(want[2][o] > 0 for o in (abi.TXP_NONE, abi.TXP_HDR, abi.TXP_L4, abi.TXP_LENGTH))
    r = Run(buf, desc)
    r.call(rx, flags)
    r.check(want)


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("skew", range(16))
def test_branch_frames_at_every_skew(rx, skew, flags):
    """Every branch of the rule, the frames at odd offsets (3 bytes apart) in a buffer that itself
    starts 0..15 bytes past a 16-byte boundary: the window's head, and which header bytes fall
    past its 96 bytes, change with both."""
    buf, desc, wd, wo = txplan_cases.batch(flags)
    want = reference("cases", buf, desc, flags)
    assert want[0].tobytes() == wd.tobytes() and np.array_equal(want[1], wo)  # the reference is the hand-written plan
    r = Run(buf, desc, skew)
    r.call(rx, flags)
    r.check(want)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257])
def test_sizes_around_wave_and_workgroup(rx, n):
    buf, desc = corpus()
    # every 33rd frame of the corpus (the captures lie one after another): a mix of every outcome it has
    sub = np.ascontiguousarray(desc[::33][:257])
    want = reference("corpus_sub", buf, sub, abi.TXP_UDP0_KEEP)
    assert len(sub) == 257 and len(set(want[1].tolist())) >= 3
    r = Run(buf, sub[:n] if n else sub[:0], skew=5)
    r.call(rx, abi.TXP_UDP0_KEEP)
    r.check(prefix(want, n))


def long_lane_batch(lane):
    """64 frames: 63 short UDP frames and, at `lane`, an IPv6 frame whose extension chain runs past
    the 96-byte window (read on from global memory by that lane alone)."""
    C = txplan_cases
    short = C.eth(0x0800) + C.ip4(C.UDP, C.l4(C.UDP, 18))
    chain = b"".join(C.ext(60, 16) for _ in range(6)) + C.ext(C.TCP, 256)
    long_ = C.eth(0x86DD, 1) + C.ip6(0, chain + C.l4(C.TCP, 40))
    frames = [short] * 64
    frames[lane] = long_
    desc = np.zeros(64, abi.DESC_DTYPE)
    parts, at = [], 0
    for i, f in enumerate(frames):
        parts.append(b"\x55" + f)
        desc[i] = (at + 1, len(f), 1, 0)
        at += 1 + len(f)
    return np.frombuffer(b"".join(parts) + bytes(32), np.uint8).copy(), desc, len(chain)


@pytest.mark.parametrize("lane", [0, 31, 63])
def test_one_long_chain_among_short_frames(rx, lane):
    buf, desc, osize = long_lane_batch(lane)
    want = reference(("long_lane", lane), buf, desc, 0)
    assert tuple(want[0][lane])[2:7] == (18, 18 + 40 + osize, osize, (abi.TX_L4_TCP6 << 4) | abi.TX_V6_NH, 6)
    assert want[2][abi.TXP_L4] == 64
    r = Run(buf, desc, skew=9)
    r.call(rx, 0)
    r.check(want)


def test_outcome_null(rx):
    buf, desc, _, _ = txplan_cases.batch(0)
    r = Run(buf, desc, skew=2, outcome=False)
    r.call(rx, 0)
    r.check(reference("cases", buf, desc, 0))


def test_twice_without_synchronisation(rx):
    """The second call clears and recounts: the info words are one call's, not the sum."""
    import torch
    buf, desc = corpus()
    r = Run(buf, desc)
    r.call(rx, 0, sync=False)
    r.call(rx, abi.TXP_UDP0_KEEP, sync=False)
    torch.cuda.synchronize()
    r.check(reference("corpus", buf, desc, abi.TXP_UDP0_KEEP))


def test_more_tiles_than_workgroups(rx):
    """2048 workgroups take the tiles of a larger batch in turns: 2048 * 256 + 300 descriptors that
    name the branch frames over and over (the planner only reads the frames)."""
    buf, desc, _, _ = txplan_cases.batch(abi.TXP_UDP0_KEEP)
    d1, o1, _ = reference("cases", buf, desc, abi.TXP_UDP0_KEEP)
    n = 2048 * 256 + 300
    reps = -(-n // len(desc))
    big = np.tile(desc, reps)[:n]
    oc = np.tile(o1, reps)[:n]
    info = np.zeros(abi.TXP_INFO_WORDS, np.uint64)
    info[:5] = np.bincount(oc, minlength=5)
    r = Run(buf, big, skew=11)
    r.call(rx, abi.TXP_UDP0_KEEP)
    r.check((np.tile(d1, reps)[:n], oc, info))


def test_return_codes(rx):
    import torch
    buf, desc, _, _ = txplan_cases.batch(0)
    r = Run(buf, desc)
    before = r.txd.clone()
    with pytest.raises(RuntimeError, match="invalid argument"):
        r.call(rx, 2)
    with pytest.raises(RuntimeError, match="-12"):
        r.call(rx, 0, n=(1 << 20) + 1)
    args = (r.frames.data_ptr(), r.desc.data_ptr(), r.n, 0, r.txd[GUARD:].data_ptr(), None, r.info[GUARD:].data_ptr())
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        rc = rx.lib.emurx_tx_plan_dev(rx.h, *args, s.cuda_stream)  # a capturing stream: refused before anything is enqueued
    assert rc == abi.EMURX_EINVAL
    torch.cuda.synchronize()
    assert torch.equal(r.txd, before)

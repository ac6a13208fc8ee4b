"""emurx_tx_checksum_dev (k_tx_csum, csrc/emurx_tx.hip) on both of its byte sources: the wave's
frames staged in LDS, and the wide path's header window per lane with cooperative span sums.

The batches are tx_cases' (arbitrary descriptors on the staged path, waves at 383 / 384 / 385
vectors, one long lane up to 65535 bytes, span lengths at the round edges, headers across the window
end, the end values of tcpipChecksum, ragged batches, empty descriptors, shuffled order); the expected
bytes are the C oracle's, which test_tx_ref.py holds equal to the independent tx_ref on the same
batches.  Each test first asserts with tx_cases.wave_paths, on the address the kernel is given, that
its waves take the path the case is built for.
"""
import numpy as np
import pytest

import tx_cases as C
from emurx import abi

pytestmark = pytest.mark.gpu
GUARD = 64
TAIL = 64


@pytest.fixture(scope="module")
def rx(gpu_ok, oracle_built):
    from emurx.rx import RxPath
    return RxPath(0, max_ns=16, max_clients=16, max_frames=256)


_want = {}


def expected(key, buf, d):
    """The oracle's buffer and status of a batch, computed once."""
    if key not in _want:
        import pyoracle
        out, st = pyoracle.tx_checksum(buf, d)
        out.setflags(write=False)
        st.setflags(write=False)
        _want[key] = (out, st)
    return _want[key]


class Run:
    """A batch on the device: d_frames `skew` bytes past a 16-byte boundary, 64 guard bytes on either
    side of the buffer, a status array 64 entries longer than n and filled with 0xEE."""

    def __init__(self, buf, d, skew, status=True):
        import torch
        self.n, self.size = len(d), len(buf)
        self.t = torch.zeros(16 + GUARD + len(buf) + GUARD + 16, dtype=torch.uint8, device="cuda")
        self.at = (skew - self.t.data_ptr() - GUARD) % 16 + GUARD       # d_frames within t
        img = np.zeros(self.t.numel(), np.uint8)
        img[self.at - GUARD:self.at] = 0x77
        img[self.at:self.at + len(buf)] = buf
        img[self.at + len(buf):self.at + len(buf) + GUARD] = 0x99
        self.img = img
        self.t.copy_(torch.from_numpy(img))
        self.frames = self.t[self.at:]
        self.addr = self.frames.data_ptr()
        assert self.addr % 16 == skew
        dd = np.ascontiguousarray(d).view(np.uint8).reshape(-1)
        self.desc = torch.zeros(dd.size + 16, dtype=torch.uint8, device="cuda")
        if dd.size:
            self.desc[:dd.size] = torch.from_numpy(dd.copy())
        self.status = torch.full((self.n + TAIL,), 0xEE, dtype=torch.uint8, device="cuda") if status else None

    def call(self, rx, n=None):
        import torch
        rx.tx_checksum_dev(self.frames, self.desc, self.n if n is None else n, self.status)
        torch.cuda.synchronize()

    def check(self, want, wst):
        """Status, every byte of the buffer (so range errors are untouched and only field bytes
        change), both guards and the status tail."""
        out = self.t.cpu().numpy()
        if self.status is not None:
            st = self.status.cpu().numpy()
            bad = np.nonzero(st[:self.n] != wst)[0]
            assert len(bad) == 0, (len(bad), bad[:10], st[bad[:10]])
            assert (st[self.n:] == 0xEE).all()
        got = out[self.at:self.at + self.size]
        diff = np.nonzero(got != want)[0]
        assert len(diff) == 0, (len(diff), diff[:10], got[diff[:10]], want[diff[:10]])
        assert (out[self.at - GUARD:self.at] == 0x77).all() and (out[self.at + self.size:][:GUARD] == 0x99).all()
        assert (out[:self.at - GUARD] == 0).all() and (out[self.at + self.size + GUARD:] == 0).all()


def run_case(rx, key, buf, d, skew, paths=None, status=True):
    r = Run(buf, d, skew, status)
    got = C.wave_paths(d, r.addr)
    if paths is not None:
        assert (got == paths) if isinstance(paths, list) else (set(got) == paths), (skew, got)
    r.call(rx)
    r.check(*expected(key, buf, d))
    return got


@pytest.mark.parametrize("skew", [0, 1, 15])
def test_staged_fuzz(rx, skew):
    """Arbitrary l3 / l4 / ops through TxLds: the fix() / seen() corrections of overlapping fields, the
    range verdicts, the next-header override and the zero-sum split, every wave staged."""
    buf, d = C.staged_fuzz()
    run_case(rx, "staged_fuzz", buf, d, skew, {"staged"})


@pytest.mark.parametrize("skew", [0, 1, 15])
def test_slab_boundary(rx, skew):
    """Waves of 383, 384 and 385 vectors (the vector count comes from the absolute address, so the
    same wave changes sides with the skew); workgroup 0 alternates staged and wide waves."""
    buf, d = C.slab_boundary()
    r = Run(buf, d, skew)
    nv = C.wave_nvec(d, r.addr)
    assert {383, 384, 385} <= set(nv), nv
    assert C.wave_paths(d, r.addr)[:4] == ["staged", "wide", "staged", "wide"]
    assert (nv[4] == 384) == (skew == 0) and (nv[6] == 384) == (skew != 15)
    r.call(rx)
    r.check(*expected("slab_boundary", buf, d))


def test_one_long_lane(rx):
    """One span of 1500, 9216 or 65535 bytes among 63 short ones at lane 0, 31, 63 (the row balance of
    coop_span_sum, up to 64 rounds, a half-sum near 2^31), and 64 spans of two rounds each."""
    buf, d = C.one_long_lane()
    run_case(rx, "one_long_lane", buf, d, 5, {"wide"})


@pytest.mark.parametrize("skew", range(16))
def test_span_rounds(rx, skew):
    buf, d = C.span_rounds()
    run_case(rx, "span_rounds", buf, d, skew, {"wide"})


@pytest.mark.parametrize("skew", range(16))
def test_window_edge(rx, skew):
    buf, d = C.window_edge()
    run_case(rx, "window_edge", buf, d, skew, {"wide"})


@pytest.mark.parametrize("skew", [0, 3])
def test_end_values(rx, skew):
    """Fields 0x0000 (a non-zero sum that is 0 modulo 0xffff; a zero span under a pseudo header that is
    0xffff) and 0xffff (a sum of exactly zero), and all-0xff frames, staged and wide."""
    buf, d, tags = C.end_values(tags=True)
    r = Run(buf, d, skew)
    paths = C.wave_paths(d, r.addr)
    seen = {"staged": set(), "wide": set()}
    for k, t in enumerate(tags):
        if t:
            seen[paths[k // 64]].add((t, int(d[k]["len"]), int(d[k]["ops"])))
    assert seen["staged"] == seen["wide"] and len(seen["staged"]) >= 180
    r.call(rx)
    want, wst = expected("end_values", buf, d)
    r.check(want, wst)
    out = r.t.cpu().numpy()[r.at:]
    for k, t in enumerate(tags):               # the device's own bytes, not only equality with the oracle
        if t in ("zero", "phz", "ffff"):
            f = int(d[k]["off"]) + int(d[k]["l4"]) + C.FIELD[int(d[k]["ops"]) >> 4]
            assert (int(out[f]) << 8 | int(out[f + 1])) == (0xFFFF if t == "ffff" else 0), (k, t)


@pytest.mark.parametrize("status", [True, False])
@pytest.mark.parametrize("n", C.RAGGED_NS)
def test_ragged_and_holes(rx, n, status):
    """n off the wave and workgroup sizes, len == 0 descriptors at lanes 0, 31, 63, a wave of nothing
    else; with d_status NULL the frames are rewritten all the same."""
    buf, d = C.ragged_and_holes(n)
    paths = run_case(rx, f"ragged_{n}", buf, d, 7, None, status)
    assert paths[0] == "staged" and (n < 192 or paths[2] == "wide")


def test_shuffled_order(rx):
    buf, d = C.shuffled_order()
    run_case(rx, "shuffled_order", buf, d, 9, ["staged", "staged", "wide", "wide"])


def test_n_zero(rx):
    """n == 0: EMURX_OK, no byte of the frames or of the status changes."""
    buf, d = C.ragged_and_holes(65)
    r = Run(buf, d, 3)
    r.call(rx, n=0)
    out = r.t.cpu().numpy()
    assert np.array_equal(out, r.img) and (r.status.cpu().numpy() == 0xEE).all()


def test_descriptor_alignment(rx):
    """The kernel takes each descriptor with one 16-byte load: a d_desc 8 bytes off is refused before
    any launch, and nothing is written."""
    buf, d = C.ragged_and_holes(65)
    r = Run(buf, d, 0)
    r.desc = r.desc[8:]
    with pytest.raises(RuntimeError, match="invalid argument"):
        r.call(rx, n=64)
    out = r.t.cpu().numpy()
    assert np.array_equal(out, r.img) and (r.status.cpu().numpy() == 0xEE).all()

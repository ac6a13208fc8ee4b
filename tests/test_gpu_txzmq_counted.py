"""GPU parity of the counted tx ZMQ framing (emurx_tx_zmq_counted_dev) against emurx_tx_zmq_dev
with n = min(count, n_max) on the same handle: d_out[:total], d_msg_off[:n_msgs + 1] and d_info
byte for byte, at the tile (64), unit (4,096) and second-level edges of n_max and of the count,
with the descriptors and frame bytes past the count poisoned and guard words around every
output; and the arrival counters clean between calls of different layouts."""
import numpy as np
import pytest

import txzmq_util as U

pytestmark = pytest.mark.gpu

GUARD = 64      # guard bytes before d_out (keeps it 16-byte aligned) and guard words behind the u64 outputs
POISON = 0xA5   # frame bytes past the count


@pytest.fixture(scope="module")
def rx(gpu_ok):
    from emurx.rx import RxPath
    r = RxPath(0, max_ns=16, max_clients=16, max_frames=1 << 10)
    yield r
    r.close()


def poisoned(buf, d, c):
    """The batch with everything past frame c replaced: descriptors of the largest offsets and
    lengths, the frames' bytes by a pattern."""
    b, p = buf.copy(), d.copy()
    if c < len(d):
        b[int(d["off"][c]):] = POISON
        p["off"][c:], p["len"][c:], p["vport"][c:], p["pad"][c:] = 0xFFFFFFF0, 0xFFFF, 0xFF, 0xFF
    return b, p


def plain(rx, tb, td, c, cap):
    import torch
    out = torch.full((max(cap, 1),), 0xEE, dtype=torch.uint8, device="cuda")
    off = torch.full((c + 1,), -1, dtype=torch.int64, device="cuda")
    info = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    rx.tx_zmq_dev(tb, td, c, out, cap, off, info)
    return out, off, info


class Counted:
    """One counted call's buffers with their guards; check() compares them with a plain call's."""

    def __init__(self, rx, tb, td, n_max, count, cap, stream=None):
        import torch
        self.n_max, self.cap = n_max, cap
        self.raw = torch.full((GUARD + max(cap, 1) + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
        self.off = torch.full((n_max + 1 + GUARD,), -1, dtype=torch.int64, device="cuda")
        self.info = torch.full((2 + GUARD,), -1, dtype=torch.int64, device="cuda")
        self.cnt = torch.tensor([count], dtype=torch.int64, device="cuda")
        rx.tx_zmq_counted_dev(tb, td, n_max, self.cnt, self.raw[GUARD:], cap, self.off, self.info, stream=stream)

    def check(self, want, tag):
        wout, woff, winfo = (x.cpu().numpy() for x in want)
        nm, total = (int(x) for x in winfo)
        raw, off, info = self.raw.cpu().numpy(), self.off.cpu().numpy(), self.info.cpu().numpy()
        assert info[:2].tolist() == [nm, total], tag
        assert (info[2:] == -1).all(), tag
        assert np.array_equal(off[: nm + 1], woff[: nm + 1]), tag
        assert (off[nm + 1:] == -1).all(), tag                      # nothing past d_msg_off[n_msgs]
        assert (raw[:GUARD] == 0xEE).all(), tag                     # nothing before d_out
        assert raw[GUARD: GUARD + total].tobytes() == wout[:total].tobytes(), tag
        assert (raw[GUARD + total:] == 0xEE).all(), tag             # nothing past the total


def counts_of(n_max):
    return sorted({c for c in (0, 1, 63, 64, 65, n_max - 1, n_max) if 0 <= c <= n_max}) + [n_max + 1000]


@pytest.mark.parametrize("n_max,kind", [(1, 0), (64, 0), (65, 1), (4096, 0), (4097, 2), (8300, 0)])
def test_counted_matches_plain(rx, n_max, kind):
    import torch
    from gpu_util import to_dev
    buf, d = U.batch(n_max, kind, seed=7)
    cap = 8 * n_max + int(d["len"].astype(np.int64).sum())
    tb, td = to_dev(buf), to_dev(d)
    for count in counts_of(n_max):
        c = min(count, n_max)
        want = plain(rx, tb, td, c, cap)
        pb, pd = poisoned(buf, d, c)
        got = Counted(rx, to_dev(pb), to_dev(pd), n_max, count, cap)
        torch.cuda.synchronize()
        got.check(want, (n_max, count))


def test_counted_thresholds(rx):
    """The frames that land on the 32 KiB rule and the 64-frame burst, cut at every message edge."""
    import torch
    from gpu_util import to_dev
    buf, d = U.threshold_batch()
    n_max = len(d)
    cap = 8 * n_max + int(d["len"].astype(np.int64).sum())
    tb, td = to_dev(buf), to_dev(d)
    for count in (0, 1, 2, 5, 9, 12, 76, 77, 140, 142, 143, n_max - 1, n_max):
        want = plain(rx, tb, td, count, cap)
        pb, pd = poisoned(buf, d, count)
        got = Counted(rx, to_dev(pb), to_dev(pd), n_max, count, cap)
        torch.cuda.synchronize()
        got.check(want, count)


def test_counted_zero_n_max(rx):
    import torch
    t = torch.zeros(64, dtype=torch.uint8, device="cuda")
    got = Counted(rx, t, t, 0, 5, 0)
    torch.cuda.synchronize()
    assert got.info.cpu().numpy()[:2].tolist() == [0, 0] and int(got.off.cpu()[0]) == 0
    assert (got.off.cpu().numpy()[1:] == -1).all() and (got.raw.cpu().numpy() == 0xEE).all()


def test_counted_capacity(rx):
    """Nothing at or past out_cap, and d_info tells the size needed."""
    import torch
    from gpu_util import to_dev
    buf, d = U.batch(3000, 2, seed=4)
    count = 2000
    need = 8 * count + int(d["len"][:count].astype(np.int64).sum())
    tb, td = to_dev(buf), to_dev(d)
    want = plain(rx, tb, td, count, need)
    pb, pd = poisoned(buf, d, count)
    cap = (need // 3) & ~15
    got = Counted(rx, to_dev(pb), to_dev(pd), len(d), count, cap)
    torch.cuda.synchronize()
    raw = got.raw.cpu().numpy()
    assert got.info.cpu().numpy()[:2].tolist() == want[2].cpu().numpy().tolist()
    assert raw[GUARD: GUARD + cap].tobytes() == want[0].cpu().numpy()[:cap].tobytes()
    assert (raw[GUARD + cap:] == 0xEE).all() and (raw[:GUARD] == 0xEE).all()


def test_counted_back_to_back(rx):
    """Counted calls of different n_max (2, 3 and 4 levels: every workgroup of the n_max-sized grid
    makes its arrival, the last one resets the counter) enqueued without a synchronisation
    between them, then a plain call: each result is its own, so the counters were zero again."""
    import torch
    from gpu_util import to_dev
    big, dbig = U.batch(3000, 0, seed=31)
    n_huge = 64 * 4096 + 7
    dhuge = np.zeros(n_huge, dbig.dtype)
    dhuge[:3000] = dbig
    cap = 8 * 3000 + int(dbig["len"].astype(np.int64).sum())
    tb, td = to_dev(big), to_dev(dbig)
    calls = [(8300, 2500), (65, 65), (n_huge, 1000), (4097, 0), (n_huge, 3000)]
    wants = [plain(rx, tb, td, min(c, 3000), cap) for _, c in calls]
    wlast = plain(rx, tb, td, 3000, cap)
    torch.cuda.synchronize()
    tds = []
    for n_max, c in calls:
        _, pd = poisoned(big, dhuge[:n_max], c)
        tds.append(to_dev(pd))
    torch.cuda.synchronize()
    gots = [Counted(rx, tb, tds[i], n_max, c, cap) for i, (n_max, c) in enumerate(calls)]
    last = plain(rx, tb, td, 3000, cap)
    torch.cuda.synchronize()
    for g, w, call in zip(gots, wants, calls):
        g.check(w, call)
    for a, b in zip(last, wlast):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


def test_counted_after_responder_info_shape(rx):
    """d_count is the first word of a longer info block (the responder's): only word 0 is read."""
    import torch
    from gpu_util import to_dev
    from emurx import abi
    buf, d = U.batch(500, 0, seed=9)
    cap = 8 * 500 + int(d["len"].astype(np.int64).sum())
    tb, td = to_dev(buf), to_dev(d)
    info = torch.full((abi.RSP_INFO_WORDS,), 1 << 40, dtype=torch.int64, device="cuda")
    info[0] = 130
    want = plain(rx, tb, td, 130, cap)
    out = torch.full((cap,), 0xEE, dtype=torch.uint8, device="cuda")
    off = torch.full((501,), -1, dtype=torch.int64, device="cuda")
    zi = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    rx.tx_zmq_counted_dev(tb, td, 500, info, out, cap, off, zi)
    torch.cuda.synchronize()
    assert zi.cpu().numpy().tolist() == want[2].cpu().numpy().tolist()
    assert out.cpu().numpy().tobytes() == want[0].cpu().numpy().tobytes()

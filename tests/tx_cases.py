"""Seeded tx checksum batches for emurx_tx_checksum_dev (k_tx_csum, csrc/emurx_tx.hip), shared by
the CPU test of the two references (test_tx_ref.py) and the GPU test (test_gpu_tx_checksum.py).

Every generator returns (buf, desc): a uint8 frame buffer and abi.TX_DESC_DTYPE descriptors, the
same arrays on every call (cached: copy before changing them).  wave_paths restates the kernel's
documented choice of byte source per wave of 64 descriptors, so a test can assert that a case
reaches the path it is built for without asking the kernel.
"""
import functools

import numpy as np

from emurx import abi

WAVE = 64
SLAB_VEC = 384          # kTxSlab / 16: the most 16-byte vectors a staged wave spans
HDR, NH, SH = abi.TX_IPV4_HDR, abi.TX_V6_NH, abi.TX_L4_SHIFT
TCP4, UDP4, TCP6, UDP6, ICMP6, ICMP4 = (abi.TX_L4_TCP4, abi.TX_L4_UDP4, abi.TX_L4_TCP6, abi.TX_L4_UDP6,
                                        abi.TX_L4_ICMP6, abi.TX_L4_ICMP4)
KINDS = (TCP4, UDP4, TCP6, UDP6, ICMP6, ICMP4)
FIELD = {TCP4: 16, UDP4: 6, TCP6: 16, UDP6: 6, ICMP6: 2, ICMP4: 2}
V6 = (TCP6, UDP6, ICMP6)
L3 = 14                 # the usual Ethernet header


def wave_nvec(desc, base_addr: int):
    """Per wave of 64 descriptors: the 16-byte vectors its frames' byte range spans, from the
    aligned vector of the absolute address base_addr + lo (0 when the range is empty)."""
    out = []
    for w in range(0, len(desc), WAVE):
        d = desc[w:w + WAVE]
        lo = int(d["off"].min())
        hi = int((d["off"].astype(np.int64) + d["len"]).max())
        out.append((hi - lo + ((base_addr + lo) & 15) + 15) >> 4 if hi > lo else 0)
    return out


def wave_paths(desc, base_addr: int):
    """'staged' (0 < nvec <= 384: the wave's range copied into its 6 KiB LDS slab) or 'wide' (a
    header window per lane, spans summed cooperatively) for every wave of 64 descriptors."""
    return ["staged" if 0 < v <= SLAB_VEC else "wide" for v in wave_nvec(desc, base_addr)]


class _Batch:
    """Frames appended at chosen gaps; descriptors alongside."""

    def __init__(self):
        self.buf = bytearray()
        self.rows = []

    def pad_to(self, mod16: int):
        while len(self.buf) % 16 != mod16:
            self.buf.append(0x5A)

    def add(self, frame, l3=0, l4=0, osize=0, ops=0, nh=0, gap=0):
        self.buf += bytes([0x5A]) * gap
        self.rows.append((len(self.buf), len(frame), l3, l4, osize, ops, nh, (0, 0)))
        self.buf += bytes(frame)

    def hole(self, ops=0):
        """A len == 0 descriptor at the current end of the buffer."""
        self.rows.append((len(self.buf), 0, L3, L3 + 20, 0, ops, 0, (0, 0)))

    def fill_wave(self):
        """len == 0, ops == 0 descriptors up to the next multiple of 64."""
        while len(self.rows) % WAVE:
            self.hole()

    def done(self):
        d = np.zeros(len(self.rows), abi.TX_DESC_DTYPE)
        for k, r in enumerate(self.rows):
            d[k] = r
        buf = np.frombuffer(bytes(self.buf) + bytes([0x5A]) * 16, np.uint8).copy()
        buf.setflags(write=False)
        d.setflags(write=False)
        return buf, d


def _rand(rng, n: int) -> bytearray:
    return bytearray(rng.integers(0, 256, n, dtype=np.uint8).tobytes())


def _l4_of(kind: int, l3: int = L3) -> int:
    return l3 + (40 if kind in V6 else 20)


def _short(rng, ln: int = 60):
    """A short random frame with an op whose slices fit 60 bytes."""
    f = _rand(rng, ln)
    f[L3] = 0x45
    kind = (TCP4, UDP4, ICMP4)[int(rng.integers(0, 3))]
    return f, dict(l3=L3, l4=L3 + 20, ops=HDR | (kind << SH))


def _long(rng, ln: int, kind: int):
    f = _rand(rng, ln)
    f[L3] = 0x60 if kind in V6 else 0x45
    return f, dict(l3=L3, l4=_l4_of(kind), ops=(0 if kind in V6 else HDR) | (kind << SH))


# ---- arbitrary descriptors on the staged path -----------------------------------------------------
@functools.lru_cache(None)
def staged_fuzz(n: int = 4099):
    """Short frames (0..95 bytes, 0..3 bytes apart), arbitrary l3 / l4 / ops / osize / nh: overlapping
    fields, slices out of range, the invalid kind 7, the next-header override; every 7th frame zero."""
    rng = np.random.default_rng(0x7C54)
    b = _Batch()
    for k in range(n):
        ln = int(rng.integers(0, 96))
        f = bytes(ln) if k % 7 == 0 else _rand(rng, ln)
        l3 = int(rng.integers(0, 24))
        l4 = l3 + (20, 24, 40)[int(rng.integers(0, 3))] if rng.random() < 0.7 else int(rng.integers(0, 60))
        ops = int(rng.integers(0, 4)) | (int(rng.integers(0, 8)) << SH)
        osize = int(rng.integers(0, 16)) if rng.random() < 0.75 else int(rng.integers(0, 65536))
        b.add(f, l3, l4, osize, ops, int(rng.integers(0, 256)), gap=int(rng.integers(0, 4)))
    return b.done()


# ---- the rule that chooses the path ---------------------------------------------------------------
# byte ranges of one wave; with the wave's first byte s bytes past a 16-byte boundary it spans
# (range + s + 15) >> 4 vectors: 6113 -> 383 for every s; 6129 -> 384 for every s; 6145 and 6160 ->
# 385 or 386; 6144 -> 384 at s == 0 only; 6128 -> 383 at s == 0, else 384; 6130 -> 384 up to s == 14
SLAB_RANGES = ((6113, 6145, 6129, 6160),      # staged, wide, staged, wide wherever d_frames lies
               (6144, 6128, 6130, 6113),      # the sides of 384 move with the address
               (6144, 6128, 6130, 6129))


@functools.lru_cache(None)
def slab_boundary():
    """Three workgroups of four full waves of contiguous frames; a wave's range is one of SLAB_RANGES.
    The waves of the first two workgroups start on a 16-byte boundary of the buffer, those of the
    third 9 bytes past one."""
    rng = np.random.default_rng(0x51AB)
    b = _Batch()
    for g, ranges in enumerate(SLAB_RANGES):
        for span in ranges:
            b.pad_to(9 if g == 2 else 0)
            for i in range(WAVE):
                ln = span // WAVE + (i < span % WAVE)
                kind = KINDS[int(rng.integers(0, 6))]
                b.add(_rand(rng, ln), L3, _l4_of(kind), int(rng.integers(0, 4)),
                      int(rng.integers(0, 4)) | (kind << SH), int(rng.integers(0, 256)))
    return b.done()


# ---- long spans -------------------------------------------------------------------------------------
LONG_LENS = (1500, 9216, 65535)


@functools.lru_cache(None)
def one_long_lane():
    """Waves of 63 frames of 60 bytes and one long frame (1500, 9216 or 65535 bytes; UDP4 with the
    header op, and TCP6) at lane 0, 31 or 63; then one wave of 64 frames of 2000 bytes.  Frames lie
    16 bytes apart, so that the wave with the 1500-byte frame exceeds the slab as well."""
    rng = np.random.default_rng(0x10A6)
    b = _Batch()
    for ln in LONG_LENS:
        for lane in (0, 31, 63):
            for kind in (UDP4, TCP6):
                for i in range(WAVE):
                    f, kw = _long(rng, ln, kind) if i == lane else _short(rng)
                    b.add(f, gap=16, **kw)
    for i in range(WAVE):
        f, kw = _long(rng, 2000, KINDS[i % 6])
        b.add(f, gap=16, **kw)
    return b.done()


SPAN_LENS = (1, 15, 16, 17, 1023, 1024, 1025, 2047, 2048, 2049)


@functools.lru_cache(None)
def span_rounds():
    """Two wide waves (one 9000-byte frame each) of frames whose L4 span p[l4:len] has a length at an
    edge of coop_span_sum's 64-vector (1 KiB) round, for all six kinds; l3 = 14 in the first wave, 15
    in the second.  Spans too short for the kind's field are range errors and stay."""
    rng = np.random.default_rng(0x5BA2)
    b = _Batch()
    for l3 in (L3, L3 + 1):
        f, kw = _long(rng, 9000, TCP4)
        b.add(f, **kw)
        for span in SPAN_LENS:
            for kind in KINDS:
                l4 = _l4_of(kind, l3)
                f = _rand(rng, l4 + span)
                f[l3] = 0x60 if kind in V6 else 0x45
                b.add(f, l3, l4, 0, (HDR if kind in (TCP4, UDP4) and span & 1 else 0) | (kind << SH), 0)
        for _ in range(3):
            f, kw = _short(rng)
            b.add(f, **kw)
    assert len(b.rows) == 2 * WAVE
    return b.done()


# ---- the end of a lane's header window --------------------------------------------------------------
@functools.lru_cache(None)
def window_edge():
    """200-byte frames (every wave wide), l3 = 40..100: a wide wave's lane holds frame bytes
    [0, 96 - head) in LDS (head = the frame's address mod 16) and reads the rest from global memory, so
    over these l3 and the 16 address skews the IPv4 / IPv6 header, the pseudo header's addresses and
    the L4 field each straddle the window's end.  Per l3: every kind at its usual l4 (IPv4 kinds with
    and without the header op), the header op alone, and L4 spans that start where another sum starts
    (l4 == l3, l3 + 8, l3 + 12) or put the field on the header checksum (l4 + 2 == l3 + 10, l3 + 11)."""
    rng = np.random.default_rng(0xED6E)
    b = _Batch()

    def add(l3, l4, ops, ihl=5):
        f = _rand(rng, 200)
        f[l3] = 0x40 | ihl
        b.add(f, l3, l4, int(rng.integers(0, 8)), ops, int(rng.integers(0, 256)))

    for l3 in range(40, 101):
        for kind in KINDS:
            add(l3, _l4_of(kind, l3), kind << SH)
        for kind in (TCP4, UDP4, ICMP4):
            add(l3, _l4_of(kind, l3), HDR | (kind << SH), ihl=5 + l3 % 3)
        add(l3, 0, HDR, ihl=6)
        add(l3, _l4_of(ICMP6, l3), NH | (ICMP6 << SH))
        add(l3, l3, HDR | (UDP4 << SH))
        add(l3, l3, HDR | (ICMP4 << SH))
        add(l3, l3 + 12, TCP4 << SH)
        add(l3, l3 + 8, UDP6 << SH)
        add(l3, l3 + 8, HDR | (ICMP4 << SH))
        add(l3, l3 + 9, HDR | (ICMP4 << SH))
        for kind in V6:                           # the field right behind the IPv6 header (at the usual
            add(l3, l3 + 40 - FIELD[kind], kind << SH)   # l4 TCP6's lies past every window)
    while len(b.rows) % WAVE:                     # a short last wave would fit the slab
        add(40 + len(b.rows) % 61, 0, HDR)
    return b.done()


# ---- the end values of tcpipChecksum ----------------------------------------------------------------
END_LENS = (80, 81, 200, 201, 1500)


def _end_frames():
    """[(tag, frame, descriptor fields)]: tag 'zero' = one payload word set so that the L4 sum is a
    non-zero multiple of 0xffff (field 0x0000), 'ffff' = an all-zero frame whose sum is exactly zero
    (field 0xffff), 'phz' = a zero span under a pseudo header that is 0xffff (field 0x0000), 'ff' =
    all bytes 0xff."""
    import tx_ref
    rng = np.random.default_rng(0xE4D5)
    out = []
    for kind in KINDS:
        l4 = _l4_of(kind)
        for hdr in (0, HDR):
            ops = hdr | (kind << SH)
            for ln in END_LENS:
                # the word at l4 + 20 lies behind every field and header (IHL 5 / 0: 20 bytes) and an
                # even count of bytes into the span: with it zero the field would be c = 0xffff -
                # fold(sum), so the word c brings the sum to 0 modulo 0xffff
                f = _rand(rng, ln)
                f[L3] = 0x60 if kind in V6 else 0x45
                f[l4 + 20:l4 + 22] = b"\0\0"
                p = bytearray(f)
                assert tx_ref.tx_frame(p, L3, l4, 0, ops, 0) == abi.TX_OK
                f[l4 + 20:l4 + 22] = p[l4 + FIELD[kind]:l4 + FIELD[kind] + 2]
                out.append(("zero", f, dict(l3=L3, l4=l4, ops=ops)))
                # the header op on an all-zero IPv6 frame writes ff ff into the source address
                out.append(("phz" if hdr and kind in V6 else "ffff", bytes(ln), dict(l3=L3, l4=l4, ops=ops)))
                out.append(("ff", b"\xff" * ln, dict(l3=L3, l4=l4, ops=ops)))
    for kind in (TCP4, UDP4):
        for hdr in (0, HDR):
            f = bytearray(80)
            f[L3 + 12:L3 + 14] = b"\xff\xff"      # IPv4 source ff ff 00 00: the pseudo header sums to 0xffff
            out.append(("phz", f, dict(l3=L3, l4=L3 + 20, ops=hdr | (kind << SH))))
    return out


@functools.lru_cache(None)
def end_values(tags: bool = False):
    """The frames of _end_frames twice: first in waves that fit the slab (at most 6000 bytes, filled
    up to 64 descriptors with len == 0 ones), then in waves of 63 beside a 9000-byte frame.  With
    tags, also the tag of every descriptor ('' for the fillers)."""
    rng = np.random.default_rng(0xE4D6)
    b, tg = _Batch(), []
    room = 0
    for tag, f, kw in _end_frames():
        if len(f) > room or len(b.rows) % WAVE == 0:
            b.fill_wave()
            room = 6000
        b.add(f, **kw)
        room -= len(f)
        tg += [""] * (len(b.rows) - 1 - len(tg)) + [tag]
    b.fill_wave()
    for k, (tag, f, kw) in enumerate(_end_frames()):
        if k % (WAVE - 1) == 0:
            b.fill_wave()
            g, gkw = _long(rng, 9000, UDP4)
            b.add(g, **gkw)
        b.add(f, **kw)
        tg += [""] * (len(b.rows) - 1 - len(tg)) + [tag]
    buf, d = b.done()
    tg += [""] * (len(d) - len(tg))
    return (buf, d, tuple(tg)) if tags else (buf, d)


# ---- ragged batches, empty descriptors, descriptor order ----------------------------------------------
RAGGED_NS = (1, 63, 64, 65, 255, 256, 257)


@functools.lru_cache(None)
def ragged_and_holes(n: int):
    """n descriptors of 60-byte frames; len == 0 descriptors at lanes 0, 31 and 63 of wave 0 (those
    below n, n > 1), the first with an op (a range error) and the others without; wave 2, where n
    reaches it, made of len == 0 descriptors only."""
    rng = np.random.default_rng(0x4A66 + n)
    b = _Batch()
    for i in range(n):
        if (n > 1 and i in (0, 31, 63)) or i // WAVE == 2:
            b.hole(ops=(HDR | (UDP4 << SH)) if i % WAVE == 0 else 0)
        else:
            f, kw = _short(rng)
            b.add(f, gap=int(rng.integers(0, 4)), **kw)
    return b.done()


@functools.lru_cache(None)
def shuffled_order():
    """256 disjoint 60-byte frames; the descriptors of waves 0 and 1 are a permutation of the frames of
    their own 64 (the wave's range still fits the slab), those of waves 2 and 3 a permutation of the
    last 128 frames (each wave's range is about 7.5 KiB)."""
    rng = np.random.default_rng(0x5FF1)
    b = _Batch()
    for _ in range(256):
        f, kw = _short(rng)
        b.add(f, **kw)
    buf, d = b.done()
    perm = np.concatenate([rng.permutation(64), 64 + rng.permutation(64), 128 + rng.permutation(128)])
    d = d[perm].copy()
    d.setflags(write=False)
    return buf, d


def fuzz_20000():
    """The batch of test_gpu_parity.test_tx_checksum_fuzz_vs_oracle: the same seed and draws."""
    from emurx import frames as F
    rng = np.random.default_rng(0x7C5)
    n = 20000
    lens = rng.integers(0, 1600, n)
    frames = [rng.integers(0, 256, int(l), dtype=np.uint8).tobytes() for l in lens]
    for k in range(0, n, 7):
        frames[k] = bytes(len(frames[k]))
    buf, desc = F.pack_frames(frames, header=int(rng.integers(0, 4)))
    d = np.zeros(n, abi.TX_DESC_DTYPE)
    d["off"], d["len"] = desc["off"], desc["len"]
    d["l3"] = rng.integers(0, 60, n)
    d["l4"] = np.where(rng.random(n) < 0.8, d["l3"] + rng.choice([20, 24, 40, 48], n), rng.integers(0, 80, n))
    d["osize"] = rng.integers(0, 16, n)
    d["ops"] = rng.integers(0, 4, n) | (rng.integers(0, 8, n) << abi.TX_L4_SHIFT)
    d["nh"] = rng.integers(0, 256, n)
    return buf, d

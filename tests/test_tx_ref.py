"""The two tx checksum references against each other, and the conditions the batches of tx_cases
are built for, from the references alone (no GPU).

tx_ref (plain Python, the Go statements in their order) and the C oracle's orc_tx_checksum were
written apart; they must agree byte for byte and status for status on every batch the GPU test uses,
on the reference's captures and on the 20 000-frame fuzz of test_gpu_parity.
"""
import numpy as np
import pytest

import tx_cases as C
import tx_ref
from emurx import abi

OK, RANGE = abi.TX_OK, abi.TX_RANGE

BATCHES = {
    "staged_fuzz": C.staged_fuzz,
    "slab_boundary": C.slab_boundary,
    "one_long_lane": C.one_long_lane,
    "span_rounds": C.span_rounds,
    "window_edge": C.window_edge,
    "end_values": C.end_values,
    "shuffled_order": C.shuffled_order,
    "fuzz_20000": C.fuzz_20000,
    **{f"ragged_{n}": (lambda n=n: C.ragged_and_holes(n)) for n in C.RAGGED_NS},
}


def both(buf, d):
    import pyoracle
    want, wst = pyoracle.tx_checksum(buf, d)
    got, st = tx_ref.tx_checksum(buf, d)
    bad = np.nonzero(st != wst)[0]
    assert len(bad) == 0, (len(bad), d[bad[:5]], st[bad[:5]], wst[bad[:5]])
    diff = np.nonzero(got != want)[0]
    assert len(diff) == 0, (len(diff), diff[:10])
    return got, st


@pytest.mark.parametrize("name", list(BATCHES))
def test_tx_ref_equals_oracle(oracle_built, name):
    buf, d = BATCHES[name]()
    got, st = both(buf, d)
    for k in np.nonzero(st == RANGE)[0]:  # a range error leaves the frame as it was
        o, n = int(d[k]["off"]), int(d[k]["len"])
        assert got[o:o + n].tobytes() == buf[o:o + n].tobytes(), k


def test_tx_ref_equals_oracle_on_captures(oracle_built):
    """The reference's own captures: both references rebuild the bytes the send paths wrote."""
    import tx_util
    buf, d, want, zeroed = tx_util.corpus_tx_cases()
    got, st = both(zeroed, d)
    assert (st == OK).all() and got.tobytes() == want.tobytes()


def test_tx_ref_kat():
    """tcpip_test.go:15-19 (0xbc5f) through tx_ref alone."""
    import kat_frames as K
    f, _, _ = K.tcpip_ipv4_udp()
    p = bytearray(f)
    p[40:42] = b"\0\0"
    assert tx_ref.tx_frame(p, 14, 34, 0, abi.TX_IPV4_HDR | (abi.TX_L4_UDP4 << abi.TX_L4_SHIFT), 0) == OK
    assert (p[40] << 8 | p[41]) == K.IPV4_UDP_CSUM and bytes(p) == bytes(f)
    q = bytearray(f[:30])
    assert tx_ref.tx_frame(q, 14, 34, 0, abi.TX_L4_UDP4 << abi.TX_L4_SHIFT, 0) == RANGE and bytes(q) == f[:30]


def test_wave_paths_rule():
    """wave_paths on hand-made waves: 64 x 96 contiguous bytes are 384 vectors at an aligned address
    and 385 one byte further; an empty wave is not staged."""
    d = np.zeros(130, abi.TX_DESC_DTYPE)
    d["off"][:64] = np.arange(64) * 96
    d["len"][:64] = 96
    d["off"][64:128] = 7000 + np.arange(64) * 95       # 6080 bytes from 7000 (8 mod 16): 381 vectors at 0
    d["len"][64:128] = 95
    d["off"][128:] = 99999                             # len 0: no range
    assert C.wave_nvec(d, 0x1000) == [384, 381, 0] and C.wave_paths(d, 0x1000) == ["staged", "staged", "wide"]
    assert C.wave_nvec(d, 0x1001) == [385, 381, 0] and C.wave_paths(d, 0x1001) == ["wide", "staged", "wide"]
    assert C.wave_nvec(d, 0x1008) == [385, 380, 0]      # 7000 + 8 is a boundary: (6080 + 0 + 15) >> 4


# ---- what each batch is built for -----------------------------------------------------------------
def test_staged_fuzz_conditions():
    buf, d = C.staged_fuzz()
    _, st = tx_ref.tx_checksum(buf, d)
    n = len(d)
    assert n == 4099 and (st == OK).sum() * 3 >= n and (st == RANGE).sum() * 3 >= n
    kind = d["ops"] >> abi.TX_L4_SHIFT
    assert set(d["ops"].tolist()) >= {a | (k << 4) for a in range(4) for k in range(8)}
    assert (st[kind == 7] == RANGE).all()
    inside = near = 0
    for x, s in zip(d.tolist(), st):
        l3, l4, ops = x[2], x[3], x[5]
        if s != OK or not ops & abi.TX_IPV4_HDR or not ops >> 4:
            continue
        fo = l4 + tx_ref.FIELD[ops >> 4]
        inside += l3 <= fo < l3 + 20
        near += abs(fo - (l3 + 10)) <= 1
    assert inside >= 20 and near >= 5, (inside, near)
    for skew in range(16):
        assert set(C.wave_paths(d, 0x7000 + skew)) == {"staged"}, skew


def test_slab_boundary_conditions():
    buf, d = C.slab_boundary()
    assert len(d) == 12 * 64
    for skew in (0, 1, 15):
        nv = C.wave_nvec(d, 0x7000 + skew)
        assert {383, 384, 385} <= set(nv), (skew, nv)
        paths = C.wave_paths(d, 0x7000 + skew)
        assert paths[:4] == ["staged", "wide", "staged", "wide"], (skew, paths)   # one workgroup, both paths
        assert any(v <= 384 for v in nv[4:]) and any(v > 384 for v in nv[4:])
    # the same wave on either side of the limit as the address moves
    assert C.wave_nvec(d, 0x7000)[4] == 384 and C.wave_nvec(d, 0x7001)[4] == 385
    assert C.wave_nvec(d, 0x700E)[6] == 384 and C.wave_nvec(d, 0x700F)[6] == 385


@pytest.mark.parametrize("name", ["one_long_lane", "span_rounds", "window_edge"])
def test_wide_batches_are_wide(name):
    buf, d = BATCHES[name]()
    assert len(d) % 64 == 0
    for skew in range(16):
        assert set(C.wave_paths(d, 0x7000 + skew)) == {"wide"}, skew


def test_one_long_lane_conditions():
    buf, d = C.one_long_lane()
    _, st = tx_ref.tx_checksum(buf, d)
    assert (st == OK).all()
    w = d["len"].reshape(-1, 64)
    assert w.shape[0] == 19 and (w[18] == 2000).all()
    seen = set()
    for row in w[:18]:
        lane = int(row.argmax())
        assert sorted(np.delete(row, lane).tolist()) == [60] * 63
        seen.add((int(row[lane]), lane))
    assert seen == {(ln, lane) for ln in C.LONG_LENS for lane in (0, 31, 63)}


def test_span_rounds_conditions():
    buf, d = C.span_rounds()
    _, st = tx_ref.tx_checksum(buf, d)
    span = (d["len"].astype(int) - d["l4"])
    kind = d["ops"] >> abi.TX_L4_SHIFT
    for k in C.KINDS:
        got = set(span[kind == k].tolist())
        assert got >= set(C.SPAN_LENS), (k, got)
        fits = (kind == k) & (span >= C.FIELD[k] + 2)
        assert (st[fits] == OK).all() and (st[(kind == k) & ~fits] == RANGE).all()
    # span 1: every kind; span 15, 16, 17: TCP alone
    assert (st == RANGE).sum() == ((span == 1).sum() + ((span >= 15) & (span <= 17) & np.isin(kind, (1, 3))).sum())


def test_window_edge_conditions():
    """For every window end 81..96 (head 15..0) some l3 puts the header, the addresses and the field
    across it."""
    buf, d = C.window_edge()
    _, st = tx_ref.tx_checksum(buf, d)
    assert (st == OK).all() and (d["len"] == 200).all()
    l3, l4, ops = d["l3"].astype(int), d["l4"].astype(int), d["ops"].astype(int)
    assert set(l3.tolist()) == set(range(40, 101))
    for wlim in range(81, 97):
        for k in C.KINDS:
            fo = l4 + C.FIELD[k]
            sel = (ops >> 4) == k
            assert (sel & (fo + 1 == wlim)).any(), (wlim, k)               # the field's two bytes on either side
            a = 8 if k in C.V6 else 12
            if k != C.ICMP4:
                assert (sel & (l3 + a < wlim) & (wlim < l3 + (40 if k in C.V6 else 20))).any(), (wlim, k)
        hdr = (ops & abi.TX_IPV4_HDR) != 0
        assert (hdr & (l3 < wlim) & (wlim < l3 + 20)).any() and (hdr & (l3 + 11 == wlim)).any(), wlim


def test_end_values_conditions():
    buf, d, tags = C.end_values(tags=True)
    out, st = tx_ref.tx_checksum(buf, d)
    tags = np.array(tags)
    assert (st == OK).all()
    count = {t: int((tags == t).sum()) for t in ("zero", "ffff", "phz", "ff")}
    assert count == {"zero": 2 * 60, "ffff": 2 * 45, "phz": 2 * (15 + 4), "ff": 2 * 60}, count
    for k in np.nonzero(tags != "")[0]:
        v = tx_ref.field_value(out, d[k])
        if tags[k] in ("zero", "phz"):
            assert v == 0x0000, (k, tags[k], hex(v), d[k])
        elif tags[k] == "ffff":
            assert v == 0xFFFF, (k, hex(v), d[k])
    # a crafted frame is not a zero frame: its span holds non-zero bytes, so 0x0000 is the folded end
    k = int(np.nonzero(tags == "zero")[0][0])
    assert buf[int(d[k]["off"]) + int(d[k]["l4"]):int(d[k]["off"]) + int(d[k]["len"])].any()
    # all-ff headers: the header checksum's own 0x0000 end
    for k in np.nonzero((tags == "ff") & ((d["ops"] & abi.TX_IPV4_HDR) != 0))[0]:
        o = int(d[k]["off"]) + int(d[k]["l3"]) + 10
        assert out[o] == 0 and out[o + 1] == 0
    for skew in range(16):                               # the first copy staged, the second wide
        paths = C.wave_paths(d, 0x7000 + skew)
        seen = {"staged": set(), "wide": set()}
        for w, p in enumerate(paths):
            for k in range(w * 64, min((w + 1) * 64, len(d))):
                if tags[k]:
                    seen[p].add((tags[k], int(d[k]["len"]), int(d[k]["ops"])))
        assert seen["staged"] == seen["wide"] and len(seen["staged"]) >= 3 * 60, skew


def test_ragged_and_shuffled_conditions():
    for n in C.RAGGED_NS:
        buf, d = C.ragged_and_holes(n)
        assert len(d) == n
        if n >= 64:
            assert (d["len"][[0, 31, 63]] == 0).all() and d["len"][:64].astype(bool).sum() == 61
        if n >= 192:
            assert (d["len"][128:192] == 0).all() and C.wave_nvec(d, 0)[2] == 0
    buf, d = C.shuffled_order()
    off = d["off"].astype(int)
    assert len(d) == 256 and len(set(off.tolist())) == 256 and (np.diff(np.sort(off)) >= 60).all()
    assert not (np.diff(off) > 0).all()
    for skew in range(16):
        assert C.wave_paths(d, 0x7000 + skew) == ["staged", "staged", "wide", "wide"]

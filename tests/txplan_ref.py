"""Python restatement of the tx planner's rule (include/emu_rx.h emurx_tx_plan_dev): the
emurx_tx_desc of a frame about to be sent, derived from the frame's own headers.

    plan_frame(p, flags) -> (l3, l4, osize, ops, nh, outcome)
    plan(buf, desc, flags) -> (TX_DESC_DTYPE[n], outcome u8[n], info u64[TXP_INFO_WORDS])

Plain Python ints and bytes; neither the library nor the C oracle is imported or called.  The walk
is the rx parser's (src/emu/core/parser.go) without its checksum tests, so that what the library
sends it also parses; `len` is the frame's length, be16 a big-endian byte pair:

  L2    len < 14 -> BAD.  EtherType at 12; each 0x8100 / 0x88a8 tag advances 4 bytes and needs the
        next EtherType inside len (else BAD); a third tag -> BAD (parser.go:700-741 accepts two).
        l3 = the byte behind the EtherType.
  IPv4  (0x0800, parser.go:771-862) BAD unless len >= l3 + 20, version 4, IHL * 4 >= 20,
        len >= l3 + IHL * 4 and totlen >= IHL * 4.  From here on ops = TX_IPV4_HDR and l4 = l3 +
        IHL * 4, the end of the header the op sums (the rx record's l4; the capture descriptors
        carry it with the header op alone too).
        l3 + totlen != len -> LENGTH, the header op alone: the tx call's L4 span is p[l4:len], as
        the Go callers slice it, so a frame with bytes behind the datagram gets no L4 sum.
        be16(p[l3+6]) & 0x3fff (fragment offset or MF), or a protocol that is none of 6 / 17 / 1
        -> HDR (IGMP with its 24-byte header among them).
        Else kind TCP4 / UDP4 / ICMP4, outcome L4; BAD when len < l4 + 20 / 8 / 4
        (the bytes up to the field the op clears).
  IPv6  (0x86dd, parser.go:864-952) BAD unless len >= l3 + 40 and version 6.
        l3 + 40 + plen != len -> LENGTH, ops 0.
        While the next header is one of {0, 43, 50, 51, 60, 135, 139, 140}: the header is
        (p[o+1] << 3) + 8 bytes; fewer than 8 bytes left, or a header that ends past len -> BAD.
        Final next header 6 / 17 / 58 -> TCP6 / UDP6 / ICMP6, outcome L4, osize = l4 - l3 - 40;
        with osize > 0, ops |= TX_V6_NH and nh = the final next header.  The same minimum
        lengths as for IPv4 (ICMPv6: 4).  Any other next header (44 and 59 among them) -> NONE.
  else  ARP, EAPOL, PPPoE and the rest -> NONE, ops 0.
  TXP_UDP0_KEEP  a UDP checksum field that is 00 00 stays: IPv4 -> HDR, IPv6 -> NONE.  Without
        the flag the field is computed.

Every other field is 0: BAD, NONE and the IPv6 LENGTH give an all-zero plan; HDR and the IPv4
LENGTH give l3, l4 and TX_IPV4_HDR alone.
"""
import numpy as np

from emurx import abi

EXT = (0, 43, 50, 51, 60, 135, 139, 140)
MIN_L4 = {6: 20, 17: 8, 1: 4, 58: 4}
KIND4 = {6: abi.TX_L4_TCP4, 17: abi.TX_L4_UDP4, 1: abi.TX_L4_ICMP4}
KIND6 = {6: abi.TX_L4_TCP6, 17: abi.TX_L4_UDP6, 58: abi.TX_L4_ICMP6}
ZERO = (0, 0, 0, 0, 0)


def be16(p, i):
    return (p[i] << 8) | p[i + 1]


def plan_frame(p, flags=0):
    p = bytes(p)
    n = len(p)
    keep = bool(flags & abi.TXP_UDP0_KEEP)
    bad = ZERO + (abi.TXP_BAD,)
    none = ZERO + (abi.TXP_NONE,)
    if n < 14:
        return bad
    et, l3, tags = be16(p, 12), 14, 0
    while et in (0x8100, 0x88A8):
        if tags == 2 or n < l3 + 4:
            return bad
        et = be16(p, l3 + 2)
        l3 += 4
        tags += 1
    if et == 0x0800:
        if n < l3 + 20 or p[l3] >> 4 != 4:
            return bad
        ihl = (p[l3] & 0xF) * 4
        if ihl < 20 or n < l3 + ihl or be16(p, l3 + 2) < ihl:
            return bad
        l4 = l3 + ihl
        hdr = (l3, l4, 0, abi.TX_IPV4_HDR, 0)
        if l3 + be16(p, l3 + 2) != n:
            return hdr + (abi.TXP_LENGTH,)
        proto = p[l3 + 9]
        if (be16(p, l3 + 6) & 0x3FFF) or proto not in KIND4:
            return hdr + (abi.TXP_HDR,)
        if n < l4 + MIN_L4[proto]:
            return bad
        if proto == 17 and keep and p[l4 + 6:l4 + 8] == b"\0\0":
            return hdr + (abi.TXP_HDR,)
        return (l3, l4, 0, abi.TX_IPV4_HDR | (KIND4[proto] << abi.TX_L4_SHIFT), 0, abi.TXP_L4)
    if et == 0x86DD:
        if n < l3 + 40 or p[l3] >> 4 != 6:
            return bad
        if l3 + 40 + be16(p, l3 + 4) != n:
            return ZERO + (abi.TXP_LENGTH,)
        nh, o = p[l3 + 6], l3 + 40
        while nh in EXT:
            if n < o + 8:
                return bad
            hl = (p[o + 1] << 3) + 8
            if n < o + hl:
                return bad
            nh = p[o]
            o += hl
        if nh not in KIND6:
            return none
        if n < o + MIN_L4[nh]:
            return bad
        if nh == 17 and keep and p[o + 6:o + 8] == b"\0\0":
            return none
        osize = o - l3 - 40
        ops = KIND6[nh] << abi.TX_L4_SHIFT
        if osize:
            return (l3, o, osize, ops | abi.TX_V6_NH, nh, abi.TXP_L4)
        return (l3, o, 0, ops, 0, abi.TXP_L4)
    return none


def plan(buf, desc, flags=0):
    """Every emurx_desc of `desc` in order -> (tx descriptors, outcomes, info words)."""
    b = np.ascontiguousarray(buf, dtype=np.uint8).tobytes()
    n = len(desc)
    d = np.zeros(n, abi.TX_DESC_DTYPE)
    oc = np.zeros(n, np.uint8)
    info = np.zeros(abi.TXP_INFO_WORDS, np.uint64)
    for i, (off, ln) in enumerate(zip(np.asarray(desc["off"]).tolist(), np.asarray(desc["len"]).tolist())):
        l3, l4, osize, ops, nh, o = plan_frame(b[off:off + ln], flags)
        d[i] = (off, ln, l3, l4, osize, ops, nh, (0, 0))
        oc[i] = o
        info[o] += 1
    return d, oc, info


def clear_fields(buf, txd):
    """A copy of buf with every checksum field the descriptors' ops name set to 00 00."""
    import tx_ref
    out = np.array(buf, dtype=np.uint8, copy=True)
    for x in np.asarray(txd).tolist():
        off, _, l3, l4, _, ops = x[:6]
        if ops & abi.TX_IPV4_HDR:
            out[off + l3 + 10:off + l3 + 12] = 0
        k = ops >> abi.TX_L4_SHIFT
        if k:
            f = off + l4 + tx_ref.FIELD[k]
            out[f:f + 2] = 0
    return out

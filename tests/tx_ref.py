"""Python restatement of what the reference's send paths do to the checksums of one frame, the
second reference of emurx_tx_checksum_dev next to the C oracle's orc_tx_checksum.

    tx_frame(p, l3, l4, osize, ops, nh) -> status          p: bytearray, rewritten in place
    tx_checksum(buf, desc) -> (new buffer, status[n])      the call shape of pyoracle.tx_checksum

Plain Python ints and bytes, nothing that can wrap unseen; the C oracle is neither imported nor
called.  The statements, in the order the Go code runs them (paths relative to
src/external/google/gopacket/layers unless they start with plugins/, which is src/emu/plugins):

  1 TX_IPV4_HDR  IPv4Header(p[l3:l3+hlen]).UpdateChecksum()                       ip4.go:132-136
        o[10:12] = 0; o[10:12] = tcpipChecksum(o, 0).  The callers slice the whole header: 20 bytes
        in transport (plugins/transport/tcp_output.go:110-112, udp.go:187), 24 bytes with IGMP's
        router-alert option (plugins/igmp/igmp.go:1186).  The C-ABI takes hlen = IHL * 4 from the
        frame and never fewer than the 20 bytes every caller slices.
  2 the L4 field cleared: PutUint16(p[l4+16:l4+18], 0) plugins/transport/tcp_output.go:68,
        udp.go:148 (l4 + 6), ip6.go:41 (l4[of:of+2]), icmp4.go:253 (o[2:4])
  3 the pseudo header, read AFTER 1 and 2 (it sees the new header checksum and the zero field
        wherever those bytes overlap it):
        TCP4 / UDP4   IPv4Header(p[l3:l3+20]).GetPhCs() ip4.go:49-58: src, dst, 0, protocol,
                      uint16(GetLength() - GetHeaderLen()) (ip4.go:68-70, 77-80), summed by getCs
                      tcpip.go:22-32
        TCP6 / UDP6 / ICMP6   IPv6Header(p[l3:l3+40]).GetPhCs(osize, nextH) ip6.go:127-134: src, dst,
                      uint32(PayloadLength() - osize) with the subtraction in uint16, three zero
                      bytes, nextH; summed by getCsv6 ip6.go:115-125.  nextH is o.NextHeader()
                      (ip6.go:42, 69-71), or the caller's constant where PktChecksumTcpUdpV6 is
                      called directly (tcpip.go:34-36, plugins/ipv6/mld.go:1271): TX_V6_NH and `nh`
        ICMP4         none: tcpipChecksum(o, 0) icmp4.go:254
  4 field = tcpipChecksum(p[l4:len], pseudo header) tcpip.go:76-94 (through PktChecksum :70-72,
        PktChecksumTcpUdp :38-40, FixL4ChecksumOffset ip6.go:40-44, UpdateChecksum icmp4.go:252-256)

tcpipChecksum adds big-endian byte pairs into a uint32 (an odd last byte as the high half), folds
while the value exceeds 0xffff and returns the complement: 0xffff only for a sum of exactly zero,
0x0000 for every other sum that is 0 modulo 0xffff.

The range rule is include/emu_rx.h's (EMURX_TX_RANGE): a frame one of whose slices above would
leave p[0:len] (Go panics there), or whose kind is none of the six, is not touched at all.
"""
import numpy as np

from emurx import abi

FIELD = {abi.TX_L4_TCP4: 16, abi.TX_L4_UDP4: 6, abi.TX_L4_TCP6: 16, abi.TX_L4_UDP6: 6, abi.TX_L4_ICMP6: 2,
         abi.TX_L4_ICMP4: 2}
V4L4 = (abi.TX_L4_TCP4, abi.TX_L4_UDP4)
V6L4 = (abi.TX_L4_TCP6, abi.TX_L4_UDP6, abi.TX_L4_ICMP6)


def pair_sum(b) -> int:
    """Sum of the big-endian byte pairs of b, an odd last byte as a high half (tcpip.go:80-89)."""
    b = bytes(b)
    return sum(b[0::2]) * 256 + sum(b[1::2])


def tcpip_checksum(data, csum: int) -> int:
    """tcpipChecksum tcpip.go:76-94 (csum is a Go uint32)."""
    csum = (csum + pair_sum(data)) & 0xFFFFFFFF
    while csum > 0xFFFF:
        csum = (csum >> 16) + (csum & 0xFFFF)
    return ~csum & 0xFFFF


def ipv4_phcs(o) -> int:
    """IPv4Header.GetPhCs ip4.go:49-58 on the 20-byte slice o."""
    length = (((o[2] << 8) | o[3]) - ((o[0] & 0xF) << 2)) & 0xFFFF
    ph = bytes(o[12:16]) + bytes(o[16:20]) + bytes([0, o[9]]) + length.to_bytes(2, "big")
    assert len(ph) == 12
    return pair_sum(ph)


def ipv6_phcs(o, osize: int, next_h: int) -> int:
    """IPv6Header.GetPhCs ip6.go:127-134 on the 40-byte slice o."""
    length = (((o[4] << 8) | o[5]) - osize) & 0xFFFF
    ph = bytes(o[8:24]) + bytes(o[24:40]) + length.to_bytes(4, "big") + bytes([0, 0, 0, next_h])
    assert len(ph) == 40
    return pair_sum(ph)


def in_range(p, l3: int, l4: int, ops: int) -> bool:
    """Every slice the statements take lies in p (include/emu_rx.h, EMURX_TX_RANGE)."""
    n, kind = len(p), ops >> abi.TX_L4_SHIFT
    if kind not in FIELD and kind != abi.TX_L4_NONE:
        return False
    if ops & abi.TX_IPV4_HDR:
        if l3 + 20 > n or l3 + max(20, (p[l3] & 0xF) * 4) > n:
            return False
    if kind in V4L4 and l3 + 20 > n:
        return False
    if kind in V6L4 and l3 + 40 > n:
        return False
    if kind and l4 + FIELD[kind] + 2 > n:
        return False
    return True


def tx_frame(p: bytearray, l3: int, l4: int, osize: int, ops: int, nh: int) -> int:
    if not in_range(p, l3, l4, ops):
        return abi.TX_RANGE
    kind = ops >> abi.TX_L4_SHIFT
    if ops & abi.TX_IPV4_HDR:                                  # 1
        hlen = max(20, (p[l3] & 0xF) * 4)
        p[l3 + 10:l3 + 12] = b"\0\0"
        p[l3 + 10:l3 + 12] = tcpip_checksum(p[l3:l3 + hlen], 0).to_bytes(2, "big")
    if kind:
        f = l4 + FIELD[kind]
        p[f:f + 2] = b"\0\0"                                   # 2
        phcs = 0                                               # 3
        if kind in V4L4:
            phcs = ipv4_phcs(p[l3:l3 + 20])
        elif kind in V6L4:
            phcs = ipv6_phcs(p[l3:l3 + 40], osize, nh if ops & abi.TX_V6_NH else p[l3 + 6])
        p[f:f + 2] = tcpip_checksum(p[l4:], phcs).to_bytes(2, "big")   # 4
    return abi.TX_OK


def tx_checksum(buf, desc):
    """Every descriptor in order, on a copy of buf -> (new buffer, status[n])."""
    out = bytearray(np.ascontiguousarray(buf, dtype=np.uint8).tobytes())
    st = np.zeros(len(desc), np.uint8)
    for i, d in enumerate(np.asarray(desc).tolist()):
        off, ln, l3, l4, osize, ops, nh = d[:7]
        p = bytearray(out[off:off + ln])
        st[i] = tx_frame(p, l3, l4, osize, ops, nh)
        out[off:off + ln] = p
    return np.frombuffer(bytes(out), np.uint8).copy(), st


def field_value(out, d) -> int:
    """The L4 checksum field of descriptor d (kind != 0) in the buffer out."""
    f = int(d["off"]) + int(d["l4"]) + FIELD[int(d["ops"]) >> abi.TX_L4_SHIFT]
    return (int(out[f]) << 8) | int(out[f + 1])

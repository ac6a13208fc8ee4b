"""Python restatement of the send side of the ping plugin and of the batch emurx_pingtx_dev makes
of it.

    template4 / template6   PreparePingPacketTemplate of the ICMPv4 / IPv6 plugin -> (icmp_off, pkt)
    send(live, icmp_off, seq, count, ts) -> (frames, live)   Ping.sendPing's loop
    closed_form(tmpl, icmp_off, seq, ts) -> checksum         the nine-term sum the device uses
    patch(tmpl, icmp_off, seq, ts) -> frame                  the template with seq, ts and that checksum
    generate(store, reqs, out_cap, desc_cap)                 emurx_pingtx_dev's outputs

The rule, with the reference's lines (paths relative to src/emu/plugins unless rooted):

  template4  icmp/icmp.go:208-237: GetL2Header(false, 0x0800) (core/client_ctx.go:353-372: six zero
             bytes, the client's MAC, one tag per non-zero Vlans word, the EtherType), the resolved
             gateway MAC over the zeros when there is one (:212-215); IPv4 version 4, IHL 5, TTL 64
             (ping/ping.go:43), Id 0xcc, protocol 1; ICMPv4 (8, 0), Id, Seq; payload_size bytes of
             payload (>= 16, icmp.go:528) with the magic big-endian in bytes 0..7; the ICMP checksum
             over header and payload (UpdateChecksum, gopacket layers/icmp4.go:252-256), then the
             IPv4 length and header checksum (:233-235)
  template6  ipv6/ipv6.go:216-262: the same L2 with 0x86dd; IPv6 version 6, next header 58, hop limit
             64; ICMPv6 (128, 0), Identifier, SeqNumber, the same payload; payload length, then
             FixIcmpL4Checksum (gopacket layers/ip6.go:54-56: pseudo header of the two addresses, the
             length and 58)
  send       ping/ping.go:317-341: per frame the sequence number is written at icmp_off + 6 and
             UpdateChecksum2(old, new) applied, then the timestamp at icmp_off + 16 and
             UpdateChecksum3(old, new) (layers/icmp4.go:258-285: UpdateInetChecksum :238-250 over
             the 16-bit words at shifts 0, 16, 32, 48), all on the live packet, which is then
             copied out; the sequence number increments per frame and wraps at 2^16; one timestamp
             per call (128 in the simulation, :322-324)

No text of the reference is restated here.
"""
import struct

import numpy as np

MAGIC = 0xC15C0C15C0BE5BE5
SIM_IDENT, SIM_SEQ, SIM_TS = 0x1234, 0xABCD, 128
PTX_OK, PTX_BAD_ID, PTX_NOSPC = 0, 1, 2
SLOT, MAX_LEN = 256, 248
REQ_DTYPE = np.dtype([("id", "<u4"), ("seq", "<u2"), ("count", "<u2"), ("ts", "<u8")])
DESC_DTYPE = np.dtype([("off", "<u4"), ("len", "<u2"), ("vport", "u1"), ("pad", "u1")])


def be16(p, i):
    return (p[i] << 8) | p[i + 1]


def fold(s: int) -> int:
    while s > 0xFFFF:
        s = (s >> 16) + (s & 0xFFFF)
    return s


def tcpip_checksum(data, csum=0) -> int:
    """gopacket layers/tcpip.go:76-94."""
    for i in range(0, len(data) - 1, 2):
        csum += (data[i] << 8) + data[i + 1]
    if len(data) % 2:
        csum += data[-1] << 8
    return ~fold(csum) & 0xFFFF


def update_inet_checksum(cs: int, old: int, new: int) -> int:
    """gopacket layers/icmp4.go:238-250."""
    return ~fold((~cs & 0xFFFF) + (~old & 0xFFFF) + new) & 0xFFFF


def l2_header(mac, vlans, ether_type, dst_mac=None):
    b = bytearray(dst_mac if dst_mac is not None else bytes(6)) + bytearray(mac)
    for v in vlans:
        if v:
            b += struct.pack(">I", v)
    return b + struct.pack(">H", ether_type)


def _payload(size, magic):
    assert size >= 16
    return struct.pack(">Q", magic) + bytes(size - 8)


def template4(mac, vlans, src, dst, ident, seq, magic=MAGIC, payload_size=16, dst_mac=None):
    pkt = l2_header(mac, vlans, 0x0800, dst_mac)
    l3 = len(pkt)
    pkt += bytes([0x45, 0, 0, 0, 0, 0xCC, 0, 0, 64, 1, 0, 0]) + bytes(src) + bytes(dst)
    icmp_off = len(pkt)
    pkt += struct.pack(">BBHHH", 8, 0, 0, ident, seq) + _payload(payload_size, magic)
    struct.pack_into(">H", pkt, icmp_off + 2, tcpip_checksum(pkt[icmp_off:]))
    struct.pack_into(">H", pkt, l3 + 2, len(pkt) - l3)
    struct.pack_into(">H", pkt, l3 + 10, tcpip_checksum(pkt[l3:l3 + 20]))
    return icmp_off, pkt


def template6(mac, vlans, src, dst, ident, seq, magic=MAGIC, payload_size=16, dst_mac=None):
    pkt = l2_header(mac, vlans, 0x86DD, dst_mac)
    l3 = len(pkt)
    pkt += bytes([0x60, 0, 0, 0, 0, 0, 58, 64]) + bytes(src) + bytes(dst)
    icmp_off = len(pkt)
    pkt += struct.pack(">BBHHH", 128, 0, 0, ident, seq) + _payload(payload_size, magic)
    plen = len(pkt) - icmp_off
    struct.pack_into(">H", pkt, l3 + 4, plen)
    ph = tcpip_checksum(pkt[l3 + 8:l3 + 40] + struct.pack(">II", plen, 58))
    struct.pack_into(">H", pkt, icmp_off + 2, tcpip_checksum(pkt[icmp_off:], ~ph & 0xFFFF))
    return icmp_off, pkt


def send(live, icmp_off, seq, count, ts):
    """sendPing's loop on the live packet: the frames it sends and the packet it leaves."""
    live = bytearray(live)
    frames = []
    for _ in range(count):
        old = be16(live, icmp_off + 6)
        struct.pack_into(">H", live, icmp_off + 6, seq)
        cs = update_inet_checksum(be16(live, icmp_off + 2), old, seq)
        struct.pack_into(">H", live, icmp_off + 2, cs)
        seq = (seq + 1) & 0xFFFF
        old_ts = struct.unpack_from(">Q", live, icmp_off + 16)[0]
        struct.pack_into(">Q", live, icmp_off + 16, ts)
        for i in range(4):
            cs = update_inet_checksum(be16(live, icmp_off + 2), (old_ts >> (16 * i)) & 0xFFFF, (ts >> (16 * i)) & 0xFFFF)
            struct.pack_into(">H", live, icmp_off + 2, cs)
        frames.append(bytes(live))
    return frames, live


def closed_form(tmpl, icmp_off, seq, ts) -> int:
    """The checksum of the template with seq and ts patched in: nine terms, folded once."""
    old_ts = struct.unpack_from(">Q", tmpl, icmp_off + 16)[0]
    s = (~be16(tmpl, icmp_off + 2) & 0xFFFF) + (~be16(tmpl, icmp_off + 6) & 0xFFFF) + seq
    for i in range(4):
        s += (~(old_ts >> (16 * i)) & 0xFFFF) + ((ts >> (16 * i)) & 0xFFFF)
    return ~fold(s) & 0xFFFF


def patch(tmpl, icmp_off, seq, ts) -> bytes:
    f = bytearray(tmpl)
    struct.pack_into(">H", f, icmp_off + 2, closed_form(tmpl, icmp_off, seq, ts))
    struct.pack_into(">H", f, icmp_off + 6, seq)
    struct.pack_into(">Q", f, icmp_off + 16, ts)
    return bytes(f)


def align16(x):
    return (x + 15) & ~15


def generate(store, reqs, out_cap, desc_cap):
    """emurx_pingtx_dev.  store: {id: (template bytes, icmp_off, vport)}, the ids in use (a free or
    out-of-range id is simply absent); reqs: (id, seq, count, ts).  A request's frames are send()'s
    from the template, so every request starts from the template and not from the last live packet.
    Whole requests that fit out_cap / desc_cap (and the descriptor's 32-bit offset) are written, a
    prefix in request order.  Returns (frames, desc, outcome, info): frames as bytes, desc as
    DESC_DTYPE, outcome u8 [len(reqs)], info u64[8]."""
    frames, desc, outcome = [], [], []
    off = nfr = 0  # needed so far, written or not
    cnt = [0, 0, 0]
    cap = min(out_cap, 1 << 32)
    for rid, seq, count, ts in reqs:
        if rid not in store:
            outcome.append(PTX_BAD_ID)
            cnt[PTX_BAD_ID] += 1
            continue
        tmpl, icmp_off, vport = store[rid]
        step = align16(len(tmpl))
        o0 = off
        off += count * step
        nfr += count
        if count and (off > cap or nfr > desc_cap):
            outcome.append(PTX_NOSPC)
            cnt[PTX_NOSPC] += 1
            continue
        outcome.append(PTX_OK)
        cnt[PTX_OK] += 1
        for k, f in enumerate(send(tmpl, icmp_off, seq, count, ts)[0]):
            frames.append(f)
            desc.append((o0 + k * step, len(f), vport, 0))
    info = np.array([len(frames), off, nfr, cnt[0], cnt[1], cnt[2], 0, 0], np.uint64)
    return frames, np.array(desc, DESC_DTYPE), np.array(outcome, np.uint8), info

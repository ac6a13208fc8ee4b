"""Hand-built frames for every branch of the tx planner's rule (tests/txplan_ref.py), with the
plan each must get written out by hand: cases() -> [(name, frame, want, want_keep)], want =
(l3, l4, osize, ops, nh, outcome) without flags, want_keep with TXP_UDP0_KEEP.  The capture
corpus has no BAD frame and few of the edges; these pin them for the reference and the kernel."""
from emurx import abi

H = abi.TX_IPV4_HDR
NH = abi.TX_V6_NH
BAD = (0, 0, 0, 0, 0, abi.TXP_BAD)
NONE = (0, 0, 0, 0, 0, abi.TXP_NONE)
LEN6 = (0, 0, 0, 0, 0, abi.TXP_LENGTH)
TCP, UDP, ICMP, ICMP6 = 6, 17, 1, 58


def K(kind):
    return kind << abi.TX_L4_SHIFT


def eth(et, tags=0, tpid=0x8100):
    b = bytes(range(1, 7)) + bytes(range(0x11, 0x17))
    for t in range(tags):
        b += (tpid if t == 0 else 0x8100).to_bytes(2, "big") + (100 + t).to_bytes(2, "big")
    return b + et.to_bytes(2, "big")


def ip4(proto, payload, ihl=5, frag=0, tot=None, ver=4):
    tot = ihl * 4 + len(payload) if tot is None else tot
    h = bytes([(ver << 4) | ihl, 0]) + (tot & 0xFFFF).to_bytes(2, "big") + b"\x12\x34" + frag.to_bytes(2, "big")
    h += bytes([64, proto, 0xAB, 0xCD]) + bytes([10, 0, 0, 1, 10, 0, 0, 2])
    h += bytes([0x94, 0x04, 0, 0] * (ihl - 5)) if ihl > 5 else b""
    return h[:ihl * 4] + payload


def ip6(nh, payload, plen=None, ver=6):
    plen = len(payload) if plen is None else plen
    return bytes([ver << 4, 0, 0, 0]) + plen.to_bytes(2, "big") + bytes([nh, 64]) + bytes(range(32)) + payload


def ext(next_h, size=8):
    assert size % 8 == 0 and 8 <= size <= 2048
    return bytes([next_h, size // 8 - 1]) + bytes(size - 2)


def l4(proto, size=None, zero_cs=False):
    """An L4 header (+ payload) of `size` bytes with a non-zero checksum field unless zero_cs."""
    base = {TCP: 20, UDP: 8, ICMP: 8, ICMP6: 8}[proto]
    size = base + 6 if size is None else size
    b = bytearray((i * 7 + 3) & 0xFF or 1 for i in range(max(size, 20)))
    f = {TCP: 16, UDP: 6, ICMP: 2, ICMP6: 2}[proto]
    b[f:f + 2] = b"\0\0" if zero_cs else b"\xBE\xEF"
    return bytes(b[:size])


def cases():
    c = []

    def add(name, frame, want, keep=None):
        c.append((name, bytes(frame), want, want if keep is None else keep))

    # ---- L2 ----
    add("len0", b"", BAD)
    add("len13", eth(0x0800)[:13], BAD)
    add("len14_arp_type", eth(0x0806), NONE)
    for tags in (0, 1, 2):
        l3 = 14 + 4 * tags
        add(f"udp4_tags{tags}", eth(0x0800, tags) + ip4(UDP, l4(UDP)), (l3, l3 + 20, 0, H | K(abi.TX_L4_UDP4), 0, abi.TXP_L4))
    add("qinq_88a8", eth(0x0800, 2, 0x88A8) + ip4(TCP, l4(TCP)), (22, 42, 0, H | K(abi.TX_L4_TCP4), 0, abi.TXP_L4))
    add("third_tag", eth(0x0800, 3) + ip4(UDP, l4(UDP)), BAD)
    add("tag_cut_len16", eth(0x0800, 1)[:16], BAD)
    add("tag_cut_len17", eth(0x0800, 1)[:17], BAD)
    add("tag_type_at_end_len18", eth(0x0806, 1), NONE)
    add("two_tags_cut_len21", eth(0x0800, 2)[:21], BAD)
    add("arp", eth(0x0806) + bytes(28), NONE)
    add("eapol", eth(0x888E) + bytes(8), NONE)
    add("pppoe", eth(0x8864) + bytes(30), NONE)
    # ---- IPv4 ----
    add("tcp4_ihl5", eth(0x0800) + ip4(TCP, l4(TCP)), (14, 34, 0, H | K(abi.TX_L4_TCP4), 0, abi.TXP_L4))
    add("tcp4_ihl6", eth(0x0800) + ip4(TCP, l4(TCP), ihl=6), (14, 38, 0, H | K(abi.TX_L4_TCP4), 0, abi.TXP_L4))
    add("udp4_ihl15_past_window", eth(0x0800, 2) + ip4(UDP, l4(UDP, 30), ihl=15),
        (22, 82, 0, H | K(abi.TX_L4_UDP4), 0, abi.TXP_L4))
    add("ip4_ihl4", eth(0x0800) + ip4(TCP, l4(TCP), ihl=4, tot=40), BAD)
    add("ip4_version5", eth(0x0800) + ip4(TCP, l4(TCP), ver=5), BAD)
    add("ip4_len_l3_19", (eth(0x0800) + ip4(253, b"", tot=20))[:33], BAD)
    add("ip4_len_l3_20_other_proto", eth(0x0800) + ip4(253, b""), (14, 34, 0, H, 0, abi.TXP_HDR))
    add("ip4_ihl6_len_l3_23", (eth(0x0800) + ip4(2, b"", ihl=6))[:37], BAD)
    add("ip4_ihl6_len_l3_24", eth(0x0800) + ip4(2, b"", ihl=6), (14, 38, 0, H, 0, abi.TXP_HDR))
    add("ip4_totlen_19", eth(0x0800) + ip4(UDP, l4(UDP), tot=19), BAD)
    add("igmp_ihl6", eth(0x0800) + ip4(2, bytes([0x22, 0, 0xAA, 0xBB, 0, 0, 0, 1]), ihl=6), (14, 38, 0, H, 0, abi.TXP_HDR))
    add("frag_mf", eth(0x0800) + ip4(UDP, l4(UDP), frag=0x2000), (14, 34, 0, H, 0, abi.TXP_HDR))
    add("frag_offset", eth(0x0800) + ip4(UDP, l4(UDP), frag=0x0001), (14, 34, 0, H, 0, abi.TXP_HDR))
    add("frag_df_only", eth(0x0800) + ip4(UDP, l4(UDP), frag=0x4000), (14, 34, 0, H | K(abi.TX_L4_UDP4), 0, abi.TXP_L4))
    add("icmp4", eth(0x0800) + ip4(ICMP, l4(ICMP)), (14, 34, 0, H | K(abi.TX_L4_ICMP4), 0, abi.TXP_L4))
    for proto, kind, need in ((TCP, abi.TX_L4_TCP4, 20), (UDP, abi.TX_L4_UDP4, 8), (ICMP, abi.TX_L4_ICMP4, 4)):
        add(f"v4_proto{proto}_min_less_1", eth(0x0800) + ip4(proto, l4(proto, need - 1)), BAD)
        add(f"v4_proto{proto}_min", eth(0x0800) + ip4(proto, l4(proto, need)), (14, 34, 0, H | K(kind), 0, abi.TXP_L4))
    add("udp4_zero", eth(0x0800) + ip4(UDP, l4(UDP, zero_cs=True)), (14, 34, 0, H | K(abi.TX_L4_UDP4), 0, abi.TXP_L4),
        keep=(14, 34, 0, H, 0, abi.TXP_HDR))
    add("tcp4_zero_field_is_computed", eth(0x0800) + ip4(TCP, l4(TCP, zero_cs=True)),
        (14, 34, 0, H | K(abi.TX_L4_TCP4), 0, abi.TXP_L4))
    add("v4_length_padding", eth(0x0800) + ip4(UDP, l4(UDP)) + bytes(4), (14, 34, 0, H, 0, abi.TXP_LENGTH))
    add("v4_length_short_by_1", eth(0x0800) + ip4(UDP, l4(UDP), tot=20 + 14 + 1), (14, 34, 0, H, 0, abi.TXP_LENGTH))
    # ---- IPv6 ----
    add("ip6_len_l3_39", (eth(0x86DD) + ip6(59, b""))[:53], BAD)
    add("ip6_len_l3_40_nonext", eth(0x86DD) + ip6(59, b""), NONE)
    add("ip6_version5", eth(0x86DD) + ip6(TCP, l4(TCP), ver=5), BAD)
    add("v6_length_padding", eth(0x86DD) + ip6(UDP, l4(UDP)) + bytes(2), LEN6)
    add("v6_length_short_by_1", eth(0x86DD) + ip6(UDP, l4(UDP), plen=15), LEN6)
    for proto, kind, need in ((TCP, abi.TX_L4_TCP6, 20), (UDP, abi.TX_L4_UDP6, 8), (ICMP6, abi.TX_L4_ICMP6, 4)):
        add(f"v6_nh{proto}", eth(0x86DD) + ip6(proto, l4(proto)), (14, 54, 0, K(kind), 0, abi.TXP_L4))
        add(f"v6_nh{proto}_min_less_1", eth(0x86DD) + ip6(proto, l4(proto, need - 1)), BAD)
        add(f"v6_nh{proto}_min", eth(0x86DD, 1) + ip6(proto, l4(proto, need)), (18, 58, 0, K(kind), 0, abi.TXP_L4))
        add(f"v6_ext_nh{proto}_min_less_1", eth(0x86DD) + ip6(0, ext(proto) + l4(proto, need - 1)), BAD)
    add("udp6_zero", eth(0x86DD) + ip6(UDP, l4(UDP, zero_cs=True)), (14, 54, 0, K(abi.TX_L4_UDP6), 0, abi.TXP_L4), keep=NONE)
    add("udp6_zero_behind_ext", eth(0x86DD) + ip6(60, ext(UDP, 16) + l4(UDP, zero_cs=True)),
        (14, 70, 16, K(abi.TX_L4_UDP6) | NH, UDP, abi.TXP_L4), keep=NONE)
    add("mld_hbh", eth(0x86DD) + ip6(0, ext(ICMP6) + l4(ICMP6, 24)), (14, 62, 8, K(abi.TX_L4_ICMP6) | NH, ICMP6, abi.TXP_L4))
    add("v6_two_ext", eth(0x86DD) + ip6(0, ext(60, 8) + ext(UDP, 16) + l4(UDP)),
        (14, 78, 24, K(abi.TX_L4_UDP6) | NH, UDP, abi.TXP_L4))
    add("v6_three_ext", eth(0x86DD, 2) + ip6(0, ext(43, 8) + ext(60, 24) + ext(TCP, 16) + l4(TCP)),
        (22, 110, 48, K(abi.TX_L4_TCP6) | NH, TCP, abi.TXP_L4))
    for e in (43, 50, 51, 60, 135, 139, 140):
        add(f"v6_ext{e}", eth(0x86DD) + ip6(e, ext(ICMP6, 16) + l4(ICMP6)), (14, 70, 16, K(abi.TX_L4_ICMP6) | NH, ICMP6, abi.TXP_L4))
    add("v6_nh44", eth(0x86DD) + ip6(44, bytes(8) + l4(UDP)), NONE)
    add("v6_nh59", eth(0x86DD) + ip6(59, bytes(12)), NONE)
    add("v6_ext_then_44", eth(0x86DD) + ip6(0, ext(44) + bytes(8) + l4(UDP)), NONE)
    add("v6_unknown_nh", eth(0x86DD) + ip6(132, bytes(16)), NONE)
    add("v6_chain_ends_at_len_nonext", eth(0x86DD) + ip6(0, ext(60, 8) + ext(59, 16)), NONE)
    add("v6_chain_ends_at_len_udp", eth(0x86DD) + ip6(0, ext(60, 8) + ext(UDP, 16)), BAD)
    add("v6_ext_one_byte_past_len", eth(0x86DD) + ip6(0, ext(60, 8) + ext(UDP, 16)[:15]), BAD)
    add("v6_ext_7_bytes_left", eth(0x86DD) + ip6(0, ext(60, 8) + ext(UDP, 8)[:7]), BAD)
    add("v6_ext_8_bytes_left_claims_16", eth(0x86DD) + ip6(0, ext(UDP, 16)[:8]), BAD)
    # chains that leave the 96-byte header window
    add("v6_chain_past_window", eth(0x86DD) + ip6(0, ext(60, 16) + ext(43, 16) + ext(60, 16) + ext(0, 16) + ext(UDP, 16) + l4(UDP)),
        (14, 134, 80, K(abi.TX_L4_UDP6) | NH, UDP, abi.TXP_L4))
    add("v6_ext_2048", eth(0x86DD) + ip6(60, ext(TCP, 2048) + l4(TCP)), (14, 2102, 2048, K(abi.TX_L4_TCP6) | NH, TCP, abi.TXP_L4))
    add("v6_long_chain_cut", eth(0x86DD) + ip6(0, ext(60, 64) + ext(43, 64) + ext(UDP, 64)[:63]), BAD)
    add("v6_long_chain_udp_zero", eth(0x86DD) + ip6(0, ext(60, 64) + ext(UDP, 64) + l4(UDP, zero_cs=True)),
        (14, 182, 128, K(abi.TX_L4_UDP6) | NH, UDP, abi.TXP_L4), keep=NONE)
    return c


def batch(flags, gap=3):
    """cases() packed into one buffer with `gap` bytes between frames (odd offsets) ->
    (buf, DESC_DTYPE desc, want tx descriptors, want outcomes)."""
    import numpy as np
    cs = cases()
    n = len(cs)
    desc = np.zeros(n, abi.DESC_DTYPE)
    want = np.zeros(n, abi.TX_DESC_DTYPE)
    oc = np.zeros(n, np.uint8)
    parts, at = [], 0
    for i, (_, f, w0, w1) in enumerate(cs):
        w = w1 if flags & abi.TXP_UDP0_KEEP else w0
        parts.append(bytes(gap) + f)
        at += gap
        desc[i] = (at, len(f), i % 251, 0)
        want[i] = (at, len(f), w[0], w[1], w[2], w[3], w[4], (0, 0))
        oc[i] = w[5]
        at += len(f)
    buf = np.frombuffer(b"".join(parts) + bytes(64), np.uint8).copy()
    return buf, desc, want, oc

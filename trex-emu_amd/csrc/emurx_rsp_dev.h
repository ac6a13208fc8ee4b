// emurx_rsp_dev.h — device functions the responder (emurx_respond.hip), the cache-learning fold
// (emurx_learn.hip) and the ping fold (emurx_ping.hip) share: the IPv4 source predicate, unaligned frame spans, the checks of a neighbour solicitation
// (plugins/ipv6/nd.go:1550-1609) and the lookup of the client that owns an ND target.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/emu_rx.h"
#include "emurx_parse.h"

namespace emurx {

__device__ __forceinline__ uint32_t rsp_le32(const uint8_t* p) {  // any alignment
    return gld1(p) | gld1(p + 1) << 8 | gld1(p + 2) << 16 | gld1(p + 3) << 24;
}

// Go 1.18 net.IP.IsLoopback || IsGlobalUnicast for an IPv4 address (bytes b0.b1.x.x, ip = the
// four wire bytes little-endian): not 0.0.0.0, 255.255.255.255, 224.0.0.0/4, 169.254.0.0/16.
// The rule is Go's standard library (net/ip.go), not the reference tree: as unpinned by the
// reference's own tests as ip6_local_or_global (emurx_parse.h) is.
__device__ __forceinline__ bool rsp_ip4_src_ok(uint32_t ip) {
    const uint32_t b0 = ip & 0xff, b1 = (ip >> 8) & 0xff;
    return !(ip == 0 || ip == 0xffffffffu || (b0 & 0xf0) == 0xe0 || (b0 == 169 && b1 == 254));
}

// E[s .. s + 16) of the frame E = [F, F + flen), s of either sign, as four little-endian words:
// the two aligned 16-byte blocks that hold the span, read only where they hold a byte of the
// frame (zeros elsewhere: the caller masks those bytes out), funnel-shifted
__device__ __forceinline__ void rsp_load16(uintptr_t F, uint32_t flen, int s, uint32_t o[4]) {
    const uintptr_t a = F + (intptr_t)s, A = a & ~(uintptr_t)15, Fend = F + flen;
    const uint32_t sh = (uint32_t)(a & 15), q = sh >> 2, bsh = sh & 3;
    uint4 x = make_uint4(0, 0, 0, 0), y = x;
    if (A < Fend && A + 16 > F) x = gld16(reinterpret_cast<const void*>(A));
    if (sh && A + 16 < Fend && A + 32 > F) y = gld16(reinterpret_cast<const void*>(A + 16));
    const uint32_t w[8] = {x.x, x.y, x.z, x.w, y.x, y.y, y.z, y.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t lo = q == 0 ? w[i] : q == 1 ? w[i + 1] : q == 2 ? w[i + 2] : w[i + 3];
        const uint32_t hi = q == 0 ? w[i + 1] : q == 1 ? w[i + 2] : q == 2 ? w[i + 3] : w[i + 4];
        o[i] = __builtin_amdgcn_alignbyte(hi, lo, bsh);
    }
}

// The client that answers a solicitation for target t (words LE), and its MAC (nd.go:1626-1678).
// EUI-64 target: CLookupByMac of the extracted MAC + IsValidPrefix (client_ctx.go:279-295);
// otherwise, a global target: CLookupByIPv6.  Then the client's ipv6 plugin.
struct RspNdHit {
    bool ok;
    uint32_t mlo, mhi;
};
__device__ __forceinline__ bool rsp_nd_eui(const uint32_t t[4]) { return (t[2] >> 24) == 0xffu && (t[3] & 0xffu) == 0xfeu; }
__device__ __forceinline__ RspNdHit rsp_nd_ip6(const emurx_dev_tables& T, uint32_t ns, uint32_t tk, const uint32_t t[4]) {
    const uint32_t bk = emurx_ip6_hash(tk, t[0], t[1], t[2], t[3]) & T.ip6_mask;
    const IpHit h = resolve_ip6(T, bk, ld_bucket(T.ip6_tab, bk), ns, t);
    return {h.cid != EMURX_ID_NONE && ((h.mhip >> 16) & (1u << EMURX_PLUG_IPV6)), h.mlo, h.mhip & 0xffffu};
}
// The client whose MAC the EUI-64 address t embeds and whose prefix t carries: {client id or
// EMURX_ID_NONE, its plugins}; m: the extracted MAC.  The neighbour advertisement's learning
// (nd.go:1740-1756) asks the same question as the solicitation's answer (:1626-1640).
__device__ __forceinline__ uint2 rsp_nd_eui_client(const emurx_dev_tables& T, uint32_t ns, uint32_t tk, const uint32_t t[4],
                                                   uint2& m) {
    m = eui_mac(t[2], t[3]);
    if (m.x == 0 && m.y == 0) return make_uint2(EMURX_ID_NONE, 0);  // MACKey.IsZero never matches
    const uint32_t bk = emurx_mac_hash(tk, m.x, m.y) & T.mac_mask;
    const uint2 c = resolve_mac(T, bk, ld_bucket(T.mac_tab, bk), ns, m.x, m.y);
    if (c.x == EMURX_ID_NONE) return make_uint2(EMURX_ID_NONE, 0);
    if (!(t[0] == 0x000080feu && t[1] == 0)) {  // not fe80::/64: the client's RA prefix, length 64
        const CInfo ci = client_info(T, c.x);
        if (!((ci.ra & 1u) && ((ci.ra >> 8) & 0xff) == 64 && ci.ra0 == t[0] && ci.ra1 == t[1])) return make_uint2(EMURX_ID_NONE, 0);
    }
    return c;
}
__device__ RspNdHit rsp_nd_client(const emurx_dev_tables& T, uint32_t ns, uint32_t tk, const uint32_t t[4], bool global) {
    if (!rsp_nd_eui(t)) return global ? rsp_nd_ip6(T, ns, tk, t) : RspNdHit{false, 0, 0};
    const uint2 m = eui_mac(t[2], t[3]);
    if (m.x == 0 && m.y == 0) return {false, 0, 0};  // MACKey.IsZero never matches
    const uint32_t bk = emurx_mac_hash(tk, m.x, m.y) & T.mac_mask;
    const uint2 c = resolve_mac(T, bk, ld_bucket(T.mac_tab, bk), ns, m.x, m.y);
    if (c.x == EMURX_ID_NONE) return {false, 0, 0};
    if (!(t[0] == 0x000080feu && t[1] == 0)) {  // not fe80::/64: the client's RA prefix, length 64
        const CInfo ci = client_info(T, c.x);
        if (!((ci.ra & 1u) && ((ci.ra >> 8) & 0xff) == 64 && ci.ra0 == t[0] && ci.ra1 == t[1])) return {false, 0, 0};
    }
    return {(c.y & (1u << EMURX_PLUG_IPV6)) != 0, m.x, m.y};
}

// The checks of a neighbour solicitation (type 135, code 0, header offsets that fit the frame)
// from its length to its target (nd.go:1550-1609; the rule with its citations is in
// include/emu_rx.h).  Where one of them decides, the result is mk(EMURX_RSP_NONE) or
// mk(EMURX_RSP_HOST); else then(w, slla, mac, src): w the target, slla whether a source
// link-layer address option is present, mac its address (x: bytes 0..3, y: bytes 4..5), src the
// IPv6 source.
template <class Mk, class Then>
__device__ __forceinline__ auto rsp_nd_checks(const uint8_t* f, uint32_t l3, uint32_t l4, uint32_t len, Mk mk, Then then)
    -> decltype(mk(0u)) {
    if (len - (l4 + 4) < 20) return mk(EMURX_RSP_NONE);  // pktRxErrTooShort
    // the options are the rest of the frame: none, or one source link-layer address
    const uint32_t nopt = len - (l4 + 24);
    if (nopt > 8) return mk(EMURX_RSP_HOST);
    if (nopt != 0 && nopt != 8) return mk(EMURX_RSP_NONE);
    const uintptr_t F = (uintptr_t)f;
    uint32_t w[4], src[4];
    uint2 mac = make_uint2(0, 0);
    const bool slla = nopt == 8;
    if (slla) {
        rsp_load16(F, len, (int)(l4 + 24), w);  // w[0], w[1]: the option
        if ((w[0] & 0xffffu) != 0x0101u) return mk(EMURX_RSP_NONE);
        if ((w[0] >> 16) == 0 && w[1] == 0) return mk(EMURX_RSP_NONE);
        mac = make_uint2(w[0] >> 16 | w[1] << 16, w[1] >> 16);
    }
    if (gld1(f + l3 + 7) != 255) return mk(EMURX_RSP_NONE);
    rsp_load16(F, len, (int)(l3 + 8), w);  // the source
#pragma unroll
    for (int j = 0; j < 4; ++j) src[j] = w[j];
    if (ip6_unspecified(w)) {
        if (slla) return mk(EMURX_RSP_NONE);
        rsp_load16(F, len, (int)(l3 + 24), w);  // the destination
        if (!ip6_multicast(w)) return mk(EMURX_RSP_NONE);
    }
    rsp_load16(F, len, (int)(l4 + 8), w);  // the target
    if (ip6_unspecified(w) || ip6_multicast(w)) return mk(EMURX_RSP_NONE);
    return then(w, slla, mac, src);
}

}  // namespace emurx

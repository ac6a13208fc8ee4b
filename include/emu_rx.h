/*
 * emu_rx.h — C-ABI of the MI355X receive path (parse + Namespace/Client classify).
 *
 * Drop-in boundary for TRex-EMU's rx hot path.  The entry points replace, one for one,
 * the Go surface listed below (paths relative to the reference tree):
 *
 *   emurx_rx_stream()        VethIFZmq.OnRxStream         src/emu/core/veth_zmq.go:277-320
 *                            + per frame CThreadCtx.HandleRxPacket  src/emu/core/thread_ctx.go:365-375
 *                            + Parser.ParsePacket / parsePacketL4   src/emu/core/parser.go:583-959
 *                            + CThreadCtx.GetNs                     src/emu/core/thread_ctx.go:772-784
 *                            + CNSCtx.CLookupBy{Mac,IPv4,IPv6,IPv6LocalGlobal} src/emu/core/ns_ctx.go:262-329
 *                            (down to, not including, the ParserCb call: plugins stay in Go)
 *   emurx_classify_dev()     the same, device-resident (frames + descriptors already in HBM)
 *   emurx_register()         Parser.Register               src/emu/core/parser.go:528-565
 *   emurx_ns_add/remove()    CThreadCtx.AddNs/RemoveNs      src/emu/core/thread_ctx.go:786-812
 *   emurx_ns_set_plugins()   ns.PluginCtx presence          src/emu/core/plugin_ctx.go:257-265
 *   emurx_client_add/remove  CNSCtx.AddClient/RemoveClient  src/emu/core/ns_ctx.go:332-440
 *   emurx_client_update_*    CNSCtx.UpdateClientIpv4/Ipv6/DIpv6 src/emu/core/ns_ctx.go:442-533
 *   emurx_client_set_ra()    CClient.Ipv6Router prefix      src/emu/core/client_ctx.go:60-66,279-295
 *   emurx_hist_to_counters() ParserStats accumulation       src/emu/core/parser.go:67-119
 *   emurx_comm_* / emurx_exchange_dev   no Go counterpart: the one MapNsT of the single main
 *                            goroutine (thread_ctx.go:139,397-419,772-784) split by Namespace
 *                            owner over the GPUs, joined by an RCCL exchange
 *
 * Conventions: plain C types, no exceptions or aborts cross the ABI; every call returns
 * EMURX_OK (0) or a negative EMURX_E* code (mirrors PARSER_OK/PARSER_ERR, parser.go:41-44).
 * Single caller thread per handle (the Go main goroutine, thread_ctx.go:397-419); every entry
 * point re-binds the handle's device, so goroutine OS-thread migration is harmless.
 */
#ifndef EMU_RX_H
#define EMU_RX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EMURX_ABI_VERSION 6

/* ---- return codes -------------------------------------------------------------------- */
#define EMURX_OK 0
#define EMURX_EINVAL (-22)   /* bad argument */
#define EMURX_ENOMEM (-12)   /* host or device allocation failed / capacity exceeded */
#define EMURX_EEXIST (-17)   /* key already present (AddNs / AddClient duplicate) */
#define EMURX_ENOENT (-2)    /* key not present */
#define EMURX_EDEVICE (-5)   /* HIP runtime error */
#define EMURX_ENOSPC (-28)   /* output buffer too small */

#define EMURX_ID_NONE 0xFFFFFFFFu

/* ---- limits (src/emu/core/mbuf.go:44-56, veth_zmq.go:8-22) ----------------------------- */
#define EMURX_MAX_FRAME 9216u      /* MAX_PACKET_SIZE: MbufPoll.Alloc panics above */
#define EMURX_ZMQ_MAGIC 0xBEEFu    /* ZMQ_PACKET_HEADER_MAGIC */

/* ---- parser callbacks: order of the Parser struct fields, parser.go:509-520 ------------ */
enum emurx_cb {
    EMURX_CB_ARP = 0,
    EMURX_CB_ICMP = 1,
    EMURX_CB_IGMP = 2,
    EMURX_CB_DHCP = 3,
    EMURX_CB_DHCPSRV = 4,
    EMURX_CB_DHCPV6 = 5,
    EMURX_CB_MDNS = 6,
    EMURX_CB_TCP = 7,
    EMURX_CB_UDP = 8,
    EMURX_CB_ICMPV6 = 9,
    EMURX_CB_EAPOL = 10,
    EMURX_CB_PPP = 11,
    EMURX_NUM_CB = 12,
    EMURX_CB_NONE = 0xFF
};
/* output queues: one per callback + one for every frame that reaches no callback */
#define EMURX_Q_DROP 12
#define EMURX_NUM_QUEUES 13

/* ---- plugins whose per-Namespace / per-Client presence gates a callback --------------- */
enum emurx_plugin {
    EMURX_PLUG_ARP = 0,       /* "arp"       */
    EMURX_PLUG_ICMP = 1,      /* "icmp"      */
    EMURX_PLUG_IGMP = 2,      /* "igmp"      */
    EMURX_PLUG_DHCP = 3,      /* "dhcp"      */
    EMURX_PLUG_DHCPSRV = 4,   /* "dhcpsrv"   */
    EMURX_PLUG_DHCPV6 = 5,    /* "dhcpv6"    */
    EMURX_PLUG_MDNS = 6,      /* "mdns"      */
    EMURX_PLUG_TRANSPORT = 7, /* "transport" */
    EMURX_PLUG_IPV6 = 8,      /* "ipv6"      */
    EMURX_PLUG_DOT1X = 9,     /* "dot1x"     */
    EMURX_PLUG_PPP = 10,      /* "ppp"       */
    EMURX_NUM_PLUG = 11
};
#define EMURX_PLUG_ALL ((1u << EMURX_NUM_PLUG) - 1u)

/* ---- per-frame parse outcome (one per distinct return path of ParsePacket) ------------ */
enum emurx_status {
    EMURX_ST_OK = 0,                 /* callback `proto` invoked                             */
    EMURX_ST_NOT_SUPPORTED = 1,      /* callback unregistered -> parserNotSupported, :524     */
    EMURX_ST_PACKET_TOO_SHORT = 2,   /* errPacketIsTooShort        :770                       */
    EMURX_ST_EAPOL_TOO_SHORT = 3,    /* errEAPolTooShort           :781                       */
    EMURX_ST_ARP_TOO_SHORT = 4,      /* errArpTooShort             :792                       */
    EMURX_ST_DOT1Q_TOO_SHORT = 5,    /* errDot1qTooShort           :802                       */
    EMURX_ST_TOO_MANY_DOT1Q = 6,     /* errToManyDot1q             :806                       */
    EMURX_ST_IPV4_TOO_SHORT = 7,     /* errIPv4TooShort            :824,846                   */
    EMURX_ST_IPV4_HDR_TOO_SHORT = 8, /* errIPv4HeaderTooShort      :829,838,842               */
    EMURX_ST_IPV4_FRAGMENT = 9,      /* errIPv4Fragment            :833                       */
    EMURX_ST_IPV4_CS = 10,           /* errIPv4cs                  :854                       */
    EMURX_ST_IPV6_TOO_SHORT = 11,    /* errIPv6TooShort            :866-877,894-926           */
    EMURX_ST_IPV6_HOPLIMIT = 12,     /* errIPv6HopLimitDrop        :879                       */
    EMURX_ST_IPV6_EMPTY = 13,        /* errIPv6Empty               :943                       */
    EMURX_ST_IPV6_JUMBO = 14,        /* errIPv6OptJumbo            :938                       */
    EMURX_ST_IPV6_FRAGMENT = 15,     /* errIPv6Fragment            :934                       */
    EMURX_ST_ICMPV4_TOO_SHORT = 16,  /* errIcmpv4TooShort (ICMP and IGMP) :592,607            */
    EMURX_ST_ICMPV4_CS = 17,         /* errIcmpv4Cse               :597                       */
    EMURX_ST_TCP_TOO_SHORT = 18,     /* errTcpTooShort             :615,621                   */
    EMURX_ST_TCP_CS = 19,            /* tcpCsErr                   :628                       */
    EMURX_ST_UDP_TOO_SHORT = 20,     /* errUdpTooShort             :637                       */
    EMURX_ST_UDP_CS = 21,            /* udpCsErr                   :644                       */
    EMURX_ST_ICMPV6_TOO_SHORT = 22,  /* errIcmpv6TooShort          :685                       */
    EMURX_ST_ICMPV6_CS = 23,         /* errIcmpv6Cse               :689                       */
    EMURX_ST_ICMPV6_UNSUPPORTED = 24,/* errIcmpv6Unsupported       :715                       */
    EMURX_ST_L4_UNSUPPORTED = 25,    /* errL4ProtoUnsupported      :720                       */
    EMURX_ST_L3_UNSUPPORTED = 26,    /* errL3ProtoUnsupported      :954                       */
    /* inputs on which the reference Go code panics: defined here, no counters */
    EMURX_ST_PANIC_L4LEN = 27,       /* IPv4 totlen < IHL, span slice p[L4:L4+l4len] :597,628,644,689 */
    EMURX_ST_PANIC_IPV6_OPT = 28,    /* processIpv6Options reads p[i+1] past the header :738  */
    EMURX_ST_PANIC_NIL_EAPOL = 29,   /* EAPOL with dot1x unregistered: nil ParserCb :789       */
    EMURX_ST_PANIC_MBUF = 30,        /* ZMQ frame > 9216 B: MbufPoll.Alloc panics, mbuf.go:106 */
    EMURX_NUM_STATUS = 31
};
/* status of the record written for an empty descriptor slot (EMURX_DESC_HOLE): no frame, no
   Namespace (ns_id = client_id = EMURX_ID_NONE), proto EMURX_CB_NONE, not counted */
#define EMURX_ST_HOLE 0xFFu

/* ---- lookup outcome of the callback's Namespace/Client rule (record.flags bits 4..6) -- */
enum emurx_lookup {
    EMURX_LK_NONE = 0,             /* not attempted: no callback is invoked for the frame */
    EMURX_LK_NO_NS = 1,            /* GetNs(ps.Tun) == nil                                */
    EMURX_LK_NS_NO_PLUGIN = 2,     /* ns.PluginCtx.Get(<plugin>) == nil                   */
    EMURX_LK_NS_LEVEL = 3,         /* namespace-level dispatch, no client key (igmp, mdns,
                                      ipv6 non-echo, arp reply)                           */
    EMURX_LK_NO_CLIENT = 4,        /* the rule's key resolved no (acceptable) client     */
    EMURX_LK_CLIENT_NO_PLUGIN = 5, /* client found, client.PluginCtx.Get(<plugin>) == nil */
    EMURX_LK_CLIENT = 6            /* client_id is valid                                  */
};
#define EMURX_FLAG_RTALERT 0x01u   /* IPV6_M_RTALERT_ML, parser.go:48 */
#define EMURX_FLAG_LK_SHIFT 4
#define EMURX_FLAG_LK_MASK 0x70u

/* ---- wire/device data structures ------------------------------------------------------ */
/* frame descriptor: byte offset of the frame in the batch buffer, its length and vport.
   (The ZMQ per-frame header 0xAA|vport|len, veth_zmq.go:296-305, carries the same fields.) */
typedef struct emurx_desc {
    uint32_t off;
    uint16_t len;
    uint8_t vport;
    uint8_t pad;   /* 0, EMURX_DESC_HOLE, or the frame's owner key (EMURX_DESC_KEYED) */
} emurx_desc;
/* pad value of an empty descriptor slot: no frame, no record, no queue entry, not counted
   (the batched ingest leaves one for every frame a message announced but did not carry) */
#define EMURX_DESC_HOLE 0xFFu
/* pad = EMURX_DESC_KEYED | k (k <= 126): the frame's Namespace-owner key, a 7-bit digest of
   the CTunnelKey its parse leaves (vport and the dot1q / QinQ words of its first 22 bytes,
   parser.go:801-818).  The device framing walk of the batched ingest writes it with every
   descriptor (it reads the frame's header there anyway); emurx_desc_keys_dev writes it for
   descriptors built elsewhere; emurx_owner_key gives it for a key.  With keyed descriptors
   emurx_parse_route_dev counts the owners from the descriptors alone instead of re-reading
   every frame's header.  A key that does not match the frame misroutes that frame. */
#define EMURX_DESC_KEYED 0x80u

/* 32-byte record, one per frame, in frame order.  The numeric fields are exactly the
   ParserPacketState the reference hands to a ParserCb (parser.go:51-61) plus the
   CTunnelData that makes ps.Tun (thread_ctx.go:37-40), the callback tag, the outcome and
   the resolved Namespace / Client ids. */
typedef struct emurx_rec {
    uint32_t ns_id;     /* id given at emurx_ns_add, or EMURX_ID_NONE                      */
    uint32_t client_id; /* id given at emurx_client_add, or EMURX_ID_NONE                  */
    uint32_t vlan[2];   /* CTunnelData.Vlans: (TPID<<16)|VID, PCP/DEI cleared, 0 if absent */
    uint16_t vport;     /* CTunnelData.Vport                                               */
    uint16_t l3;        /* ParserPacketState.L3                                            */
    uint16_t l4;        /* ParserPacketState.L4                                            */
    uint16_t l7;        /* ParserPacketState.L7                                            */
    uint16_t l7_len;    /* ParserPacketState.L7Len (uint16 wraparound preserved)           */
    uint8_t next_hdr;   /* ParserPacketState.NextHeader                                    */
    uint8_t proto;      /* enum emurx_cb of the callback reached, EMURX_CB_NONE on errors  */
    uint8_t status;     /* enum emurx_status                                               */
    uint8_t flags;      /* bit0 EMURX_FLAG_RTALERT (ps.Flags); bits 4..6 enum emurx_lookup */
    uint16_t rsv;
} emurx_rec;

/* Outcome histogram: EMURX_HIST_BINS × {pkts, bytes}.  Bin = hist_bin(status, proto).
   Counter deltas are derived from it by emurx_hist_to_counters(). */
#define EMURX_HIST_BINS 64
#define EMURX_HIST_BIN(status, proto) \
    ((status) <= EMURX_ST_NOT_SUPPORTED ? (unsigned)(status) * EMURX_NUM_CB + (unsigned)(proto) \
                                        : 2u * EMURX_NUM_CB + (unsigned)(status) - 2u)

/* ParserStats in declaration order, parser.go:67-119 (all uint64). */
enum emurx_parser_counter {
    EMURX_PC_errInternalHandler = 0, EMURX_PC_errParser, EMURX_PC_errEAPolTooShort,
    EMURX_PC_errArpTooShort, EMURX_PC_errIcmpv4TooShort, EMURX_PC_errIgmpv4TooShort,
    EMURX_PC_errUdpTooShort, EMURX_PC_errTcpTooShort, EMURX_PC_errDot1qTooShort,
    EMURX_PC_errToManyDot1q, EMURX_PC_errIPv4TooShort, EMURX_PC_errIPv4HeaderTooShort,
    EMURX_PC_errIPv4Fragment, EMURX_PC_errIPv4cs, EMURX_PC_errTCP, EMURX_PC_errUDP,
    EMURX_PC_eapolPkts, EMURX_PC_eapolBytes, EMURX_PC_arpPkts, EMURX_PC_arpBytes,
    EMURX_PC_icmpPkts, EMURX_PC_icmpBytes, EMURX_PC_igmpPkts, EMURX_PC_igmpBytes,
    EMURX_PC_dhcpPkts, EMURX_PC_dhcpBytes, EMURX_PC_dhcpSrvPkts, EMURX_PC_dhcpSrvBytes,
    EMURX_PC_mDnsPkts, EMURX_PC_mDnsBytes, EMURX_PC_tcpPkts, EMURX_PC_tcpBytes,
    EMURX_PC_udpPkts, EMURX_PC_udpBytes, EMURX_PC_udpCsErr, EMURX_PC_tcpCsErr,
    EMURX_PC_errIPv6TooShort, EMURX_PC_errIPv6HopLimitDrop, EMURX_PC_errIPv6Empty,
    EMURX_PC_errIPv6OptJumbo, EMURX_PC_errIPv6Fragment, EMURX_PC_errIcmpv6TooShort,
    EMURX_PC_errIcmpv6Cse, EMURX_PC_errIcmpv4Cse, EMURX_PC_errIcmpv6Unsupported,
    EMURX_PC_Icmpv6Pkt, EMURX_PC_Icmpv6Bytes, EMURX_PC_errL4ProtoUnsupported,
    EMURX_PC_errL3ProtoUnsupported, EMURX_PC_errPacketIsTooShort,
    EMURX_NUM_PARSER_COUNTERS
};

typedef struct emurx_counters {
    uint64_t parser[EMURX_NUM_PARSER_COUNTERS]; /* ParserStats deltas (parse-side errParser
                                                   included; callback returns are added by
                                                   the caller, thread_ctx.go:365-375)      */
    uint64_t rx_pkts;      /* VethStats.RxPkts    veth_zmq.go:233 */
    uint64_t rx_bytes;     /* VethStats.RxBytes   veth_zmq.go:234 */
    uint64_t rx_batch;     /* VethStats.RxBatch   veth_zmq.go:278 */
    uint64_t rx_parse_err; /* VethStats.RxParseErr veth_zmq.go:281-312 */
    uint64_t ref_panic;    /* frames with an EMURX_ST_PANIC_* status (reference would abort) */
} emurx_counters;

typedef struct emurx_cfg {
    int device;            /* HIP device ordinal; < 0: a host-only handle (the table mirror,
                              generations and image queries, no device: data-path calls
                              return EMURX_EDEVICE) */
    uint32_t max_ns;       /* ns ids must be < max_ns */
    uint32_t max_clients;  /* client ids must be < max_clients.  The device tables are sized
                              for max_ns / max_clients and kept sparse so that a lookup
                              almost always ends in its home bucket (one memory trip for a
                              wave of 64 lookups): about 128 B of device memory per Namespace
                              and 1.7 KB per client (MAC, IPv4, IPv6, client info), 1/n_parts
                              of that when partitioned.  The memory is traded for lookup
                              latency: a table that would pass 2 GiB, or whose device
                              allocation fails, is built at half the spread (down to 2 slots
                              per entry: more probe trips) instead of failing;
                              env EMURX_TABLE_SPREAD="ns,mac,ip,ci" (slots per entry, powers of
                              two >= 2; default 8,8,16,16) sets the spreads */
    uint32_t max_frames;   /* frames per batch (device scratch is sized for it) */
    uint32_t max_bytes;    /* bytes per host batch (emurx_rx_stream staging) */
} emurx_cfg;

/* Device-resident outputs of one batch (all pointers are device memory).
   Frames are processed in tiles of EMURX_QUEUE_TILE (frame i is in tile i / TILE).  Each
   callback owns a region of qlist, and each tile a segment of that region: the indices of
   tile t's frames that reach callback q are, in frame order,
       qlist[q*qcap + t*TILE .. q*qcap + t*TILE + tile_cnt[t*16 + q])
   so queue q (EMURX_Q_DROP = no callback) is the concatenation of its segments over t.
   The histogram is kept as EMURX_HIST_SHARDS accumulating copies (fold them with
   emurx_hist_fold).  rec / qlist / tile_cnt may individually be NULL; hist is required. */
#define EMURX_QUEUE_TILE 256
#define EMURX_HIST_SHARDS 64
typedef struct emurx_dev_out {
    emurx_rec* rec;        /* [n] records, frame order                                     */
    uint32_t* qlist;       /* [EMURX_NUM_QUEUES * qcap] frame indices                       */
    uint32_t qcap;         /* per-queue region, >= ceil(n / TILE) * TILE                    */
    uint32_t* tile_cnt;    /* [ceil(n / TILE) * 16] frames per (tile, queue), 13 used of 16  */
    uint64_t* hist;        /* [EMURX_HIST_SHARDS * 2 * EMURX_HIST_BINS], ACCUMULATED         */
    uint32_t* flow;        /* [n] transport flow outcome (EMURX_FLOW_* / flow id), or NULL   */
} emurx_dev_out;

/* Transport flow outcome per frame (emurx_dev_out.flow), the decision
   TransportCtx.handleRxPacket (src/emu/plugins/transport/client_ctx.go:912-969) takes before
   any socket code runs.  Only frames that reach a client's transport handler get one of these
   (tcp / udp callback, lookup EMURX_LK_CLIENT); the key is the reference's c5tuplekey
   (client_ctx.go:44-112): src, dst, src port, dst port, protocol (IPv4: the header's protocol
   field; IPv6: ParserPacketState.NextHeader). */
#define EMURX_FLOW_NONE 0xFFFFFFFFu      /* the transport handler is not reached              */
#define EMURX_FLOW_NO_CTX 0xFFFFFFF0u    /* client without a TransportCtx: handler returns -1
                                            (PluginTransClient.handleRxTransPacket :73-80)     */
#define EMURX_FLOW_NO_SYN 0xFFFFFFF1u    /* new TCP flow without a bare SYN (ft_new_tcp_no_syn) :840-844 */
#define EMURX_FLOW_NO_SERVER 0xFFFFFFF2u /* new flow, no listener on the port (ft_new_no_cb) :848-853,884-887 */
#define EMURX_FLOW_NEW 0xFFFFFFF3u       /* new flow with a listener: OnAccept runs in Go :855-868,890-903 */
#define EMURX_FLOW_UNKNOWN 0xFFFFFFF4u   /* emurx_lookup_dev only: the handler is reached but the head came
                                            without its c5tuplekey (the source's handle saw no TransportCtx,
                                            or the tuple did not fit its tail shard): the caller decides */
#define EMURX_FLOW_ID_MAX 0xFFFFFFEFu    /* flow ids are 0 .. EMURX_FLOW_ID_MAX                */

typedef struct emurx_ctx emurx_t;

/* ---- lifecycle --------------------------------------------------------------------- */
int emurx_abi_version(void);
int emurx_open(const emurx_cfg* cfg, emurx_t** out);
void emurx_close(emurx_t* h);
const char* emurx_strerror(int code);

/* ---- parser registration (Parser.Register / Init, parser.go:528-581) ------------------ */
int emurx_register(emurx_t* h, const char* protocol);     /* "arp","icmp",...,"transport" */
int emurx_set_callbacks_mask(emurx_t* h, uint32_t mask);  /* bit i = enum emurx_cb i live */
uint32_t emurx_get_callbacks_mask(const emurx_t* h);

/* ---- table sync (control plane runs on the same goroutine as rx) ---------- */
/* key = CTunnelKey bytes (thread_ctx.go:58,92-97): [0:2] vport LE, [2:4] 0, [4:8] Vlans[0] LE,
   [8:12] Vlans[1] LE. */
int emurx_ns_add(emurx_t* h, const uint8_t key[12], uint32_t ns_id, uint32_t plugin_mask);
int emurx_ns_remove(emurx_t* h, const uint8_t key[12]);
int emurx_ns_set_plugins(emurx_t* h, uint32_t ns_id, uint32_t plugin_mask);
/* ipv4 / ipv6 / dhcpv6 may be NULL or all-zero (= absent, as Ipv4Key.IsZero etc.). */
int emurx_client_add(emurx_t* h, uint32_t ns_id, uint32_t client_id, const uint8_t mac[6],
                     const uint8_t ipv4[4], const uint8_t ipv6[16], const uint8_t dhcpv6[16],
                     uint32_t plugin_mask);
/* ctx_client_add (ApiClientAddHandler rpc_base_cmds.go:350-406): a list of clients, each
   through CNSCtx.AddClient in order; stops at the first error and returns it, *n_added =
   clients added before it.  Zero address fields mean absent. */
typedef struct emurx_client_spec {
    uint32_t ns_id, client_id, plugin_mask;
    uint8_t mac[6], ipv4[4], ipv6[16], dhcpv6[16];
    uint8_t pad[2];
} emurx_client_spec; /* 56 bytes */
int emurx_clients_add(emurx_t* h, const emurx_client_spec* clients, uint32_t n, uint32_t* n_added);
int emurx_client_remove(emurx_t* h, uint32_t ns_id, const uint8_t mac[6]);
int emurx_client_set_plugins(emurx_t* h, uint32_t client_id, uint32_t plugin_mask);
int emurx_client_update_ipv4(emurx_t* h, uint32_t client_id, const uint8_t ipv4[4]);
int emurx_client_update_ipv6(emurx_t* h, uint32_t client_id, const uint8_t ipv6[16]);
int emurx_client_update_dipv6(emurx_t* h, uint32_t client_id, const uint8_t dhcpv6[16]);
int emurx_client_set_ra(emurx_t* h, uint32_t client_id, const uint8_t prefix[16],
                        uint8_t prefix_len);
/* Transport flow tables.  A flow key is the reference's tuple bytes: 13 for IPv4
   (c5tuplekeyv4: src[4] dst[4] sport BE dport BE proto), 37 for IPv6 (c5tuplekeyv6: src[16]
   dst[16] sport dport next header), as buildTuplev4/v6 (client_ctx.go:89-112) builds it from a
   received frame.  flow_add / flow_remove mirror TransportCtx.addFlowv4/6 / removeFlowv4/6
   (client_ctx.go:597-651); server_add / server_remove the listener map serverCb
   (lookupServerPort :1142-1155, proto 6 or 17).  Adding either marks the client as having a
   TransportCtx (created on first use, socketApi.go:174-193); client_set_transport sets or
   clears that mark directly.  Removing a client drops its flows and listeners. */
int emurx_flow_add(emurx_t* h, uint32_t client_id, const uint8_t* tuple, uint32_t tuple_len, uint32_t flow_id);
int emurx_flow_remove(emurx_t* h, uint32_t client_id, const uint8_t* tuple, uint32_t tuple_len);
int emurx_server_add(emurx_t* h, uint32_t client_id, uint16_t port, uint8_t proto);
int emurx_server_remove(emurx_t* h, uint32_t client_id, uint16_t port, uint8_t proto);
int emurx_client_set_transport(emurx_t* h, uint32_t client_id, int has_ctx);
/* Table edits reach the device incrementally: every call above edits the slots of the
   device table image it changes (deleted slots become tombstones) and marks the 64-byte
   blocks it touched.  Before the next launch that reads the tables, the edited blocks are
   copied to the device and scattered by one kernel on that launch's stream, ordered after
   every launch on any stream that read the tables since the previous shipment (stream
   events, no host synchronisation) and before every later reader.  A table that outgrows
   its load factor is rebuilt larger and shipped whole (then the host waits for the device
   once).  Streams given to the library must outlive the handle.
   emurx_sync ships pending edits now, on `stream` (NULL = the handle's stream). */
int emurx_sync(emurx_t* h, void* stream);
/* diagnostics: 64-byte blocks shipped as deltas and whole tables uploaded since emurx_open,
   and the bytes of this handle's device tables (any pointer may be NULL) */
int emurx_table_stats(const emurx_t* h, uint64_t* delta_blocks, uint64_t* whole_tables, uint64_t* image_bytes);

/* Partitioned tables (multi-GPU, one handle per GPU): with n_parts > 1 this handle's device
   tables hold only the Namespaces with emurx_ns_owner(key, n_parts) == part and their
   clients, flows and listeners; the host maps stay complete, so every table call keeps Go's
   semantics and return codes.  Device memory per handle ~ 1/n_parts of the tables.
   Rebuilds and ships every table.  (1, 0) = replicated (the default). */
int emurx_set_partition(emurx_t* h, uint32_t n_parts, uint32_t part);

/* ---- mid-batch table mutations ---------------------------------------
   A batch is classified against the tables as they stand when it is launched (a snapshot);
   the Go loop dispatches its records in frame order, and a callback may mutate the maps
   (DHCP's UpdateClientIpv4 dhcp.go:718, a TCP accept adding a flow) before later frames of
   the same batch are dispatched, which Go would classify against the mutated maps.
   emurx_table_gen() is the generation of the tables (it advances on every mutation); read it
   when launching a batch.  While dispatching, a record whose emurx_recs_stale flag is set
   may differ from what the live maps give (its Namespace was added, removed or mutated --
   any of its clients, addresses, plugins, RA prefix, flows -- after that generation): the
   caller re-probes it in its own maps.  Unflagged records equal the live classification. */
uint64_t emurx_table_gen(const emurx_t* h);
int emurx_recs_stale(const emurx_t* h, const emurx_rec* rec, uint32_t n, uint64_t gen, uint8_t* stale);

/* The device tables' answer for a key, computed on the host image by the kernels' bucket walk
   (tests of the incremental maintenance).  table: 0 ns {vport, vlan0, vlan1} -> ns id,
   1 mac {ns, mac lo, mac hi} -> client, 2 ipv4 {ns, ip} -> client, 3 ipv6 {ns, ip[4]} -> client,
   4 client info {client} -> plugin mask, 5 flow4 {client, src, dst, ports, proto} -> flow,
   6 flow6 {client, src[4], dst[4], ports, nh} -> flow, 7 listener {client, port | proto << 16} -> 1
   (words little-endian as in the tables).  EMURX_ENOENT when absent. */
int emurx_image_lookup(emurx_t* h, uint32_t table, const uint32_t* key, uint32_t* value);
/* The same walk with its trace (tests that need keys at chosen places of a table: long chains,
   the step across the table's end, tombstones).  Tables, key words and return codes as
   emurx_image_lookup.  out[0] the value (EMURX_ID_NONE when absent), out[1] the table's bucket
   count, out[2] the key's home bucket, out[3] buckets the walk read, out[4] 1 if it stepped
   from the last bucket to bucket 0, out[5] tombstone slots it passed.  A mac / ipv4 / ipv6 key
   whose Namespace is not alive reads no bucket: EMURX_ENOENT, out all zero. */
int emurx_image_probe(emurx_t* h, uint32_t table, const uint32_t* key, uint32_t out[6]);
/* The hash emurx_learn_dev's two sets place a key by (tests that need keys at chosen places of
   the sets: chains, the step from the last slot to slot 0, owners with an equal tag).  key: the
   key's seven words as the kernels hold them: ns id, the IP as four little-endian words (ARP: the
   IPv4 address, then zeros), the MAC's bytes 0..3, its bytes 4..5 | kind (EMURX_LRN_*) << 16.
   The workgroup's set of 512 slots starts the key at (h >> 9) & 511; the global set of a batch
   of n frames has the smallest power of two >= max(128, 2 n) slots, starts the key at
   h & (slots - 1) and tags the slot's owner with h >> 27; both probe linearly and wrap. */
uint32_t emurx_learn_key_hash(const uint32_t key[7]);
/* Compare the device tables with the host image after a shipment (synchronises the handle's
   stream): *mismatched = 32-bit words that differ. */
int emurx_image_check(emurx_t* h, uint64_t* mismatched);

/* ---- data path ---------------------------------------------------------------------- */
/* Host batch, ZMQ wire format (veth_zmq.go:8-22).  Decodes the stream exactly like
   OnRxStream (uint16 running offset, abort-on-header-error), stages it in pinned memory,
   parses + classifies on the GPU and returns records in frame order plus per-queue frame
   index lists.  out_qoff[q]..out_qoff[q+1] indexes out_qlist for queue q
   (out_qoff has EMURX_NUM_QUEUES+1 entries).  *n_out = frames decoded.  `delta` receives
   the ParserStats + VethStats deltas of this batch. */
int emurx_rx_stream(emurx_t* h, const uint8_t* msg, size_t len, emurx_rec* out_rec,
                    uint32_t* out_qlist, uint32_t out_cap, uint32_t* n_out,
                    uint32_t out_qoff[EMURX_NUM_QUEUES + 1], emurx_counters* delta);

/* Device-resident batch: frames (d_frames) and descriptors (d_desc) already in HBM.
   Enqueues parse+classify+compaction on `stream` (hipStream_t, NULL = handle stream) and
   returns without synchronising.  out->hist is accumulated into (zero it to reset).
   n <= cfg.max_frames, out->qcap >= ceil(n / EMURX_QUEUE_TILE) * EMURX_QUEUE_TILE.
   d_frames must be 16-byte aligned and d_desc 8-byte aligned (EMURX_EINVAL otherwise), and
   the frame buffer must stay readable up to the next 64-byte boundary past its last byte
   (frames are staged with 16-byte loads).  One k_rx launch; when table edits are pending
   (emurx_ns_* / emurx_client_* since the last launch) a k_apply launch and cross-stream
   events go ahead of it, and a whole-table or growing shipment synchronises the host with
   the stream (or the device).  Not capturable in a hipGraph: the kernel arguments carry the
   table addresses, which a later table growth reallocates; a capturing stream gets
   EMURX_EINVAL before anything is enqueued (the same for emurx_classify_route_dev,
   emurx_parse_route_dev, emurx_lookup_dev and emurx_route_dev, whose scratch may be allocated
   or change streams behind an event).  Call emurx_sync first to take the shipment out of a
   latency-critical call.  No emurx_* call reads or clears the thread's last HIP error
   (hipGetLastError): a launch's status is hipLaunchKernel's return value, so an error a
   caller's earlier HIP call left pending is still pending after the call (the one exception:
   the out-of-memory status of a table allocation the library recovered from, emurx_cfg). */
int emurx_classify_dev(emurx_t* h, const uint8_t* d_frames, const emurx_desc* d_desc,
                       uint32_t n, const emurx_dev_out* out, void* stream);

/* Device-resident, parse only (no table lookups): records with ns_id/client_id NONE and
   lookup EMURX_LK_NONE (ParsePacket alone).  The multi-GPU path uses emurx_parse_route_dev,
   which parses and packs the lookup records for the Namespace owners in the same pass. */
int emurx_parse_dev(emurx_t* h, const uint8_t* d_frames, const emurx_desc* d_desc,
                    uint32_t n, const emurx_dev_out* out, void* stream);

/* Build descriptors for a ZMQ message on the host (the sequential offset walk of
   OnRxStream).  Returns frames decoded in *n_out; *parse_err = 1 when the walk stopped on a
   header error (RxParseErr).  Frames longer than EMURX_MAX_FRAME stop the walk with
   *parse_err = 2 (the reference panics there). */
int emurx_zmq_descriptors(const uint8_t* msg, size_t len, emurx_desc* out, uint32_t cap,
                          uint32_t* n_out, int* parse_err);

/* ---- batched host ingest: many ZMQ messages per GPU round trip -------
   The per-message loop of VethIFZmq.OnRxStream (veth_zmq.go:277-320) over a whole batch of
   messages, with the framing walk on the GPU (one lane per message, same uint16 offset and
   abort-on-header-error rules as emurx_zmq_descriptors), then parse + classify (k_rx), then
   the per-callback queues packed on the GPU.  Several slots let the caller fill one pinned
   staging buffer while the other slots' batches are in flight (a slot's buffers are allocated
   at its first emurx_ingest_buffer: unused slots cost nothing):

       buf = emurx_ingest_buffer(h, s, bytes)    pinned host memory owned by the library
       ... the caller writes ZMQ messages into buf (the receive copy it does anyway) ...
       emurx_ingest_submit(h, s, msgs, nmsg)     H2D + 4 launches + D2H, returns at once
       emurx_ingest_wait(h, s, &res)             results of slot s, valid until its next submit

   Frames are numbered in message order, then wire order (the order the Go loop handles
   them).  res.desc[i].off is the frame's offset in the slot's buffer.  Counters in res.delta
   are those of OnRxStream called once per message (RxBatch = nmsg). */
#define EMURX_INGEST_SLOTS 4
#define EMURX_MSG_OK 0u          /* every announced frame decoded                           */
#define EMURX_MSG_PARSE_ERR 1u   /* RxParseErr: the walk stopped on a header error           */
#define EMURX_MSG_PANIC 2u       /* the reference panics: frame > 9216 B or offset wrap      */
typedef struct emurx_msg {
    uint32_t off; /* message start in the slot buffer (any alignment) */
    uint32_t len; /* message bytes                                    */
} emurx_msg;
typedef struct emurx_ingest_result {
    const emurx_rec* rec;        /* [n_frames] records, frame order                         */
    const emurx_desc* desc;      /* [n_frames] frame offset / length / vport in the buffer  */
    const uint32_t* qlist;       /* [n_frames] frame indices grouped by queue (qoff)        */
    const uint32_t* msg_frames;  /* [n_msgs] frames decoded from each message               */
    const uint8_t* msg_status;   /* [n_msgs] EMURX_MSG_*                                    */
    uint32_t n_frames;
    uint32_t n_msgs;
    uint32_t qoff[EMURX_NUM_QUEUES + 1];
    emurx_counters delta;        /* ParserStats + VethStats deltas of the batch             */
    uint32_t one_launch;         /* 1: the batch ran as one kernel (k_ingest_small, the
                                    small-batch path), 0: the copy + four-launch pipeline (always
                                    with answers on, emurx_ingest_set_answers: the one-launch path
                                    never brings the frames into device memory)              */
    uint32_t degraded;           /* 1: a one-launch batch whose workgroups did not all arrive
                                    within the wait bound (EMURX_INGEST_SPIN_US, default 200 us,
                                    read at emurx_open, plus 0.1 ns per byte of the batch's
                                    messages: at most 1.2 ms; 0 forces it): its queues were
                                    packed by the last workgroup from device scratch.  Same
                                    results.                                                    */
} emurx_ingest_result;
/* Pinned staging buffer of slot s (0 <= s < EMURX_INGEST_SLOTS) with room for `bytes`
   (grown on demand; not while the slot has a batch in flight). */
int emurx_ingest_buffer(emurx_t* h, uint32_t slot, size_t bytes, uint8_t** buf);
/* Enqueue the slot's messages.  EMURX_ENOSPC when the messages could announce more frames
   than cfg.max_frames (split the batch) or, with answers on (emurx_ingest_set_answers), end past
   cfg.max_bytes; EMURX_EINVAL for a message outside the buffer or a slot still in flight. */
int emurx_ingest_submit(emurx_t* h, uint32_t slot, const emurx_msg* msgs, uint32_t nmsg);
/* Wait for the slot's batch and point `res` at its results (library-owned pinned memory). */
int emurx_ingest_wait(emurx_t* h, uint32_t slot, emurx_ingest_result* res);
/* The framing walk alone on messages already in device memory (the first stage of the
   batched ingest, k_zmq_walk): one lane per message follows OnRxStream's offset chain
   (veth_zmq.go:277-320) and writes the descriptors of its frames, each with its Namespace-owner
   key (EMURX_DESC_KEYED, from the frame's bytes 12..19: what emurx_parse_route_dev's owner
   count reads instead of the frame), and msg_stat[m] = frames | EMURX_MSG_* << 24.  d_ctl:
   emurx_msg[nmsg] then slot_base[nmsg + 1] (message m's descriptor slots are
   [slot_base[m], slot_base[m + 1]); slots a message announced but did not carry become
   EMURX_DESC_HOLE).  The buffer must be readable 32 bytes past every message.  flags:
   EMURX_WALK_NO_KEYS leaves the pad byte 0 (for the measurement of what the keys cost; the
   bench folds the difference into the exchange's rate).  One launch, no host sync. */
#define EMURX_WALK_NO_KEYS 1u
int emurx_zmq_walk_dev(emurx_t* h, const uint8_t* d_buf, const uint32_t* d_ctl, uint32_t nmsg, emurx_desc* d_desc,
                       uint32_t* d_msg_stat, uint32_t flags, void* stream);
/* The slot's HIP stream (hipStream_t, created on first use), so that a caller can order its
   own work with the slot's batches: make the next batch wait for a device-side producer
   (hipStreamWaitEvent before emurx_ingest_submit), or chain a consumer after the D2H. */
int emurx_ingest_stream(emurx_t* h, uint32_t slot, void** stream);

/* ---- tx-side checksum generation -----------------------------------
   What the plugins' tx paths do to a frame before Veth.Send, for a batch of frames in
   device memory, in place.  Per frame, `ops` selects:
     EMURX_TX_IPV4_HDR   IPv4Header(p[l3:l3+IHL*4]).UpdateChecksum()         ip4.go:132-136
                   (the callers' slice is the whole header: 20 B in transport, tcp_output.go:110-112;
                   24 B with IGMP's router-alert option, igmp.go:1179-1186)
   and one L4 kind (ops >> EMURX_TX_L4_SHIFT), the field zeroed first, the span p[l4:len]:
     TCP4 / UDP4   p[l4+16 | l4+6] = PktChecksumTcpUdp(p[l4:], 0, IPv4Header(p[l3:l3+20]))
                   tcpip.go:38-40 + ip4.go:49-58 (callers tcp_output.go:64-70, udp.go:143-150)
     TCP6 / UDP6 / ICMP6   IPv6Header(p[l3:l3+40]).FixL4ChecksumOffset(p[l4:], osize, 16 | 6 | 2)
                   ip6.go:40-56,127-134 (tcp_output.go:71-76, udp.go:151-156, ipv6/nd.go:1111);
                   with EMURX_TX_V6_NH the pseudo header's next header is `nh` instead of
                   o.NextHeader(): PktChecksumTcpUdpV6(p[l4:], 0, ipv6, osize, nh) tcpip.go:34-36
                   (MLD reports behind a hop-by-hop header, ipv6/mld.go:1271)
     ICMP4         ICMPv4Header(p[l4:]).UpdateChecksum()                      icmp4.go:252-256
   A frame whose header or field would lie past `len` (the Go slices panic there) is left
   untouched and gets status EMURX_TX_RANGE; so does a kind that is none of the six.  The IPv4
   header slice is IHL * 4 bytes and never fewer than the 20 every caller takes.
   `len` up to 65535 is accepted (an L4 span that long is summed exactly).  The frames of one
   call must not overlap: each is rewritten independently of the others, in no given order. */
#define EMURX_TX_IPV4_HDR 0x01u
#define EMURX_TX_V6_NH 0x02u
#define EMURX_TX_L4_SHIFT 4
enum emurx_tx_l4 {
    EMURX_TX_L4_NONE = 0,
    EMURX_TX_L4_TCP4 = 1,
    EMURX_TX_L4_UDP4 = 2,
    EMURX_TX_L4_TCP6 = 3,
    EMURX_TX_L4_UDP6 = 4,
    EMURX_TX_L4_ICMP6 = 5,
    EMURX_TX_L4_ICMP4 = 6
};
#define EMURX_TX_OK 0u
#define EMURX_TX_RANGE 1u
typedef struct emurx_tx_desc {
    uint32_t off;      /* frame start in the buffer                              */
    uint16_t len;      /* frame length (the L4 span ends here)                   */
    uint16_t l3, l4;   /* header offsets in the frame                            */
    uint16_t osize;    /* IPv6 extension bytes given to FixL4ChecksumOffset      */
    uint8_t ops;       /* EMURX_TX_IPV4_HDR | EMURX_TX_V6_NH | kind << EMURX_TX_L4_SHIFT */
    uint8_t nh;        /* pseudo-header next header with EMURX_TX_V6_NH          */
    uint8_t pad[2];
} emurx_tx_desc;       /* 16 bytes */
/* d_frames: device buffer, rewritten in place; d_status: [n] EMURX_TX_* (may be NULL).
   One launch on `stream`, no host synchronisation. */
int emurx_tx_checksum_dev(emurx_t* h, uint8_t* d_frames, const emurx_tx_desc* d_desc, uint32_t n,
                          uint8_t* d_status, void* stream);

/* ---- tx framing: VethIFZmq.Send / FlushTx (src/emu/core/veth_zmq.go:149-200) ------------
   The n frames desc[i] = {off, len, vport} of d_frames, in order, are packed into ZMQ
   messages exactly as n consecutive Send calls followed by one FlushTx would pack them:
     a frame whose length would bring the open message's frame bytes to
     ZMQ_TX_MAX_BUFFER_SIZE or more first closes it (:186-188); a message closes at
     ZMQ_TX_PKT_BURST_SIZE frames (:198-200);
     message = BE32 EMURX_ZMQ_MAGIC << 16 | frames (:157-159), then per frame
     BE32 0xAA << 24 | vport << 16 | len (:167-169) and the frame's bytes.
   The messages land back to back in d_out.  d_msg_off[m] (u64) is message m's start and
   d_msg_off[n_msgs] the total; capacity n + 1.  d_info = {n_msgs, total bytes}.  Nothing is
   written at or past out_cap; out_cap >= 8 * n + sum(len) always suffices, and d_info
   tells the size needed when it did not.  d_out 16-byte aligned; the frames are read as
   the aligned 16-byte blocks that hold them.  n < EMURX_TX_ZMQ_MAX_FRAMES.  Two launches on
   `stream` (the chain scan, then the write), no host synchronisation; calls on different
   streams of one handle share its scratch, so they must not overlap.  Replaces
   VethIFZmq.FlushTx's per-frame append loop. */
#define EMURX_ZMQ_TX_BURST 64u            /* ZMQ_TX_PKT_BURST_SIZE  veth_zmq.go:36 */
#define EMURX_ZMQ_TX_MAX_BUFFER 32768u    /* ZMQ_TX_MAX_BUFFER_SIZE veth_zmq.go:37 */
#define EMURX_ZMQ_PKT_MAGIC 0xAAu         /* per-frame header tag   veth_zmq.go:167 */
#define EMURX_TX_ZMQ_MAX_FRAMES (1u << 26) /* n must be below it (else EMURX_EINVAL)       */
int emurx_tx_zmq_dev(emurx_t* h, const uint8_t* d_frames, const emurx_desc* d_desc, uint32_t n,
                     uint8_t* d_out, uint64_t out_cap, uint64_t* d_msg_off, uint64_t* d_info, void* stream);
/* The same framing with the frame count taken from device memory: the first min(*d_count, n_max)
   descriptors are framed exactly as emurx_tx_zmq_dev with that n would frame them (d_out,
   d_msg_off[0 .. n_msgs] and d_info).  *d_count (u64, 8-byte aligned) is read on the device when
   the kernels run, so a call enqueued behind the responder on the same stream takes d_count =
   the responder's d_info (word 0: replies written) and no host synchronisation sits between the
   two.  Descriptors at or past the count are never read (the responder leaves them
   unspecified), nor are the frames they would name.  d_msg_off has capacity n_max + 1; words
   past d_msg_off[n_msgs] are left as they were.  out_cap as above for the counted frames.
   n_max >= EMURX_TX_ZMQ_MAX_FRAMES, a NULL d_count, or the alignments above are EMURX_EINVAL;
   n_max == 0 writes a zero d_info and d_msg_off[0] = 0.  Two launches of n_max's size on
   `stream`, no host synchronisation; the same scratch and the same "must not overlap" rule as
   emurx_tx_zmq_dev.  The write's LDS image is the one the plain calls last chose; a counted
   call samples no feedback for that choice. */
int emurx_tx_zmq_counted_dev(emurx_t* h, const uint8_t* d_frames, const emurx_desc* d_desc,
                             uint32_t n_max, const uint64_t* d_count,
                             uint8_t* d_out, uint64_t out_cap, uint64_t* d_msg_off, uint64_t* d_info, void* stream);

/* ---- the tx planner: emurx_tx_desc from the frames themselves ------------------------------
   emurx_tx_checksum_dev wants {l3, l4, osize, ops, nh} per frame; the plugins' send paths know
   them while they build a frame, a caller that only holds finished frames does not.  The planner
   derives them with the header walk of the rx parser (src/emu/core/parser.go), without its
   checksum tests, so that what the library sends it also parses.  p: the frame, len: its length,
   be16: a big-endian byte pair.  Outcome per frame (enum emurx_txp) and descriptor:
     L2    len < 14 -> BAD.  EtherType at 12; each 0x8100 / 0x88a8 tag advances 4 bytes and needs
           the next EtherType inside len (else BAD); a third tag -> BAD (parser.go:700-741 accepts
           two).  l3 = the byte behind the EtherType.
     IPv4  0x0800 (parser.go:771-862): BAD unless len >= l3 + 20, version 4, IHL * 4 >= 20,
           len >= l3 + IHL * 4 and totlen >= IHL * 4.  From here on ops = EMURX_TX_IPV4_HDR and
           l4 = l3 + IHL * 4 (the end of the header that op sums, the rx record's l4).
           l3 + totlen != len -> LENGTH, the header op alone: the checksum call's L4 span is
           p[l4:len], as the Go callers slice it (tcp_output.go:64-70, udp.go:143-150), so a frame
           with bytes behind the datagram gets no L4 sum.
           be16(p + l3 + 6) & 0x3fff (fragment offset or MF) or a protocol that is none of 6 / 17 /
           1 -> HDR (IGMP with its 24-byte header, igmp.go:1179-1186, among them).
           Else kind TCP4 / UDP4 / ICMP4, outcome L4; BAD when len < l4 + 20 / 8 / 4 (the bytes
           up to the field the op clears).
     IPv6  0x86dd (parser.go:864-952): BAD unless len >= l3 + 40 and version 6.
           l3 + 40 + plen != len -> LENGTH with ops 0.
           While the next header is one of {0, 43, 50, 51, 60, 135, 139, 140} (the parser's set):
           the header is (p[o + 1] << 3) + 8 bytes; fewer than 8 bytes left or a header ending
           past len -> BAD.  A final next header 6 / 17 / 58 -> TCP6 / UDP6 / ICMP6, outcome L4,
           osize = l4 - l3 - 40 and, when osize > 0, ops |= EMURX_TX_V6_NH with nh = that next
           header (ipv6/mld.go:1271); the same minimum lengths (ICMPv6: 4).  Any other next
           header (44 and 59 among them) -> NONE.
     else  ARP, EAPOL, PPPoE and the rest -> NONE, ops 0.
   EMURX_TXP_UDP0_KEEP: a UDP checksum field that is 00 00 stays (IPv4: HDR, IPv6: NONE), for a
   caller whose plugins still run their own checksum calls, where a zero field means "not used"
   (DHCP sends it so); without the flag the field is computed.
   d_txdesc[i] = {off, len, l3, l4, osize, ops, nh, pad 0}, off and len from d_desc[i]; every
   field not named above is 0 (BAD, NONE and the IPv6 LENGTH: all of them), so the array compares
   bytewise.  d_outcome [n] may be NULL; d_info (u64[EMURX_TXP_INFO_WORDS]) = frames per outcome
   in enum order, then zeros; n == 0 writes a zero d_info.  d_desc 8-byte and d_txdesc 16-byte
   aligned; frames are read as the aligned 16-byte blocks that hold their first 96 bytes, and
   bytewise past that (IPv6 extension chains alone get there).  n > cfg.max_frames is
   EMURX_ENOMEM; a NULL pointer, an unknown flag bit, a misaligned array or a capturing stream
   EMURX_EINVAL; a host-only handle EMURX_EDEVICE.  One clear and one launch on `stream`, no host
   synchronisation and no allocation. */
#define EMURX_TXP_UDP0_KEEP 1u   /* flags: a UDP checksum field that is zero stays zero */
enum emurx_txp { EMURX_TXP_NONE = 0, EMURX_TXP_HDR = 1, EMURX_TXP_L4 = 2,
                 EMURX_TXP_LENGTH = 3, EMURX_TXP_BAD = 4 };
#define EMURX_TXP_INFO_WORDS 8   /* frames per outcome in enum order, then zeros */
int emurx_tx_plan_dev(emurx_t* h, const uint8_t* d_frames, const emurx_desc* d_desc, uint32_t n,
                      uint32_t flags, emurx_tx_desc* d_txdesc, uint8_t* d_outcome /* may be NULL */,
                      uint64_t* d_info, void* stream);

/* ---- egress slots: tx for a caller without device memory -----------------------------------
   What the ingest slots are to rx.  The caller appends outgoing frames and their descriptors
   into the slot's pinned memory, submits, and gets back finished ZMQ messages: planned
   (emurx_tx_plan_dev), checksummed (emurx_tx_checksum_dev) and framed as n Send calls and one
   FlushTx would leave them (emurx_tx_zmq_dev).
   emurx_egress_buffer returns the slot's pinned frame area (cfg.max_bytes bytes) and descriptor
   array (cfg.max_frames entries).  The first call on a slot allocates everything the slot will
   ever need (it waits for the device once and grows the handle's framing scratch to max_frames,
   as emurx_ingest_set_answers does), so that no submit allocates or synchronises.
   emurx_egress_submit: desc[i] = {off, len, vport, pad} names frame i in the frame area, the
   frames in send order and not overlapping; `bytes` = the part of the frame area in use; flags:
   the planner's.  It reads every descriptor once on the host, touches no frame byte, enqueues on
   the slot's own stream
     1. the H2D copies of `bytes` of frames and n descriptors,
     2. the planner, 3. the checksum launch, in place on the device copy,
     4. the framing (two launches) with out_cap = 8 n + bytes,
     5. one launch (k_egr_out) that reads the framing's counts on the device and writes the
        messages, msg_off, the two per-frame byte arrays and the info words straight into the
        slot's pinned result block, no more than was produced,
   and returns.  emurx_egress_wait blocks on the slot's event and points `res` at library memory,
   valid until the slot's next submit.  No host synchronisation between submit and wait.
   EMURX_EINVAL: a slot still in flight, slot >= EMURX_EGRESS_SLOTS, an unknown flag, a descriptor
   that ends past `bytes`, a wait with nothing submitted; EMURX_ENOMEM: n > cfg.max_frames;
   EMURX_ENOSPC: bytes > cfg.max_bytes; EMURX_EDEVICE: a host-only handle.
   The framing scratch and the write image's choice belong to the handle, and ingest slots with
   answers on use them too: an egress batch's framing joins the event hand-off of their answer
   stages (it waits for the previous stage's event and records its own), while the copies, the
   plan and the checksum of one egress slot overlap another slot's work.  A caller's own
   emurx_tx_zmq_dev / emurx_tx_zmq_counted_dev calls must not overlap an egress batch.
   INTEGRATION.md has the loop. */
#define EMURX_EGRESS_SLOTS 2
typedef struct emurx_egress_result {
    const uint8_t* msgs;        /* ZMQ messages back to back, emurx_tx_zmq_dev's layout      */
    const uint64_t* msg_off;    /* [n_msgs + 1] */
    uint32_t n_msgs, n_frames;
    uint64_t bytes;
    const uint8_t* plan;        /* [n_frames] enum emurx_txp                                  */
    const uint8_t* status;      /* [n_frames] EMURX_TX_OK / EMURX_TX_RANGE of the checksum call */
    uint64_t plan_info[EMURX_TXP_INFO_WORDS];
} emurx_egress_result;         /* 112 bytes */
int emurx_egress_buffer(emurx_t* h, uint32_t slot, uint8_t** frames, emurx_desc** desc);
int emurx_egress_submit(emurx_t* h, uint32_t slot, uint32_t n, uint64_t bytes, uint32_t flags);
int emurx_egress_wait(emurx_t* h, uint32_t slot, emurx_egress_result* res);

/* ---- the send side of ping: resident templates -------------------------------------------------
   Ping.sendPing (plugins/ping/ping.go:317-341) sends, per echo request, the packet that
   PreparePingPacketTemplate built once (plugins/icmp/icmp.go:208-237, plugins/ipv6/ipv6.go:216-262)
   with ten bytes changed: BE16 seq at icmp_off + 6, BE64 ts at icmp_off + 16 (one time.Now() per
   call; seq increments per frame and wraps at 2^16), and the checksum at icmp_off + 2 through
   UpdateChecksum2 / UpdateChecksum3 (gopacket layers/icmp4.go:238-285) on the live packet.  Frame
   k of any such chain carries
       cs = ~fold(~cs_t + ~seq_t + seq + sum over the four 16-bit words i of (~ts_t[i] + ts[i]))
   all terms added as integers and folded once, cs_t, seq_t, ts_t the template's own fields: this
   is also the full recompute over the patched frame, whenever the template's checksum field is
   not 0xffff (UpdateChecksum and FixIcmpL4Checksum write none for a type 8 / 128 message; with it
   the chain depends on its path).  So the templates live on the device and a sendPing call is one
   16-byte request however many frames it bursts.
   The store: emurx_pingtx_reserve(max_pings), once per handle, allocates it (EMURX_PINGTX_SLOT
   device bytes per ping and a host shadow) and everything the calls below need: none of them
   allocates.  A device slot is {u16 len, u16 icmp_off, u8 vport, 3 pad bytes} and the template's
   bytes; len == 0 marks a free slot; the id is the slot index.  The host keeps the length per id,
   so submit-time checks touch no template.
     reserve  EMURX_EEXIST a second call; EMURX_ENOMEM a failed allocation; EMURX_EDEVICE a
              host-only handle; EMURX_EINVAL max_pings == 0 or above 2^24.
     add      EMURX_EINVAL: no reserve before it, a NULL pointer, icmp_off + 24 > len (the
              timestamp must lie inside), len > EMURX_PINGTX_MAX_LEN (a large-payload ping stays on
              the Go path), vport > 255, a checksum field of 0xffff; EMURX_ENOSPC: the store is
              full.  *id = the lowest id that may be handed out.
     remove   EMURX_ENOENT: a free or out-of-range id (or no reserve).
   Edits are host calls that enqueue nothing.  They are shipped ahead of the next launch that reads
   the store, on that launch's stream, behind the work of every stream that read it since the last
   shipment; other streams wait for the shipment once, by event: the table shipment's rule
   (emurx_classify_dev).  A removed id is not handed out again until every egress batch with
   requests that was submitted before the remove has been waited for, so a batch in flight always
   reads the template it was submitted with.  A caller of emurx_pingtx_dev on streams of its own
   keeps that rule itself.  EMURX_PINGTX_SLOT bytes of device memory per reserved ping.
   The shipment's two host waits: its four staging buffers hold 1,024 edited slots each, so a
   launch behind more than 4,096 pending edits (a bulk add of 65,536 pings) waits on the host for
   its own earlier k_ptx_apply launches while it ships; and the 17th distinct stream to read the
   store since the last shipment drains the device once (hipDeviceSynchronize), as the table
   shipment does.  A launch with no edit pending, or with up to 4,096, waits for nothing on the
   host.  The library records an event on every stream that read the store since the last
   shipment: a caller's stream must outlive the next launch that ships an edit (or emurx_close);
   a destroyed one makes that launch fail with EMURX_EDEVICE. */
#define EMURX_PINGTX_SLOT 256u      /* device bytes per template: 8-byte head + frame */
#define EMURX_PINGTX_MAX_LEN 248u
int emurx_pingtx_reserve(emurx_t* h, uint32_t max_pings);
int emurx_pingtx_add(emurx_t* h, const uint8_t* tmpl, uint32_t len, uint32_t icmp_off,
                     uint32_t vport, uint32_t* id);
int emurx_pingtx_remove(emurx_t* h, uint32_t id);
/* The generator.  Request r stands for `count` frames: frame k is the template of `id` with
   seq + k (mod 2^16) and ts patched in and the checksum above.  The frames come out in request
   order, then in k, in the responder's layout, so that emurx_tx_zmq_dev takes them: frame j at
   d_out_desc[j].off, a multiple of 16 = the sum of align16(len) of the frames before it;
   d_out_desc[j] = {off, len, vport, 0}; the bytes between a frame's end and the next 16-byte
   boundary are unspecified; nothing is written at or past out_cap, nor at or past descriptor
   desc_cap.  A request whose id is free or >= max_pings gets EMURX_PTX_BAD_ID and no frames;
   count == 0 is EMURX_PTX_OK with no frames.  With too little room the whole requests that fit
   are written, a prefix in request order, and every later request with frames gets
   EMURX_PTX_NOSPC (so does one that would end past 4 GiB, the descriptor's offset range).
   d_info (u64[EMURX_PTX_INFO_WORDS]) = {frames written, bytes needed, frames needed, requests with
   outcome 0, 1, 2, 0, 0}; n_req == 0 writes a zero d_info.  d_outcome [n_req] may be NULL.
   d_out 16-byte aligned, d_req, d_out_desc and d_info 8-byte.  EMURX_EINVAL: a NULL d_info, with
   n_req > 0 a NULL d_req or d_out_desc, a NULL d_out with out_cap > 0, a misaligned array, a
   capturing stream, no reserve; EMURX_ENOMEM: n_req > cfg.max_frames; EMURX_EDEVICE: a host-only
   handle.  Three launches on `stream` (count, scan, emit: the emit deals 16-byte output chunks
   over its lanes, so one request of 60,000 frames is as parallel as 60,000 requests of one), no
   host synchronisation (but for the shipment's two cases above) and no allocation; the scratch is the handle's, handed from call to call
   by event, so calls on different streams are safe and run one after the other. */
typedef struct emurx_pingtx_req { uint32_t id; uint16_t seq; uint16_t count; uint64_t ts; } emurx_pingtx_req; /* 16 B */
enum emurx_ptx { EMURX_PTX_OK = 0, EMURX_PTX_BAD_ID = 1, EMURX_PTX_NOSPC = 2 };
#define EMURX_PTX_INFO_WORDS 8
int emurx_pingtx_dev(emurx_t* h, const emurx_pingtx_req* d_req, uint32_t n_req,
                     uint8_t* d_out, uint64_t out_cap, emurx_desc* d_out_desc, uint32_t desc_cap,
                     uint8_t* d_outcome /* [n_req], may be NULL */, uint64_t* d_info, void* stream);
/* On an egress slot.  emurx_egress_ping_buffer returns the slot's pinned request array
   (cfg.max_frames entries; behind emurx_egress_buffer on the slot and emurx_pingtx_reserve, else
   EMURX_EINVAL; the first call allocates it and its device copy).  emurx_egress_submit_ping is
   emurx_egress_submit with n_req requests behind the n plain frames: the batch comes out as if the
   caller had sent its n plain frames and then the requests' frames in request order, followed by
   one FlushTx.  The submit reads each request once on the host against the per-id lengths, so the
   sizes are exact: with G = the sum of count and B = the sum of count * align16(len), an id that is
   free or out of range is EMURX_EINVAL, n + G > cfg.max_frames EMURX_ENOMEM, align16(bytes) + B >
   cfg.max_bytes EMURX_ENOSPC; the other errors are emurx_egress_submit's; nothing is enqueued on
   an error.  It enqueues the copies (now with 16 * n_req bytes of requests), the plan and the
   checksum over the n plain frames only, the generator writing into the slot's device frame buffer
   at align16(bytes) with its descriptors appended at index n, the framing over n + G frames, and
   k_egr_out.  emurx_egress_wait is unchanged: n_frames = n + G, plan[i] / status[i] for i >= n are
   EMURX_TXP_NONE / EMURX_TX_OK, plan_info counts the plain frames only. */
int emurx_egress_ping_buffer(emurx_t* h, uint32_t slot, emurx_pingtx_req** req);
int emurx_egress_submit_ping(emurx_t* h, uint32_t slot, uint32_t n, uint64_t bytes, uint32_t flags, uint32_t n_req);

/* ---- the stateless answers on the device ------------------------------------------------
   Three of the plugins' answers are a pure function of the frame and of a table the device
   holds; emurx_respond_dev builds them from a classified batch, shaped for emurx_tx_zmq_dev:
     ARP reply to a request for a client's IPv4   plugins/arp/arp.go:904-933 -> Respond :776-790
     ICMPv4 echo reply                            plugins/icmp/icmp.go:396-461 -> HandleEcho :289-325
     ICMPv6 echo reply                            plugins/ipv6/ipv6.go:465-504 -> HandleEcho :315-357
   A frame is considered only if rec.status == EMURX_ST_OK, its lookup is EMURX_LK_CLIENT, its
   callback is arp / icmp / icmpv6 and its descriptor is no hole; every other frame gets
   EMURX_RSP_NONE.  d_rec: the records emurx_classify_dev wrote for d_frames / d_desc.
     arp     the template's reply (14 + 4 per VLAN tag + 28 bytes, no padding): dst = the request's
             sender hardware address, src = the client's MAC, one tag per non-zero rec.vlan[i]
             (the Namespace key's TPID | VID), 0x0806, 00 01 08 00 06 04 00 02, {client MAC, the
             request's target IP}, {the request's sender hardware address and IP}.  The MAC is
             the IPv4 table slot's: the table is probed again with the record's tunnel key and
             the target IP, and a probe that does not return rec.client_id (a partitioned handle
             that does not own the Namespace, tables changed since the classify) gives
             EMURX_RSP_HOST.
     icmp    source IP neither loopback nor net.IP.IsGlobalUnicast (Go 1.18: 0.0.0.0,
             255.255.255.255, 224.0.0.0/4, 169.254.0.0/16; Go's standard library, not the
             reference tree) -> DROP_MCAST; then type, code (8, 0) -> reply, (13, 0) -> HOST, else
             NONE; an Ethernet source with the group bit -> DROP_MCAST.  The reply is the whole
             frame (tags and trailing bytes kept) with the Ethernet and the IPv4 addresses
             swapped, type 0 and the checksum UpdateInetChecksum(cs, 0x0800, 0x0000).
     icmpv6  an Ethernet source with the group bit -> DROP_MCAST; else the addresses swapped,
             type 129, extension headers stripped (next header 58, payload length less
             l4 - l3 - 40, p[l4:] moved down to l3 + 40, the frame shorter by as much), checksum
             UpdateInetChecksum(cs, 0x8000, 0x8100).
   Header offsets of a record that do not fit its frame (emurx_classify_dev writes none) give HOST.
   Output: the replies compacted in rx frame order; reply k at d_out_desc[k].off, a multiple of
   16 = the sum of align16(len) of the replies before it; d_out_desc[k] = {off, len, vport =
   rec.vport, pad 0} (the array emurx_tx_zmq_dev takes); d_out_src[k] = the rx frame index.  The
   up to 15 bytes between a reply's end and the next 16-byte boundary are unspecified; nothing is
   written at or past out_cap, nor past the aligned end of the last reply; out_cap >=
   sum(align16(desc.len)) always suffices.  d_info (u64[8]) = {replies written, bytes needed,
   frames with outcome 1..6}.  With too small a buffer the replies that fit are written (a
   prefix), the others get EMURX_RSP_NOSPC (so does a reply that would end past 4 GiB, the
   descriptor's offset range) and d_info[1] tells the size needed.  d_out_desc and d_out_src
   have capacity n; d_outcome [n] may be NULL.  d_out and d_rec 16-byte aligned, the descriptor
   arrays 8-byte; frames are read as the aligned 16-byte blocks that hold them.  n <
   EMURX_TX_ZMQ_MAX_FRAMES; n == 0 writes a zero d_info.  Three launches on `stream` (decide,
   scan, emit), no host synchronisation, behind the table shipment emurx_classify_dev describes;
   calls on different streams of one handle share its scratch, so they must not overlap. */
enum emurx_rsp {            /* per-frame outcome, d_outcome[i] */
    EMURX_RSP_NONE = 0,       /* not a frame this call answers */
    EMURX_RSP_ARP = 1, EMURX_RSP_ICMP = 2, EMURX_RSP_ICMPV6 = 3,   /* reply written */
    EMURX_RSP_DROP_MCAST = 4, /* the handler counts pktRxErrMulticastB and sends nothing */
    EMURX_RSP_HOST = 5,       /* the Go handler must answer (a timestamp request without EMURX_RSPK_TS; client not in this handle's tables) */
    EMURX_RSP_NOSPC = 6,      /* a reply was due but did not fit out_cap */
    EMURX_RSP_ND = 7,         /* reply written (neighbour advertisement; emurx_respond_kinds_dev only) */
    EMURX_RSP_TS = 8,         /* timestamp reply written (emurx_respond_ts_dev with EMURX_RSPK_TS only) */
    EMURX_RSP_DROP_SHORT = 9  /* len - l4 < 20: the handler counts pktRxErrTooShort, sends nothing (EMURX_RSPK_TS only) */
};
int emurx_respond_dev(emurx_t* h, const uint8_t* d_frames, const emurx_desc* d_desc,
                      const emurx_rec* d_rec, uint32_t n,
                      uint8_t* d_out, uint64_t out_cap, emurx_desc* d_out_desc,
                      uint32_t* d_out_src, uint8_t* d_outcome, uint64_t* d_info, void* stream);
/* The same call with the answers chosen by `kinds`, and a fourth answer, ARP's IPv6 counterpart:
     neighbour advertisement (NA) to a neighbour solicitation (NS)
                                   plugins/ipv6/nd.go:1546-1685 -> NdClientCtx.Respond :1220-1253
   kinds == 0 or a bit above EMURX_RSPK_ALL is EMURX_EINVAL; a frame of a kind that was not
   selected gets EMURX_RSP_NONE.  d_info is u64[EMURX_RSP_INFO_WORDS] = {replies written, bytes
   needed, frames with outcome 1..7, zeros}.  Everything else is emurx_respond_dev's contract,
   which is this call with kinds = ARP | ICMP | ICMPV6 and the eight-word d_info.
     nd      considered only if rec.status == EMURX_ST_OK, the callback is icmpv6, the lookup is
             EMURX_LK_NS_LEVEL, the descriptor is no hole and p[l4], p[l4+1] == 135, 0.  The device
             writes a reply if and only if the Go handler would reach nd.Respond; where it cannot
             cheaply decide it gives HOST, and NONE / HOST leave the Go handler running as today.
             Header offsets that do not fit the frame (l3 < 14, l3 + 40 > l4, l4 + 4 > len; checked
             before the type byte is read) -> HOST.  len - (l4 + 4) < 20 -> NONE (nd.go:1550-1553).
             The options are p[l4+24 : len], the rest of the frame and not the IPv6 payload length
             (gopacket layers/icmp6msg.go:299-312, 497-529): none -> no source link-layer address
             (SLLA); 8 bytes -> the SLLA if {type 1, length 1}, else NONE (a wrong option, a zero
             length and a truncated option are all errors, nd.go:1555-1587); 1..7 bytes -> NONE;
             more than 8 -> HOST (a lane walks no option chain).  Then, each NONE (nd.go:1561-1609):
             hop limit p[l3+7] != 255; an all-zero SLLA; source unspecified with an SLLA; source
             unspecified and destination not multicast; target unspecified or multicast.  NdLearn
             (:1611-1620) stays on the host and does not change the answer.  The target must be
             net.IP.IsLinkLocalUnicast or IsGlobalUnicast (else NONE, :1622-1624).  An EUI-64
             target (t[11], t[12] == ff, fe; ExtractOnlyMac core/client_ctx.go:314-329): the MAC
             table is probed with the record's tunnel key and the extracted MAC (a zero MAC never
             matches); miss -> NONE; IsValidPrefix (core/client_ctx.go:279-295: t[0:8] is fe80::/64
             or the client's RA prefix of length 64) else NONE; a client without the ipv6 plugin ->
             NONE; else the reply carries that MAC (:1626-1652).  Any other target: not global ->
             NONE; CLookupByIPv6 in the IPv6 table, miss -> NONE, no ipv6 plugin -> NONE, else the
             reply carries the slot's client MAC (:1653-1678).  The net.IP predicates are Go
             1.18's on a 16-byte slice, IPv4-mapped readings included (::ffff:0.0.0.0 is
             unspecified, ::ffff:224.x multicast, ::ffff:169.254.x link-local): Go's standard
             library, not the reference tree, pinned by no capture.
             The reply (nd.go:835-865, 1220-1253) is 14 + 4 per non-zero rec.vlan[i] + 72 bytes:
             Ethernet source the client MAC, the tags as in the ARP reply, 86dd; 60 00 00 00 00 20
             3a ff; 88 00 cs cs fl 00 00 00, the target, 02 01, the client MAC.  Source specified:
             Ethernet destination the request's p[6:12], IPv6 source the target, IPv6 destination
             the request's source, fl = 0x60.  Source unspecified (duplicate address detection):
             Ethernet destination 33:33:00:00:00:01, IPv6 source the client's link-local address
             fe80::(mac[0]^2) mac[1] mac[2] ff fe mac[3..5], IPv6 destination ff02::1, fl = 0.  cs
             is the ICMPv6 checksum over the pseudo header (length 32, next header 58) and the 32
             bytes (FixIcmpL4Checksum, gopacket layers/ip6.go:54-56). */
#define EMURX_RSPK_ARP 1u
#define EMURX_RSPK_ICMP 2u
#define EMURX_RSPK_ICMPV6 4u
#define EMURX_RSPK_ND 8u            /* neighbour solicitation -> neighbour advertisement */
#define EMURX_RSPK_ALL 15u
#define EMURX_RSP_INFO_WORDS 16
int emurx_respond_kinds_dev(emurx_t* h, const uint8_t* d_frames, const emurx_desc* d_desc,
                            const emurx_rec* d_rec, uint32_t n, uint32_t kinds,
                            uint8_t* d_out, uint64_t out_cap, emurx_desc* d_out_desc,
                            uint32_t* d_out_src, uint8_t* d_outcome, uint64_t* d_info, void* stream);
/* The same call with a fifth answer, the one whose only outside input is the time of day:
     ICMPv4 timestamp reply to a timestamp request
                      plugins/icmp/icmp.go:396-462 -> PluginIcmpNs.HandleEcho(ps, true) :289-325
   kinds: EMURX_RSPK_* bits in 1..EMURX_RSPK_ALL_TS (0 or a bit above is EMURX_EINVAL).  With
   kinds <= EMURX_RSPK_ALL the call is emurx_respond_kinds_dev(kinds) byte for byte (the same
   kernels; ip_time_ms is not read).  ip_time_ms: what the reference's iptime() (icmp.go:281-287)
   returns, milliseconds since midnight UTC; it is written as given, any u32, no range check.  The
   handler reads the clock per frame; this call has one value per batch.  d_info
   is u64[EMURX_RSP_INFO_WORDS] = {replies written (timestamp replies included), bytes needed,
   frames with outcome 1..9, zeros}.  Everything else is emurx_respond_kinds_dev's contract:
   capacity, the NOSPC prefix rule, alignment, three launches, no host synchronisation, the
   handle's shared scratch.
     icmp    a candidate if kinds has EMURX_RSPK_ICMP or EMURX_RSPK_TS (status OK, lookup
             EMURX_LK_CLIENT, callback icmp, no hole: the client lookup and IsUnicastToMe of
             icmp.go:417-427 are the classifier's).  In this order: header offsets that do not fit
             (l3 < 14, l3 + 20 > len, l4 + 8 > len) -> HOST; the source-IP rule (:429-436) ->
             DROP_MCAST, for every type; type, code (8, 0) -> the echo rule above if kinds has
             EMURX_RSPK_ICMP, else NONE; (13, 0) without EMURX_RSPK_TS -> HOST; any other -> NONE.
     ts      (13, 0) with EMURX_RSPK_TS, HandleEcho(ps, true) in the handler's order: the Ethernet
             source p[6] has the group bit (the swapped destination is broadcast or multicast,
             :293-299) -> DROP_MCAST; len - l4 < 20 (:312-316, behind the multicast test) ->
             EMURX_RSP_DROP_SHORT; an odd l4 (no parse of ours produces one) -> HOST; else
             EMURX_RSP_TS.  The reply is the whole frame (tags and trailing bytes kept, :324) with
             the Ethernet addresses swapped (:293-294), the IPv4 addresses swapped (:301-302; the
             header checksum holds), p[l4], p[l4+1] = 14, 0 (:310-311), ip_time_ms big-endian in
             p[l4+12:l4+16] and again in p[l4+16:l4+20] (receive and transmit, :317-319; the
             originate timestamp p[l4+8:l4+12] stays) and the ICMP checksum recomputed (:320,
             UpdateChecksum, gopacket layers/icmp4.go:252-256: p[l4+2:l4+4] zeroed, then
             tcpipChecksum(p[l4:len], 0), layers/tcpip.go:76-94): the sum of the big-endian byte
             pairs, an odd last byte as its high byte, folded while above 0xffff, complemented.
             The span is the rest of the frame and not the IPv4 total length: Ethernet padding
             and trailers are summed; a folded sum of 0xffff stores 0x0000. */
#define EMURX_RSPK_TS 16u           /* ICMPv4 timestamp request -> timestamp reply */
#define EMURX_RSPK_ALL_TS 31u
int emurx_respond_ts_dev(emurx_t* h, const uint8_t* d_frames, const emurx_desc* d_desc,
                         const emurx_rec* d_rec, uint32_t n, uint32_t kinds, uint32_t ip_time_ms,
                         uint8_t* d_out, uint64_t out_cap, emurx_desc* d_out_desc,
                         uint32_t* d_out_src, uint8_t* d_outcome, uint64_t* d_info, void* stream);

/* ---- ARP and ND cache learning, folded per batch ------------------------------------------
   The ARP handler learns the sender of every request before it answers and of every unicast
   reply (plugins/arp/arp.go:904-946 -> PluginArpNs.ArpLearn :886-901); the ND handler learns a
   solicitation's source (plugins/ipv6/nd.go:1611-1620) and an advertisement's target
   (:1687-1776).  ArpFlowTable.ArpLearn (arp.go:435-451) and Ipv6NsCacheFlowTable.NdLearn
   (nd.go:608-624) are idempotent after their second application (they write the MAC, then
   MoveToComplete from Incomplete or Refresh and otherwise set touch = true), so a batch's learning
   folds exactly into one event per distinct (ns, kind, ip, mac) with a frame count: applying each
   event's learn call once, and once more if count > 1, in the order the events are written,
   leaves the Go tables as frame-by-frame handling would.  emurx_learn_dev writes those events.
   d_rec: the records emurx_classify_dev wrote for d_frames / d_desc.  A frame is considered only
   if rec.status == EMURX_ST_OK and its descriptor is no hole (else EMURX_LRN_NONE); header offsets
   that do not fit the frame (emurx_classify_dev writes none) give EMURX_LRN_HOST.
     arp     with kinds & EMURX_LRNK_ARP, callback arp and lookup >= EMURX_LK_NS_LEVEL: the Namespace
             exists and has the arp plugin (arp.go:956-969).  l3 < 14 or l3 + 28 > len -> HOST.
             Operation p[l3+6:l3+8] 1 -> ARP_REQ, whatever the target resolves to (ArpLearn runs
             before the client lookup, :915-918); 2 -> ARP_REPLY unless the Ethernet destination is
             ff:ff:ff:ff:ff:ff (:936-941), then NONE; any other -> NONE.  The key is {rec.ns_id,
             kind, p[l3+14:l3+18], p[l3+8:l3+14]} (:886-901); a sender IP of 0.0.0.0 is learned like
             any other (the Go code has no test for it).
     nd      with kinds & EMURX_LRNK_ND, callback icmpv6, lookup EMURX_LK_NS_LEVEL.  l3 < 14, l3 +
             40 > l4 or l4 + 4 > len -> HOST, before the type byte is read; code p[l4+1] != 0 or a
             type other than 135, 136 -> NONE.
             Type 135: the checks of nd.go:1550-1609 exactly as emurx_respond_kinds_dev runs them
             (above, up to "target unspecified or multicast"; the same device functions), its option
             reading included: more than 8 option bytes -> HOST.  Then :1611-1620: the source is
             net.IP.IsGlobalUnicast, an SLLA is present and the IPv6 table holds no client for the
             source in this Namespace -> ND_NS with the key {ns, kind, source, SLLA}; else NONE.
             Type 136 (:1687-1776): len - (l4 + 4) < 20 -> NONE.  The options p[l4+24:len]: none ->
             NONE; exactly {2, 1, mac} -> the target MAC; any other 8 bytes or 1..7 bytes -> NONE;
             more than 8 -> HOST.  Hop limit p[l3+7] != 255 -> NONE; override flag p[l4+4] & 0x20
             clear -> NONE; a target p[l4+8:l4+24] neither link-local nor global -> NONE.  An EUI-64
             target is learned unless the MAC table holds the extracted MAC with IsValidPrefix (the
             responder's question, without the plugin test); any other target unless the IPv6 table
             holds it (pktRxNeighborAdvWithOwnAddr).  The key is {ns, kind, target, target MAC}; a
             zero target MAC is learned (the Go code checks it only for solicitations).
             The net.IP predicates are those of the responder.
   An event is the fold of all frames with one key: count frames, first / last the lowest and
   highest rx frame index among them.  Events are written in ascending `last` (frame indices are
   distinct, so the output is fully determined).  d_info (u64[EMURX_LRN_INFO_WORDS]) = {events
   written, distinct keys, overflow (0 or 1), frames with outcome 1..5}.  Overflow is distinct
   keys > ev_cap and nothing else: then d_info[0] is 0 and nothing is written to d_ev, while
   d_outcome and d_info[1..7] stay valid (handle the batch's learning frames one by one, or call
   again with a larger ev_cap).  Nothing is ever written at or past d_ev[ev_cap].
   kinds == 0 or a bit above EMURX_LRNK_ALL, ev_cap == 0 or ev_cap > emurx_learn_max_events(h)
   are EMURX_EINVAL; n > cfg.max_frames is EMURX_ENOMEM.  emurx_learn_max_events(h) is half the
   slot count of the handle's set (a power of two >= 2 * max_frames, so a batch's keys always
   fit it and a probe always ends at a free slot).  d_rec 16-byte aligned, d_desc, d_ev and d_info
   8-byte; d_outcome [n] may be NULL.  n < EMURX_TX_ZMQ_MAX_FRAMES; n == 0 writes a zero d_info.
   Four launches on `stream` (decide + fold, mark, scan, emit), no host synchronisation and no
   allocation (the scratch is sized at emurx_open from max_frames), behind the table shipment
   emurx_classify_dev describes; calls on different streams of one handle share the scratch, so
   they must not overlap.  A frame the responder answered (outcome EMURX_RSP_ARP or EMURX_RSP_ND)
   whose learn outcome is not EMURX_LRN_HOST needs no Go handler when the batch did not overflow:
   INTEGRATION.md has the replay loop. */
typedef struct emurx_learn_ev {
    uint32_t ns_id;    /* rec.ns_id of the frames folded                                   */
    uint32_t count;    /* frames folded into this event (>= 1)                             */
    uint32_t first;    /* lowest rx frame index among them                                 */
    uint32_t last;     /* highest; events are written in ascending `last`                  */
    uint8_t  ip[16];   /* ARP: sender IPv4 in ip[0:4] (wire order), ip[4:16] zero; ND: IPv6 */
    uint8_t  mac[6];
    uint8_t  kind;     /* enum emurx_lrn 1..4                                              */
    uint8_t  pad;      /* 0                                                                */
} emurx_learn_ev;      /* 40 bytes */
enum emurx_lrn {            /* per-frame outcome, d_outcome[i]; 1..4 are also the event kinds */
    EMURX_LRN_NONE = 0,       /* nothing to learn from this frame */
    EMURX_LRN_ARP_REQ = 1, EMURX_LRN_ARP_REPLY = 2, EMURX_LRN_ND_NS = 3, EMURX_LRN_ND_NA = 4,
    EMURX_LRN_HOST = 5        /* the Go handler must decide (an option chain, offsets that do not fit) */
};
#define EMURX_LRNK_ARP 1u
#define EMURX_LRNK_ND  2u
#define EMURX_LRNK_ALL 3u
#define EMURX_LRN_INFO_WORDS 8
uint32_t emurx_learn_max_events(const emurx_t* h);
int emurx_learn_dev(emurx_t* h, const uint8_t* d_frames, const emurx_desc* d_desc,
                    const emurx_rec* d_rec, uint32_t n, uint32_t kinds,
                    emurx_learn_ev* d_ev, uint32_t ev_cap,
                    uint8_t* d_outcome, uint64_t* d_info, void* stream);

/* ---- the handlers' per-Namespace counters, folded per batch ---------------------------------
   The ARP, ICMPv4 and ICMPv6 / ND handlers count per Namespace (ArpNsStats plugins/arp/arp.go:797,
   IcmpNsStats plugins/icmp/icmp.go:255, the ipv6 and nd stats of PluginIpv6Ns).  For a frame the
   responder has answered and the learning fold has folded, the counters are all that is left of
   its handler.  emurx_nsstat_dev decides per frame whether the Go handler still has to run
   (d_done) and folds the counters of the frames whose handler does not into one event per
   Namespace.  d_rec: the records emurx_classify_dev wrote for d_frames / d_desc on this handle
   (records of emurx_lookup_dev from another GPU are out of scope: their frames are elsewhere).
   kinds: EMURX_RSPK_* bits.  d_rsp_outcome: the outcome array of an emurx_respond_kinds_dev call
   on the same batch and records with at least these kinds.  d_lrn_outcome: that of an
   emurx_learn_dev call with ARP and / or ND as selected here; read only when kinds has
   EMURX_RSPK_ARP or EMURX_RSPK_ND (else it may be NULL).  If that learn call overflowed, repeat it
   with a larger ev_cap before trusting d_done for frames with learn outcome 1..4.
   d_done[i] (may be NULL):
     0  the Go handler runs as today and counts itself; the frame contributes nothing here
     1  everything the handler would do besides the reply and the learning is in this call's
        counters: skip the handler (every such handler returns 0)
     2  the handler would only return PARSER_ERR: lookup EMURX_LK_NO_NS or EMURX_LK_NS_NO_PLUGIN
        (arp.go:958-965, icmp.go:486-493, ipv6.go:546-553); add d_info[4] to errParser and skip it
   A frame is a candidate if rec.status == EMURX_ST_OK, its descriptor is no hole and its callback
   is one `kinds` selects (arp: ARP; icmp: ICMP; icmpv6: ICMPV6 or ND); every other frame gets 0.
   A candidate with lookup NO_NS / NS_NO_PLUGIN gets 2, one with EMURX_LK_NONE 0.  Then, before any
   byte of the frame is read, the header offsets (the responder's and the learner's tests): arp
   l3 < 14 or l3 + 28 > len; icmp l3 < 14, l3 + 20 > len or l4 + 8 > len; icmpv6 l3 < 14, l3 + 40 >
   l4 or l4 + 4 > len: each gives 0.  So does a record whose ns_id is not below cfg.max_ns (and
   2^27).  Then (idx: enum emurx_nsc below; paths relative to src/emu/plugins):
     arp     learn outcome EMURX_LRN_HOST -> 0.  Operation p[l3+6:l3+8] (arp.go:914-945):
             1: pktRxArpQuery (:916); lookup NO_CLIENT: also pktRxArpQueryNotForUs (:932), done 1;
                CLIENT_NO_PLUGIN: done 1 (:926-927); CLIENT with responder outcome EMURX_RSP_ARP:
                also pktTxReply (Respond :778), done 1; CLIENT with any other responder outcome
                (HOST, NOSPC, NONE): done 0 and no counter at all; lookup NS_LEVEL (no classify
                gives it to a request): done 0.
             2: Ethernet destination ff:ff:ff:ff:ff:ff: pktRxErrNoBroadcast (:937), else
                pktRxArpReply (:940); done 1.    any other: pktRxErrWrongOp (:944), done 1.
     icmp    HandleRxIcmpPacket icmp.go:396-462; the classifier has done CLookupByIPv4(dst) and
             IsUnicastToMe (:417-427), NO_CLIENT where either fails.  NO_CLIENT:
             pktRxNoClientUnhandled (:419, :425), done 1.  CLIENT: responder outcome DROP_MCAST:
             pktRxErrMulticastB (:434, HandleEcho :296), done 1; EMURX_RSP_ICMP: pktRxIcmpQuery and
             pktTxIcmpResponse (:322-323; one word, EMURX_NSC_ICMP_ECHO), done 1; else type, code
             p[l4], p[l4+1] (gopacket layers/icmp4.go:20-43): (8,0) echo request (a reply that
             did not fit, a kind the responder did not build), (13,0) timestamp request, (0,0) echo
             reply, (3, 0..4) destination unreachable Net / Host / Protocol / Port /
             FragmentationNeeded (:438-456): done 0; every other type / code: pktRxErrUnhandled
             (:458), done 1.  Any other lookup: done 0.
     icmpv6  HandleRxIpv6Packet ipv6/ipv6.go:465-539; type, code p[l4], p[l4+1] (gopacket
             layers/icmp6.go:21-52).
             (128,0) echo request, with EMURX_RSPK_ICMPV6: NO_CLIENT with IPv6 source byte p[l3+8] ==
             0xff: done 0 (the classifier folds the source test of :499 into NO_CLIENT, so the
             record cannot tell pktRxErrMulticastB from pktRxNoClientUnhandled); NO_CLIENT otherwise:
             pktRxNoClientUnhandled (:488, :494), done 1; CLIENT: responder EMURX_RSP_ICMPV6:
             pktRxIcmpQuery and pktTxIcmpResponse (:354-355; one word), done 1; DROP_MCAST:
             pktRxErrMulticastB (:322), done 1; else done 0.
             Every other type needs lookup NS_LEVEL (else done 0).
             (135,0) neighbour solicitation, with EMURX_RSPK_ND: responder outcome EMURX_RSP_ND and
             learn outcome NONE or ND_NS: pktRxNeighborSolicitation (nd.go:1547) and, if the IPv6
             source is unspecified (the responder's predicate, IPv4-mapped reading included),
             pktTxNeighborDADError (:1240), else pktTxNeighborAdvUnicast (:1246); done 1.  Any other
             combination: done 0 (every unanswered solicitation has a rejection counter of its
             own, which stays with Go).
             (136,0) neighbour advertisement, with EMURX_RSPK_ND: learn outcome ND_NA:
             pktRxNeighborAdvertisement (:1688) and pktRxNeighborAdvLearn (:1758, :1768), done 1;
             else done 0.
             done 0: (130..132,0) and (143,0) MLD (:505-509), (133,0), (134,0), (137,0) router
             solicitation, router advertisement, redirect (:511-516), (129,0) echo reply (:517),
             (1, 0..6) destination unreachable (:522-528).
             Every other type / code the parser lets through, with EMURX_RSPK_ICMPV6:
             pktRxErrUnhandled (:535), done 1.
   Output: one event per Namespace that has a frame with done 1, in ascending ns_id (fully
   determined).  d_info (u64[EMURX_NSS_INFO_WORDS]) = {events written, distinct Namespaces,
   overflow (0 or 1), frames with done 1, frames with done 2, candidates left at done 0, 0, 0}.
   Overflow is distinct Namespaces > ev_cap and nothing else: then d_info[0] is 0 and nothing is
   written to d_ev, while d_done and the rest of d_info stay valid.  Nothing is ever written at or
   past d_ev[ev_cap].  kinds == 0 or a bit above EMURX_RSPK_ALL, ev_cap == 0 or ev_cap >
   emurx_nsstat_max_events(h) (= min(cfg.max_frames, cfg.max_ns)), a NULL d_ev or d_info, with
   n > 0 a NULL d_frames, d_desc, d_rec, d_rsp_outcome or (kinds with ARP or ND) d_lrn_outcome, and
   a capturing stream are EMURX_EINVAL; n > cfg.max_frames is EMURX_ENOMEM; a host-only handle
   EMURX_EDEVICE.  d_rec 16-byte aligned, d_desc, d_ev and d_info 8-byte.  n == 0 writes a zero
   d_info.  Three launches on `stream` (decide + fold, scan, emit), no host synchronisation and no
   allocation (the scratch is sized at emurx_open from max_frames and max_ns), behind the table
   shipment emurx_classify_dev describes; calls on different streams of one handle share the
   scratch, so they must not overlap.  INTEGRATION.md has the replay loop and the dispatch rule. */
enum emurx_nsc {                 /* index into emurx_nsstat_ev.cnt */
    EMURX_NSC_ARP_QUERY = 0,            /* ArpNsStats.pktRxArpQuery            */
    EMURX_NSC_ARP_QUERY_NOT_FOR_US = 1, /* pktRxArpQueryNotForUs               */
    EMURX_NSC_ARP_REPLY = 2,            /* pktRxArpReply                       */
    EMURX_NSC_ARP_ERR_NO_BROADCAST = 3, /* pktRxErrNoBroadcast                 */
    EMURX_NSC_ARP_ERR_WRONG_OP = 4,     /* pktRxErrWrongOp                     */
    EMURX_NSC_ARP_TX_REPLY = 5,         /* pktTxReply                          */
    EMURX_NSC_ICMP_ECHO = 6,            /* IcmpNsStats.pktRxIcmpQuery and pktTxIcmpResponse */
    EMURX_NSC_ICMP_NO_CLIENT = 7,       /* pktRxNoClientUnhandled              */
    EMURX_NSC_ICMP_ERR_MCAST = 8,       /* pktRxErrMulticastB                  */
    EMURX_NSC_ICMP_ERR_UNHANDLED = 9,   /* pktRxErrUnhandled                   */
    EMURX_NSC_V6_ECHO = 10,             /* ipv6 pktRxIcmpQuery and pktTxIcmpResponse */
    EMURX_NSC_V6_NO_CLIENT = 11,        /* ipv6 pktRxNoClientUnhandled         */
    EMURX_NSC_V6_ERR_MCAST = 12,        /* ipv6 pktRxErrMulticastB             */
    EMURX_NSC_V6_ERR_UNHANDLED = 13,    /* ipv6 pktRxErrUnhandled              */
    EMURX_NSC_ND_RX_NS = 14,            /* nd pktRxNeighborSolicitation        */
    EMURX_NSC_ND_TX_ADV_UNICAST = 15,   /* pktTxNeighborAdvUnicast             */
    EMURX_NSC_ND_TX_DAD_ERROR = 16,     /* pktTxNeighborDADError               */
    EMURX_NSC_ND_RX_NA = 17,            /* pktRxNeighborAdvertisement          */
    EMURX_NSC_ND_RX_NA_LEARN = 18,      /* pktRxNeighborAdvLearn               */
    /* 19, counted by emurx_nsstat_ts_dev alone: IcmpNsStats.pktRxErrTooShort; 20..21 zero */
    EMURX_NSC_ICMP_ERR_TOO_SHORT = EMURX_NSC_ND_RX_NA_LEARN + 1
};
#define EMURX_NSC_WORDS 22
#define EMURX_NSS_INFO_WORDS 8
typedef struct emurx_nsstat_ev {
    uint32_t ns_id;                  /* rec.ns_id of the frames folded                         */
    uint32_t frames;                 /* frames with done == 1 folded into this event (>= 1)    */
    uint32_t cnt[EMURX_NSC_WORDS];   /* enum emurx_nsc; unused words 0                         */
} emurx_nsstat_ev;                   /* 96 bytes */
uint32_t emurx_nsstat_max_events(const emurx_t* h);   /* min(cfg.max_frames, cfg.max_ns) */
int emurx_nsstat_dev(emurx_t* h, const uint8_t* d_frames, const emurx_desc* d_desc,
                     const emurx_rec* d_rec, uint32_t n, uint32_t kinds,
                     const uint8_t* d_rsp_outcome, const uint8_t* d_lrn_outcome,
                     emurx_nsstat_ev* d_ev, uint32_t ev_cap,
                     uint8_t* d_done, uint64_t* d_info, void* stream);
/* The same call for outcomes of emurx_respond_ts_dev.  kinds in 1..EMURX_RSPK_ALL_TS; EMURX_RSPK_TS
   without EMURX_RSPK_ICMP is EMURX_EINVAL (the timestamp rule refines the icmp handler's).  With
   kinds <= EMURX_RSPK_ALL it is emurx_nsstat_dev(kinds).  d_rsp_outcome: the outcome array of an
   emurx_respond_ts_dev call on the same batch and records with at least these kinds.  With
   EMURX_RSPK_TS, an icmp frame with lookup CLIENT and responder outcome
     EMURX_RSP_TS          counts pktRxIcmpQuery and pktTxIcmpResponse (icmp.go:322-323; the one
                           word EMURX_NSC_ICMP_ECHO), done 1;
     EMURX_RSP_DROP_SHORT  counts pktRxErrTooShort (icmp.go:313; EMURX_NSC_ICMP_ERR_TOO_SHORT, a
                           counter a frame bumps alone: it adds to the event's `frames`), done 1;
   a timestamp request with DROP_MCAST counts pktRxErrMulticastB like every DROP_MCAST, done 1;
   with HOST, NOSPC or NONE it stays at done 0.  Everything else is emurx_nsstat_dev's contract. */
int emurx_nsstat_ts_dev(emurx_t* h, const uint8_t* d_frames, const emurx_desc* d_desc,
                        const emurx_rec* d_rec, uint32_t n, uint32_t kinds,
                        const uint8_t* d_rsp_outcome, const uint8_t* d_lrn_outcome,
                        emurx_nsstat_ev* d_ev, uint32_t ev_cap,
                        uint8_t* d_done, uint64_t* d_info, void* stream);

/* ---- echo replies and destination-unreachable messages, folded per ping ------------------------
   The rx half of icmp_c_start_ping / ipv6_start_ping: an ICMPv4 echo reply (0,0) or destination
   unreachable (3,0..4) reaches PluginIcmpNs.HandleEchoReply / HandleDestinationUnreachable
   (plugins/icmp/icmp.go:328-393, from HandleRxIcmpPacket :396-462), an ICMPv6 echo reply (129,0) or
   destination unreachable (1,0..6) PluginIpv6Ns.HandleEchoReply / HandleDestinationUnreachable
   (plugins/ipv6/ipv6.go:359-462, from :517-532); both hand the frame to the client's Ping
   (icmp.go:180-203, ipv6.go:188-210; plugins/ping/ping.go:246-311).  emurx_nsstat_dev leaves these
   frames at done 0.  All a frame does there is bump counters and advance a small per-ping state,
   and only the in-order test and the minimum-latency rule depend on frame order, among the
   frames of one ping: emurx_ping_dev folds a batch's frames into one event per {ns_id, client_id,
   family, identifier}.  The identifier is the one on the wire: whether the client has a ping
   running and whether the identifier is its own is decided when Go replays the event, so no
   mid-batch change of the ping state can make the device's view stale.
   d_rec: the records emurx_classify_dev wrote for d_frames / d_desc on this handle.  fams:
   EMURX_PNGK_* bits.  now_unix_ns: the caller's time.Now().UnixNano(), one value per batch (the
   contract of emurx_respond_ts_dev's ip_time_ms), below 2^63; the reference's simulation uses
   128 + 1,000,000 (ping.go:263-265).
   A frame is a candidate if rec.status == EMURX_ST_OK, its descriptor is no hole and its callback
   is icmp with fams & EMURX_PNGK_V4 or icmpv6 with fams & EMURX_PNGK_V6; every other frame gets
   EMURX_PNG_NONE.  Before any byte of a candidate is read, the header offsets (emurx_nsstat_dev's
   tests): icmp l3 < 14, l3 + 20 > len or l4 + 8 > len; icmpv6 l3 < 14, l3 + 40 > l4 or l4 + 4 >
   len: each gives EMURX_PNG_HOST.  Then
     icmp    lookup other than CLIENT / CLIENT_NO_PLUGIN -> NONE (NO_CLIENT is emurx_nsstat_dev's
             pktRxNoClientUnhandled).  Type, code p[l4], p[l4+1] other than (0,0), (3,0..4) -> NONE.
             A source p[l3+12:l3+16] that is neither loopback nor global unicast -> MCAST
             (pktRxErrMulticastB, icmp.go:433-436; the responder's predicate).  l4 != l3 + 20 -> HOST:
             gopacket's IPv4.DecodeFromBytes over the 20-byte slice fails for IHL > 5 (layers/
             ip4.go:336-343, pktRxErrTooShort), which stays with Go.  CLIENT_NO_PLUGIN, or a client
             without the icmp plugin in the client info table (the classifier gives this callback
             CLIENT whatever the client's plugins are) -> NO_CLIENT (GetIcmpClientByMac
             icmp.go:349-351, :384-386: after IsUnicastToMe the client of the destination MAC is
             rec.client_id).  Echo reply: len - (l4 + 8) < 16 -> HOST (icmp.go:182-185),
             else REPLY with identifier p[l4+4:l4+6], sequence number p[l4+6:l4+8], magic
             p[l4+8:l4+16] and timestamp p[l4+16:l4+24], all big-endian.  Unreachable: len < l4 + 36
             -> HOST (icmp.go:378), else UNREACH with the nested identifier p[l4+32:l4+34].  The
             client is rec.client_id.
     icmpv6  type, code other than (129,0), (1,0..6), or a lookup other than NS_LEVEL -> NONE.  Echo
             reply: len - l4 < 24 -> HOST (ipv6.go:389); unreachable: len - l4 < 72 -> HOST (:445).
             The client is CLookupByMac(p[0:6]) in rec.ns_id (GetIcmpClientByMac ipv6.go:559-573),
             probed in the MAC table; none, or one without the ipv6 plugin -> NO_CLIENT
             (pktRxNoClientUnhandled :397-399, :453-455).  The reply's fields sit at the same offsets
             from l4 as in icmp; the unreachable's identifier is p[l4+52:l4+54].
   A REPLY (Ping.HandleEchoReply ping.go:246-295) whose magic is not 0xc15c0c15c0be5be5 (:198) is
   malformed; else, with ts the timestamp as int64, it is accepted iff now - 5e9 <= ts <= now
   (signed: Go's latency < 0 || latency > 5 s with Time.Sub saturating), with latency now - ts;
   otherwise it has a bad latency.
   An event folds all frames of one key {ns_id, client_id, family, ident}; MCAST and NO_CLIENT
   frames fold into the Namespace-level key {ns_id, 0xffffffff, family, 0}.  lat_min_tail is the
   minimum over the accepted replies behind the last accepted reply with latency 0 (over all of
   them if none has latency 0; 0 if that reply is the last one): what ping.go:290-293 leaves, where
   a zero minimum is replaced by the next latency.  Events are written in ascending `last`, so the
   output is fully determined.  d_info (u64[EMURX_PNG_INFO_WORDS]) = {events written, distinct
   keys, overflow (0 or 1), frames with outcome 1..5}; overflow is distinct keys > ev_cap and
   nothing else: then d_info[0] is 0 and nothing is written to d_ev, while d_outcome and
   d_info[1..7] stay valid.  Nothing is ever written at or past d_ev[ev_cap].  A frame with outcome
   1..4 needs no Go handler when the batch did not overflow: INTEGRATION.md has the replay loop.
   fams == 0 or a bit above EMURX_PNGK_ALL, now_unix_ns >= 2^63, ev_cap == 0 or ev_cap >
   emurx_ping_max_events(h), a NULL d_ev or d_info, with n > 0 a NULL d_frames, d_desc or d_rec,
   and a capturing stream are EMURX_EINVAL; n > cfg.max_frames is EMURX_ENOMEM; a host-only handle
   EMURX_EDEVICE.  d_rec 16-byte aligned, d_desc, d_ev and d_info 8-byte; d_outcome [n] may be
   NULL.  n < EMURX_TX_ZMQ_MAX_FRAMES; n == 0 writes a zero d_info.  Five launches on `stream`
   (decide, fold, mark, scan + the ordered pass, emit), no host synchronisation and no allocation
   (the scratch, its own, is sized at emurx_open from max_frames and every call leaves it as it
   found it), behind the table shipment emurx_classify_dev describes; calls on different streams
   of one handle share the scratch, so they must not overlap.  emurx_ping_max_events(h) is
   emurx_learn_max_events(h). */
typedef struct emurx_ping_ev {       /* 80 bytes */
    uint32_t ns_id, client_id;       /* client_id 0xffffffff: Namespace-level event */
    uint16_t ident; uint8_t family /* 4 | 6 */, flags /* bit 0: an accepted latency was 0 */;
    uint32_t first, last;            /* lowest / highest rx frame index folded */
    uint32_t n_reply, n_unreach;     /* REPLY / UNREACH frames */
    uint32_t n_malformed, n_bad_latency, n_ok;   /* partition of n_reply */
    uint32_t n_succ;                 /* accepted replies whose predecessor (previous accepted
                                        reply of this key in rx order) has seq - 1 mod 2^16 */
    uint16_t seq_first, seq_last;    /* seq of the first / last accepted reply */
    uint64_t lat_sum, lat_min_tail, lat_max;
    uint32_t n_no_client, n_mcast;   /* Namespace-level events only */
} emurx_ping_ev;
enum emurx_png {            /* per-frame outcome, d_outcome[i] */
    EMURX_PNG_NONE = 0,       /* not this call's frame */
    EMURX_PNG_REPLY = 1, EMURX_PNG_UNREACH = 2,
    EMURX_PNG_NO_CLIENT = 3,  /* pktRxNoClientUnhandled */
    EMURX_PNG_MCAST = 4,      /* pktRxErrMulticastB */
    EMURX_PNG_HOST = 5        /* the Go handler must decide */
};
#define EMURX_PNGK_V4 1u
#define EMURX_PNGK_V6 2u
#define EMURX_PNGK_ALL 3u
#define EMURX_PNG_INFO_WORDS 8
#define EMURX_PING_MAGIC 0xc15c0c15c0be5be5ull   /* ping.go:198 */
#define EMURX_PING_TIMEOUT_NS 5000000000ull      /* DefaultPingTimeout, ping.go:267 */
uint32_t emurx_ping_max_events(const emurx_t* h);
int emurx_ping_dev(emurx_t* h, const uint8_t* d_frames, const emurx_desc* d_desc,
                   const emurx_rec* d_rec, uint32_t n, uint32_t fams, uint64_t now_unix_ns,
                   emurx_ping_ev* d_ev, uint32_t ev_cap,
                   uint8_t* d_outcome, uint64_t* d_info, void* stream);

/* ---- TCP / UDP frames the transport plugin refuses, folded per client --------------------------
   A tcp / udp frame reaches HandleRxTransPacket (plugins/transport/plugin_transport.go:74-128),
   which finds the Namespace plugin, the client and its plugin, then the client's TransportCtx, whose
   handleRxPacket (client_ctx.go:912-969) probes the flow table and, on a miss, calls
   handleRxTcpNewFlow / handleRxUdpNewFlow (:829-906).  The classifier takes that decision on the
   device (emurx_dev_out.flow).  For a frame that reaches no socket all the handler does is bump two
   to four ftStats counters (client_ctx.go:158-197) or return PARSER_ERR: pure counts, so nothing
   depends on frame order and emurx_ftstat_dev folds them exactly, one event per client.
   d_frames, d_desc, d_rec, d_flow: as ONE emurx_classify_dev call on this handle wrote them
   (out.flow non-NULL); records and flow words of emurx_lookup_dev on another GPU are out of scope.
   A frame is a candidate if rec.status == EMURX_ST_OK, its descriptor is no hole and rec.proto is
   EMURX_CB_TCP or EMURX_CB_UDP; every other frame gets EMURX_FT_NONE.  For a candidate, by lookup:
     NO_NS, NS_NO_PLUGIN, NO_CLIENT, CLIENT_NO_PLUGIN -> EMURX_FT_ERR: the handler would only return
             PARSER_ERR (-1, plugin_transport.go:82-128), which HandleRxPacket counts as errParser
             (core/thread_ctx.go:365-372).
     LK_NONE, NS_LEVEL -> NONE.  CLIENT with rec.client_id >= cfg.max_clients or rec.ns_id >=
             cfg.max_ns -> NONE.
     CLIENT  by d_flow[i]:
             EMURX_FLOW_NO_CTX -> EMURX_FT_ERR (plugin_transport.go:75-78, returns -1).
             EMURX_FLOW_NO_SYN with the tcp callback -> EMURX_FT_NO_SYN: ft_lookupv4 | ft_lookupv6
             (client_ctx.go:927 / :951), ft_new_tcp (:837), ft_new_tcp_no_syn (:842); with the udp
             callback -> NONE (the classifier never produces that combination).
             EMURX_FLOW_NO_SERVER with the tcp callback -> EMURX_FT_NO_SRV_TCP: ft_lookup*,
             ft_new_tcp (:837), ft_new_no_cb (:851); with the udp callback -> EMURX_FT_NO_SRV_UDP:
             ft_lookup*, ft_new_udp (:878), ft_new_no_cb (:886).
             A flow id, EMURX_FLOW_NEW, EMURX_FLOW_UNKNOWN and EMURX_FLOW_NONE -> NONE: the handler
             runs and counts itself.
   handleRxPacket returns 0 on the three folded paths (it ignores the new-flow functions' return
   values, :936-942), so these frames add nothing to errParser.  The family is p[l3] >> 4 == 4, as
   :918-920 and get_tuple read it: the only byte of the frame the fold reads, and only for outcomes
   1..3; before that read l3 < 14 or l3 >= len gives NONE.  IPv6 sets EMURX_FT_V6 in the outcome
   byte, which therefore states exactly which counters a frame contributed: outcome & 7 = 1 -> LOOKUP,
   NEW_TCP, NEW_TCP_NO_SYN; 2 -> LOOKUP, NEW_TCP, NEW_NO_CB; 3 -> LOOKUP, NEW_UDP, NEW_NO_CB, where
   LOOKUP is EMURX_FTC_LOOKUP_V6 with EMURX_FT_V6 and EMURX_FTC_LOOKUP_V4 without.
   There is one event per client_id that has a frame with outcome 1..3 (ns_id: its last such
   frame's record's); first / last are the lowest / highest rx frame index folded, frames their
   number, cnt[EMURX_FTC_*] what to add to the client's ftStats (cnt[6] is zero).  Events are written
   in ascending `last`, so the output is fully determined.  EMURX_FT_ERR frames make no event.
   d_info (u64[EMURX_FT_INFO_WORDS]) = {events written, distinct clients, overflow (0 or 1), frames
   NO_SYN, NO_SRV_TCP, NO_SRV_UDP, ERR, candidates left at NONE}; overflow is distinct clients >
   ev_cap and nothing else: then d_info[0] is 0 and nothing is written to d_ev, while d_outcome and
   d_info[1..7] stay valid.  Nothing is ever written at or past d_ev[ev_cap].  INTEGRATION.md has
   the replay loop, the dispatch rule and the rule for frames emurx_recs_stale flags.
   ev_cap == 0 or ev_cap > emurx_ftstat_max_events(h), a NULL d_ev or d_info, with n > 0 a NULL
   d_frames, d_desc, d_rec or d_flow, and a capturing stream are EMURX_EINVAL; n > cfg.max_frames is
   EMURX_ENOMEM; a host-only handle EMURX_EDEVICE.  d_rec 16-byte aligned, d_desc, d_ev and d_info
   8-byte, d_flow 4-byte; d_outcome [n] may be NULL.  n < EMURX_TX_ZMQ_MAX_FRAMES; n == 0 writes a
   zero d_info.  Four launches on `stream` (decide + fold, mark, scan, emit), no host synchronisation
   and no allocation (the scratch, its own, is sized at emurx_open from max_frames and every call
   leaves it as it found it), behind the table shipment emurx_classify_dev describes; calls on
   different streams of one handle share the scratch, so they must not overlap.
   emurx_ftstat_max_events(h) is min(cfg.max_frames, cfg.max_clients). */
enum emurx_ft {             /* per-frame outcome, d_outcome[i] & 7 */
    EMURX_FT_NONE = 0,        /* the transport handler runs (or the frame is none of its) */
    EMURX_FT_NO_SYN = 1, EMURX_FT_NO_SRV_TCP = 2, EMURX_FT_NO_SRV_UDP = 3,
    EMURX_FT_ERR = 4          /* the handler would return PARSER_ERR: errParser += 1 */
};
#define EMURX_FT_V6 0x08u   /* with outcome 1..3: the frame is IPv6 */
enum emurx_ftc {            /* ftStats words of an event, client_ctx.go:158-197 */
    EMURX_FTC_LOOKUP_V4 = 0, EMURX_FTC_LOOKUP_V6, EMURX_FTC_NEW_TCP, EMURX_FTC_NEW_TCP_NO_SYN,
    EMURX_FTC_NEW_UDP, EMURX_FTC_NEW_NO_CB
};
#define EMURX_FTC_WORDS 7   /* word 6 is zero */
#define EMURX_FT_INFO_WORDS 8
typedef struct emurx_ft_ev {         /* 48 bytes */
    uint32_t ns_id, client_id;
    uint32_t first, last;            /* lowest / highest rx frame index folded */
    uint32_t frames;                 /* frames folded */
    uint32_t cnt[EMURX_FTC_WORDS];
} emurx_ft_ev;
uint32_t emurx_ftstat_max_events(const emurx_t* h);
int emurx_ftstat_dev(emurx_t* h, const uint8_t* d_frames, const emurx_desc* d_desc,
                     const emurx_rec* d_rec, const uint32_t* d_flow, uint32_t n,
                     emurx_ft_ev* d_ev, uint32_t ev_cap,
                     uint8_t* d_outcome, uint64_t* d_info, void* stream);

/* ---- the device answers on an ingest slot ---------------------------------------------------
   The batched ingest keeps a batch's frames, descriptors and records private to its slot, so a
   caller without device memory cannot hand them to the four calls above.  With answers on, a
   slot runs them itself: after k_rx and the queue pack, on the slot's stream,
     1. emurx_respond_kinds_dev(kinds) over the slot's frames, descriptors and records (holes are
        EMURX_DESC_HOLE descriptors, which every stage skips), with an out_cap no batch can exceed
        (below), so EMURX_RSP_NOSPC does not occur;
     2. emurx_tx_zmq_counted_dev over the replies, d_count = the responder's d_info;
     3. emurx_learn_dev with ARP and / or ND as `kinds` selects them (neither: no learn call, every
        learn outcome EMURX_LRN_NONE), ev_cap = emurx_learn_max_events(h): it cannot overflow;
     4. emurx_nsstat_dev(kinds) with ev_cap = emurx_nsstat_max_events(h);
   then one launch (k_ans_out) that reads the stages' counts on the device and writes what was
   produced, and no more, into pinned host memory; the three per-frame byte arrays ride the
   batch's one result copy.  No host synchronisation between submit and wait; a batch with no
   reply and no event moves a few hundred bytes more than one without answers.
   emurx_ingest_set_answers(h, slot, kinds) holds for the slot's later submits; kinds: EMURX_RSPK_*
   bits, 0 = off (the default).  A slot with a batch in flight, slot >= EMURX_INGEST_SLOTS or a
   bit above EMURX_RSPK_ALL are EMURX_EINVAL; a host-only handle EMURX_EDEVICE.  The first call
   with kinds != 0 allocates everything the chain needs for cfg.max_frames and cfg.max_bytes (it
   waits for the device once, and grows the handle's framing and responder scratch to
   max_frames), so that no submit allocates or synchronises for it.  The sizes follow from the
   stages' rules: an answered or learned frame is at least 42 bytes long, so a batch has at most
   max_bytes / 42 replies and learn events; align16(reply) <= len + 54, so the replies take at
   most max_bytes * 96 / 42 bytes and their messages 8 bytes per reply more.  With answers on,
   emurx_ingest_submit returns EMURX_ENOSPC for messages that end past cfg.max_bytes.
   A batch submitted with answers on always takes the copy + launches pipeline:
   res.one_launch is 0, because the one-launch path never brings the frames into device memory.
   emurx_ingest_wait is unchanged.  emurx_ingest_answers(h, slot, &out), after the
   emurx_ingest_wait of that batch, points `out` at library-owned memory, valid until the slot's
   next submit; frame indices (reply_src, the events' first / last, the per-frame arrays) are in
   res.rec's numbering, also when messages fell short of the frames they announced.  It returns
   EMURX_ENOENT when the slot's last batch ran without answers, EMURX_EINVAL before any wait or
   with a batch in flight.
   The four stages' scratch belongs to the handle: the answer stages of different slots run one
   after another (each waits for the previous one's event; parse and classify of different slots
   still overlap), and a caller's own emurx_respond_dev / emurx_respond_kinds_dev /
   emurx_learn_dev / emurx_nsstat_dev / emurx_tx_zmq_dev / emurx_tx_zmq_counted_dev calls must not
   overlap a slot's batch that has answers on.  INTEGRATION.md has the loop. */
typedef struct emurx_answers {
    const uint8_t* tx;            /* the replies as ZMQ messages, back to back (emurx_tx_zmq_dev's layout) */
    const uint64_t* tx_msg_off;   /* [n_tx_msgs + 1] message starts in tx, then tx_bytes */
    uint32_t n_tx_msgs, n_replies;
    uint64_t tx_bytes;
    const uint32_t* reply_src;    /* [n_replies] rx frame index of each reply, res.rec numbering */
    const uint8_t* rsp_outcome;   /* [n_frames] enum emurx_rsp */
    const uint8_t* lrn_outcome;   /* [n_frames] enum emurx_lrn (all 0 when kinds has neither ARP nor ND) */
    const uint8_t* done;          /* [n_frames] emurx_nsstat_dev's d_done */
    const emurx_learn_ev* learn_ev;  /* [n_learn] ascending `last` */
    uint32_t n_learn;
    const emurx_nsstat_ev* ns_ev;    /* [n_ns] ascending ns_id */
    uint32_t n_ns;
    uint64_t rsp_info[EMURX_RSP_INFO_WORDS], lrn_info[EMURX_LRN_INFO_WORDS], nss_info[EMURX_NSS_INFO_WORDS];
} emurx_answers;               /* 352 bytes */
int emurx_ingest_set_answers(emurx_t* h, uint32_t slot, uint32_t kinds);
int emurx_ingest_answers(emurx_t* h, uint32_t slot, emurx_answers* out);
/* The timestamp reply on a slot.  emurx_ingest_set_answers_ts is emurx_ingest_set_answers with
   kinds up to EMURX_RSPK_ALL_TS (EMURX_RSPK_TS without EMURX_RSPK_ICMP is EMURX_EINVAL); the slot's
   chain then runs emurx_respond_ts_dev and emurx_nsstat_ts_dev.  emurx_ingest_set_time stores the
   ip_time_ms the slot's next submits pass to the responder (each submit takes the value stored
   at that moment, so two slots in flight carry their own times): a host store, no device work,
   default 0; EMURX_EINVAL with a batch in flight on the slot or slot >= EMURX_INGEST_SLOTS.  The
   sizing of the answer buffers holds: a timestamp reply is as long as its request, which is at
   least 54 bytes (l4 + 20 <= len with l4 >= 34).  emurx_ingest_set_answers keeps rejecting 16. */
int emurx_ingest_set_answers_ts(emurx_t* h, uint32_t slot, uint32_t kinds);
int emurx_ingest_set_time(emurx_t* h, uint32_t slot, uint32_t ip_time_ms);
/* The ping fold on a slot.  emurx_ingest_set_ping(h, slot, fams) holds for the slot's later
   submits; fams: EMURX_PNGK_* bits, 0 = off (the default).  It needs answers on for the slot, with
   any kinds (else EMURX_EINVAL), and turning answers off turns it off.  The stage runs behind
   nsstat in the slot's chain: emurx_ping_dev(fams) over the slot's frames, descriptors and records
   with ev_cap = emurx_ping_max_events(h), so it cannot overflow, and the now_unix_ns that
   emurx_ingest_set_now stored when the batch was submitted (each submit takes the value stored at
   that moment, so two slots in flight carry their own; a host store, no device work, default 0;
   2^63 and above are EMURX_EINVAL).  Then a launch of its own reads the stage's counts on the
   device and writes the info words, the outcome array and the events produced, and no more, into
   pinned memory the slot owns.  The first call with fams != 0 allocates everything for
   cfg.max_frames and cfg.max_bytes (a folded frame is at least 42 bytes long, so a batch has at
   most max_bytes / 42 events): no submit allocates or synchronises for it.  A slot with a batch
   in flight, slot >= EMURX_INGEST_SLOTS or a bit above EMURX_PNGK_ALL are EMURX_EINVAL; a host-only
   handle EMURX_EDEVICE.  emurx_ingest_ping(h, slot, &out), after the emurx_ingest_wait of that
   batch, points `out` at library-owned memory, valid until the slot's next submit; outcome and the
   events' first / last are in res.rec's numbering, also when messages fell short.  It returns
   EMURX_ENOENT when the slot's last batch ran without ping, EMURX_EINVAL before any wait or with a
   batch in flight.  The stage's scratch is the handle's: like the other stages', a caller's own
   emurx_ping_dev must not overlap a slot's batch that has ping on.  emurx_answers, and everything
   emurx_ingest_answers returns, are the same with ping on or off. */
typedef struct emurx_ping_out {
    const emurx_ping_ev* ev;      /* [n_ev] ascending `last` */
    uint32_t n_ev;
    const uint8_t* outcome;       /* [n_frames] enum emurx_png */
    uint64_t info[EMURX_PNG_INFO_WORDS];
} emurx_ping_out;
int emurx_ingest_set_ping(emurx_t* h, uint32_t slot, uint32_t fams);
int emurx_ingest_set_now(emurx_t* h, uint32_t slot, uint64_t now_unix_ns);
int emurx_ingest_ping(emurx_t* h, uint32_t slot, emurx_ping_out* out);
/* The flow decisions on a slot.  emurx_ingest_set_flows(h, slot, on) holds for the slot's later
   submits; on: 0 = off (the default), anything else on.  The stage is independent of
   emurx_ingest_set_answers: either may be on without the other.  With flows on, the slot's k_rx
   writes the per-frame flow words (emurx_dev_out.flow); the batch always takes the copy + launches
   pipeline (res.one_launch is 0, as with answers); emurx_ingest_submit returns EMURX_ENOSPC for
   messages that end past cfg.max_bytes.  Behind the queue pack, and behind the answer stages and
   the ping stage where the slot has them on, emurx_ftstat_dev runs over the slot's frames,
   descriptors, records and flow words with an ev_cap no batch can exceed: a folded frame is at
   least 42 bytes long (l3 >= 14, an IPv4 header and 8 bytes of UDP, or more), so a batch has at
   most min(emurx_ftstat_max_events(h), max_bytes / 42 + 1) events.  The fold's scratch is the
   handle's: with or without answers the stage takes part in the hand-off of the handle's scratches
   from slot to slot (it waits for the previous slot's event and records its own behind the fold),
   and a caller's own emurx_ftstat_dev must not overlap a slot's batch that has flows on.  Then one
   launch reads the stage's counts on the device and writes the info words, the flow and outcome
   arrays and the events produced, and no more, into pinned memory the slot owns.  The first call
   with on != 0 allocates everything for cfg.max_frames and cfg.max_bytes: no submit allocates or
   synchronises for it.  A slot with a batch in flight or slot >= EMURX_INGEST_SLOTS are
   EMURX_EINVAL; a host-only handle EMURX_EDEVICE.  emurx_ingest_flows(h, slot, &out), after the
   emurx_ingest_wait of that batch, points `out` at library-owned memory, valid until the slot's
   next submit; flow, outcome and the events' first / last are in res.rec's numbering, also when
   messages fell short of the frames they announced.  It returns EMURX_ENOENT when the slot's last
   batch ran without flows, EMURX_EINVAL before any wait or with a batch in flight.
   emurx_ingest_result, emurx_answers and emurx_ping_out are the same with flows on or off (but
   res.one_launch). */
typedef struct emurx_flows_out {
    const uint32_t* flow;         /* [n_frames] EMURX_FLOW_* / flow id */
    const uint8_t* outcome;       /* [n_frames] enum emurx_ft | EMURX_FT_V6 */
    const emurx_ft_ev* ev;        /* [n_ev] ascending `last` */
    uint32_t n_ev;
    uint64_t info[EMURX_FT_INFO_WORDS];
} emurx_flows_out;
int emurx_ingest_set_flows(emurx_t* h, uint32_t slot, uint32_t on);
int emurx_ingest_flows(emurx_t* h, uint32_t slot, emurx_flows_out* out);

/* ParserStats delta from an outcome histogram (pure host arithmetic). */
void emurx_hist_to_counters(const uint64_t hist[2 * EMURX_HIST_BINS], emurx_counters* out);
/* Sum the EMURX_HIST_SHARDS copies of a device histogram (after a D2H copy). */
void emurx_hist_fold(const uint64_t* shards, uint64_t out[2 * EMURX_HIST_BINS]);

/* Kernel timing with HIP events recorded on the launch stream around every batch.
   emurx_set_timing(h, slots, stride): slots > 0 keeps the last `slots` timed batches (ring),
   0 disables; every `stride`-th batch is timed (0 or 1 = every batch), so that a timed run
   can keep most launches free of event markers.
   emurx_kernel_times(): waits for the most recent timed batch and returns the device time in
   ms of every batch timed since the previous call (oldest first, at most min(cap, slots));
   then resets the ring. */
int emurx_set_timing(emurx_t* h, uint32_t slots, uint32_t stride);
int emurx_kernel_times(emurx_t* h, float* batch_ms, uint32_t cap, uint32_t* n_out);

/* The source tree this library was built from: the first 16 hex digits of the sha1 of its
   sources, headers and Makefile (trex-emu_amd/Makefile SRC_ID).  No ABI replacement: build
   provenance, printed by the Python binding when it loads the library. */
const char* emurx_build_id(void);

/* LDS staging slab (bytes per wave) of the most recent k_rx launch: 7168, 6144 or 5120 (0
   before the first).  Chosen per launch from sampled feedback of earlier launches (a wave whose
   frames span 6-7 KiB fits only the widest slab; 5120 once two samples in a row saw at most
   1 % of the waves over 5 KiB); EMURX_STAGE=wide|narrow|tight in the environment at emurx_open
   forces one.  Results never depend on it.  No ABI replacement: a tuning
   observable of this implementation. */
uint32_t emurx_last_stage(const emurx_t* h);
/* Which of the sampled waves of the most recent k_rx launch took the uniform-wave path: a staged
   wave whose 64 frames share one plain shape (the same number of 802.1Q tags, IPv4 without
   options or fragments, all UDP or all TCP, each exactly as long as its total length says) is
   parsed by straight-line code, and in a classifying launch its lookups are too when every
   frame reached the plain udp / tcp callback and hit the first slot of its home buckets.  Any
   other wave runs the general code; results never depend on the path.  The waves of every 64th
   tile are sampled: words[(tile / 64 % 64) * 4 + wave] is EMURX_UNI_SAMPLED, or-ed with
   EMURX_UNI_PARSE and EMURX_UNI_LOOKUP for the parts that took the path; 0 for a wave the
   launch did not sample.  Waits for the device.  EMURX_UNIFORM=0 in the environment at emurx_open
   switches the path off (default on).  A tuning observable, no ABI replacement. */
#define EMURX_UNI_WORDS 256
#define EMURX_UNI_PARSE 1u
#define EMURX_UNI_LOOKUP 2u
#define EMURX_UNI_SAMPLED 4u
int emurx_last_uniform(emurx_t* h, uint32_t words[EMURX_UNI_WORDS]);
/* One more fact about the same sampled waves, in the same layout: words[...] is
   EMURX_UNI_SAMPLED, or-ed with EMURX_TRIM_RANGE when the wave read its byte range off its end
   lanes (no empty slot, offsets and ends that never fall from one lane to the next) instead of
   reducing over the lanes.  Results never depend on it.  Waits for the device.  A tuning
   observable, no ABI replacement. */
#define EMURX_TRIM_RANGE 1u
int emurx_last_trim(emurx_t* h, uint32_t words[EMURX_UNI_WORDS]);
/* LDS image (bytes per wave) of the most recent tx framing write (emurx_tx_zmq_dev): 6144,
   4608 or 0 (every tile on the rows-over-lanes path); -1 before the first.  Chosen per call from
   the tile sizes an earlier call's chain kernel saw; EMURX_TXZ=wide|narrow|long at emurx_open
   forces one.  Results never depend on it.  A tuning observable, no ABI replacement. */
int32_t emurx_last_txz(const emurx_t* h);

/* HBM copy ceiling of this GPU for the roofline context (bench.py): a streaming 16-byte copy
   of `bytes` (a multiple of 16, 16-byte aligned device pointers) on `stream`, one launch.
   Not part of the receive path. */
int emurx_copy_ceiling_dev(void* d_dst, const void* d_src, size_t bytes, void* stream);

/* ---- Namespace-partitioned exchange (multi-GPU, one process per GPU) -------------------
   Frames shard by input offset across the GPUs of a node; each Namespace is owned by one
   partition, emurx_ns_owner(key) = a hash of its CTunnelKey (thread_ctx.go:92-97) mapped
   onto [0, n_parts).  After a batch is classified, emurx_route_dev packs every record whose
   Namespace was found (ns_id != EMURX_ID_NONE) into the send region of its owner:
       send[d * cap .. d * cap + send_count[d])   in frame order, as emurx_route_rec
   An equal-split all-to-all (RCCL over xGMI; n_parts regions of `cap` records) then delivers
   each record to the GPU that owns its Namespace, with send_count exchanged alongside so the
   receiver knows how many of each region are valid.  send_count[d] > cap means the region
   overflowed (records past cap were not written): the caller must raise cap and resend.
   Records without a Namespace stay with the receiving GPU (they are in its counters). */
#define EMURX_MAX_PARTS 8
typedef struct emurx_route_rec {
    emurx_rec rec;       /* the classified record                                        */
    uint32_t src_index;  /* frame index in the source GPU's batch                        */
    uint32_t src_rank;   /* source partition                                             */
} emurx_route_rec;       /* 40 bytes */

uint32_t emurx_ns_owner(const uint8_t key[12], uint32_t n_parts);
/* the descriptor owner key of a CTunnelKey (EMURX_DESC_KEYED | k); emurx_ns_owner(key, n) =
   ((k & 0x7f) * n) >> 7 for every n_parts <= EMURX_MAX_PARTS */
uint8_t emurx_owner_key(const uint8_t key[12]);
/* Write the owner key (EMURX_DESC_KEYED) of every frame into d_desc[i].pad, in place (holes
   stay holes): what the device framing walk does, for descriptors built without it.  Reads
   8 bytes of every frame.  One launch, no host synchronisation. */
int emurx_desc_keys_dev(emurx_t* h, const uint8_t* d_frames, emurx_desc* d_desc, uint32_t n, void* stream);
/* d_rec: the batch's records (device), n frames; d_send: [n_parts * cap] (device);
   d_send_count: [n_parts] (device).  Three kernel launches on `stream`, no host sync. */
int emurx_route_dev(emurx_t* h, const emurx_rec* d_rec, uint32_t n, uint32_t n_parts, uint32_t my_rank,
                    uint32_t cap, emurx_route_rec* d_send, uint32_t* d_send_count, void* stream);
/* Classify + route in one call: emurx_classify_dev of the batch (out->rec required) with the
   route's per-owner counts taken inside the k_rx launch, then the group scan and the packing
   of emurx_route_dev into d_send / d_send_count.  Equal to the two calls in sequence.  The
   route scratch is one set per stream (4 sets; a further stream takes a set over behind an
   event), so routes of batches pipelined over several streams run side by side. */
int emurx_classify_route_dev(emurx_t* h, const uint8_t* d_frames, const emurx_desc* d_desc, uint32_t n,
                             const emurx_dev_out* out, uint32_t n_parts, uint32_t my_rank, uint32_t cap,
                             emurx_route_rec* d_send, uint32_t* d_send_count, void* stream);

/* ---- owner-partitioned classification ---------------------------------
   With partitioned tables (emurx_set_partition) the lookups run on the GPU that owns the
   frame's Namespace.  The receiving GPU parses its shard and derives each frame's lookup key
   (emurx_parse_route_dev); every frame travels to the owner of its CTunnelKey as a 32-byte
   emurx_lookup_rec head, plus a tail of 16-byte units for the few classes whose key does not
   fit the head (an equal-split all-to-all of one region per owner, as for emurx_route_rec);
   the owner resolves Namespace, Client and flow against its partition for the frames that
   reached a callback (emurx_lookup_dev) and keeps the records of the others as parsed.  The
   owner's output for a frame equals emurx_classify_dev's record for it on replicated tables,
   bit for bit (the MapNsT / MapClient* maps thread_ctx.go:139, ns_ctx.go:110-112 split by
   owner).

   Region of one owner (EMURX_LOOKUP_REGION_BYTES(cap, tail_cap) bytes, 16-byte aligned):
     [0, 32 cap)                        heads, frame order: head j of the `count` valid ones
     [32 cap, + 16 EMURX_TAIL_SHARDS tail_cap)   tails: EMURX_TAIL_SHARDS shards of tail_cap
                                        16-byte units; a head's `x` names its tail's first unit
   Tails (the head's key kind / tuple bit say which):
     ICMPv6 echo, CLookupByIPv6 / LocalGlobal key (ns_ctx.go:288-329): 1 unit, the IPv6
       destination; the head carries the client-table hash of the key in place of L7 / L7Len
       (both 0 for ICMPv6, parser.go:684-717), so the owner issues the client probe without
       waiting for the tail
     tcp / udp while some client has a TransportCtx (client_ctx.go:46,78, the c5tuplekey):
       1 unit over IPv4 {ports, src, dst, 0}, 3 over IPv6 {ports, src[4], dst[4], 0, 0, 0}
   Every other frame is its head alone: config D's traffic averages 32.8 bytes per frame
   against the 64 of ABI version 4.  Tail units are taken per (wave, owner) by atomics on one
   of EMURX_TAIL_SHARDS cursors (spread so that no address serialises), so the ORDER of the
   tail units in a shard is not deterministic; what each head's tail holds is. */
#define EMURX_TAIL_SHARDS 64u
#define EMURX_TAIL_CURSOR_STRIDE 64u  /* words between two tail cursors: one per 256-byte line */
#define EMURX_LOOKUP_REGION_BYTES(cap, tail_cap) \
    ((uint64_t)(cap) * 32u + (uint64_t)EMURX_TAIL_SHARDS * (uint64_t)(tail_cap) * 16u)
#define EMURX_TAIL_NONE 0xFFFFFFFFu   /* head.x of a record whose tail did not fit its shard */
typedef struct emurx_lookup_rec {
    uint32_t frame;    /* source frame index (the source rank is the region it arrives in)  */
    uint32_t w[6];     /* the parse packed: CTunnelKey VLAN words (14-bit codes), vport, l3,
                          next header, l4, l7, l7_len, proto, status, RTALERT; the key kind,
                          the tuple bit; the destination MAC and TCP flags (emurx_parse.h)  */
    uint32_t x;        /* MAC key bytes 0..3 / IPv4 key, or the first tail unit's index     */
} emurx_lookup_rec;    /* 32 bytes */
/* Parse the batch (records without lookups into out->rec when non-NULL, queues, histogram as
   emurx_parse_dev) and pack the lookup record of every frame (holes excepted) into the region
   of its Namespace's owner: region d of d_send (EMURX_LOOKUP_REGION_BYTES(cap, tail_cap)
   bytes each) gets d_send_count[2 d] heads in frame order.  Three launches: the owner counts
   (from the descriptors' owner keys, EMURX_DESC_KEYED; a frame without one has its L2 header
   read, 8 bytes), their group scan (which also clears the tail cursors), and k_rx writing
   each head at its final place and each tail at the units its wave took.  Reads no table.
   d_send_count: [2 n_parts]; d_send_count[2 d] is the true head count (> cap: heads past cap
   were dropped); d_send_count[2 d + 1] is 0, or, when a tail did not fit its shard, the units
   the fullest shard of region d needed (> tail_cap; that head's x is EMURX_TAIL_NONE).  The
   caller must check both of every batch (after the count exchange, on every rank) and, on
   overflow, grow cap / tail_cap and route the batch again; the library raises no error of its
   own on the device path. */
int emurx_parse_route_dev(emurx_t* h, const uint8_t* d_frames, const emurx_desc* d_desc, uint32_t n,
                          const emurx_dev_out* out, uint32_t n_parts, uint32_t my_rank, uint32_t cap,
                          uint32_t tail_cap, emurx_lookup_rec* d_send, uint32_t* d_send_count, void* stream);
/* The owner's half: d_recv holds n_parts regions (EMURX_LOOKUP_REGION_BYTES(cap, tail_cap)
   bytes each, the all-to-all's receive buffer), d_recv_count[2 s] heads of them valid in region
   s.  Writes d_out[s * cap + j] (the classified record + source index / rank, emurx_route_rec)
   and d_flow (optional, the transport flow decision) for every valid slot.  One launch, no
   host synchronisation.  Counts must not exceed the capacities (the counts the sources
   reported; an overflow is for the sources to resolve first, emurx_parse_route_dev): slots past
   cap are not read, and a tail index past the shards is not read either. */
int emurx_lookup_dev(emurx_t* h, const emurx_lookup_rec* d_recv, const uint32_t* d_recv_count,
                     uint32_t n_parts, uint32_t cap, uint32_t tail_cap, emurx_route_rec* d_out,
                     uint32_t* d_flow, void* stream);

/* ---- the exchange behind the C-ABI: a library-owned communicator (RCCL over xGMI) -------
   The reference is one process whose main goroutine owns every table (MapNsT / GetNs
   thread_ctx.go:139,772-784, MainLoop :397-419).  Sharded over the GPUs of a node, the one new
   step is the exchange of every frame's lookup record to its Namespace owner; these calls run
   it from the caller's thread (cgo) with no Python or torch in between:
     one process per GPU:  rank 0 calls emurx_comm_unique_id and hands the 128 bytes to every
                           rank out of band; each rank calls emurx_comm_init(h, id, nranks, rank)
                           on its handle (ncclCommInitRank: blocks until every rank has joined)
     one process, N GPUs:  emurx_comm_init_all(handles, n) (ncclCommInitAll over the handles'
                           devices, one per GPU), the reference's process model; the exchanges of
                           the N handles are then issued between emurx_group_start and
                           emurx_group_end (whole-region mode only)
   The communicator's nranks is the n_parts of the exchange; handle k of emurx_comm_init_all is
   rank k.  emurx_close destroys it. */
#define EMURX_ECOMM (-71)          /* RCCL error (init, send / receive, group) */
#define EMURX_COMM_ID_BYTES 128    /* ncclUniqueId */
int emurx_comm_unique_id(uint8_t id[EMURX_COMM_ID_BYTES]);
int emurx_comm_init(emurx_t* h, const uint8_t id[EMURX_COMM_ID_BYTES], uint32_t nranks, uint32_t rank);
int emurx_comm_init_all(emurx_t* const* hs, uint32_t n);
int emurx_comm_destroy(emurx_t* h);
/* EMURX_ENOENT when the handle has no communicator */
int emurx_comm_info(emurx_t* h, uint32_t* nranks, uint32_t* rank);
/* The RCCL library the communicators use, bound at the first communicator call (dlopen of
   librccl.so.1: the copy already in the process if any, else the system's); its path into
   `path`.  EMURX_ECOMM when none loads. */
int emurx_comm_library(char* path, size_t cap);
/* A group is per OS thread (RCCL's ncclGroupStart / ncclGroupEnd are): emurx_group_start, the
   group's exchanges and emurx_group_end must run on one thread (from Go: between
   runtime.LockOSThread and runtime.UnlockOSThread).  emurx_group_end returns EMURX_EINVAL on a
   thread with no open group. */
int emurx_group_start(void);
int emurx_group_end(void);
/* One exchange of the regions emurx_parse_route_dev packed (lookup regions of
   EMURX_LOOKUP_REGION_BYTES(cap, tail_cap) bytes, two counts each) or, with EMURX_XCH_ROUTE,
   those emurx_classify_route_dev packed (cap emurx_route_rec, one count each): rank r receives
   region r of every source s into region s of d_recv, and its counts into d_recv_count, the
   layout emurx_lookup_dev reads.  Enqueued on `stream` (NULL = the handle's stream):
     EMURX_XCH_EQUAL    whole regions and counts in one group (ncclSend / ncclRecv to every
                        peer, the own region by a device copy); no host synchronisation
     EMURX_XCH_PAYLOAD  the counts first, then the host waits for them (the stream up to the
                        batch's packing) and only the spans that carry data travel: the first
                        min(count, cap) records and the tail shards (not inside a group)
   *bytes_moved (optional): bytes sent to other ranks by this call.  A count > cap (the sources'
   overflow, emurx_parse_route_dev) is delivered as is, so every rank sees it. */
#define EMURX_XCH_EQUAL 0u
#define EMURX_XCH_PAYLOAD 1u
#define EMURX_XCH_ROUTE 2u
int emurx_exchange_dev(emurx_t* h, const void* d_send, const uint32_t* d_send_count, void* d_recv,
                       uint32_t* d_recv_count, uint32_t cap, uint32_t tail_cap, uint32_t flags,
                       uint64_t* bytes_moved, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EMU_RX_H */

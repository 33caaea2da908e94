/*
 * vpcsum.h -- C-ABI of libvpcsum.so, the MI355X (gfx950) batched Internet
 * checksum engine for vproxy's vswitch.
 *
 * The library replaces the per-packet Java checksum path
 *   io.vproxy.base.util.Utils.calculateChecksum / calculateChecksumIntermediate /
 *   calculateChecksumDoFinal          (base/src/main/java/io/vproxy/base/util/Utils.java:778-801)
 *   Utils.buildPseudoIPv4Header / buildPseudoIPv6Header          (Utils.java:758-776)
 *   Ipv4Packet.__updateChecksum                                   (vpacket/Ipv4Packet.java:209-217)
 *   TcpPacket.updateChecksumWithIPv4 / IPv6                       (vpacket/TcpPacket.java:475-485, 508-518)
 *   UdpPacket.updateChecksumWithIPv4 / IPv6                       (vpacket/UdpPacket.java:136-164)
 *   IcmpPacket.__updateChecksum / updateChecksumWithIPv6          (vpacket/IcmpPacket.java:64-74, 124-135)
 * with ONE batched GPU launch per flush point (Iface.completeTx, Switch.java:1076-1078), in the
 * same flag-and-flush shape the XDP path already uses for its native checksum
 * (SwitchUtils.checksumFlagsFor, core/.../vswitch/util/SwitchUtils.java:297-316;
 *  XDPIface.sendPacket / completeTx, core/.../vswitch/iface/XDPIface.java:100-178, 227-243).
 *
 * Two entry-point families:
 *   1. vpcsum_*                      plain C, return 0 on success, <0 on error
 *                                    (message via vpcsum_last_error()).
 *   2. Java_io_vproxy_vpcsum_VPCsum_* PNI convention (base/src/main/c-generated/pni.h:15-82):
 *                                    int f(PNIEnv_<ret>* env, args...), 0 = ok, -1 = exception
 *                                    stored in env->ex, result in env->return_.
 *
 * No torch types, no CUDA types: plain pointers and sizes.  Device pointers are
 * hipMalloc'd (or torch) device memory; `stream` is a hipStream_t passed as void*.
 */
#ifndef VPCSUM_H
#define VPCSUM_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2 (round 4): VPCSUM_NAT_DEC_TTL refuses a TTL / hop limit <= 1 (S_BAD_DESC | S_TTL_EXPIRED)
 * instead of writing 0; vpcsum_synth_async takes a NULL arena (descriptors only).
 * 3 (round 5): VPCSUM_F_PRE and the pre-image entry points (vpcsum_pre_async,
 * vpcsum_ctx_submit_pre, vpcsum_group_submit_pre, vpcsum_batch_submit_pre, VPCsum.submitPre);
 * vpcsum_compute_async leaves F_PRE descriptors to vpcsum_pre_async; a handle of the process-wide
 * group from before a vpcsum_shutdown is refused.
 * 4 (round 6): the ingress header sum (vpcsum_hsum_t, VPCSUM_PRE_HSUM entries;
 * vpcsum_ctx_verify_frames_hsum, vpcsum_parse_ether_hsum_async, VPCsum.verifyFramesHsum): the
 * egress pre-image flush no longer depends on which setters ran; vpcsum_ctx_submit stages memory
 * the context has not registered instead of copying from it directly.
 * Additive since (the version stays 4): VPCSUM_NAT_TCP entries under the nat_mode bit
 * VPCSUM_NAT_TCP_REWRITES; a library from before answers that bit with "bad nat_mode", which is
 * how a caller probes for it; the flow table and its Fastpath; the TCP segment build
 * (vpcsum_tcp_build_async, vpcsum_ctx_build_tcp_frames, VPCsum.buildTcpFrames) and the TCP receive
 * (vpcsum_tcp_recv_async, vpcsum_tcp_digest_async, vpcsum_ctx_recv_tcp_frames, VPCsum.recvTcpFrames);
 * the TCP send bursts (vpcsum_tcp_build_bursts_async, vpcsum_ctx_build_tcp_bursts,
 * VPCsum.buildTcpBursts); the UDP datagram build and receive (vpcsum_udp_build_async,
 * vpcsum_udp_recv_async, vpcsum_ctx_build_udp_frames, vpcsum_ctx_recv_udp_frames,
 * VPCsum.buildUdpFrames, VPCsum.recvUdpFrames); the ICMP replies (vpcsum_icmp_reply_async,
 * vpcsum_ctx_reply_icmp_frames, VPCsum.replyIcmpFrames): new symbols, which a caller probes for by
 * looking them up. */
#define VPCSUM_ABI_VERSION 4

/* ------------------------------------------------------------------------ */
/* Data formats                                                             */
/* ------------------------------------------------------------------------ */

/* Per-packet descriptor flags (which sums are dirty).
 * F_IP / F_L4 are the batched form of AbstractPacket.isRequireUpdatingChecksum()
 * on the IP packet and on its upper-layer packet (AbstractPacket.java:38-65,
 * Ipv4Packet.java:219-234, Ipv6Packet.java:219-236), i.e. XDP's VP_CSUM_IP / VP_CSUM_UP. */
#define VPCSUM_F_IP    0x01u /* IPv4 header checksum (field L3+10)                        */
#define VPCSUM_F_L4    0x02u /* TCP(+16) / UDP(+6) / ICMP(+2) / ICMPv6(+2) checksum        */
#define VPCSUM_F_L4P   0x08u /* checksum offload (VP_CSUM_UP_PSEUDO, SwitchUtils.java:297-316): the L4
                              * field gets the folded, uncomplemented pseudo-header sum, the value
                              * Linux stores for CHECKSUM_PARTIAL (the reference's pcap fixtures
                              * hold 12 such TCP frames); the device adds the segment sum.  Not
                              * with VPCSUM_F_L4; TCP / UDP / ICMPv6 only (ICMPv4 has no pseudo
                              * header).  VERIFY compares the stored field with that value.    */
#define VPCSUM_F_RAW   0x04u /* Utils.calculateChecksum(buf, len) over [l3_off, l3_off+l3_len);
                                result in out bits 0..15; nothing else is interpreted       */
#define VPCSUM_F_PRE   0x10u /* with VPCSUM_F_L4 and / or F_IP: the packet was NAT'd by Java's
                              * setters after its stored L4 sum was verified on ingress
                              * (VPCSUM_S_L4_OK); its L4 sum is updated by RFC 1624 from the
                              * packet's pre-image (vpcsum_pre_t: the words the setters
                              * overwrote, or with VPCSUM_PRE_HSUM the ingress header sum
                              * recorded on receipt) instead of summed over the segment, its IPv4 header
                              * sum recomputed.  Only the header is read.  Handled by
                              * vpcsum_pre_async / vpcsum_ctx_submit_pre; vpcsum_compute_async
                              * reads nothing of such a packet, writes nothing into its frame and
                              * reports out 0 / S_DONE for it.                                 */

typedef struct vpcsum_desc {
    uint64_t l3_off;   /* byte offset of the L3 (IP) header inside the arena               */
    uint16_t l3_len;   /* IPv4 totalLength / IPv6 40+payloadLength (L2 padding excluded,
                          Ipv4Packet.java:100-103, Ipv6Packet.java:103-106)                  */
    uint16_t l4_off;   /* L4 header offset relative to l3_off (ihl*4, or 40+ext headers)    */
    uint8_t  l3_ver;   /* 4 or 6                                                             */
    uint8_t  l4_proto; /* 6 TCP, 17 UDP, 1 ICMP, 58 ICMPv6; anything else: no L4 sum          */
    uint8_t  flags;    /* VPCSUM_F_*                                                          */
    uint8_t  rsv;      /* must be 0                                                          */
} vpcsum_desc_t;       /* 16 bytes, naturally aligned                                        */

/* Output word per packet: bits 0..15 = IPv4 header checksum, bits 16..31 = L4 checksum
 * (host-order values, exactly the ints Java writes with ByteArray.int16). */

/* Status byte per packet (optional output). */
#define VPCSUM_S_IP_OK       0x01u /* verify: stored IPv4 header checksum == recomputed   */
#define VPCSUM_S_L4_OK       0x02u /* verify: stored L4 checksum == recomputed            */
#define VPCSUM_S_UDP_NOCSUM  0x04u /* UDP with stored checksum 0 (RFC 768 "no checksum")  */
#define VPCSUM_S_MSS_ABSENT  0x08u /* NAT with VPCSUM_NAT_TCP_REWRITES, next to S_DONE:
                                    * VPCSUM_TCP_CLAMP_MSS on a SYN whose options parse and hold no
                                    * MSS option.  The packet is otherwise complete; the caller adds
                                    * the option on the host (checkAndUpdateMss's rebuild branch,
                                    * SwitchUtils.java:83-94: it changes lengths)                  */
#define VPCSUM_S_TTL_EXPIRED 0x20u /* NAT: VPCSUM_NAT_DEC_TTL on a TTL / hop limit <= 1 (the value
                                    * after VPCSUM_NAT_SET_TTL when both are set): the packet is
                                    * refused with S_BAD_DESC and nothing is written.  The reference
                                    * never decrements such a packet: IPInputRoute drops it and
                                    * answers ICMP time exceeded (IPInputRoute.java:81-88); that
                                    * answer is vpcsum_icmp_reply_async's VPCSUM_ICMP_TIME_EXCEEDED */
#define VPCSUM_S_DONE        0x40u /* descriptor processed                                */
#define VPCSUM_S_BAD_DESC    0x80u /* descriptor rejected (bounds/lengths); nothing written */

/* Batch modes. */
#define VPCSUM_MODE_COMPUTE  0x00u /* compute dirty sums                                    */
#define VPCSUM_MODE_VERIFY   0x01u /* compute and compare with the stored fields (ingress)  */
#define VPCSUM_MODE_WRITE    0x10u /* also write results big-endian into the arena in place */

/* NAT / TTL rewrites (SwitchUtils.applyNat, core/.../vswitch/util/SwitchUtils.java:522-542): the
 * setters Ipv4Packet.setSrc/setDst (vpacket/Ipv4Packet.java:433-458), Ipv6Packet.setSrc/setDst
 * (Ipv6Packet.java:374-396), TcpPacket/UdpPacket.setSrcPort/setDstPort (TcpPacket.java:31-51,
 * UdpPacket.java:188-209), Ipv4Packet.setTtl (:401-407; IPInputRoute.java:79-91 decrements) and
 * Ipv6Packet.setHopLimit (:354-359), each followed by Java's recompute of the sums it dirtied.
 * Address and port bytes in NETWORK byte order, exactly the bytes written into the packet. */
#define VPCSUM_NAT_SRC      0x01u /* source address (IPv4 bytes 12..15 / IPv6 8..23)             */
#define VPCSUM_NAT_DST      0x02u /* destination address (IPv4 16..19 / IPv6 24..39)              */
#define VPCSUM_NAT_SPORT    0x04u /* TCP / UDP source port                                        */
#define VPCSUM_NAT_DPORT    0x08u /* TCP / UDP destination port                                   */
#define VPCSUM_NAT_DEC_TTL  0x10u /* IPv4 TTL / IPv6 hop limit minus 1 (after SET_TTL if both); a
                                   * value <= 1 refuses the packet (VPCSUM_S_TTL_EXPIRED)        */
#define VPCSUM_NAT_SET_TTL  0x20u /* IPv4 TTL / IPv6 hop limit := the entry's ttl value           */
#define VPCSUM_NAT_TCP      0x40u /* vpcsum_nat_t only, honoured only under the nat_mode bit
                                   * VPCSUM_NAT_TCP_REWRITES: rsv[0..7] hold TCP-header rewrites   */

/* The TCP part of a vpcsum_nat_t entry with VPCSUM_NAT_TCP -- what the reference does to a NAT'd
 * TCP packet in place besides applyNat: buildSynPacketForProxyProtocol (SwitchUtils.java:461-465,
 * setSeqNum(seq - N)), buildSynAckPacketForProxyProtocol (:467-473, setSeqNum(seq - 1),
 * setFlags(SYN|ACK)) and checkAndUpdateMss (:46-95, run by every Switch.sendPacket).
 *   rsv[0]     ops, VPCSUM_TCP_*
 *   rsv[1]     the flags value (low 6 bits; TcpPacket.setFlags, TcpPacket.java:90-96)
 *   rsv[2..3]  maxMss, network order
 *   rsv[4..7]  the sequence addend, network order, added mod 2^32 (seq - N: the addend -N)
 *   rsv[8..9]  0
 * Applied after the address / port / TTL rewrite, to a packet that rewrite did not refuse, with
 * l4_proto 6 and 20 bytes of segment; any other packet ignores the ops (as SPORT / DPORT on ICMP).
 * SET_FLAGS and SEQ_ADD always dirty the TCP sum (the setters call checksumSkipped() whatever the
 * value).  CLAMP_MSS applies when SYN is set after SET_FLAGS: the options are walked as
 * TcpPacket.from walks them (TcpPacket.java:241-287, TcpOption.check :622-636); a walk that fails
 * changes nothing (Java's ensurePartialPacketParsed returns); else the first MSS option before any
 * END has its 2 data bytes overwritten when its value is above maxMss (sum dirtied), is left
 * alone when not (nothing dirtied), and when there is none VPCSUM_S_MSS_ABSENT is set. */
#define VPCSUM_TCP_SEQ_ADD   0x01u
#define VPCSUM_TCP_SET_FLAGS 0x02u
#define VPCSUM_TCP_CLAMP_MSS 0x04u

/* IPv4-only entry, 16 bytes (BASELINE config C5: 72 algorithmic bytes per packet).
 * rsv[0] carries the VPCSUM_NAT_SET_TTL value; an IPv6 descriptor is rejected (S_BAD_DESC). */
typedef struct vpcsum_nat4 {
    uint8_t  src[4];
    uint8_t  dst[4];
    uint8_t  sport[2];
    uint8_t  dport[2];
    uint8_t  mask;     /* VPCSUM_NAT_*  */
    uint8_t  rsv[3];   /* rsv[0]: TTL value for VPCSUM_NAT_SET_TTL, others 0 */
} vpcsum_nat4_t;

/* IPv4 and IPv6 entry, 48 bytes: an IPv4 packet uses src[0..3] / dst[0..3]. */
typedef struct vpcsum_nat {
    uint8_t  src[16];
    uint8_t  dst[16];
    uint8_t  sport[2];
    uint8_t  dport[2];
    uint8_t  mask;     /* VPCSUM_NAT_*                                  */
    uint8_t  ttl;      /* TTL / hop limit value for VPCSUM_NAT_SET_TTL    */
    uint8_t  rsv[10];  /* 0, or with VPCSUM_NAT_TCP the TCP rewrites above */
} vpcsum_nat_t;

/* IPv4 record, 32 bytes: a packet's descriptor and its IPv4 entry side by side, so the rewrite
 * kernel reads one stream of 32 B per packet instead of two of 16 B (vpcsum_nat4r_async). */
typedef struct vpcsum_nat4_rec {
    vpcsum_desc_t desc;
    vpcsum_nat4_t rw;
} vpcsum_nat4_rec_t;

/* NAT modes. */
#define VPCSUM_NAT_RFC1624     0x00u /* incremental update (RFC 1624 eqn. 3); header bytes only */
#define VPCSUM_NAT_STRICT_JAVA 0x01u /* rewrite, then full recompute: identical to Java for ANY
                                        input, including invalid input checksums              */
#define VPCSUM_NAT_TCP_REWRITES 0x02u /* honour VPCSUM_NAT_TCP in this batch (48-byte entries only,
                                        * a status buffer required).  Without it the mask bit and
                                        * rsv are ignored and the kernels launched are unchanged.
                                        * RFC 1624: the TCP sum is updated over the changed words,
                                        * composed with the address / port update.  Strict Java: the
                                        * rewrite adds F_L4 to the packet's dirty flags before the
                                        * recompute; S_MSS_ABSENT is derived from the bytes after it */

/* Pre-image of a packet NAT'd by Java's own setters (VPCSUM_F_PRE): the OLD addresses and ports,
 * recorded just before SwitchUtils.applyNat ran the setters (SwitchUtils.java:531-542), in the
 * layout of the NAT entries: vpcsum_pre_t = vpcsum_nat_t (48 B; an IPv4 packet uses src[0..3] /
 * dst[0..3]) and vpcsum_pre4_t = vpcsum_nat4_t (16 B, IPv4 only).  mask: VPCSUM_NAT_SRC / DST /
 * SPORT / DPORT, the fields recorded (a field recorded but not changed adds nothing); the TTL
 * bits and values are ignored: the IPv4 header sum is recomputed in full from the header. */
typedef vpcsum_nat_t vpcsum_pre_t;
typedef vpcsum_nat4_t vpcsum_pre4_t;
#define VPCSUM_PRE_FMT_PRE4 0u   /* vpcsum_pre4_t entries */
#define VPCSUM_PRE_FMT_PRE  1u   /* vpcsum_pre_t entries  */

/* Ingress header sum of a received TCP / UDP frame, recorded by the RX verify
 * (vpcsum_ctx_verify_frames_hsum) from the frame as it arrived.  `sum` is the one's complement sum
 * (16-bit big-endian words, folded end-around; host order) of every word of the L4 sum that the
 * vswitch's in-place setters can reach: the pseudo-header addresses (IPv4 L3+12..19, IPv6
 * L3+8..39) and the L4 header's words [0, hlen) except the checksum field -- ports, sequence and
 * acknowledgement numbers, flags, window, options (TcpPacket.java:31-110, TcpOption.setData
 * :561-569; UdpPacket.java:188-209; Ipv4Packet/Ipv6Packet.setSrc/setDst).  At egress
 * (VPCSUM_PRE_HSUM) the L4 sum is updated from it, RFC 1624 eqn. 3 with the header as one word:
 * HC' = ~(~HC + ~sum + sum'), sum' the same words of the frame now.  That equals Java's full
 * recompute (getRawPacket(0), AbstractPacket.java:15-22) for ANY change of those words, provided the
 * stored HC was correct on receipt (VPCSUM_S_L4_OK) and the payload and lengths are the received
 * ones: the caller's part (INTEGRATION.md §5 gives the vswitch's rule).  l2_len = 0: no record
 * (not TCP / UDP, a refused frame, a segment shorter than its header). */
typedef struct vpcsum_hsum {
    uint16_t sum;
    uint16_t l4_len;   /* segment length on receipt: l3_len - l4_off                         */
    uint8_t  hlen;     /* L4 header bytes summed: TCP data offset * 4 (20..60), UDP 8         */
    uint8_t  l4_proto; /* 6 / 17                                                              */
    uint8_t  l3_ver;   /* 4 / 6                                                               */
    uint8_t  l2_len;   /* 14 / 18 (802.1Q): the L3 header's offset in the frame; 0: no record  */
} vpcsum_hsum_t;       /* 8 bytes */

/* vpcsum_pre_t / vpcsum_pre4_t mask bit: the entry's first 8 bytes (src[0..7], or src[0..3] and
 * dst[0..3] of a vpcsum_pre4_t) hold the packet's vpcsum_hsum_t instead of old addresses and
 * ports (the other mask bits are then ignored).  The packet is refused (S_BAD_DESC, nothing
 * written) unless its version, protocol, segment length and L4 header length (the TCP data offset
 * now in the frame) equal the record's. */
#define VPCSUM_PRE_HSUM 0x80u

/* ------------------------------------------------------------------------ */
/* Library / device                                                         */
/* ------------------------------------------------------------------------ */
int         vpcsum_abi_version(void);
const char* vpcsum_last_error(void);          /* thread-local message of the last failure */
int         vpcsum_device_count(int* out_n);
int         vpcsum_set_device(int device);

/* ------------------------------------------------------------------------ */
/* Device-resident batch ops (async on `stream`; all pointers device memory) */
/* ------------------------------------------------------------------------ */

/* Compute / verify the checksums named by each descriptor's flags.
 * d_out (n words) and d_status (n bytes) may each be NULL. */
int vpcsum_compute_async(const uint8_t* d_arena, uint64_t arena_len,
                         const vpcsum_desc_t* d_desc, uint32_t n,
                         uint32_t* d_out, uint8_t* d_status,
                         uint32_t mode, void* stream);

/* Two batches in flight.  A launch spends its first and last microseconds
 * ramping up and draining; a caller that keeps two batches in flight overlaps those with its
 * neighbour's steady state (C1, 64-B frames: +29%).  A pipe owns two streams on the
 * caller's device: vpcsum_pipe_begin forks them from `stream` (they wait for the work queued on it
 * so far), each vpcsum_pipe_compute_async (vpcsum_compute_async's arguments) goes to the next of the
 * two in turn, so consecutive batches may run concurrently -- their out / status / written frames
 * must not overlap -- and vpcsum_pipe_join makes `stream` wait for every batch launched since.  The
 * host contexts do the same on their own: each keeps two slots, each with its stream, and a submit
 * goes to the other slot than the last (wait for ticket t before reusing t's buffers). */
typedef struct vpcsum_pipe vpcsum_pipe_t;
int vpcsum_pipe_create(void* stream, vpcsum_pipe_t** out);
int vpcsum_pipe_begin(vpcsum_pipe_t* pipe);
int vpcsum_pipe_compute_async(vpcsum_pipe_t* pipe, const uint8_t* d_arena, uint64_t arena_len,
                              const vpcsum_desc_t* d_desc, uint32_t n, uint32_t* d_out, uint8_t* d_status,
                              uint32_t mode);
int vpcsum_pipe_join(vpcsum_pipe_t* pipe);
int vpcsum_pipe_destroy(vpcsum_pipe_t* pipe);

/* NAT / TTL rewrite + checksum update, in place in the arena; d_rw[i] rewrites packet i.
 * d_status (n bytes): S_DONE, or S_BAD_DESC for a rejected descriptor (nothing written);
 * required with VPCSUM_NAT_STRICT_JAVA and with VPCSUM_NAT_TCP_REWRITES.  That mode bit is taken
 * by vpcsum_nat_async (and the host-frame submits built on it) only: the 16-byte entry formats
 * refuse it. */
int vpcsum_nat4_async(uint8_t* d_arena, uint64_t arena_len,
                      const vpcsum_desc_t* d_desc, const vpcsum_nat4_t* d_rw, uint32_t n,
                      uint8_t* d_status, uint32_t nat_mode, void* stream);
int vpcsum_nat_async(uint8_t* d_arena, uint64_t arena_len,
                     const vpcsum_desc_t* d_desc, const vpcsum_nat_t* d_rw, uint32_t n,
                     uint8_t* d_status, uint32_t nat_mode, void* stream);
/* vpcsum_nat4_async over records (descriptor + entry per packet, one read stream); IPv4 only,
 * VPCSUM_NAT_RFC1624 only (the strict-Java recompute reads plain descriptors). */
int vpcsum_nat4r_async(uint8_t* d_arena, uint64_t arena_len, const vpcsum_nat4_rec_t* d_rec, uint32_t n,
                       uint8_t* d_status, uint32_t nat_mode, void* stream);

/* Egress sums of NAT'd packets from their pre-images: every descriptor with VPCSUM_F_PRE gets its
 * L4 sum by RFC 1624 eqn. 3 from the stored field, the old words d_pre[i] records and the words now
 * in the frame (HC' = ~(~HC + sum(~m + m'))) -- with VPCSUM_PRE_HSUM, the recorded header sum and the
 * same header words now (any in-place change of them) --, its IPv4 header sum (F_IP) recomputed in full from the
 * header; a UDP stored 0 (no checksum) is summed in full.  The results equal Java's full recompute
 * (getRawPacket(0) after the setters, AbstractPacket.java:15-22) whenever the stored L4 sum was
 * correct before the rewrite -- what ingress verify's VPCSUM_S_L4_OK proves -- and nothing but the
 * recorded fields changed since.  pre_fmt: VPCSUM_PRE_FMT_PRE4 (IPv4 only) or VPCSUM_PRE_FMT_PRE.
 * mode: VPCSUM_MODE_WRITE to store the sums into the frames.  Out / status as vpcsum_compute_async
 * (S_BAD_DESC: F_PRE without F_L4 or F_IP, with F_L4P / F_RAW, F_IP on IPv6, an IPv6 packet with
 * 16-B entries, bounds).  d_pre holds n entries; those of descriptors without F_PRE are ignored.  Descriptors without F_PRE are not touched (out / status not written): run
 * vpcsum_compute_async on the same batch first, on the same stream, for them. */
int vpcsum_pre_async(uint8_t* d_arena, uint64_t arena_len, const vpcsum_desc_t* d_desc, const void* d_pre,
                     uint32_t pre_fmt, uint32_t n, uint32_t* d_out, uint8_t* d_status, uint32_t mode, void* stream);

/* Build descriptors on the GPU by parsing Ethernet frames (EthernetPacket.from,
 * Ipv4Packet.from, Ipv6Packet.from rules). frame i = [d_frame_off[i], +d_frame_len[i]).
 * flags = VPCSUM_F_* applied to every IP packet found; non-IP / unparsable frames get
 * flags 0 and status VPCSUM_S_BAD_DESC. */
int vpcsum_parse_ether_async(const uint8_t* d_arena, uint64_t arena_len,
                             const uint64_t* d_frame_off, const uint32_t* d_frame_len, uint32_t n,
                             uint8_t flags, vpcsum_desc_t* d_desc, uint8_t* d_status, void* stream);

/* Flow tuple of a parsed frame: what the vswitch's L4 input nodes read before their conntrack
 * lookup (TcpInput.java:47-51: tcpPkt.getSrc(ipPkt) / getDst(ipPkt) -> conntrack.lookupTcp, and
 * getFlags() == SYN -> lookupTcpListen; UdpInput.java:45-47: IPPort(ipPkt.getDst(),
 * udpPkt.getDstPort()) -> lookupUdpListen), and what SwitchUtils.executeTcpNat / executeUdpNat
 * compare (:321-322, :506-507).  Addresses and ports in network order; an IPv4 address is the
 * first 4 bytes (zeros after).  Ports (TcpPacket / UdpPacket.initPartial: uint16 at 0 and 2) and
 * tcp_flags (TcpPacket.initPartial :192-195: uint16 at 12 & 0x3f) are 0 for other protocols.  A
 * refused frame (status S_BAD_DESC) gets an all-zero tuple (l3_ver 0). */
typedef struct vpcsum_tuple {
    uint8_t src[16];
    uint8_t dst[16];
    uint8_t sport[2];
    uint8_t dport[2];
    uint8_t l3_ver;      /* 4 / 6; 0: refused frame */
    uint8_t l4_proto;
    uint8_t tcp_flags;
    uint8_t rsv;
} vpcsum_tuple_t;        /* 40 bytes */

/* vpcsum_parse_ether_async that also writes one vpcsum_tuple_t per frame to d_tuples (batched
 * header parse + tuple extraction), in the same pass over the headers. */
int vpcsum_parse_ether_tuples_async(const uint8_t* d_arena, uint64_t arena_len,
                                    const uint64_t* d_frame_off, const uint32_t* d_frame_len, uint32_t n,
                                    uint8_t flags, vpcsum_desc_t* d_desc, uint8_t* d_status,
                                    vpcsum_tuple_t* d_tuples, void* stream);

/* vpcsum_parse_ether_async that also writes each frame's ingress header sum (vpcsum_hsum_t,
 * l2_len 0 for a frame without one) to d_hsum, from the header bytes the parse reads. */
int vpcsum_parse_ether_hsum_async(const uint8_t* d_arena, uint64_t arena_len,
                                  const uint64_t* d_frame_off, const uint32_t* d_frame_len, uint32_t n,
                                  uint8_t flags, vpcsum_desc_t* d_desc, uint8_t* d_status,
                                  vpcsum_hsum_t* d_hsum, void* stream);

/* NAT flow table (additive, the ABI version stays 4): an exact-match table on one device from the
 * tuple vpcsum_parse_ether_tuples_async writes -- conntrack.lookupTcp / lookupUdp's key (remote =
 * the packet's source IPPort, local = its destination; Conntrack.java:106-125, TcpInput.java:47-51,
 * UdpInput.java:45-47): protocol, both addresses, both ports, as received -- to the vpcsum_nat_t
 * that SwitchUtils.applyNat writes for that flow direction (SwitchUtils.java:522-542).  The host
 * inserts and erases flows at connection-setup rate; parse, lookup and rewrite of every packet
 * stay on the device.  Only the stateless fast path is offloaded: in ESTABLISHED a TCP packet
 * without FIN / SYN / RST gets resetTimer() and applyNat (executeTcpNat, SwitchUtils.java:318-459),
 * a UDP packet always (executeUdpNat); every other packet of a known flow is handed back untouched
 * (PUNT), and vpcsum_flowtab_collect tells the host which flows were hit (its resetTimer).
 * INTEGRATION.md §5 has the vswitch's rule.  A table belongs to one device: there is no device
 * group, process-wide or service-grid form. */
#define VPCSUM_FLOW_MISS 0u /* no such flow, a refused frame (l3_ver 0), or not TCP / UDP           */
#define VPCSUM_FLOW_HIT  1u /* found: the flow's entry is the packet's rewrite                      */
#define VPCSUM_FLOW_PUNT 2u /* found, but TCP with FIN | SYN | RST (tcp_flags & 0x07): the host's   */
typedef struct vpcsum_flow {
    vpcsum_tuple_t key;   /* tcp_flags and rsv 0; an IPv4 address in the first 4 bytes, zeros after */
    vpcsum_nat_t   rw;    /* the rewrite of every HIT packet of the flow                             */
    uint64_t       cookie;/* the caller's name for the flow, returned by vpcsum_flowtab_collect      */
} vpcsum_flow_t;          /* 96 bytes */
typedef struct vpcsum_flowtab vpcsum_flowtab_t;

/* A table for up to max_flows flows on `device` (slots: a power of two >= 2 x max_flows, 128 B each). */
int vpcsum_flowtab_create(int device, uint32_t max_flows, vpcsum_flowtab_t** out);
int vpcsum_flowtab_destroy(vpcsum_flowtab_t* tab);
/* erase h_del[0..n_del) (a key not present is not an error), then insert / replace h_add[0..n_add)
 * (a key already present keeps its flow and takes the new rw and cookie).
 * The changed slots are copied on `stream` and the call returns after those copies completed:
 * lookups queued on `stream` before the call see the old table, lookups after it the new one.
 * A refused insert -- l4_proto other than 6 / 17, l3_ver other than 4 / 6, an IPv4 key with non-zero
 * address bytes 4..15, non-zero tcp_flags / rsv, a full table -- fails the call with nothing changed. */
int vpcsum_flowtab_update(vpcsum_flowtab_t* tab, const vpcsum_tuple_t* h_del, uint32_t n_del,
                          const vpcsum_flow_t* h_add, uint32_t n_add, void* stream);
/* slots, live flows, and the largest distance of a live flow from its home slot (any may be NULL) */
int vpcsum_flowtab_info(vpcsum_flowtab_t* tab, uint32_t* slots, uint32_t* flows, uint32_t* max_probe);
/* the table's hash of a key's 38 bytes (tcp_flags / rsv are not read): home slot = hash & (slots - 1) */
int vpcsum_flow_hash(const vpcsum_tuple_t* key, uint64_t* out);
/* Look n tuples up (device pointers, 4-byte aligned; d_rw n x vpcsum_nat_t, d_verdict n bytes):
 * d_verdict[i] = VPCSUM_FLOW_*; d_rw[i] = the flow's entry on HIT, 48 zero bytes otherwise (mask 0:
 * vpcsum_nat_async answers S_DONE and leaves the frame alone).  A HIT marks the flow for
 * vpcsum_flowtab_collect.  On the table's device. */
int vpcsum_flow_lookup_async(vpcsum_flowtab_t* tab, const vpcsum_tuple_t* d_tuples, uint32_t n,
                             vpcsum_nat_t* d_rw, uint8_t* d_verdict, void* stream);
/* cookies of the live flows that had a HIT since the last collect, each once; clears the marks.
 * Synchronises `stream`. *n_out > cap: nothing cleared, call again with room. */
int vpcsum_flowtab_collect(vpcsum_flowtab_t* tab, uint64_t* h_cookies, uint32_t cap, uint32_t* n_out, void* stream);

/* A flow's Fastpath (additive, the ABI version stays 4): what Switch.sendPacket records on the
 * connection entry from the first packet of a flow that leaves (Fastpath.java:11-22,
 * Switch.java:660-672) -- the Ethernet addresses the frame left with and where it went --, so that
 * later HIT frames of the flow need no route and no MAC lookup on the host.  port is the caller's
 * name for Fastpath.output (and the vrf, if it wants to encode one); port 0 means "no Fastpath":
 * zeroed slots and every flow vpcsum_flowtab_update inserts have none.
 * vpcsum_flowtab_update and the Fastpath: a new flow has none; a replaced key keeps its flow id and
 * its Fastpath; an erased flow's Fastpath goes with it, and a flow that later takes the slot starts
 * with none; the backward shift of an erase moves the Fastpath with its flow. */
typedef struct vpcsum_fastpath {
    uint8_t  dst[6];      /* Fastpath.remote: frame bytes [0,6), wire order                          */
    uint8_t  src[6];      /* Fastpath.local: frame bytes [6,12)                                      */
    uint32_t port;        /* 0 = no Fastpath                                                         */
} vpcsum_fastpath_t;      /* 16 bytes */
/* Set the Fastpath of each key h_keys[i] that is present to h_fp[i]; port 0 clears it (the stored
 * record is then all zeros).  A key not present is not an error (the host may have erased the flow
 * meanwhile): such keys are counted in *n_missing (may be NULL).  A malformed key (the refusals of
 * vpcsum_flowtab_update) fails the call with nothing changed.  Ordered as vpcsum_flowtab_update: the
 * changed slots are copied on `stream` and the call returns after those copies completed. */
int vpcsum_flowtab_set_fastpath(vpcsum_flowtab_t* tab, const vpcsum_tuple_t* h_keys, const vpcsum_fastpath_t* h_fp,
                                uint32_t n, uint32_t* n_missing, void* stream);
/* vpcsum_flow_lookup_async that also writes d_fp[i] (n x 16 bytes, 4-byte aligned): the flow's
 * Fastpath record on HIT, 16 zero bytes otherwise. */
int vpcsum_flow_lookup_fp_async(vpcsum_flowtab_t* tab, const vpcsum_tuple_t* d_tuples, uint32_t n,
                                vpcsum_nat_t* d_rw, uint8_t* d_verdict, vpcsum_fastpath_t* d_fp, void* stream);
/* The L2 write of a looked-up and rewritten batch (device pointers; d_fp 4-byte aligned, d_frame_off
 * of any alignment): frame i gets d_fp[i].dst written to its bytes [0,6), d_fp[i].src to [6,12) and
 * d_port[i] = d_fp[i].port only when d_verdict[i] is VPCSUM_FLOW_HIT, d_status[i] has S_DONE and not
 * S_BAD_DESC (S_MSS_ABSENT beside S_DONE does not matter) and d_fp[i].port != 0 -- exactly
 * EthernetPacket.setDst / setSrc on a packet with its raw bytes (EthernetPacket.java:184-205):
 * EtherType, an 802.1Q tag, lengths and padding are untouched.  Every other frame keeps its Ethernet
 * header and gets d_port[i] = 0; so does a frame with frame_len < 14 or frame_off + frame_len >
 * arena_len. */
int vpcsum_l2_forward_async(uint8_t* d_arena, uint64_t arena_len, const uint64_t* d_frame_off,
                            const uint32_t* d_frame_len, const uint8_t* d_verdict, const uint8_t* d_status,
                            const vpcsum_fastpath_t* d_fp, uint32_t n, uint32_t* d_port, void* stream);

/* TCP segment build (additive, the ABI version stays 4): what the userspace TCP stack does on the
 * host for every segment it sends (TcpStack.transmitTcpPsh -> sendTcpPsh, TcpStack.java:469-503,
 * 553-566: TcpUtils.buildCommonTcpResponse / buildIpResponse, TcpUtils.java:15-57; on the Fastpath
 * a new Ethernet header, L4Output.java:56-72, Fastpath.java:24-47; XDPIface.sendPacket's copy into
 * a umem chunk), as one fused copy-and-checksum: "connection header + payload run" in, finished
 * frames out.  The payload is read once from the send buffer and written once into the frame, the
 * TCP sum accumulated on the way, the headers generated from the template; the result equals
 * getRawPacket(0) of what sendTcpPsh / sendTcpFin / buildAckResponse / buildRstResponse build.
 * SYNs carry options and stay on the host.  Fields marked "wire" are network order, exactly the
 * bytes written into the frame. */
typedef struct vpcsum_tcphdr {     /* one per connection direction; 64 bytes */
    uint8_t  eth_dst[6];   /*  0  Fastpath.remote  (frame bytes [0,6))  */
    uint8_t  eth_src[6];   /*  6  Fastpath.local   (frame bytes [6,12)) */
    uint8_t  l2_len;       /* 12  14: Ethernet header written, EtherType from l3_ver (0x0800 / 0x86dd,
                                  Fastpath.java:39-43); 0: the frame starts at the IP header (L4Output's ip-output edge) */
    uint8_t  l3_ver;       /* 13  4 / 6 */
    uint8_t  tos;          /* 14  IPv4 byte 1 (dscp<<2|ecn) / IPv6 traffic class; the stack uses 0 */
    uint8_t  ttl;          /* 15  TTL / hop limit; the stack uses 64 */
    uint8_t  src[16];      /* 16  IPv4: first 4 bytes, the rest ignored */
    uint8_t  dst[16];      /* 32 */
    uint8_t  sport[2];     /* 48  wire */
    uint8_t  dport[2];     /* 50  wire */
    uint8_t  ack[4];       /* 52  wire */
    uint8_t  window[2];    /* 56  wire */
    uint8_t  ident[2];     /* 58  IPv4 identification, wire (the stack: 0); ignored for IPv6 */
    uint8_t  frag[2];      /* 60  IPv4 flags<<13 | fragment offset, wire (the stack: 0); ignored for IPv6 */
    uint8_t  rsv[2];       /* 62  must be 0 */
} vpcsum_tcphdr_t;

typedef struct vpcsum_tcpseg {     /* one per frame to build; 32 bytes */
    uint64_t frame_off;    /*  0  where the frame starts in the destination arena, any alignment */
    uint64_t data_off;     /*  8  where the payload starts in the source arena, any alignment */
    uint32_t seq;          /* 16  host order; written big-endian */
    uint32_t hdr;          /* 20  index into the header array */
    uint32_t frame_cap;    /* 24  room at frame_off (the chunk's); a frame that needs more is refused */
    uint16_t data_len;     /* 28  0 for ACK / FIN / RST */
    uint8_t  flags;        /* 30  TCP flags, low 6 bits (TcpPacket.setFlags) */
    uint8_t  rsv;          /* 31  must be 0 */
} vpcsum_tcpseg_t;

/* Frame i, of length L = l2_len + (20 | 40) + 20 + data_len, at d_dst + frame_off:
 *   Ethernet (l2_len 14): eth_dst, eth_src, EtherType.
 *   IPv4 (Ipv4Packet.genHeaderWithChecksumUnfilled :279-294, IHL 5): 45, tos, totalLength 40 +
 *     data_len, ident, frag, ttl, 06, the header sum (Utils.calculateChecksum over the 20 bytes),
 *     src[0..3], dst[0..3].
 *   IPv6 (Ipv6Packet.buildPacket :185-190, no extension headers, flow label 0): 60 | tos>>4,
 *     (tos<<4) & 0xff, 00 00, payloadLength 20 + data_len, 06, ttl, src, dst.
 *   TCP (TcpPacket.buildCommonPart :394-452, no options): sport, dport, seq, ack, 50, flags, window,
 *     the TCP sum (pseudo-header and segment; 0x0000 is stored as it is), urgent pointer 00 00, the
 *     data_len payload bytes from d_src + data_off.
 * A record is refused -- d_frame_len[i] 0, d_out[i] 0, S_BAD_DESC, not one byte written, nothing read
 * but the record and its template -- when hdr >= n_hdr; the template's l3_ver is not 4 / 6, its l2_len
 * not 0 / 14 or its rsv not 0; flags & ~0x3f or the record's rsv != 0; L > frame_cap; 40 + data_len
 * (IPv4) or 20 + data_len (IPv6) > 65535 (Java would silently truncate the length field: the build
 * refuses); frame_off + L > dst_len or data_off + data_len > src_len (both checked without wrapping).
 * Otherwise d_frame_len[i] = L (required), d_out[i] (may be NULL) holds the IPv4 header sum in bits
 * 0..15 (0 for IPv6) and the TCP sum in bits 16..31, d_status[i] (may be NULL) S_DONE.
 * Templates and frame lengths 4-byte aligned, records 8-byte aligned; n at most 2^28; n == 0 returns 0.
 * Frames of one batch must not overlap each other or any payload range: the caller's rule, as for the
 * NAT submits. */
int vpcsum_tcp_build_async(uint8_t* d_dst, uint64_t dst_len, const uint8_t* d_src, uint64_t src_len,
                           const vpcsum_tcphdr_t* d_hdr, uint32_t n_hdr, const vpcsum_tcpseg_t* d_seg, uint32_t n,
                           uint32_t* d_frame_len, uint32_t* d_out, uint8_t* d_status, void* stream);

/* TCP send bursts (additive, the ABI version stays 4): the segment build with the stack's slicing
 * done on the device.  One record per SendingQueue.fetch() (TcpEntry.java:213-241) instead of one
 * per frame: transmitTcpPsh (TcpStack.java:469-503) sends every piece of a fetch with the same
 * template and the same flags, so a burst says where the run of payload starts, how long it is, its
 * first sequence number and the MSS, and the frames are cut from it on the GPU. */
typedef struct vpcsum_tcpburst {   /* one per fetch(); 32 bytes, 8-byte aligned */
    uint64_t data_off;  /*  0  first payload byte in the source arena, any alignment          */
    uint32_t data_len;  /*  8  payload bytes of the whole burst: min(window, queued) of fetch() */
    uint32_t seq;       /* 12  sequence number of the first byte, host order                   */
    uint32_t hdr;       /* 16  index into the template array                                   */
    uint32_t first;     /* 20  index of the burst's first frame in the frame table             */
    uint16_t mss;       /* 24  payload bytes of every frame but the last                       */
    uint8_t  flags;     /* 26  TCP flags of every frame (the stack: PSH | ACK)                 */
    uint8_t  rsv;       /* 27  must be 0                                                       */
    uint32_t count;     /* 28  frames of the burst                                             */
} vpcsum_tcpburst_t;

/* Frame j of the table d_frame_off[0..n_frames) belongs to the last burst b with first[b] <= j (the
 * search takes `first` to be non-decreasing).  With k = j - first[b], frame j is exactly the frame
 * vpcsum_tcp_build_async builds from the record
 *   {d_frame_off[j], data_off + k * mss, seq + k * mss (mod 2^32), hdr, frame_cap,
 *    min(mss, data_len - k * mss), flags, 0},
 * with the same d_frame_len[j] (required), d_out[j] and d_status[j] (each may be NULL).  A burst with
 * data_len 0 has one frame without payload -- the ACK / FIN / RST of the per-segment build; its mss
 * is not read -- so one call carries a whole transmit round.  frame_cap is one value for the call
 * (umem chunks have one size).
 * A whole burst is refused -- every frame of it gets d_frame_len 0, d_out 0, S_BAD_DESC, not one byte
 * is written, nothing is read but the burst record and its template -- when hdr >= n_hdr or the
 * template is one vpcsum_tcp_build_async refuses; flags & ~0x3f or rsv != 0; data_len > 0 and mss == 0;
 * count != max(1, ceil(data_len / mss)); 40 (IPv4) or 20 (IPv6) + min(mss, data_len), the length field
 * of the longest frame, > 65535; the header length + min(mss, data_len) > frame_cap; data_off >
 * src_len or data_len > src_len - data_off (no wrapping).  A single frame is refused, its siblings
 * built, only by its own destination: d_frame_off[j] + L > dst_len (no wrapping).  A frame no burst
 * covers -- j - first[b] >= count[b], or no burst at or before it -- is refused; so is every frame
 * when n_bursts is 0.
 * Memory safety does not rest on the table being sorted: a frame is only built from a burst record
 * it has checked itself against (first <= j, j - first < count) with all the bounds above, so an
 * unsorted table gives refused or oddly attributed frames, never an access outside
 * [d_frame_off[j], d_frame_off[j] + L) and the burst's own source range.
 * Templates and frame lengths 4-byte aligned, burst records and frame offsets 8-byte aligned;
 * n_frames and n_bursts each at most 2^28; n_frames == 0 returns 0.  Frames of one batch must not
 * overlap each other or any payload range: the caller's rule, as for the build. */
int vpcsum_tcp_build_bursts_async(uint8_t* d_dst, uint64_t dst_len, const uint8_t* d_src, uint64_t src_len,
                                  const vpcsum_tcphdr_t* d_hdr, uint32_t n_hdr, const vpcsum_tcpburst_t* d_burst,
                                  uint32_t n_bursts, const uint64_t* d_frame_off, uint32_t n_frames, uint32_t frame_cap,
                                  uint32_t* d_frame_len, uint32_t* d_out, uint8_t* d_status, void* stream);

/* TCP receive (additive, the ABI version stays 4): the build's mirror.  What the userspace TCP stack
 * does on the host for every data segment it receives -- TcpStack.handleTcpEstablished ->
 * receivingQueue.store(new Segment(seq, tcpPkt.getData())), TcpStack.java:302-306; ReceivingQueue.store
 * trims what was already received and copies the rest out of the RX chunk, TcpEntry.java:390-426 --
 * fused into the ingress verify: the segment is read once, its TCP sum recomputed and compared with
 * the stored field, and the payload bytes past `skip` stored into the connection's receive buffer
 * from the registers that summed them.  This call REPLACES vpcsum_compute_async / VPCSUM_MODE_VERIFY
 * for the frames it is given; it does not come on top of it.
 *
 * THE BYTES ARE STORED WHATEVER THE VERDICT: the sum is only known once the last byte has passed.
 * The caller advances expectingSeq only on VPCSUM_S_L4_OK; what it did not accept is overwritten by
 * the next batch. */
#define VPCSUM_TCPRX_STORE 0x01u
typedef struct vpcsum_tcprx {   /* one per descriptor; 16 bytes, 8-byte aligned */
    uint64_t dst_off;  /* where payload byte `skip` goes in the receive arena, any alignment */
    uint32_t dst_cap;  /* room at dst_off; a segment that needs more is refused */
    uint16_t skip;     /* leading payload bytes already received: store()'s incr = expectingSeq - seq */
    uint8_t  ops;      /* VPCSUM_TCPRX_STORE, or 0: verify only (pure ACKs, segments store() would drop) */
    uint8_t  rsv;      /* must be 0 */
} vpcsum_tcprx_t;

typedef struct vpcsum_tcpinfo { /* 16 bytes: what TcpStack reads of a segment before it decides */
    uint32_t seq, ack;          /* host order */
    uint16_t window, data_len;  /* host order; data_len = l3_len - l4_off - hlen */
    uint8_t  hlen;              /* data offset * 4 (20..60); 0: no record, the rest 0 */
    uint8_t  flags;             /* uint16 at 12 & 0x3f, as vpcsum_tuple_t.tcp_flags */
    uint8_t  rsv[2];
} vpcsum_tcpinfo_t;

/* Descriptor i (as vpcsum_parse_ether_async writes them) pairs with record i.  With hlen the TCP data
 * offset * 4 and data_len = l3_len - l4_off - hlen, a record that is not refused gets
 *   d_status[i], d_out[i] (each may be NULL): exactly what vpcsum_compute_async writes for the
 *     descriptor with VPCSUM_MODE_VERIFY -- S_DONE; S_L4_OK iff the stored TCP field equals the
 *     recomputed sum (exact: a stored 0xffff against a recomputed 0x0000 is not OK); S_IP_OK iff the
 *     descriptor has F_IP and the IPv4 header sum matches; d_out the recomputed sums;
 *   with VPCSUM_TCPRX_STORE: segment bytes [hlen + skip, l3_len - l4_off) at d_dst + dst_off and
 *     d_stored[i] (required) = data_len - skip; without it d_stored[i] = 0 and d_dst is not written.
 * L2 padding after l3_len is neither read nor summed.  No byte outside [dst_off, dst_off + stored) is
 * written.  A record is refused -- d_stored[i] 0, d_out[i] 0, S_BAD_DESC, not one byte written to
 * d_dst, nothing of the arena read but the TCP header's first 16 bytes, and those only when the
 * descriptor's bounds allow -- when l4_proto != 6; l3_ver is not 4 / 6; the descriptor lacks F_L4 or
 * carries F_L4P, F_RAW or F_PRE; F_IP on IPv6; l4_off > l3_len, or an l4_off vpcsum_compute_async
 * refuses (IPv4: below 20 or not a multiple of 4; IPv6: below 40); l3_off + l3_len > arena_len
 * (checked without wrapping); the segment is shorter than 20 bytes; the data offset is below 5 or
 * hlen larger than the segment; ops & ~VPCSUM_TCPRX_STORE or rsv != 0; skip > data_len; with STORE,
 * data_len - skip > dst_cap or dst_off + stored > dst_len (without wrapping).  skip == data_len is
 * legal and stores 0 bytes.  Descriptors and records 8-byte aligned, d_stored / d_out 4-byte aligned;
 * n at most 2^28; n == 0 returns 0.  Stored ranges of one batch must not overlap each other: the
 * caller's rule, as for the build. */
int vpcsum_tcp_recv_async(const uint8_t* d_arena, uint64_t arena_len, const vpcsum_desc_t* d_desc,
                          const vpcsum_tcprx_t* d_rx, uint32_t n, uint8_t* d_dst, uint64_t dst_len,
                          uint32_t* d_stored, uint32_t* d_out, uint8_t* d_status, void* stream);
/* What a device-resident caller needs between the parse and the receive: d_info[i] (16-byte aligned)
 * from the TCP header's first 16 bytes of descriptor i, so that the host runs store()'s arithmetic
 * on 16 bytes per segment instead of touching the frames.  The header refusals above apply (the
 * descriptor's and the data offset's); a refused descriptor's record is all zero. */
int vpcsum_tcp_digest_async(const uint8_t* d_arena, uint64_t arena_len, const vpcsum_desc_t* d_desc,
                            uint32_t n, vpcsum_tcpinfo_t* d_info, void* stream);

/* UDP datagram build (additive, the ABI version stays 4): the TCP segment build for the stack's UDP
 * sockets (UdpListenEntry: the vswitch's DNS, the datagram FDs).  What UdpOutput.sendUdp does on the
 * host for every datagram of sendingQueue.fetch() (UdpOutput.java:47-70: UdpUtils.buildCommonUdpResponse
 * / buildIpResponse, UdpUtils.java:15-56; on the EnhancedUDPEntry's Fastpath a new Ethernet header,
 * L4Output.java:39-55; XDPIface.sendPacket's copy into a umem chunk), as one fused copy-and-checksum:
 * the payload is read once and written once, the UDP sum accumulated on the way, the headers
 * generated from the template; the result equals getRawPacket(0) of what sendUdp builds, behind the
 * Fastpath's Ethernet header.
 *
 * The template is vpcsum_tcphdr_t's 64 bytes, one per EnhancedUDPEntry (remote, local): src / sport
 * from udp.listening, dst / dport from the datagram's remote, eth_dst / eth_src / l2_len 14 from the
 * entry's Fastpath (l2_len 0: the frame starts at the IP header), tos / ttl / ident / frag as for TCP
 * (the stack: 0, 64, 0, 0).  Bytes 52..57 (ack, window) and rsv must be 0. */
typedef vpcsum_tcphdr_t vpcsum_udphdr_t;

typedef struct vpcsum_udpdg {      /* one per datagram to build; 32 bytes, 8-byte aligned */
    uint64_t frame_off;    /*  0  where the frame starts in the destination arena, any alignment */
    uint64_t data_off;     /*  8  where the payload starts in the source arena, any alignment */
    uint32_t hdr;          /* 16  index into the template array */
    uint32_t frame_cap;    /* 20  room at frame_off (the chunk's); a frame that needs more is refused */
    uint32_t data_len;     /* 24  payload bytes; 0 is a legal datagram.  32 bits: a length the 16-bit
                                  fields cannot hold is refused, not truncated */
    uint32_t rsv;          /* 28  must be 0 */
} vpcsum_udpdg_t;

/* Frame i, of length L = l2_len + (20 | 40) + 8 + data_len, at d_dst + frame_off:
 *   Ethernet (l2_len 14): eth_dst, eth_src, EtherType, as in the TCP build.
 *   IPv4 (Ipv4Packet.genHeaderWithChecksumUnfilled :279-294, IHL 5): 45, tos, totalLength 28 +
 *     data_len, ident, frag, ttl, 11, the header sum (Utils.calculateChecksum over the 20 bytes),
 *     src[0..3], dst[0..3].
 *   IPv6 (Ipv6Packet.buildPacket :185-190, no extension headers, flow label 0): 60 | tos>>4,
 *     (tos<<4) & 0xff, 00 00, payloadLength 8 + data_len, 11, ttl, src, dst.
 *   UDP (UdpPacket.buildCommonPart + buildIPv4UdpPacket / buildIPv6UdpPacket, UdpPacket.java:68-124):
 *     sport, dport, length 8 + data_len, the UDP sum over the pseudo-header (protocol 17, length 8 +
 *     data_len), the header and the payload -- A COMPUTED 0x0000 IS STORED AS 0xffff --, the data_len
 *     payload bytes from d_src + data_off.
 * A record is refused -- d_frame_len[i] 0, d_out[i] 0, S_BAD_DESC, not one byte written, nothing read
 * but the record and its template -- when hdr >= n_hdr; the template's l3_ver is not 4 / 6, its l2_len
 * not 0 / 14, its bytes 52..57 or its rsv not 0; the record's rsv != 0; 28 + data_len (IPv4) or 8 +
 * data_len (IPv6) > 65535 (Java would silently truncate both length fields: the build refuses);
 * L > frame_cap; frame_off + L > dst_len or data_off + data_len > src_len (both checked without
 * wrapping).  Otherwise d_frame_len[i] = L (required), d_out[i] (may be NULL) holds the IPv4 header
 * sum in bits 0..15 (0 for IPv6) and the stored UDP field in bits 16..31, d_status[i] (may be NULL)
 * S_DONE.  Alignment, the limit on n, n == 0 and the no-overlap rule are vpcsum_tcp_build_async's. */
int vpcsum_udp_build_async(uint8_t* d_dst, uint64_t dst_len, const uint8_t* d_src, uint64_t src_len,
                           const vpcsum_udphdr_t* d_hdr, uint32_t n_hdr, const vpcsum_udpdg_t* d_dg, uint32_t n,
                           uint32_t* d_frame_len, uint32_t* d_out, uint8_t* d_status, void* stream);

/* UDP receive (additive, the ABI version stays 4): the build's mirror, the TCP receive for datagrams.
 * What UdpInput.handle does on the host for every datagram of a listening socket --
 * receivingQueue.store(src, port, udpPkt.getData().getRawPacket(0)), UdpInput.java:44-68;
 * ReceivingQueue.store's data.copy(), UdpListenEntry.java:51-65 -- fused into the ingress verify: the
 * segment is read once, its UDP sum recomputed and compared, and the data bytes stored from the
 * registers that summed them.  This call REPLACES vpcsum_compute_async / VPCSUM_MODE_VERIFY for the
 * frames it is given.  THE BYTES ARE STORED WHATEVER THE VERDICT, as in the TCP receive: the caller
 * enqueues the datagram only on the verdict its csum-recalc policy accepts; the source address and
 * port of the Datagram come from the parse's vpcsum_tuple_t. */
#define VPCSUM_UDPRX_STORE 0x01u
typedef struct vpcsum_udprx {   /* one per descriptor; 16 bytes, 8-byte aligned */
    uint64_t dst_off;  /* where data byte 0 goes in the receive arena, any alignment */
    uint32_t dst_cap;  /* room at dst_off; a datagram that needs more is refused */
    uint8_t  ops;      /* VPCSUM_UDPRX_STORE, or 0: verify only */
    uint8_t  rsv[3];   /* must be 0 */
} vpcsum_udprx_t;

/* Descriptor i (as vpcsum_parse_ether_async writes them) pairs with record i.  With seg_len = l3_len -
 * l4_off, a record that is not refused gets
 *   d_status[i], d_out[i] (each may be NULL): exactly what vpcsum_compute_async writes for the
 *     descriptor with VPCSUM_MODE_VERIFY -- S_DONE; the recomputed sum with a computed 0 as 0xffff;
 *     S_L4_OK iff the stored field equals it (so a stored 0xffff on a datagram whose sum computes to 0
 *     is OK); S_UDP_NOCSUM, and never S_L4_OK, for a stored 0; S_IP_OK iff the descriptor has F_IP and
 *     the IPv4 header sum matches;
 *   with VPCSUM_UDPRX_STORE: segment bytes [8, seg_len) at d_dst + dst_off and d_stored[i] (required)
 *     = seg_len - 8; without it d_stored[i] = 0 and d_dst is not written.
 * The UDP length field is summed and not consulted: UdpInput parses with initPartial(
 * LEVEL_HANDLED_FIELDS), whose data is bytes.sub(8, bytes.length() - 8) of the IP-truncated buffer
 * (UdpPacket.java:30-38); only the full from() compares the field.  L2 padding after l3_len is neither
 * read, summed nor stored.  No byte outside [dst_off, dst_off + stored) is written.  A record is
 * refused -- d_stored[i] 0, d_out[i] 0, S_BAD_DESC, not one byte written to d_dst, nothing of the
 * arena read -- when l4_proto != 17; l3_ver is not 4 / 6; the descriptor lacks F_L4 or carries F_L4P,
 * F_RAW or F_PRE; F_IP on IPv6; l4_off > l3_len, or an l4_off vpcsum_compute_async refuses (IPv4:
 * below 20 or not a multiple of 4; IPv6: below 40); l3_off + l3_len > arena_len (checked without
 * wrapping); seg_len < 8; ops & ~VPCSUM_UDPRX_STORE or rsv != 0; with STORE, seg_len - 8 > dst_cap or
 * dst_off + stored > dst_len (without wrapping).  seg_len == 8 is legal and stores 0 bytes.
 * Alignment, the limit on n, n == 0 and the no-overlap rule are vpcsum_tcp_recv_async's. */
int vpcsum_udp_recv_async(const uint8_t* d_arena, uint64_t arena_len, const vpcsum_desc_t* d_desc,
                          const vpcsum_udprx_t* d_rx, uint32_t n, uint8_t* d_dst, uint64_t dst_len,
                          uint32_t* d_stored, uint32_t* d_out, uint8_t* d_status, void* stream);

/* ICMP replies (additive, the ABI version stays 4): the packets the switch generates itself in answer
 * to a frame the fast path hands back -- the echo reply to a ping of one of its synthetic IPs, port
 * unreachable for a datagram without a listener, time exceeded for a packet whose TTL / hop limit
 * would expire (VPCSUM_S_TTL_EXPIRED).  All three end in SwitchUtils.buildEtherIpIcmpPacket
 * (SwitchUtils.java:202-241); each reply frame is byte-equal to getRawPacket(0) of what it builds.
 * The source is named by a parse descriptor over the RX arena, as in the receives; the headers are
 * generated from a 64-byte template, as in the builds; the request's bytes are read once and written
 * once, summed on the way. */
#define VPCSUM_ICMP_ECHO_REPLY    1u  /* IcmpInput.respondIcmpPong, IcmpInput.java:100-131            */
#define VPCSUM_ICMP_PORT_UNREACH  2u  /* IcmpPortUnreachableOutput.handle, :34-78 (from UdpInput :47-50) */
#define VPCSUM_ICMP_TIME_EXCEEDED 3u  /* IPInputRoute.respondIcmpTimeExceeded, IPInputRoute.java:222-263 */

/* The template carries everything the host decides; the kernel derives no address from the frame.
 * eth_dst / eth_src: Java's pkb.pkt.getSrc() and the looked-up MAC (or what ip-output-route would
 * make of them); l2_len 14 or 0; l3_ver; dst: the request's source; src: the request's destination
 * (echo, port unreachable) or the IP getRoutedSrcIpAndMac picks (time exceeded) -- the host has the
 * request's addresses from the parse's vpcsum_tuple_t; tos / ttl / ident / frag: the reference uses
 * 0 / 64 / 0 / 0. */
typedef vpcsum_tcphdr_t vpcsum_icmphdr_t;   /* bytes 48..57 (ports, ack, window) and rsv must be 0 */

typedef struct vpcsum_icmprp {   /* one per descriptor; 24 bytes, 8-byte aligned */
    uint64_t frame_off;   /* where the reply starts in the destination arena, any alignment */
    uint32_t hdr;         /* index into the template array */
    uint32_t frame_cap;   /* room at frame_off */
    uint8_t  kind;        /* VPCSUM_ICMP_* */
    uint8_t  rsv[7];      /* must be 0 */
} vpcsum_icmprp_t;

/* Descriptor i (as vpcsum_parse_ether_async writes them) pairs with record i.  With seg_len = l3_len -
 * l4_off and M the ICMP message length, the reply frame of length L = l2_len + (20 | 40) + M at
 * d_dst + frame_off:
 *   Ethernet and IP header: exactly as vpcsum_udp_build_async writes them -- IPv4: IHL 5, protocol 1,
 *     totalLength 20 + M; IPv6: no extension headers, next header 58, payloadLength M.  The reply never
 *     carries the request's IP options or extension headers.
 *   Echo reply, M = seg_len: type (0 for IPv4, 129 for IPv6), CODE 0 WHATEVER THE REQUEST'S CODE WAS
 *     (icmp.setCode(0)), the sum, then request segment bytes [4, seg_len) (inIcmp.getOther()).
 *   Port unreachable (type 3 code 3, or type 1 code 4) and time exceeded (type 11 or 3, code 0),
 *     M = 8 + q: type, code, the sum, four zero bytes, then the first q = min(l3_len, l4_off + 64)
 *     bytes of the IP packet as it lies in the arena (headerLen + 64, headerLen being the rebuilt
 *     header: IHL * 4 with options, or 40 + extension headers, which is l4_off).  The quoted bytes
 *     include the TTL as received.
 *   The ICMP sum: Utils.calculateChecksum over the message with a zero field; ICMPv6 puts the
 *     pseudo-header of the TEMPLATE's addresses in front.  A computed 0x0000 is stored as it is; a
 *     message that is all zero stores 0xffff.
 * A record that is not refused gets d_frame_len[i] = L (required); d_csum[i] (may be NULL) = the
 * reply's IPv4 header sum in bits 0..15 (0 for IPv6) and its ICMP field in bits 16..31; d_out[i] /
 * d_status[i] (each may be NULL): for an echo reply exactly what vpcsum_compute_async writes for the
 * descriptor under VPCSUM_MODE_VERIFY -- THE CALL REPLACES THE VERIFY OF THOSE FRAMES, and the reply
 * is written whatever the verdict, as in the receives: the caller posts the TX descriptor only on the
 * verdict its csum-recalc policy accepts --; for the two error kinds 0 and S_DONE.
 * A record is refused -- d_frame_len[i] 0, d_csum[i] 0, d_out[i] 0, S_BAD_DESC, not one byte written
 * to d_dst, nothing of the arena read except the one type byte where the rule needs it -- when
 * hdr >= n_hdr; the template is one vpcsum_udp_build_async refuses or its bytes 48..51 are not 0; its
 * l3_ver is not the descriptor's; kind is not 1..3; rsv != 0; the descriptor carries F_L4P, F_RAW or
 * F_PRE, or F_IP on IPv6; l4_off > l3_len, or an l4_off vpcsum_compute_async refuses (IPv4: below 20
 * or not a multiple of 4; IPv6: below 40); l3_off + l3_len > arena_len (checked without wrapping);
 * L > frame_cap, or frame_off + L > dst_len (without wrapping); echo: no F_L4, l4_proto not 1 on IPv4
 * or not 58 on IPv6 (Java drops ICMP of the other family), seg_len < 8, request type not 8 / 128;
 * port unreachable: l4_proto != 17; time exceeded: an ICMPv6 segment of at least one byte whose type
 * is 135 or 136 (IPInputRoute.java:64-75 drops NS / NA before the hop check).  Refused means "Java
 * drops it or the host handles it".
 * The caller's rules, not checked: error replies go only to frames whose full parse accepted them
 * (Java runs ensurePartialPacketParsed() first and sends nothing otherwise); reply frames overlap
 * neither each other nor any request of the batch.  Source and destination may be the same
 * allocation: an XDP umem holds both rings' chunks.
 * Alignment (templates, d_frame_len, d_csum and d_out 4-byte, descriptors and records 8-byte), the
 * limit n <= 2^28 and n == 0 are vpcsum_udp_recv_async's. */
int vpcsum_icmp_reply_async(const uint8_t* d_arena, uint64_t arena_len, const vpcsum_desc_t* d_desc,
                            const vpcsum_icmphdr_t* d_hdr, uint32_t n_hdr, const vpcsum_icmprp_t* d_rp, uint32_t n,
                            uint8_t* d_dst, uint64_t dst_len, uint32_t* d_frame_len,
                            uint32_t* d_csum, uint32_t* d_out, uint8_t* d_status, void* stream);

/* Streaming-read ceiling probe: reads `bytes` from d_buf with 16-B lanes, writes one word per
 * block into d_sink.  Used by bench.py to report a measured HBM read roof next to 8 TB/s. */
int vpcsum_read_probe_async(const uint8_t* d_buf, uint64_t bytes, uint32_t* d_sink,
                            uint32_t grid, void* stream);

/* Pattern read ceiling: reads exactly the 16-B chunks the checksum kernel reads for each
 * descriptor's L3 range (teams of 8 lanes, non-temporal), with no checksum work, and writes
 * one word per block into d_sink[0..1023].  grid 0 = 8 blocks per CU; grid bit 31 set = walk the
 * packets in the checksum kernel's unit order instead of grid-consecutively.  Arenas < 4 GiB.
 * Tooling: prices a workload's frame layout. */
int vpcsum_pattern_probe_async(const uint8_t* d_arena, uint64_t arena_len, const vpcsum_desc_t* d_desc,
                               uint32_t n, uint32_t* d_sink, uint32_t grid, void* stream);

/* NAT pattern ceiling: the memory operations of vpcsum_nat4_async (RFC 1624, wide kernel) for a
 * rewrite of both addresses and both ports -- descriptor and entry reads, the header window loads,
 * the one contiguous store of [L3+10, end of the L4 checksum field) -- with no rewrite: every byte
 * is stored back unchanged.  Tooling: prices BASELINE config C5's access pattern. */
int vpcsum_nat4_pattern_probe_async(uint8_t* d_arena, uint64_t arena_len, const vpcsum_desc_t* d_desc,
                                    const vpcsum_nat4_t* d_rw, uint32_t n, void* stream);
/* The same over records (vpcsum_nat4r_async's memory operations with no rewrite). */
int vpcsum_nat4r_pattern_probe_async(uint8_t* d_arena, uint64_t arena_len, const vpcsum_nat4_rec_t* d_rec,
                                     uint32_t n, void* stream);

/* Synthetic workload generator (bench / tests): deterministic counter-based splitmix64 bytes,
 * identical to oracle/csum_oracle.c:orc_synth_frame.  workload: see VPCSUM_SYNTH_*.  d_arena NULL
 * (with d_desc set): the descriptors alone, e.g. the lengths a rank needs to cut one global batch
 * into byte-balanced shards before it generates only its own. */
#define VPCSUM_SYNTH_C1_UDP64     1  /* IPv4/UDP L3 50 B                     */
#define VPCSUM_SYNTH_C2_TCP1500   2  /* IPv4/TCP L3 1500 B                   */
#define VPCSUM_SYNTH_C3_MIXED     3  /* IPv4 {64,576,1500} x {UDP,TCP,ICMP}  */
#define VPCSUM_SYNTH_C4_V6JUMBO   4  /* IPv6/TCP L3 9000 B                   */
#define VPCSUM_SYNTH_FUZZ         5  /* v4/v6, options, odd lengths, all protos */
#define VPCSUM_SYNTH_C5_NAT1500   6  /* IPv4 L3 1500 B, TCP or UDP (50/50): NAT input */
int vpcsum_synth_async(uint8_t* d_arena, uint64_t arena_len, uint32_t n, uint32_t stride,
                       uint32_t l3_pad, uint32_t workload, uint64_t seed, uint64_t first_index,
                       vpcsum_desc_t* d_desc, void* stream);

/* Tooling: a grid of `workgroups` x `threads` (a multiple of 64) that stays resident for `micros`
 * doing nothing but s_sleep -- no memory traffic.  The control of the A/B that asks whether a
 * resident kernel on another queue, as such, slows launched batches. */
int vpcsum_spin_probe_async(uint32_t workgroups, uint32_t threads, uint32_t micros, void* stream);

/* Kernel timing on the caller's stream (HIP events). */
int vpcsum_event_create(void** ev);
int vpcsum_event_destroy(void* ev);
int vpcsum_event_record(void* ev, void* stream);
int vpcsum_event_elapsed_ms(void* start, void* end, float* ms);
int vpcsum_stream_sync(void* stream);

/* ------------------------------------------------------------------------ */
/* Host-memory API (what the Java side drives): host arena + descriptors,   */
/* library-owned device buffers, pinned staging, async submit / wait.        */
/* ------------------------------------------------------------------------ */
typedef struct vpcsum_ctx vpcsum_ctx_t;

int vpcsum_ctx_create(int device, uint64_t max_arena_bytes, uint32_t max_pkts, vpcsum_ctx_t** out);
int vpcsum_ctx_destroy(vpcsum_ctx_t* ctx);
/* Page-lock a long-lived host arena (e.g. an AF_XDP umem, UMem.java:36-44) once, so that
 * submits from it DMA directly without a staging copy. */
int vpcsum_ctx_register_arena(vpcsum_ctx_t* ctx, void* h_arena, uint64_t len);
int vpcsum_ctx_unregister_arena(vpcsum_ctx_t* ctx, void* h_arena);
/* Copy the frames the descriptors touch to the device, run the batch, copy results back
 * (and, with VPCSUM_MODE_WRITE, the checksum fields back into the host frames).
 * Returns a ticket; results are valid after vpcsum_ctx_wait(ticket). */
int vpcsum_ctx_submit(vpcsum_ctx_t* ctx, uint8_t* h_arena, uint64_t arena_len,
                      const vpcsum_desc_t* h_desc, uint32_t n,
                      uint32_t* h_out, uint8_t* h_status, uint32_t mode, uint64_t* ticket);
int vpcsum_ctx_wait(vpcsum_ctx_t* ctx, uint64_t ticket);
/* Low-latency flushes (idle_us > 0): zero-copy batches of up to 512 frames from a registered arena
 * -- vpcsum_ctx_submit, vpcsum_ctx_submit_pre, vpcsum_ctx_egress_frames, vpcsum_ctx_verify_frames,
 * vpcsum_ctx_parse_frames -- are handed to a small persistent grid that polls a pinned mailbox,
 * instead of a kernel launch + event wait per batch (the Iface.completeTx flush of a few dozen
 * frames, XDPIface.java:227-243, and the RX poll).  Batches then run one at a time.  The grid leaves
 * after idle_us without a batch and is restarted by the next one; an idle grid costs launched batches
 * beside it nothing measurable (its pollers use relaxed loads), so larger batches,
 * which are launched, leave it resident.  idle_us = 0 stops it (the default).  Staged submits are
 * unaffected. */
int vpcsum_ctx_set_service(vpcsum_ctx_t* ctx, uint32_t idle_us);
/* Counters of a context: batches the service ran, service grids launched (either may be NULL). */
int vpcsum_ctx_stats(vpcsum_ctx_t* ctx, uint64_t* service_batches, uint64_t* service_launches);
/* Ingress verify of a received batch (XDPIface.readable, XDPIface.java:281-314): the raw Ethernet
 * frames at h_frame_off[i] (h_frame_len[i] bytes) of a registered arena are parsed on the GPU with
 * the rules of EthernetPacket/Ipv4Packet/Ipv6Packet.from (as vpcsum_parse_ether_async) and
 * verified (VPCSUM_MODE_VERIFY) where they lie, in one submission.  h_status[i]: S_DONE |
 * S_IP_OK | S_L4_OK | S_UDP_NOCSUM, or S_BAD_DESC for a frame that does not parse; h_out (may
 * be NULL): the sums the frames should carry.  Returns a ticket for vpcsum_ctx_wait. */
int vpcsum_ctx_verify_frames(vpcsum_ctx_t* ctx, const uint8_t* h_arena, uint64_t arena_len,
                             const uint64_t* h_frame_off, const uint32_t* h_frame_len, uint32_t n,
                             uint32_t* h_out, uint8_t* h_status, uint64_t* ticket);
/* vpcsum_ctx_verify_frames that also records every frame's ingress header sum in h_hsum (n
 * vpcsum_hsum_t, valid at vpcsum_ctx_wait): what the egress flush of the frame needs for a
 * VPCSUM_PRE_HSUM pre-image after the vswitch's in-place setters ran. */
int vpcsum_ctx_verify_frames_hsum(vpcsum_ctx_t* ctx, const uint8_t* h_arena, uint64_t arena_len,
                                  const uint64_t* h_frame_off, const uint32_t* h_frame_len, uint32_t n,
                                  uint32_t* h_out, uint8_t* h_status, vpcsum_hsum_t* h_hsum, uint64_t* ticket);
/* Batched parse of a received batch with flow tuples (the conntrack key TcpInput / UdpInput read,
 * TcpInput.java:47-51, UdpInput.java:45-47): the frames of a registered arena, as for
 * vpcsum_ctx_verify_frames, are parsed on the GPU where they lie; at vpcsum_ctx_wait h_desc[i]
 * holds frame i's descriptor (l3_off relative to h_arena, flags F_IP | F_L4 as the frame allows),
 * h_status[i] 0 or S_BAD_DESC, h_tuples[i] its vpcsum_tuple_t (any of the three may be NULL).
 * The descriptors can go straight to vpcsum_ctx_submit / vpcsum_ctx_nat_submit. */
int vpcsum_ctx_parse_frames(vpcsum_ctx_t* ctx, const uint8_t* h_arena, uint64_t arena_len,
                            const uint64_t* h_frame_off, const uint32_t* h_frame_len, uint32_t n,
                            vpcsum_desc_t* h_desc, uint8_t* h_status, vpcsum_tuple_t* h_tuples,
                            uint64_t* ticket);
/* Egress flush straight from the frames (the alternative to building descriptors on the host): the
 * frames at h_frame_off[i] (h_frame_len[i] bytes) of a registered arena, as the TX ring sends them
 * (XDPIface.sendPacket: chunk.getAddr() + pkb.pktOff and pkb.pktBuf.length(), or the copy's
 * pktaddr), each with the VPCSUM_F_* sums it needs (h_frame_flags[i]: F_IP / F_L4 / F_L4P, the
 * mapping of SwitchUtils.checksumFlagsFor, SwitchUtils.java:297-316).  The GPU parses every frame
 * with the vswitch's rules (as vpcsum_parse_ether_async: L3 after the Ethernet / 802.1Q header,
 * lengths from totalLength / payloadLength, L4 after IHL / the extension header), so padding,
 * options and extension headers are placed as Java's recompute places them, and writes the sums
 * into the frames (MODE_WRITE), in one submission.  At vpcsum_ctx_wait h_status[i] is S_DONE, or
 * S_BAD_DESC (nothing written) for a frame the parser refuses or whose flags it cannot honour (an
 * IPv4 header sum on IPv6, an L4 sum its segment cannot hold, F_L4P for ICMPv4): hand such a frame
 * back to the native path.  h_out (may be NULL): the sums, as vpcsum_ctx_submit. */
int vpcsum_ctx_egress_frames(vpcsum_ctx_t* ctx, uint8_t* h_arena, uint64_t arena_len,
                             const uint64_t* h_frame_off, const uint32_t* h_frame_len,
                             const uint8_t* h_frame_flags, uint32_t n,
                             uint32_t* h_out, uint8_t* h_status, uint64_t* ticket);
/* NAT / TTL rewrites of host frames (SwitchUtils.applyNat for a batch): h_rw[i] rewrites the
 * packet of h_desc[i] in place in the caller's frames, with the checksums updated as Java's
 * recompute leaves them (nat_mode as vpcsum_nat_async).  Frames in a registered arena are
 * rewritten where they lie (zero-copy); others are staged to the device and their rewritten
 * header bytes (L3 header through the L4 checksum field; with VPCSUM_NAT_TCP_REWRITES the TCP
 * header too) copied back at vpcsum_ctx_wait.
 * h_status (may be NULL, but not with VPCSUM_NAT_TCP_REWRITES: S_MSS_ABSENT is the caller's to
 * act on): S_DONE / S_BAD_DESC per packet.  Frames of one batch must not overlap. */
int vpcsum_ctx_nat_submit(vpcsum_ctx_t* ctx, uint8_t* h_arena, uint64_t arena_len,
                          const vpcsum_desc_t* h_desc, const vpcsum_nat_t* h_rw, uint32_t n,
                          uint8_t* h_status, uint32_t nat_mode, uint64_t* ticket);
/* The NAT fast path of a received batch in one submission: the frames at h_frame_off[i]
 * (h_frame_len[i] bytes) of a REGISTERED arena are parsed (vpcsum_parse_ether_tuples_async's rules),
 * looked up in `tab` (vpcsum_flow_lookup_async) and rewritten in place with the entries found
 * (nat_mode as vpcsum_ctx_nat_submit, VPCSUM_NAT_TCP_REWRITES included); tuples, entries and
 * descriptors never leave the device.  At vpcsum_ctx_wait h_verdict[i] is VPCSUM_FLOW_* and
 * h_status[i] S_DONE, or S_BAD_DESC (+ S_TTL_EXPIRED) for a frame the parse or the rewrite refuses,
 * S_MSS_ABSENT next to S_DONE as vpcsum_nat_async sets it.  A frame with verdict MISS / PUNT or
 * status S_BAD_DESC is left as it was: it takes the host's path.  An unregistered arena is refused
 * (the frames' extents are unknown before the parse); the batch is launched also when the service
 * grid is on.  tab must live on the context's device; a HIT marks its flow as vpcsum_flow_lookup_async
 * does (the context's stream: call vpcsum_ctx_wait before vpcsum_flowtab_collect). */
int vpcsum_ctx_nat_flow_frames(vpcsum_ctx_t* ctx, vpcsum_flowtab_t* tab, uint8_t* h_arena, uint64_t arena_len,
                               const uint64_t* h_frame_off, const uint32_t* h_frame_len, uint32_t n,
                               uint8_t* h_status, uint8_t* h_verdict, uint32_t nat_mode, uint64_t* ticket);
/* vpcsum_ctx_nat_flow_frames that also forwards: the lookup fetches each flow's Fastpath
 * (vpcsum_flow_lookup_fp_async) and, after the rewrite, vpcsum_l2_forward_async's rule writes the
 * two Ethernet addresses into each HIT frame that was rewritten (S_DONE, not S_BAD_DESC) and whose
 * flow has a Fastpath.  At vpcsum_ctx_wait h_port[i] (required when n > 0) is that flow's port --
 * the frame is ready for that port's TX ring -- or 0: the frame's Ethernet header is as received
 * and it takes the path it takes after vpcsum_ctx_nat_flow_frames.  Verdicts, status, rewritten
 * bytes, marks, refusals and the launch whatever the batch size are vpcsum_ctx_nat_flow_frames'. */
int vpcsum_ctx_nat_flow_forward_frames(vpcsum_ctx_t* ctx, vpcsum_flowtab_t* tab, uint8_t* h_arena, uint64_t arena_len,
                                       const uint64_t* h_frame_off, const uint32_t* h_frame_len, uint32_t n,
                                       uint8_t* h_status, uint8_t* h_verdict, uint32_t* h_port, uint32_t nat_mode,
                                       uint64_t* ticket);
/* vpcsum_tcp_build_async from host memory, in one submission: the frames are written where they lie
 * in h_dst, which must be inside a REGISTERED arena (the TX umem; an unregistered destination is
 * refused, like vpcsum_ctx_nat_flow_frames).  A registered h_src is read in place; any other is staged:
 * the span [min data_off, max data_off + data_len) over the batch's records with a payload inside
 * src_len goes to the device in one copy (refused if larger than the context's max_arena_bytes) and
 * the kernel reads that copy, data_off rebased in the library's own copy of the records -- the
 * caller's array is not written.  n and n_hdr are each at most the context's max_pkts.  At
 * vpcsum_ctx_wait h_frame_len[i] (required), h_out[i] and h_status[i] (each may be NULL) hold what
 * vpcsum_tcp_build_async writes.  The batch is always launched: there is no service-grid,
 * device-group or process-wide form. */
int vpcsum_ctx_build_tcp_frames(vpcsum_ctx_t* ctx, uint8_t* h_dst, uint64_t dst_len, const uint8_t* h_src, uint64_t src_len,
                                const vpcsum_tcphdr_t* h_hdr, uint32_t n_hdr, const vpcsum_tcpseg_t* h_seg, uint32_t n,
                                uint32_t* h_frame_len, uint32_t* h_out, uint8_t* h_status, uint64_t* ticket);
/* vpcsum_tcp_build_bursts_async from host memory, in one submission: vpcsum_ctx_build_tcp_frames'
 * rules with bursts for records.  h_dst must be inside a REGISTERED arena; a registered h_src is read
 * in place; any other is staged: the span [min data_off, max data_off + data_len) over the bursts
 * with a payload inside src_len goes to the device in one copy (refused if larger than the context's
 * max_arena_bytes), data_off rebased in the library's own copy of the bursts -- the caller's arrays
 * are not written.  n_frames, n_bursts and n_hdr are each at most the context's max_pkts.  At
 * vpcsum_ctx_wait h_frame_len[j] (required), h_out[j] and h_status[j] (each may be NULL) hold what
 * vpcsum_tcp_build_bursts_async writes.  Always launched: no service-grid, device-group or
 * process-wide form. */
int vpcsum_ctx_build_tcp_bursts(vpcsum_ctx_t* ctx, uint8_t* h_dst, uint64_t dst_len, const uint8_t* h_src, uint64_t src_len,
                                const vpcsum_tcphdr_t* h_hdr, uint32_t n_hdr, const vpcsum_tcpburst_t* h_burst,
                                uint32_t n_bursts, const uint64_t* h_frame_off, uint32_t n_frames, uint32_t frame_cap,
                                uint32_t* h_frame_len, uint32_t* h_out, uint8_t* h_status, uint64_t* ticket);
/* vpcsum_tcp_recv_async from host memory, in one submission: the payloads are written where they lie
 * in h_dst, through its mapping, so h_dst must be inside a REGISTERED arena (the connections'
 * receive buffers; an unregistered destination is refused, as in vpcsum_ctx_build_tcp_frames).  A
 * registered h_arena (the RX umem) is read in place; any other is staged exactly as
 * vpcsum_ctx_submit stages it (the descriptors' span, or their gathered 16-byte blocks, refused when
 * larger than the context's max_arena_bytes), the descriptors rebased in the library's own copy.  n
 * is at most the context's max_pkts.  At vpcsum_ctx_wait h_stored[i] (required), h_out[i] and
 * h_status[i] (each may be NULL) hold what vpcsum_tcp_recv_async writes, and the payloads are in
 * h_dst -- whatever the verdict: see vpcsum_tcp_recv_async.  The batch is always launched: there is
 * no service-grid, device-group or process-wide form. */
int vpcsum_ctx_recv_tcp_frames(vpcsum_ctx_t* ctx, const uint8_t* h_arena, uint64_t arena_len,
                               const vpcsum_desc_t* h_desc, const vpcsum_tcprx_t* h_rx, uint32_t n,
                               uint8_t* h_dst, uint64_t dst_len, uint32_t* h_stored, uint32_t* h_out,
                               uint8_t* h_status, uint64_t* ticket);
/* vpcsum_udp_build_async from host memory, in one submission, by vpcsum_ctx_build_tcp_frames' plan:
 * h_dst must be inside a REGISTERED arena (an unregistered destination is refused); a registered
 * h_src is read in place, any other is staged as the one span of the batch's payloads (refused if
 * larger than the context's max_arena_bytes), data_off rebased in the library's own copy of the
 * records.  n and n_hdr are each at most the context's max_pkts.  At vpcsum_ctx_wait h_frame_len[i]
 * (required), h_out[i] and h_status[i] (each may be NULL) hold what vpcsum_udp_build_async writes.
 * Always launched: no service-grid, device-group or process-wide form. */
int vpcsum_ctx_build_udp_frames(vpcsum_ctx_t* ctx, uint8_t* h_dst, uint64_t dst_len, const uint8_t* h_src, uint64_t src_len,
                                const vpcsum_udphdr_t* h_hdr, uint32_t n_hdr, const vpcsum_udpdg_t* h_dg, uint32_t n,
                                uint32_t* h_frame_len, uint32_t* h_out, uint8_t* h_status, uint64_t* ticket);
/* vpcsum_udp_recv_async from host memory, in one submission, by vpcsum_ctx_recv_tcp_frames' plan:
 * h_dst must be inside a REGISTERED arena (an unregistered destination is refused); a registered
 * h_arena (the RX umem) is read in place, any other is staged exactly as vpcsum_ctx_submit stages
 * it.  n is at most the context's max_pkts.  At vpcsum_ctx_wait h_stored[i] (required), h_out[i] and
 * h_status[i] (each may be NULL) hold what vpcsum_udp_recv_async writes, and the data bytes are in
 * h_dst whatever the verdict.  Always launched: no service-grid, device-group or process-wide form. */
int vpcsum_ctx_recv_udp_frames(vpcsum_ctx_t* ctx, const uint8_t* h_arena, uint64_t arena_len,
                               const vpcsum_desc_t* h_desc, const vpcsum_udprx_t* h_rx, uint32_t n,
                               uint8_t* h_dst, uint64_t dst_len, uint32_t* h_stored, uint32_t* h_out,
                               uint8_t* h_status, uint64_t* ticket);
/* vpcsum_icmp_reply_async from host memory, in one submission: the source by
 * vpcsum_ctx_recv_udp_frames' plan -- a registered h_arena (the RX umem) is read in place, any other
 * is staged exactly as vpcsum_ctx_submit stages it --, the destination by
 * vpcsum_ctx_build_udp_frames' -- h_dst must be inside a REGISTERED arena (an unregistered
 * destination is refused); it may be the arena h_arena lies in.  n and n_hdr are each at most the
 * context's max_pkts.  At vpcsum_ctx_wait h_frame_len[i] (required), h_csum[i], h_out[i] and
 * h_status[i] (each may be NULL) hold what vpcsum_icmp_reply_async writes, and the replies are in
 * h_dst whatever an echo's verdict.  Always launched: no service-grid, device-group or process-wide
 * form. */
int vpcsum_ctx_reply_icmp_frames(vpcsum_ctx_t* ctx, const uint8_t* h_arena, uint64_t arena_len,
                                 const vpcsum_desc_t* h_desc, const vpcsum_icmphdr_t* h_hdr, uint32_t n_hdr,
                                 const vpcsum_icmprp_t* h_rp, uint32_t n, uint8_t* h_dst, uint64_t dst_len,
                                 uint32_t* h_frame_len, uint32_t* h_csum, uint32_t* h_out, uint8_t* h_status,
                                 uint64_t* ticket);
/* The egress flush of a batch holding NAT'd frames: vpcsum_ctx_submit where
 * descriptors with VPCSUM_F_PRE take their L4 sum from h_pre[i] (pre_fmt as vpcsum_pre_async;
 * entries of other descriptors are ignored) and the others are summed in full, in one submission.
 * Frames of a registered arena are read and written in place (an F_PRE packet: its header only);
 * others are staged, an F_PRE packet's header only (its whole segment when it is UDP with a stored
 * 0).  mode: VPCSUM_MODE_COMPUTE / VPCSUM_MODE_WRITE (not VERIFY).  A batch of up to 512 packets
 * from a registered arena goes to the low-latency service grid when it is on
 * (vpcsum_ctx_set_service), F_PRE frames and the others together; larger ones are launched.  The
 * entries' rsv bytes are ignored. */
int vpcsum_ctx_submit_pre(vpcsum_ctx_t* ctx, uint8_t* h_arena, uint64_t arena_len, const vpcsum_desc_t* h_desc,
                          const void* h_pre, uint32_t pre_fmt, uint32_t n, uint32_t* h_out, uint8_t* h_status,
                          uint32_t mode, uint64_t* ticket);
/* Pipelined host->device->host throughput helper: processes a host arena of n fixed-stride
 * frames in `chunks` double-buffered pieces over two streams (H2D || kernel || D2H).  The arena,
 * descriptors and h_out must be registered (page-locked); with VPCSUM_MODE_WRITE the checksum
 * fields are also stored into the host frames (through the arena's mapping). */
int vpcsum_ctx_pipeline(vpcsum_ctx_t* ctx, uint8_t* h_arena, uint32_t stride, uint32_t copy_bytes,
                        const vpcsum_desc_t* h_desc, uint32_t n, uint32_t* h_out,
                        uint32_t mode, uint32_t chunks);

/* ------------------------------------------------------------------------ */
/* Device groups (multi-GPU host batches): one context per GPU in dev_mask;  */
/* a submitted batch is cut into contiguous descriptor ranges of nearly      */
/* equal byte totals (prefix sum of l3_len), one per GPU, each processed by  */
/* its own context; wait joins them.  No data crosses devices.               */
/* ------------------------------------------------------------------------ */
typedef struct vpcsum_group vpcsum_group_t;
int vpcsum_group_create(uint64_t dev_mask, uint64_t max_arena_bytes, uint32_t max_pkts, vpcsum_group_t** out);
/* devices[0..ndev): a device may repeat (several contexts on one GPU) */
int vpcsum_group_create_list(const int* devices, int ndev, uint64_t max_arena_bytes, uint32_t max_pkts,
                             vpcsum_group_t** out);
int vpcsum_group_destroy(vpcsum_group_t* g);
/* page-lock once (portable: every GPU of the group maps it) */
int vpcsum_group_register_arena(vpcsum_group_t* g, void* h_arena, uint64_t len);
/* finish every zero-copy batch still reading the arena on each device, then unpin it */
int vpcsum_group_unregister_arena(vpcsum_group_t* g, void* h_arena);
/* as vpcsum_ctx_submit, capacity per GPU; h_out / h_status hold all n results in batch order */
int vpcsum_group_submit(vpcsum_group_t* g, uint8_t* h_arena, uint64_t arena_len, const vpcsum_desc_t* h_desc,
                        uint32_t n, uint32_t* h_out, uint8_t* h_status, uint32_t mode, uint64_t* ticket);
int vpcsum_group_wait(vpcsum_group_t* g, uint64_t ticket);
/* as vpcsum_ctx_nat_submit, cut over the group's devices like vpcsum_group_submit; h_rw[i]
 * rewrites the packet of h_desc[i]; the ticket is joined by vpcsum_group_wait */
int vpcsum_group_nat_submit(vpcsum_group_t* g, uint8_t* h_arena, uint64_t arena_len, const vpcsum_desc_t* h_desc,
                            const vpcsum_nat_t* h_rw, uint32_t n, uint8_t* h_status, uint32_t nat_mode,
                            uint64_t* ticket);
/* as vpcsum_ctx_submit_pre, cut over the group's devices like vpcsum_group_submit */
int vpcsum_group_submit_pre(vpcsum_group_t* g, uint8_t* h_arena, uint64_t arena_len, const vpcsum_desc_t* h_desc,
                            const void* h_pre, uint32_t pre_fmt, uint32_t n, uint32_t* h_out, uint8_t* h_status,
                            uint32_t mode, uint64_t* ticket);

/* ------------------------------------------------------------------------ */
/* SURVEY.md §8(b)'s entry points: the same over ONE process-wide group.     */
/* vpcsum_init(dev_mask) creates it (error if one exists), vpcsum_shutdown   */
/* destroys it; the others fail with "vpcsum_init first" before it.  The     */
/* handle of a submit is waited on with vpcsum_batch_wait (checksum and NAT  */
/* batches alike).  vpcsum_shutdown first completes every batch still in     */
/* flight (results delivered into the callers' buffers); a handle issued     */
/* before it is then refused by vpcsum_batch_wait ("before vpcsum_shutdown"),*/
/* also after a new vpcsum_init.                                             */
/* ------------------------------------------------------------------------ */
int vpcsum_init(uint64_t dev_mask, uint64_t max_arena_bytes, uint32_t max_pkts);
int vpcsum_shutdown(void);
int vpcsum_register_arena(void* h_arena, uint64_t len);
int vpcsum_batch_submit(uint8_t* h_arena, uint64_t arena_len, const vpcsum_desc_t* h_desc, uint32_t n,
                        uint32_t* h_out, uint8_t* h_status, uint32_t mode, uint64_t* handle);
int vpcsum_batch_submit_pre(uint8_t* h_arena, uint64_t arena_len, const vpcsum_desc_t* h_desc, const void* h_pre,
                            uint32_t pre_fmt, uint32_t n, uint32_t* h_out, uint8_t* h_status, uint32_t mode,
                            uint64_t* handle);
int vpcsum_nat_submit(uint8_t* h_arena, uint64_t arena_len, const vpcsum_desc_t* h_desc, const vpcsum_nat_t* h_rw,
                      uint32_t n, uint8_t* h_status, uint32_t nat_mode, uint64_t* handle);
int vpcsum_batch_wait(uint64_t handle);

/* ------------------------------------------------------------------------ */
/* PNI entry points (bound by io.vproxy.vpcsum.VPCsum)   */
/* Layout copied from the PNI convention, base/src/main/c-generated/pni.h   */
/* ------------------------------------------------------------------------ */
typedef struct PNIException_vpcsum {
    char*   type;
    char    message[4096];
    int32_t errno_;    /* EINVAL (IllegalArgumentException) / EIO (IOException) on a throw */
} PNIException_vpcsum;   /* sizeof 4112: message at 8, errno_ at 4104 (tests/cpp/pni_layout.c) */

typedef struct PNIEnv_vpcsum_long {
    PNIException_vpcsum ex;
    union { int64_t return_; struct { uint64_t a, b; } placeholder_; };
} PNIEnv_vpcsum_long;   /* sizeof 4128, return_ at 4112: PNIEnv_long of pni.h */

typedef struct PNIEnv_vpcsum_int {
    PNIException_vpcsum ex;
    union { int32_t return_; struct { uint64_t a, b; } placeholder_; };
} PNIEnv_vpcsum_int;

typedef struct PNIEnv_vpcsum_void {
    PNIException_vpcsum ex;
    struct { uint64_t a, b; } placeholder_;
} PNIEnv_vpcsum_void;

/* VPCsum.create(int device, long maxArena, int maxPkts) -> long ctx */
int Java_io_vproxy_vpcsum_VPCsum_create(PNIEnv_vpcsum_long* env, int32_t device, int64_t maxArena, int32_t maxPkts);
/* VPCsum.registerArena(long ctx, MemorySegment arena, long len) */
int Java_io_vproxy_vpcsum_VPCsum_registerArena(PNIEnv_vpcsum_void* env, int64_t ctx, void* arena, int64_t len);
/* VPCsum.submit(long ctx, MemorySegment arena, long arenaLen, MemorySegment desc, int n,
 *               MemorySegment out, MemorySegment status, int mode) -> long ticket */
int Java_io_vproxy_vpcsum_VPCsum_submit(PNIEnv_vpcsum_long* env, int64_t ctx, void* arena, int64_t arenaLen,
                                        void* desc, int32_t n, void* out, void* status, int32_t mode);
/* VPCsum.verifyFrames(long ctx, MemorySegment arena, long arenaLen, MemorySegment frameOff,
 *                     MemorySegment frameLen, int n, MemorySegment out, MemorySegment status) -> long ticket */
int Java_io_vproxy_vpcsum_VPCsum_verifyFrames(PNIEnv_vpcsum_long* env, int64_t ctx, void* arena, int64_t arenaLen,
                                              void* frameOff, void* frameLen, int32_t n, void* out, void* status);
/* VPCsum.verifyFramesHsum(long ctx, MemorySegment arena, long arenaLen, MemorySegment frameOff,
 *                         MemorySegment frameLen, int n, MemorySegment out, MemorySegment status,
 *                         MemorySegment hsum) -> long ticket (vpcsum_ctx_verify_frames_hsum) */
int Java_io_vproxy_vpcsum_VPCsum_verifyFramesHsum(PNIEnv_vpcsum_long* env, int64_t ctx, void* arena, int64_t arenaLen,
                                                  void* frameOff, void* frameLen, int32_t n, void* out, void* status,
                                                  void* hsum);
/* VPCsum.parseFrames(long ctx, MemorySegment arena, long arenaLen, MemorySegment frameOff,
 *                    MemorySegment frameLen, int n, MemorySegment desc, MemorySegment status,
 *                    MemorySegment tuples) -> long ticket */
int Java_io_vproxy_vpcsum_VPCsum_parseFrames(PNIEnv_vpcsum_long* env, int64_t ctx, void* arena, int64_t arenaLen,
                                             void* frameOff, void* frameLen, int32_t n, void* desc, void* status,
                                             void* tuples);
/* VPCsum.egressFrames(long ctx, MemorySegment arena, long arenaLen, MemorySegment frameOff,
 *                     MemorySegment frameLen, MemorySegment frameFlags, int n, MemorySegment out,
 *                     MemorySegment status) -> long ticket */
int Java_io_vproxy_vpcsum_VPCsum_egressFrames(PNIEnv_vpcsum_long* env, int64_t ctx, void* arena, int64_t arenaLen,
                                              void* frameOff, void* frameLen, void* frameFlags, int32_t n, void* out,
                                              void* status);
/* VPCsum.submitPre(long ctx, MemorySegment arena, long arenaLen, MemorySegment desc,
 *                  MemorySegment pre, int n, MemorySegment out, MemorySegment status, int mode)
 *   -> long ticket (vpcsum_ctx_submit_pre with 48-B vpcsum_pre_t entries) */
int Java_io_vproxy_vpcsum_VPCsum_submitPre(PNIEnv_vpcsum_long* env, int64_t ctx, void* arena, int64_t arenaLen,
                                           void* desc, void* pre, int32_t n, void* out, void* status, int32_t mode);
/* VPCsum.natSubmit(long ctx, MemorySegment arena, long arenaLen, MemorySegment desc,
 *                  MemorySegment rw, int n, MemorySegment status, int natMode) -> long ticket */
int Java_io_vproxy_vpcsum_VPCsum_natSubmit(PNIEnv_vpcsum_long* env, int64_t ctx, void* arena, int64_t arenaLen,
                                           void* desc, void* rw, int32_t n, void* status, int32_t natMode);
/* VPCsum.flowtabCreate(int device, int maxFlows) -> long tab */
int Java_io_vproxy_vpcsum_VPCsum_flowtabCreate(PNIEnv_vpcsum_long* env, int32_t device, int32_t maxFlows);
/* VPCsum.flowtabUpdate(long tab, MemorySegment del, int nDel, MemorySegment add, int nAdd): 40-B
 * vpcsum_tuple_t keys to erase, 96-B vpcsum_flow_t flows to insert / replace; returns when the
 * device table holds them (vpcsum_flowtab_update, stream NULL: a natFlowFrames batch still in flight
 * is not ordered against it -- waitFor it first; batches submitted afterwards see the new table) */
int Java_io_vproxy_vpcsum_VPCsum_flowtabUpdate(PNIEnv_vpcsum_void* env, int64_t tab, void* del, int32_t nDel, void* add,
                                               int32_t nAdd);
/* VPCsum.flowtabCollect(long tab, MemorySegment cookies, int cap) -> int count (vpcsum_flowtab_collect;
 * count > cap: nothing cleared) */
int Java_io_vproxy_vpcsum_VPCsum_flowtabCollect(PNIEnv_vpcsum_int* env, int64_t tab, void* cookies, int32_t cap);
/* VPCsum.flowtabClose(long tab) */
int Java_io_vproxy_vpcsum_VPCsum_flowtabClose(PNIEnv_vpcsum_void* env, int64_t tab);
/* VPCsum.natFlowFrames(long ctx, long tab, MemorySegment arena, long arenaLen, MemorySegment frameOff,
 *                      MemorySegment frameLen, int n, MemorySegment status, MemorySegment verdict,
 *                      int natMode) -> long ticket (vpcsum_ctx_nat_flow_frames) */
int Java_io_vproxy_vpcsum_VPCsum_natFlowFrames(PNIEnv_vpcsum_long* env, int64_t ctx, int64_t tab, void* arena,
                                               int64_t arenaLen, void* frameOff, void* frameLen, int32_t n, void* status,
                                               void* verdict, int32_t natMode);
/* VPCsum.flowtabSetFastpath(long tab, MemorySegment keys, MemorySegment fp, int n) -> int missing:
 * 40-B vpcsum_tuple_t keys and their 16-B vpcsum_fastpath_t records (vpcsum_flowtab_set_fastpath,
 * stream NULL, ordered as flowtabUpdate); the keys that were not in the table are counted */
int Java_io_vproxy_vpcsum_VPCsum_flowtabSetFastpath(PNIEnv_vpcsum_int* env, int64_t tab, void* keys, void* fp, int32_t n);
/* VPCsum.natFlowForwardFrames(long ctx, long tab, MemorySegment arena, long arenaLen, MemorySegment frameOff,
 *                             MemorySegment frameLen, int n, MemorySegment status, MemorySegment verdict,
 *                             MemorySegment port, int natMode) -> long ticket (vpcsum_ctx_nat_flow_forward_frames) */
int Java_io_vproxy_vpcsum_VPCsum_natFlowForwardFrames(PNIEnv_vpcsum_long* env, int64_t ctx, int64_t tab, void* arena,
                                                      int64_t arenaLen, void* frameOff, void* frameLen, int32_t n,
                                                      void* status, void* verdict, void* port, int32_t natMode);
/* VPCsum.buildTcpFrames(long ctx, MemorySegment dst, long dstLen, MemorySegment src, long srcLen,
 *                       MemorySegment hdr, int nHdr, MemorySegment seg, int n, MemorySegment frameLen,
 *                       MemorySegment out, MemorySegment status) -> long ticket (vpcsum_ctx_build_tcp_frames) */
int Java_io_vproxy_vpcsum_VPCsum_buildTcpFrames(PNIEnv_vpcsum_long* env, int64_t ctx, void* dst, int64_t dstLen, void* src,
                                                int64_t srcLen, void* hdr, int32_t nHdr, void* seg, int32_t n,
                                                void* frameLen, void* out, void* status);
/* VPCsum.buildTcpBursts(long ctx, MemorySegment dst, long dstLen, MemorySegment src, long srcLen,
 *                       MemorySegment hdr, int nHdr, MemorySegment burst, int nBursts, MemorySegment frameOff,
 *                       int nFrames, int frameCap, MemorySegment frameLen, MemorySegment out,
 *                       MemorySegment status) -> long ticket (vpcsum_ctx_build_tcp_bursts) */
int Java_io_vproxy_vpcsum_VPCsum_buildTcpBursts(PNIEnv_vpcsum_long* env, int64_t ctx, void* dst, int64_t dstLen, void* src,
                                                int64_t srcLen, void* hdr, int32_t nHdr, void* burst, int32_t nBursts,
                                                void* frameOff, int32_t nFrames, int32_t frameCap, void* frameLen,
                                                void* out, void* status);
/* VPCsum.recvTcpFrames(long ctx, MemorySegment arena, long arenaLen, MemorySegment desc, MemorySegment rx, int n,
 *                      MemorySegment dst, long dstLen, MemorySegment stored, MemorySegment out,
 *                      MemorySegment status) -> long ticket (vpcsum_ctx_recv_tcp_frames) */
int Java_io_vproxy_vpcsum_VPCsum_recvTcpFrames(PNIEnv_vpcsum_long* env, int64_t ctx, void* arena, int64_t arenaLen, void* desc,
                                               void* rx, int32_t n, void* dst, int64_t dstLen, void* stored, void* out,
                                               void* status);
/* VPCsum.buildUdpFrames(long ctx, MemorySegment dst, long dstLen, MemorySegment src, long srcLen,
 *                       MemorySegment hdr, int nHdr, MemorySegment dg, int n, MemorySegment frameLen,
 *                       MemorySegment out, MemorySegment status) -> long ticket (vpcsum_ctx_build_udp_frames) */
int Java_io_vproxy_vpcsum_VPCsum_buildUdpFrames(PNIEnv_vpcsum_long* env, int64_t ctx, void* dst, int64_t dstLen, void* src,
                                                int64_t srcLen, void* hdr, int32_t nHdr, void* dg, int32_t n,
                                                void* frameLen, void* out, void* status);
/* VPCsum.recvUdpFrames(long ctx, MemorySegment arena, long arenaLen, MemorySegment desc, MemorySegment rx, int n,
 *                      MemorySegment dst, long dstLen, MemorySegment stored, MemorySegment out,
 *                      MemorySegment status) -> long ticket (vpcsum_ctx_recv_udp_frames) */
int Java_io_vproxy_vpcsum_VPCsum_recvUdpFrames(PNIEnv_vpcsum_long* env, int64_t ctx, void* arena, int64_t arenaLen, void* desc,
                                               void* rx, int32_t n, void* dst, int64_t dstLen, void* stored, void* out,
                                               void* status);
/* VPCsum.replyIcmpFrames(long ctx, MemorySegment arena, long arenaLen, MemorySegment desc, MemorySegment hdr,
 *                        int nHdr, MemorySegment rp, int n, MemorySegment dst, long dstLen, MemorySegment frameLen,
 *                        MemorySegment csum, MemorySegment out, MemorySegment status)
 *   -> long ticket (vpcsum_ctx_reply_icmp_frames) */
int Java_io_vproxy_vpcsum_VPCsum_replyIcmpFrames(PNIEnv_vpcsum_long* env, int64_t ctx, void* arena, int64_t arenaLen, void* desc,
                                                 void* hdr, int32_t nHdr, void* rp, int32_t n, void* dst, int64_t dstLen,
                                                 void* frameLen, void* csum, void* out, void* status);
/* VPCsum.setService(long ctx, int idleUs) */
int Java_io_vproxy_vpcsum_VPCsum_setService(PNIEnv_vpcsum_void* env, int64_t ctx, int32_t idleUs);
/* VPCsum.waitFor(long ctx, long ticket) */
int Java_io_vproxy_vpcsum_VPCsum_waitFor(PNIEnv_vpcsum_void* env, int64_t ctx, int64_t ticket);
/* VPCsum.close(long ctx) */
int Java_io_vproxy_vpcsum_VPCsum_close(PNIEnv_vpcsum_void* env, int64_t ctx);

#ifdef __cplusplus
}
#endif
#endif /* VPCSUM_H */

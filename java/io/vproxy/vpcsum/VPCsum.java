package io.vproxy.vpcsum;

import io.vproxy.pni.PNIEnv;
import io.vproxy.pni.PNILinkOptions;
import io.vproxy.pni.PanamaUtils;

import java.lang.foreign.MemorySegment;
import java.lang.invoke.MethodHandle;

/**
 * Downcalls into libvpcsum.so (MI355X batched Internet checksum), written in the shape the PNI
 * generator emits for the existing natives (compare
 * base/src/main/generated/io/vproxy/vfd/posix/PosixNative.java:729-744 in vproxy): one
 * downcall per method, exceptions travel through the PNIEnv (0 = ok, -1 = exception stored in
 * ENV).  The C side is include/vpcsum.h, symbols Java_io_vproxy_vpcsum_VPCsum_*.
 *
 * No method is linked critical ({@code setCritical(false)} throughout): every entry point may
 * block -- create / registerArena allocate and page-lock through the HIP runtime, submit / submitPre /
 * natSubmit / verifyFrames / parseFrames finish the batch that last used their slot (an event wait, or the
 * service grid's completion), waitFor and setService wait by design.  A critical downcall keeps
 * the thread in Java state and would stall every safepoint (GC included) for that long.
 *
 * Load the library the same way vproxy loads its other natives:
 * {@code Utils.loadDynamicLibrary("vpcsum")} (base/src/main/java/io/vproxy/base/util/Utils.java:1014-1030).
 *
 * Not compiled in this repository (the build image has no JDK); see INTEGRATION.md.
 */
public class VPCsum {
    private VPCsum() {
    }

    private static final VPCsum INSTANCE = new VPCsum();

    public static VPCsum get() {
        return INSTANCE;
    }

    /** include/vpcsum.h VPCSUM_ABI_VERSION this binding was written against (4: the ingress header
     * sum, verifyFramesHsum and PRE_HSUM entries; 3: VPCSUM_F_PRE and submitPre; 2: NAT_DEC_TTL
     * refuses TTL <= 1 with S_TTL_EXPIRED).  {@link #abiVersion} reports the loaded library's. */
    public static final int ABI_VERSION = 4;

    /** vpcsum_abi_version() of the loaded library (a plain C function, no PNIEnv; {@link VPCsumLib}).
     * Throws an IOException when libvpcsum is not loaded. */
    public int abiVersion() throws java.io.IOException {
        return VPCsumLib.abiVersion();
    }

    // descriptor flags (include/vpcsum.h)
    public static final int F_IP = 0x01;
    public static final int F_L4 = 0x02;
    public static final int F_RAW = 0x04;
    /** checksum offload (VP_CSUM_UP_PSEUDO): L4 field = folded pseudo-header sum (CHECKSUM_PARTIAL) */
    public static final int F_L4P = 0x08;
    /** a received packet changed in place whose stored L4 sum was verified on ingress: its L4 sum
     * is updated from its pre-image entry by RFC 1624 -- only the header is read ({@link PreImage}) */
    public static final int F_PRE = 0x10;
    /** bytes of one vpcsum_pre_t pre-image entry (the vpcsum_nat_t layout) */
    public static final int PRE_ENTRY = 48;
    /** pre-image entry mask: the entry's first 8 bytes hold the frame's ingress header sum
     * (vpcsum_hsum_t, {@link #verifyFramesHsum}) */
    public static final int PRE_HSUM = 0x80;
    /** bytes of one vpcsum_hsum_t: sum(u16) l4Len(u16) hlen proto ver l2Len */
    public static final int HSUM_ENTRY = 8;
    // status bits
    public static final int S_IP_OK = 0x01;
    public static final int S_L4_OK = 0x02;
    public static final int S_UDP_NOCSUM = 0x04;
    public static final int S_DONE = 0x40;
    public static final int S_BAD_DESC = 0x80;
    /** NAT: a TTL / hop-limit decrement of a packet at TTL <= 1 is refused (with S_BAD_DESC);
     * IPInputRoute drops such packets and answers ICMP time exceeded (IPInputRoute.java:81-88). */
    public static final int S_TTL_EXPIRED = 0x20;
    // modes
    public static final int MODE_COMPUTE = 0x00;
    public static final int MODE_VERIFY = 0x01;
    public static final int MODE_WRITE = 0x10;
    // NAT / TTL rewrite masks (vpcsum_nat_t.mask) and modes
    public static final int NAT_SRC = 0x01;
    public static final int NAT_DST = 0x02;
    public static final int NAT_SPORT = 0x04;
    public static final int NAT_DPORT = 0x08;
    public static final int NAT_DEC_TTL = 0x10;
    public static final int NAT_SET_TTL = 0x20;
    public static final int NAT_RFC1624 = 0x00;
    public static final int NAT_STRICT_JAVA = 0x01;
    /** bytes of one vpcsum_nat_t rewrite entry: src[16] dst[16] sport[2] dport[2] mask ttl rsv[10] */
    public static final int NAT_ENTRY = 48;
    /** natMode bit: honour {@link #NAT_TCP} entries in this batch (a status segment is required).  A
     * library from before the feature throws "bad nat_mode": that refusal is the probe. */
    public static final int NAT_TCP_REWRITES = 0x02;
    /** vpcsum_nat_t.mask bit: rsv[0..7] hold TCP-header rewrites ({@link #natTcp}) -- what the
     * reference does to a NAT'd TCP packet besides applyNat: buildSynPacketForProxyProtocol
     * (SwitchUtils.java:461-465), buildSynAckPacketForProxyProtocol (:467-473), checkAndUpdateMss
     * (:46-95).  Ignored without {@link #NAT_TCP_REWRITES}. */
    public static final int NAT_TCP = 0x40;
    public static final int TCP_SEQ_ADD = 0x01;
    public static final int TCP_SET_FLAGS = 0x02;
    public static final int TCP_CLAMP_MSS = 0x04;
    /** NAT with NAT_TCP_REWRITES, next to S_DONE: TCP_CLAMP_MSS on a SYN whose options parse and hold
     * no MSS option.  The packet is otherwise done; add the option on the host (checkAndUpdateMss's
     * rebuild branch, SwitchUtils.java:83-94) and flush that frame in full. */
    public static final int S_MSS_ABSENT = 0x08;

    /** Fill the TCP part of the 48-byte entry at {@code rw[off..]}: {@code ops} TCP_*, {@code flags}
     * the new TCP flags (low 6 bits, TcpPacket.setFlags), {@code maxMss} the egress port's clamp,
     * {@code seqAdd} added to the sequence number mod 2^32 (seq - N: pass -N).  setSeqNum and setFlags
     * dirty the TCP sum whatever the value; the clamp only when it writes. */
    public static void natTcp(MemorySegment rw, long off, int ops, int flags, int maxMss, int seqAdd) {
        rw.set(java.lang.foreign.ValueLayout.JAVA_BYTE, off + 36,
            (byte) (rw.get(java.lang.foreign.ValueLayout.JAVA_BYTE, off + 36) | NAT_TCP));
        rw.set(java.lang.foreign.ValueLayout.JAVA_BYTE, off + 38, (byte) ops);
        rw.set(java.lang.foreign.ValueLayout.JAVA_BYTE, off + 39, (byte) (flags & 0x3f));
        rw.set(java.lang.foreign.ValueLayout.JAVA_BYTE, off + 40, (byte) (maxMss >> 8));
        rw.set(java.lang.foreign.ValueLayout.JAVA_BYTE, off + 41, (byte) maxMss);
        rw.set(java.lang.foreign.ValueLayout.JAVA_BYTE, off + 42, (byte) (seqAdd >> 24));
        rw.set(java.lang.foreign.ValueLayout.JAVA_BYTE, off + 43, (byte) (seqAdd >> 16));
        rw.set(java.lang.foreign.ValueLayout.JAVA_BYTE, off + 44, (byte) (seqAdd >> 8));
        rw.set(java.lang.foreign.ValueLayout.JAVA_BYTE, off + 45, (byte) seqAdd);
        rw.set(java.lang.foreign.ValueLayout.JAVA_BYTE, off + 46, (byte) 0);
        rw.set(java.lang.foreign.ValueLayout.JAVA_BYTE, off + 47, (byte) 0);
    }

    /** bytes of one vpcsum_tcphdr_t header template ({@link #tcpHdr}) */
    public static final int TCP_HDR = 64;
    /** bytes of one vpcsum_tcpseg_t record ({@link #tcpSeg}) */
    public static final int TCP_SEG = 32;

    /** Fill the 64-byte header template at {@code hdr[off..]} for one direction of a TcpEntry, as
     * TcpUtils.buildCommonTcpResponse / buildIpResponse read it at the moment of the batch:
     * {@code fastpathRemote} / {@code fastpathLocal} the entry's Fastpath addresses (6 bytes each; null:
     * no Ethernet header, the frame starts at the IP header), {@code src} / {@code dst} 4 or 16 address
     * bytes (tcp.local / tcp.remote), ports, {@code ack} (receivingQueue.getAckedSeq()) and {@code window}
     * (receivingQueue.getWindow() / scale) as the ints Java passes to setAckNum / setWindow.  tos 0,
     * TTL / hop limit 64, identification and fragment word 0: what the stack uses. */
    public static void tcpHdr(MemorySegment hdr, long off, byte[] fastpathRemote, byte[] fastpathLocal, byte[] src, byte[] dst,
                              int sport, int dport, int ack, int window) {
        final var B = java.lang.foreign.ValueLayout.JAVA_BYTE;
        hdr.asSlice(off, TCP_HDR).fill((byte) 0);
        boolean eth = fastpathRemote != null && fastpathLocal != null;
        for (int i = 0; eth && i < 6; ++i) {
            hdr.set(B, off + i, fastpathRemote[i]);
            hdr.set(B, off + 6 + i, fastpathLocal[i]);
        }
        hdr.set(B, off + 12, (byte) (eth ? 14 : 0));
        hdr.set(B, off + 13, (byte) (src.length == 4 ? 4 : 6));
        hdr.set(B, off + 15, (byte) 64);
        for (int i = 0; i < src.length; ++i) {
            hdr.set(B, off + 16 + i, src[i]);
            hdr.set(B, off + 32 + i, dst[i]);
        }
        hdr.set(B, off + 48, (byte) (sport >> 8));
        hdr.set(B, off + 49, (byte) sport);
        hdr.set(B, off + 50, (byte) (dport >> 8));
        hdr.set(B, off + 51, (byte) dport);
        hdr.set(B, off + 52, (byte) (ack >> 24));
        hdr.set(B, off + 53, (byte) (ack >> 16));
        hdr.set(B, off + 54, (byte) (ack >> 8));
        hdr.set(B, off + 55, (byte) ack);
        hdr.set(B, off + 56, (byte) (window >> 8));
        hdr.set(B, off + 57, (byte) window);
    }

    /** Fill the 32-byte record at {@code seg[off..]}: the frame goes to {@code frameOff} of the
     * destination arena (room {@code frameCap} there), its {@code dataLen} payload bytes come from
     * {@code dataOff} of the source arena, {@code seq} is Segment.seqBeginInclusive (or the sequence
     * number of a FIN / ACK / RST, dataLen 0), {@code hdrIndex} the template, {@code flags} the TCP
     * flags (Consts.TCP_FLAGS_*, low 6 bits). */
    public static void tcpSeg(MemorySegment seg, long off, long frameOff, long dataOff, int seq, int hdrIndex, int frameCap,
                              int dataLen, int flags) {
        final var LE = java.nio.ByteOrder.LITTLE_ENDIAN;
        seg.set(java.lang.foreign.ValueLayout.JAVA_LONG_UNALIGNED.withOrder(LE), off, frameOff);
        seg.set(java.lang.foreign.ValueLayout.JAVA_LONG_UNALIGNED.withOrder(LE), off + 8, dataOff);
        seg.set(java.lang.foreign.ValueLayout.JAVA_INT_UNALIGNED.withOrder(LE), off + 16, seq);
        seg.set(java.lang.foreign.ValueLayout.JAVA_INT_UNALIGNED.withOrder(LE), off + 20, hdrIndex);
        seg.set(java.lang.foreign.ValueLayout.JAVA_INT_UNALIGNED.withOrder(LE), off + 24, frameCap);
        seg.set(java.lang.foreign.ValueLayout.JAVA_SHORT_UNALIGNED.withOrder(LE), off + 28, (short) dataLen);
        seg.set(java.lang.foreign.ValueLayout.JAVA_BYTE, off + 30, (byte) (flags & 0x3f));
        seg.set(java.lang.foreign.ValueLayout.JAVA_BYTE, off + 31, (byte) 0);
    }

    /** bytes of one vpcsum_tcpburst_t record ({@link #tcpBurst}) */
    public static final int TCP_BURST = 32;

    /** Fill the 32-byte burst record at {@code burst[off..]}: one SendingQueue.fetch().  {@code dataOff}
     * is where the byte with sequence number ackSeq lies in the source arena, {@code dataLen} =
     * min(window, queued bytes from ackSeq on), {@code seq} = ackSeq (the first Segment's
     * seqBeginInclusive), {@code hdrIndex} the template, {@code firstFrame} the index of the burst's
     * first frame in the call's frame table (non-decreasing over the records), {@code mss} the
     * sendingQueue's, {@code flags} the TCP flags of every frame (PSH | ACK).  The frame count,
     * max(1, ceil(dataLen / mss)), is written here and returned: the caller reserves that many chunks.
     * dataLen 0: one frame without payload (FIN / ACK / RST), mss ignored. */
    public static int tcpBurst(MemorySegment burst, long off, long dataOff, int dataLen, int seq, int hdrIndex, int firstFrame,
                               int mss, int flags) {
        final var LE = java.nio.ByteOrder.LITTLE_ENDIAN;
        int count = dataLen == 0 ? 1 : (int) ((Integer.toUnsignedLong(dataLen) - 1) / mss + 1);
        burst.set(java.lang.foreign.ValueLayout.JAVA_LONG_UNALIGNED.withOrder(LE), off, dataOff);
        burst.set(java.lang.foreign.ValueLayout.JAVA_INT_UNALIGNED.withOrder(LE), off + 8, dataLen);
        burst.set(java.lang.foreign.ValueLayout.JAVA_INT_UNALIGNED.withOrder(LE), off + 12, seq);
        burst.set(java.lang.foreign.ValueLayout.JAVA_INT_UNALIGNED.withOrder(LE), off + 16, hdrIndex);
        burst.set(java.lang.foreign.ValueLayout.JAVA_INT_UNALIGNED.withOrder(LE), off + 20, firstFrame);
        burst.set(java.lang.foreign.ValueLayout.JAVA_SHORT_UNALIGNED.withOrder(LE), off + 24, (short) mss);
        burst.set(java.lang.foreign.ValueLayout.JAVA_BYTE, off + 26, (byte) (flags & 0x3f));
        burst.set(java.lang.foreign.ValueLayout.JAVA_BYTE, off + 27, (byte) 0);
        burst.set(java.lang.foreign.ValueLayout.JAVA_INT_UNALIGNED.withOrder(LE), off + 28, count);
        return count;
    }

    /** bytes of one vpcsum_tcprx_t receive record ({@link #tcpRx}) */
    public static final int TCP_RX = 16;
    /** bytes of one vpcsum_tcpinfo_t segment digest ({@link #tcpInfoSeq} and its neighbours) */
    public static final int TCP_INFO = 16;
    /** vpcsum_tcprx_t.ops: store the payload past {@code skip}; 0: verify only */
    public static final int TCPRX_STORE = 0x01;

    /** Fill the 16-byte receive record at {@code rx[off..]} for one received segment: payload byte
     * {@code skip} (ReceivingQueue.store's incr = expectingSeq - seqBeginInclusive, 0 for a segment that
     * begins on expectingSeq) goes to {@code dstOff} of the receive arena, which has room {@code dstCap}
     * there; {@code store} false: verify only (a pure ACK, or a segment store() would drop). */
    public static void tcpRx(MemorySegment rx, long off, long dstOff, int dstCap, int skip, boolean store) {
        final var LE = java.nio.ByteOrder.LITTLE_ENDIAN;
        rx.set(java.lang.foreign.ValueLayout.JAVA_LONG_UNALIGNED.withOrder(LE), off, dstOff);
        rx.set(java.lang.foreign.ValueLayout.JAVA_INT_UNALIGNED.withOrder(LE), off + 8, dstCap);
        rx.set(java.lang.foreign.ValueLayout.JAVA_SHORT_UNALIGNED.withOrder(LE), off + 12, (short) skip);
        rx.set(java.lang.foreign.ValueLayout.JAVA_BYTE, off + 14, (byte) (store ? TCPRX_STORE : 0));
        rx.set(java.lang.foreign.ValueLayout.JAVA_BYTE, off + 15, (byte) 0);
    }

    /** bytes of one vpcsum_udpdg_t datagram record ({@link #udpDg}) */
    public static final int UDP_DG = 32;
    /** bytes of one vpcsum_udprx_t receive record ({@link #udpRx}) */
    public static final int UDP_RX = 16;
    /** vpcsum_udprx_t.ops: store the datagram's data; 0: verify only */
    public static final int UDPRX_STORE = 0x01;

    /** Fill the 32-byte record at {@code dg[off..]} for one datagram of UdpOutput.sendUdp's loop: the
     * frame goes to {@code frameOff} of the destination arena (room {@code frameCap} there), its
     * {@code dataLen} bytes (Datagram.data; 0 is legal) come from {@code dataOff} of the source arena,
     * {@code hdrIndex} names the template ({@link #tcpHdr} with ack 0 and window 0: src / sport from
     * udp.listening, dst / dport from the datagram's remote). */
    public static void udpDg(MemorySegment dg, long off, long frameOff, long dataOff, int hdrIndex, int frameCap, int dataLen) {
        final var LE = java.nio.ByteOrder.LITTLE_ENDIAN;
        dg.set(java.lang.foreign.ValueLayout.JAVA_LONG_UNALIGNED.withOrder(LE), off, frameOff);
        dg.set(java.lang.foreign.ValueLayout.JAVA_LONG_UNALIGNED.withOrder(LE), off + 8, dataOff);
        dg.set(java.lang.foreign.ValueLayout.JAVA_INT_UNALIGNED.withOrder(LE), off + 16, hdrIndex);
        dg.set(java.lang.foreign.ValueLayout.JAVA_INT_UNALIGNED.withOrder(LE), off + 20, frameCap);
        dg.set(java.lang.foreign.ValueLayout.JAVA_INT_UNALIGNED.withOrder(LE), off + 24, dataLen);
        dg.set(java.lang.foreign.ValueLayout.JAVA_INT_UNALIGNED.withOrder(LE), off + 28, 0);
    }

    /** Fill the 16-byte receive record at {@code rx[off..]} for one received datagram: its data (segment
     * bytes 8 on) goes to {@code dstOff} of the receive arena, which has room {@code dstCap} there;
     * {@code store} false: verify only (a datagram ReceivingQueue.store's connect filter drops). */
    public static void udpRx(MemorySegment rx, long off, long dstOff, int dstCap, boolean store) {
        final var LE = java.nio.ByteOrder.LITTLE_ENDIAN;
        rx.set(java.lang.foreign.ValueLayout.JAVA_LONG_UNALIGNED.withOrder(LE), off, dstOff);
        rx.set(java.lang.foreign.ValueLayout.JAVA_INT_UNALIGNED.withOrder(LE), off + 8, dstCap);
        rx.set(java.lang.foreign.ValueLayout.JAVA_INT_UNALIGNED.withOrder(LE), off + 12, store ? UDPRX_STORE : 0);   // ops, rsv[3] 0
    }

    /** bytes of one vpcsum_icmprp_t reply record ({@link #icmpRp}) */
    public static final int ICMP_RP = 24;
    /** vpcsum_icmprp_t.kind: IcmpInput.respondIcmpPong / IcmpPortUnreachableOutput.handle /
     * IPInputRoute.respondIcmpTimeExceeded */
    public static final int ICMP_ECHO_REPLY = 1, ICMP_PORT_UNREACH = 2, ICMP_TIME_EXCEEDED = 3;

    /** Fill the 24-byte record at {@code rp[off..]} for the ICMP reply to one received frame: the
     * reply goes to {@code frameOff} of the destination arena (room {@code frameCap} there, a TX chunk),
     * {@code hdrIndex} names the template ({@link #tcpHdr} with ports, ack and window 0: eth_dst the
     * request's pkb.pkt.getSrc(), eth_src the looked-up MAC, dst the request's source, src the
     * request's destination -- for time exceeded the IP getRoutedSrcIpAndMac picks --, ttl 64),
     * {@code kind} one of ICMP_*. */
    public static void icmpRp(MemorySegment rp, long off, long frameOff, int hdrIndex, int frameCap, int kind) {
        final var LE = java.nio.ByteOrder.LITTLE_ENDIAN;
        rp.set(java.lang.foreign.ValueLayout.JAVA_LONG_UNALIGNED.withOrder(LE), off, frameOff);
        rp.set(java.lang.foreign.ValueLayout.JAVA_INT_UNALIGNED.withOrder(LE), off + 8, hdrIndex);
        rp.set(java.lang.foreign.ValueLayout.JAVA_INT_UNALIGNED.withOrder(LE), off + 12, frameCap);
        rp.set(java.lang.foreign.ValueLayout.JAVA_LONG_UNALIGNED.withOrder(LE), off + 16, (long) (kind & 0xff));   // kind, rsv[7] 0
    }

    /** Fields of the 16-byte digest at {@code info[off..]} (vpcsum_tcp_digest_async): seq and ack as
     * TcpPacket.getSeqNum / getAckNum return them (unsigned, in a long), window, payload length,
     * header length (0: no record, the descriptor was refused) and flags. */
    public static long tcpInfoSeq(MemorySegment info, long off) {
        return info.get(java.lang.foreign.ValueLayout.JAVA_INT_UNALIGNED.withOrder(java.nio.ByteOrder.LITTLE_ENDIAN), off) & 0xffffffffL;
    }

    public static long tcpInfoAck(MemorySegment info, long off) {
        return info.get(java.lang.foreign.ValueLayout.JAVA_INT_UNALIGNED.withOrder(java.nio.ByteOrder.LITTLE_ENDIAN), off + 4) & 0xffffffffL;
    }

    public static int tcpInfoWindow(MemorySegment info, long off) {
        return info.get(java.lang.foreign.ValueLayout.JAVA_SHORT_UNALIGNED.withOrder(java.nio.ByteOrder.LITTLE_ENDIAN), off + 8) & 0xffff;
    }

    public static int tcpInfoDataLen(MemorySegment info, long off) {
        return info.get(java.lang.foreign.ValueLayout.JAVA_SHORT_UNALIGNED.withOrder(java.nio.ByteOrder.LITTLE_ENDIAN), off + 10) & 0xffff;
    }

    public static int tcpInfoHlen(MemorySegment info, long off) {
        return info.get(java.lang.foreign.ValueLayout.JAVA_BYTE, off + 12) & 0xff;
    }

    public static int tcpInfoFlags(MemorySegment info, long off) {
        return info.get(java.lang.foreign.ValueLayout.JAVA_BYTE, off + 13) & 0xff;
    }

    private static final MethodHandle createMH = PanamaUtils.lookupPNIFunction(new PNILinkOptions().setCritical(false),
        "Java_io_vproxy_vpcsum_VPCsum_create", int.class /* device */, long.class /* maxArena */, int.class /* maxPkts */);

    /** Create a context on GPU {@code device}: device buffers for one batch of up to maxPkts
     * packets spanning at most maxArena bytes (double buffered). Returns an opaque handle. */
    public long create(PNIEnv ENV, int device, long maxArena, int maxPkts) throws java.io.IOException {
        ENV.reset();
        int ERR;
        try {
            ERR = (int) createMH.invokeExact(ENV.MEMORY, device, maxArena, maxPkts);
        } catch (Throwable THROWABLE) {
            throw PanamaUtils.convertInvokeExactException(THROWABLE);
        }
        if (ERR != 0) {
            ENV.throwIf(java.io.IOException.class);
            ENV.throwLast();
        }
        return ENV.returnLong();
    }

    private static final MethodHandle registerArenaMH = PanamaUtils.lookupPNIFunction(new PNILinkOptions().setCritical(false),
        "Java_io_vproxy_vpcsum_VPCsum_registerArena", long.class /* ctx */, MemorySegment.class /* arena */, long.class /* len */);

    /** Page-lock a long-lived arena (an AF_XDP umem, UMem.java:36-44) once, so batches from it
     * DMA straight to the GPU without a staging copy. */
    public void registerArena(PNIEnv ENV, long ctx, MemorySegment arena, long len) throws java.io.IOException {
        ENV.reset();
        int ERR;
        try {
            ERR = (int) registerArenaMH.invokeExact(ENV.MEMORY, ctx, arena, len);
        } catch (Throwable THROWABLE) {
            throw PanamaUtils.convertInvokeExactException(THROWABLE);
        }
        if (ERR != 0) {
            ENV.throwIf(java.io.IOException.class);
            ENV.throwLast();
        }
    }

    private static final MethodHandle submitMH = PanamaUtils.lookupPNIFunction(new PNILinkOptions().setCritical(false),
        "Java_io_vproxy_vpcsum_VPCsum_submit", long.class /* ctx */, MemorySegment.class /* arena */, long.class /* arenaLen */,
        MemorySegment.class /* desc */, int.class /* n */, MemorySegment.class /* out */, MemorySegment.class /* status */,
        int.class /* mode */);

    /** Asynchronously checksum n packets described by 16-byte descriptors (vpcsum_desc_t) over
     * {@code arena}. Returns a ticket for {@link #waitFor}. */
    public long submit(PNIEnv ENV, long ctx, MemorySegment arena, long arenaLen, MemorySegment desc, int n,
                       MemorySegment out, MemorySegment status, int mode) throws java.io.IOException {
        ENV.reset();
        int ERR;
        try {
            ERR = (int) submitMH.invokeExact(ENV.MEMORY, ctx, arena, arenaLen, desc, n, out, status, mode);
        } catch (Throwable THROWABLE) {
            throw PanamaUtils.convertInvokeExactException(THROWABLE);
        }
        if (ERR != 0) {
            ENV.throwIf(java.io.IOException.class);
            ENV.throwLast();
        }
        return ENV.returnLong();
    }

    private static final MethodHandle submitPreMH = PanamaUtils.lookupPNIFunction(new PNILinkOptions().setCritical(false),
        "Java_io_vproxy_vpcsum_VPCsum_submitPre", long.class /* ctx */, MemorySegment.class /* arena */,
        long.class /* arenaLen */, MemorySegment.class /* desc */, MemorySegment.class /* pre */, int.class /* n */,
        MemorySegment.class /* out */, MemorySegment.class /* status */, int.class /* mode */);

    /** {@link #submit} for an egress batch that holds frames changed in place: descriptors with
     * F_PRE take their L4 sum from {@code pre[i]} (48-B vpcsum_pre_t: a PRE_HSUM entry,
     * {@link PreImage#writeTo}) by RFC 1624, reading only the frame's header; the others are summed
     * in full (vpcsum_ctx_submit_pre).  mode: MODE_COMPUTE or MODE_WRITE.  Returns a ticket for
     * {@link #waitFor}. */
    public long submitPre(PNIEnv ENV, long ctx, MemorySegment arena, long arenaLen, MemorySegment desc, MemorySegment pre,
                          int n, MemorySegment out, MemorySegment status, int mode) throws java.io.IOException {
        ENV.reset();
        int ERR;
        try {
            ERR = (int) submitPreMH.invokeExact(ENV.MEMORY, ctx, arena, arenaLen, desc, pre, n, out, status, mode);
        } catch (Throwable THROWABLE) {
            throw PanamaUtils.convertInvokeExactException(THROWABLE);
        }
        if (ERR != 0) {
            ENV.throwIf(java.io.IOException.class);
            ENV.throwLast();
        }
        return ENV.returnLong();
    }

    private static final MethodHandle waitForMH = PanamaUtils.lookupPNIFunction(new PNILinkOptions().setCritical(false),
        "Java_io_vproxy_vpcsum_VPCsum_waitFor", long.class /* ctx */, long.class /* ticket */);

    /** Block until the batch of {@code ticket} is done; results (and, with MODE_WRITE, the
     * checksum fields inside the frames) are valid afterwards. */
    public void waitFor(PNIEnv ENV, long ctx, long ticket) throws java.io.IOException {
        ENV.reset();
        int ERR;
        try {
            ERR = (int) waitForMH.invokeExact(ENV.MEMORY, ctx, ticket);
        } catch (Throwable THROWABLE) {
            throw PanamaUtils.convertInvokeExactException(THROWABLE);
        }
        if (ERR != 0) {
            ENV.throwIf(java.io.IOException.class);
            ENV.throwLast();
        }
    }

    private static final MethodHandle verifyFramesMH = PanamaUtils.lookupPNIFunction(new PNILinkOptions().setCritical(false),
        "Java_io_vproxy_vpcsum_VPCsum_verifyFrames", long.class /* ctx */, MemorySegment.class /* arena */,
        long.class /* arenaLen */, MemorySegment.class /* frameOff */, MemorySegment.class /* frameLen */, int.class /* n */,
        MemorySegment.class /* out */, MemorySegment.class /* status */);

    /** Ingress verify of a received batch: the raw Ethernet frames at frameOff[i] (u64, bytes into
     * {@code arena}, which must be registered) of frameLen[i] (u32) bytes are parsed on the GPU with
     * the rules of EthernetPacket/Ipv4Packet/Ipv6Packet.from and verified where they lie.
     * status[i] gets S_IP_OK / S_L4_OK / S_UDP_NOCSUM (or S_BAD_DESC when the frame does not parse).
     * Returns a ticket for {@link #waitFor}. */
    public long verifyFrames(PNIEnv ENV, long ctx, MemorySegment arena, long arenaLen, MemorySegment frameOff,
                             MemorySegment frameLen, int n, MemorySegment out, MemorySegment status) throws java.io.IOException {
        ENV.reset();
        int ERR;
        try {
            ERR = (int) verifyFramesMH.invokeExact(ENV.MEMORY, ctx, arena, arenaLen, frameOff, frameLen, n, out, status);
        } catch (Throwable THROWABLE) {
            throw PanamaUtils.convertInvokeExactException(THROWABLE);
        }
        if (ERR != 0) {
            ENV.throwIf(java.io.IOException.class);
            ENV.throwLast();
        }
        return ENV.returnLong();
    }

    private static final MethodHandle verifyFramesHsumMH = PanamaUtils.lookupPNIFunction(new PNILinkOptions().setCritical(false),
        "Java_io_vproxy_vpcsum_VPCsum_verifyFramesHsum", long.class /* ctx */, MemorySegment.class /* arena */,
        long.class /* arenaLen */, MemorySegment.class /* frameOff */, MemorySegment.class /* frameLen */, int.class /* n */,
        MemorySegment.class /* out */, MemorySegment.class /* status */, MemorySegment.class /* hsum */);

    /** {@link #verifyFrames} that also records each frame's ingress header sum: hsum[i] (8 B,
     * vpcsum_hsum_t: the sum of the L4 sum's words the in-place setters can reach, the segment and
     * header lengths, protocol, version and the L3 offset in the frame; all zero for a frame without
     * one).  The egress flush of a frame changed in place updates its L4 sum from it
     * ({@link GpuCsumBatch#defer}, INTEGRATION.md §5).  Returns a ticket for {@link #waitFor}. */
    public long verifyFramesHsum(PNIEnv ENV, long ctx, MemorySegment arena, long arenaLen, MemorySegment frameOff,
                                 MemorySegment frameLen, int n, MemorySegment out, MemorySegment status,
                                 MemorySegment hsum) throws java.io.IOException {
        ENV.reset();
        int ERR;
        try {
            ERR = (int) verifyFramesHsumMH.invokeExact(ENV.MEMORY, ctx, arena, arenaLen, frameOff, frameLen, n, out, status,
                                                       hsum);
        } catch (Throwable THROWABLE) {
            throw PanamaUtils.convertInvokeExactException(THROWABLE);
        }
        if (ERR != 0) {
            ENV.throwIf(java.io.IOException.class);
            ENV.throwLast();
        }
        return ENV.returnLong();
    }

    private static final MethodHandle parseFramesMH = PanamaUtils.lookupPNIFunction(new PNILinkOptions().setCritical(false),
        "Java_io_vproxy_vpcsum_VPCsum_parseFrames", long.class /* ctx */, MemorySegment.class /* arena */,
        long.class /* arenaLen */, MemorySegment.class /* frameOff */, MemorySegment.class /* frameLen */, int.class /* n */,
        MemorySegment.class /* desc */, MemorySegment.class /* status */, MemorySegment.class /* tuples */);

    /** Batched parse of a received batch with flow tuples: the frames at frameOff[i] / frameLen[i]
     * of the registered {@code arena} are parsed on the GPU (EthernetPacket/Ipv4Packet/Ipv6Packet
     * rules).  After {@link #waitFor}: desc[i] (16 B, ready for submit / natSubmit), status[i]
     * (0 or S_BAD_DESC) and tuples[i] (40 B: src[16] dst[16] sport[2] dport[2] ver proto
     * tcpFlags rsv, network order), the key TcpInput / UdpInput look up in the conntrack
     * (TcpInput.java:47-51, UdpInput.java:45-47).  Returns a ticket. */
    public long parseFrames(PNIEnv ENV, long ctx, MemorySegment arena, long arenaLen, MemorySegment frameOff,
                            MemorySegment frameLen, int n, MemorySegment desc, MemorySegment status,
                            MemorySegment tuples) throws java.io.IOException {
        ENV.reset();
        int ERR;
        try {
            ERR = (int) parseFramesMH.invokeExact(ENV.MEMORY, ctx, arena, arenaLen, frameOff, frameLen, n, desc, status, tuples);
        } catch (Throwable THROWABLE) {
            throw PanamaUtils.convertInvokeExactException(THROWABLE);
        }
        if (ERR != 0) {
            ENV.throwIf(java.io.IOException.class);
            ENV.throwLast();
        }
        return ENV.returnLong();
    }

    private static final MethodHandle egressFramesMH = PanamaUtils.lookupPNIFunction(new PNILinkOptions().setCritical(false),
        "Java_io_vproxy_vpcsum_VPCsum_egressFrames", long.class /* ctx */, MemorySegment.class /* arena */,
        long.class /* arenaLen */, MemorySegment.class /* frameOff */, MemorySegment.class /* frameLen */,
        MemorySegment.class /* frameFlags */, int.class /* n */, MemorySegment.class /* out */,
        MemorySegment.class /* status */);

    /** Egress flush straight from the frames: frameOff[i] (u64) / frameLen[i] (u32) as the TX ring
     * sends them, frameFlags[i] (u8) the F_* sums each needs.  The GPU parses every frame with the
     * vswitch's rules and writes its sums in place, in one submission; after {@link #waitFor}
     * status[i] is S_DONE or S_BAD_DESC (refused, nothing written: hand the frame back).
     * Returns a ticket. */
    public long egressFrames(PNIEnv ENV, long ctx, MemorySegment arena, long arenaLen, MemorySegment frameOff,
                             MemorySegment frameLen, MemorySegment frameFlags, int n, MemorySegment out,
                             MemorySegment status) throws java.io.IOException {
        ENV.reset();
        int ERR;
        try {
            ERR = (int) egressFramesMH.invokeExact(ENV.MEMORY, ctx, arena, arenaLen, frameOff, frameLen, frameFlags, n,
                                                   out, status);
        } catch (Throwable THROWABLE) {
            throw PanamaUtils.convertInvokeExactException(THROWABLE);
        }
        if (ERR != 0) {
            ENV.throwIf(java.io.IOException.class);
            ENV.throwLast();
        }
        return ENV.returnLong();
    }

    private static final MethodHandle natSubmitMH = PanamaUtils.lookupPNIFunction(new PNILinkOptions().setCritical(false),
        "Java_io_vproxy_vpcsum_VPCsum_natSubmit", long.class /* ctx */, MemorySegment.class /* arena */,
        long.class /* arenaLen */, MemorySegment.class /* desc */, MemorySegment.class /* rw */, int.class /* n */,
        MemorySegment.class /* status */, int.class /* natMode */);

    /** SwitchUtils.applyNat for a batch (SwitchUtils.java:522-542): rewrite {@code rw[i]}
     * (48-byte vpcsum_nat_t entries: addresses, ports, TTL / hop limit) into the packet of
     * {@code desc[i]} in place, with the checksums updated as getRawPacket(0) would recompute them
     * (NAT_RFC1624 on valid input, NAT_STRICT_JAVA for any input).  Frames in the registered umem
     * are rewritten where they lie.  status[i]: S_DONE or S_BAD_DESC.  With NAT_TCP_REWRITES in
     * natMode, entries with NAT_TCP also rewrite the sequence number, the flags and the MSS option
     * ({@link #natTcp}); status[i] may then carry S_MSS_ABSENT.  Returns a ticket for
     * {@link #waitFor}. */
    public long natSubmit(PNIEnv ENV, long ctx, MemorySegment arena, long arenaLen, MemorySegment desc,
                          MemorySegment rw, int n, MemorySegment status, int natMode) throws java.io.IOException {
        ENV.reset();
        int ERR;
        try {
            ERR = (int) natSubmitMH.invokeExact(ENV.MEMORY, ctx, arena, arenaLen, desc, rw, n, status, natMode);
        } catch (Throwable THROWABLE) {
            throw PanamaUtils.convertInvokeExactException(THROWABLE);
        }
        if (ERR != 0) {
            ENV.throwIf(java.io.IOException.class);
            ENV.throwLast();
        }
        return ENV.returnLong();
    }

    /** Verdicts of {@link #natFlowFrames} (VPCSUM_FLOW_*): no such flow (or not TCP / UDP, or a frame
     * the parser refuses); rewritten with the flow's entry; known flow but TCP with FIN / SYN / RST. */
    public static final int FLOW_MISS = 0, FLOW_HIT = 1, FLOW_PUNT = 2;
    /** sizeof(vpcsum_flow_t): key (40-byte vpcsum_tuple_t, tcp_flags / rsv 0), rw (48-byte vpcsum_nat_t), cookie (u64). */
    public static final int FLOW_BYTES = 96;

    private static final MethodHandle flowtabCreateMH = PanamaUtils.lookupPNIFunction(new PNILinkOptions().setCritical(false),
        "Java_io_vproxy_vpcsum_VPCsum_flowtabCreate", int.class /* device */, int.class /* maxFlows */);

    /** A NAT flow table for up to {@code maxFlows} flows on {@code device}: the part of Conntrack's
     * lookup (Conntrack.java:106-125) the vswitch offloads (INTEGRATION.md §5). */
    public long flowtabCreate(PNIEnv ENV, int device, int maxFlows) throws java.io.IOException {
        ENV.reset();
        int ERR;
        try {
            ERR = (int) flowtabCreateMH.invokeExact(ENV.MEMORY, device, maxFlows);
        } catch (Throwable THROWABLE) {
            throw PanamaUtils.convertInvokeExactException(THROWABLE);
        }
        if (ERR != 0) {
            ENV.throwIf(java.io.IOException.class);
            ENV.throwLast();
        }
        return ENV.returnLong();
    }

    private static final MethodHandle flowtabUpdateMH = PanamaUtils.lookupPNIFunction(new PNILinkOptions().setCritical(false),
        "Java_io_vproxy_vpcsum_VPCsum_flowtabUpdate", long.class /* tab */, MemorySegment.class /* del */, int.class /* nDel */,
        MemorySegment.class /* add */, int.class /* nAdd */);

    /** Erase the {@code nDel} keys of {@code del} (40 B each), then insert / replace the {@code nAdd}
     * flows of {@code add} (FLOW_BYTES each).  Returns when the device table holds them; a refused
     * flow (malformed key, full table) throws and changes nothing.  Wait for natFlowFrames batches
     * in flight first: they are not ordered against the update. */
    public void flowtabUpdate(PNIEnv ENV, long tab, MemorySegment del, int nDel, MemorySegment add, int nAdd)
        throws java.io.IOException {
        ENV.reset();
        int ERR;
        try {
            ERR = (int) flowtabUpdateMH.invokeExact(ENV.MEMORY, tab, del, nDel, add, nAdd);
        } catch (Throwable THROWABLE) {
            throw PanamaUtils.convertInvokeExactException(THROWABLE);
        }
        if (ERR != 0) {
            ENV.throwIf(java.io.IOException.class);
            ENV.throwLast();
        }
    }

    private static final MethodHandle flowtabCollectMH = PanamaUtils.lookupPNIFunction(new PNILinkOptions().setCritical(false),
        "Java_io_vproxy_vpcsum_VPCsum_flowtabCollect", long.class /* tab */, MemorySegment.class /* cookies */, int.class /* cap */);

    /** The cookies (u64 each, room for {@code cap}) of the flows hit since the last collect, each
     * once: the entries to resetTimer().  Returns their number; above {@code cap} nothing was
     * written or cleared: call again with room. */
    public int flowtabCollect(PNIEnv ENV, long tab, MemorySegment cookies, int cap) throws java.io.IOException {
        ENV.reset();
        int ERR;
        try {
            ERR = (int) flowtabCollectMH.invokeExact(ENV.MEMORY, tab, cookies, cap);
        } catch (Throwable THROWABLE) {
            throw PanamaUtils.convertInvokeExactException(THROWABLE);
        }
        if (ERR != 0) {
            ENV.throwIf(java.io.IOException.class);
            ENV.throwLast();
        }
        return ENV.returnInt();
    }

    private static final MethodHandle flowtabCloseMH = PanamaUtils.lookupPNIFunction(new PNILinkOptions().setCritical(false),
        "Java_io_vproxy_vpcsum_VPCsum_flowtabClose", long.class /* tab */);

    public void flowtabClose(PNIEnv ENV, long tab) {
        ENV.reset();
        int ERR;
        try {
            ERR = (int) flowtabCloseMH.invokeExact(ENV.MEMORY, tab);
        } catch (Throwable THROWABLE) {
            throw PanamaUtils.convertInvokeExactException(THROWABLE);
        }
        if (ERR != 0) {
            ENV.throwLast();
        }
    }

    private static final MethodHandle natFlowFramesMH = PanamaUtils.lookupPNIFunction(new PNILinkOptions().setCritical(false),
        "Java_io_vproxy_vpcsum_VPCsum_natFlowFrames", long.class /* ctx */, long.class /* tab */, MemorySegment.class /* arena */,
        long.class /* arenaLen */, MemorySegment.class /* frameOff */, MemorySegment.class /* frameLen */, int.class /* n */,
        MemorySegment.class /* status */, MemorySegment.class /* verdict */, int.class /* natMode */);

    /** The NAT fast path of a received batch of the registered umem in one submission: parse
     * ({@link #parseFrames}' rules), lookup in {@code tab}, rewrite in place ({@link #natSubmit}'s
     * natMode).  After {@link #waitFor}: verdict[i] FLOW_*, status[i] S_DONE / S_BAD_DESC
     * (+ S_TTL_EXPIRED, S_MSS_ABSENT).  A frame with FLOW_MISS / FLOW_PUNT or S_BAD_DESC is
     * untouched and takes TcpInput / UdpInput's path. */
    public long natFlowFrames(PNIEnv ENV, long ctx, long tab, MemorySegment arena, long arenaLen, MemorySegment frameOff,
                              MemorySegment frameLen, int n, MemorySegment status, MemorySegment verdict, int natMode)
        throws java.io.IOException {
        ENV.reset();
        int ERR;
        try {
            ERR = (int) natFlowFramesMH.invokeExact(ENV.MEMORY, ctx, tab, arena, arenaLen, frameOff, frameLen, n, status, verdict, natMode);
        } catch (Throwable THROWABLE) {
            throw PanamaUtils.convertInvokeExactException(THROWABLE);
        }
        if (ERR != 0) {
            ENV.throwIf(java.io.IOException.class);
            ENV.throwLast();
        }
        return ENV.returnLong();
    }

    private static final MethodHandle flowtabSetFastpathMH = PanamaUtils.lookupPNIFunction(new PNILinkOptions().setCritical(false),
        "Java_io_vproxy_vpcsum_VPCsum_flowtabSetFastpath", long.class /* tab */, MemorySegment.class /* keys */,
        MemorySegment.class /* fp */, int.class /* n */);

    /** Sets the Fastpath of {@code n} flows: {@code keys} 40-byte vpcsum_tuple_t each, {@code fp}
     * 16-byte vpcsum_fastpath_t each -- dst[6] (Fastpath.remote), src[6] (Fastpath.local), u32 port
     * (the caller's name for Fastpath.output; 0 clears the record).  What Switch.sendPacket records
     * on the connection entry, once the first packet of that direction has left by the host's path.
     * Returns how many keys were not in the table (erased meanwhile: not an error); a malformed key
     * throws and changes nothing.  Ordered like {@link #flowtabUpdate}. */
    public int flowtabSetFastpath(PNIEnv ENV, long tab, MemorySegment keys, MemorySegment fp, int n) throws java.io.IOException {
        ENV.reset();
        int ERR;
        try {
            ERR = (int) flowtabSetFastpathMH.invokeExact(ENV.MEMORY, tab, keys, fp, n);
        } catch (Throwable THROWABLE) {
            throw PanamaUtils.convertInvokeExactException(THROWABLE);
        }
        if (ERR != 0) {
            ENV.throwIf(java.io.IOException.class);
            ENV.throwLast();
        }
        return ENV.returnInt();
    }

    private static final MethodHandle natFlowForwardFramesMH = PanamaUtils.lookupPNIFunction(new PNILinkOptions().setCritical(false),
        "Java_io_vproxy_vpcsum_VPCsum_natFlowForwardFrames", long.class /* ctx */, long.class /* tab */, MemorySegment.class /* arena */,
        long.class /* arenaLen */, MemorySegment.class /* frameOff */, MemorySegment.class /* frameLen */, int.class /* n */,
        MemorySegment.class /* status */, MemorySegment.class /* verdict */, MemorySegment.class /* port */, int.class /* natMode */);

    /** {@link #natFlowFrames} that also forwards: a FLOW_HIT frame that was rewritten (S_DONE, not
     * S_BAD_DESC) and whose flow has a Fastpath gets the record's two Ethernet addresses written
     * (EthernetPacket.setDst / setSrc on the raw bytes: nothing else of the frame changes) and
     * port[i] (u32 each) = the record's port: the frame is ready for that port's TX ring.
     * port[i] == 0: the frame's Ethernet header is as received and it takes the path it takes after
     * {@link #natFlowFrames}. */
    public long natFlowForwardFrames(PNIEnv ENV, long ctx, long tab, MemorySegment arena, long arenaLen, MemorySegment frameOff,
                                     MemorySegment frameLen, int n, MemorySegment status, MemorySegment verdict,
                                     MemorySegment port, int natMode) throws java.io.IOException {
        ENV.reset();
        int ERR;
        try {
            ERR = (int) natFlowForwardFramesMH.invokeExact(ENV.MEMORY, ctx, tab, arena, arenaLen, frameOff, frameLen, n, status, verdict,
                port, natMode);
        } catch (Throwable THROWABLE) {
            throw PanamaUtils.convertInvokeExactException(THROWABLE);
        }
        if (ERR != 0) {
            ENV.throwIf(java.io.IOException.class);
            ENV.throwLast();
        }
        return ENV.returnLong();
    }

    private static final MethodHandle buildTcpFramesMH = PanamaUtils.lookupPNIFunction(new PNILinkOptions().setCritical(false),
        "Java_io_vproxy_vpcsum_VPCsum_buildTcpFrames", long.class /* ctx */, MemorySegment.class /* dst */, long.class /* dstLen */,
        MemorySegment.class /* src */, long.class /* srcLen */, MemorySegment.class /* hdr */, int.class /* nHdr */,
        MemorySegment.class /* seg */, int.class /* n */, MemorySegment.class /* frameLen */, MemorySegment.class /* out */,
        MemorySegment.class /* status */);

    /** The TCP segment build (vpcsum_ctx_build_tcp_frames): {@code n} records of {@link #TCP_SEG} bytes
     * ({@link #tcpSeg}) over {@code nHdr} templates of {@link #TCP_HDR} bytes ({@link #tcpHdr}); each
     * frame -- Ethernet, IP and TCP headers with both sums, then the payload copied from {@code src} --
     * is written at its frameOff of {@code dst}, which must lie in a registered arena (the TX umem).  A
     * registered {@code src} is read in place, any other staged.  After {@link #waitFor}:
     * frameLen[i] (u32) the frame's length, 0 for a refused record (status[i] S_BAD_DESC, nothing
     * written); out / status may be MemorySegment.NULL.  SYNs carry options: build them on the host. */
    public long buildTcpFrames(PNIEnv ENV, long ctx, MemorySegment dst, long dstLen, MemorySegment src, long srcLen,
                               MemorySegment hdr, int nHdr, MemorySegment seg, int n, MemorySegment frameLen, MemorySegment out,
                               MemorySegment status) throws java.io.IOException {
        ENV.reset();
        int ERR;
        try {
            ERR = (int) buildTcpFramesMH.invokeExact(ENV.MEMORY, ctx, dst, dstLen, src, srcLen, hdr, nHdr, seg, n, frameLen, out,
                status);
        } catch (Throwable THROWABLE) {
            throw PanamaUtils.convertInvokeExactException(THROWABLE);
        }
        if (ERR != 0) {
            ENV.throwIf(java.io.IOException.class);
            ENV.throwLast();
        }
        return ENV.returnLong();
    }

    /* Resolved on first use, not in the static initialiser: the entry came after ABI version 4 was
     * fixed, and a library from before it must still initialise this class (VPCsumLib.hasTcpBursts). */
    private static volatile MethodHandle buildTcpBurstsMH;

    /** The TCP send bursts (vpcsum_ctx_build_tcp_bursts): {@link #buildTcpFrames} with one record of
     * {@link #TCP_BURST} bytes ({@link #tcpBurst}) per SendingQueue.fetch() instead of one per frame.
     * {@code frameOff} holds {@code nFrames} u64 frame offsets of {@code dst}, every frame with
     * {@code frameCap} bytes of room (the umem chunk's); the frames of burst b are
     * frameOff[first .. first + count), cut from the burst's payload run on the GPU.  After
     * {@link #waitFor}: frameLen[j] (u32) the frame's length, 0 for a refused frame (status[j]
     * S_BAD_DESC, nothing written); out / status may be MemorySegment.NULL. */
    public long buildTcpBursts(PNIEnv ENV, long ctx, MemorySegment dst, long dstLen, MemorySegment src, long srcLen,
                               MemorySegment hdr, int nHdr, MemorySegment burst, int nBursts, MemorySegment frameOff, int nFrames,
                               int frameCap, MemorySegment frameLen, MemorySegment out, MemorySegment status)
        throws java.io.IOException {
        MethodHandle MH = buildTcpBurstsMH;
        if (MH == null) {
            if (!VPCsumLib.hasTcpBursts()) {
                throw new java.io.IOException("libvpcsum has no buildTcpBursts: the library is older than this binding");
            }
            MH = PanamaUtils.lookupPNIFunction(new PNILinkOptions().setCritical(false),
                "Java_io_vproxy_vpcsum_VPCsum_buildTcpBursts", long.class /* ctx */, MemorySegment.class /* dst */,
                long.class /* dstLen */, MemorySegment.class /* src */, long.class /* srcLen */, MemorySegment.class /* hdr */,
                int.class /* nHdr */, MemorySegment.class /* burst */, int.class /* nBursts */, MemorySegment.class /* frameOff */,
                int.class /* nFrames */, int.class /* frameCap */, MemorySegment.class /* frameLen */,
                MemorySegment.class /* out */, MemorySegment.class /* status */);
            buildTcpBurstsMH = MH;
        }
        ENV.reset();
        int ERR;
        try {
            ERR = (int) MH.invokeExact(ENV.MEMORY, ctx, dst, dstLen, src, srcLen, hdr, nHdr, burst, nBursts, frameOff, nFrames,
                frameCap, frameLen, out, status);
        } catch (Throwable THROWABLE) {
            throw PanamaUtils.convertInvokeExactException(THROWABLE);
        }
        if (ERR != 0) {
            ENV.throwIf(java.io.IOException.class);
            ENV.throwLast();
        }
        return ENV.returnLong();
    }

    private static final MethodHandle recvTcpFramesMH = PanamaUtils.lookupPNIFunction(new PNILinkOptions().setCritical(false),
        "Java_io_vproxy_vpcsum_VPCsum_recvTcpFrames", long.class /* ctx */, MemorySegment.class /* arena */, long.class /* arenaLen */,
        MemorySegment.class /* desc */, MemorySegment.class /* rx */, int.class /* n */, MemorySegment.class /* dst */,
        long.class /* dstLen */, MemorySegment.class /* stored */, MemorySegment.class /* out */, MemorySegment.class /* status */);

    /** The TCP receive (vpcsum_ctx_recv_tcp_frames): {@code n} descriptors of received frames in
     * {@code arena} (read in place when registered, staged otherwise), each with a record of
     * {@link #TCP_RX} bytes ({@link #tcpRx}); every segment's TCP sum (and IPv4 header sum) is verified
     * as {@link #verifyFrames} would and, in the same pass, its payload past {@code skip} stored at its
     * dstOff of {@code dst}, which must lie in a registered arena (the receive buffers).  This call
     * replaces the verify of these frames.  After {@link #waitFor}: stored[i] (u32) the bytes stored,
     * status[i] the verify status or S_BAD_DESC for a refused record (nothing written); out / status
     * may be MemorySegment.NULL.  THE BYTES ARE STORED WHATEVER THE VERDICT: advance expectingSeq only
     * on S_L4_OK. */
    public long recvTcpFrames(PNIEnv ENV, long ctx, MemorySegment arena, long arenaLen, MemorySegment desc, MemorySegment rx, int n,
                              MemorySegment dst, long dstLen, MemorySegment stored, MemorySegment out, MemorySegment status)
        throws java.io.IOException {
        ENV.reset();
        int ERR;
        try {
            ERR = (int) recvTcpFramesMH.invokeExact(ENV.MEMORY, ctx, arena, arenaLen, desc, rx, n, dst, dstLen, stored, out, status);
        } catch (Throwable THROWABLE) {
            throw PanamaUtils.convertInvokeExactException(THROWABLE);
        }
        if (ERR != 0) {
            ENV.throwIf(java.io.IOException.class);
            ENV.throwLast();
        }
        return ENV.returnLong();
    }

    /* The UDP pair: resolved on first use, as buildTcpBursts is (VPCsumLib.hasUdp). */
    private static volatile MethodHandle buildUdpFramesMH;
    private static volatile MethodHandle recvUdpFramesMH;

    /** The UDP datagram build (vpcsum_ctx_build_udp_frames): {@link #buildTcpFrames} for the datagrams
     * of UdpOutput.sendUdp, one record of {@link #UDP_DG} bytes ({@link #udpDg}) each.  A UDP sum that
     * computes to 0 is stored as 0xffff, as UdpPacket does.  After {@link #waitFor}: frameLen[i] (u32)
     * the frame's length, 0 for a refused record (status[i] S_BAD_DESC, nothing written); out / status
     * may be MemorySegment.NULL. */
    public long buildUdpFrames(PNIEnv ENV, long ctx, MemorySegment dst, long dstLen, MemorySegment src, long srcLen,
                               MemorySegment hdr, int nHdr, MemorySegment dg, int n, MemorySegment frameLen, MemorySegment out,
                               MemorySegment status) throws java.io.IOException {
        MethodHandle MH = buildUdpFramesMH;
        if (MH == null) {
            if (!VPCsumLib.hasUdp()) {
                throw new java.io.IOException("libvpcsum has no buildUdpFrames: the library is older than this binding");
            }
            MH = PanamaUtils.lookupPNIFunction(new PNILinkOptions().setCritical(false),
                "Java_io_vproxy_vpcsum_VPCsum_buildUdpFrames", long.class /* ctx */, MemorySegment.class /* dst */,
                long.class /* dstLen */, MemorySegment.class /* src */, long.class /* srcLen */, MemorySegment.class /* hdr */,
                int.class /* nHdr */, MemorySegment.class /* dg */, int.class /* n */, MemorySegment.class /* frameLen */,
                MemorySegment.class /* out */, MemorySegment.class /* status */);
            buildUdpFramesMH = MH;
        }
        ENV.reset();
        int ERR;
        try {
            ERR = (int) MH.invokeExact(ENV.MEMORY, ctx, dst, dstLen, src, srcLen, hdr, nHdr, dg, n, frameLen, out, status);
        } catch (Throwable THROWABLE) {
            throw PanamaUtils.convertInvokeExactException(THROWABLE);
        }
        if (ERR != 0) {
            ENV.throwIf(java.io.IOException.class);
            ENV.throwLast();
        }
        return ENV.returnLong();
    }

    /** The UDP receive (vpcsum_ctx_recv_udp_frames): {@link #recvTcpFrames} for datagrams, one record
     * of {@link #UDP_RX} bytes ({@link #udpRx}) per descriptor.  status[i] is the verify status --
     * S_UDP_NOCSUM for a stored 0, S_L4_OK for a stored 0xffff whose sum computes to 0 -- or S_BAD_DESC
     * for a refused record; stored[i] (u32) the data bytes, segment bytes 8 on whatever the UDP length
     * field says (UdpPacket.initPartial).  THE BYTES ARE STORED WHATEVER THE VERDICT: enqueue the
     * Datagram only on the verdict the csum-recalc policy accepts, with the source address and port of
     * the parse's tuple. */
    public long recvUdpFrames(PNIEnv ENV, long ctx, MemorySegment arena, long arenaLen, MemorySegment desc, MemorySegment rx, int n,
                              MemorySegment dst, long dstLen, MemorySegment stored, MemorySegment out, MemorySegment status)
        throws java.io.IOException {
        MethodHandle MH = recvUdpFramesMH;
        if (MH == null) {
            if (!VPCsumLib.hasUdp()) {
                throw new java.io.IOException("libvpcsum has no recvUdpFrames: the library is older than this binding");
            }
            MH = PanamaUtils.lookupPNIFunction(new PNILinkOptions().setCritical(false),
                "Java_io_vproxy_vpcsum_VPCsum_recvUdpFrames", long.class /* ctx */, MemorySegment.class /* arena */,
                long.class /* arenaLen */, MemorySegment.class /* desc */, MemorySegment.class /* rx */, int.class /* n */,
                MemorySegment.class /* dst */, long.class /* dstLen */, MemorySegment.class /* stored */,
                MemorySegment.class /* out */, MemorySegment.class /* status */);
            recvUdpFramesMH = MH;
        }
        ENV.reset();
        int ERR;
        try {
            ERR = (int) MH.invokeExact(ENV.MEMORY, ctx, arena, arenaLen, desc, rx, n, dst, dstLen, stored, out, status);
        } catch (Throwable THROWABLE) {
            throw PanamaUtils.convertInvokeExactException(THROWABLE);
        }
        if (ERR != 0) {
            ENV.throwIf(java.io.IOException.class);
            ENV.throwLast();
        }
        return ENV.returnLong();
    }

    /* The ICMP replies: resolved on first use, as the UDP pair is (VPCsumLib.hasIcmpReply). */
    private static volatile MethodHandle replyIcmpFramesMH;

    /** The ICMP replies (vpcsum_ctx_reply_icmp_frames): for descriptor i of {@code arena} (the RX
     * umem, read in place when registered) the reply that record i of {@link #ICMP_RP} bytes
     * ({@link #icmpRp}) names -- echo reply, port unreachable, time exceeded -- written as a finished
     * Ethernet / IP / ICMP frame into {@code dst}, a registered arena (the same umem's TX chunks, or
     * another).  After {@link #waitFor}: frameLen[i] (u32) is the frame's length, 0 for a refused record
     * (Java drops that packet, or the host answers it); csum[i] (u32, may be NULL) the reply's sums;
     * for an echo status[i] / out[i] (each may be NULL) are the REQUEST's verify verdict -- the call
     * replaces the verify of those frames, and THE REPLY IS WRITTEN WHATEVER THE VERDICT: post the TX
     * descriptor only on the verdict the csum-recalc policy accepts; for the two errors S_DONE / 0. */
    public long replyIcmpFrames(PNIEnv ENV, long ctx, MemorySegment arena, long arenaLen, MemorySegment desc, MemorySegment hdr,
                                int nHdr, MemorySegment rp, int n, MemorySegment dst, long dstLen, MemorySegment frameLen,
                                MemorySegment csum, MemorySegment out, MemorySegment status) throws java.io.IOException {
        MethodHandle MH = replyIcmpFramesMH;
        if (MH == null) {
            if (!VPCsumLib.hasIcmpReply()) {
                throw new java.io.IOException("libvpcsum has no replyIcmpFrames: the library is older than this binding");
            }
            MH = PanamaUtils.lookupPNIFunction(new PNILinkOptions().setCritical(false),
                "Java_io_vproxy_vpcsum_VPCsum_replyIcmpFrames", long.class /* ctx */, MemorySegment.class /* arena */,
                long.class /* arenaLen */, MemorySegment.class /* desc */, MemorySegment.class /* hdr */, int.class /* nHdr */,
                MemorySegment.class /* rp */, int.class /* n */, MemorySegment.class /* dst */, long.class /* dstLen */,
                MemorySegment.class /* frameLen */, MemorySegment.class /* csum */, MemorySegment.class /* out */,
                MemorySegment.class /* status */);
            replyIcmpFramesMH = MH;
        }
        ENV.reset();
        int ERR;
        try {
            ERR = (int) MH.invokeExact(ENV.MEMORY, ctx, arena, arenaLen, desc, hdr, nHdr, rp, n, dst, dstLen, frameLen, csum, out, status);
        } catch (Throwable THROWABLE) {
            throw PanamaUtils.convertInvokeExactException(THROWABLE);
        }
        if (ERR != 0) {
            ENV.throwIf(java.io.IOException.class);
            ENV.throwLast();
        }
        return ENV.returnLong();
    }

    private static final MethodHandle setServiceMH =PanamaUtils.lookupPNIFunction(new PNILinkOptions().setCritical(false),
        "Java_io_vproxy_vpcsum_VPCsum_setService", long.class /* ctx */, int.class /* idleUs */);

    /** Low-latency flushes: batches of up to 512 packets from a registered arena go to a resident
     * GPU grid that polls a pinned mailbox, instead of a kernel launch each (about 13 us for 32
     * frames instead of 19).  The grid leaves after {@code idleUs} without a batch and restarts on
     * the next submit; 0 turns it off.  It waits for batches in flight. */
    public void setService(PNIEnv ENV, long ctx, int idleUs) throws java.io.IOException {
        ENV.reset();
        int ERR;
        try {
            ERR = (int) setServiceMH.invokeExact(ENV.MEMORY, ctx, idleUs);
        } catch (Throwable THROWABLE) {
            throw PanamaUtils.convertInvokeExactException(THROWABLE);
        }
        if (ERR != 0) {
            ENV.throwIf(java.io.IOException.class);
            ENV.throwLast();
        }
    }

    private static final MethodHandle closeMH = PanamaUtils.lookupPNIFunction(new PNILinkOptions().setCritical(false),
        "Java_io_vproxy_vpcsum_VPCsum_close", long.class /* ctx */);

    public void close(PNIEnv ENV, long ctx) {
        ENV.reset();
        int ERR;
        try {
            ERR = (int) closeMH.invokeExact(ENV.MEMORY, ctx);
        } catch (Throwable THROWABLE) {
            throw PanamaUtils.convertInvokeExactException(THROWABLE);
        }
        if (ERR != 0) {
            ENV.throwLast();
        }
    }
}

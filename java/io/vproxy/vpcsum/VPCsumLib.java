package io.vproxy.vpcsum;

import java.io.IOException;
import java.lang.foreign.FunctionDescriptor;
import java.lang.foreign.Linker;
import java.lang.foreign.MemorySegment;
import java.lang.foreign.SymbolLookup;
import java.lang.foreign.ValueLayout;
import java.lang.invoke.MethodHandle;
import java.util.Optional;

/**
 * The library check that must work before anything else of libvpcsum is touched.
 *
 * {@link VPCsum} resolves its PNI downcalls in its static initialiser, as the generated PNI
 * classes do (PosixNative.java:729-744): initialising it without the library loaded fails with an
 * ExceptionInInitializerError.  This class holds no such handle: {@link #requireAbi} resolves
 * vpcsum_abi_version on first use and turns a missing library or a different ABI into an
 * IOException, so {@link GpuCsumBatch} can check before it initialises {@link VPCsum}.
 *
 * Not compiled in this repository (the build image has no JDK); see INTEGRATION.md.
 */
final class VPCsumLib {
    private VPCsumLib() {
    }

    private static volatile MethodHandle abiVersionMH;

    /** vpcsum_abi_version() of the loaded library; IOException when it is not loaded. */
    static int abiVersion() throws IOException {
        MethodHandle mh = abiVersionMH;
        if (mh == null) {
            Optional<MemorySegment> sym = SymbolLookup.loaderLookup().find("vpcsum_abi_version");
            if (sym.isEmpty()) {
                throw new IOException("libvpcsum is not loaded (vpcsum_abi_version not found): load it with " +
                                      "Utils.loadDynamicLibrary(\"vpcsum\") before creating a GpuCsumBatch");
            }
            mh = Linker.nativeLinker().downcallHandle(sym.get(), FunctionDescriptor.of(ValueLayout.JAVA_INT));
            abiVersionMH = mh;
        }
        try {
            return (int) mh.invokeExact();
        } catch (Throwable t) {
            throw new IOException("vpcsum_abi_version failed", t);
        }
    }

    /** Whether the loaded library exports {@code symbol}: how a caller probes for an entry point added
     * since ABI version 4 was fixed (include/vpcsum.h), e.g. before it plans a transmit round as bursts. */
    static boolean has(String symbol) {
        return SymbolLookup.loaderLookup().find(symbol).isPresent();
    }

    /** The TCP send bursts ({@link VPCsum#buildTcpBursts}, {@link GpuCsumBatch#buildTcpBursts}). */
    static boolean hasTcpBursts() {
        return has("Java_io_vproxy_vpcsum_VPCsum_buildTcpBursts");
    }

    /** The UDP datagram build and receive ({@link VPCsum#buildUdpFrames}, {@link VPCsum#recvUdpFrames},
     * {@link GpuCsumBatch#buildUdp}, {@link GpuCsumBatch#recvUdp}). */
    static boolean hasUdp() {
        return has("Java_io_vproxy_vpcsum_VPCsum_buildUdpFrames") && has("Java_io_vproxy_vpcsum_VPCsum_recvUdpFrames");
    }

    /** The ICMP replies ({@link VPCsum#replyIcmpFrames}, {@link GpuCsumBatch#replyIcmp}). */
    static boolean hasIcmpReply() {
        return has("Java_io_vproxy_vpcsum_VPCsum_replyIcmpFrames");
    }

    /** IOException unless the loaded library speaks ABI {@code expected} (VPCsum.ABI_VERSION). */
    static void requireAbi(int expected) throws IOException {
        int v = abiVersion();
        if (v != expected) {
            throw new IOException("libvpcsum ABI " + v + ", binding expects " + expected);
        }
    }
}

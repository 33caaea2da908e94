"""ctypes binding of libvpcsum.so (C-ABI in include/vpcsum.h) plus the host-side helpers the
vswitch mirror and the tests use.

There is deliberately NO CPU fallback: if the HIP library cannot be loaded, every entry point
raises :class:`VpcsumUnavailable`.  Device memory and streams come from PyTorch (plumbing only);
``import torch`` happens before the library is loaded so that libvpcsum binds to the same HIP
runtime instance as torch (both carry SONAME libamdhip64.so.7).
"""
from __future__ import annotations

import ctypes
import os
import threading

import numpy as np

from .build import LIB

F_IP, F_L4, F_RAW, F_L4P, F_PRE = 0x01, 0x02, 0x04, 0x08, 0x10
S_IP_OK, S_L4_OK, S_UDP_NOCSUM, S_DONE, S_BAD_DESC = 0x01, 0x02, 0x04, 0x40, 0x80
S_TTL_EXPIRED = 0x20
MODE_COMPUTE, MODE_VERIFY, MODE_WRITE = 0x00, 0x01, 0x10
NAT_SRC, NAT_DST, NAT_SPORT, NAT_DPORT, NAT_DEC_TTL, NAT_SET_TTL = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20
NAT_RFC1624, NAT_STRICT_JAVA = 0x00, 0x01
# TCP-header rewrites of a NAT'd packet (include/vpcsum.h): NAT_TCP in a NAT_DTYPE entry's mask says
# its rsv[0..7] hold them (nat_tcp_fill), honoured only in a batch run with the NAT_TCP_REWRITES mode
# bit; S_MSS_ABSENT: a clamp on a SYN without an MSS option (the caller adds it on the host)
NAT_TCP, NAT_TCP_REWRITES, S_MSS_ABSENT = 0x40, 0x02, 0x08
TCP_SEQ_ADD, TCP_SET_FLAGS, TCP_CLAMP_MSS = 0x01, 0x02, 0x04
PRE_FMT_PRE4, PRE_FMT_PRE = 0, 1   # pre-image entries: NAT4_DTYPE (16 B, IPv4) / NAT_DTYPE (48 B)
PRE_HSUM = 0x80   # pre-image entry mask: the entry's first 8 bytes hold an HSUM_DTYPE record
ABI_VERSION = 4   # include/vpcsum.h VPCSUM_ABI_VERSION: the library this binding was written against
SYNTH_C1, SYNTH_C2, SYNTH_C3, SYNTH_C4, SYNTH_FUZZ, SYNTH_C5 = 1, 2, 3, 4, 5, 6

DESC_DTYPE = np.dtype([("l3_off", "<u8"), ("l3_len", "<u2"), ("l4_off", "<u2"), ("l3_ver", "u1"),
                       ("l4_proto", "u1"), ("flags", "u1"), ("rsv", "u1")])
NAT4_DTYPE = np.dtype([("src", "u1", 4), ("dst", "u1", 4), ("sport", "u1", 2), ("dport", "u1", 2),
                       ("mask", "u1"), ("rsv", "u1", 3)])
NAT_DTYPE = np.dtype([("src", "u1", 16), ("dst", "u1", 16), ("sport", "u1", 2), ("dport", "u1", 2),
                      ("mask", "u1"), ("ttl", "u1"), ("rsv", "u1", 10)])
NAT4R_DTYPE = np.dtype([("desc", DESC_DTYPE), ("rw", NAT4_DTYPE)])   # vpcsum_nat4_rec_t, 32 B
# vpcsum_tuple_t: the flow tuple of a parsed frame (network-order addresses and ports)
TUPLE_DTYPE = np.dtype([("src", "u1", 16), ("dst", "u1", 16), ("sport", "u1", 2), ("dport", "u1", 2),
                        ("l3_ver", "u1"), ("l4_proto", "u1"), ("tcp_flags", "u1"), ("rsv", "u1")])
# vpcsum_hsum_t: a received TCP / UDP frame's ingress header sum (l2_len 0: no record)
HSUM_DTYPE = np.dtype([("sum", "<u2"), ("l4_len", "<u2"), ("hlen", "u1"), ("l4_proto", "u1"), ("l3_ver", "u1"),
                       ("l2_len", "u1")])
# vpcsum_flow_t: one flow of the NAT flow table -- key (tcp_flags / rsv 0), rewrite, caller's cookie
FLOW_DTYPE = np.dtype([("key", TUPLE_DTYPE), ("rw", NAT_DTYPE), ("cookie", "<u8")])
FLOW_MISS, FLOW_HIT, FLOW_PUNT = 0, 1, 2
# vpcsum_fastpath_t: a flow's Ethernet addresses (wire order) and output port; port 0 = no Fastpath
FASTPATH_DTYPE = np.dtype([("dst", "u1", 6), ("src", "u1", 6), ("port", "<u4")])
# vpcsum_tcphdr_t (64 B): one connection direction's header template for the TCP segment build --
# Ethernet addresses, l2_len 14 / 0, version, tos, ttl, addresses, and the wire bytes of ports,
# ack, window, IPv4 identification and flags | fragment offset
TCPHDR_DTYPE = np.dtype([("eth_dst", "u1", 6), ("eth_src", "u1", 6), ("l2_len", "u1"), ("l3_ver", "u1"), ("tos", "u1"),
                         ("ttl", "u1"), ("src", "u1", 16), ("dst", "u1", 16), ("sport", "u1", 2), ("dport", "u1", 2),
                         ("ack", "u1", 4), ("window", "u1", 2), ("ident", "u1", 2), ("frag", "u1", 2), ("rsv", "u1", 2)])
# vpcsum_tcpseg_t (32 B): one frame to build -- where it goes, where its payload lies, seq (host
# order), template index, the room at frame_off, payload length, TCP flags
TCPSEG_DTYPE = np.dtype([("frame_off", "<u8"), ("data_off", "<u8"), ("seq", "<u4"), ("hdr", "<u4"), ("frame_cap", "<u4"),
                         ("data_len", "<u2"), ("flags", "u1"), ("rsv", "u1")])
# vpcsum_tcpburst_t (32 B): one SendingQueue.fetch() of the TCP send bursts -- the run of payload, the
# first sequence number (host order), template index, the burst's first frame in the frame table, MSS,
# TCP flags, frame count
TCPBURST_DTYPE = np.dtype([("data_off", "<u8"), ("data_len", "<u4"), ("seq", "<u4"), ("hdr", "<u4"), ("first", "<u4"),
                           ("mss", "<u2"), ("flags", "u1"), ("rsv", "u1"), ("count", "<u4")])
# vpcsum_tcprx_t (16 B): what the TCP receive does with descriptor i -- where payload byte `skip`
# goes in the receive arena, the room there, the bytes already received, TCPRX_STORE or 0 (verify only)
TCPRX_DTYPE = np.dtype([("dst_off", "<u8"), ("dst_cap", "<u4"), ("skip", "<u2"), ("ops", "u1"), ("rsv", "u1")])
TCPRX_STORE = 0x01
# vpcsum_tcpinfo_t (16 B): a segment's seq, ack, window, payload length (host order), header length
# and flags; hlen 0: no record (a refused descriptor), the rest 0
TCPINFO_DTYPE = np.dtype([("seq", "<u4"), ("ack", "<u4"), ("window", "<u2"), ("data_len", "<u2"), ("hlen", "u1"),
                          ("flags", "u1"), ("rsv", "u1", 2)])
# vpcsum_udphdr_t is vpcsum_tcphdr_t (TCPHDR_DTYPE) with ack / window / rsv 0.
# vpcsum_udpdg_t (32 B): one datagram to build -- where its frame goes, where its payload lies,
# template index, the room at frame_off, payload length (32 bits: too long is refused, not truncated)
UDPDG_DTYPE = np.dtype([("frame_off", "<u8"), ("data_off", "<u8"), ("hdr", "<u4"), ("frame_cap", "<u4"), ("data_len", "<u4"),
                        ("rsv", "<u4")])
# vpcsum_udprx_t (16 B): what the UDP receive does with descriptor i -- where data byte 0 goes in the
# receive arena, the room there, UDPRX_STORE or 0 (verify only)
UDPRX_DTYPE = np.dtype([("dst_off", "<u8"), ("dst_cap", "<u4"), ("ops", "u1"), ("rsv", "u1", 3)])
UDPRX_STORE = 0x01
# vpcsum_icmphdr_t is vpcsum_tcphdr_t (TCPHDR_DTYPE) with ports / ack / window / rsv 0.
# vpcsum_icmprp_t (24 B): the ICMP reply to descriptor i -- where the reply frame goes, template index,
# the room at frame_off, ICMP_ECHO_REPLY / ICMP_PORT_UNREACH / ICMP_TIME_EXCEEDED
ICMPRP_DTYPE = np.dtype([("frame_off", "<u8"), ("hdr", "<u4"), ("frame_cap", "<u4"), ("kind", "u1"), ("rsv", "u1", 7)])
ICMP_ECHO_REPLY, ICMP_PORT_UNREACH, ICMP_TIME_EXCEEDED = 1, 2, 3

# Every symbol include/vpcsum.h declares (tests check the .so exports all of them).
EXPORTS = [
    "vpcsum_abi_version", "vpcsum_last_error", "vpcsum_device_count", "vpcsum_set_device",
    "vpcsum_compute_async", "vpcsum_nat4_async", "vpcsum_nat_async", "vpcsum_parse_ether_async",
    "vpcsum_parse_ether_tuples_async", "vpcsum_read_probe_async",
    "vpcsum_pattern_probe_async", "vpcsum_nat4_pattern_probe_async", "vpcsum_nat4r_async",
    "vpcsum_nat4r_pattern_probe_async",
    "vpcsum_synth_async", "vpcsum_event_create", "vpcsum_event_destroy", "vpcsum_event_record",
    "vpcsum_event_elapsed_ms", "vpcsum_stream_sync", "vpcsum_ctx_create", "vpcsum_ctx_destroy",
    "vpcsum_ctx_register_arena", "vpcsum_ctx_unregister_arena", "vpcsum_ctx_submit", "vpcsum_ctx_wait",
    "vpcsum_ctx_pipeline", "vpcsum_ctx_set_service", "vpcsum_ctx_stats", "vpcsum_ctx_verify_frames",
    "vpcsum_ctx_parse_frames", "vpcsum_ctx_egress_frames", "Java_io_vproxy_vpcsum_VPCsum_egressFrames",
    "vpcsum_ctx_nat_submit", "Java_io_vproxy_vpcsum_VPCsum_natSubmit",
    "vpcsum_group_create", "vpcsum_group_create_list", "vpcsum_group_destroy", "vpcsum_group_register_arena",
    "vpcsum_group_unregister_arena", "vpcsum_group_submit", "vpcsum_group_wait", "vpcsum_group_nat_submit",
    "vpcsum_init", "vpcsum_shutdown", "vpcsum_register_arena", "vpcsum_batch_submit", "vpcsum_nat_submit",
    "vpcsum_batch_wait", "vpcsum_pre_async", "vpcsum_ctx_submit_pre", "vpcsum_group_submit_pre",
    "vpcsum_batch_submit_pre", "Java_io_vproxy_vpcsum_VPCsum_submitPre",
    "Java_io_vproxy_vpcsum_VPCsum_create", "Java_io_vproxy_vpcsum_VPCsum_registerArena",
    "Java_io_vproxy_vpcsum_VPCsum_submit", "Java_io_vproxy_vpcsum_VPCsum_waitFor",
    "Java_io_vproxy_vpcsum_VPCsum_close", "Java_io_vproxy_vpcsum_VPCsum_setService",
    "Java_io_vproxy_vpcsum_VPCsum_verifyFrames", "Java_io_vproxy_vpcsum_VPCsum_parseFrames",
    "vpcsum_ctx_verify_frames_hsum", "vpcsum_parse_ether_hsum_async", "Java_io_vproxy_vpcsum_VPCsum_verifyFramesHsum",
    "vpcsum_spin_probe_async", "vpcsum_pipe_create", "vpcsum_pipe_begin", "vpcsum_pipe_compute_async",
    "vpcsum_pipe_join", "vpcsum_pipe_destroy",
    "vpcsum_flowtab_create", "vpcsum_flowtab_destroy", "vpcsum_flowtab_update", "vpcsum_flowtab_info",
    "vpcsum_flow_hash", "vpcsum_flow_lookup_async", "vpcsum_flowtab_collect", "vpcsum_ctx_nat_flow_frames",
    "Java_io_vproxy_vpcsum_VPCsum_flowtabCreate", "Java_io_vproxy_vpcsum_VPCsum_flowtabUpdate",
    "Java_io_vproxy_vpcsum_VPCsum_flowtabCollect", "Java_io_vproxy_vpcsum_VPCsum_flowtabClose",
    "Java_io_vproxy_vpcsum_VPCsum_natFlowFrames",
    "vpcsum_flowtab_set_fastpath", "vpcsum_flow_lookup_fp_async", "vpcsum_l2_forward_async",
    "vpcsum_ctx_nat_flow_forward_frames", "Java_io_vproxy_vpcsum_VPCsum_flowtabSetFastpath",
    "Java_io_vproxy_vpcsum_VPCsum_natFlowForwardFrames",
    "vpcsum_tcp_build_async", "vpcsum_ctx_build_tcp_frames", "Java_io_vproxy_vpcsum_VPCsum_buildTcpFrames",
    "vpcsum_tcp_recv_async", "vpcsum_tcp_digest_async", "vpcsum_ctx_recv_tcp_frames",
    "Java_io_vproxy_vpcsum_VPCsum_recvTcpFrames",
    "vpcsum_tcp_build_bursts_async", "vpcsum_ctx_build_tcp_bursts", "Java_io_vproxy_vpcsum_VPCsum_buildTcpBursts",
    "vpcsum_udp_build_async", "vpcsum_udp_recv_async", "vpcsum_ctx_build_udp_frames", "vpcsum_ctx_recv_udp_frames",
    "Java_io_vproxy_vpcsum_VPCsum_buildUdpFrames", "Java_io_vproxy_vpcsum_VPCsum_recvUdpFrames",
    "vpcsum_icmp_reply_async", "vpcsum_ctx_reply_icmp_frames", "Java_io_vproxy_vpcsum_VPCsum_replyIcmpFrames",
]

# additive entry points this binding probes for instead of requiring (see _declare)
_PROBED = ("vpcsum_tcp_recv_async", "vpcsum_tcp_digest_async", "vpcsum_ctx_recv_tcp_frames",
           "vpcsum_tcp_build_bursts_async", "vpcsum_ctx_build_tcp_bursts",
           "vpcsum_udp_build_async", "vpcsum_udp_recv_async", "vpcsum_ctx_build_udp_frames", "vpcsum_ctx_recv_udp_frames",
           "vpcsum_icmp_reply_async", "vpcsum_ctx_reply_icmp_frames")


class VpcsumUnavailable(RuntimeError):
    pass


class VpcsumError(RuntimeError):
    pass


_lib = None
_lock = threading.Lock()

# Host ranges this binding page-locked (ptr -> nbytes, counted per registration) and the ranges it
# released since the last `released_ranges(clear=True)`: the GPU tests' audit checks that HIP no
# longer holds a released range as registered (tests/conftest.py, tests/hiputil.py).
_live_regs: dict[int, list[int]] = {}
_released: list[tuple[int, int]] = []
_leaked: list[dict] = []   # arrays of a context / group whose destroy failed: kept alive


# VPCSUM_AUDIT_REGISTRATIONS=1 (the GPU tests set it): right after each release, while the array
# is still referenced, ask HIP whether it still holds the range as page-locked; any that it does is
# recorded in _stale (a registration outliving its release: a later pageable copy from memory
# allocated at those addresses would go through its dead mapping).
_AUDIT = os.environ.get("VPCSUM_AUDIT_REGISTRATIONS") == "1"
_stale: list[tuple[int, int]] = []
_hip = None


class _PtrAttr(ctypes.Structure):   # hipPointerAttribute_t (hip_runtime_api.h)
    _fields_ = [("type", ctypes.c_int), ("device", ctypes.c_int), ("devicePointer", ctypes.c_void_p),
                ("hostPointer", ctypes.c_void_p), ("isManaged", ctypes.c_int), ("allocationFlags", ctypes.c_uint)]


def hip_holds_registered(ptr: int) -> bool:
    """Whether the HIP runtime (the libamdhip64 this process loaded) holds host address `ptr` as
    page-locked memory (hipPointerGetAttributes: hipMemoryTypeHost)."""
    global _hip
    if _hip is None:
        lib()
        path = None
        with open("/proc/self/maps") as f:
            for line in f:
                if "libamdhip64.so" in line:
                    path = line.split()[-1]
                    break
        if path is None:
            raise VpcsumUnavailable("libamdhip64 is not loaded")
        h = ctypes.CDLL(path)
        h.hipPointerGetAttributes.argtypes = [ctypes.POINTER(_PtrAttr), ctypes.c_void_p]
        h.hipPointerGetAttributes.restype = ctypes.c_int
        h.hipGetLastError.restype = ctypes.c_int
        _hip = h
    a = _PtrAttr()
    rc = _hip.hipPointerGetAttributes(ctypes.byref(a), ctypes.c_void_p(ptr))
    _hip.hipGetLastError()   # an unknown pointer leaves hipErrorInvalidValue behind
    return rc == 0 and a.type == 1


def _reg_add(ptr: int, nbytes: int):
    with _lock:
        _live_regs.setdefault(ptr, []).append(nbytes)


def _reg_drop(ptr: int):
    with _lock:
        lst = _live_regs.get(ptr)
        if not lst:
            return
        n = lst.pop()
        _released.append((ptr, n))
        if not lst:
            del _live_regs[ptr]
        covered = any(q <= ptr < q + max(m) for q, m in _live_regs.items())
    if _AUDIT and not covered and any(hip_holds_registered(q) for q in _audit_points(ptr, n)):
        _stale.append((ptr, n))


def _audit_points(ptr: int, n: int, cap: int = 256) -> list[int]:
    """Addresses of a released range HIP is asked about: both ends and one address in every page
    between them (at most `cap`, evenly spread over a larger range)."""
    first, last = ptr, ptr + n - 1
    pages = (last >> 12) - (ptr >> 12) + 1
    step = max(1, -(-pages // cap))
    pts = [first, last]
    pts += [((ptr >> 12) + k) << 12 for k in range(1, pages - 1, step)]
    return pts


def released_ranges(clear: bool = True) -> list[tuple[int, int]]:
    """Ranges released (unregistered, or their context / group destroyed) that no registration of
    this binding covers any more."""
    with _lock:
        out = [(p, n) for p, n in _released
               if not any(q <= p < q + max(m) for q, m in _live_regs.items())]
        if clear:
            _released.clear()
        return out


def _declare(L):
    P, I, U8, U32, U64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint8, ctypes.c_uint32, ctypes.c_uint64
    sig = {
        "vpcsum_abi_version": ([], I),
        "vpcsum_last_error": ([], ctypes.c_char_p),
        "vpcsum_device_count": ([P], I),
        "vpcsum_set_device": ([I], I),
        "vpcsum_compute_async": ([P, U64, P, U32, P, P, U32, P], I),
        "vpcsum_nat4_async": ([P, U64, P, P, U32, P, U32, P], I),
        "vpcsum_nat4r_async": ([P, U64, P, U32, P, U32, P], I),
        "vpcsum_nat4r_pattern_probe_async": ([P, U64, P, U32, P], I),
        "vpcsum_nat_async": ([P, U64, P, P, U32, P, U32, P], I),
        "vpcsum_ctx_nat_submit": ([P, P, U64, P, P, U32, P, U32, P], I),
        "vpcsum_pre_async": ([P, U64, P, P, U32, U32, P, P, U32, P], I),
        "vpcsum_ctx_submit_pre": ([P, P, U64, P, P, U32, U32, P, P, U32, P], I),
        "vpcsum_group_submit_pre": ([P, P, U64, P, P, U32, U32, P, P, U32, P], I),
        "vpcsum_batch_submit_pre": ([P, U64, P, P, U32, U32, P, P, U32, P], I),
        "vpcsum_group_create": ([U64, U64, U32, P], I),
        "vpcsum_group_create_list": ([P, I, U64, U32, P], I),
        "vpcsum_group_destroy": ([P], I),
        "vpcsum_group_register_arena": ([P, P, U64], I),
        "vpcsum_group_unregister_arena": ([P, P], I),
        "vpcsum_group_submit": ([P, P, U64, P, U32, P, P, U32, P], I),
        "vpcsum_group_wait": ([P, U64], I),
        "vpcsum_group_nat_submit": ([P, P, U64, P, P, U32, P, U32, P], I),
        "vpcsum_init": ([U64, U64, U32], I),
        "vpcsum_shutdown": ([], I),
        "vpcsum_register_arena": ([P, U64], I),
        "vpcsum_batch_submit": ([P, U64, P, U32, P, P, U32, P], I),
        "vpcsum_nat_submit": ([P, U64, P, P, U32, P, U32, P], I),
        "vpcsum_batch_wait": ([U64], I),
        "vpcsum_parse_ether_async": ([P, U64, P, P, U32, U8, P, P, P], I),
        "vpcsum_parse_ether_tuples_async": ([P, U64, P, P, U32, U8, P, P, P, P], I),
        "vpcsum_parse_ether_hsum_async": ([P, U64, P, P, U32, U8, P, P, P, P], I),
        "vpcsum_read_probe_async": ([P, U64, P, U32, P], I),
        "vpcsum_pattern_probe_async": ([P, U64, P, U32, P, U32, P], I),
        "vpcsum_nat4_pattern_probe_async": ([P, U64, P, P, U32, P], I),
        "vpcsum_synth_async": ([P, U64, U32, U32, U32, U32, U64, U64, P, P], I),
        "vpcsum_event_create": ([P], I),
        "vpcsum_event_destroy": ([P], I),
        "vpcsum_event_record": ([P, P], I),
        "vpcsum_event_elapsed_ms": ([P, P, P], I),
        "vpcsum_stream_sync": ([P], I),
        "vpcsum_ctx_create": ([I, U64, U32, P], I),
        "vpcsum_ctx_destroy": ([P], I),
        "vpcsum_ctx_register_arena": ([P, P, U64], I),
        "vpcsum_ctx_unregister_arena": ([P, P], I),
        "vpcsum_ctx_set_service": ([P, U32], I),
        "vpcsum_ctx_stats": ([P, P, P], I),
        "vpcsum_ctx_verify_frames": ([P, P, U64, P, P, U32, P, P, P], I),
        "vpcsum_ctx_verify_frames_hsum": ([P, P, U64, P, P, U32, P, P, P, P], I),
        "vpcsum_pipe_create": ([P, P], I),
        "vpcsum_pipe_begin": ([P], I),
        "vpcsum_pipe_compute_async": ([P, P, U64, P, U32, P, P, U32], I),
        "vpcsum_pipe_join": ([P], I),
        "vpcsum_pipe_destroy": ([P], I),
        "vpcsum_spin_probe_async": ([U32, U32, U32, P], I),
        "vpcsum_ctx_parse_frames": ([P, P, U64, P, P, U32, P, P, P, P], I),
        "vpcsum_ctx_egress_frames": ([P, P, U64, P, P, P, U32, P, P, P], I),
        "vpcsum_ctx_submit": ([P, P, U64, P, U32, P, P, U32, P], I),
        "vpcsum_ctx_wait": ([P, U64], I),
        "vpcsum_ctx_pipeline": ([P, P, U32, U32, P, U32, P, U32, U32], I),
        "vpcsum_flowtab_create": ([I, U32, P], I),
        "vpcsum_flowtab_destroy": ([P], I),
        "vpcsum_flowtab_update": ([P, P, U32, P, U32, P], I),
        "vpcsum_flowtab_info": ([P, P, P, P], I),
        "vpcsum_flow_hash": ([P, P], I),
        "vpcsum_flow_lookup_async": ([P, P, U32, P, P, P], I),
        "vpcsum_flowtab_collect": ([P, P, U32, P, P], I),
        "vpcsum_ctx_nat_flow_frames": ([P, P, P, U64, P, P, U32, P, P, U32, P], I),
        "vpcsum_flowtab_set_fastpath": ([P, P, P, U32, P, P], I),
        "vpcsum_flow_lookup_fp_async": ([P, P, U32, P, P, P, P], I),
        "vpcsum_l2_forward_async": ([P, U64, P, P, P, P, P, U32, P, P], I),
        "vpcsum_ctx_nat_flow_forward_frames": ([P, P, P, U64, P, P, U32, P, P, P, U32, P], I),
        "vpcsum_tcp_build_async": ([P, U64, P, U64, P, U32, P, U32, P, P, P, P], I),
        "vpcsum_ctx_build_tcp_frames": ([P, P, U64, P, U64, P, U32, P, U32, P, P, P, P], I),
        "vpcsum_tcp_recv_async": ([P, U64, P, P, U32, P, U64, P, P, P, P], I),
        "vpcsum_tcp_digest_async": ([P, U64, P, U32, P, P], I),
        "vpcsum_ctx_recv_tcp_frames": ([P, P, U64, P, P, U32, P, U64, P, P, P, P], I),
        "vpcsum_tcp_build_bursts_async": ([P, U64, P, U64, P, U32, P, U32, P, U32, U32, P, P, P, P], I),
        "vpcsum_ctx_build_tcp_bursts": ([P, P, U64, P, U64, P, U32, P, U32, P, U32, U32, P, P, P, P], I),
        "vpcsum_udp_build_async": ([P, U64, P, U64, P, U32, P, U32, P, P, P, P], I),
        "vpcsum_ctx_build_udp_frames": ([P, P, U64, P, U64, P, U32, P, U32, P, P, P, P], I),
        "vpcsum_udp_recv_async": ([P, U64, P, P, U32, P, U64, P, P, P, P], I),
        "vpcsum_ctx_recv_udp_frames": ([P, P, U64, P, P, U32, P, U64, P, P, P, P], I),
        "vpcsum_icmp_reply_async": ([P, U64, P, P, U32, P, U32, P, U64, P, P, P, P, P], I),
        "vpcsum_ctx_reply_icmp_frames": ([P, P, U64, P, P, U32, P, U32, P, U64, P, P, P, P, P], I),
    }
    for name, (args, res) in sig.items():
        # The TCP receive, the TCP send bursts, the UDP pair and the ICMP replies came after ABI version 4 was fixed: a
        # caller probes for them by looking the symbols up (include/vpcsum.h).  So does this binding -- it
        # loads a library from before them (tools/ab_libs.sh compares against one), and using tcp_recv(),
        # tcp_build_bursts() or udp_build() on such a library raises ctypes' "undefined symbol", never a fallback.
        if name in _PROBED and not hasattr(L, name):
            continue
        f = getattr(L, name)
        f.argtypes = args
        f.restype = res


def lib():
    """Load libvpcsum.so (after torch, so both share one HIP runtime)."""
    global _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB):
                raise VpcsumUnavailable(f"{LIB} is missing: run `python -m vproxy_amd.build` "
                                        "(there is no CPU fallback)")
            try:
                import torch  # noqa: F401  -- bind torch's libamdhip64 first
            except ImportError:
                pass
            try:
                L = ctypes.CDLL(LIB)
            except OSError as e:
                raise VpcsumUnavailable(f"cannot load {LIB}: {e}") from e
            _declare(L)
            if L.vpcsum_abi_version() != ABI_VERSION:
                raise VpcsumUnavailable("ABI version mismatch")
            _lib = L
        return _lib


def _check(rc: int, what: str):
    if rc != 0:
        msg = lib().vpcsum_last_error()
        raise VpcsumError(f"{what}: {msg.decode() if msg else rc}")


def _ptr(t) -> int | None:
    if t is None:
        return None
    if isinstance(t, np.ndarray):
        return t.ctypes.data
    return t.data_ptr()


def _stream(stream) -> int | None:
    if stream is None:
        import torch
        return torch.cuda.current_stream().cuda_stream
    if isinstance(stream, int):
        return stream
    return stream.cuda_stream


# ------------------------------------------------------------------------------------------
# Device-resident API (torch CUDA tensors)
# ------------------------------------------------------------------------------------------
def _tune_bits(team_log2: int = 0, plain_loads: bool = False, blocks_per_cu: int = 0, full_grid: bool = False) -> int:
    """The compute mode's tuning fields (csrc/launch_modes.h csum_bits; not part of the stable ABI):
    kernel variant id, plain loads, workgroups per CU, no adaptive grid."""
    return ((team_log2 & 0x1F) << 8) | (((team_log2 >> 5) & 0x7) << 24) | (0x2000 if plain_loads else 0) | \
        (0x4000 if full_grid else 0) | ((blocks_per_cu & 0xFF) << 16)


def compute(arena, desc, n: int | None = None, out=None, status=None, mode: int = MODE_COMPUTE,
            team_log2: int = 0, stream=None, plain_loads: bool = False, blocks_per_cu: int = 0,
            full_grid: bool = False):
    """Checksum a device-resident batch.  `arena` uint8 tensor, `desc` tensor holding n
    16-byte vpcsum_desc_t, `out` int32/uint32 tensor (n), `status` uint8 tensor (n)."""
    if n is None:
        n = desc.numel() * desc.element_size() // 16
    m = mode | _tune_bits(team_log2, plain_loads, blocks_per_cu, full_grid)
    _check(lib().vpcsum_compute_async(_ptr(arena), arena.numel(), _ptr(desc), n, _ptr(out), _ptr(status), m,
                                      _stream(stream)), "vpcsum_compute_async")


def nat4(arena, desc, rw, n: int, status=None, nat_mode: int = NAT_RFC1624, stream=None):
    _check(lib().vpcsum_nat4_async(_ptr(arena), arena.numel(), _ptr(desc), _ptr(rw), n, _ptr(status), nat_mode,
                                   _stream(stream)), "vpcsum_nat4_async")


def nat(arena, desc, rw, n: int, status=None, nat_mode: int = NAT_RFC1624, stream=None):
    """NAT / TTL rewrite with 48-B vpcsum_nat_t entries (IPv4 and IPv6): `rw` a uint8 tensor of n x 48."""
    _check(lib().vpcsum_nat_async(_ptr(arena), arena.numel(), _ptr(desc), _ptr(rw), n, _ptr(status), nat_mode,
                                  _stream(stream)), "vpcsum_nat_async")


def nat_tcp_fill(entry, seq_add: int | None = None, flags: int | None = None, max_mss: int | None = None):
    """Fill the TCP part of one NAT_DTYPE entry (`entry`: rw[i]): seq_add the sequence addend (any
    sign, taken mod 2^32: seq - N is -N), flags the new TCP flags (low 6 bits), max_mss the MSS
    clamp of a SYN; None leaves that rewrite out.  Sets NAT_TCP in the mask; the batch needs the
    NAT_TCP_REWRITES mode bit."""
    ops = (TCP_SEQ_ADD if seq_add is not None else 0) | (TCP_SET_FLAGS if flags is not None else 0) | \
          (TCP_CLAMP_MSS if max_mss is not None else 0)
    rsv = bytes([ops, (flags or 0) & 0x3F]) + ((max_mss or 0) & 0xFFFF).to_bytes(2, "big") + \
        ((seq_add or 0) & 0xFFFFFFFF).to_bytes(4, "big") + b"\x00\x00"
    entry["rsv"] = np.frombuffer(rsv, np.uint8)
    entry["mask"] = int(entry["mask"]) | NAT_TCP


def pre(arena, desc, pre_img, n: int, out=None, status=None, mode: int = MODE_WRITE, pre_fmt: int = PRE_FMT_PRE4,
        stream=None):
    """vpcsum_pre_async: the sums of the F_PRE descriptors from their pre-images (`pre_img`: n
    entries, NAT4_DTYPE bytes for PRE_FMT_PRE4 or NAT_DTYPE for PRE_FMT_PRE, holding the OLD
    addresses / ports); descriptors without F_PRE are left alone (run `compute` for them first)."""
    _check(lib().vpcsum_pre_async(_ptr(arena), arena.numel(), _ptr(desc), _ptr(pre_img), pre_fmt, n, _ptr(out),
                                  _ptr(status), mode, _stream(stream)), "vpcsum_pre_async")


def parse_ether(arena, frame_off, frame_len, n: int, desc, status=None, flags: int = F_IP | F_L4, stream=None,
                tuples=None, hsum=None):
    """Descriptors from raw frames on the GPU; with `tuples` (n x 40 bytes, TUPLE_DTYPE) also each
    frame's flow tuple (vpcsum_parse_ether_tuples_async); with `hsum` (n x 8 bytes, HSUM_DTYPE) each
    frame's ingress header sum instead (vpcsum_parse_ether_hsum_async)."""
    if hsum is not None:
        assert tuples is None and hsum.numel() * hsum.element_size() >= n * HSUM_DTYPE.itemsize
        _check(lib().vpcsum_parse_ether_hsum_async(_ptr(arena), arena.numel(), _ptr(frame_off), _ptr(frame_len), n,
                                                   flags, _ptr(desc), _ptr(status), _ptr(hsum), _stream(stream)),
               "vpcsum_parse_ether_hsum_async")
        return
    if tuples is None:
        _check(lib().vpcsum_parse_ether_async(_ptr(arena), arena.numel(), _ptr(frame_off), _ptr(frame_len), n, flags,
                                              _ptr(desc), _ptr(status), _stream(stream)), "vpcsum_parse_ether_async")
        return
    assert tuples.numel() * tuples.element_size() >= n * TUPLE_DTYPE.itemsize
    _check(lib().vpcsum_parse_ether_tuples_async(_ptr(arena), arena.numel(), _ptr(frame_off), _ptr(frame_len), n,
                                                 flags, _ptr(desc), _ptr(status), _ptr(tuples), _stream(stream)),
           "vpcsum_parse_ether_tuples_async")


def pattern_probe(arena, desc, n: int, sink, grid: int = 0, stream=None):
    """Read exactly the chunks the checksum kernel reads for `desc`, no checksum work (tooling)."""
    assert sink.numel() * sink.element_size() >= 4096, "sink needs 1024 words"
    _check(lib().vpcsum_pattern_probe_async(_ptr(arena), arena.numel(), _ptr(desc), n, _ptr(sink), grid,
                                            _stream(stream)), "vpcsum_pattern_probe_async")


def nat4r(arena, rec, n: int, status=None, nat_mode: int = NAT_RFC1624, stream=None):
    """vpcsum_nat4r_async: `rec` holds n NAT4R_DTYPE records (descriptor + IPv4 entry)."""
    _check(lib().vpcsum_nat4r_async(_ptr(arena), arena.numel(), _ptr(rec), n, _ptr(status), nat_mode, _stream(stream)),
           "vpcsum_nat4r_async")


def nat4r_pattern_probe(arena, rec, n: int, stream=None):
    _check(lib().vpcsum_nat4r_pattern_probe_async(_ptr(arena), arena.numel(), _ptr(rec), n, _stream(stream)),
           "vpcsum_nat4r_pattern_probe_async")


def nat4_pattern_probe(arena, desc, rw, n: int, stream=None):
    """NAT's memory operations for `desc` / `rw` (16-B entries) with no rewrite (tooling)."""
    _check(lib().vpcsum_nat4_pattern_probe_async(_ptr(arena), arena.numel(), _ptr(desc), _ptr(rw), n,
                                                 _stream(stream)), "vpcsum_nat4_pattern_probe_async")


def read_probe(buf, nbytes: int, sink, grid: int = 0, stream=None):
    _check(lib().vpcsum_read_probe_async(_ptr(buf), nbytes, _ptr(sink), grid, _stream(stream)),
           "vpcsum_read_probe_async")


def synth(arena, n: int, stride: int, l3_pad: int, workload: int, seed: int, first_index: int = 0,
          desc=None, stream=None):
    """arena None: the descriptors alone (desc required)."""
    _check(lib().vpcsum_synth_async(_ptr(arena) if arena is not None else None, arena.numel() if arena is not None else 0,
                                    n, stride, l3_pad, workload, seed, first_index, _ptr(desc), _stream(stream)),
           "vpcsum_synth_async")


class Pipe:
    """Two batches in flight on the device API (vpcsum_pipe_*): `begin()` forks the pipe's two
    streams from `stream`, `compute()` launches alternate between them (consecutive batches may run
    concurrently: their outputs must not overlap), `join()` makes `stream` wait for all of them."""

    def __init__(self, stream=None):
        h = ctypes.c_void_p()
        _check(lib().vpcsum_pipe_create(_stream(stream), ctypes.byref(h)), "vpcsum_pipe_create")
        self.h = h.value

    def begin(self):
        _check(lib().vpcsum_pipe_begin(self.h), "vpcsum_pipe_begin")

    def compute(self, arena, desc, n: int | None = None, out=None, status=None, mode: int = MODE_COMPUTE,
                team_log2: int = 0):
        if n is None:
            n = desc.numel() * desc.element_size() // 16
        m = mode | _tune_bits(team_log2)
        _check(lib().vpcsum_pipe_compute_async(self.h, _ptr(arena), arena.numel(), _ptr(desc), n, _ptr(out),
                                               _ptr(status), m), "vpcsum_pipe_compute_async")

    def join(self):
        _check(lib().vpcsum_pipe_join(self.h), "vpcsum_pipe_join")

    def close(self):
        if self.h:
            lib().vpcsum_pipe_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Event:
    """HIP event recorded on an arbitrary (e.g. the kernel's) stream."""

    def __init__(self):
        h = ctypes.c_void_p()
        _check(lib().vpcsum_event_create(ctypes.byref(h)), "vpcsum_event_create")
        self.h = h.value

    def record(self, stream=None):
        _check(lib().vpcsum_event_record(self.h, _stream(stream)), "vpcsum_event_record")

    def elapsed_ms(self, end: "Event") -> float:
        ms = ctypes.c_float()
        _check(lib().vpcsum_event_elapsed_ms(self.h, end.h, ctypes.byref(ms)), "vpcsum_event_elapsed_ms")
        return ms.value

    def __del__(self):
        try:
            if _lib is not None and self.h:
                _lib.vpcsum_event_destroy(self.h)
        except Exception:
            pass


def flow_hash(key) -> int:
    """vpcsum_flow_hash of one TUPLE_DTYPE key (tcp_flags / rsv are not read): a table of `slots`
    slots keeps the key at or after slot hash & (slots - 1)."""
    k = np.ascontiguousarray(np.asarray(key, TUPLE_DTYPE).reshape(1))
    h = ctypes.c_uint64()
    _check(lib().vpcsum_flow_hash(k.ctypes.data, ctypes.byref(h)), "vpcsum_flow_hash")
    return h.value


def l2_forward(arena, frame_off, frame_len, verdict, status, fastpath, n: int, port, stream=None):
    """vpcsum_l2_forward_async on device tensors: `arena` uint8, `frame_off` n x uint64, `frame_len`
    n x uint32, `verdict` / `status` n bytes, `fastpath` n x 16 bytes, `port` n x uint32 (written).
    A frame gets its record's addresses in bytes [0,12) and its port only when its verdict is
    FLOW_HIT, its status S_DONE without S_BAD_DESC and the record's port not 0."""
    assert verdict.numel() >= n and status.numel() >= n
    assert frame_off.numel() * frame_off.element_size() >= n * 8 and frame_len.numel() * frame_len.element_size() >= n * 4
    assert fastpath.numel() * fastpath.element_size() >= n * FASTPATH_DTYPE.itemsize
    assert port.numel() * port.element_size() >= n * 4
    _check(lib().vpcsum_l2_forward_async(_ptr(arena), arena.numel() * arena.element_size(), _ptr(frame_off), _ptr(frame_len),
                                         _ptr(verdict), _ptr(status), _ptr(fastpath), n, _ptr(port), _stream(stream)),
           "vpcsum_l2_forward_async")


def tcp_build(dst, src, hdrs, n_hdr: int, segs, n: int, frame_len, out=None, status=None, stream=None):
    """vpcsum_tcp_build_async on device tensors: `dst` / `src` uint8 arenas, `hdrs` n_hdr x 64 bytes
    (TCPHDR_DTYPE), `segs` n x 32 bytes (TCPSEG_DTYPE), `frame_len` n x uint32 (written: L, or 0 for a
    refused record), `out` n x uint32 and `status` n bytes (each may be None).  Frame i is built at
    dst + frame_off from its template and the payload at src + data_off, sums included."""
    assert hdrs.numel() * hdrs.element_size() >= n_hdr * TCPHDR_DTYPE.itemsize
    assert segs.numel() * segs.element_size() >= n * TCPSEG_DTYPE.itemsize
    assert frame_len.numel() * frame_len.element_size() >= n * 4
    assert out is None or out.numel() * out.element_size() >= n * 4
    assert status is None or status.numel() >= n
    _check(lib().vpcsum_tcp_build_async(_ptr(dst), dst.numel() * dst.element_size(), _ptr(src),
                                        src.numel() * src.element_size(), _ptr(hdrs), n_hdr, _ptr(segs), n, _ptr(frame_len),
                                        _ptr(out), _ptr(status), _stream(stream)), "vpcsum_tcp_build_async")


def tcp_build_bursts(dst, src, hdrs, n_hdr: int, bursts, n_bursts: int, frame_off, n_frames: int, frame_cap: int, frame_len,
                     out=None, status=None, stream=None):
    """vpcsum_tcp_build_bursts_async on device tensors: tcp_build() with one record per fetch().
    `bursts` n_bursts x 32 bytes (TCPBURST_DTYPE, `first` non-decreasing), `frame_off` n_frames x uint64,
    `frame_cap` the room at every frame; frame j is piece j - first of the last burst that starts at or
    before it, cut on the device.  `frame_len` / `out` / `status` are per frame, as tcp_build() writes them."""
    assert hdrs.numel() * hdrs.element_size() >= n_hdr * TCPHDR_DTYPE.itemsize
    assert bursts.numel() * bursts.element_size() >= n_bursts * TCPBURST_DTYPE.itemsize
    assert frame_off.numel() * frame_off.element_size() >= n_frames * 8
    assert frame_len.numel() * frame_len.element_size() >= n_frames * 4
    assert out is None or out.numel() * out.element_size() >= n_frames * 4
    assert status is None or status.numel() >= n_frames
    _check(lib().vpcsum_tcp_build_bursts_async(_ptr(dst), dst.numel() * dst.element_size(), _ptr(src),
                                               src.numel() * src.element_size(), _ptr(hdrs), n_hdr, _ptr(bursts), n_bursts,
                                               _ptr(frame_off), n_frames, frame_cap, _ptr(frame_len), _ptr(out), _ptr(status),
                                               _stream(stream)), "vpcsum_tcp_build_bursts_async")


def tcp_recv(arena, desc, rx, n: int, dst, stored, out=None, status=None, stream=None):
    """vpcsum_tcp_recv_async on device tensors: `arena` the received frames, `desc` n x 16 bytes (the
    parse's descriptors), `rx` n x 16 bytes (TCPRX_DTYPE), `dst` the uint8 receive arena, `stored`
    n x uint32 (written: the bytes stored, 0 for a refused or verify-only record), `out` n x uint32 and
    `status` n bytes (each may be None; what compute() writes with MODE_VERIFY).  The payload bytes
    are stored whatever the verdict: accept them on S_L4_OK only."""
    assert desc.numel() * desc.element_size() >= n * 16 and rx.numel() * rx.element_size() >= n * TCPRX_DTYPE.itemsize
    assert stored.numel() * stored.element_size() >= n * 4
    assert out is None or out.numel() * out.element_size() >= n * 4
    assert status is None or status.numel() >= n
    _check(lib().vpcsum_tcp_recv_async(_ptr(arena), arena.numel() * arena.element_size(), _ptr(desc), _ptr(rx), n, _ptr(dst),
                                       dst.numel() * dst.element_size(), _ptr(stored), _ptr(out), _ptr(status),
                                       _stream(stream)), "vpcsum_tcp_recv_async")


def tcp_digest(arena, desc, n: int, info, stream=None):
    """vpcsum_tcp_digest_async on device tensors: `info` n x 16 bytes (TCPINFO_DTYPE, 16-byte aligned),
    written from the TCP header's first 16 bytes of each descriptor; all zero for a refused one."""
    assert desc.numel() * desc.element_size() >= n * 16 and info.numel() * info.element_size() >= n * TCPINFO_DTYPE.itemsize
    _check(lib().vpcsum_tcp_digest_async(_ptr(arena), arena.numel() * arena.element_size(), _ptr(desc), n, _ptr(info),
                                         _stream(stream)), "vpcsum_tcp_digest_async")


def udp_build(dst, src, hdrs, n_hdr: int, dgs, n: int, frame_len, out=None, status=None, stream=None):
    """vpcsum_udp_build_async on device tensors: tcp_build() for datagrams.  `hdrs` n_hdr x 64 bytes
    (TCPHDR_DTYPE with ack / window / rsv 0), `dgs` n x 32 bytes (UDPDG_DTYPE), `frame_len` n x uint32
    (written: L, or 0 for a refused record), `out` n x uint32 and `status` n bytes (each may be None).
    A UDP sum that computes to 0 is stored as 0xffff."""
    assert hdrs.numel() * hdrs.element_size() >= n_hdr * TCPHDR_DTYPE.itemsize
    assert dgs.numel() * dgs.element_size() >= n * UDPDG_DTYPE.itemsize
    assert frame_len.numel() * frame_len.element_size() >= n * 4
    assert out is None or out.numel() * out.element_size() >= n * 4
    assert status is None or status.numel() >= n
    _check(lib().vpcsum_udp_build_async(_ptr(dst), dst.numel() * dst.element_size(), _ptr(src),
                                        src.numel() * src.element_size(), _ptr(hdrs), n_hdr, _ptr(dgs), n, _ptr(frame_len),
                                        _ptr(out), _ptr(status), _stream(stream)), "vpcsum_udp_build_async")


def udp_recv(arena, desc, rx, n: int, dst, stored, out=None, status=None, stream=None):
    """vpcsum_udp_recv_async on device tensors: tcp_recv() for datagrams.  `rx` n x 16 bytes
    (UDPRX_DTYPE); `stored` n x uint32 (written: the segment's bytes past its 8-byte header, 0 for a
    refused or verify-only record); `out` / `status` (each may be None) what compute() writes with
    MODE_VERIFY, S_UDP_NOCSUM included.  The bytes are stored whatever the verdict."""
    assert desc.numel() * desc.element_size() >= n * 16 and rx.numel() * rx.element_size() >= n * UDPRX_DTYPE.itemsize
    assert stored.numel() * stored.element_size() >= n * 4
    assert out is None or out.numel() * out.element_size() >= n * 4
    assert status is None or status.numel() >= n
    _check(lib().vpcsum_udp_recv_async(_ptr(arena), arena.numel() * arena.element_size(), _ptr(desc), _ptr(rx), n, _ptr(dst),
                                       dst.numel() * dst.element_size(), _ptr(stored), _ptr(out), _ptr(status),
                                       _stream(stream)), "vpcsum_udp_recv_async")


def icmp_reply(arena, desc, hdrs, n_hdr: int, rps, n: int, dst, frame_len, csum=None, out=None, status=None, stream=None):
    """vpcsum_icmp_reply_async on device tensors: the ICMP reply to each descriptor of `arena` -- echo
    reply, port unreachable or time exceeded, as rps[i].kind says -- written into `dst` as a finished
    Ethernet / IP / ICMP frame.  `hdrs` n_hdr x 64 bytes (TCPHDR_DTYPE with ports / ack / window / rsv
    0), `rps` n x 24 bytes (ICMPRP_DTYPE), `frame_len` n x uint32 (written: L, or 0 for a refused
    record), `csum` n x uint32 (the reply's sums), `out` n x uint32 and `status` n bytes (an echo: what
    compute() writes for the request with MODE_VERIFY; an error: 0 and S_DONE); each of the last three
    may be None.  `dst` may be `arena`.  An echo reply is written whatever the request's verdict."""
    assert desc.numel() * desc.element_size() >= n * 16 and rps.numel() * rps.element_size() >= n * ICMPRP_DTYPE.itemsize
    assert hdrs.numel() * hdrs.element_size() >= n_hdr * TCPHDR_DTYPE.itemsize
    assert frame_len.numel() * frame_len.element_size() >= n * 4
    assert csum is None or csum.numel() * csum.element_size() >= n * 4
    assert out is None or out.numel() * out.element_size() >= n * 4
    assert status is None or status.numel() >= n
    _check(lib().vpcsum_icmp_reply_async(_ptr(arena), arena.numel() * arena.element_size(), _ptr(desc), _ptr(hdrs), n_hdr,
                                         _ptr(rps), n, _ptr(dst), dst.numel() * dst.element_size(), _ptr(frame_len),
                                         _ptr(csum), _ptr(out), _ptr(status), _stream(stream)), "vpcsum_icmp_reply_async")


class FlowTable:
    """The NAT flow table on one device (vpcsum_flowtab_*): TUPLE_DTYPE key -> NAT_DTYPE rewrite,
    updated from the host, looked up on the GPU (lookup, Context.nat_flow_frames)."""

    def __init__(self, max_flows: int, device: int = 0):
        h = ctypes.c_void_p()
        _check(lib().vpcsum_flowtab_create(device, max_flows, ctypes.byref(h)), "vpcsum_flowtab_create")
        self.h = h.value
        self.device = device

    def update(self, delete=None, add=None, stream=None):
        """Erase the TUPLE_DTYPE keys `delete`, then insert / replace the FLOW_DTYPE flows `add`;
        returns once the device table holds them (ordered on `stream`).  A refused flow raises and
        changes nothing."""
        d = np.zeros(0, TUPLE_DTYPE) if delete is None else np.ascontiguousarray(np.asarray(delete, TUPLE_DTYPE).reshape(-1))
        a = np.zeros(0, FLOW_DTYPE) if add is None else np.ascontiguousarray(np.asarray(add, FLOW_DTYPE).reshape(-1))
        _check(lib().vpcsum_flowtab_update(self.h, d.ctypes.data if len(d) else None, len(d),
                                           a.ctypes.data if len(a) else None, len(a), _stream(stream)),
               "vpcsum_flowtab_update")

    def set_fastpath(self, keys, fps, stream=None) -> int:
        """vpcsum_flowtab_set_fastpath: the Fastpath of each TUPLE_DTYPE key present becomes its
        FASTPATH_DTYPE record (port 0 clears it); returns how many keys were not in the table.  A
        malformed key raises and changes nothing.  Ordered on `stream` as update."""
        k = np.ascontiguousarray(np.asarray(keys, TUPLE_DTYPE).reshape(-1))
        f = np.ascontiguousarray(np.asarray(fps, FASTPATH_DTYPE).reshape(-1))
        assert len(k) == len(f)
        missing = ctypes.c_uint32()
        _check(lib().vpcsum_flowtab_set_fastpath(self.h, k.ctypes.data if len(k) else None, f.ctypes.data if len(f) else None,
                                                 len(k), ctypes.byref(missing), _stream(stream)),
               "vpcsum_flowtab_set_fastpath")
        return missing.value

    def lookup(self, tuples, n: int, rw, verdict, stream=None, fastpath=None):
        """vpcsum_flow_lookup_async: `tuples` n x 40 bytes, `rw` n x 48 bytes and `verdict` n bytes,
        uint8 device tensors.  With `fastpath` (n x 16 bytes) vpcsum_flow_lookup_fp_async: each
        flow's FASTPATH_DTYPE record too (fastpath=True: a new tensor, which is returned)."""
        assert tuples.numel() * tuples.element_size() >= n * TUPLE_DTYPE.itemsize
        assert rw.numel() * rw.element_size() >= n * NAT_DTYPE.itemsize and verdict.numel() >= n
        if fastpath is None or fastpath is False:
            _check(lib().vpcsum_flow_lookup_async(self.h, _ptr(tuples), n, _ptr(rw), _ptr(verdict), _stream(stream)),
                   "vpcsum_flow_lookup_async")
            return None
        if fastpath is True:
            import torch
            fastpath = torch.zeros(max(n, 1) * FASTPATH_DTYPE.itemsize, dtype=torch.uint8, device=verdict.device)
        assert fastpath.numel() * fastpath.element_size() >= n * FASTPATH_DTYPE.itemsize
        _check(lib().vpcsum_flow_lookup_fp_async(self.h, _ptr(tuples), n, _ptr(rw), _ptr(verdict), _ptr(fastpath),
                                                 _stream(stream)), "vpcsum_flow_lookup_fp_async")
        return fastpath

    def collect(self, cap: int | None = None, stream=None):
        """Cookies of the flows hit since the last collect (marks cleared).  With `cap`, a count
        above it is returned as (count, None) and nothing is cleared."""
        room = self.info()["flows"] if cap is None else cap
        out = np.zeros(max(room, 1), np.uint64)
        n = ctypes.c_uint32()
        _check(lib().vpcsum_flowtab_collect(self.h, out.ctypes.data, room, ctypes.byref(n), _stream(stream)),
               "vpcsum_flowtab_collect")
        if cap is None:
            return out[:n.value].copy()
        return n.value, (out[:n.value].copy() if n.value <= cap else None)

    def info(self) -> dict:
        s, f, m = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        _check(lib().vpcsum_flowtab_info(self.h, ctypes.byref(s), ctypes.byref(f), ctypes.byref(m)), "vpcsum_flowtab_info")
        return {"slots": s.value, "flows": f.value, "max_probe": m.value}

    def close(self):
        if self.h:
            lib().vpcsum_flowtab_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ------------------------------------------------------------------------------------------
# Host-memory API (what the Java binding drives)
# ------------------------------------------------------------------------------------------
class Context:
    def __init__(self, device: int = 0, max_arena: int = 1 << 26, max_pkts: int = 1 << 16):
        h = ctypes.c_void_p()
        _check(lib().vpcsum_ctx_create(device, max_arena, max_pkts, ctypes.byref(h)), "vpcsum_ctx_create")
        self.h = h.value
        # numpy buffers the library holds raw pointers to: registered arrays (until unregister /
        # close) and the buffers of the batch in flight on each of the context's two slots
        self._pinned = {}
        self._inflight = {}

    def register(self, arr: np.ndarray):
        _check(lib().vpcsum_ctx_register_arena(self.h, arr.ctypes.data, arr.nbytes), "vpcsum_ctx_register_arena")
        self._pinned[arr.ctypes.data] = arr
        _reg_add(arr.ctypes.data, arr.nbytes)

    def unregister(self, arr: np.ndarray):
        _check(lib().vpcsum_ctx_unregister_arena(self.h, arr.ctypes.data), "vpcsum_ctx_unregister_arena")
        self._pinned.pop(arr.ctypes.data, None)
        _reg_drop(arr.ctypes.data)

    def submit(self, arena: np.ndarray, desc: np.ndarray, out: np.ndarray | None, status: np.ndarray | None = None,
               mode: int = MODE_COMPUTE) -> int:
        """out None: no out words (a verify whose result is the status bytes)."""
        t = ctypes.c_uint64()
        _check(lib().vpcsum_ctx_submit(self.h, arena.ctypes.data, arena.nbytes, desc.ctypes.data, len(desc),
                                       None if out is None else out.ctypes.data,
                                       None if status is None else status.ctypes.data, mode,
                                       ctypes.byref(t)), "vpcsum_ctx_submit")
        self._inflight[t.value & 1] = (arena, desc, out, status)
        return t.value

    def wait(self, ticket: int):
        _check(lib().vpcsum_ctx_wait(self.h, ticket), "vpcsum_ctx_wait")

    def submit_pre(self, arena: np.ndarray, desc: np.ndarray, pre_img: np.ndarray, out: np.ndarray,
                   status: np.ndarray | None = None, mode: int = MODE_COMPUTE) -> int:
        """vpcsum_ctx_submit_pre: F_PRE descriptors take their L4 sum from pre_img[i] (NAT_DTYPE or
        NAT4_DTYPE entries, old values), the others are summed in full; one submission."""
        fmt = PRE_FMT_PRE if pre_img.dtype == NAT_DTYPE else PRE_FMT_PRE4
        assert pre_img.dtype in (NAT_DTYPE, NAT4_DTYPE) and len(pre_img) >= len(desc)
        t = ctypes.c_uint64()
        _check(lib().vpcsum_ctx_submit_pre(self.h, arena.ctypes.data, arena.nbytes, desc.ctypes.data,
                                           pre_img.ctypes.data, fmt, len(desc), out.ctypes.data,
                                           None if status is None else status.ctypes.data, mode, ctypes.byref(t)),
               "vpcsum_ctx_submit_pre")
        self._inflight[t.value & 1] = (arena, desc, pre_img, out, status)
        return t.value

    def run_pre(self, arena, desc, pre_img, mode: int = MODE_COMPUTE):
        out = np.zeros(len(desc), np.uint32)
        status = np.zeros(len(desc), np.uint8)
        self.wait(self.submit_pre(arena, desc, pre_img, out, status, mode))
        return out, status

    def verify_frames(self, arena: np.ndarray, frame_off: np.ndarray, frame_len: np.ndarray, sums: bool = True):
        """Ingress verify of received Ethernet frames in a registered arena: parsed and verified
        on the GPU in one submission.  Returns (out, status) per frame; sums=False: (None, status),
        the kernel writes no out words (GpuCsumBatch.verifyFrames' form)."""
        n = len(frame_off)
        fo = np.ascontiguousarray(frame_off, dtype=np.uint64)
        fl = np.ascontiguousarray(frame_len, dtype=np.uint32)
        out = np.zeros(n, np.uint32) if sums else None
        status = np.zeros(n, np.uint8)
        t = ctypes.c_uint64()
        _check(lib().vpcsum_ctx_verify_frames(self.h, arena.ctypes.data, arena.nbytes, fo.ctypes.data, fl.ctypes.data,
                                              n, None if out is None else out.ctypes.data, status.ctypes.data,
                                              ctypes.byref(t)),
               "vpcsum_ctx_verify_frames")
        self.wait(t.value)
        return out, status

    def verify_frames_hsum(self, arena: np.ndarray, frame_off: np.ndarray, frame_len: np.ndarray):
        """verify_frames(sums=False) that also records each frame's ingress header sum
        (vpcsum_ctx_verify_frames_hsum, GpuCsumBatch.verifyFrames' form since ABI 4).  Returns
        (status, hsum): S_* bytes and HSUM_DTYPE records per frame."""
        n = len(frame_off)
        fo = np.ascontiguousarray(frame_off, dtype=np.uint64)
        fl = np.ascontiguousarray(frame_len, dtype=np.uint32)
        status = np.zeros(n, np.uint8)
        hsum = np.zeros(n, HSUM_DTYPE)
        t = ctypes.c_uint64()
        _check(lib().vpcsum_ctx_verify_frames_hsum(self.h, arena.ctypes.data, arena.nbytes, fo.ctypes.data,
                                                   fl.ctypes.data, n, None, status.ctypes.data, hsum.ctypes.data,
                                                   ctypes.byref(t)), "vpcsum_ctx_verify_frames_hsum")
        self.wait(t.value)
        return status, hsum

    def parse_frames(self, arena: np.ndarray, frame_off: np.ndarray, frame_len: np.ndarray):
        """Batched parse of received Ethernet frames in a registered arena, with flow tuples
        (vpcsum_ctx_parse_frames).  Returns (descriptors, status, tuples) per frame."""
        n = len(frame_off)
        fo = np.ascontiguousarray(frame_off, dtype=np.uint64)
        fl = np.ascontiguousarray(frame_len, dtype=np.uint32)
        desc = np.zeros(n, DESC_DTYPE)
        status = np.zeros(n, np.uint8)
        tuples = np.zeros(n, TUPLE_DTYPE)
        t = ctypes.c_uint64()
        _check(lib().vpcsum_ctx_parse_frames(self.h, arena.ctypes.data, arena.nbytes, fo.ctypes.data, fl.ctypes.data,
                                             n, desc.ctypes.data, status.ctypes.data, tuples.ctypes.data,
                                             ctypes.byref(t)), "vpcsum_ctx_parse_frames")
        self.wait(t.value)
        return desc, status, tuples

    def egress_frames(self, arena: np.ndarray, frame_off: np.ndarray, frame_len: np.ndarray,
                      frame_flags: np.ndarray):
        """Egress flush of frames in a registered arena, each with its own F_* flags: parsed on
        the GPU and written in place in one submission (vpcsum_ctx_egress_frames).  Returns
        (out, status) per frame; S_BAD_DESC = refused, nothing written."""
        n = len(frame_off)
        fo = np.ascontiguousarray(frame_off, dtype=np.uint64)
        fl = np.ascontiguousarray(frame_len, dtype=np.uint32)
        ff = np.ascontiguousarray(frame_flags, dtype=np.uint8)
        out = np.zeros(n, np.uint32)
        status = np.zeros(n, np.uint8)
        t = ctypes.c_uint64()
        _check(lib().vpcsum_ctx_egress_frames(self.h, arena.ctypes.data, arena.nbytes, fo.ctypes.data, fl.ctypes.data,
                                              ff.ctypes.data, n, out.ctypes.data, status.ctypes.data,
                                              ctypes.byref(t)), "vpcsum_ctx_egress_frames")
        self.wait(t.value)
        return out, status

    def nat_submit(self, arena: np.ndarray, desc: np.ndarray, rw: np.ndarray, status: np.ndarray | None = None,
                   nat_mode: int = NAT_RFC1624) -> int:
        """NAT / TTL rewrites of host frames (vpcsum_ctx_nat_submit); rw: NAT_DTYPE entries."""
        assert rw.dtype == NAT_DTYPE and len(rw) >= len(desc)
        t = ctypes.c_uint64()
        _check(lib().vpcsum_ctx_nat_submit(self.h, arena.ctypes.data, arena.nbytes, desc.ctypes.data,
                                           rw.ctypes.data, len(desc), None if status is None else status.ctypes.data,
                                           nat_mode, ctypes.byref(t)), "vpcsum_ctx_nat_submit")
        self._inflight[t.value & 1] = (arena, desc, rw, status)
        return t.value

    def nat(self, arena: np.ndarray, desc: np.ndarray, rw: np.ndarray, nat_mode: int = NAT_RFC1624) -> np.ndarray:
        status = np.zeros(len(desc), np.uint8)
        self.wait(self.nat_submit(arena, desc, rw, status, nat_mode))
        return status

    def nat_flow_frames(self, tab: "FlowTable", arena: np.ndarray, frame_off: np.ndarray, frame_len: np.ndarray,
                        nat_mode: int = NAT_RFC1624):
        """The NAT fast path of received frames in a registered arena (vpcsum_ctx_nat_flow_frames):
        parsed, looked up in `tab` and rewritten in place on the GPU.  Returns (status, verdict)
        per frame; a frame with verdict FLOW_MISS / FLOW_PUNT or status S_BAD_DESC is untouched."""
        n = len(frame_off)
        fo = np.ascontiguousarray(frame_off, dtype=np.uint64)
        fl = np.ascontiguousarray(frame_len, dtype=np.uint32)
        status = np.zeros(n, np.uint8)
        verdict = np.zeros(n, np.uint8)
        t = ctypes.c_uint64()
        _check(lib().vpcsum_ctx_nat_flow_frames(self.h, tab.h, arena.ctypes.data, arena.nbytes, fo.ctypes.data,
                                                fl.ctypes.data, n, status.ctypes.data, verdict.ctypes.data, nat_mode,
                                                ctypes.byref(t)), "vpcsum_ctx_nat_flow_frames")
        self.wait(t.value)
        return status, verdict

    def nat_flow_forward_frames(self, tab: "FlowTable", arena: np.ndarray, frame_off: np.ndarray, frame_len: np.ndarray,
                                nat_mode: int = NAT_RFC1624):
        """nat_flow_frames that also forwards (vpcsum_ctx_nat_flow_forward_frames): a HIT frame that
        was rewritten and whose flow has a Fastpath gets the flow's Ethernet addresses written and
        its port returned.  Returns (status, verdict, port) per frame; port 0: the frame's Ethernet
        header is as received."""
        n = len(frame_off)
        fo = np.ascontiguousarray(frame_off, dtype=np.uint64)
        fl = np.ascontiguousarray(frame_len, dtype=np.uint32)
        status = np.zeros(n, np.uint8)
        verdict = np.zeros(n, np.uint8)
        port = np.zeros(n, np.uint32)
        t = ctypes.c_uint64()
        _check(lib().vpcsum_ctx_nat_flow_forward_frames(self.h, tab.h, arena.ctypes.data, arena.nbytes, fo.ctypes.data,
                                                        fl.ctypes.data, n, status.ctypes.data, verdict.ctypes.data,
                                                        port.ctypes.data, nat_mode, ctypes.byref(t)),
               "vpcsum_ctx_nat_flow_forward_frames")
        self.wait(t.value)
        return status, verdict, port

    def build_tcp_frames(self, dst: np.ndarray, src: np.ndarray, hdrs: np.ndarray, segs: np.ndarray, want_out: bool = True,
                         want_status: bool = True):
        """vpcsum_ctx_build_tcp_frames: the frames of `segs` (TCPSEG_DTYPE) built from `hdrs`
        (TCPHDR_DTYPE) and the payloads in `src` into `dst`, which must lie in a registered arena;
        a registered `src` is read in place, any other staged.  Returns (frame_len, out, status) per
        record (out / status None when not asked for); frame_len 0: the record was refused."""
        assert hdrs.dtype == TCPHDR_DTYPE and segs.dtype == TCPSEG_DTYPE
        n, n_hdr = len(segs), len(hdrs)
        hd, sg = np.ascontiguousarray(hdrs), np.ascontiguousarray(segs)
        frame_len = np.zeros(n, np.uint32)
        out = np.zeros(n, np.uint32) if want_out else None
        status = np.zeros(n, np.uint8) if want_status else None
        t = ctypes.c_uint64()
        _check(lib().vpcsum_ctx_build_tcp_frames(self.h, dst.ctypes.data, dst.nbytes, src.ctypes.data if src.nbytes else None,
                                                 src.nbytes, hd.ctypes.data if n_hdr else None, n_hdr,
                                                 sg.ctypes.data if n else None, n, frame_len.ctypes.data,
                                                 None if out is None else out.ctypes.data,
                                                 None if status is None else status.ctypes.data, ctypes.byref(t)),
               "vpcsum_ctx_build_tcp_frames")
        self.wait(t.value)
        return frame_len, out, status

    def build_tcp_bursts(self, dst: np.ndarray, src: np.ndarray, hdrs: np.ndarray, bursts: np.ndarray, frame_off: np.ndarray,
                         frame_cap: int, want_out: bool = True, want_status: bool = True):
        """vpcsum_ctx_build_tcp_bursts: build_tcp_frames with one record per fetch() -- the frames of
        `frame_off` cut from `bursts` (TCPBURST_DTYPE) on the device, each with `frame_cap` bytes of
        room.  `dst` must lie in a registered arena; a registered `src` is read in place, any other
        staged.  Returns (frame_len, out, status) per frame; frame_len 0: the frame was refused."""
        assert hdrs.dtype == TCPHDR_DTYPE and bursts.dtype == TCPBURST_DTYPE
        n, n_bursts, n_hdr = len(frame_off), len(bursts), len(hdrs)
        hd, bu = np.ascontiguousarray(hdrs), np.ascontiguousarray(bursts)
        fo = np.ascontiguousarray(frame_off, dtype=np.uint64)
        frame_len = np.zeros(n, np.uint32)
        out = np.zeros(n, np.uint32) if want_out else None
        status = np.zeros(n, np.uint8) if want_status else None
        t = ctypes.c_uint64()
        _check(lib().vpcsum_ctx_build_tcp_bursts(self.h, dst.ctypes.data, dst.nbytes, src.ctypes.data if src.nbytes else None,
                                                 src.nbytes, hd.ctypes.data if n_hdr else None, n_hdr,
                                                 bu.ctypes.data if n_bursts else None, n_bursts,
                                                 fo.ctypes.data if n else None, n, frame_cap, frame_len.ctypes.data,
                                                 None if out is None else out.ctypes.data,
                                                 None if status is None else status.ctypes.data, ctypes.byref(t)),
               "vpcsum_ctx_build_tcp_bursts")
        self.wait(t.value)
        return frame_len, out, status

    def recv_tcp_frames(self, arena: np.ndarray, desc: np.ndarray, rx: np.ndarray, dst: np.ndarray, want_out: bool = True,
                        want_status: bool = True):
        """vpcsum_ctx_recv_tcp_frames: descriptor i of `arena` verified and, under rx[i] (TCPRX_DTYPE),
        its payload stored into `dst`, which must lie in a registered arena; a registered `arena` is
        read in place, any other staged as submit() stages it.  Returns (stored, out, status) per
        record (out / status None when not asked for).  Stored whatever the verdict: accept a
        segment's bytes on S_L4_OK only."""
        assert desc.dtype == DESC_DTYPE and rx.dtype == TCPRX_DTYPE and len(desc) == len(rx)
        n = len(desc)
        ds, rr = np.ascontiguousarray(desc), np.ascontiguousarray(rx)
        stored = np.zeros(n, np.uint32)
        out = np.zeros(n, np.uint32) if want_out else None
        status = np.zeros(n, np.uint8) if want_status else None
        t = ctypes.c_uint64()
        _check(lib().vpcsum_ctx_recv_tcp_frames(self.h, arena.ctypes.data, arena.nbytes, ds.ctypes.data if n else None,
                                                rr.ctypes.data if n else None, n, dst.ctypes.data if dst.nbytes else None,
                                                dst.nbytes, stored.ctypes.data,
                                                None if out is None else out.ctypes.data,
                                                None if status is None else status.ctypes.data, ctypes.byref(t)),
               "vpcsum_ctx_recv_tcp_frames")
        self.wait(t.value)
        return stored, out, status

    def build_udp_frames(self, dst: np.ndarray, src: np.ndarray, hdrs: np.ndarray, dgs: np.ndarray, want_out: bool = True,
                         want_status: bool = True):
        """vpcsum_ctx_build_udp_frames: build_tcp_frames for datagrams -- the frames of `dgs`
        (UDPDG_DTYPE) built from `hdrs` (TCPHDR_DTYPE with ack / window / rsv 0) and the payloads in
        `src` into `dst`, which must lie in a registered arena; a registered `src` is read in place,
        any other staged.  Returns (frame_len, out, status) per record; frame_len 0: refused."""
        assert hdrs.dtype == TCPHDR_DTYPE and dgs.dtype == UDPDG_DTYPE
        n, n_hdr = len(dgs), len(hdrs)
        hd, dg = np.ascontiguousarray(hdrs), np.ascontiguousarray(dgs)
        frame_len = np.zeros(n, np.uint32)
        out = np.zeros(n, np.uint32) if want_out else None
        status = np.zeros(n, np.uint8) if want_status else None
        t = ctypes.c_uint64()
        _check(lib().vpcsum_ctx_build_udp_frames(self.h, dst.ctypes.data, dst.nbytes, src.ctypes.data if src.nbytes else None,
                                                 src.nbytes, hd.ctypes.data if n_hdr else None, n_hdr,
                                                 dg.ctypes.data if n else None, n, frame_len.ctypes.data,
                                                 None if out is None else out.ctypes.data,
                                                 None if status is None else status.ctypes.data, ctypes.byref(t)),
               "vpcsum_ctx_build_udp_frames")
        self.wait(t.value)
        return frame_len, out, status

    def recv_udp_frames(self, arena: np.ndarray, desc: np.ndarray, rx: np.ndarray, dst: np.ndarray, want_out: bool = True,
                        want_status: bool = True):
        """vpcsum_ctx_recv_udp_frames: recv_tcp_frames for datagrams -- descriptor i of `arena`
        verified and, under rx[i] (UDPRX_DTYPE), its data stored into `dst`, which must lie in a
        registered arena; a registered `arena` is read in place, any other staged.  Returns
        (stored, out, status) per record.  Stored whatever the verdict."""
        assert desc.dtype == DESC_DTYPE and rx.dtype == UDPRX_DTYPE and len(desc) == len(rx)
        n = len(desc)
        ds, rr = np.ascontiguousarray(desc), np.ascontiguousarray(rx)
        stored = np.zeros(n, np.uint32)
        out = np.zeros(n, np.uint32) if want_out else None
        status = np.zeros(n, np.uint8) if want_status else None
        t = ctypes.c_uint64()
        _check(lib().vpcsum_ctx_recv_udp_frames(self.h, arena.ctypes.data, arena.nbytes, ds.ctypes.data if n else None,
                                                rr.ctypes.data if n else None, n, dst.ctypes.data if dst.nbytes else None,
                                                dst.nbytes, stored.ctypes.data,
                                                None if out is None else out.ctypes.data,
                                                None if status is None else status.ctypes.data, ctypes.byref(t)),
               "vpcsum_ctx_recv_udp_frames")
        self.wait(t.value)
        return stored, out, status

    def reply_icmp_frames(self, arena: np.ndarray, desc: np.ndarray, hdrs: np.ndarray, rps: np.ndarray, dst: np.ndarray,
                          want_csum: bool = True, want_out: bool = True, want_status: bool = True):
        """vpcsum_ctx_reply_icmp_frames: the ICMP reply to descriptor i of `arena` under rps[i]
        (ICMPRP_DTYPE) and its template of `hdrs` (TCPHDR_DTYPE with ports / ack / window / rsv 0),
        written into `dst`, which must lie in a registered arena (it may be the one `arena` lies in);
        a registered `arena` is read in place, any other staged.  Returns (frame_len, csum, out,
        status) per record; frame_len 0: refused."""
        assert desc.dtype == DESC_DTYPE and rps.dtype == ICMPRP_DTYPE and hdrs.dtype == TCPHDR_DTYPE and len(desc) == len(rps)
        n, n_hdr = len(desc), len(hdrs)
        ds, rr, hd = np.ascontiguousarray(desc), np.ascontiguousarray(rps), np.ascontiguousarray(hdrs)
        frame_len = np.zeros(n, np.uint32)
        csum = np.zeros(n, np.uint32) if want_csum else None
        out = np.zeros(n, np.uint32) if want_out else None
        status = np.zeros(n, np.uint8) if want_status else None
        t = ctypes.c_uint64()
        _check(lib().vpcsum_ctx_reply_icmp_frames(self.h, arena.ctypes.data, arena.nbytes, ds.ctypes.data if n else None,
                                                  hd.ctypes.data if n_hdr else None, n_hdr, rr.ctypes.data if n else None, n,
                                                  dst.ctypes.data if dst.nbytes else None, dst.nbytes, frame_len.ctypes.data,
                                                  None if csum is None else csum.ctypes.data,
                                                  None if out is None else out.ctypes.data,
                                                  None if status is None else status.ctypes.data, ctypes.byref(t)),
               "vpcsum_ctx_reply_icmp_frames")
        self.wait(t.value)
        return frame_len, csum, out, status

    def set_service(self, idle_us: int):
        """Low-latency flushes from registered arenas (persistent service grid); 0 = off."""
        _check(lib().vpcsum_ctx_set_service(self.h, idle_us), "vpcsum_ctx_set_service")

    def stats(self) -> dict:
        b, n = ctypes.c_uint64(), ctypes.c_uint64()
        _check(lib().vpcsum_ctx_stats(self.h, ctypes.byref(b), ctypes.byref(n)), "vpcsum_ctx_stats")
        return {"service_batches": b.value, "service_launches": n.value}

    def run(self, arena, desc, mode: int = MODE_COMPUTE):
        out = np.zeros(len(desc), np.uint32)
        status = np.zeros(len(desc), np.uint8)
        self.wait(self.submit(arena, desc, out, status, mode))
        return out, status

    def pipeline(self, arena: np.ndarray, stride: int, copy_bytes: int, desc: np.ndarray, out: np.ndarray,
                 mode: int = MODE_COMPUTE, chunks: int = 8):
        _check(lib().vpcsum_ctx_pipeline(self.h, arena.ctypes.data, stride, copy_bytes, desc.ctypes.data, len(desc),
                                         out.ctypes.data, mode, chunks), "vpcsum_ctx_pipeline")

    def close(self):
        """Destroy the context (its batches finish, its page-locks go).  If an unregister failed,
        the arrays it held stay referenced (never freed while HIP may still map them) and the error
        is raised."""
        if self.h:
            rc = lib().vpcsum_ctx_destroy(self.h)
            self.h = None
            if rc != 0:
                _leaked.append(self._pinned.copy())
                _check(rc, "vpcsum_ctx_destroy")
            for p in self._pinned:
                _reg_drop(p)
            self._pinned.clear()
            self._inflight.clear()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Group:
    """Several GPUs behind one host batch (vpcsum_group_*): the batch is cut by bytes into one
    contiguous range per device.  `devices` may repeat a device (several contexts on one GPU)."""

    def __init__(self, devices=(0,), max_arena: int = 1 << 26, max_pkts: int = 1 << 16):
        h = ctypes.c_void_p()
        arr = (ctypes.c_int * len(devices))(*devices)
        _check(lib().vpcsum_group_create_list(arr, len(devices), max_arena, max_pkts, ctypes.byref(h)),
               "vpcsum_group_create_list")
        self.h = h.value
        self._pinned = {}
        self._inflight = {}

    def register(self, arr: np.ndarray):
        _check(lib().vpcsum_group_register_arena(self.h, arr.ctypes.data, arr.nbytes), "vpcsum_group_register_arena")
        self._pinned[arr.ctypes.data] = arr
        _reg_add(arr.ctypes.data, arr.nbytes)

    def unregister(self, arr: np.ndarray):
        _check(lib().vpcsum_group_unregister_arena(self.h, arr.ctypes.data), "vpcsum_group_unregister_arena")
        self._pinned.pop(arr.ctypes.data, None)
        _reg_drop(arr.ctypes.data)

    def submit(self, arena: np.ndarray, desc: np.ndarray, out: np.ndarray, status: np.ndarray | None = None,
               mode: int = MODE_COMPUTE) -> int:
        t = ctypes.c_uint64()
        _check(lib().vpcsum_group_submit(self.h, arena.ctypes.data, arena.nbytes, desc.ctypes.data, len(desc),
                                         out.ctypes.data, None if status is None else status.ctypes.data, mode,
                                         ctypes.byref(t)), "vpcsum_group_submit")
        self._inflight[t.value & 1] = (arena, desc, out, status)
        return t.value

    def submit_pre(self, arena: np.ndarray, desc: np.ndarray, pre_img: np.ndarray, out: np.ndarray,
                   status: np.ndarray | None = None, mode: int = MODE_COMPUTE) -> int:
        """vpcsum_group_submit_pre: Context.submit_pre cut over the group's devices."""
        fmt = PRE_FMT_PRE if pre_img.dtype == NAT_DTYPE else PRE_FMT_PRE4
        assert pre_img.dtype in (NAT_DTYPE, NAT4_DTYPE) and len(pre_img) >= len(desc)
        t = ctypes.c_uint64()
        _check(lib().vpcsum_group_submit_pre(self.h, arena.ctypes.data, arena.nbytes, desc.ctypes.data,
                                             pre_img.ctypes.data, fmt, len(desc), out.ctypes.data,
                                             None if status is None else status.ctypes.data, mode, ctypes.byref(t)),
               "vpcsum_group_submit_pre")
        self._inflight[t.value & 1] = (arena, desc, pre_img, out, status)
        return t.value

    def nat_submit(self, arena: np.ndarray, desc: np.ndarray, rw: np.ndarray, status: np.ndarray | None = None,
                   nat_mode: int = NAT_RFC1624) -> int:
        """NAT / TTL rewrites of host frames cut over the group's devices (vpcsum_group_nat_submit)."""
        assert rw.dtype == NAT_DTYPE and len(rw) >= len(desc)
        t = ctypes.c_uint64()
        _check(lib().vpcsum_group_nat_submit(self.h, arena.ctypes.data, arena.nbytes, desc.ctypes.data,
                                             rw.ctypes.data, len(desc), None if status is None else status.ctypes.data,
                                             nat_mode, ctypes.byref(t)), "vpcsum_group_nat_submit")
        self._inflight[t.value & 1] = (arena, desc, rw, status)
        return t.value

    def wait(self, ticket: int):
        _check(lib().vpcsum_group_wait(self.h, ticket), "vpcsum_group_wait")

    def run(self, arena, desc, mode: int = MODE_COMPUTE):
        out = np.zeros(len(desc), np.uint32)
        status = np.zeros(len(desc), np.uint8)
        self.wait(self.submit(arena, desc, out, status, mode))
        return out, status

    def close(self):
        if self.h:
            rc = lib().vpcsum_group_destroy(self.h)
            self.h = None
            if rc != 0:
                _leaked.append(self._pinned.copy())
                _check(rc, "vpcsum_group_destroy")
            for p in self._pinned:
                _reg_drop(p)
            self._pinned.clear()
            self._inflight.clear()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def desc_to_tensor(desc: np.ndarray, device="cuda"):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(desc).view(np.uint8).copy())
    # through page-locked memory: no pageable host-to-device copy of an array whose addresses a
    # context may have registered and unregistered before (DESIGN_HISTORY.md "Round 5: experiments")
    return (t.pin_memory() if str(device).startswith("cuda") else t).to(device)


def tensor_to_desc(t) -> np.ndarray:
    return t.cpu().numpy().view(DESC_DTYPE).copy()

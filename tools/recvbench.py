"""The TCP receive, device-resident: N received Ethernet / IPv4 / TCP frames in 2,048-byte chunks at
chunk + 384 (umem geometry), payloads of 1,360 bytes (TcpEntry.SND_DEFAULT_MSS) and of 1,460 bytes,
verified and stored back to back into per-connection runs of a receive buffer.  The frames are built
on the device (vpcsum_tcp_build_async) and parsed once (vpcsum_parse_ether_async) outside the timed
window.  Timed with events over --launches launches after a warm-up, legs in alternating rounds
(tools/segbench.py's protocol):
  r  vpcsum_tcp_recv_async (k_tcp_recv): the verify and the payload store in one pass
  a  vpcsum_compute_async with MODE_VERIFY over the same descriptors: the ingress verify alone, which
     writes nothing but out / status
  b  a, then a hipMemcpy2DAsync of the payloads out of the chunks: what a device caller does without
     the receive, from the entry points that existed before it (every payload byte read twice)
  c  for scale, a contiguous device copy of the same payload bytes
a, b and c use only entry points and kernels that this tool's library shares with its parent.
Algorithmic bytes per frame: the segment read + data_len written + descriptor and record.  Before
timing, r's receive buffer is compared with b's and with the send buffer, r's status and out with a's.
With --udp only the UDP leg runs: vpcsum_udp_recv_async (k_udp_recv) on datagrams of 1,360 and 1,472
payload bytes, timed against leg r on segments of the same payload and against leg c, in the same run.
With --icmp-echo only the echo leg runs: vpcsum_icmp_reply_async (k_icmp_reply) answering IPv4 echo
requests whose ICMP messages are 1,360 and 1,472 bytes into a second arena of the same layout (leg e)
and into chunks with 6 more bytes of headroom (leg s), timed
against k_udp_recv with STORE on UDP frames of the same segment lengths and against leg c.
Prints one JSON line.  usage: recvbench.py [frames] [--launches N] [--udp | --icmp-echo]"""
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vproxy_amd import vpcsum as V  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 1 << 17
launches = int(sys.argv[sys.argv.index("--launches") + 1]) if "--launches" in sys.argv else 50
rounds = 3
STRIDE, HEADROOM, HLEN = 2048, 384, 54
SHIFT = 6   # --icmp-echo leg s: the replies' chunks have 6 more bytes of headroom than the requests'

V.lib()
hip = None
with open("/proc/self/maps") as f:
    for line in f:
        if "libamdhip64.so" in line:
            hip = ctypes.CDLL(line.split()[-1])
            break
assert hip is not None, "libamdhip64 is not loaded"
hip.hipMemcpy2DAsync.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t,
                                 ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
hip.hipMemcpy2DAsync.restype = ctypes.c_int
D2D = 3   # hipMemcpyDeviceToDevice


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).pin_memory().cuda()


def timed(fn):
    for _ in range(3):
        fn()
    e0, e1 = V.Event(), V.Event()
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_ms(e1) / launches * 1e3   # us per launch


hdr = np.zeros(1, V.TCPHDR_DTYPE)
hdr["eth_dst"], hdr["eth_src"] = np.frombuffer(bytes.fromhex("02aa00000001"), np.uint8), np.frombuffer(bytes.fromhex("02bb00000002"), np.uint8)
hdr["l2_len"], hdr["l3_ver"], hdr["ttl"] = 14, 4, 64
hdr["src"][0, :4], hdr["dst"][0, :4] = (10, 0, 0, 1), (10, 0, 0, 2)
hdr["sport"], hdr["dport"] = np.frombuffer((43210).to_bytes(2, "big"), np.uint8), np.frombuffer((443).to_bytes(2, "big"), np.uint8)
hdr["ack"], hdr["window"] = np.frombuffer((0x01020304).to_bytes(4, "big"), np.uint8), np.frombuffer((65535).to_bytes(2, "big"), np.uint8)
d_hdr = dev(hdr)

def udp_leg():
    """--udp: vpcsum_udp_recv_async (k_udp_recv) on datagrams of 1,360 and 1,472 payload bytes, against
    k_tcp_recv on segments of the same payload and a contiguous copy of the same bytes, in the same run."""
    uh = hdr.copy()
    uh["ack"], uh["window"] = 0, 0
    d_uh = dev(uh)
    r_all = {"frames_per_batch": n, "launches": launches, "rounds": rounds, "stride": STRIDE, "frame_at": HEADROOM,
             "frames": "Ethernet / IPv4 / UDP against Ethernet / IPv4 / TCP of the same payload"}
    for data_len in (1360, 1472):
        off = np.arange(n, dtype=np.uint64)
        dg, seg = np.zeros(n, V.UDPDG_DTYPE), np.zeros(n, V.TCPSEG_DTYPE)
        for rec in (dg, seg):
            rec["frame_off"], rec["data_off"] = off * STRIDE + HEADROOM, off * data_len
            rec["frame_cap"], rec["data_len"] = STRIDE - HEADROOM, data_len
        seg["flags"] = 0x18
        g = torch.Generator(device="cuda").manual_seed(data_len)
        sent = torch.randint(0, 256, (n * data_len,), dtype=torch.uint8, device="cuda", generator=g)
        fr_u, fr_t = (torch.zeros(n * STRIDE, dtype=torch.uint8, device="cuda") for _ in range(2))
        flen_u, flen_t = (torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(2))
        V.udp_build(fr_u, sent, d_uh, 1, dev(dg), n, flen_u, None, None)
        V.tcp_build(fr_t, sent, d_hdr, 1, dev(seg), n, flen_t, None, None)
        foff = dev(dg["frame_off"].copy())
        desc_u, desc_t = (torch.zeros(n * 16, dtype=torch.uint8, device="cuda") for _ in range(2))
        V.parse_ether(fr_u, foff, flen_u, n, desc_u)
        V.parse_ether(fr_t, foff, flen_t, n, desc_t)
        urx, trx = np.zeros(n, V.UDPRX_DTYPE), np.zeros(n, V.TCPRX_DTYPE)
        for rec, store in ((urx, V.UDPRX_STORE), (trx, V.TCPRX_STORE)):
            rec["dst_off"], rec["dst_cap"], rec["ops"] = off * data_len, data_len, store
        d_urx, d_trx = dev(urx), dev(trx)
        rb_u, rb_t, copy = (torch.zeros(n * data_len, dtype=torch.uint8, device="cuda") for _ in range(3))
        stored, out = (torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(2))
        st = torch.zeros(n, dtype=torch.uint8, device="cuda")
        legs = {"u_udp_recv": lambda: V.udp_recv(fr_u, desc_u, d_urx, n, rb_u, stored, out, st),
                "r_tcp_recv": lambda: V.tcp_recv(fr_t, desc_t, d_trx, n, rb_t, stored, out, st),
                "c_contiguous_copy": lambda: copy.copy_(sent)}
        legs["u_udp_recv"]()
        torch.cuda.synchronize()
        assert int((st != (V.S_DONE | V.S_IP_OK | V.S_L4_OK)).sum().item()) == 0 and int((stored != data_len).sum().item()) == 0
        assert torch.equal(rb_u, sent), "u stores the sent bytes"
        us = {k: [] for k in legs}
        for _ in range(rounds):
            for k, fn in legs.items():
                us[k].append(round(timed(fn), 2))
        assert torch.equal(rb_u, sent) and torch.equal(rb_t, sent)
        r = {"udp_frame_len": 42 + data_len, "tcp_frame_len": 54 + data_len}
        for k, v in us.items():
            r[k] = {"us_rounds": v, "us_median": sorted(v)[len(v) // 2]}
        r["u_over_r"] = round(r["u_udp_recv"]["us_median"] / r["r_tcp_recv"]["us_median"], 4)
        r["u_over_c"] = round(r["u_udp_recv"]["us_median"] / r["c_contiguous_copy"]["us_median"], 3)
        r["r_round_spread"] = round(max(us["r_tcp_recv"]) / min(us["r_tcp_recv"]) - 1, 4)
        r["u_round_spread"] = round(max(us["u_udp_recv"]) / min(us["u_udp_recv"]) - 1, 4)
        r_all[f"data_len_{data_len}"] = r
        del sent, fr_u, fr_t, rb_u, rb_t, copy
    print(json.dumps(r_all))


def icmp_echo_leg():
    """--icmp-echo: vpcsum_icmp_reply_async (k_icmp_reply) on IPv4 echo requests whose ICMP messages are
    1,360 and 1,472 bytes, answered into a second arena of the same layout, against k_udp_recv with
    STORE on UDP frames of the same segment lengths and a contiguous copy of the same bytes, in the
    same run.  Leg e writes each reply at its request's own offset in the chunk (source and the reply's
    16-B grid agree, every group is one aligned load); leg s writes it SHIFT bytes further on, a TX chunk
    of another headroom (source and grid differ modulo 4, as they do for the receive's back-to-back
    runs).  The requests are laid out on the device (a header row and random bodies), their sums
    written by vpcsum_compute_async with MODE_WRITE; before timing every request must verify, and the
    replies -- parsed and verified in turn -- must carry the requests' bytes from 4 on."""
    uh = hdr.copy()
    uh["ack"], uh["window"] = 0, 0
    d_uh = dev(uh)
    ih = uh.copy()
    ih["sport"], ih["dport"] = 0, 0
    ih["src"][0, :4], ih["dst"][0, :4] = (10, 0, 0, 2), (10, 0, 0, 1)
    d_ih = dev(ih)
    r_all = {"frames_per_batch": n, "launches": launches, "rounds": rounds, "stride": STRIDE, "frame_at": HEADROOM,
             "shifted_reply_at": HEADROOM + SHIFT,
             "frames": "Ethernet / IPv4 / ICMP echo requests against Ethernet / IPv4 / UDP of the same segment length"}
    off = np.arange(n, dtype=np.uint64)
    foff = dev((off * STRIDE + HEADROOM).copy())
    for M in (1360, 1472):
        g = torch.Generator(device="cuda").manual_seed(M)
        # the requests: 02bb.. -> 02aa.., 10.0.0.1 -> 10.0.0.2, type 8 code 0, sums 0 until MODE_WRITE fills them
        row = bytes.fromhex("02aa0000000102bb000000020800") + bytes([0x45, 0]) + (20 + M).to_bytes(2, "big") + bytes.fromhex("00004000") + \
            bytes([64, 1, 0, 0, 10, 0, 0, 1, 10, 0, 0, 2]) + bytes([8, 0, 0, 0])
        req = torch.zeros(n * STRIDE, dtype=torch.uint8, device="cuda")
        r2 = req.view(n, STRIDE)
        r2[:, HEADROOM:HEADROOM + len(row)] = dev(np.frombuffer(row, np.uint8))
        r2[:, HEADROOM + len(row):HEADROOM + 34 + M] = torch.randint(0, 256, (n, M - 4), dtype=torch.uint8, device="cuda", generator=g)
        flen_q = torch.full((n,), 34 + M, dtype=torch.int32, device="cuda")
        desc_q = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
        V.parse_ether(req, foff, flen_q, n, desc_q)
        V.compute(req, desc_q, n, None, None, V.MODE_WRITE)
        rp = np.zeros(n, V.ICMPRP_DTYPE)
        rp["frame_off"], rp["frame_cap"], rp["kind"] = off * STRIDE + HEADROOM, STRIDE - HEADROOM, V.ICMP_ECHO_REPLY
        d_rp = dev(rp)
        rp["frame_off"], rp["frame_cap"] = off * STRIDE + HEADROOM + SHIFT, STRIDE - HEADROOM - SHIFT
        d_rp_s = dev(rp)
        rep, rep_s = (torch.zeros(n * STRIDE, dtype=torch.uint8, device="cuda") for _ in range(2))
        flen_e, cs_e, out_e = (torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(3))
        st_e = torch.zeros(n, dtype=torch.uint8, device="cuda")
        # the UDP twin: datagrams whose segment is M bytes, stored back to back
        data_len = M - 8
        dg = np.zeros(n, V.UDPDG_DTYPE)
        dg["frame_off"], dg["data_off"], dg["frame_cap"], dg["data_len"] = off * STRIDE + HEADROOM, off * data_len, STRIDE - HEADROOM, data_len
        sent = torch.randint(0, 256, (n * data_len,), dtype=torch.uint8, device="cuda", generator=g)
        fr_u = torch.zeros(n * STRIDE, dtype=torch.uint8, device="cuda")
        flen_u = torch.zeros(n, dtype=torch.int32, device="cuda")
        V.udp_build(fr_u, sent, d_uh, 1, dev(dg), n, flen_u, None, None)
        desc_u = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
        V.parse_ether(fr_u, foff, flen_u, n, desc_u)
        urx = np.zeros(n, V.UDPRX_DTYPE)
        urx["dst_off"], urx["dst_cap"], urx["ops"] = off * data_len, data_len, V.UDPRX_STORE
        d_urx = dev(urx)
        rb_u, copy = (torch.zeros(n * data_len, dtype=torch.uint8, device="cuda") for _ in range(2))
        stored, out_u = (torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(2))
        st_u = torch.zeros(n, dtype=torch.uint8, device="cuda")
        legs = {"e_icmp_echo": lambda: V.icmp_reply(req, desc_q, d_ih, 1, d_rp, n, rep, flen_e, cs_e, out_e, st_e),
                "s_icmp_echo_shifted": lambda: V.icmp_reply(req, desc_q, d_ih, 1, d_rp_s, n, rep_s, flen_e, cs_e, out_e, st_e),
                "u_udp_recv": lambda: V.udp_recv(fr_u, desc_u, d_urx, n, rb_u, stored, out_u, st_u),
                "c_contiguous_copy": lambda: copy.copy_(sent)}
        legs["s_icmp_echo_shifted"]()
        legs["e_icmp_echo"]()
        legs["u_udp_recv"]()
        torch.cuda.synchronize()
        ok = V.S_DONE | V.S_IP_OK | V.S_L4_OK
        assert int((st_e != ok).sum().item()) == 0 and int((flen_e != 34 + M).sum().item()) == 0, "every request verifies and is answered"
        assert int((st_u != ok).sum().item()) == 0 and torch.equal(rb_u, sent)
        p2 = rep.view(n, STRIDE)
        assert torch.equal(p2[:, HEADROOM + 38:HEADROOM + 34 + M], r2[:, HEADROOM + 38:HEADROOM + 34 + M]), "the replies carry the requests' bytes"
        assert int(p2[:, HEADROOM + 34:HEADROOM + 36].sum().item()) == 0 and int(p2[:, :HEADROOM].sum().item()) == 0
        assert torch.equal(rep_s.view(n, STRIDE)[:, HEADROOM + SHIFT:HEADROOM + SHIFT + 34 + M], p2[:, HEADROOM:HEADROOM + 34 + M]), \
            "the shifted replies are the same frames"
        desc_p = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
        st_p = torch.zeros(n, dtype=torch.uint8, device="cuda")
        V.parse_ether(rep, foff, flen_e, n, desc_p)
        V.compute(rep, desc_p, n, None, st_p, V.MODE_VERIFY)
        torch.cuda.synchronize()
        assert int((st_p != ok).sum().item()) == 0, "every reply verifies"
        us = {k: [] for k in legs}
        for _ in range(rounds):
            for k, fn in legs.items():
                us[k].append(round(timed(fn), 2))
        # bytes moved per frame: the segment read once; the echo writes the frame (34 + M), the receive M - 8
        r = {"icmp_msg_len": M, "echo_frame_len": 34 + M, "udp_frame_len": 34 + M, "echo_bytes_per_frame": M + 34 + M + 64,
             "udp_bytes_per_frame": M + M - 8}
        for k, v in us.items():
            r[k] = {"us_rounds": v, "us_median": sorted(v)[len(v) // 2]}
        r["s_over_u"] = round(r["s_icmp_echo_shifted"]["us_median"] / r["u_udp_recv"]["us_median"], 4)
        r["s_over_e"] = round(r["s_icmp_echo_shifted"]["us_median"] / r["e_icmp_echo"]["us_median"], 4)
        r["e_over_u"] = round(r["e_icmp_echo"]["us_median"] / r["u_udp_recv"]["us_median"], 4)
        r["byte_ratio"] = round(r["echo_bytes_per_frame"] / r["udp_bytes_per_frame"], 4)
        r["e_over_c"] = round(r["e_icmp_echo"]["us_median"] / r["c_contiguous_copy"]["us_median"], 3)
        r["e_round_spread"] = round(max(us["e_icmp_echo"]) / min(us["e_icmp_echo"]) - 1, 4)
        r["u_round_spread"] = round(max(us["u_udp_recv"]) / min(us["u_udp_recv"]) - 1, 4)
        r_all[f"msg_len_{M}"] = r
        del req, rep, rep_s, sent, fr_u, rb_u, copy, r2, p2
    print(json.dumps(r_all))


if "--udp" in sys.argv:
    udp_leg()
    sys.exit(0)
if "--icmp-echo" in sys.argv:
    icmp_echo_leg()
    sys.exit(0)

res = {"frames_per_batch": n, "launches": launches, "rounds": rounds, "stride": STRIDE, "frame_at": HEADROOM,
       "frames": "Ethernet / IPv4 / TCP, PSH|ACK, no options"}
for data_len in (1360, 1460):
    L = HLEN + data_len
    seg = np.zeros(n, V.TCPSEG_DTYPE)
    seg["frame_off"] = np.arange(n, dtype=np.uint64) * STRIDE + HEADROOM
    seg["data_off"] = np.arange(n, dtype=np.uint64) * data_len
    seg["seq"] = (np.arange(n, dtype=np.uint64) * data_len & 0xffffffff).astype(np.uint32)
    seg["frame_cap"], seg["data_len"], seg["flags"] = STRIDE - HEADROOM, data_len, 0x18
    g = torch.Generator(device="cuda").manual_seed(data_len)
    sent = torch.randint(0, 256, (n * data_len,), dtype=torch.uint8, device="cuda", generator=g)
    frames = torch.zeros(n * STRIDE, dtype=torch.uint8, device="cuda")
    flen = torch.zeros(n, dtype=torch.int32, device="cuda")
    V.tcp_build(frames, sent, d_hdr, 1, dev(seg), n, flen, None, None)
    desc = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    V.parse_ether(frames, dev(seg["frame_off"].copy()), flen, n, desc)
    rx = np.zeros(n, V.TCPRX_DTYPE)
    rx["dst_off"] = np.arange(n, dtype=np.uint64) * data_len   # runs of consecutive segments, back to back
    rx["dst_cap"], rx["ops"] = data_len, V.TCPRX_STORE
    d_rx = dev(rx)
    rbuf = torch.zeros(n * data_len, dtype=torch.uint8, device="cuda")
    stored = torch.zeros(n, dtype=torch.int32, device="cuda")
    out_r = torch.zeros(n, dtype=torch.int32, device="cuda")
    st_r = torch.zeros(n, dtype=torch.uint8, device="cuda")
    out_a = torch.zeros(n, dtype=torch.int32, device="cuda")
    st_a = torch.zeros(n, dtype=torch.uint8, device="cuda")
    flat = torch.zeros(n * data_len, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def leg_r():
        V.tcp_recv(frames, desc, d_rx, n, rbuf, stored, out_r, st_r)

    def leg_a():
        V.compute(frames, desc, n, out_a, st_a, V.MODE_VERIFY)

    def leg_b():
        leg_a()
        rc = hip.hipMemcpy2DAsync(flat.data_ptr(), data_len, frames.data_ptr() + HEADROOM + HLEN, STRIDE, data_len, n, D2D, stream)
        assert rc == 0, rc

    copy = torch.empty_like(sent)

    def leg_c():
        copy.copy_(sent)

    leg_r()
    leg_b()
    torch.cuda.synchronize()
    want = V.S_DONE | V.S_IP_OK | V.S_L4_OK
    assert int((st_r != want).sum().item()) == 0 and int((stored != data_len).sum().item()) == 0
    assert torch.equal(st_r, st_a) and torch.equal(out_r, out_a), "r reports a's verdicts"
    assert torch.equal(rbuf, sent) and torch.equal(flat, sent), "r and b store the sent bytes"
    legs = {"r_tcp_recv": leg_r, "a_compute_verify": leg_a, "b_verify_plus_copy2d": leg_b, "c_contiguous_copy": leg_c}
    us = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            us[k].append(round(timed(fn), 2))
    assert torch.equal(rbuf, sent)
    bytes_per_frame = (L - 14 - 20) + data_len + 32
    r = {"frame_len": L, "algorithmic_bytes_per_frame": bytes_per_frame}
    for k, v in us.items():
        med = sorted(v)[len(v) // 2]
        r[k] = {"us_rounds": v, "us_median": med, "Mframes_per_s": round(n / med, 2), "GB_per_s": round(n * bytes_per_frame / med / 1e3, 1)}
    r["c_contiguous_copy"]["GB_per_s"] = round(n * 2 * data_len / r["c_contiguous_copy"]["us_median"] / 1e3, 1)   # its own bytes
    r["r_over_a"] = round(r["r_tcp_recv"]["us_median"] / r["a_compute_verify"]["us_median"], 3)
    r["b_over_r"] = round(r["b_verify_plus_copy2d"]["us_median"] / r["r_tcp_recv"]["us_median"], 3)
    r["r_over_c"] = round(r["r_tcp_recv"]["us_median"] / r["c_contiguous_copy"]["us_median"], 3)
    res[f"data_len_{data_len}"] = r
    del sent, frames, rbuf, flat, copy
print(json.dumps(res))

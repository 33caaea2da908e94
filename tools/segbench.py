"""The TCP segment build, device-resident: N data segments of 1,360 bytes (TcpEntry.SND_DEFAULT_MSS)
and of 1,460 bytes, payloads back to back in a send buffer, built as Ethernet / IPv4 / TCP frames into
2,048-byte chunks at chunk + 384 (umem geometry: the payload lands at chunk + 438).  Timed with events
over --launches launches after a warm-up, legs in alternating rounds:
  a  vpcsum_tcp_build_async (k_tcp_build): headers, copy and both sums in one pass
  b  today's device equivalent from the entry points that existed before it: hipMemcpy2DAsync of the
     payloads into frames whose headers are already there, then vpcsum_compute_async with MODE_WRITE
     over the frames (descriptors prepared once, outside the timed window)
  c  that 2-D copy alone: the copy ceiling
  d  for scale, a contiguous device copy of the same payload bytes (no frames): what moving
     2 x data_len bytes per segment costs when nothing is strided
  s  vpcsum_tcp_build_bursts_async (k_tcp_build_bursts): the same frames described as bursts of 45, 10
     and 1 frames (s45, s10, s1) and a frame table, the cut made on the device; its yardstick is leg a of
     the same process
Algorithmic bytes per segment: data_len read + L written + the 32-byte record.  Before timing, b's
and s's frames are compared with a's: all must build the same bytes.
With --udp only the UDP leg runs: vpcsum_udp_build_async (k_udp_build) on datagrams of 1,360 and 1,472
payload bytes, timed against leg a on segments of the same payload and against leg d, in the same run.
Prints one JSON line.  usage: segbench.py [segments] [--launches N] [--lib libvpcsum.so] [--udp]
(--lib: another build of the library, e.g. one compiled with -DVPCSUM_BURST_BINARY_SEARCH)"""
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
if "--lib" in sys.argv:
    V.LIB = os.path.abspath(sys.argv[sys.argv.index("--lib") + 1])
STRIDE, HEADROOM, HLEN = 2048, 384, 54

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
    """--udp: vpcsum_udp_build_async (k_udp_build) on datagrams of 1,360 and 1,472 payload bytes, against
    k_tcp_build on segments of the same payload and a contiguous copy of the same bytes, in the same run."""
    uh = hdr.copy()
    uh["ack"], uh["window"] = 0, 0
    d_uh = dev(uh)
    r_all = {"datagrams": n, "launches": launches, "rounds": rounds, "stride": STRIDE, "frame_at": HEADROOM,
             "frames": "Ethernet / IPv4 / UDP against Ethernet / IPv4 / TCP of the same payload"}
    for data_len in (1360, 1472):
        off = np.arange(n, dtype=np.uint64)
        dg, seg = np.zeros(n, V.UDPDG_DTYPE), np.zeros(n, V.TCPSEG_DTYPE)
        for rec in (dg, seg):
            rec["frame_off"], rec["data_off"] = off * STRIDE + HEADROOM, off * data_len
            rec["frame_cap"], rec["data_len"] = STRIDE - HEADROOM, data_len
        seg["flags"] = 0x18
        d_dg, d_seg = dev(dg), dev(seg)
        g = torch.Generator(device="cuda").manual_seed(data_len)
        src = torch.randint(0, 256, (n * data_len,), dtype=torch.uint8, device="cuda", generator=g)
        dst_u, dst_t = (torch.zeros(n * STRIDE, dtype=torch.uint8, device="cuda") for _ in range(2))
        flen, out = (torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(2))
        st = torch.zeros(n, dtype=torch.uint8, device="cuda")
        flat = torch.empty_like(src)
        legs = {"u_udp_build": lambda: V.udp_build(dst_u, src, d_uh, 1, d_dg, n, flen, out, st),
                "a_tcp_build": lambda: V.tcp_build(dst_t, src, d_hdr, 1, d_seg, n, flen, out, st),
                "d_contiguous_copy": lambda: flat.copy_(src)}
        legs["u_udp_build"]()
        torch.cuda.synchronize()
        assert int((st != V.S_DONE).sum().item()) == 0 and int((flen != 42 + data_len).sum().item()) == 0
        assert torch.equal(dst_u.view(n, STRIDE)[:, HEADROOM + 42:HEADROOM + 42 + data_len].reshape(-1), src), "the payloads arrive"
        us = {k: [] for k in legs}
        for _ in range(rounds):
            for k, fn in legs.items():
                us[k].append(round(timed(fn), 2))
        r = {"udp_frame_len": 42 + data_len, "tcp_frame_len": 54 + data_len}
        for k, v in us.items():
            r[k] = {"us_rounds": v, "us_median": sorted(v)[len(v) // 2]}
        r["u_over_a"] = round(r["u_udp_build"]["us_median"] / r["a_tcp_build"]["us_median"], 4)
        r["u_over_d"] = round(r["u_udp_build"]["us_median"] / r["d_contiguous_copy"]["us_median"], 3)
        r["a_round_spread"] = round(max(us["a_tcp_build"]) / min(us["a_tcp_build"]) - 1, 4)
        r["u_round_spread"] = round(max(us["u_udp_build"]) / min(us["u_udp_build"]) - 1, 4)
        r_all[f"data_len_{data_len}"] = r
        del src, dst_u, dst_t, flat
    print(json.dumps(r_all))


if "--udp" in sys.argv:
    udp_leg()
    sys.exit(0)

res = {"segments": n, "launches": launches, "rounds": rounds, "stride": STRIDE, "frame_at": HEADROOM,
       "frames": "Ethernet / IPv4 / TCP, PSH|ACK"}
for data_len in (1360, 1460):
    L = HLEN + data_len
    seg = np.zeros(n, V.TCPSEG_DTYPE)
    seg["frame_off"] = np.arange(n, dtype=np.uint64) * STRIDE + HEADROOM
    seg["data_off"] = np.arange(n, dtype=np.uint64) * data_len
    seg["seq"] = (np.arange(n, dtype=np.uint64) * data_len & 0xffffffff).astype(np.uint32)
    seg["frame_cap"], seg["data_len"], seg["flags"] = STRIDE - HEADROOM, data_len, 0x18
    d_seg = dev(seg)
    g = torch.Generator(device="cuda").manual_seed(data_len)
    src = torch.randint(0, 256, (n * data_len,), dtype=torch.uint8, device="cuda", generator=g)
    dst = torch.zeros(n * STRIDE, dtype=torch.uint8, device="cuda")
    flen = torch.zeros(n, dtype=torch.int32, device="cuda")
    out = torch.zeros(n, dtype=torch.int32, device="cuda")
    st = torch.zeros(n, dtype=torch.uint8, device="cuda")

    def leg_a():
        V.tcp_build(dst, src, d_hdr, 1, d_seg, n, flen, out, st)

    leg_a()
    torch.cuda.synchronize()
    assert int((st != V.S_DONE).sum().item()) == 0 and int((flen != L).sum().item()) == 0
    built = dst.clone()
    # b's frames: the headers a wrote (sums and all), payload bytes cleared; descriptors once
    dst2 = built.clone()
    dst2.view(n, STRIDE)[:, HEADROOM + HLEN:HEADROOM + L] = 0
    foff = dev(seg["frame_off"].copy())
    desc = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    V.parse_ether(dst2, foff, flen, n, desc)
    out2 = torch.zeros(n, dtype=torch.int32, device="cuda")
    st2 = torch.zeros(n, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def leg_c():
        rc = hip.hipMemcpy2DAsync(dst2.data_ptr() + HEADROOM + HLEN, STRIDE, src.data_ptr(), data_len, data_len, n, D2D, stream)
        assert rc == 0, rc

    def leg_b():
        leg_c()
        V.compute(dst2, desc, n, out2, st2, V.MODE_WRITE)

    leg_b()
    torch.cuda.synchronize()
    assert torch.equal(dst2, built) and torch.equal(out2, out), "b builds a's frames"
    flat = torch.empty_like(src)

    def leg_d():
        flat.copy_(src)

    legs = {"a_tcp_build": leg_a, "b_copy2d_plus_compute_write": leg_b, "c_copy2d_alone": leg_c, "d_contiguous_copy": leg_d}
    # s: the same frames as bursts of 45, 10 and 1 frames over one frame table
    dst3 = torch.zeros(n * STRIDE, dtype=torch.uint8, device="cuda")
    flen3, out3, st3 = torch.zeros_like(flen), torch.zeros_like(out), torch.zeros_like(st)
    record_bytes = {"a": n * 32}
    for per in (45, 10, 1):
        nb = (n + per - 1) // per
        bu = np.zeros(nb, V.TCPBURST_DTYPE)
        first = np.arange(nb, dtype=np.uint64) * per
        bu["first"], bu["data_off"] = first, first * data_len
        bu["count"] = np.minimum(per, n - first)
        bu["data_len"] = bu["count"] * data_len
        bu["seq"] = (first * data_len & 0xffffffff).astype(np.uint32)
        bu["mss"], bu["flags"] = data_len, 0x18
        d_bu = dev(bu)

        def leg_s(d_bu=d_bu, nb=nb):
            V.tcp_build_bursts(dst3, src, d_hdr, 1, d_bu, nb, foff, n, STRIDE - HEADROOM, flen3, out3, st3)

        dst3.zero_()
        leg_s()
        torch.cuda.synchronize()
        assert torch.equal(dst3, built) and torch.equal(out3, out) and torch.equal(flen3, flen) and torch.equal(st3, st), per
        legs[f"s{per}_tcp_build_bursts"] = leg_s
        record_bytes[f"s{per}"] = nb * 32 + n * 8
    us = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            us[k].append(round(timed(fn), 2))
    assert torch.equal(dst, built) and torch.equal(dst2, built)
    bytes_per_seg = data_len + L + 32
    r = {"frame_len": L, "algorithmic_bytes_per_segment": bytes_per_seg}
    for k, v in us.items():
        med = sorted(v)[len(v) // 2]
        r[k] = {"us_rounds": v, "us_median": med, "Mseg_per_s": round(n / med, 2), "GB_per_s": round(n * bytes_per_seg / med / 1e3, 1)}
    a_spread = max(us["a_tcp_build"]) / min(us["a_tcp_build"]) - 1
    r["a_round_spread"] = round(a_spread, 4)
    for per in (45, 10, 1):
        r[f"s{per}_over_a"] = round(r[f"s{per}_tcp_build_bursts"]["us_median"] / r["a_tcp_build"]["us_median"], 4)
    r["record_bytes_uploaded"] = record_bytes
    r["b_over_a"] = round(r["b_copy2d_plus_compute_write"]["us_median"] / r["a_tcp_build"]["us_median"], 3)
    r["a_over_c"] = round(r["a_tcp_build"]["us_median"] / r["c_copy2d_alone"]["us_median"], 3)
    res[f"data_len_{data_len}"] = r
    r["d_contiguous_copy"]["GB_per_s"] = round(n * 2 * data_len / r["d_contiguous_copy"]["us_median"] / 1e3, 1)   # its own bytes
    del src, dst, dst2, dst3, built, flat
print(json.dumps(res))

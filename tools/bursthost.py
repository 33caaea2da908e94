"""The host form of the TCP send bursts against the host form of the segment build, from a registered
source into a registered destination at umem geometry: wall time per batch (submit + wait) of
vpcsum_ctx_build_tcp_bursts, its frames described as bursts of 45, 10 and 1, beside
vpcsum_ctx_build_tcp_frames on the per-segment records of the same frames, and the record bytes each
copies into pinned memory.  --batches calls per leg after a warm-up, legs in 3 alternating rounds,
medians.  Both must build the same bytes.  Prints one JSON line.
usage: bursthost.py [frames] [--batches N]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vproxy_amd import vpcsum as V  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 4096
batches = int(sys.argv[sys.argv.index("--batches") + 1]) if "--batches" in sys.argv else 30
rounds = 3
STRIDE, HEADROOM, DATA = 2048, 384, 1460


def page_aligned(nbytes):
    raw = np.zeros(nbytes + 8192, np.uint8)
    skip = (-raw.ctypes.data) % 4096
    return raw, raw[skip:skip + nbytes]


hdr = np.zeros(1, V.TCPHDR_DTYPE)
hdr["l2_len"], hdr["l3_ver"], hdr["ttl"] = 14, 4, 64
hdr["src"][0, :4], hdr["dst"][0, :4] = (10, 0, 0, 1), (10, 0, 0, 2)
keep_a, arena = page_aligned(n * STRIDE)
keep_s, src = page_aligned(n * DATA)
src[:] = np.random.default_rng(1).integers(0, 256, n * DATA, dtype=np.uint8)
fo = np.arange(n, dtype=np.uint64) * STRIDE + HEADROOM
seg = np.zeros(n, V.TCPSEG_DTYPE)
seg["frame_off"], seg["data_off"] = fo, np.arange(n, dtype=np.uint64) * DATA
seg["seq"] = (np.arange(n, dtype=np.uint64) * DATA & 0xffffffff).astype(np.uint32)
seg["frame_cap"], seg["data_len"], seg["flags"] = STRIDE - HEADROOM, DATA, 0x18

ctx = V.Context(0, max_arena=1 << 20, max_pkts=n)
ctx.register(arena)
ctx.register(src)
legs, record_bytes = {}, {"frames": n * 32}
legs["frames"] = lambda: ctx.build_tcp_frames(arena, src, hdr, seg, want_out=False)
for per in (45, 10, 1):
    nb = (n + per - 1) // per
    bu = np.zeros(nb, V.TCPBURST_DTYPE)
    first = np.arange(nb, dtype=np.uint64) * per
    bu["first"], bu["data_off"] = first, first * DATA
    bu["count"] = np.minimum(per, n - first)
    bu["data_len"] = bu["count"] * DATA
    bu["seq"] = (first * DATA & 0xffffffff).astype(np.uint32)
    bu["mss"], bu["flags"] = DATA, 0x18
    legs[f"bursts_of_{per}"] = lambda bu=bu: ctx.build_tcp_bursts(arena, src, hdr, bu, fo, STRIDE - HEADROOM, want_out=False)
    record_bytes[f"bursts_of_{per}"] = nb * 32 + n * 8

try:
    want = None
    for k, fn in legs.items():
        arena[:] = 0
        flen, _, st = fn()
        assert (st == V.S_DONE).all() and (flen == 54 + DATA).all(), k
        if want is None:
            want = arena.copy()
        assert np.array_equal(arena, want), k
    us = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            for _ in range(3):
                fn()
            t = []
            for _ in range(batches):
                t0 = time.perf_counter()
                fn()
                t.append((time.perf_counter() - t0) * 1e6)
            us[k].append(round(sorted(t)[len(t) // 2], 1))
finally:
    ctx.unregister(src)
    ctx.unregister(arena)
    ctx.close()
res = {"frames": n, "data_len": DATA, "batches": batches, "rounds": rounds, "record_bytes_copied": record_bytes}
for k, v in us.items():
    res[k] = {"us_rounds": v, "us_median": sorted(v)[len(v) // 2]}
for per in (45, 10, 1):
    res[f"bursts_of_{per}_over_frames"] = round(res[f"bursts_of_{per}"]["us_median"] / res["frames"]["us_median"], 3)
print(json.dumps(res))

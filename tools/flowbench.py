"""The device-resident NAT fast path on BASELINE config C5 frames (VPCSUM_SYNTH_C5_NAT1500 in Ethernet
frames), timed with events over 100 launches after warm-up, legs in alternating rounds:
  a  vpcsum_parse_ether_tuples_async alone
  b  vpcsum_flow_lookup_async alone: 64 K, 256 K and 1 M flows, 100 % hits and 50 % misses
  c  vpcsum_nat_async with host-prepared 48-B entries (the reference figure: the code before the table)
  d  a + b + c on one stream (1 M flows: every frame's flow is in the table)
  e  d with the Fastpath: parse, vpcsum_flow_lookup_fp_async, rewrite, vpcsum_l2_forward_async (every
     flow carries a Fastpath, so every frame gets its Ethernet addresses written and a port)
  f  vpcsum_l2_forward_async alone, on the verdicts, status bytes and records e left
The flows are the frames' own tuples; every entry rewrites both addresses and both ports to the values
the frame already carries, and every Fastpath carries the Ethernet addresses all frames have, so the
frames -- and their tuples -- stay the same launch after launch.
Prints one JSON line.  usage: flowbench.py [frames] [--launches N]"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vproxy_amd import vpcsum as V  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 1 << 20
launches = int(sys.argv[sys.argv.index("--launches") + 1]) if "--launches" in sys.argv else 100
rounds = 3
stride, l2 = 2048, 14
FLOWS = [min(f, n) for f in (1 << 16, 1 << 18, 1 << 20)]

arena = torch.zeros(n * stride, dtype=torch.uint8, device="cuda")
d = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
V.synth(arena, n, stride, l2, V.SYNTH_C5, 0x20241020, 0, d)
fr = arena.view(n, stride)
fr[:, 12], fr[:, 13] = 0x08, 0x00                # EtherType IPv4
MACS = bytes.fromhex("02aa00000001" "02bb00000002")  # one pair of Ethernet addresses on every frame: e rewrites the same
fr[:, :12] = torch.tensor(list(MACS), dtype=torch.uint8, device="cuda")
fr[:, l2 + 20 + 13] = 0x10                       # TCP: ACK alone (no PUNT); UDP: a payload byte
V.compute(arena, d, n, None, None, V.MODE_WRITE)  # valid stored sums: RFC 1624's premise
foff = (torch.arange(n, dtype=torch.int64, device="cuda") * stride).contiguous()
flen = torch.full((n,), l2 + 1500, dtype=torch.int32, device="cuda")
desc = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
st = torch.zeros(n, dtype=torch.uint8, device="cuda")
tu = torch.zeros(n * 40, dtype=torch.uint8, device="cuda")
rw = torch.zeros(n * 48, dtype=torch.uint8, device="cuda")
vd = torch.zeros(n, dtype=torch.uint8, device="cuda")
V.parse_ether(arena, foff, flen, n, desc, st, tuples=tu)
torch.cuda.synchronize()
assert int(st.sum().item()) == 0, "every C5 frame parses"
tuples = tu.cpu().numpy().view(V.TUPLE_DTYPE).copy()
assert set(np.unique(tuples["l4_proto"])) <= {6, 17} and not (tuples["tcp_flags"] & 7).any()
keys = tuples.copy()
keys["tcp_flags"] = 0
_, first = np.unique(keys.view(np.dtype((np.void, 40))), return_index=True)
distinct = np.sort(first)
# the largest table holds every frame's flow (1 M of them at the default size)
FLOWS = sorted({min(f, len(distinct)) for f in FLOWS})


def flows_of(idx):
    f = np.zeros(len(idx), V.FLOW_DTYPE)
    f["key"] = keys[idx]
    f["rw"]["src"], f["rw"]["dst"] = keys["src"][idx], keys["dst"][idx]
    f["rw"]["sport"], f["rw"]["dport"] = keys["sport"][idx], keys["dport"][idx]
    f["rw"]["mask"] = V.NAT_SRC | V.NAT_DST | V.NAT_SPORT | V.NAT_DPORT
    f["cookie"] = idx
    return f


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


res = {"frames": n, "launches": launches, "rounds": rounds, "workload": "C5_NAT1500 in Ethernet frames, stride 2048"}
legs = {"a_parse_tuples": lambda: V.parse_ether(arena, foff, flen, n, desc, st, tuples=tu)}
tables, info = {}, {}
for F in FLOWS:
    tab = V.FlowTable(F)
    tab.update(add=flows_of(distinct[:F]))
    tables[F], info[F] = tab, tab.info()
    rng = np.random.default_rng(F)
    hit_idx = distinct[rng.integers(0, F, n)]
    # keys not in the table: the distinct tuples past F, or (1 M flows of 1 M frames) made-up source ports
    absent = tuples[hit_idx].copy()
    absent["src"][:, 0] ^= 0x80
    mixed = tuples[hit_idx].copy()
    mixed[1::2] = absent[1::2]
    for name, t in (("hit100", tuples[hit_idx]), ("miss50", mixed)):
        dt = torch.from_numpy(np.ascontiguousarray(t).view(np.uint8).reshape(-1)).pin_memory().cuda()
        tab.lookup(dt, n, rw, vd)
        torch.cuda.synchronize()
        hits = int((vd == V.FLOW_HIT).sum().item())
        assert hits == (n if name == "hit100" else (n + 1) // 2), (name, F, hits)
        legs[f"b_lookup_{F >> 10}K_{name}"] = (lambda tab=tab, dt=dt: tab.lookup(dt, n, rw, vd))
    tab.collect()
big = tables[max(FLOWS)]
# host-prepared entries for c: what the lookup produces for the frames themselves
big.lookup(tu, n, rw, vd)
torch.cuda.synchronize()
res["chain_hit_fraction"] = round(int((vd == V.FLOW_HIT).sum().item()) / n, 4)
rw_host = rw.clone()
legs["c_nat_host_entries"] = lambda: V.nat(arena, desc, rw_host, n, st, V.NAT_RFC1624)


def chain():
    V.parse_ether(arena, foff, flen, n, desc, None, tuples=tu)
    big.lookup(tu, n, rw, vd)
    V.nat(arena, desc, rw, n, st, V.NAT_RFC1624)


legs["d_chain_parse_lookup_nat"] = chain
# e: every flow of the big table gets a Fastpath (the frames' own addresses, port = cookie + 1)
fkeys = keys[distinct[:max(FLOWS)]]
frec = np.zeros(len(fkeys), V.FASTPATH_DTYPE)
frec["dst"], frec["src"] = np.frombuffer(MACS[:6], np.uint8), np.frombuffer(MACS[6:], np.uint8)
frec["port"] = (distinct[:max(FLOWS)] + 1).astype(np.uint32)
assert big.set_fastpath(fkeys, frec) == 0
fp = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
port = torch.zeros(n, dtype=torch.int32, device="cuda")


def chain_fp():
    V.parse_ether(arena, foff, flen, n, desc, None, tuples=tu)
    big.lookup(tu, n, rw, vd, fastpath=fp)
    V.nat(arena, desc, rw, n, st, V.NAT_RFC1624)
    V.l2_forward(arena, foff, flen, vd, st, fp, n, port)


chain_fp()   # f's inputs
torch.cuda.synchronize()
legs["e_chain_fastpath_l2"] = chain_fp
legs["f_l2_forward_alone"] = lambda: V.l2_forward(arena, foff, flen, vd, st, fp, n, port)
before = arena[: 64 * stride].clone()
us = {k: [] for k in legs}
for _ in range(rounds):
    for k, fn in legs.items():
        us[k].append(round(timed(fn), 2))
assert int((st & V.S_BAD_DESC).sum().item()) == 0
assert torch.equal(arena[: 64 * stride], before), "the identity rewrite left the frames as they were"
if res["chain_hit_fraction"] == 1.0:
    assert int((port == 0).sum().item()) == 0, "every frame of e has a port"
for k, v in us.items():
    med = sorted(v)[len(v) // 2]
    res[k] = {"us_rounds": v, "us_median": med, "Gpps": round(n / med / 1e3, 3)}
res["tables"] = {f"{F >> 10}K": info[F] for F in FLOWS}
# counted traffic of one lookup at load factor a = flows / slots (linear probing: a hit reads
# (1 + 1/(1-a))/2 slots on average, a miss (1 + 1/(1-a)^2)/2): tuple 40 B + slots x 128 B read,
# entry 48 B + verdict 1 B (+ 1 mark byte on a hit) written
for F in FLOWS:
    a = info[F]["flows"] / info[F]["slots"]
    ph, pm = (1 + 1 / (1 - a)) / 2, (1 + 1 / (1 - a) ** 2) / 2
    res["tables"][f"{F >> 10}K"].update(load=round(a, 3), bytes_per_hit=round(40 + 128 * ph + 50, 1),
                                        bytes_per_miss=round(40 + 128 * pm + 49, 1), table_MiB=info[F]["slots"] * 128 >> 20)
res["pcie_bound_Gpps_16B_entries"] = 4.0
res["e_over_d"] = round(res["e_chain_fastpath_l2"]["us_median"] / res["d_chain_parse_lookup_nat"]["us_median"], 4)
res["e_minus_d_us"] = round(res["e_chain_fastpath_l2"]["us_median"] - res["d_chain_parse_lookup_nat"]["us_median"], 2)
res["chain_vs_pcie_bound"] = round(res["d_chain_parse_lookup_nat"]["Gpps"] / 4.0, 2)
print(json.dumps(res))

"""The L2 write rule of the flow table's Fastpath (include/vpcsum.h vpcsum_l2_forward_async),
restated in Python for the GPU tests: what EthernetPacket.setDst / setSrc do to a packet that has
its raw bytes -- six bytes at offset 0, six at offset 6, nothing else -- for exactly the frames the
device may forward."""
import numpy as np

FP_DTYPE = np.dtype([("dst", "u1", 6), ("src", "u1", 6), ("port", "<u4")])   # vpcsum_fastpath_t
HIT = 1                                  # VPCSUM_FLOW_HIT
S_DONE, S_BAD_DESC = 0x40, 0x80          # VPCSUM_S_*
ETH_HLEN = 14


def mk_fp(dst: bytes, src: bytes, port: int):
    f = np.zeros(1, FP_DTYPE)
    f["dst"][0] = np.frombuffer(bytes(dst), np.uint8)
    f["src"][0] = np.frombuffer(bytes(src), np.uint8)
    f["port"] = port
    return f[0]


def eligible(verdict: int, status: int, port: int, off: int, length: int, arena_len: int) -> bool:
    """Whether frame (off, length) of an arena of arena_len bytes is forwarded."""
    if length < ETH_HLEN or off + length > arena_len:
        return False
    return verdict == HIT and (status & S_DONE) != 0 and (status & S_BAD_DESC) == 0 and port != 0


def l2_forward(arena: np.ndarray, offs, lens, verdict, status, fps):
    """(arena after the L2 write, ports): the input arena is not changed."""
    out = np.array(arena, np.uint8, copy=True)
    fps = np.asarray(fps, FP_DTYPE)
    ports = np.zeros(len(offs), np.uint32)
    for i in range(len(offs)):
        o, port = int(offs[i]), int(fps["port"][i])
        if not eligible(int(verdict[i]), int(status[i]), port, o, int(lens[i]), len(out)):
            continue
        out[o:o + 6] = fps["dst"][i]
        out[o + 6:o + 12] = fps["src"][i]
        ports[i] = port
    return out, ports

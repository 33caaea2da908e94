"""The rule of the TCP send bursts (include/vpcsum.h vpcsum_tcp_build_bursts_async), restated in
Python for the tests: which burst a frame belongs to, the per-segment record (tests/tcpbuildvec.py's
TCPSEG_DTYPE) it is built from, the refusals -- and a line-by-line transcription of the reference's
SendingQueue.fetch() / fetch0() over a list of queued segments.  Nothing of the library is used here."""
import bisect

import numpy as np

import tcpbuildvec as B

TCPBURST_DTYPE = np.dtype([("data_off", "<u8"), ("data_len", "<u4"), ("seq", "<u4"), ("hdr", "<u4"), ("first", "<u4"),
                           ("mss", "<u2"), ("flags", "u1"), ("rsv", "u1"), ("count", "<u4")])


def count_of(data_len: int, mss: int) -> int:
    """max(1, ceil(data_len / mss))"""
    return max(1, -(-data_len // mss)) if data_len else 1


def mk_burst(data_off, data_len, mss, first, seq=0, hdr=0, flags=B.PSH | B.ACK, rsv=0, count=None):
    b = np.zeros(1, TCPBURST_DTYPE)
    b["data_off"], b["data_len"], b["seq"], b["hdr"], b["first"] = data_off, data_len, seq, hdr, first
    b["mss"], b["flags"], b["rsv"] = mss, flags, rsv
    b["count"] = (count_of(data_len, mss) if mss or not data_len else 0) if count is None else count
    return b[0]


def burst_refused(hdrs, b, frame_cap: int, src_len: int) -> bool:
    """The whole-burst refusals, in the header's order."""
    if int(b["hdr"]) >= len(hdrs):
        return True
    h = hdrs[int(b["hdr"])]
    if not B.hdr_ok(h):
        return True
    if int(b["flags"]) & ~0x3f or int(b["rsv"]) != 0:
        return True
    d, mss = int(b["data_len"]), int(b["mss"])
    if d > 0 and mss == 0:
        return True
    if int(b["count"]) != count_of(d, mss):
        return True
    longest = min(mss, d) if d else 0
    if (40 if int(h["l3_ver"]) == 4 else 20) + longest > 65535:
        return True
    if B.header_len(h) + longest > frame_cap:
        return True
    if int(b["data_off"]) + d > src_len:   # Python integers do not wrap
        return True
    return False


# a record no template accepts: what a frame of a refused burst, or one no burst covers, expands to
def _refused_seg(frame_off: int, frame_cap: int):
    return B.mk_seg(frame_off, 0, 0, hdr=0xffffffff, frame_cap=frame_cap)


def expand(bursts, frame_off, frame_cap: int, hdrs=None, src_len: int | None = None):
    """The TCPSEG_DTYPE records of frames 0..len(frame_off): frame j from the last burst b with
    first[b] <= j, piece k = j - first[b].  A frame of a refused burst (judged when `hdrs` and `src_len`
    are given), a frame with k >= count[b] and a frame before the first burst get a record that
    tcpbuildvec refuses (hdr 0xffffffff).  Returns (records, refused mask); a single frame's own
    destination bound is left to tcpbuildvec.refused."""
    firsts = [int(b["first"]) for b in bursts]
    assert firsts == sorted(firsts), "expand: `first` must be non-decreasing"
    segs = np.zeros(len(frame_off), B.TCPSEG_DTYPE)
    marked = np.zeros(len(frame_off), bool)
    for j, fo in enumerate(frame_off):
        bi = bisect.bisect_right(firsts, j) - 1
        b = bursts[bi] if bi >= 0 else None
        k = j - firsts[bi] if bi >= 0 else 0
        if b is None or k >= int(b["count"]) or (hdrs is not None and burst_refused(hdrs, b, frame_cap, src_len)):
            segs[j], marked[j] = _refused_seg(int(fo), frame_cap), True
            continue
        d, mss = int(b["data_len"]), int(b["mss"])
        skip = k * mss if d else 0
        segs[j] = B.mk_seg(int(fo), int(b["data_off"]) + skip, min(mss, d - skip) if d else 0, seq=(int(b["seq"]) + skip) & 0xffffffff,
                           hdr=int(b["hdr"]), frame_cap=frame_cap, flags=int(b["flags"]), rsv=0)
    return segs, marked


# ------------------------------------------------------------------------------------------
# SendingQueue.fetch() / fetch0() (TcpEntry.java:213-280), line by line
# ------------------------------------------------------------------------------------------
class Segment:
    def __init__(self, seq_begin_inclusive: int, data: bytes):
        self.seqBeginInclusive = seq_begin_inclusive
        self.seqEndExclusive = seq_begin_inclusive + len(data)
        self.data = data


class SendingQueue:
    """The fields fetch() reads; `q` a list of Segment in sequence order."""

    def __init__(self, q, ack_seq: int, window: int, mss: int):
        self.q, self.ackSeq, self.window, self.mss, self.fetchSeq = list(q), ack_seq, window, mss, ack_seq

    def fetch(self):
        endSeq = self.ackSeq + self.mss
        if self.mss > self.window:
            endSeq = self.ackSeq + self.window
        s = self.fetch0(self.ackSeq, endSeq)
        if s is None:
            return []
        ret = [s]
        total = len(s.data)
        while True:
            length = self.mss
            if total + length > self.window:
                length = self.window - total
            if length <= 0:
                break
            s = self.fetch0(self.ackSeq + total, self.ackSeq + total + length)
            if s is None:
                break
            total += len(s.data)
            ret.append(s)
        return ret

    def fetch0(self, begin: int, endExclusive: int):
        if len(self.q) == 0:
            return None
        if self.q[0].seqBeginInclusive > begin:
            return None
        arr = None
        for s in self.q:
            if s.seqBeginInclusive >= endExclusive:
                break
            if s.seqEndExclusive <= begin:
                continue
            data = s.data
            if s.seqBeginInclusive < begin:
                frm = begin - s.seqBeginInclusive
                to = min(endExclusive, s.seqEndExclusive) - s.seqBeginInclusive - (begin - s.seqBeginInclusive)
                data = data[frm:frm + to]      # ByteArray.sub(from, len)
            elif s.seqEndExclusive > endExclusive:
                data = data[0:endExclusive - s.seqBeginInclusive]
            arr = data if arr is None else arr + data
        if arr is None:
            return None
        seg = Segment(begin, arr)
        self.fetchSeq = seg.seqEndExclusive
        return seg

"""CPU-side checks of the NAT flow table: its host logic (vproxy_amd/csrc/flow_table.h) against a
model in a stand-alone program under ASan / UBSan, the layouts the binding and the header share, and
the entry points that need no device (hash, argument refusals)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    from vproxy_amd import build
    lib = ctypes.CDLL(build.build())
    lib.vpcsum_last_error.restype = ctypes.c_char_p
    return lib


def test_flow_table_under_sanitizers(tmp_path):
    """flow_table.h alone (nothing of the library is linked) against a std::map model over a few
    thousand random insert / replace / erase / lookup steps on an 8-slot and a 1,024-slot table:
    after every step each live key is found within max_probe + 1 slots, no probe chain crosses an
    empty slot, flow ids are unique among live flows; a full table and each malformed key are
    refused with nothing changed (tests/cpp/flow_table_test.cpp)."""
    exe = tmp_path / "flow_table_test"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(REPO, "include"), "-I", os.path.join(REPO, "vproxy_amd", "csrc"),
                           os.path.join(REPO, "tests", "cpp", "flow_table_test.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "flow_table ok" in r.stdout, (r.returncode, r.stdout, r.stderr)


def test_flow_dtype_is_the_headers_layout():
    """FLOW_DTYPE equals vpcsum_flow_t as the header declares it: key (vpcsum_tuple_t, 40 B), rw
    (vpcsum_nat_t, 48 B), cookie (uint64), 96 bytes; the verdict values are the header's."""
    from vproxy_amd import vpcsum as V
    src = open(os.path.join(REPO, "include", "vpcsum.h")).read()
    m = re.search(r"typedef struct vpcsum_flow \{(.*?)\} vpcsum_flow_t;", src, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = re.findall(r"(\w+)\s+(\w+)\s*;", body)
    assert fields == [("vpcsum_tuple_t", "key"), ("vpcsum_nat_t", "rw"), ("uint64_t", "cookie")]
    assert V.FLOW_DTYPE.names == ("key", "rw", "cookie")
    assert [V.FLOW_DTYPE.fields[k][1] for k in V.FLOW_DTYPE.names] == [0, 40, 88] and V.FLOW_DTYPE.itemsize == 96
    assert V.FLOW_DTYPE.fields["key"][0] == V.TUPLE_DTYPE and V.TUPLE_DTYPE.itemsize == 40
    assert V.FLOW_DTYPE.fields["rw"][0] == V.NAT_DTYPE and V.NAT_DTYPE.itemsize == 48
    for name, val in (("MISS", V.FLOW_MISS), ("HIT", V.FLOW_HIT), ("PUNT", V.FLOW_PUNT)):
        assert re.search(rf"#define VPCSUM_FLOW_{name}\s+{val}u", src), name


def test_flow_hash_reads_the_38_key_bytes(L):
    """vpcsum_flow_hash without a device: every one of the 38 key bytes changes it, tcp_flags and
    rsv do not, and it is a function of the key alone."""
    from vproxy_amd import vpcsum as V

    def h(k):
        out = ctypes.c_uint64()
        assert L.vpcsum_flow_hash(ctypes.c_void_p(k.ctypes.data), ctypes.byref(out)) == 0
        return out.value

    k = np.zeros(1, V.TUPLE_DTYPE)
    k.view(np.uint8)[:38] = np.arange(1, 39, dtype=np.uint8)
    base = h(k)
    assert base == h(k.copy())
    seen = {base}
    for b in range(38):
        m = k.copy()
        m.view(np.uint8)[b] ^= 0x80
        seen.add(h(m))
    assert len(seen) == 39
    m = k.copy()
    m["tcp_flags"], m["rsv"] = 0x12, 0xff
    assert h(m) == base
    assert L.vpcsum_flow_hash(None, None) != 0 and b"vpcsum_flow_hash" in L.vpcsum_last_error()


def test_flow_kernel_budget(L):
    """The lookup kernel as DESIGN.md §7 describes it: one kernel, no scratch, no LDS, few enough
    registers for full occupancy (read from the code object the build left, no GPU needed)."""
    from test_kernel_resources import kernels
    ks = [v for name, v in kernels("flow.hip.o").items() if "k_flow_lookup" in name]
    assert len(ks) == 1
    assert ks[0]["private_segment_fixed_size"] == 0 and ks[0]["group_segment_fixed_size"] == 0
    assert ks[0]["vgpr_count"] <= 32, ks[0]


def test_flow_entry_points_refuse_null_handles(L):
    """Every flow-table entry point answers a NULL table (or context) with an error and a message,
    before it touches a device."""
    n = ctypes.c_uint32()
    assert L.vpcsum_flowtab_create(0, ctypes.c_uint32(0), None) != 0
    assert L.vpcsum_flowtab_update(None, None, ctypes.c_uint32(0), None, ctypes.c_uint32(0), None) != 0
    assert b"NULL table" in L.vpcsum_last_error()
    assert L.vpcsum_flowtab_info(None, None, None, None) != 0
    assert L.vpcsum_flow_lookup_async(None, None, ctypes.c_uint32(1), None, None, None) != 0
    assert L.vpcsum_flowtab_collect(None, None, ctypes.c_uint32(0), ctypes.byref(n), None) != 0
    t = ctypes.c_uint64()
    assert L.vpcsum_ctx_nat_flow_frames(None, None, None, ctypes.c_uint64(0), None, None, ctypes.c_uint32(0), None, None,
                                        ctypes.c_uint32(0), ctypes.byref(t)) != 0
    assert b"vpcsum_ctx_nat_flow_frames" in L.vpcsum_last_error()
    assert L.vpcsum_flowtab_destroy(None) == 0

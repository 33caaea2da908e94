"""Register, scratch and LDS budgets of the shipped gfx950 kernels, read from the code objects the
build left in vproxy_amd/csrc/*.o (no GPU needed).  They guard what DESIGN.md states and the
launchers assume: every default K2 build (compute and verify, unstaged and staging, and their
window builds for arenas past 4 GiB) fits 6 waves per SIMD (the dense-frame grid is one resident
round of it, §5 items 26, 28, 29), and no default kernel spills to scratch (the NAT rewrite once
kept its accumulator struct there, §7)."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def kernels(obj: str) -> dict:
    """{mangled name: {vgpr_count, private_segment_fixed_size, group_segment_fixed_size}}"""
    path = os.path.join(REPO, "vproxy_amd", "csrc", obj)
    if not os.path.exists(path) or not os.path.exists(os.path.join(LLVM, "clang-offload-bundler")):
        pytest.skip("build artefacts or ROCm LLVM tools missing")
    with tempfile.TemporaryDirectory() as td:
        fat, co = os.path.join(td, "k.fat"), os.path.join(td, "k.co")
        subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), f"--dump-section=.hip_fatbin={fat}", path])
        subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--type=o", f"--input={fat}",
                               f"--targets={TARGET}", f"--output={co}", "--unbundle"])
        notes = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", co], text=True)
    # one YAML map per kernel, its first key marked "- ": collect the keys of each map
    res, cur = {}, None
    entries = []
    for line in notes.splitlines():
        m = re.match(r"(\s+)(- )?\.(\w+):\s+(\S+)", line)
        if not m:
            continue
        indent, dash, key, val = m.groups()
        if dash and len(indent) <= 3:   # a kernel entry (the args' own list items are deeper)
            cur = {}
            entries.append(cur)
        if cur is not None and len(indent) <= 4 and key in ("name", "vgpr_count", "private_segment_fixed_size",
                                                                "group_segment_fixed_size"):
            cur[key] = val if key == "name" else int(val)
    for e in entries:
        if "name" in e:
            res[e.pop("name")] = e
    return res


def pick(ks: dict, pattern: str) -> dict:
    sel = {k: v for k, v in ks.items() if re.search(pattern, k)}
    assert sel, f"no kernel matches {pattern}"
    return sel


def test_k2_default_builds_budgets():
    ks = kernels("kernels.hip.o")
    # k_csum_d<8, 6, 2, 2, VERIFY, NT, 1, 0, -9, true, false, DS, WIN, WGS>: the default builds,
    # their window builds for arenas past 4 GiB (WIN) and the workgroup-sorted build (WGS)
    unstaged_compute = pick(ks, r"k_csum_dILi8ELi6ELi2ELi2ELb0ELb[01]ELi1ELi0ELin9ELb1ELb0ELb0ELb[01]ELb0E")
    staged_compute = pick(ks, r"k_csum_dILi8ELi6ELi2ELi2ELb0ELb[01]ELi1ELi0ELin9ELb1ELb0ELb1ELb[01]ELb0E")
    sorted_units = pick(ks, r"k_csum_dILi8ELi6ELi2ELi2ELb[01]ELb[01]ELi1ELi0ELin9ELb1ELb0ELb1ELb0ELb1E")
    verify = pick(ks, r"k_csum_dILi8ELi6ELi2ELi2ELb1ELb[01]ELi1ELi0ELin9ELb1ELb0ELb[01]ELb[01]ELb[01]E")
    assert len(unstaged_compute) == len(staged_compute) == len(sorted_units) == 4 and len(verify) == 10
    staged_compute.update(sorted_units)
    # every default build fits 6 waves per SIMD (the verify and staging builds since round 4: the
    # stored field written to the slot by the lane that loads it, a scalar wave index, opaque
    # result-store indices)
    for k, v in {**unstaged_compute, **staged_compute, **verify}.items():
        assert v["vgpr_count"] <= 80, (k, v)
    for k, v in {**unstaged_compute, **staged_compute, **verify}.items():
        assert v["private_segment_fixed_size"] == 0, (k, v)
    # the slot plans, and the staged result words: 16 KiB and 26 KiB per workgroup (+ 64 B of class
    # counts in the workgroup-sorted build)
    assert all(v["group_segment_fixed_size"] <= 16384 for v in unstaged_compute.values())
    assert all(v["group_segment_fixed_size"] <= 26624 + 64 for v in staged_compute.values())


def template_args(mangled: str, kernel: str):
    """The integer / bool template arguments of `kernel<...>` in an Itanium-mangled name
    (Li8E -> 8, Lin9E -> -9, Lb1E -> True), or None when the name is another kernel's."""
    m = re.search(rf"\d+{kernel}I((?:L[ib]n?\d+E)+)E", mangled)
    if not m:
        return None
    return tuple(bool(int(v)) if t == "b" else (-int(v[1:]) if v[0] == "n" else int(v))
                 for t, v in re.findall(r"L([ib])(n?\d+)E", m.group(1)))


def compiled_csum_builds():
    ks = kernels("kernels.hip.o")
    d = {a for a in (template_args(k, "k_csum_d") for k in ks) if a is not None}
    t = {a for a in (template_args(k, "k_csum") for k in ks) if a is not None}
    return d, t


def test_template_args_decoder():
    assert template_args("_ZN6vpcsum8k_csum_dILi8ELi6ELi2ELi2ELb0ELb1ELi1ELi0ELin9ELb1ELb0ELb0ELb0ELb0EEEvPKhm", "k_csum_d") == \
        (8, 6, 2, 2, False, True, 1, 0, -9, True, False, False, False, False)
    assert template_args("_ZN6vpcsum6k_csumILi64ELi4ELb1ELb0ELb1EEEvPKhm", "k_csum") == (64, 4, True, False, True)
    assert template_args("_ZN6vpcsum6k_csumILi64ELi4ELb1ELb0ELb1EEEvPKhm", "k_csum_d") is None
    assert template_args("_ZN6vpcsum8k_csum_dILi8ELi6ELi2ELi2ELb0ELb1ELi1ELi0ELin9ELb1ELb0ELb0ELb0ELb0EEEvPKhm", "k_csum") is None
    assert template_args("_ZN6vpcsum14k_csum_serviceEPNS_10SvcMailboxEPjj", "k_csum") is None


def test_csum_build_table_is_the_code_object():
    """tests/csumbuilds.py against kernels.hip.o: the k_csum_d and k_csum kernels compiled for gfx950
    are the table's distinct builds x VERIFY x NT, no more and no fewer -- a build added to
    launch_csum's switch without a row (or a row whose build the switch lost) fails here."""
    import csumbuilds as CB
    got_d, got_t = compiled_csum_builds()
    want_d, want_t = CB.kernel_set()
    assert got_d == want_d, {"compiled, no row": sorted(got_d - want_d), "row, not compiled": sorted(want_d - got_d)}
    assert got_t == want_t, {"compiled, no row": sorted(got_t - want_t), "row, not compiled": sorted(want_t - got_t)}
    assert len(want_d) == 4 * len(CB.K2_BUILDS) == 80 and len(want_t) == 4 * len(CB.team_builds())


def test_csum_build_table_words():
    """The table's mode words: put together from launch_modes.h's named fields they equal
    vpcsum._tune_bits, every id round-trips through the variant fields, and the ids are launch_csum's
    switch as it stands (tests/test_gpu_csum_builds.py::test_id_sweep holds them to the library)."""
    import csumbuilds as CB
    from vproxy_amd import vpcsum
    assert CB.IDS == [0, *range(2, 13), 40, 41, 43, 45, 46, 47, 48, 49, 50, 54, 58, 62, 66, 70, 72, 74, 76, 78, 79, 84]
    for r in CB.ID_ROWS:
        for plain in (False, True):
            for no_adapt in (False, True):
                for wgs in (0, 1, 12, 255):
                    w = r.word(plain, no_adapt, wgs)
                    assert w == vpcsum._tune_bits(r.id, plain, wgs, no_adapt), r.label
                    assert ((w >> 8) & 0x1F) | (((w >> 24) & 7) << 5) == r.id and not w & 0x11   # VERIFY / WRITE free
    assert CB.word(255, True, True, 255) == 0x07FF7F00


def test_no_scratch_in_default_kernels():
    ks = {**kernels("kernels.hip.o"), **kernels("nat.hip.o")}
    # the NAT kernels at their default occupancy (k_natq ... WPE 1), the byte kernel, the lane
    # layout, parse, service, probes, every K2 build (the window builds included); the
    # forced-occupancy tuning shapes (WPE 6 / 8) may spill
    default = {k: v for k, v in ks.items()
               if re.search(r"k_natq\w*ELi1EEEv|k_natw|k_natILi|k_parse_ether|k_csum_service|k_pattern_probe|k_read_probe|"
                            r"k_csum_d", k)}
    assert len(default) > 20
    spills = {k: v["private_segment_fixed_size"] for k, v in default.items() if v["private_segment_fixed_size"]}
    assert not spills, spills

"""CPU-side checks of the product library: it builds, loads, and exports exactly the C-ABI
that include/vpcsum.h declares (no compute calls: there is no GPU here)."""
import ctypes
import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_functions():
    src = open(os.path.join(REPO, "include", "vpcsum.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"^\s*(?:int|const char\*)\s+(\w+)\s*\(", src, re.M)))


@pytest.fixture(scope="module")
def libpath():
    from vproxy_amd import build
    return build.build()


def test_header_declares_expected_surface():
    fns = header_functions()
    assert len(fns) >= 25
    assert "vpcsum_compute_async" in fns and "Java_io_vproxy_vpcsum_VPCsum_submit" in fns


def test_binding_lists_every_header_symbol():
    from vproxy_amd import vpcsum
    assert sorted(vpcsum.EXPORTS) == header_functions()


def test_so_exports_every_declared_symbol(libpath):
    out = subprocess.check_output(["nm", "-D", "--defined-only", libpath], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    missing = [f for f in header_functions() if f not in exported]
    assert not missing, missing


def test_so_loads_and_reports_abi(libpath):
    L = ctypes.CDLL(libpath)
    for f in header_functions():
        assert hasattr(L, f)
    L.vpcsum_abi_version.restype = ctypes.c_int
    assert L.vpcsum_abi_version() == 4


def test_code_object_is_gfx950(libpath):
    # the embedded HIP fat binary names its only target
    data = open(libpath, "rb").read()
    assert b"amdgcn-amd-amdhsa--gfx950" in data
    assert b"gfx942" not in data and b"gfx90a" not in data


def test_fails_loudly_without_library(monkeypatch, tmp_path):
    from vproxy_amd import vpcsum
    monkeypatch.setattr(vpcsum, "_lib", None)
    monkeypatch.setattr(vpcsum, "LIB", str(tmp_path / "missing.so"))
    with pytest.raises(vpcsum.VpcsumUnavailable):
        vpcsum.lib()


def test_descriptor_layout_matches_header():
    from vproxy_amd import vpcsum
    from oracle import oracle as O
    assert vpcsum.DESC_DTYPE == O.DESC_DTYPE and vpcsum.DESC_DTYPE.itemsize == 16
    assert vpcsum.NAT4_DTYPE.itemsize == 16
    assert [vpcsum.DESC_DTYPE.fields[k][1] for k in vpcsum.DESC_DTYPE.names] == [0, 8, 10, 12, 13, 14, 15]


def test_cpp_consumer_builds(libpath, tmp_path):
    """The C-ABI is consumable from plain C++ (no torch, no Python): compile + link only."""
    exe = tmp_path / "capi_smoke"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(REPO, "include"),
                           os.path.join(REPO, "tests", "cpp", "capi_smoke.cpp"), "-L", os.path.dirname(libpath),
                           "-lvpcsum", "-o", str(exe)])
    assert exe.exists()


def test_pni_env_layout_and_errno(libpath, tmp_path):
    """PNIEnv offsets equal the PNI runtime's (pni.h:15-73: message at 8, errno_ at 4104, return_
    at 4112, 4128 bytes), checked by _Static_assert in a C file; running it throws through two PNI
    entry points (argument errors, no GPU needed) and finds type, message and errno_ set."""
    exe = tmp_path / "pni_layout"
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-Wall", "-I", os.path.join(REPO, "include"),
                           os.path.join(REPO, "tests", "cpp", "pni_layout.c"), "-L", os.path.dirname(libpath),
                           "-lvpcsum", "-Wl,-rpath," + os.path.dirname(libpath), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "pni layout ok" in r.stdout, (r.returncode, r.stdout, r.stderr)


def test_batch_plan_under_sanitizers(tmp_path):
    """The host arithmetic of the context's batch path (vproxy_amd/csrc/batch_plan.h: span, 16-B
    block gather, header extents) in a stand-alone program under ASan / UBSan, every buffer at its
    exact size (tests/cpp/batch_plan_test.cpp); nothing of the library is linked."""
    exe = tmp_path / "batch_plan_test"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(REPO, "include"), "-I", os.path.join(REPO, "vproxy_amd", "csrc"),
                           os.path.join(REPO, "tests", "cpp", "batch_plan_test.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "batch_plan ok" in r.stdout, (r.returncode, r.stdout, r.stderr)


@pytest.fixture(scope="module")
def launch_modes_exe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("launch_modes") / "launch_modes_test"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(REPO, "include"), "-I", os.path.join(REPO, "vproxy_amd", "csrc"),
                           os.path.join(REPO, "tests", "cpp", "launch_modes_test.cpp"), "-o", str(exe)])
    return str(exe)


@pytest.fixture(scope="module")
def launch_modes_run(launch_modes_exe):
    return subprocess.run([launch_modes_exe], capture_output=True, text=True, timeout=120)


def test_nat_build_table_is_the_header_list(launch_modes_exe):
    """tests/natbuilds.py names every non-probe NAT rewrite build of launch_modes.h once per entry
    format, nothing missing and nothing twice, and each of its nat_mode words resolves (nat_build)
    to the build it stands next to: 70 builds today, 34 / 20 / 16 by format.  A build added to the
    header without a word in the table -- so without a run against the oracle in
    tests/test_gpu_nat_builds.py -- fails here.  The host program runs under ASan / UBSan."""
    import natbuilds as NB
    args = [f"{b.fmt}:{b.word():#x}" for b in NB.BUILDS]
    r = subprocess.run([launch_modes_exe, "builds"] + args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "builds ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    exists, resolves = [], []
    for line in r.stdout.splitlines():
        f = line.split()
        if f[0] == "exists":
            exists.append(tuple(int(x) for x in f[1:]))
        elif f[0] == "resolves":
            resolves.append((int(f[1]), int(f[2], 16), tuple(int(x) for x in f[3:])))
    assert len(exists) == len(set(exists)), "the header's list names a build twice"
    assert len(resolves) == len(NB.BUILDS)
    for b, (fmt, w, got) in zip(NB.BUILDS, resolves):
        assert (fmt, w) == (b.fmt, b.word()) and got == b.key, (b.id, hex(w), got)
    keys = [b.key for b in NB.BUILDS]
    assert len(set(keys)) == len(keys), "the table names a build twice"
    assert len({b.id for b in NB.BUILDS}) == len(keys)
    assert set(keys) == set(exists), (sorted(set(exists) - set(keys)), sorted(set(keys) - set(exists)))
    by_fmt = {f: sum(1 for k in exists if k[1] == f) for f in (0, 1, 2)}
    assert by_fmt == NB.COUNT_BY_FMT and len(exists) == 70, by_fmt
    # the second-trip test's builds are in the table for both of its formats
    for fam, w in NB.SECOND_TRIP:
        for fmt in (NB.FMT_NAT4, NB.FMT_NAT):
            assert NB.Build(fam, fmt, False, w, 0 if fam == "nat" else 6, 1) in NB.BUILDS
    # the grid field changes the grid alone
    r = subprocess.run([launch_modes_exe, "builds"] + [f"{b.fmt}:{b.word(wgs_per_cu=1):#x}" for b in NB.BUILDS],
                       capture_output=True, text=True, timeout=120)
    got = [tuple(int(x) for x in l.split()[3:]) for l in r.stdout.splitlines() if l.startswith("resolves")]
    assert r.returncode == 0 and got == keys


def test_pre_build_table_is_the_header_list(launch_modes_exe):
    """tests/prebuilds.py names every k_pre build of launch_modes.h once (pre_exists over the
    dispatcher's candidates, the two probes included), and each of its mode words resolves
    (pre_build) to the build it stands next to with exactly the run-time switches asked for: 8
    builds today, 6 / 2 by format.  A build added to the header without a word in the table -- so
    without a run against the oracle in tests/test_gpu_pre_builds.py -- fails here.  The host
    program runs under ASan / UBSan."""
    import prebuilds as PB
    runs = [(b, sw) for b in PB.BUILDS for sw in ((),) + tuple((s,) for s in PB.SWITCHES) + (tuple(PB.SWITCHES),)]
    args = [f"{b.fmt}:{b.word(switches=sw):#x}" for b, sw in runs]
    r = subprocess.run([launch_modes_exe, "prebuilds"] + args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "prebuilds ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    exists, resolves = [], []
    for line in r.stdout.splitlines():
        f = line.split()
        if f[0] == "exists":
            exists.append(tuple(int(x) for x in f[1:]))
        elif f[0] == "resolves":
            resolves.append((int(f[1]), int(f[2], 16), tuple(int(x) for x in f[3:])))
    assert len(exists) == len(set(exists)), "the header's list names a build twice"
    assert len(resolves) == len(runs)
    for (b, sw), (fmt, w, got) in zip(runs, resolves):
        on = tuple(int(s in sw) for s in ("write", "byte_path", "nt_store"))
        assert (fmt, w) == (b.fmt, b.word(switches=sw)) and got == b.key + on, (b.id, sw, hex(w), got)
    keys = [b.key for b in PB.BUILDS]
    assert len(set(keys)) == len(keys), "the table names a build twice"
    assert len({b.id for b in PB.BUILDS}) == len(keys)
    assert set(keys) == set(exists), (sorted(set(exists) - set(keys)), sorted(set(keys) - set(exists)))
    by_fmt = {f: sum(1 for k in exists if k[0] == f) for f in (0, 1)}
    assert by_fmt == PB.COUNT_BY_FMT and len(exists) == 8, by_fmt
    assert sorted(PB.LIVE + PB.PROBES) == sorted(PB.BUILDS) and len(PB.PROBES) == 2
    assert set(sw for run in PB.RUNS for sw in run) == set(PB.SWITCHES)
    # the second-trip test's builds are in the table
    for fmt, w in PB.SECOND_TRIP:
        assert PB.Build(fmt, w, 6, False) in PB.BUILDS
    # the grid field changes the grid alone
    r = subprocess.run([launch_modes_exe, "prebuilds"] + [f"{b.fmt}:{b.word(wgs_per_cu=1):#x}" for b in PB.BUILDS],
                       capture_output=True, text=True, timeout=120)
    got = [tuple(int(x) for x in l.split()[3:7]) for l in r.stdout.splitlines() if l.startswith("resolves")]
    assert r.returncode == 0 and got == keys


def test_launch_modes_under_sanitizers(launch_modes_run):
    """The mode-word decoders (vproxy_amd/csrc/launch_modes.h: accept masks, csum_tune, nat_build,
    nat_probe_build, pre_build) equal a transcription of the launch ladders they replaced on every
    combination of the bits they read, and reach exactly the builds the launchers instantiate
    (tests/cpp/launch_modes_test.cpp, stand-alone under ASan / UBSan)."""
    r = launch_modes_run
    assert r.returncode == 0 and "launch_modes ok" in r.stdout, (r.returncode, r.stdout, r.stderr)


def test_launch_modes_builds_are_the_kernels_built(launch_modes_run):
    """As many NAT / pre-image builds are reachable through the mode words as the code object holds
    k_nat / k_natw / k_natq / k_pre kernels (probes included): a dispatcher that instantiates more
    than the decoders can ask for, or a decoder asking for a kernel that is not built, fails here."""
    from test_kernel_resources import kernels
    ks = kernels("nat.hip.o")
    m = re.search(r"nat builds (\d+) pre builds (\d+)", launch_modes_run.stdout)
    assert m, launch_modes_run.stdout
    assert int(m.group(1)) == len([k for k in ks if re.search(r"k_nat[wq]?ILi", k)])
    assert int(m.group(2)) == len([k for k in ks if re.search(r"k_preILi", k)])


def test_survey_entry_points_refuse_before_init(libpath):
    """SURVEY.md §8(b)'s names (vpcsum_init / vpcsum_batch_submit / vpcsum_batch_wait /
    vpcsum_nat_submit) work over one process-wide group; before vpcsum_init every one of them
    fails with a message instead of touching a device (no GPU call here)."""
    L = ctypes.CDLL(libpath)
    L.vpcsum_last_error.restype = ctypes.c_char_p
    h = ctypes.c_uint64()
    assert L.vpcsum_batch_submit(None, ctypes.c_uint64(0), None, ctypes.c_uint32(0), None, None,
                                 ctypes.c_uint32(0), ctypes.byref(h)) != 0
    assert b"vpcsum_init first" in L.vpcsum_last_error()
    assert L.vpcsum_batch_wait(ctypes.c_uint64(1)) != 0
    assert L.vpcsum_nat_submit(None, ctypes.c_uint64(0), None, None, ctypes.c_uint32(0), None,
                               ctypes.c_uint32(0), ctypes.byref(h)) != 0
    assert L.vpcsum_register_arena(None, ctypes.c_uint64(0)) != 0
    assert L.vpcsum_shutdown() == 0   # nothing to shut down: a no-op


def test_allocation_failure_returns_error(libpath, tmp_path):
    """A host allocation failure inside an extern "C" entry returns -1 with a message instead of
    unwinding a C++ exception into the caller (api.cpp VPC_CATCH): tests/cpp/alloc_fail.cpp makes
    the global operator new throw during vpcsum_group_create_list (no GPU call before it)."""
    exe = tmp_path / "alloc_fail"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(REPO, "include"),
                           os.path.join(REPO, "tests", "cpp", "alloc_fail.cpp"), "-L", os.path.dirname(libpath),
                           "-lvpcsum", "-Wl,-rpath," + os.path.dirname(libpath), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "out of host memory" in r.stdout, (r.returncode, r.stdout, r.stderr)


def test_default_group_calls_race_shutdown_without_gpu(libpath):
    """The process-wide group's entry points from several threads racing vpcsum_shutdown (no GPU
    here, so every call is refused): no crash, every refusal says "vpcsum_init first"."""
    import threading
    L = ctypes.CDLL(libpath)
    L.vpcsum_last_error.restype = ctypes.c_char_p
    bad = []

    def worker():
        h = ctypes.c_uint64()
        for _ in range(2000):
            if L.vpcsum_batch_submit(None, ctypes.c_uint64(0), None, ctypes.c_uint32(0), None, None,
                                     ctypes.c_uint32(0), ctypes.byref(h)) == 0 or \
                    b"vpcsum_init first" not in L.vpcsum_last_error():
                bad.append(1)
            L.vpcsum_batch_wait(ctypes.c_uint64(1))

    ts = [threading.Thread(target=worker) for _ in range(4)]
    for t in ts:
        t.start()
    for _ in range(2000):
        assert L.vpcsum_shutdown() == 0
    for t in ts:
        t.join()
    assert not bad


def test_registration_audit_covers_every_page():
    """The release audit (vpcsum._audit_points) asks HIP about both ends of a released range and
    one address in every page between them, at most 256 spread evenly over a larger range."""
    from vproxy_amd.vpcsum import _audit_points
    p, n = 0x1010, 164238
    pts = _audit_points(p, n)
    assert p in pts and p + n - 1 in pts
    assert {q >> 12 for q in pts} == set(range(p >> 12, ((p + n - 1) >> 12) + 1))
    assert all(p <= q < p + n for q in pts)
    big = _audit_points(0x10, 1 << 30)
    assert len(big) <= 258 and min(big) == 0x10 and max(big) == 0x10 + (1 << 30) - 1
    assert _audit_points(0x2000, 1) == [0x2000, 0x2000]

"""The row-major feature products (include/hisparse_wide.h) without a GPU: the cases of tests/wide_cases.py on libhisparse_cpu.so, each in
a child process with HISPARSE_HIP_LIB set (as tests/test_pattern_cpu.py runs its cases); header, libraries and binding in agreement on
exactly twelve names; the binding's launch constants against wide_products.h; the CPU twin's source under the sanitizers as a
stand-alone program.  The same cases on the device: tests/test_gpu_wide.py."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "hisparse_amd", "lib")
CPU_LIB = os.path.join(LIBDIR, "libhisparse_cpu.so")

CHILD = r"""
import sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import numpy as np
from hisparse_amd import device, wide
import wide_cases as wc
assert device._LIB_PATH.endswith("libhisparse_cpu.so")
mem = wc.HostMemory()
%(body)s
print("wide child ok")
"""

NAMES = ["hsw_create", "hsw_destroy", "hsw_info", "hsw_last_error", "hsw_sddmm", "hsw_sddmm_device", "hsw_set_stream", "hsw_spmm", "hsw_spmm_device", "hsw_spmm_t",
         "hsw_spmm_t_device", "hsw_sync"]


def run_child(body):
    if not os.path.exists(CPU_LIB):
        subprocess.check_call(["make", "-C", ROOT, "cpu"], stdout=subprocess.DEVNULL)
    env = dict(os.environ, HISPARSE_HIP_LIB=CPU_LIB)
    for k in [k for k in env if k.startswith("HISPARSE_") and k != "HISPARSE_HIP_LIB"]:
        env.pop(k)
    r = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests"), "body": body}], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "wide child ok" in r.stdout, r.stdout + r.stderr
    return r.stdout


def test_general():
    """300 x 517, 4000 entries, d in {1, 3, 4, 5, 16, 17, 63, 64, 65, 128, 256}, pad 0 and 8, the three calls, host and device form"""
    run_child("wc.general(mem)")


def test_edges():
    run_child("wc.edges(mem)")


def test_non_finite_values():
    run_child("wc.non_finite(mem)")


def test_adjoint_identities():
    run_child("wc.adjoint(mem)")


def test_a_call_leaves_nothing_for_the_next():
    run_child("wc.nothing_carried_over(mem)")


def test_refusals():
    run_child("wc.refusals(mem)")


def test_info_holds_nothing_on_a_device():
    run_child("with wide.WideProducts((np.array([0, 2, 2, 3], dtype=np.uint32), np.array([1, 0, 1], dtype=np.uint32), (3, 2))) as wp:\n"
              "    assert wp.info() == {'nnz': 3, 'device_bytes': 0}")


def prototypes():
    text = open(os.path.join(ROOT, "include", "hisparse_wide.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(hsw_[a-z0-9_]+)\s*\(", text)))


def test_header_libraries_and_binding_agree():
    from hisparse_amd import device, pattern, rows, wide
    names = prototypes()
    assert names == NAMES and len(names) == 12
    assert sorted(wide.EXPORTS) == names
    assert not set(names) & (set(device.EXPORTS) | set(pattern.EXPORTS) | set(rows.EXPORTS))      # an object of its own
    for lib in ("libhisparse_hip.so", "libhisparse_cpu.so"):
        exported = subprocess.run(["nm", "-D", "--defined-only", os.path.join(LIBDIR, lib)], capture_output=True, text=True, check=True).stdout
        assert sorted(set(re.findall(r"\b(hsw_[a-z0-9_]+)\b", exported))) == names, lib
        l = ctypes.CDLL(os.path.join(LIBDIR, lib))
        for n in names:
            assert hasattr(l, n), (lib, n)
    bound = wide.lib()
    for n in names:
        assert getattr(bound, n).argtypes is not None, n
    import hisparse_amd
    assert hisparse_amd.wide is wide
    hip_h = open(os.path.join(ROOT, "include", "hisparse_hip.h")).read()
    assert "hisparse_wide.h" in hip_h and not re.search(r"\bhsw_[a-z_]+\s*\(", re.sub(r"/\*.*?\*/", "", hip_h, flags=re.S))


def test_launch_constants_of_the_binding_are_the_kernels():
    from hisparse_amd import wide
    text = open(os.path.join(ROOT, "hisparse_amd", "csrc", "wide_products.h")).read()
    got = {n: int(v) for n, v in re.findall(r"constexpr uint32_t (kWide\w+) = (\d+);", text)}
    assert got == {"kWideThreads": wide.WIDE_THREADS, "kWideBlocksPerCu": wide.WIDE_BLOCKS_PER_CU, "kWideInFlight": wide.WIDE_IN_FLIGHT, "kWideLong": wide.WIDE_LONG,
                   "kWideMaxD": wide.MAX_D, "kWideClasses": 4}
    common = open(os.path.join(ROOT, "hisparse_amd", "csrc", "hsw_common.h")).read()
    assert int(re.search(r"kMaxD = (\d+);", common).group(1)) == wide.MAX_D == 256
    assert [wide.group_lanes(d) for d in (1, 4, 5, 16, 17, 64, 65, 128, 129, 256)] == [1, 1, 2, 4, 8, 16, 32, 32, 64, 64]
    assert [wide.team_lanes(c, 4) for c in (1, 2, 3)] == [4, 16, 64] and [wide.team_lanes(c, 64) for c in (1, 2, 3)] == [64, 64, 64] and wide.team_lanes(1, 256) == 64
    assert wide.rows_per_trip(256, 1, 4) == 256 * wide.WIDE_BLOCKS_PER_CU * 64


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present")
def test_hip_library_has_no_cpu_fallback():
    from hisparse_amd import device, wide
    if not device._LIB_PATH.endswith("libhisparse_hip.so"):
        pytest.skip("another library is selected")
    with pytest.raises(device.DeviceError) as e:
        wide.WideProducts((np.array([0, 1], dtype=np.uint32), np.array([0], dtype=np.uint32), (1, 1)))
    assert e.value.code in (-2, -3) and str(e.value)


def test_cpu_twin_stand_alone_under_the_sanitizers(tmp_path):
    """tests/cpp/test_wide_cpu.cpp: the edge patterns and the refusals through the C boundary, compiled together with hsw_cpu.cpp under
    -fsanitize=address,undefined with the runtimes linked in statically (a program of its own, whatever else the environment preloads:
    nothing loaded into python is run under a sanitizer)."""
    exe = tmp_path / "wide_cpu"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           f"-I{ROOT}/include", f"-I{ROOT}/hisparse_amd/csrc", f"{ROOT}/tests/cpp/test_wide_cpu.cpp", f"{ROOT}/hisparse_amd/csrc/hsw_cpu.cpp", "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "WIDE CPU OK" in out.stdout, out.stdout + out.stderr

"""The row softmax (include/hisparse_rows.h) without a GPU: the cases of tests/rows_cases.py on libhisparse_cpu.so, each in a child
process with HISPARSE_HIP_LIB set (as tests/test_pattern_cpu.py runs its cases); header, libraries and binding in agreement on exactly
ten names; the binding's launch constants against row_softmax.h; the CPU twin's source under the sanitizers as a stand-alone program.
The same cases on the device: tests/test_gpu_rows.py."""
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
from hisparse_amd import device, rows
import rows_cases as rc
assert device._LIB_PATH.endswith("libhisparse_cpu.so")
mem = rc.HostMemory()
%(body)s
print("rows child ok")
"""


def run_child(body):
    if not os.path.exists(CPU_LIB):
        subprocess.check_call(["make", "-C", ROOT, "cpu"], stdout=subprocess.DEVNULL)
    env = dict(os.environ, HISPARSE_HIP_LIB=CPU_LIB)
    for k in [k for k in env if k.startswith("HISPARSE_") and k != "HISPARSE_HIP_LIB"]:
        env.pop(k)
    r = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests"), "body": body}], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "rows child ok" in r.stdout, r.stdout + r.stderr
    return r.stdout


def test_general():
    """223 rows of every class, about 13 000 entries, four (scale, magnitude) pairs, forward and backward, host and device form, in place"""
    print(run_child("rc.general(mem)"))


def test_exact_answers():
    run_child("rc.exact_answers(mem)")


def test_non_finite_scores():
    run_child("rc.non_finite(mem)")


def test_edges():
    run_child("rc.edges(mem)")


def test_refusals():
    run_child("rc.refusals(mem)")


def test_info_holds_nothing_on_a_device():
    run_child("with rows.RowSoftmax(rc.indptr_of([3, 0, 2])) as rs:\n    assert rs.info() == {'nnz': 5, 'device_bytes': 0}")


def prototypes():
    text = open(os.path.join(ROOT, "include", "hisparse_rows.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(hsr_[a-z0-9_]+)\s*\(", text)))


def test_header_libraries_and_binding_agree():
    from hisparse_amd import device, pattern, rows
    names = prototypes()
    assert len(names) == 10 and "hsr_create" in names and "hsr_softmax_backward_device" in names
    assert sorted(rows.EXPORTS) == names
    assert not set(names) & set(device.EXPORTS) and not set(names) & set(pattern.EXPORTS)      # an object of its own
    for lib in ("libhisparse_hip.so", "libhisparse_cpu.so"):
        exported = subprocess.run(["nm", "-D", "--defined-only", os.path.join(LIBDIR, lib)], capture_output=True, text=True, check=True).stdout
        assert sorted(set(re.findall(r"\b(hsr_[a-z0-9_]+)\b", exported))) == names, lib
        l = ctypes.CDLL(os.path.join(LIBDIR, lib))
        for n in names:
            assert hasattr(l, n), (lib, n)
    bound = rows.lib()
    for n in names:
        assert getattr(bound, n).argtypes is not None, n
    import hisparse_amd
    assert hisparse_amd.rows is rows


def test_launch_constants_of_the_binding_are_the_kernels():
    from hisparse_amd import rows
    text = open(os.path.join(ROOT, "hisparse_amd", "csrc", "row_softmax.h")).read()
    got = {n: int(v) for n, v in re.findall(r"constexpr uint32_t (kRows\w+) = (\d+);", text)}
    assert got == {"kRowsThreads": rows.ROWS_THREADS, "kRowsBlocksPerCu": rows.ROWS_BLOCKS_PER_CU, "kRowsPerLane": rows.ROWS_PER_LANE, "kRowsLong": rows.ROWS_LONG,
                   "kRowsClasses": 6, "kRowsTableWords": 16}
    assert rows.ROWS_LONG == rows.ROWS_PER_LANE * 64 and rows.rows_per_trip(256, 4) == 256 * rows.ROWS_BLOCKS_PER_CU * 64


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present")
def test_hip_library_has_no_cpu_fallback():
    from hisparse_amd import device, rows
    if not device._LIB_PATH.endswith("libhisparse_hip.so"):
        pytest.skip("another library is selected")
    with pytest.raises(device.DeviceError) as e:
        rows.RowSoftmax(np.array([0, 1], dtype=np.uint32))
    assert e.value.code in (-2, -3) and str(e.value)


def test_cpu_twin_stand_alone_under_the_sanitizers(tmp_path):
    """tests/cpp/test_rows_cpu.cpp: the edges and the refusals through the C boundary, compiled together with hsr_cpu.cpp under
    -fsanitize=address,undefined with the runtimes linked in statically (a program of its own, whatever else the environment preloads:
    nothing loaded into python is run under a sanitizer)."""
    exe = tmp_path / "rows_cpu"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           f"-I{ROOT}/include", f"-I{ROOT}/hisparse_amd/csrc", f"{ROOT}/tests/cpp/test_rows_cpu.cpp", f"{ROOT}/hisparse_amd/csrc/hsr_cpu.cpp", "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "ROWS CPU OK" in out.stdout, out.stdout + out.stderr

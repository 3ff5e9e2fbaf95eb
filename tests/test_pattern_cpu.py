"""The sampled dense product (include/hisparse_pattern.h) without a GPU: the cases of tests/pattern_cases.py on libhisparse_cpu.so, each
in a child process with HISPARSE_HIP_LIB set (as tests/test_context_model_cpu.py runs its driver); the fixed-point reference pinned to
the oracle; header, libraries and binding in agreement; the CPU twin's source under the sanitizers as a stand-alone program.  The same
cases on the device: tests/test_gpu_pattern.py."""
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
from hisparse_amd import device, host, pattern
import pattern_cases as pc
assert device._LIB_PATH.endswith("libhisparse_cpu.so")
mem = pc.HostMemory()
%(body)s
print("pattern child ok")
"""


def run_child(body):
    if not os.path.exists(CPU_LIB):
        subprocess.check_call(["make", "-C", ROOT, "cpu"], stdout=subprocess.DEVNULL)
    env = dict(os.environ, HISPARSE_HIP_LIB=CPU_LIB)
    for k in [k for k in env if k.startswith("HISPARSE_") and k != "HISPARSE_HIP_LIB"]:
        env.pop(k)
    r = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests"), "body": body}], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "pattern child ok" in r.stdout, r.stdout + r.stderr
    return r.stdout


ORACLE_PIN = r"""
from oracle import oracle as orc
# one non-zero per row: value word u[r] at column c[r]; through host's formatter and the oracle y[r] = q8_24_mul(u[r], v[c[r]])
pairs = [(1.0 / (1 << 24), 0.5), (3.0 / (1 << 24), 0.5), (1.0 / (1 << 24), 0.5 - 1.0 / (1 << 24)), (5.0 / (1 << 24), 0.75),      # round up, round up, round down, tie-free
         (200.0, 1.5), (255.0, 255.0), (16.0, 16.0), (255.99, 1.0),                                                              # saturate ... just not
         (0.0, 1.25), (1.25, 0.0), (0.0, 0.0), (1.0, 1.0), (1.9999999, 1.9999999)]
rng = np.random.default_rng(7)
rows, cols = 128, 40
uf = np.array([p[0] for p in pairs] + list(rng.uniform(0.0, 2.0, rows - len(pairs))), dtype=np.float32)
c = rng.integers(0, cols, rows).astype(np.uint32)
vf = rng.uniform(0.0, 2.0, cols).astype(np.float32)
for i, p in enumerate(pairs):                 # give every designed pair a column of its own
    c[i] = i
    vf[i] = p[1]
c[len(pairs):] = rng.integers(len(pairs), cols, rows - len(pairs))
indptr = np.arange(rows + 1, dtype=np.uint32)
csr = host.CSRMatrix.from_arrays(rows, cols, indptr, c, uf)
cp = host.format_matrix(csr, 0, skip_empty_rows=True)
assert cp.num_rows == rows and cp.num_cols == cols
u, v = host.pack_vector(0, uf), host.pack_vector(0, vf)
y = orc.spmv(0, [cp.channel_ptr(ch)[0] for ch in range(16)], v, cp.num_rows, cp.num_cols, cp.num_row_partitions, cp.num_col_partitions, cp.ob_bank, cp.vb_bank)
a, b = u.astype(object), v[c].astype(object)
restated = np.array([min((int(x) * int(z) + (1 << 23)) >> 24, (1 << 32) - 1) for x, z in zip(a, b)], dtype=np.uint64)
assert np.array_equal(y.astype(np.uint64), restated), "the numpy restatement is not the oracle's product"
assert np.array_equal(pc.q_mul(u, v[c]), restated)
up = [(int(x) * int(z)) >> 23 & 1 for x, z in zip(a, b)]
assert sum(up) >= 20 and restated[0] == 1 and restated[1] == 2 and restated[2] == 0                 # pairs that round up, and one that does not
assert (restated[4:7] == pc.SAT).all() and restated[7] < pc.SAT and not restated[8:11].any()         # pairs that saturate, zeros
with pattern.SampledProduct(0, (indptr, c, (rows, cols)), 1) as sp:
    got = sp.sddmm(u[None, :], v[None, :])
assert np.array_equal(got.astype(np.uint64), restated), "k = 1 over the same pattern is not the oracle's product"
"""


def test_fixed_point_reference_is_the_oracles_product():
    run_child(ORACLE_PIN)


@pytest.mark.parametrize("impl", [0, 1, 2])
def test_general(impl):
    """300 x 517, about 4000 entries, k in {1, 3, 4, 5, 16, 17, 64}, host and device form; saturating sums; accumulate 5 + 12 = 17"""
    run_child(f"pc.general(mem, ({impl},))")


def test_both_float_modes_give_the_same_words():
    run_child("w = pc.general(mem, (1, 2))\nassert all(np.array_equal(w[1][k], w[2][k]) for k in pc.KS)")


def test_nan_reaches_exactly_its_entry():
    run_child("pc.nan_reaches_its_entry(mem, (1, 2))")


def test_pattern_edges():
    run_child("pc.edges(mem, (0, 1, 2))")


def test_refusals():
    run_child("pc.refusals(mem, (0, 1, 2))")


def prototypes():
    text = open(os.path.join(ROOT, "include", "hisparse_pattern.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(hsp_[a-z0-9_]+)\s*\(", text)))


def test_header_libraries_and_binding_agree():
    from hisparse_amd import device, pattern
    names = prototypes()
    assert len(names) == 8 and "hsp_create" in names and "hsp_sddmm_device" in names
    assert sorted(pattern.EXPORTS) == names
    assert not set(names) & set(device.EXPORTS)                     # an object of its own: the context's list is untouched
    for lib in ("libhisparse_hip.so", "libhisparse_cpu.so"):
        l = ctypes.CDLL(os.path.join(LIBDIR, lib))
        for n in names:
            assert hasattr(l, n), (lib, n)
    bound = pattern.lib()
    for n in names:
        assert getattr(bound, n).argtypes is not None, n
    hip_h = open(os.path.join(ROOT, "include", "hisparse_hip.h")).read()
    assert "hisparse_pattern.h" in hip_h and not re.search(r"\bhsp_[a-z_]+\s*\(", re.sub(r"/\*.*?\*/", "", hip_h, flags=re.S))


def test_launch_constants_of_the_binding_are_the_kernels():
    from hisparse_amd import pattern
    text = open(os.path.join(ROOT, "hisparse_amd", "csrc", "sddmm.h")).read()
    got = {n: int(v) for n, v in re.findall(r"constexpr uint32_t (kSddmm\w+) = (\d+);", text)}
    assert got == {"kSddmmThreads": pattern.SDDMM_THREADS, "kSddmmBlocksPerCu": pattern.SDDMM_BLOCKS_PER_CU, "kSddmmEntriesPerLane": pattern.SDDMM_ENTRIES_PER_LANE}
    common = open(os.path.join(ROOT, "hisparse_amd", "csrc", "hsp_common.h")).read()
    assert int(re.search(r"kMaxK = (\d+);", common).group(1)) == pattern.MAX_K == 64


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present")
def test_hip_library_has_no_cpu_fallback():
    from hisparse_amd import device, pattern
    if not device._LIB_PATH.endswith("libhisparse_hip.so"):
        pytest.skip("another library is selected")
    with pytest.raises(device.DeviceError) as e:
        pattern.SampledProduct(0, (np.array([0, 1], dtype=np.uint32), np.array([0], dtype=np.uint32), (1, 1)), 1)
    assert e.value.code in (-2, -3) and str(e.value)


def test_cpu_twin_stand_alone_under_the_sanitizers(tmp_path):
    """tests/cpp/test_pattern_cpu.cpp: the edge patterns and the refusals through the C boundary, compiled together with hsp_cpu.cpp
    under -fsanitize=address,undefined with the runtimes linked in statically (a program of its own, whatever else the environment
    preloads: nothing loaded into python is run under a sanitizer)."""
    exe = tmp_path / "pattern_cpu"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           f"-I{ROOT}/include", f"-I{ROOT}/hisparse_amd/csrc", f"{ROOT}/tests/cpp/test_pattern_cpu.cpp", f"{ROOT}/hisparse_amd/csrc/hsp_cpu.cpp", "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "PATTERN CPU OK" in out.stdout, out.stdout + out.stderr

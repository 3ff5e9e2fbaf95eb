"""The fused attention step (include/hisparse_attention.h) without a GPU: the cases of tests/attention_cases.py on libhisparse_cpu.so, each
in a child process with HISPARSE_HIP_LIB set (as tests/test_wide_cpu.py runs its cases); the reference against three planted defects;
header, libraries and binding in agreement on exactly eight names; the CPU twin's source under the sanitizers as a stand-alone program;
the kernel's code-object metadata.  The same cases on the device: tests/test_gpu_attention.py."""
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
from hisparse_amd import attention, device
import attention_cases as ac
assert device._LIB_PATH.endswith("libhisparse_cpu.so")
mem = ac.HostMemory()
%(body)s
print("attention child ok")
"""

NAMES = ["hsat_create", "hsat_destroy", "hsat_forward", "hsat_forward_device", "hsat_info", "hsat_last_error", "hsat_set_stream", "hsat_sync"]


def run_child(body):
    if not os.path.exists(CPU_LIB):
        subprocess.check_call(["make", "-C", ROOT, "cpu"], stdout=subprocess.DEVNULL)
    env = dict(os.environ, HISPARSE_HIP_LIB=CPU_LIB)
    for k in [k for k in env if k.startswith("HISPARSE_") and k != "HISPARSE_HIP_LIB"]:
        env.pop(k)
    r = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests"), "body": body}], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "attention child ok" in r.stdout, r.stdout + r.stderr
    return r.stdout


def test_general():
    """300 x 517, 4000 entries, d in {1, 3, 4, 5, 16, 17, 63, 64, 65, 128, 256}, scale 0.125, 1 and -2, pad 0 and 8, lse taken and NULL"""
    run_child("ac.general(mem)")


def test_edges():
    run_child("ac.edges(mem)")


def test_score_order():
    run_child("ac.score_order(mem)")


def test_non_finite_scores():
    run_child("ac.non_finite(mem)")


def test_scale_zero():
    run_child("ac.scale_zero(mem)")


def test_heads_by_leading_dimension():
    run_child("ac.heads(mem)")


def test_a_call_leaves_nothing_for_the_next():
    run_child("ac.nothing_carried_over(mem)")


def test_refusals():
    run_child("ac.refusals(mem)")


def test_info_holds_nothing_on_a_device():
    run_child("with attention.PatternAttention((np.array([0, 2, 2, 3], dtype=np.uint32), np.array([1, 0, 1], dtype=np.uint32), (3, 2))) as pa:\n"
              "    assert pa.info() == {'nnz': 3, 'device_bytes': 0}")


def test_reference_rejects_planted_defects():
    """No library involved: a correct result (the reference's own words, rounded once) passes, and each of three defects applied to it
    is rejected: the last entry of every row with n >= 2 left out, a finite pad word (index d of a row with ld > d) included in the
    dot, lse without the maximum added back."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import attention_cases as ac
    indptr, indices = ac.random_pattern(ac.ROWS, ac.COLS, ac.NNZ, 9)
    shape, d, scale = (ac.ROWS, ac.COLS), 5, 1.0
    Q, K, V = ac.operands(shape, 8, 2000)                       # rows of ld = 8 words: word 5 is a finite pad word
    q, k, v = (np.ascontiguousarray(a[:, :d]) for a in (Q, K, V))
    ref = ac.reference(indptr, indices, q, k, v, scale)
    y, lse = ref.rounded()
    assert ref.check(y, lse, "a correct result") <= 1.0
    # the last entry of every row with n >= 2 left out
    n = np.diff(indptr.astype(np.int64))
    keep = np.ones(indices.size, dtype=bool)
    keep[(indptr[1:].astype(np.int64) - 1)[n >= 2]] = False
    short = np.concatenate([[0], np.cumsum(n - (n >= 2))]).astype(np.uint32)
    wrong_y, wrong_lse = ac.reference(short, indices[keep], q, k, v, scale).rounded()
    with pytest.raises(AssertionError, match="words of y break"):
        ref.check(wrong_y, lse, "last entries left out")
    with pytest.raises(AssertionError, match="lse words break"):
        ref.check(y, wrong_lse, "last entries left out")
    # a pad word in the dot
    wrong_y, wrong_lse = ac.reference(indptr, indices, np.ascontiguousarray(Q[:, :d + 1]), np.ascontiguousarray(K[:, :d + 1]), v, scale).rounded()
    with pytest.raises(AssertionError, match="words of y break"):
        ref.check(wrong_y[:, :d], lse, "pad word in the dot")
    with pytest.raises(AssertionError, match="lse words break"):
        ref.check(y, wrong_lse, "pad word in the dot")
    # lse without the maximum
    with pytest.raises(AssertionError, match="lse words break"):
        ref.check(y, np.where(ref.finite, np.log(np.where(ref.finite, ref.L, 1.0)), -np.inf).astype(np.float32), "lse without the maximum")


def prototypes():
    text = open(os.path.join(ROOT, "include", "hisparse_attention.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(hsat_[a-z0-9_]+)\s*\(", text)))


def test_header_libraries_and_binding_agree():
    from hisparse_amd import attention, device, pattern, rows, wide
    names = prototypes()
    assert names == NAMES and len(names) == 8
    assert sorted(attention.EXPORTS) == names
    assert not set(names) & (set(device.EXPORTS) | set(pattern.EXPORTS) | set(rows.EXPORTS) | set(wide.EXPORTS))      # an object of its own
    for lib in ("libhisparse_hip.so", "libhisparse_cpu.so"):
        exported = subprocess.run(["nm", "-D", "--defined-only", os.path.join(LIBDIR, lib)], capture_output=True, text=True, check=True).stdout
        assert sorted(set(re.findall(r"\b(hsat_[a-z0-9_]+)\b", exported))) == names, lib
        l = ctypes.CDLL(os.path.join(LIBDIR, lib))
        for n in names:
            assert hasattr(l, n), (lib, n)
    bound = attention.lib()
    for n in names:
        assert getattr(bound, n).argtypes is not None, n
    import hisparse_amd
    assert hisparse_amd.attention is attention
    hip_h = open(os.path.join(ROOT, "include", "hisparse_hip.h")).read()
    assert "hisparse_attention.h" in hip_h and not re.search(r"\bhsat_[a-z_]+\s*\(", re.sub(r"/\*.*?\*/", "", hip_h, flags=re.S))


def test_schedule_is_the_wide_products_unchanged():
    """pattern_attention.h adds no kWide* constant and the kernel's launcher takes the classes, teams and grid cap from wide_products.h"""
    text = open(os.path.join(ROOT, "hisparse_amd", "csrc", "pattern_attention.h")).read()
    assert '#include "wide_products.h"' in text and not re.search(r"constexpr\s+\w+\s+kWide", text)
    hip = open(os.path.join(ROOT, "hisparse_amd", "csrc", "pattern_attention.hip")).read()
    for name in ("wide_table", "wide_group_lanes", "kWideBlocksPerCu", "kWideInFlight", "kWideThreads"):
        assert name in hip, name


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present")
def test_hip_library_has_no_cpu_fallback():
    from hisparse_amd import attention, device
    if not device._LIB_PATH.endswith("libhisparse_hip.so"):
        pytest.skip("another library is selected")
    with pytest.raises(device.DeviceError) as e:
        attention.PatternAttention((np.array([0, 1], dtype=np.uint32), np.array([0], dtype=np.uint32), (1, 1)))
    assert e.value.code in (-2, -3) and str(e.value)


def test_cpu_twin_stand_alone_under_the_sanitizers(tmp_path):
    """tests/cpp/test_attention_cpu.cpp: the edge patterns and the refusals through the C boundary, compiled together with hsat_cpu.cpp
    under -fsanitize=address,undefined with the runtimes linked in statically (a program of its own: nothing loaded into python is run
    under a sanitizer)."""
    exe = tmp_path / "attention_cpu"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", f"-I{ROOT}/include", f"-I{ROOT}/hisparse_amd/csrc", f"{ROOT}/tests/cpp/test_attention_cpu.cpp", f"{ROOT}/hisparse_amd/csrc/hsat_cpu.cpp",
                           "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "ATTENTION CPU OK" in out.stdout, out.stdout + out.stderr


def test_kernel_uses_no_scratch(tmp_path):
    """code-object metadata only: the fused kernel's private segment is empty (no spills, no runtime-indexed arrays in scratch)"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_isa_invariants as isa
    if not os.path.exists(isa.LIB):
        pytest.skip("libhisparse_hip.so has not been built")
    if not os.path.exists(f"{isa.LLVM}/llvm-readelf"):
        pytest.skip("no llvm-readelf")
    meta = {}
    for co in isa._code_objects(tmp_path):
        meta.update(isa._metadata(co))
    mine = {n: m for n, m in meta.items() if "pattern_attention_kernel" in n}
    assert len(mine) == 1, sorted(mine)
    for n, m in mine.items():
        assert m["private_segment_fixed_size"] == 0, (n, m)
        assert m["group_segment_fixed_size"] <= 8192 + 64, (n, m)

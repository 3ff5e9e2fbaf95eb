"""The GATv2 calls (include/hisparse_gatv2.h) without a GPU: the reference of tests/gatv2_cases.py against torch's float64 autograd first,
then its cases on libhisparse_cpu.so, each in a child process with HISPARSE_HIP_LIB set (as tests/test_gat_cpu.py runs its cases); the
checker against three planted defects; header, libraries and binding in agreement on exactly six functions; the kernels' source on the
unchanged schedule; the launch counts the header states.  The same cases on the device: tests/test_gpu_gatv2.py."""
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
from hisparse_amd import device, heads, gatv2
import gatv2_cases as gc
assert device._LIB_PATH.endswith("libhisparse_cpu.so")
mem = gc.HostMemory()
%(body)s
print("gatv2 child ok")
"""

NAMES = ["hsgat2_backward", "hsgat2_backward_device", "hsgat2_forward", "hsgat2_forward_device", "hsgat2_work_bytes"]
KERNELS = ["gatv2_backward_cols_kernel", "gatv2_backward_rows_kernel", "gatv2_forward_kernel", "gatv2_reduce_kernel"]


def run_child(body):
    if not os.path.exists(CPU_LIB):
        subprocess.check_call(["make", "-C", ROOT, "cpu"], stdout=subprocess.DEVNULL)
    env = dict(os.environ, HISPARSE_HIP_LIB=CPU_LIB)
    for k in [k for k in env if k.startswith("HISPARSE_") and k != "HISPARSE_HIP_LIB"]:
        env.pop(k)
    r = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests"), "body": body}], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "gatv2 child ok" in r.stdout, r.stdout[-4000:] + r.stderr[-4000:]
    return r.stdout


def _cases():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import gatv2_cases as gc
    return gc


SHAPES = _cases().SHAPES      # heads_cases.SHAPES, imported


@pytest.fixture(scope="module", autouse=True)
def the_reference_is_the_gradient():
    """before any library is tested: the reference's exact values against torch.autograd in float64 (once for this file)"""
    return _cases().reference_against_autograd()


def test_reference_against_autograd(the_reference_is_the_gradient):
    """the same check under a name of its own, so that a failure of the formulas reads as one"""
    w = the_reference_is_the_gradient
    assert set(w) == {"y", "lse", "gxd", "gxs", "ga"} and max(w.values()) <= 1.0


@pytest.mark.parametrize("heads,d", SHAPES)
def test_general(heads, d):
    """300 x 517, 4000 entries, slope 0.2, 0 and 1, both forms, tight and padded, lse taken and NULL, forward then backward with the lse
    just written, two backward calls with the same words"""
    print("\n".join(l for l in run_child(f"gc.general(mem, (({heads}, {d}),))").splitlines() if "backward worst" in l))


def test_ties():
    run_child("gc.ties(mem)")


def test_heads_do_not_leak():
    run_child("gc.heads_do_not_leak(mem)")


def test_edges():
    run_child("gc.edges(mem)")


def test_a_call_leaves_nothing_for_the_next():
    run_child("gc.nothing_carried_over(mem)")


def test_refusals():
    run_child("gc.refusals(mem)")


def test_info_is_unchanged_by_the_new_calls():
    run_child("""
indptr, indices = gc.random_pattern(gc.ROWS, gc.COLS, gc.NNZ, 1)
shape = (gc.ROWS, gc.COLS)
with gatv2.GraphAttentionV2((indptr, indices, shape), 5) as ga, heads.MultiHeadAttention((indptr, indices, shape), 5) as mh:
    before = ga.info()
    assert before == mh.info() and before["nnz"] == gc.NNZ
    XD, XS, a, gY = gc.operands(shape, 5, 4, 15000)
    y, lse = gc.forward_device(mem, ga, XD, XS, a, 5, 0.2)
    gc.backward_device(mem, ga, XD, XS, a, gY, lse, 5, 0.2)
    gc.backward_host(ga, XD, XS, a, gY, lse, 5, 0.2)
    assert ga.work_bytes(5, 4) == 5 * 4 * 8 and ga.info() == before
""")


def test_checker_rejects_planted_defects():
    """No library involved: a correct result (the references' own words, rounded once) passes with ratio <= 1, and each of three defects
    planted in it is rejected: the derivative of the negative branch taken as 1, ga summed with dz in the place of w (the gradient of the
    score with respect to z, not to a), head h's a used for head h + 1."""
    gc = _cases()
    indptr, indices = gc.random_pattern(gc.ROWS, gc.COLS, gc.NNZ, 9)
    shape, heads, d, slope = (gc.ROWS, gc.COLS), 3, 8, 0.2
    XD, XS, a, gY = gc.operands(shape, heads, d, 15100)
    fwd = gc.forward_refs(indptr, indices, XD, XS, a, heads, slope)
    assert gc.both_signs(fwd)
    y, lse = gc.rounded_forward(fwd)
    assert gc.check_forward(fwd, y, lse, "a correct forward result") <= 1.0
    bwd = gc.backward_refs(fwd, gY, lse)
    gxd, gxs, ga = gc.rounded_backward(bwd)
    assert max(gc.check_backward(bwd, gxd, gxs, ga, "a correct backward result").values()) <= 1.0
    # the derivative of the negative branch taken as 1
    wrong = []
    for r in bwd:
        keep, r.C = r.C, r.s.a.astype(np.float64)[None, :] * np.ones_like(r.s.dz)
        wrong.append(r.gradients(r.GT, r.P))
        r.C = keep
    w_gxd, w_gxs, _ = gc.rounded_backward(bwd, wrong)
    with pytest.raises(AssertionError, match="words of gxd break"):
        gc.check_backward(bwd, w_gxd, gxs, ga, "dz = 1 on the negative branch")
    with pytest.raises(AssertionError, match="words of gxs break"):
        gc.check_backward(bwd, gxd, w_gxs, ga, "dz = 1 on the negative branch")
    # ga summed with dz in the place of w
    wrong = []
    for r in bwd:
        keep, r.W = r.W, r.s.dz
        wrong.append(r.gradients(r.GT, r.P))
        r.W = keep
    with pytest.raises(AssertionError, match="words of ga break"):
        gc.check_backward(bwd, gxd, gxs, gc.rounded_backward(bwd, wrong)[2], "ga from dz")
    # head h's a used for head h + 1
    rolled = np.ascontiguousarray(np.roll(a, 1, axis=0))
    wrong_f = gc.forward_refs(indptr, indices, XD, XS, rolled, heads, slope)
    wrong_y, wrong_l = gc.rounded_forward(wrong_f)
    with pytest.raises(AssertionError, match="words of y break"):
        gc.check_forward(fwd, wrong_y, None, "another head's a")
    with pytest.raises(AssertionError, match="lse words break"):
        gc.check_forward(fwd, y, wrong_l, "another head's a")
    with pytest.raises(AssertionError, match="words of ga break"):
        gc.check_backward(bwd, gxd, gxs, gc.rounded_backward(gc.backward_refs(wrong_f, gY, lse))[2], "another head's a")


def test_header_libraries_and_binding_agree():
    """exactly the hsgat2_* functions of the issue in the header, in both libraries and in the binding's EXPORTS, apart from every other
    object's names; the header includes hisparse_heads.h and hisparse_hip.h names it in its comment only"""
    from hisparse_amd import attention, attention_backward, device, gat, gatv2, heads, heads16, heads_bias, heads_dropout, pattern, rows, wide
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hisparse_gatv2.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\bhsgat2_[a-z0-9_]+\b", header))) == NAMES
    assert sorted(set(re.findall(r"\b(hsgat2_[a-z0-9_]+)\s*\(", header))) == NAMES and '#include "hisparse_heads.h"' in header
    assert set(re.findall(r"\bhsmh[a-z0-9]*_[a-z0-9_]+\b", header)) == {"hsmh_pattern"}      # the existing object's type and nothing else of it
    assert sorted(gatv2.EXPORTS) == NAMES
    others = set(device.EXPORTS) | set(pattern.EXPORTS) | set(rows.EXPORTS) | set(wide.EXPORTS) | set(attention.EXPORTS) | set(attention_backward.EXPORTS) | set(heads.EXPORTS) \
        | set(heads16.EXPORTS) | set(heads_bias.EXPORTS) | set(heads_dropout.EXPORTS) | set(gat.EXPORTS)
    assert not set(NAMES) & others
    for lib in ("libhisparse_hip.so", "libhisparse_cpu.so"):
        exported = subprocess.run(["nm", "-D", "--defined-only", os.path.join(LIBDIR, lib)], capture_output=True, text=True, check=True).stdout
        assert sorted(set(re.findall(r"\b(hsgat2_[a-z0-9_]+)\b", exported))) == NAMES, lib
        l = ctypes.CDLL(os.path.join(LIBDIR, lib))
        for n in NAMES:
            assert hasattr(l, n), (lib, n)
    bound = gatv2.lib()
    for n in NAMES:
        assert getattr(bound, n).argtypes is not None, n
    assert bound is heads.lib() and issubclass(gatv2.GraphAttentionV2, heads.MultiHeadAttention)
    import hisparse_amd
    assert hisparse_amd.gatv2 is gatv2 and "gatv2" in hisparse_amd.__all__
    hip_h = open(os.path.join(ROOT, "include", "hisparse_hip.h")).read()
    assert "hisparse_gatv2.h" in hip_h and not re.search(r"\bhsgat2_[a-z_]+\s*\(", re.sub(r"/\*.*?\*/", "", hip_h, flags=re.S))


def test_schedule_is_the_wide_products_unchanged():
    """gatv2_attention.{h,hip} add no kWide* constant, the launchers take the classes, teams and grid cap from wide_products.h at the width
    heads * d, the file holds exactly the four kernels under names the other kernel counts do not match, without inline assembly, atomics
    or the matrix engine, and z and w are spelled as one fp32 add and one fp32 multiply"""
    text = open(os.path.join(ROOT, "hisparse_amd", "csrc", "gatv2_attention.h")).read()
    assert '#include "wide_products.h"' in text and not re.search(r"constexpr\s+\w+\s+kWide", text)
    hip = open(os.path.join(ROOT, "hisparse_amd", "csrc", "gatv2_attention.hip")).read()
    code = re.sub(r"//[^\n]*", "", hip)
    assert not re.search(r"constexpr\s+\w+\s+kWide", hip) and "asm" not in code and "atomic" not in code and "mfma" not in code
    for name in ("wide_table(s.count, heads * d)", "wide_group_lanes(heads * d)", "kWideBlocksPerCu", "kWideInFlight", "kWideThreads", "__fadd_rn(a.x, b.x)", "__fmul_rn(slope, z)",
                 '#include "wide_lanes.h"'):
        assert name in hip, name
    kernels = re.findall(r"__global__[^\n]*?\bvoid\s+(\w+)\s*\(", hip)
    assert sorted(kernels) == KERNELS
    for k in kernels:
        assert not any(old in k for old in ("gat_", "heads_forward", "heads_backward", "attention_backward_", "pattern_attention", "heads16_", "biased_attention_", "dropout_attention_"))


def test_cpu_twin_stand_alone_under_the_sanitizers(tmp_path):
    """tests/cpp/test_gatv2_cpu.cpp: the edge patterns and a few refusals through the C boundary over buffers of exactly the contract's
    reach, compiled together with hsmh_cpu.cpp under -fsanitize=address,undefined with the runtimes linked in statically (a program of
    its own: nothing loaded into python is run under a sanitizer)."""
    exe = tmp_path / "gatv2_cpu"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", f"-I{ROOT}/include", f"-I{ROOT}/hisparse_amd/csrc", f"{ROOT}/tests/cpp/test_gatv2_cpu.cpp", f"{ROOT}/hisparse_amd/csrc/hsmh_cpu.cpp",
                           "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "GATV2 CPU OK" in out.stdout, out.stdout + out.stderr


def test_the_launch_counts_the_header_states():
    """ONE launch forward and THREE backward, stated in the header and held in the source of both device entry points: the kernels are
    launched only by gatv2_attention.hip's four launchers, one kernel each, and hsgat2_forward_device calls one of them and
    hsgat2_backward_device three, the row side, the column side and the sum of ga in that order.  (The GPU test of the training step
    counts four launches on one stream with one synchronisation.)"""
    header = open(os.path.join(ROOT, "include", "hisparse_gatv2.h")).read()
    assert "The forward is ONE launch and the backward THREE" in header
    hip = open(os.path.join(ROOT, "hisparse_amd", "csrc", "gatv2_attention.hip")).read()
    assert len(re.findall(r"hipLaunchKernelGGL\(", hip)) == 4 and sorted(re.findall(r"hipLaunchKernelGGL\((\w+),", hip)) == KERNELS
    api = open(os.path.join(ROOT, "hisparse_amd", "csrc", "hsmh_api.cpp")).read()

    def body(name):
        start = api.index(f"int {name}(")
        return api[start: api.index("\n}\n", start)]
    assert re.findall(r"\blaunch_(\w+)\(", body("hsgat2_forward_device")) == ["gatv2_forward"]
    assert re.findall(r"\blaunch_(\w+)\(", body("hsgat2_backward_device")) == ["gatv2_backward_rows", "gatv2_backward_cols", "gatv2_reduce"]
    assert "hipMalloc" not in body("hsgat2_backward_device") and "alloc" not in body("hsgat2_backward_device")

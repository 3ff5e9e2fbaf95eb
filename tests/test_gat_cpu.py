"""The graph attention (GAT) calls (include/hisparse_gat.h) without a GPU: the cases of tests/gat_cases.py on libhisparse_cpu.so, each in a
child process with HISPARSE_HIP_LIB set (as tests/test_heads_cpu.py runs its cases); the checker against three planted defects; the CPU
twin against torch's float64 autograd of the dense masked GAT layer; header, libraries and binding in agreement on exactly four
functions; the kernels' source on the unchanged schedule; the CPU twin's source under the sanitizers as a stand-alone program.  The same
cases on the device: tests/test_gpu_gat.py."""
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
from hisparse_amd import device, heads, gat
import gat_cases as gc
assert device._LIB_PATH.endswith("libhisparse_cpu.so")
mem = gc.HostMemory()
%(body)s
print("gat child ok")
"""

NAMES = ["hsgat_backward", "hsgat_backward_device", "hsgat_forward", "hsgat_forward_device"]


def run_child(body):
    if not os.path.exists(CPU_LIB):
        subprocess.check_call(["make", "-C", ROOT, "cpu"], stdout=subprocess.DEVNULL)
    env = dict(os.environ, HISPARSE_HIP_LIB=CPU_LIB)
    for k in [k for k in env if k.startswith("HISPARSE_") and k != "HISPARSE_HIP_LIB"]:
        env.pop(k)
    r = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests"), "body": body}], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "gat child ok" in r.stdout, r.stdout[-4000:] + r.stderr[-4000:]
    return r.stdout


def _cases():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import gat_cases as gc
    return gc


SHAPES = _cases().SHAPES      # heads_cases.SHAPES, imported


@pytest.mark.parametrize("heads,d", SHAPES)
def test_general(heads, d):
    """300 x 517, 4000 entries, slope 0.2, 0 and 1, both forms, tight and padded, lse taken and NULL, both signs of x in every row"""
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


def test_checker_rejects_planted_defects():
    """No library involved: a correct result (the references' own words, rounded once) passes with ratio <= 1, and each of three defects
    planted in it is rejected: the derivative of the negative branch taken as 1, head h's er word used for head h + 1, ger summed with dx
    of the positive branch only."""
    gc = _cases()
    indptr, indices = gc.random_pattern(gc.ROWS, gc.COLS, gc.NNZ, 9)
    shape, heads, d, slope = (gc.ROWS, gc.COLS), 3, 8, 0.2
    EL, ER, V, gY = gc.operands(shape, indptr, indices, heads, d, 12000)
    assert gc.both_signs_in_every_row(indptr, indices, EL, ER)
    fwd = gc.forward_refs(indptr, indices, EL, ER, V, slope)
    y, lse = gc.rounded_forward(fwd)
    assert gc.check_forward(fwd, y, lse, "a correct forward result") <= 1.0
    bwd = gc.backward_refs(fwd, gY, lse)
    gel, ger, gv = gc.rounded_backward(bwd)
    assert max(gc.check_backward(bwd, gel, ger, gv, "a correct backward result").values()) <= 1.0
    # the derivative of the negative branch taken as 1: GX = P (GP - D)
    wrong = [r.gradients(r.P * (r.GP - r.D[r.f.of]), r.P) for r in bwd]
    w_gel, w_ger, _ = gc.rounded_backward(bwd, wrong)
    with pytest.raises(AssertionError, match="words of gel break"):
        gc.check_backward(bwd, w_gel, ger, gv, "dx = 1 on the negative branch")
    with pytest.raises(AssertionError, match="words of ger break"):
        gc.check_backward(bwd, gel, w_ger, gv, "dx = 1 on the negative branch")
    # head h's er word used for head h + 1
    rolled = np.ascontiguousarray(np.roll(ER, 1, axis=1))
    wrong_f = gc.forward_refs(indptr, indices, EL, rolled, V, slope)
    wrong_y, wrong_l = gc.rounded_forward(wrong_f)
    with pytest.raises(AssertionError, match="words of y break"):
        gc.check_forward(fwd, wrong_y, None, "another head's er word")
    with pytest.raises(AssertionError, match="lse words break"):
        gc.check_forward(fwd, y, wrong_l, "another head's er word")
    with pytest.raises(AssertionError, match="words of gv break"):
        gc.check_backward(bwd, gel, ger, gc.rounded_backward(gc.backward_refs(wrong_f, gY, lse))[2], "another head's er word")
    # ger summed with dx of the positive branch only: the entries of the negative branch left out
    wrong = [r.gradients(np.where(r.f.x > 0, r.GX, 0.0), r.P) for r in bwd]
    with pytest.raises(AssertionError, match="words of ger break"):
        gc.check_backward(bwd, gel, gc.rounded_backward(bwd, wrong)[1], gv, "ger over the positive branch only")


def test_cpu_twin_against_autograd():
    """40 x 50, 600 distinct pairs, 3 heads of d = 8: hsgat_backward on the CPU twin, with lse from hsgat_forward on the CPU twin, against
    torch float64 autograd of the dense masked layer Y_h = softmax(leaky_relu(el_h[:, None] + er_h[None, :], 0.25) + mask) V_h and the
    loss sum(gY * Y).  This guards the formulas and the layouts themselves, which the references share with the code.

    el, er, V and gY are multiples of 1/8 and slope is 0.25, so x and t are exact and the contract's function is autograd's, ties included
    (torch's derivative at x == 0 is the slope).  What is left between the two is lse: P'_e = f_r P_e with f_r = exp(LSE_r - lse_r) and
    k_r = expm1(bound_lse_r), so, as tests/test_heads_cpu.py derives it,
        |GX'_e - GX_e| <= P'_e (k_r |GP_e| + k_r (2 + k_r) |D'_r|) dx_e,   |P'_e - P_e| <= k_r P'_e
    summed over a word's entries (times |gY_ej| for gV) and added to the contract's bound."""
    import tempfile

    import torch
    body = """
import wide_cases as wc
rng = np.random.default_rng(12100)
rows, cols, H, d, slope = 40, 50, 3, 8, 0.25
flat = np.sort(rng.choice(rows * cols, 600, replace=False))
indptr = np.zeros(rows + 1, dtype=np.uint32); indptr[1:] = np.cumsum(np.bincount(flat // cols, minlength=rows))
indices = (flat % cols).astype(np.uint32)
EL, ER = wc.grid_values(rng, (rows, H)), wc.grid_values(rng, (cols, H))
V, gY = wc.grid_values(rng, (cols, H * d)), wc.grid_values(rng, (rows, H * d))
with gat.GraphAttention((indptr, indices, (rows, cols)), H) as ga:
    y, lse = ga.forward(EL, ER, V, H, slope)
    gel, ger, gv = ga.backward(EL, ER, V, gY, lse, H, slope)
np.savez(PATH, indptr=indptr, indices=indices, EL=EL, ER=ER, V=V, gY=gY, y=y, lse=lse, gel=gel, ger=ger, gv=gv)
"""
    gc = _cases()
    ac = gc.ac
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "twin.npz")
        run_child(body.replace("PATH", repr(path)))
        z = dict(np.load(path))
    indptr, indices, EL, ER, V, gY, lse = (z[k] for k in ("indptr", "indices", "EL", "ER", "V", "gY", "lse"))
    rows, cols, H, d, slope = 40, 50, 3, 8, 0.25
    assert (np.diff(indptr.astype(np.int64)) > 0).all() and lse.shape == (rows, H)
    fwd = gc.forward_refs(indptr, indices, EL, ER, V, slope)
    bwd = gc.backward_refs(fwd, gY, lse)
    of, ix = fwd[0].of, fwd[0].indices
    assert (fwd[0].x == 0).any()
    tl, tr = (torch.tensor(a.astype(np.float64), requires_grad=True) for a in (EL, ER))
    tv = torch.tensor(V.astype(np.float64).reshape(cols, H, d), requires_grad=True)
    mask = torch.full((rows, cols), -np.inf, dtype=torch.float64)
    mask[torch.tensor(of), torch.tensor(ix)] = 0.0
    t = torch.nn.functional.leaky_relu(tl.T[:, :, None] + tr.T[:, None, :], 0.25) + mask      # (H, rows, cols)
    ty = torch.einsum("hrc,chj->rhj", torch.softmax(t, dim=2), tv)
    (ty * torch.tensor(gY.astype(np.float64).reshape(rows, H, d))).sum().backward()
    auto_y = ty.detach().numpy().reshape(rows, H * d)
    auto = {"gel": tl.grad.numpy(), "ger": tr.grad.numpy(), "gv": tv.grad.numpy().reshape(cols, H * d)}
    for h in range(H):
        f, r = fwd[h], bwd[h]
        assert (np.abs(lse[:, h].astype(np.float64) - f.LSE) <= f.bound_lse).all()
        assert (np.abs(f.Y - gc.cut(auto_y, h, d)) <= 2.0 ** -40 * (1.0 + np.abs(f.Y))).all(), f"the forward formula, head {h}"
        k = np.expm1(f.bound_lse)[of]
        d_gx = r.P * (k * np.abs(r.GP) + k * (2.0 + k) * np.abs(r.D[of])) * r.dx
        d_p = k * r.P
        pm = r.perm
        extra = {"gel": ac._seg_sum(d_gx[:, None], f.indptr), "ger": ac._seg_sum(d_gx[pm][:, None], r.cptr), "gv": ac._seg_sum((d_p[:, None] * np.abs(r.G64))[pm], r.cptr)}
        mine = {"gel": r.GEL, "ger": r.GER, "gv": r.GV}
        r.want = {"gel": auto["gel"][:, h: h + 1], "ger": auto["ger"][:, h: h + 1], "gv": gc.cut(auto["gv"], h, d)}
        worst = r.check(gc.col(z["gel"], h), gc.col(z["ger"], h), gc.cut(z["gv"], h, d), f"the CPU twin against autograd, head {h}", extra=extra)
        assert max(worst.values()) <= 1.0
        for name in gc.OUTPUTS:      # the formula alone: the reference's own float64 gradients against autograd's
            assert (np.abs(mine[name] - r.want[name]) <= extra[name] + 2.0 ** -40 * (1.0 + np.abs(mine[name]))).all(), (name, h)
    gc.check_forward(fwd, z["y"], lse, "the CPU twin's forward")


def test_header_libraries_and_binding_agree():
    """exactly four hsgat_* functions in the header, in both libraries and in the binding's EXPORTS, apart from every other object's names;
    the header includes hisparse_heads.h and hisparse_hip.h names it in its comment only"""
    from hisparse_amd import attention, attention_backward, device, gat, heads, heads16, heads_bias, heads_dropout, pattern, rows, wide
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hisparse_gat.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\bhsgat_[a-z0-9_]+\b", header))) == NAMES
    assert sorted(set(re.findall(r"\b(hsgat_[a-z0-9_]+)\s*\(", header))) == NAMES and len(NAMES) == 4 and '#include "hisparse_heads.h"' in header
    assert set(re.findall(r"\bhsmh[a-z0-9]*_[a-z0-9_]+\b", header)) == {"hsmh_pattern"}      # the existing object's type and nothing else of it
    assert sorted(gat.EXPORTS) == NAMES
    others = set(device.EXPORTS) | set(pattern.EXPORTS) | set(rows.EXPORTS) | set(wide.EXPORTS) | set(attention.EXPORTS) | set(attention_backward.EXPORTS) | set(heads.EXPORTS) \
        | set(heads16.EXPORTS) | set(heads_bias.EXPORTS) | set(heads_dropout.EXPORTS)
    assert not set(NAMES) & others and not any(n.startswith("hsmh_") for n in NAMES)
    for lib in ("libhisparse_hip.so", "libhisparse_cpu.so"):
        exported = subprocess.run(["nm", "-D", "--defined-only", os.path.join(LIBDIR, lib)], capture_output=True, text=True, check=True).stdout
        assert sorted(set(re.findall(r"\b(hsgat_[a-z0-9_]+)\b", exported))) == NAMES, lib
        l = ctypes.CDLL(os.path.join(LIBDIR, lib))
        for n in NAMES:
            assert hasattr(l, n), (lib, n)
    bound = gat.lib()
    for n in NAMES:
        assert getattr(bound, n).argtypes is not None, n
    assert bound is heads.lib() and issubclass(gat.GraphAttention, heads.MultiHeadAttention)
    import hisparse_amd
    assert hisparse_amd.gat is gat and "gat" in hisparse_amd.__all__
    hip_h = open(os.path.join(ROOT, "include", "hisparse_hip.h")).read()
    assert "hisparse_gat.h" in hip_h and not re.search(r"\bhsgat_[a-z_]+\s*\(", re.sub(r"/\*.*?\*/", "", hip_h, flags=re.S))


def test_schedule_is_the_wide_products_unchanged():
    """gat_attention.{h,hip} add no kWide* constant, the launchers take the classes, teams and grid cap from wide_products.h at the width
    heads * d, the file holds exactly the three kernels under names the other kernel counts do not match, without inline assembly,
    atomics or the matrix engine, and x and t are spelled as one fp32 add and one fp32 multiply"""
    text = open(os.path.join(ROOT, "hisparse_amd", "csrc", "gat_attention.h")).read()
    assert '#include "wide_products.h"' in text and not re.search(r"constexpr\s+\w+\s+kWide", text)
    hip = open(os.path.join(ROOT, "hisparse_amd", "csrc", "gat_attention.hip")).read()
    code = re.sub(r"//[^\n]*", "", hip)
    assert not re.search(r"constexpr\s+\w+\s+kWide", hip) and "asm" not in code and "atomic" not in code and "mfma" not in code
    for name in ("wide_table(s.count, heads * d)", "wide_group_lanes(heads * d)", "kWideBlocksPerCu", "kWideInFlight", "kWideThreads", "__fadd_rn(a, b)", "__fmul_rn(slope, x)"):
        assert name in hip, name
    kernels = re.findall(r"__global__[^\n]*?\bvoid\s+(\w+)\s*\(", hip)
    assert sorted(kernels) == ["gat_backward_cols_kernel", "gat_backward_rows_kernel", "gat_forward_kernel"]
    for k in kernels:
        assert not any(old in k for old in ("heads_forward", "heads_backward", "attention_backward_", "pattern_attention", "heads16_", "biased_attention_", "dropout_attention_"))


def test_cpu_twin_stand_alone_under_the_sanitizers(tmp_path):
    """tests/cpp/test_gat_cpu.cpp: the edge patterns and the refusals through the C boundary, compiled together with hsmh_cpu.cpp under
    -fsanitize=address,undefined with the runtimes linked in statically (a program of its own: nothing loaded into python is run under
    a sanitizer)."""
    exe = tmp_path / "gat_cpu"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", f"-I{ROOT}/include", f"-I{ROOT}/hisparse_amd/csrc", f"{ROOT}/tests/cpp/test_gat_cpu.cpp", f"{ROOT}/hisparse_amd/csrc/hsmh_cpu.cpp",
                           "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "GAT CPU OK" in out.stdout, out.stdout + out.stderr

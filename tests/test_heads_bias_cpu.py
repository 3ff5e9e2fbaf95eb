"""The multi-head attention calls with a per-entry, per-head bias (include/hisparse_heads_bias.h) without a GPU: the cases of
tests/heads_bias_cases.py on libhisparse_cpu.so, each in a child process with HISPARSE_HIP_LIB set (as tests/test_heads_cpu.py runs its
cases); the restated references anchored to the existing ones at a zero bias; the checker against four planted defects; the CPU twin
against torch's float64 autograd of the dense masked multi-head attention with a bias, the bias's gradient included; header, libraries
and binding in agreement on exactly five functions; the CPU twin's source under the sanitizers as a stand-alone program.  The same cases
on the device: tests/test_gpu_heads_bias.py."""
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
from hisparse_amd import device, heads, heads_bias
import heads_bias_cases as hb
assert device._LIB_PATH.endswith("libhisparse_cpu.so")
mem = hb.HostMemory()
%(body)s
print("heads bias child ok")
"""

NAMES = ["hsmhb_backward", "hsmhb_backward_device", "hsmhb_create", "hsmhb_forward", "hsmhb_forward_device"]


def run_child(body):
    if not os.path.exists(CPU_LIB):
        subprocess.check_call(["make", "-C", ROOT, "cpu"], stdout=subprocess.DEVNULL)
    env = dict(os.environ, HISPARSE_HIP_LIB=CPU_LIB)
    for k in [k for k in env if k.startswith("HISPARSE_") and k != "HISPARSE_HIP_LIB"]:
        env.pop(k)
    r = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests"), "body": body}], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "heads bias child ok" in r.stdout, r.stdout[-4000:] + r.stderr[-4000:]
    return r.stdout


def _cases():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import heads_bias_cases as hb
    return hb


SHAPES = _cases().SHAPES      # heads_cases.SHAPES, imported


@pytest.mark.parametrize("heads,d", SHAPES)
def test_general(heads, d):
    """300 x 517, 4000 entries, scale 0.125, 1 and -2, a bias in [-4, 4], both forms, tight and padded, lse and gbias taken and NULL"""
    print("\n".join(l for l in run_child(f"hb.general(mem, (({heads}, {d}),))").splitlines() if "backward worst" in l))


def test_edges():
    run_child("hb.edges(mem)")


def test_zero_bias_gives_the_words_of_the_plain_calls():
    run_child("hb.zero_bias(mem)")


def test_mask():
    run_child("hb.mask(mem)")


def test_heads_do_not_leak():
    run_child("hb.heads_do_not_leak(mem)")


def test_long_rows_and_columns():
    """the host has no grid: 2000 rows and columns hold the long row and the long column"""
    run_child("hb.long_rows_and_columns(mem, 2000)")


def test_objects():
    run_child("hb.objects(mem)")


def test_refusals():
    run_child("hb.refusals(mem)")


@pytest.mark.parametrize("heads,d", SHAPES)
def test_zero_bias_anchors_the_references(heads, d):
    """No library involved.  With an all-zero bias the restated references' Y, LSE, GQ, GK and GV equal the existing references' exactly
    in float64, on every general case, and every bound lies between 1 and 2.01 times the existing one: eta' = (1 + u) eta + u |T| <=
    (2 + u) eta because eta >= u |T|, and every bound grows at most linearly in eta, apart from terms that do not change."""
    hb = _cases()
    hc = hb.hc
    indptr, indices = hb.random_pattern(hb.ROWS, hb.COLS, hb.NNZ, 1)
    shape = (hb.ROWS, hb.COLS)
    Q, K, V, gY = hb.operands(shape, heads * d, 6100 + 1000 * heads + d)
    zero = np.zeros((hb.NNZ, heads), dtype=np.float32)
    scores = hb.head_scores(indptr, indices, Q, K, heads)
    for scale in (0.125, 1.0, -2.0):
        old_f, new_f = hc.forward_refs(scores, V, scale), hb.forward_refs(scores, V, scale, zero)
        lse = hb.rounded_forward(old_f)[1]
        old_b, new_b = hc.backward_refs(scores, V, gY, lse, scale), hb.backward_refs(scores, V, gY, lse, scale, zero)
        for o, n in zip(old_f, new_f):
            assert np.array_equal(o.Y, n.Y) and np.array_equal(o.LSE, n.LSE) and np.array_equal(o.finite, n.finite)
            for a, b in ((o.bound_y[o.finite], n.bound_y[o.finite]), (o.bound_lse[o.finite], n.bound_lse[o.finite])):
                assert (b >= a).all() and (b <= 2.01 * a).all(), (heads, d, scale, float((b / a).max()))
        for o, n in zip(old_b, new_b):
            assert np.array_equal(o.GQ, n.GQ) and np.array_equal(o.GK, n.GK) and np.array_equal(o.GV, n.GV)
            for name in hb.bc.OUTPUTS:
                assert (n.bound[name] >= o.bound[name]).all() and (n.bound[name] <= 2.01 * o.bound[name]).all(), (heads, d, scale, name)


def test_checker_rejects_planted_defects():
    """No library involved: a correct result (the references' own words, rounded once) passes, and each of four defects planted in it
    is rejected every time: the bias added before the scale, the bias of head h used for head h + 1, gbias written in transposed
    order, gbias multiplied by scale."""
    hb = _cases()
    indptr, indices = hb.random_pattern(hb.ROWS, hb.COLS, hb.NNZ, 9)
    shape, heads, d, scale = (hb.ROWS, hb.COLS), 3, 8, 0.5
    Q, K, V, gY = hb.operands(shape, heads * d, 11000)
    bias = hb.biases(hb.NNZ, heads, 11010)
    scores = hb.head_scores(indptr, indices, Q, K, heads)
    fwd = hb.forward_refs(scores, V, scale, bias)
    y, lse = hb.rounded_forward(fwd)
    assert hb.check_forward(fwd, y, lse, "a correct forward result") <= 1.0
    bwd = hb.backward_refs(scores, V, gY, lse, scale, bias)
    gq, gk, gv = hb.rounded_backward(bwd)
    gb = hb.rounded_gbias(bwd)
    assert max(hb.check_backward(bwd, gq, gk, gv, "a correct backward result").values()) <= 1.0 and hb.check_gbias(bwd, gb, "a correct gbias") <= 1.0
    # the bias added before the scale: t = scale (s + b) = scale s + scale b
    wrong_y, wrong_l = hb.rounded_forward(hb.forward_refs(scores, V, scale, (np.float32(scale) * bias).astype(np.float32)))
    with pytest.raises(AssertionError, match="words of y break"):
        hb.check_forward(fwd, wrong_y, None, "the bias added before the scale")
    with pytest.raises(AssertionError, match="lse words break"):
        hb.check_forward(fwd, y, wrong_l, "the bias added before the scale")
    lse_b = hb.rounded_forward(hb.forward_refs(scores, V, scale, (np.float32(scale) * bias).astype(np.float32)))[1]
    wq = hb.rounded_backward(hb.backward_refs(scores, V, gY, lse_b, scale, (np.float32(scale) * bias).astype(np.float32)))[0]
    with pytest.raises(AssertionError, match="words of gq break"):
        hb.check_backward(bwd, wq, gk, gv, "the bias added before the scale")
    # the bias of head h used for head h + 1
    rolled = np.ascontiguousarray(np.roll(bias, 1, axis=1))
    wrong_y = hb.rounded_forward(hb.forward_refs(scores, V, scale, rolled))[0]
    with pytest.raises(AssertionError, match="words of y break"):
        hb.check_forward(fwd, wrong_y, None, "another head's bias")
    wrong = hb.backward_refs(scores, V, gY, lse, scale, rolled)
    with pytest.raises(AssertionError, match="words of gk break"):
        hb.check_backward(bwd, gq, hb.rounded_backward(wrong)[1], gv, "another head's bias")
    with pytest.raises(AssertionError, match="words of gbias break"):
        hb.check_gbias(bwd, hb.rounded_gbias(wrong), "another head's bias")
    # gbias written in transposed order: the same words, [head][entry] read back as [entry][head]
    transposed = np.ascontiguousarray(gb.T).reshape(gb.shape)
    with pytest.raises(AssertionError, match="words of gbias break"):
        hb.check_gbias(bwd, transposed, "gbias stored [head][entry]")
    # gbias multiplied by scale (GS stored where GB belongs)
    with pytest.raises(AssertionError, match="words of gbias break"):
        hb.check_gbias(bwd, (np.float32(scale) * gb).astype(np.float32), "gbias times scale")


def test_cpu_twin_against_autograd():
    """40 x 50, about 600 entries (no pair twice: a dense mask holds a pair once), 3 heads of d = 8: hsmhb_backward on the CPU twin, with
    lse from hsmhb_forward on the CPU twin, against torch float64 autograd of Y_h = softmax(scale Q_h K_h^T + B_h + mask) V_h and the
    loss sum(gY * Y), g_bias included.  This guards the formulas and the layouts themselves, which the references share with the code.

    It is tests/test_heads_cpu.py's comparison with its tolerance.  The operands and the bias are multiples of 1/8 below 4 and scale is
    1/8, so every fp32 product and t itself are exact; what is left between the contract's function and autograd's is lse,
    P'_e = f_r P_e with f_r = exp(LSE_r - lse_r) and k_r = expm1(bound_lse_r), so
        |GB'_e - GB_e| <= P'_e (k_r |GP_e| + k_r (2 + k_r) |D'_r|),   |GS'_e - GS_e| <= |scale| times that,   |P'_e - P_e| <= k_r P'_e
    summed over a word's entries times |K_ej|, |Q_ej| or |gY_ej| and added to the contract's bound."""
    import tempfile

    import torch
    body = """
import wide_cases as wc
rng = np.random.default_rng(11100)
rows, cols, H, d, scale = 40, 50, 3, 8, 0.125
flat = np.sort(rng.choice(rows * cols, 600, replace=False))
indptr = np.zeros(rows + 1, dtype=np.uint32); indptr[1:] = np.cumsum(np.bincount(flat // cols, minlength=rows))
indices = (flat % cols).astype(np.uint32)
Q, gY = (wc.grid_values(rng, (rows, H * d)) for _ in range(2)); K, V = (wc.grid_values(rng, (cols, H * d)) for _ in range(2))
bias = wc.grid_values(rng, (600, H))
with heads_bias.BiasedMultiHeadAttention((indptr, indices, (rows, cols)), H) as mh:
    y, lse = mh.forward(Q, K, V, bias, H, scale)
    gq, gk, gv, gb = mh.backward(Q, K, V, gY, lse, bias, H, scale)
np.savez(PATH, indptr=indptr, indices=indices, Q=Q, K=K, V=V, gY=gY, bias=bias, y=y, lse=lse, gq=gq, gk=gk, gv=gv, gb=gb)
"""
    hb = _cases()
    ac = hb.ac
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "twin.npz")
        run_child(body.replace("PATH", repr(path)))
        z = dict(np.load(path))
    indptr, indices, Q, K, V, gY, bias, lse = (z[k] for k in ("indptr", "indices", "Q", "K", "V", "gY", "bias", "lse"))
    rows, cols, H, d, scale = 40, 50, 3, 8, 0.125
    assert (np.diff(indptr.astype(np.int64)) > 0).all() and lse.shape == (rows, H) and z["gb"].shape == (600, H)
    scores = hb.head_scores(indptr, indices, Q, K, H)
    fwd = hb.forward_refs(scores, V, scale, bias)
    bwd = hb.backward_refs(scores, V, gY, lse, scale, bias)
    of, ix = scores[0].of, scores[0].indices
    tq, tk, tv = (torch.tensor(a.astype(np.float64).reshape(-1, H, d), requires_grad=True) for a in (Q, K, V))
    dense = torch.full((H, rows, cols), -np.inf, dtype=torch.float64)
    dense[:, torch.tensor(of), torch.tensor(ix)] = torch.tensor(bias.astype(np.float64).T)
    dense.requires_grad_(True)
    p = torch.softmax(scale * torch.einsum("rhj,chj->hrc", tq, tk) + dense, dim=2)
    ty = torch.einsum("hrc,chj->rhj", p, tv)
    (ty * torch.tensor(gY.astype(np.float64).reshape(rows, H, d))).sum().backward()
    auto_y = ty.detach().numpy().reshape(rows, H * d)
    auto = [g.grad.numpy().reshape(-1, H * d) for g in (tq, tk, tv)]
    auto_gb = dense.grad.numpy()[:, of, ix].T      # (entries, H)
    for h in range(H):
        s, f, r = scores[h], fwd[h], bwd[h]
        assert (np.abs(lse[:, h].astype(np.float64) - f.LSE) <= f.bound_lse).all()
        assert (np.abs(f.Y - hb.cut(auto_y, h, d)) <= 2.0 ** -40 * (1.0 + np.abs(f.Y))).all(), f"the forward formula, head {h}"
        k = np.expm1(f.bound_lse)[of]
        d_gb = r.P * (k * np.abs(r.GP) + k * (2.0 + k) * np.abs(r.D[of]))
        d_gs = abs(r.sc) * d_gb
        d_p = k * r.P
        pm = r.perm
        extra = {"gq": ac._seg_sum(d_gs[:, None] * np.abs(r.K64), s.indptr), "gk": ac._seg_sum((d_gs[:, None] * np.abs(r.Q64))[pm], r.cptr),
                 "gv": ac._seg_sum((d_p[:, None] * np.abs(r.G64))[pm], r.cptr)}
        mine = {"gq": r.GQ, "gk": r.GK, "gv": r.GV}
        r.want = {name: hb.cut(a, h, d) for name, a in zip(hb.bc.OUTPUTS, auto)}
        worst = r.check(*(hb.cut(z[name], h, d) for name in hb.bc.OUTPUTS), f"the CPU twin against autograd, head {h}", extra=extra)
        assert max(worst.values()) <= 1.0
        for name in hb.bc.OUTPUTS:      # the formula alone: the reference's own float64 gradients against autograd's
            assert (np.abs(mine[name] - r.want[name]) <= extra[name] + 2.0 ** -40 * (1.0 + np.abs(mine[name]))).all(), (name, h)
        assert r.check_gbias(np.ascontiguousarray(z["gb"][:, h]), f"the CPU twin's gbias against autograd, head {h}", extra=d_gb, want=auto_gb[:, h]) <= 1.0
        assert (np.abs(r.GB - auto_gb[:, h]) <= d_gb + 2.0 ** -40 * (1.0 + np.abs(r.GB))).all(), f"the formula of gbias, head {h}"
    hb.check_forward(fwd, z["y"], lse, "the CPU twin's forward")


def test_header_libraries_and_binding_agree():
    """exactly five hsmhb_* functions in the header, in both libraries and in the binding's EXPORTS, apart from every other module's
    names; the header includes hisparse_heads.h and hisparse_hip.h names it in its comment only"""
    from hisparse_amd import attention, attention_backward, device, heads, heads16, heads_bias, pattern, rows, wide
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hisparse_heads_bias.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\bhsmhb_[a-z0-9_]+\b", header))) == NAMES
    assert sorted(set(re.findall(r"\b(hsmhb_[a-z0-9_]+)\s*\(", header))) == NAMES and len(NAMES) == 5 and '#include "hisparse_heads.h"' in header
    assert set(re.findall(r"\bhsmh_[a-z0-9_]+\b", header)) == {"hsmh_pattern"}      # the existing object's type and nothing else of it
    assert sorted(heads_bias.EXPORTS) == NAMES
    others = set(device.EXPORTS) | set(pattern.EXPORTS) | set(rows.EXPORTS) | set(wide.EXPORTS) | set(attention.EXPORTS) | set(attention_backward.EXPORTS) | set(heads.EXPORTS) \
        | set(heads16.EXPORTS)
    assert not set(NAMES) & others
    for lib in ("libhisparse_hip.so", "libhisparse_cpu.so"):
        exported = subprocess.run(["nm", "-D", "--defined-only", os.path.join(LIBDIR, lib)], capture_output=True, text=True, check=True).stdout
        assert sorted(set(re.findall(r"\b(hsmhb_[a-z0-9_]+)\b", exported))) == NAMES, lib
        l = ctypes.CDLL(os.path.join(LIBDIR, lib))
        for n in NAMES:
            assert hasattr(l, n), (lib, n)
    bound = heads_bias.lib()
    for n in NAMES:
        assert getattr(bound, n).argtypes is not None, n
    assert bound is heads.lib() and issubclass(heads_bias.BiasedMultiHeadAttention, heads.MultiHeadAttention)
    import hisparse_amd
    assert hisparse_amd.heads_bias is heads_bias and "heads_bias" in hisparse_amd.__all__
    hip_h = open(os.path.join(ROOT, "include", "hisparse_hip.h")).read()
    assert "hisparse_heads_bias.h" in hip_h and not re.search(r"\bhsmhb_[a-z_]+\s*\(", re.sub(r"/\*.*?\*/", "", hip_h, flags=re.S))


def test_schedule_is_the_wide_products_unchanged():
    """heads_bias_attention.{h,hip} add no kWide* constant, the launchers take the classes, teams and grid cap from wide_products.h at the
    width heads * d, the file holds exactly the three kernels under names the other kernel counts do not match, without inline assembly
    or atomics; heads_attention.hip and heads16_attention.hip hold what they held"""
    text = open(os.path.join(ROOT, "hisparse_amd", "csrc", "heads_bias_attention.h")).read()
    assert '#include "wide_products.h"' in text and not re.search(r"constexpr\s+\w+\s+kWide", text)
    hip = open(os.path.join(ROOT, "hisparse_amd", "csrc", "heads_bias_attention.hip")).read()
    code = re.sub(r"//[^\n]*", "", hip)
    assert not re.search(r"constexpr\s+\w+\s+kWide", hip) and "asm" not in code and "atomic" not in code
    for name in ("wide_table(s.count, heads * d)", "wide_group_lanes(heads * d)", "kWideBlocksPerCu", "kWideInFlight", "kWideThreads", "__builtin_nontemporal_load(bias_head",
                 "__builtin_nontemporal_load(perm + ei)", "__fadd_rn(__fmul_rn("):
        assert name in hip, name
    kernels = re.findall(r"__global__[^\n]*?\bvoid\s+(\w+)\s*\(", hip)
    assert sorted(kernels) == ["biased_attention_cols_kernel", "biased_attention_forward_kernel", "biased_attention_rows_kernel"]
    for k in kernels:
        assert not any(old in k for old in ("heads_forward", "heads_backward", "heads16_"))


def test_cpu_twin_stand_alone_under_the_sanitizers(tmp_path):
    """tests/cpp/test_heads_bias_cpu.cpp: the edge patterns and the refusals through the C boundary, compiled together with hsmh_cpu.cpp
    under -fsanitize=address,undefined with the runtimes linked in statically (a program of its own: nothing loaded into python is run
    under a sanitizer)."""
    exe = tmp_path / "heads_bias_cpu"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", f"-I{ROOT}/include", f"-I{ROOT}/hisparse_amd/csrc", f"{ROOT}/tests/cpp/test_heads_bias_cpu.cpp",
                           f"{ROOT}/hisparse_amd/csrc/hsmh_cpu.cpp", "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "HEADS BIAS CPU OK" in out.stdout, out.stdout + out.stderr

"""The multi-head attention object (include/hisparse_heads.h) without a GPU: the cases of tests/heads_cases.py on libhisparse_cpu.so, each
in a child process with HISPARSE_HIP_LIB set (as tests/test_attention_cpu.py runs its cases); the checker against three planted defects;
the CPU twin against torch's float64 autograd of the dense masked multi-head attention; header, libraries and binding in agreement on
exactly ten functions; the CPU twin's source under the sanitizers as a stand-alone program.  The same cases on the device:
tests/test_gpu_heads.py."""
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
from hisparse_amd import device, heads
import heads_cases as hc
assert device._LIB_PATH.endswith("libhisparse_cpu.so")
mem = hc.HostMemory()
%(body)s
print("heads child ok")
"""

NAMES = ["hsmh_backward", "hsmh_backward_device", "hsmh_create", "hsmh_destroy", "hsmh_forward", "hsmh_forward_device", "hsmh_info", "hsmh_last_error", "hsmh_set_stream",
         "hsmh_sync"]
SHAPES = ((1, 4), (2, 4), (5, 4), (3, 8), (4, 16), (3, 16), (2, 32), (4, 64), (2, 128), (1, 256), (8, 32), (64, 4))


def run_child(body):
    if not os.path.exists(CPU_LIB):
        subprocess.check_call(["make", "-C", ROOT, "cpu"], stdout=subprocess.DEVNULL)
    env = dict(os.environ, HISPARSE_HIP_LIB=CPU_LIB)
    for k in [k for k in env if k.startswith("HISPARSE_") and k != "HISPARSE_HIP_LIB"]:
        env.pop(k)
    r = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests"), "body": body}], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "heads child ok" in r.stdout, r.stdout[-4000:] + r.stderr[-4000:]
    return r.stdout


def _cases():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import heads_cases as hc
    return hc


def test_the_shapes_are_the_shared_ones():
    assert SHAPES == _cases().SHAPES


@pytest.mark.parametrize("heads,d", SHAPES)
def test_general(heads, d):
    """300 x 517, 4000 entries, scale 0.125, 1 and -2, pad 0 and 8, ldl = heads and heads + 3, lse taken and NULL, both forms, forward then
    backward with the lse just written"""
    print("\n".join(l for l in run_child(f"hc.general(mem, (({heads}, {d}),))").splitlines() if "backward worst" in l))


def test_heads_do_not_leak():
    run_child("hc.heads_do_not_leak(mem)")


def test_edges():
    run_child("hc.edges(mem)")


def test_agreement_with_the_single_head_objects():
    run_child("hc.agreement(mem)")


def test_a_call_leaves_nothing_for_the_next():
    run_child("hc.nothing_carried_over(mem)")


def test_refusals():
    run_child("hc.refusals(mem)")


def test_info_holds_nothing_on_a_device():
    run_child("for backward in (True, False):\n"
              "    with heads.MultiHeadAttention((np.array([0, 2, 2, 3], dtype=np.uint32), np.array([1, 0, 1], dtype=np.uint32), (3, 2)), 8, backward=backward) as mh:\n"
              "        assert mh.info() == {'nnz': 3, 'device_bytes': 0} and mh.max_heads == 8")


def test_checker_rejects_planted_defects():
    """No library involved: a correct result (the references' own words, rounded once) passes, and each of three defects applied to it is
    rejected: lse stored [head][row], the dot reduced over the whole group (all heads' words) instead of the head, head h's D used for
    head h + 1."""
    hc = _cases()
    bc, ac = hc.bc, hc.ac
    indptr, indices = hc.random_pattern(hc.ROWS, hc.COLS, hc.NNZ, 9)
    shape, heads, d, scale = (hc.ROWS, hc.COLS), 3, 8, 0.5
    Q, K, V, gY = hc.operands(shape, heads * d, 7000)
    scores = hc.head_scores(indptr, indices, Q, K, heads)
    fwd = hc.forward_refs(scores, V, scale)
    y, lse = hc.rounded_forward(fwd)
    assert hc.check_forward(fwd, y, lse, "a correct forward result") <= 1.0
    bwd = hc.backward_refs(scores, V, gY, lse, scale)
    gq, gk, gv = hc.rounded_backward(bwd)
    assert max(hc.check_backward(bwd, gq, gk, gv, "a correct backward result").values()) <= 1.0
    # lse stored [head][row]: the same words, read back as [row][head]
    transposed = np.ascontiguousarray(lse.T).reshape(lse.shape)
    assert not np.array_equal(transposed.view(np.uint32), lse.view(np.uint32))
    with pytest.raises(AssertionError, match="lse"):
        hc.check_forward(fwd, y, transposed, "lse stored [head][row]")
    # the dot reduced over the whole group: every head weighs with the sum of all heads' scores
    whole = bc.scores_of(indptr, indices, Q, K)
    wrong_y = np.concatenate([ac.Reference(whole, hc.cut(V, h, d), scale).rounded()[0] for h in range(heads)], axis=1)
    with pytest.raises(AssertionError, match="words of y break"):
        hc.check_forward(fwd, wrong_y, None, "the dot over the whole group")
    # head h's D used for head h + 1
    grads = []
    for h, r in enumerate(bwd):
        other = bwd[h - 1].D[r.scores.of]
        grads.append(r.gradients(r.sc * r.P * (r.GP - other), r.P))
    wq, wk, wv = hc.rounded_backward(bwd, grads)
    with pytest.raises(AssertionError, match="words of gq break"):
        hc.check_backward(bwd, wq, gk, gv, "another head's D")
    with pytest.raises(AssertionError, match="words of gk break"):
        hc.check_backward(bwd, gq, wk, gv, "another head's D")
    assert hc.same_words((wv,), (gv,))      # gV does not depend on D


def test_cpu_twin_against_autograd():
    """40 x 50, about 600 entries (no pair twice: a dense mask holds a pair once), 3 heads of d = 8: hsmh_backward on the CPU twin, with lse
    from hsmh_forward on the CPU twin, against torch float64 autograd of the dense masked multi-head attention
    Y_h = softmax(scale Q_h K_h^T + mask) V_h and the loss sum(gY * Y).  This guards the formulas and the head layout themselves, which the
    references share with the code.

    Per head this is tests/test_attention_backward_cpu.py's comparison, with its tolerance: the operands are multiples of 1/8 below 4, so
    every fp32 product is exact; what is left between the contract's function and autograd's is lse, P'_e = f_r P_e with
    f_r = exp(LSE_r - lse_r) and k_r = expm1(bound_lse_r), so
        |GS'_e - GS_e| <= |scale| P'_e (k_r |GP_e| + k_r (2 + k_r) |D'_r|),      |P'_e - P_e| <= k_r P'_e
    summed over a word's entries times |K_ej|, |Q_ej| or |gY_ej| and added to the contract's bound.  The forward's Y is held to autograd's
    Y inside the forward contract's own bound (exact products: the contract's function is autograd's)."""
    import tempfile

    import torch
    body = """
import wide_cases as wc
rng = np.random.default_rng(7100)
rows, cols, H, d, scale = 40, 50, 3, 8, 0.125
flat = np.sort(rng.choice(rows * cols, 600, replace=False))
indptr = np.zeros(rows + 1, dtype=np.uint32); indptr[1:] = np.cumsum(np.bincount(flat // cols, minlength=rows))
indices = (flat % cols).astype(np.uint32)
Q, gY = (wc.grid_values(rng, (rows, H * d)) for _ in range(2)); K, V = (wc.grid_values(rng, (cols, H * d)) for _ in range(2))
with heads.MultiHeadAttention((indptr, indices, (rows, cols)), H) as mh:
    y, lse = mh.forward(Q, K, V, H, scale)
    gq, gk, gv = mh.backward(Q, K, V, gY, lse, H, scale)
np.savez(PATH, indptr=indptr, indices=indices, Q=Q, K=K, V=V, gY=gY, y=y, lse=lse, gq=gq, gk=gk, gv=gv)
"""
    hc = _cases()
    ac = hc.ac
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "twin.npz")
        run_child(body.replace("PATH", repr(path)))
        z = dict(np.load(path))
    indptr, indices, Q, K, V, gY, lse = (z[k] for k in ("indptr", "indices", "Q", "K", "V", "gY", "lse"))
    rows, cols, H, d, scale = 40, 50, 3, 8, 0.125
    assert (np.diff(indptr.astype(np.int64)) > 0).all() and lse.shape == (rows, H)
    scores = hc.head_scores(indptr, indices, Q, K, H)
    fwd = hc.forward_refs(scores, V, scale)
    bwd = hc.backward_refs(scores, V, gY, lse, scale)
    of, ix = scores[0].of, scores[0].indices
    # autograd over (rows, H, d) tensors
    tq, tk, tv = (torch.tensor(a.astype(np.float64).reshape(-1, H, d), requires_grad=True) for a in (Q, K, V))
    mask = torch.full((rows, cols), -np.inf, dtype=torch.float64)
    mask[torch.tensor(of), torch.tensor(ix)] = 0.0
    p = torch.softmax(scale * torch.einsum("rhj,chj->hrc", tq, tk) + mask, dim=2)
    ty = torch.einsum("hrc,chj->rhj", p, tv)
    (ty * torch.tensor(gY.astype(np.float64).reshape(rows, H, d))).sum().backward()
    auto_y = ty.detach().numpy().reshape(rows, H * d)
    auto = [g.grad.numpy().reshape(-1, H * d) for g in (tq, tk, tv)]
    for h in range(H):
        s, f, r = scores[h], fwd[h], bwd[h]
        assert (s.A == np.abs((hc.cut(Q, h, d).astype(np.float64)[of] * hc.cut(K, h, d).astype(np.float64)[ix])).sum(axis=1)).all()      # the fp32 products are exact
        assert (np.abs(lse[:, h].astype(np.float64) - f.LSE) <= f.bound_lse).all()
        assert (np.abs(f.Y - hc.cut(auto_y, h, d)) <= 2.0 ** -40 * (1.0 + np.abs(f.Y))).all(), f"the forward formula, head {h}"
        k = np.expm1(f.bound_lse)[of]
        d_gs = abs(r.sc) * r.P * (k * np.abs(r.GP) + k * (2.0 + k) * np.abs(r.D[of]))
        d_p = k * r.P
        pm = r.perm
        extra = {"gq": ac._seg_sum(d_gs[:, None] * np.abs(r.K64), s.indptr), "gk": ac._seg_sum((d_gs[:, None] * np.abs(r.Q64))[pm], r.cptr),
                 "gv": ac._seg_sum((d_p[:, None] * np.abs(r.G64))[pm], r.cptr)}
        mine = {"gq": r.GQ, "gk": r.GK, "gv": r.GV}
        r.want = {name: hc.cut(a, h, d) for name, a in zip(hc.bc.OUTPUTS, auto)}
        worst = r.check(*(hc.cut(z[name], h, d) for name in hc.bc.OUTPUTS), f"the CPU twin against autograd, head {h}", extra=extra)
        assert max(worst.values()) <= 1.0
        for name in hc.bc.OUTPUTS:      # the formula alone: the reference's own float64 gradients against autograd's
            assert (np.abs(mine[name] - r.want[name]) <= extra[name] + 2.0 ** -40 * (1.0 + np.abs(mine[name]))).all(), (name, h)
    hc.check_forward(fwd, z["y"], lse, "the CPU twin's forward")


def prototypes():
    text = open(os.path.join(ROOT, "include", "hisparse_heads.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(hsmh_[a-z0-9_]+)\s*\(", text)))


def test_header_libraries_and_binding_agree():
    """exactly eleven hsmh_* names in the header, the object's type and ten functions; exactly those ten functions in both libraries and
    in the binding's EXPORTS, apart from every other object's names; none in hisparse_hip.h, which names the header"""
    from hisparse_amd import attention, attention_backward, device, heads, pattern, rows, wide
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hisparse_heads.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\bhsmh_[a-z0-9_]+\b", header))) == sorted(NAMES + ["hsmh_pattern"])
    assert re.search(r"#define\s+HSMH_BACKWARD\s+1u", header)
    names = prototypes()
    assert names == NAMES and len(names) == 10
    assert sorted(heads.EXPORTS) == names and heads.BACKWARD == 1
    others = set(device.EXPORTS) | set(pattern.EXPORTS) | set(rows.EXPORTS) | set(wide.EXPORTS) | set(attention.EXPORTS) | set(attention_backward.EXPORTS)
    assert not set(names) & others      # an object of its own
    for lib in ("libhisparse_hip.so", "libhisparse_cpu.so"):
        exported = subprocess.run(["nm", "-D", "--defined-only", os.path.join(LIBDIR, lib)], capture_output=True, text=True, check=True).stdout
        assert sorted(set(re.findall(r"\b(hsmh_[a-z0-9_]+)\b", exported))) == names, lib
        l = ctypes.CDLL(os.path.join(LIBDIR, lib))
        for n in names:
            assert hasattr(l, n), (lib, n)
    bound = heads.lib()
    for n in names:
        assert getattr(bound, n).argtypes is not None, n
    import hisparse_amd
    assert hisparse_amd.heads is heads and "heads" in hisparse_amd.__all__
    hip_h = open(os.path.join(ROOT, "include", "hisparse_hip.h")).read()
    assert "hisparse_heads.h" in hip_h and not re.search(r"\bhsmh_[a-z_]+\s*\(", re.sub(r"/\*.*?\*/", "", hip_h, flags=re.S))


def test_schedule_is_the_wide_products_unchanged():
    """heads_attention.h adds no kWide* constant and the launchers take the classes, teams and grid cap from wide_products.h at the width
    heads * d; the three kernels' names stay apart from the single-head kernels', which other tests count"""
    text = open(os.path.join(ROOT, "hisparse_amd", "csrc", "heads_attention.h")).read()
    assert '#include "wide_products.h"' in text and not re.search(r"constexpr\s+\w+\s+kWide", text)
    hip = open(os.path.join(ROOT, "hisparse_amd", "csrc", "heads_attention.hip")).read()
    assert not re.search(r"constexpr\s+\w+\s+kWide", hip)
    for name in ("wide_table(s.count, heads * d)", "wide_group_lanes(heads * d)", "kWideBlocksPerCu", "kWideInFlight", "kWideThreads"):
        assert name in hip, name
    kernels = re.findall(r"__global__[^\n]*?\bvoid\s+(\w+)\s*\(", hip)
    assert sorted(kernels) == ["heads_backward_cols_kernel", "heads_backward_rows_kernel", "heads_forward_kernel"]
    for k in kernels:
        assert not any(old in k for old in ("pattern_attention_kernel", "attention_backward_rows_kernel", "attention_backward_cols_kernel"))


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present")
def test_hip_library_has_no_cpu_fallback():
    from hisparse_amd import device, heads
    if not device._LIB_PATH.endswith("libhisparse_hip.so"):
        pytest.skip("another library is selected")
    with pytest.raises(device.DeviceError) as e:
        heads.MultiHeadAttention((np.array([0, 1], dtype=np.uint32), np.array([0], dtype=np.uint32), (1, 1)), 1)
    assert e.value.code in (-2, -3) and str(e.value)


def test_cpu_twin_stand_alone_under_the_sanitizers(tmp_path):
    """tests/cpp/test_heads_cpu.cpp: the edge patterns and the refusals through the C boundary, compiled together with hsmh_cpu.cpp under
    -fsanitize=address,undefined with the runtimes linked in statically (a program of its own: nothing loaded into python is run under a
    sanitizer)."""
    exe = tmp_path / "heads_cpu"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", f"-I{ROOT}/include", f"-I{ROOT}/hisparse_amd/csrc", f"{ROOT}/tests/cpp/test_heads_cpu.cpp", f"{ROOT}/hisparse_amd/csrc/hsmh_cpu.cpp",
                           "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "HEADS CPU OK" in out.stdout, out.stdout + out.stderr

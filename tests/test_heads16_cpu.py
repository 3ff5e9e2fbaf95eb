"""The bf16 calls of the multi-head attention object (include/hisparse_heads_bf16.h) without a GPU: the cases of tests/heads16_cases.py on
libhisparse_cpu.so, each in a child process with HISPARSE_HIP_LIB set (as tests/test_heads_cpu.py runs its cases); to_bf16 against torch;
the checker against three planted defects; the CPU twin against torch's float64 autograd of the dense masked multi-head attention;
header, libraries and binding in agreement on exactly four functions; the CPU twin's source under the sanitizers as a stand-alone
program.  The same cases on the device: tests/test_gpu_heads16.py."""
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
from hisparse_amd import device, heads, heads16
import heads16_cases as c16
assert device._LIB_PATH.endswith("libhisparse_cpu.so")
mem = c16.HostMemory()
%(body)s
print("heads16 child ok")
"""

NAMES = ["hsmh16_backward", "hsmh16_backward_device", "hsmh16_forward", "hsmh16_forward_device"]
SHAPES = ((1, 8), (2, 8), (5, 8), (3, 16), (4, 32), (3, 32), (2, 64), (4, 64), (4, 128), (2, 256), (8, 64), (64, 8))


def run_child(body):
    if not os.path.exists(CPU_LIB):
        subprocess.check_call(["make", "-C", ROOT, "cpu"], stdout=subprocess.DEVNULL)
    env = dict(os.environ, HISPARSE_HIP_LIB=CPU_LIB)
    for k in [k for k in env if k.startswith("HISPARSE_") and k != "HISPARSE_HIP_LIB"]:
        env.pop(k)
    r = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests"), "body": body}], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "heads16 child ok" in r.stdout, r.stdout[-4000:] + r.stderr[-4000:]
    return r.stdout


def _cases():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import heads16_cases as c16
    return c16


def test_the_shapes_are_the_shared_ones():
    assert SHAPES == _cases().SHAPES


@pytest.mark.parametrize("heads,d", SHAPES)
def test_general(heads, d):
    """300 x 517, 4000 entries, scale 0.125, 1 and -2, pad 0 and 8 elements, ldl = heads and heads + 3, lse taken and NULL, both forms,
    forward then backward with the lse just written; the references assert their input condition on the bf16-rounded operands"""
    print("\n".join(l for l in run_child(f"c16.general(mem, (({heads}, {d}),))").splitlines() if "backward worst" in l or "input condition" in l))


def test_heads_do_not_leak():
    run_child("c16.heads_do_not_leak(mem)")


def test_edges():
    run_child("c16.edges(mem)")


def test_a_call_leaves_nothing_for_the_next_whichever_precision():
    run_child("c16.nothing_carried_over(mem)")


def test_forward_in_one_precision_backward_in_the_other():
    run_child("c16.mixed(mem)")


def test_refusals():
    run_child("c16.refusals(mem)")


def test_to_bf16_is_torchs_rounding():
    """10^5 random words plus NaN, +-inf, +-0, subnormals and exact ties: round to nearest even, NaN stays NaN; from_bf16 is exact"""
    import torch

    from hisparse_amd import heads16
    rng = np.random.default_rng(7200)
    special = np.array([0x7FC00000, 0x7F800001, 0xFFFFFFFF, 0xFFC00001, 0x7F800000, 0xFF800000, 0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x00008000, 0x00018000,
                        0x00008001, 0x007FFFFF, 0x3F808000, 0x3F818000, 0x3F808001, 0x3F807FFF, 0xBF808000, 0xBF818000, 0x7F7FFFFF, 0x7F7F8000, 0x7F7F7FFF, 0xFF7F8000], dtype=np.uint32)
    words = np.concatenate([rng.integers(0, 2 ** 32, 100000, dtype=np.uint64).astype(np.uint32), special])
    x = words.view(np.float32)
    got = heads16.to_bf16(x)
    want = torch.from_numpy(x.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    nan = np.isnan(x)
    assert got.dtype == np.uint16 and nan.sum() >= 4
    assert np.array_equal(got[~nan], want[~nan])
    back = heads16.from_bf16(got)
    assert np.isnan(back[nan]).all() and np.array_equal(got[nan] & 0x8000, (words[nan] >> 16) & 0x8000)      # NaN stays NaN, with its sign
    assert np.array_equal(back[~nan].view(np.uint32), want[~nan].astype(np.uint32) << 16)
    assert np.array_equal(heads16.to_bf16(back[~nan]), got[~nan])      # a bf16 value is kept


def test_checker_rejects_planted_defects():
    """No library involved: a correct result (the references' own words rounded to fp32 and then to bf16) passes and sits close under the
    bf16 term, which is therefore tight; each of three defects applied to it is rejected: outputs truncated instead of rounded, the dot
    reduced over a 16-byte chunk's neighbour head (head_lanes taken as d / 4, so the heads 2 k and 2 k + 1 of d = 8 share their
    score), the two elements of every dword swapped."""
    c16 = _cases()
    bc, ac = c16.bc, c16.hc.ac
    indptr, indices = c16.random_pattern(c16.ROWS, c16.COLS, c16.NNZ, 9)
    shape, heads, d, scale = (c16.ROWS, c16.COLS), 4, 8, 0.5
    Q, K, V, gY = c16.operands(shape, heads * d, 7300)
    scores = c16.head_scores(indptr, indices, Q, K, heads)
    fwd = c16.forward_refs(scores, V, scale)
    y32, lse = c16.rounded_forward(fwd)
    y = c16.twice(y32)
    assert c16.check_forward(fwd, y, lse, "a correct forward result") <= 1.0
    bwd = c16.backward_refs(scores, V, gY, lse, scale)
    g32 = c16.rounded_backward(bwd)
    gq, gk, gv = (c16.twice(g) for g in g32)
    assert max(c16.check_backward(bwd, gq, gk, gv, "a correct backward result").values()) <= 1.0
    # the bound is tight: the rounded words use more than 0.9 of the half-ulp term somewhere
    f = fwd[0].finite
    used = np.abs(c16.cut(y, 0, d).astype(np.float64)[f] - fwd[0].Y[f]) / (c16.HALF_ULP * np.abs(fwd[0].Y[f]) + c16.HALF_SUBNORMAL)
    print(f"the second rounding uses up to {used.max():.3f} of 2^-8 |x|")
    assert 0.9 < used.max() <= 1.0 + 2.0 ** -14
    # truncated instead of rounded
    cut_off = lambda a: (np.ascontiguousarray(a, dtype=np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)      # noqa: E731
    with pytest.raises(AssertionError, match="words of y break"):
        c16.check_forward(fwd, cut_off(y32), lse, "y truncated")
    for i, name in enumerate(bc.OUTPUTS):
        wrong = [gq, gk, gv]
        wrong[i] = cut_off(g32[i])
        with pytest.raises(AssertionError, match=f"words of {name} break"):
            c16.check_backward(bwd, *wrong, f"{name} truncated")
    # the dot reduced over the neighbour head too: heads 2 k and 2 k + 1 weigh with the sum of their two scores
    pairs = [bc.scores_of(indptr, indices, np.ascontiguousarray(Q[:, 2 * d * (h // 2): 2 * d * (h // 2 + 1)]), np.ascontiguousarray(K[:, 2 * d * (h // 2): 2 * d * (h // 2 + 1)]))
             for h in range(heads)]
    wrong_y = c16.twice(np.concatenate([ac.Reference(pairs[h], c16.cut(V, h, d), scale).rounded()[0] for h in range(heads)], axis=1))
    with pytest.raises(AssertionError, match="words of y break"):
        c16.check_forward(fwd, wrong_y, None, "the dot over two heads")
    # the two elements of every dword swapped
    swap = lambda a: np.ascontiguousarray(a.reshape(a.shape[0], -1, 2)[:, :, ::-1]).reshape(a.shape)      # noqa: E731
    with pytest.raises(AssertionError, match="words of y break"):
        c16.check_forward(fwd, swap(y), lse, "elements swapped")
    with pytest.raises(AssertionError, match="words of gq break"):
        c16.check_backward(bwd, swap(gq), gk, gv, "elements swapped")
    with pytest.raises(AssertionError, match="words of gv break"):
        c16.check_backward(bwd, gq, gk, swap(gv), "elements swapped")


def test_cpu_twin_against_autograd():
    """40 x 50, about 600 entries, 3 heads of d = 8 with the grid operands of wide_cases.grid_values (multiples of 1/8 below 4: bf16 values,
    and every fp32 product exact): hsmh16_backward on the CPU twin, with lse from hsmh16_forward on the CPU twin, against torch float64
    autograd of the dense masked multi-head attention.  The comparison and its tolerance are tests/test_heads_cpu.py's
    (test_cpu_twin_against_autograd there derives the lse term) plus the bf16 term of every output word."""
    import tempfile

    import torch
    body = """
import wide_cases as wc
rng = np.random.default_rng(7400)
rows, cols, H, d, scale = 40, 50, 3, 8, 0.125
flat = np.sort(rng.choice(rows * cols, 600, replace=False))
indptr = np.zeros(rows + 1, dtype=np.uint32); indptr[1:] = np.cumsum(np.bincount(flat // cols, minlength=rows))
indices = (flat % cols).astype(np.uint32)
Q, gY = (wc.grid_values(rng, (rows, H * d)) for _ in range(2)); K, V = (wc.grid_values(rng, (cols, H * d)) for _ in range(2))
with heads16.MultiHeadAttentionBF16((indptr, indices, (rows, cols)), H) as mh:
    y, lse = c16.forward_host(mh, Q, K, V, H, scale)
    gq, gk, gv = c16.backward_host(mh, Q, K, V, gY, lse, H, scale)
np.savez(PATH, indptr=indptr, indices=indices, Q=Q, K=K, V=V, gY=gY, y=y, lse=lse, gq=gq, gk=gk, gv=gv)
"""
    c16 = _cases()
    hc = c16.hc
    ac = hc.ac
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "twin16.npz")
        run_child(body.replace("PATH", repr(path)))
        z = dict(np.load(path))
    indptr, indices, Q, K, V, gY, lse = (z[k] for k in ("indptr", "indices", "Q", "K", "V", "gY", "lse"))
    rows, cols, H, d, scale = 40, 50, 3, 8, 0.125
    assert (np.diff(indptr.astype(np.int64)) > 0).all() and lse.shape == (rows, H)
    scores = c16.head_scores(indptr, indices, Q, K, H)
    fwd = c16.forward_refs(scores, V, scale)
    bwd = c16.backward_refs(scores, V, gY, lse, scale)
    of, ix = scores[0].of, scores[0].indices
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
        r.want = {name: hc.cut(a, h, d) for name, a in zip(hc.bc.OUTPUTS, auto)}
        extra = {name: extra[name] + c16.bf16_term(r.want[name], r.bound[name] + extra[name]) for name in hc.bc.OUTPUTS}
        worst = r.check(*(hc.cut(z[name], h, d) for name in hc.bc.OUTPUTS), f"the bf16 CPU twin against autograd, head {h}", extra=extra)
        assert max(worst.values()) <= 1.0
    c16.check_forward(fwd, z["y"], lse, "the bf16 CPU twin's forward")


def test_header_libraries_and_binding_agree():
    """exactly four hsmh16_* names in the header, in both libraries and in the binding's EXPORTS, apart from every other object's names;
    the header includes hisparse_heads.h and hisparse_hip.h names it"""
    from hisparse_amd import attention, attention_backward, device, heads, heads16, pattern, rows, wide
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hisparse_heads_bf16.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\bhsmh16_[a-z0-9_]+\b", header))) == NAMES
    assert sorted(set(re.findall(r"\b(hsmh16_[a-z0-9_]+)\s*\(", header))) == NAMES and '#include "hisparse_heads.h"' in header
    assert set(re.findall(r"\bhsmh_[a-z0-9_]+\b", header)) == {"hsmh_pattern"}      # the existing object's type and nothing else of it
    assert sorted(heads16.EXPORTS) == NAMES
    others = set(device.EXPORTS) | set(pattern.EXPORTS) | set(rows.EXPORTS) | set(wide.EXPORTS) | set(attention.EXPORTS) | set(attention_backward.EXPORTS) | set(heads.EXPORTS)
    assert not set(NAMES) & others
    for lib in ("libhisparse_hip.so", "libhisparse_cpu.so"):
        exported = subprocess.run(["nm", "-D", "--defined-only", os.path.join(LIBDIR, lib)], capture_output=True, text=True, check=True).stdout
        assert sorted(set(re.findall(r"\b(hsmh16_[a-z0-9_]+)\b", exported))) == NAMES, lib
        l = ctypes.CDLL(os.path.join(LIBDIR, lib))
        for n in NAMES:
            assert hasattr(l, n), (lib, n)
    bound = heads16.lib()
    for n in NAMES:
        assert getattr(bound, n).argtypes is not None, n
    assert bound is heads.lib() and issubclass(heads16.MultiHeadAttentionBF16, heads.MultiHeadAttention)
    import hisparse_amd
    assert hisparse_amd.heads16 is heads16 and "heads16" in hisparse_amd.__all__
    hip_h = open(os.path.join(ROOT, "include", "hisparse_hip.h")).read()
    assert "hisparse_heads_bf16.h" in hip_h and not re.search(r"\bhsmh16_[a-z_]+\s*\(", re.sub(r"/\*.*?\*/", "", hip_h, flags=re.S))


def test_schedule_is_the_wide_products_at_the_rows_chunks():
    """heads16_attention.{h,hip} add no kWide* constant, the launchers take the classes, teams and grid cap from wide_products.h at the
    row's size in 16-byte chunks (heads * d / 2), and the file holds exactly the three kernels"""
    text = open(os.path.join(ROOT, "hisparse_amd", "csrc", "heads16_attention.h")).read()
    assert '#include "wide_products.h"' in text and not re.search(r"constexpr\s+\w+\s+kWide", text)
    hip = open(os.path.join(ROOT, "hisparse_amd", "csrc", "heads16_attention.hip")).read()
    assert not re.search(r"constexpr\s+\w+\s+kWide", hip) and "asm" not in re.sub(r"//[^\n]*", "", hip) and "atomic" not in re.sub(r"//[^\n]*", "", hip)
    for name in ("wide_table(s.count, heads * d / 2)", "wide_group_lanes(heads * d / 2)", "kWideBlocksPerCu", "kWideInFlight", "kWideThreads"):
        assert name in hip, name
    kernels = re.findall(r"__global__[^\n]*?\bvoid\s+(\w+)\s*\(", hip)
    assert sorted(kernels) == ["heads16_backward_cols_kernel", "heads16_backward_rows_kernel", "heads16_forward_kernel"]


def test_cpu_twin_stand_alone_under_the_sanitizers(tmp_path):
    """tests/cpp/test_heads16_cpu.cpp: the edge patterns and the refusals through the C boundary, compiled together with hsmh_cpu.cpp under
    -fsanitize=address,undefined with the runtimes linked in statically (a program of its own: nothing loaded into python is run under a
    sanitizer)."""
    exe = tmp_path / "heads16_cpu"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", f"-I{ROOT}/include", f"-I{ROOT}/hisparse_amd/csrc", f"{ROOT}/tests/cpp/test_heads16_cpu.cpp", f"{ROOT}/hisparse_amd/csrc/hsmh_cpu.cpp",
                           "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "HEADS16 CPU OK" in out.stdout, out.stdout + out.stderr

"""The bf16 multi-head attention calls with a bias and dropout (include/hisparse_heads_dropout_bf16.h) without a GPU: the cases of
tests/heads16_dropout_cases.py on libhisparse_cpu.so, each in a child process with HISPARSE_HIP_LIB set (as tests/test_heads_dropout_cpu.py
runs its cases); the checker against five planted defects; the CPU twin against torch's float64 autograd of the dense masked multi-head
attention with bias and dropout on bf16-representable operands; header, libraries and binding in agreement on exactly four functions;
the CPU twin's source under the sanitizers as a stand-alone program.  The same cases on the device: tests/test_gpu_heads16_dropout.py."""
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
from hisparse_amd import device, heads, heads16, heads_dropout, heads16_dropout
import heads16_dropout_cases as hdx
assert device._LIB_PATH.endswith("libhisparse_cpu.so")
mem = hdx.HostMemory()
%(body)s
print("heads16 dropout child ok")
"""

NAMES = ["hsmhd16_backward", "hsmhd16_backward_device", "hsmhd16_forward", "hsmhd16_forward_device"]


def run_child(body):
    if not os.path.exists(CPU_LIB):
        subprocess.check_call(["make", "-C", ROOT, "cpu"], stdout=subprocess.DEVNULL)
    env = dict(os.environ, HISPARSE_HIP_LIB=CPU_LIB)
    for k in [k for k in env if k.startswith("HISPARSE_") and k != "HISPARSE_HIP_LIB"]:
        env.pop(k)
    r = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests"), "body": body}], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "heads16 dropout child ok" in r.stdout, r.stdout[-4000:] + r.stderr[-4000:]
    return r.stdout


def _cases():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import heads16_dropout_cases as hdx
    return hdx


def _keep_mask(nnz, heads, drop_p, seed, offset):
    """hsmhd_keep_mask of libhisparse_cpu.so through ctypes alone (host code, no object; tests/test_heads_dropout_cpu.py holds it to an
    independent numpy Philox4x32-10): (nnz, heads) uint8"""
    l = ctypes.CDLL(CPU_LIB)
    l.hsmhd_keep_mask.argtypes = [ctypes.c_uint64, ctypes.c_uint32, ctypes.c_float, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p]
    keep = np.full((nnz, heads), 9, dtype=np.uint8)
    assert l.hsmhd_keep_mask(nnz, heads, drop_p, seed, offset, keep.ctypes.data) == 0
    return keep


SHAPES = _cases().GENERAL_SHAPES      # heads16_cases.SHAPES and (8, 16)


# ---- the cases on the CPU twin ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("heads,d", SHAPES)
def test_general(heads, d):
    """300 x 517, 4000 entries, drop_p 0.1 and 0.5, a bias and NULL, both forms, tight and padded, lse and gbias taken and NULL"""
    print("\n".join(l for l in run_child(f"hdx.general(mem, (({heads}, {d}),))").splitlines() if "backward worst" in l))


def test_drop_zero_gives_the_words_of_the_bf16_calls():
    run_child("hdx.zero_drop(mem)")


def test_forward_and_backward_agree_on_the_mask():
    run_child("hdx.mask_agreement(mem)")


def test_fully_dropped_rows():
    run_child("hdx.fully_dropped_rows(mem)")


def test_cross_precision():
    run_child("hdx.cross_precision(mem)")


def test_long_rows_and_columns():
    """the host has no grid: 2000 rows and columns hold the long row and the long column"""
    run_child("hdx.long_rows_and_columns(mem, 2000)")


def test_edges():
    run_child("hdx.edges(mem)")


def test_seeds_and_offsets():
    run_child("hdx.seeds_and_offsets(mem)")


def test_a_masking_bias_with_dropout():
    run_child("hdx.mask_and_dropout(mem)")


def test_refusals():
    run_child("hdx.refusals(mem)")


# ---- the checker ---------------------------------------------------------------------------------------------------------------------------
def test_checker_rejects_planted_defects():
    """The mask is hsmhd_keep_mask's, nothing else of a library is involved: a correct result (the references' own words, rounded to fp32 and then to bf16;
    lse and gbias rounded once) passes, and each of five defects planted in it is rejected: the column side keyed by an entry's position
    in the transposed order instead of its CSR index; c applied twice; gbias of a dropped entry set to zero instead of -P D; the mask of
    head h & 3 used for head h; the output truncated to bf16 instead of rounded."""
    hdx = _cases()
    h16 = hdx.h16
    keep_mask = _keep_mask
    indptr, indices = hdx.random_pattern(hdx.ROWS, hdx.COLS, hdx.NNZ, 9)
    shape, heads, d, scale, p, seed, offset = (hdx.ROWS, hdx.COLS), 5, 8, 0.5, 0.5, 2024, 77
    Q, K, V, gY = hdx.operands(shape, heads * d, 19000)
    bias = hdx.biases(hdx.NNZ, heads, 19010)
    scores = hdx.head_scores(indptr, indices, Q, K, heads)
    keep = keep_mask(hdx.NNZ, heads, p, seed, offset)
    W = hdx.weights(keep, p)
    fwd = hdx.forward_refs(scores, V, scale, bias, W)
    y32, lse = hdx.rounded_forward(fwd)
    y = h16.twice(y32)
    assert hdx.check_forward(fwd, y, lse, "a correct forward result") <= 1.0
    bwd = hdx.backward_refs(scores, V, gY, lse, scale, bias, W)
    gq, gk, gv = (h16.twice(g) for g in hdx.rounded_backward(bwd))
    gb = hdx.rounded_gbias(bwd)
    assert max(hdx.check_backward(bwd, gq, gk, gv, "a correct backward result").values()) <= 1.0 and hdx.check_gbias(bwd, gb, "a correct gbias") <= 1.0

    def wrong_backward(wrong_W):
        wrong = hdx.backward_refs(scores, V, gY, lse, scale, bias, wrong_W)
        return tuple(h16.twice(g) for g in hdx.rounded_backward(wrong)) + (hdx.rounded_gbias(wrong),)

    # 1. the column side indexes the mask by the transposed entry index: the entry with CSR index perm[e'] is given W[e'].  gQ and D come
    # from the row side and stay right; gK, gV and gbias come from the column side
    by_column = np.empty_like(W)
    by_column[bwd[0].perm] = W
    _, wk, wv, wb = wrong_backward(by_column)
    with pytest.raises(AssertionError, match="words of gk break"):
        hdx.check_backward(bwd, gq, wk, gv, "the mask by the transposed index")
    with pytest.raises(AssertionError, match="words of gv break"):
        hdx.check_backward(bwd, gq, gk, wv, "the mask by the transposed index")
    with pytest.raises(AssertionError, match="words of gbias break"):
        hdx.check_gbias(bwd, wb, "the mask by the transposed index")
    # 2. c applied twice: w = keep c^2
    c = hdx.hd.scale_c(p)
    twice_c = W * c
    with pytest.raises(AssertionError, match="words of y break"):
        hdx.check_forward(fwd, h16.twice(hdx.rounded_forward(hdx.forward_refs(scores, V, scale, bias, twice_c))[0]), None, "c applied twice")
    wq, wk, wv, wb = wrong_backward(twice_c)
    for name, args in (("gq", (wq, gk, gv)), ("gk", (gq, wk, gv)), ("gv", (gq, gk, wv))):
        with pytest.raises(AssertionError, match=f"words of {name} break"):
            hdx.check_backward(bwd, *args, "c applied twice")
    with pytest.raises(AssertionError, match="words of gbias break"):
        hdx.check_gbias(bwd, wb, "c applied twice")
    # 3. gbias of a dropped entry set to zero instead of -P D
    zeroed = np.where(keep != 0, gb, np.float32(0.0))
    assert (gb[keep == 0] != 0).any()
    with pytest.raises(AssertionError, match="words of gbias break"):
        hdx.check_gbias(bwd, zeroed, "gbias of a dropped entry zeroed")
    # 4. the mask of head h & 3 used for head h: head 4 takes head 0's decisions, heads 0 ... 3 stay right
    folded = np.ascontiguousarray(W[:, np.arange(heads) & 3])
    assert np.array_equal(folded[:, :4], W[:, :4]) and not np.array_equal(folded[:, 4], W[:, 4])
    with pytest.raises(AssertionError, match="words of y break"):
        hdx.check_forward(fwd, h16.twice(hdx.rounded_forward(hdx.forward_refs(scores, V, scale, bias, folded))[0]), None, "the mask of head h & 3")
    wq, wk, wv, wb = wrong_backward(folded)
    for name, args in (("gq", (wq, gk, gv)), ("gk", (gq, wk, gv)), ("gv", (gq, gk, wv))):
        with pytest.raises(AssertionError, match=f"words of {name} break"):
            hdx.check_backward(bwd, *args, "the mask of head h & 3")
    with pytest.raises(AssertionError, match="words of gbias break"):
        hdx.check_gbias(bwd, wb, "the mask of head h & 3")
    # 5. the output truncated to bf16: the low 16 bits of the fp32 word dropped
    def truncated(a):
        return (np.ascontiguousarray(a, dtype=np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    with pytest.raises(AssertionError, match="words of y break"):
        hdx.check_forward(fwd, truncated(y32), None, "truncation to bf16")
    tq, tk, tv = (truncated(g) for g in hdx.rounded_backward(bwd))
    for name, args in (("gq", (tq, gk, gv)), ("gk", (gq, tk, gv)), ("gv", (gq, gk, tv))):
        with pytest.raises(AssertionError, match=f"words of {name} break"):
            hdx.check_backward(bwd, *args, "truncation to bf16")


def test_cpu_twin_against_autograd():
    """40 x 50, about 600 entries (no pair twice: a dense mask holds a pair once), 3 heads of d = 8, drop_p = 0.3: hsmhd16_backward on the CPU
    twin, with lse from hsmhd16_forward on the CPU twin, against torch float64 autograd of
        Y_h = (M_h c softmax(scale Q_h K_h^T + B_h + mask)) V_h
    with M_h the dense keep matrix of head h from hsmhd_keep_mask, and the loss sum(gY * Y), g_bias included.  The operands and the bias
    are multiples of 1/8 below 4 (bf16 values) and scale is 1/8, so every fp32 product and t itself are exact.

    It is tests/test_heads_dropout_cpu.py's comparison with its extra terms (what lse's rounding leaves between the contract's function
    and autograd's), and on top of a word's fp32 bound b' = b + extra the header's term for its second rounding, bf16_term(x, b')."""
    import tempfile

    import torch
    body = """
import wide_cases as wc
rng = np.random.default_rng(19100)
rows, cols, H, d, scale, p, seed, offset = 40, 50, 3, 8, 0.125, 0.3, 99, (5 << 32) + 1
flat = np.sort(rng.choice(rows * cols, 600, replace=False))
indptr = np.zeros(rows + 1, dtype=np.uint32); indptr[1:] = np.cumsum(np.bincount(flat // cols, minlength=rows))
indices = (flat % cols).astype(np.uint32)
Q, gY = (wc.grid_values(rng, (rows, H * d)) for _ in range(2)); K, V = (wc.grid_values(rng, (cols, H * d)) for _ in range(2))
bias = wc.grid_values(rng, (600, H))
with heads16_dropout.DropoutMultiHeadAttentionBF16((indptr, indices, (rows, cols)), H) as mh:
    y, lse = hdx.forward_host(mh, Q, K, V, bias, H, scale, hdx.Drop(p, seed, offset))
    gq, gk, gv, gb = hdx.backward_host(mh, Q, K, V, gY, lse, bias, H, scale, hdx.Drop(p, seed, offset))
np.savez(PATH, indptr=indptr, indices=indices, Q=Q, K=K, V=V, gY=gY, bias=bias, y=y, lse=lse, gq=gq, gk=gk, gv=gv, gb=gb)
"""
    hdx = _cases()
    hd, ac = hdx.hd, hdx.hd.ac
    keep_mask = _keep_mask
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "twin.npz")
        run_child(body.replace("PATH", repr(path)))
        z = dict(np.load(path))
    indptr, indices, Q, K, V, gY, bias, lse = (z[k] for k in ("indptr", "indices", "Q", "K", "V", "gY", "bias", "lse"))
    rows, cols, H, d, scale, p, seed, offset = 40, 50, 3, 8, 0.125, 0.3, 99, (5 << 32) + 1
    assert (np.diff(indptr.astype(np.int64)) > 0).all() and lse.shape == (rows, H) and z["gb"].shape == (600, H)
    for a in (Q, K, V, gY):
        assert np.array_equal(hdx.h16.twice(a), a), "the operands are bf16 values"
    keep = keep_mask(600, H, p, seed, offset)
    assert 0.55 < keep.mean() < 0.85
    W = hd.weights(keep, p)
    scores = hdx.head_scores(indptr, indices, Q, K, H)
    fwd = hdx.forward_refs(scores, V, scale, bias, W)
    bwd = hdx.backward_refs(scores, V, gY, lse, scale, bias, W)
    of, ix = scores[0].of, scores[0].indices
    tq, tk, tv = (torch.tensor(a.astype(np.float64).reshape(-1, H, d), requires_grad=True) for a in (Q, K, V))
    dense = torch.full((H, rows, cols), -np.inf, dtype=torch.float64)
    dense[:, torch.tensor(of), torch.tensor(ix)] = torch.tensor(bias.astype(np.float64).T)
    dense.requires_grad_(True)
    mask = torch.zeros((H, rows, cols), dtype=torch.float64)
    mask[:, torch.tensor(of), torch.tensor(ix)] = torch.tensor(W.T)
    pr = mask * torch.softmax(scale * torch.einsum("rhj,chj->hrc", tq, tk) + dense, dim=2)
    ty = torch.einsum("hrc,chj->rhj", pr, tv)
    (ty * torch.tensor(gY.astype(np.float64).reshape(rows, H, d))).sum().backward()
    auto_y = ty.detach().numpy().reshape(rows, H * d)
    auto = [g.grad.numpy().reshape(-1, H * d) for g in (tq, tk, tv)]
    auto_gb = dense.grad.numpy()[:, of, ix].T      # (entries, H)
    for h in range(H):
        s, f, r = scores[h], fwd[h], bwd[h]
        assert (np.abs(lse[:, h].astype(np.float64) - f.LSE) <= f.bound_lse).all()
        assert (np.abs(f.Y - hdx.cut(auto_y, h, d)) <= 2.0 ** -40 * (1.0 + np.abs(f.Y))).all(), f"the forward formula, head {h}"
        k = np.expm1(f.bound_lse)[of]
        d_gb = r.P * (k * np.abs(r.GP) + k * (2.0 + k) * np.abs(r.D[of]))
        d_gs = abs(r.sc) * d_gb
        d_p = k * r.PW
        pm = r.perm
        extra = {"gq": ac._seg_sum(d_gs[:, None] * np.abs(r.K64), s.indptr), "gk": ac._seg_sum((d_gs[:, None] * np.abs(r.Q64))[pm], r.cptr),
                 "gv": ac._seg_sum((d_p[:, None] * np.abs(r.G64))[pm], r.cptr)}
        r.want = {name: hdx.cut(a, h, d) for name, a in zip(hd.bc.OUTPUTS, auto)}
        extra16 = {name: extra[name] + hdx.bf16_term(r.want[name], r.bound[name] + extra[name]) for name in hd.bc.OUTPUTS}
        worst = r.check(*(hdx.cut(z[name], h, d) for name in hd.bc.OUTPUTS), f"the CPU twin against autograd, head {h}", extra=extra16)
        assert max(worst.values()) <= 1.0
        assert r.check_gbias(np.ascontiguousarray(z["gb"][:, h]), f"the CPU twin's gbias against autograd, head {h}", extra=d_gb, want=auto_gb[:, h]) <= 1.0
        assert (auto_gb[keep[:, h] == 0, h] != 0).any(), "a dropped entry's gbias is -P D"
    hdx.check_forward(fwd, z["y"], lse, "the CPU twin's forward")


# ---- names, sources, the sanitizers ------------------------------------------------------------------------------------------------------
def test_header_libraries_and_binding_agree():
    """exactly four hsmhd16_* functions in the header, in both libraries and in the binding's EXPORTS, apart from every other module's
    names; the header holds no hsmh_ identifier but hsmh_pattern, includes hisparse_heads.h, and hisparse_hip.h names it in a line of its
    comment without repeating a prototype"""
    from hisparse_amd import attention, attention_backward, device, gat, gatv2, heads, heads16, heads16_dropout, heads_bias, heads_dropout, pattern, rows, wide
    text = open(os.path.join(ROOT, "include", "hisparse_heads_dropout_bf16.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert sorted(set(re.findall(r"\bhsmhd16_[a-z0-9_]+\b", header))) == NAMES
    assert sorted(set(re.findall(r"\b(hsmhd16_[a-z0-9_]+)\s*\(", header))) == NAMES and len(NAMES) == 4 and '#include "hisparse_heads.h"' in header
    assert set(re.findall(r"\bhsmh_[a-z0-9_]+\b", text)) == {"hsmh_pattern"}      # comment included: no new create, no new type
    assert not re.search(r"\bhsmh(b|d|16)_", header)
    assert sorted(heads16_dropout.EXPORTS) == NAMES
    others = set(device.EXPORTS) | set(pattern.EXPORTS) | set(rows.EXPORTS) | set(wide.EXPORTS) | set(attention.EXPORTS) | set(attention_backward.EXPORTS) | set(heads.EXPORTS) \
        | set(heads16.EXPORTS) | set(heads_bias.EXPORTS) | set(heads_dropout.EXPORTS) | set(gat.EXPORTS) | set(gatv2.EXPORTS)
    assert not set(NAMES) & others
    for lib in ("libhisparse_hip.so", "libhisparse_cpu.so"):
        exported = subprocess.run(["nm", "-D", "--defined-only", os.path.join(LIBDIR, lib)], capture_output=True, text=True, check=True).stdout
        assert sorted(set(re.findall(r"\b(hsmhd16_[a-z0-9_]+)\b", exported))) == NAMES, lib
        l = ctypes.CDLL(os.path.join(LIBDIR, lib))
        for n in NAMES:
            assert hasattr(l, n), (lib, n)
    bound = heads16_dropout.lib()
    for n in NAMES:
        assert getattr(bound, n).argtypes is not None, n
    assert bound is heads.lib() and issubclass(heads16_dropout.DropoutMultiHeadAttentionBF16, heads_dropout.DropoutMultiHeadAttention)
    for method in ("forward", "backward", "forward_device", "backward_device"):
        assert method in vars(heads16_dropout.DropoutMultiHeadAttentionBF16), method
    import hisparse_amd
    assert hisparse_amd.heads16_dropout is heads16_dropout and "heads16_dropout" in hisparse_amd.__all__
    hip_h = open(os.path.join(ROOT, "include", "hisparse_hip.h")).read()
    assert "hisparse_heads_dropout_bf16.h" in hip_h and not re.search(r"\bhsmhd16_[a-z_]+\s*\(", hip_h)
    common = open(os.path.join(ROOT, "hisparse_amd", "csrc", "hsmh_common.h")).read()
    assert '#include "hisparse_heads_dropout_bf16.h"' in common


def test_schedule_is_the_wide_products_unchanged():
    """heads16_dropout_attention.{h,hip} add no kWide* constant, the launchers take the classes, teams and grid cap from wide_products.h
    at the row's size in 16-byte chunks (heads * d / 2), the file holds exactly the three kernels under names no other kernel count
    matches, without inline assembly or atomics, and uses philox.h's keep and one ballot"""
    csrc = os.path.join(ROOT, "hisparse_amd", "csrc")
    text = open(os.path.join(csrc, "heads16_dropout_attention.h")).read()
    assert '#include "wide_products.h"' in text and '#include "philox.h"' in text and not re.search(r"constexpr\s+\w+\s+kWide", text)
    hip = open(os.path.join(csrc, "heads16_dropout_attention.hip")).read()
    code = re.sub(r"//[^\n]*", "", hip)
    assert not re.search(r"constexpr\s+\w+\s+kWide", hip) and "asm" not in code and "atomic" not in code
    for name in ("wide_table(s.count, heads * d / 2)", "wide_group_lanes(heads * d / 2)", "kWideBlocksPerCu", "kWideInFlight", "kWideThreads", "__builtin_nontemporal_load(perm + ei)",
                 "__fadd_rn(", "__fmul_rn(", "philox::keep(", "__ballot(", "place_of<kChunk>"):
        assert name in hip, name
    kernels = re.findall(r"__global__[^\n]*?\bvoid\s+(\w+)\s*\(", hip)
    assert sorted(kernels) == ["bf16_drop_cols_kernel", "bf16_drop_forward_kernel", "bf16_drop_rows_kernel"]
    for k in kernels:
        assert not any(old in k for old in ("heads16_", "dropout_attention_", "biased_attention_", "heads_forward", "heads_backward", "gat_", "gatv2_", "pattern_attention",
                                            "attention_backward_"))


def test_cpu_twin_stand_alone_under_the_sanitizers(tmp_path):
    """tests/cpp/test_heads16_dropout_cpu.cpp: the edge patterns and the refusals through the C boundary, compiled together with
    hsmh_cpu.cpp under -fsanitize=address,undefined with the runtimes linked in statically (a program of its own: nothing loaded into
    python is run under a sanitizer)."""
    exe = tmp_path / "heads16_dropout_cpu"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", f"-I{ROOT}/include", f"-I{ROOT}/hisparse_amd/csrc", f"{ROOT}/tests/cpp/test_heads16_dropout_cpu.cpp",
                           f"{ROOT}/hisparse_amd/csrc/hsmh_cpu.cpp", "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "HEADS16 DROPOUT CPU OK" in out.stdout, out.stdout + out.stderr

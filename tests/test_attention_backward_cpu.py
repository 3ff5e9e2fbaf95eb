"""The fused attention backward step (include/hisparse_attention_backward.h) without a GPU: the cases of tests/attention_backward_cases.py
on libhisparse_cpu.so, each in a child process with HISPARSE_HIP_LIB set (as tests/test_attention_cpu.py runs its cases); the reference
against four planted defects; the CPU twin against torch's float64 autograd of the dense masked attention; header, libraries and binding
in agreement on exactly nine names; the CPU twin's source under the sanitizers as a stand-alone program.  The same cases on the device:
tests/test_gpu_attention_backward.py."""
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
from hisparse_amd import attention, attention_backward, device
import attention_backward_cases as bc
assert device._LIB_PATH.endswith("libhisparse_cpu.so")
mem = bc.HostMemory()
%(body)s
print("attention backward child ok")
"""

NAMES = ["hsab_backward", "hsab_backward_device", "hsab_create", "hsab_destroy", "hsab_info", "hsab_last_error", "hsab_set_stream", "hsab_sync"]


def run_child(body):
    if not os.path.exists(CPU_LIB):
        subprocess.check_call(["make", "-C", ROOT, "cpu"], stdout=subprocess.DEVNULL)
    env = dict(os.environ, HISPARSE_HIP_LIB=CPU_LIB)
    for k in [k for k in env if k.startswith("HISPARSE_") and k != "HISPARSE_HIP_LIB"]:
        env.pop(k)
    r = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests"), "body": body}], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "attention backward child ok" in r.stdout, r.stdout + r.stderr
    return r.stdout


def test_general():
    """300 x 517, 4000 entries, d in {1, 3, 4, 5, 16, 17, 63, 64, 65, 128, 256}, scale 0.125, 1 and -2, pad 0 and 8, both forms"""
    print(run_child("bc.general(mem)").splitlines()[-2])


def test_edges():
    run_child("bc.edges(mem)")


def test_special_rows():
    run_child("bc.special_rows(mem)")


def test_scale_zero():
    run_child("bc.scale_zero(mem)")


def test_heads_by_leading_dimension():
    run_child("bc.heads(mem)")


def test_a_call_leaves_nothing_for_the_next():
    run_child("bc.nothing_carried_over(mem)")


def test_refusals():
    run_child("bc.refusals(mem)")


def test_info_holds_nothing_on_a_device():
    run_child("with attention_backward.PatternAttentionBackward((np.array([0, 2, 2, 3], dtype=np.uint32), np.array([1, 0, 1], dtype=np.uint32), (3, 2))) as pb:\n"
              "    assert pb.info() == {'nnz': 3, 'device_bytes': 0}")


def test_reference_rejects_planted_defects():
    """No library involved: a correct result (the reference's own words, rounded once) passes, and each of four defects applied to it is
    rejected: D dropped from gs, scale missing from gs, one word of each output off by twice its bound, gK and gV exchanged."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import attention_backward_cases as bc
    indptr, indices = bc.random_pattern(bc.ROWS, bc.COLS, bc.NNZ, 9)
    shape, d, scale = (bc.ROWS, bc.COLS), 5, 0.5
    Q, K, V, gY = bc.operands(shape, d, 4000)
    scores = bc.scores_of(indptr, indices, Q, K)
    lse = bc.forward_lse(scores, V, scale)
    ref = bc.Reference(scores, V, gY, lse, scale)
    gq, gk, gv = ref.rounded()
    assert max(ref.check(gq, gk, gv, "a correct result").values()) <= 1.0
    # D dropped: gs = scale p gp
    wq, wk, _ = ref.rounded(ref.gradients(ref.sc * ref.P * ref.GP, ref.P))
    with pytest.raises(AssertionError, match="words of gq break"):
        ref.check(wq, gk, gv, "D dropped")
    with pytest.raises(AssertionError, match="words of gk break"):
        ref.check(gq, wk, gv, "D dropped")
    # scale missing from gs
    wq, wk, _ = ref.rounded(ref.gradients(ref.GS / ref.sc, ref.P))
    with pytest.raises(AssertionError, match="words of gq break"):
        ref.check(wq, gk, gv, "scale missing")
    with pytest.raises(AssertionError, match="words of gk break"):
        ref.check(gq, wk, gv, "scale missing")
    # one word off by twice its bound
    for i, name in enumerate(bc.OUTPUTS):
        out = [gq.copy(), gk.copy(), gv.copy()]
        r, j = (int(k[0]) for k in np.nonzero(~ref.empty[name][:, None] & np.ones(d, dtype=bool)))
        off = ref.want[name][r, j] + 2.0 * ref.bound[name][r, j]
        out[i][r, j] = np.float32(off) if float(np.float32(off)) >= off else np.nextafter(np.float32(off), np.float32(np.inf))      # the fp32 word at or above it
        assert out[i][r, j] != (gq, gk, gv)[i][r, j]
        with pytest.raises(AssertionError, match=f"1 of .* words of {name} break"):
            ref.check(*out, f"one word of {name} off")
    # gK and gV exchanged
    with pytest.raises(AssertionError, match="words of gk break"):
        ref.check(gq, gv, gk, "gk and gv exchanged")


def test_cpu_twin_against_autograd():
    """40 x 50, about 600 entries (no pair twice: a dense mask holds a pair once), d = 8: hsab_backward on the CPU twin, with lse from
    hsat_forward on the CPU twin, against torch float64 autograd of the dense masked attention Y = softmax(scale Q K^T + mask) V and the
    loss sum(gY * Y).  This guards the formula itself, which the reference shares with the code.

    The operands are multiples of 1/8 below 4 (wide_cases.grid_values), so every fp32 product is exact and the contract's S_e and GP_e
    are the real dots that autograd sees.  What is left between the contract's function and autograd's is lse: the call forms
    P'_e = exp(T_e - lse_r) from the word it is given, autograd the true P_e = exp(T_e - LSE_r), so P'_e = f_r P_e with one factor
    f_r = exp(LSE_r - lse_r) per row, and with k_r = expm1(bound_lse_r) (attention_cases.Reference.bound_lse, which the forward's lse is
    asserted to keep) both |f - 1| and |1 / f - 1| are at most k_r, and |1 - 1 / f^2| <= expm1(2 bound_lse_r) = k_r (2 + k_r).  Then
    D' = f D and GS'_e = scale P'_e (GP_e - D'_r), so in terms of the primed quantities, which are the reference's,
        |GS'_e - GS_e| = |scale| P'_e |(1 - 1 / f) GP_e - (1 - 1 / f^2) D'_r| <= |scale| P'_e (k_r |GP_e| + k_r (2 + k_r) |D'_r|)
        |P'_e - P_e|   <= k_r P'_e
    and the tolerance per word is the contract's bound plus these, summed over the word's entries times |K_ej|, |Q_ej| or |gY_ej|: to
    first order expm1(bound_lse_r) times the bound's own magnitude sums (with 2 |D|).  Autograd's own float64 rounding, about 2^-52
    times the same sums, is far below the bound's 2^-24 terms."""
    import torch
    body = """
import wide_cases as wc, attention_cases as ac
rng = np.random.default_rng(4100)
rows, cols, d, scale = 40, 50, 8, 0.125
flat = np.sort(rng.choice(rows * cols, 600, replace=False))
indptr = np.zeros(rows + 1, dtype=np.uint32); indptr[1:] = np.cumsum(np.bincount(flat // cols, minlength=rows))
indices = (flat % cols).astype(np.uint32)
Q, gY = (wc.grid_values(rng, (rows, d)) for _ in range(2)); K, V = (wc.grid_values(rng, (cols, d)) for _ in range(2))
with attention.PatternAttention((indptr, indices, (rows, cols))) as pa, attention_backward.PatternAttentionBackward((indptr, indices, (rows, cols))) as pb:
    y, lse = pa.forward(Q, K, V, scale)
    gq, gk, gv = pb.backward(Q, K, V, gY, lse, scale)
np.savez(PATH, indptr=indptr, indices=indices, Q=Q, K=K, V=V, gY=gY, lse=lse, gq=gq, gk=gk, gv=gv)
"""
    import tempfile
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import attention_backward_cases as bc
    import attention_cases as ac
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "twin.npz")
        run_child(body.replace("PATH", repr(path)))
        z = dict(np.load(path))
    indptr, indices, Q, K, V, gY, lse = (z[k] for k in ("indptr", "indices", "Q", "K", "V", "gY", "lse"))
    rows, cols, d, scale = 40, 50, 8, 0.125
    assert (np.diff(indptr.astype(np.int64)) > 0).all()
    scores = bc.scores_of(indptr, indices, Q, K)
    assert (scores.A == np.abs((Q.astype(np.float64)[scores.of] * K.astype(np.float64)[scores.indices])).sum(axis=1)).all()      # the fp32 products are exact
    fwd = ac.Reference(scores, V, scale)
    assert (np.abs(lse.astype(np.float64) - fwd.LSE) <= fwd.bound_lse).all()
    ref = bc.Reference(scores, V, gY, lse, scale)
    # the tolerance for lse, from the reference's (primed) quantities
    k = np.expm1(fwd.bound_lse)[scores.of]
    d_gs = abs(ref.sc) * ref.P * (k * np.abs(ref.GP) + k * (2.0 + k) * np.abs(ref.D[scores.of]))
    d_p = k * ref.P
    pm = ref.perm
    extra = {"gq": ac._seg_sum(d_gs[:, None] * np.abs(ref.K64), scores.indptr), "gk": ac._seg_sum((d_gs[:, None] * np.abs(ref.Q64))[pm], ref.cptr),
             "gv": ac._seg_sum((d_p[:, None] * np.abs(ref.G64))[pm], ref.cptr)}
    # autograd
    tq, tk, tv = (torch.tensor(a.astype(np.float64), requires_grad=True) for a in (Q, K, V))
    mask = torch.full((rows, cols), -np.inf, dtype=torch.float64)
    mask[torch.tensor(scores.of), torch.tensor(scores.indices)] = 0.0
    y = torch.softmax(scale * (tq @ tk.T) + mask, dim=1) @ tv
    (y * torch.tensor(gY.astype(np.float64))).sum().backward()
    ref.want = {"gq": tq.grad.numpy(), "gk": tk.grad.numpy(), "gv": tv.grad.numpy()}
    worst = ref.check(z["gq"], z["gk"], z["gv"], "the CPU twin against autograd", extra=extra)
    # and the formula alone, without any rounding of the code's: the reference's own float64 gradients against autograd's
    for name, mine in zip(bc.OUTPUTS, (ref.GQ, ref.GK, ref.GV)):
        assert (np.abs(mine - ref.want[name]) <= extra[name] + 2.0 ** -40 * (1.0 + np.abs(mine))).all(), name
    assert max(worst.values()) <= 1.0


def prototypes():
    text = open(os.path.join(ROOT, "include", "hisparse_attention_backward.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(hsab_[a-z0-9_]+)\s*\(", text)))


def test_header_libraries_and_binding_agree():
    """exactly nine hsab_* names in the header, the object's type and eight functions; exactly those eight functions in both libraries and
    in the binding's EXPORTS, apart from every other object's names; none in hisparse_hip.h"""
    from hisparse_amd import attention, attention_backward, device, pattern, rows, wide
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hisparse_attention_backward.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\bhsab_[a-z0-9_]+\b", header))) == sorted(NAMES + ["hsab_pattern"])      # nine names: eight functions on one type
    names = prototypes()
    assert names == NAMES and len(names) == 8
    assert sorted(attention_backward.EXPORTS) == names
    others = set(device.EXPORTS) | set(pattern.EXPORTS) | set(rows.EXPORTS) | set(wide.EXPORTS) | set(attention.EXPORTS)
    assert not set(names) & others      # an object of its own
    for lib in ("libhisparse_hip.so", "libhisparse_cpu.so"):
        exported = subprocess.run(["nm", "-D", "--defined-only", os.path.join(LIBDIR, lib)], capture_output=True, text=True, check=True).stdout
        assert sorted(set(re.findall(r"\b(hsab_[a-z0-9_]+)\b", exported))) == names, lib
        l = ctypes.CDLL(os.path.join(LIBDIR, lib))
        for n in names:
            assert hasattr(l, n), (lib, n)
    bound = attention_backward.lib()
    for n in names:
        assert getattr(bound, n).argtypes is not None, n
    import hisparse_amd
    assert hisparse_amd.attention_backward is attention_backward
    hip_h = open(os.path.join(ROOT, "include", "hisparse_hip.h")).read()
    assert "hisparse_attention_backward.h" in hip_h and not re.search(r"\bhsab_[a-z_]+\s*\(", re.sub(r"/\*.*?\*/", "", hip_h, flags=re.S))


def test_schedule_is_the_wide_products_unchanged():
    """attention_backward.h adds no kWide* constant and both launchers take the classes, teams and grid cap from wide_products.h"""
    text = open(os.path.join(ROOT, "hisparse_amd", "csrc", "attention_backward.h")).read()
    assert '#include "wide_products.h"' in text and not re.search(r"constexpr\s+\w+\s+kWide", text)
    hip = open(os.path.join(ROOT, "hisparse_amd", "csrc", "attention_backward.hip")).read()
    assert not re.search(r"constexpr\s+\w+\s+kWide", hip)
    for name in ("wide_table", "wide_group_lanes", "kWideBlocksPerCu", "kWideInFlight", "kWideThreads"):
        assert name in hip, name


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present")
def test_hip_library_has_no_cpu_fallback():
    from hisparse_amd import attention_backward, device
    if not device._LIB_PATH.endswith("libhisparse_hip.so"):
        pytest.skip("another library is selected")
    with pytest.raises(device.DeviceError) as e:
        attention_backward.PatternAttentionBackward((np.array([0, 1], dtype=np.uint32), np.array([0], dtype=np.uint32), (1, 1)))
    assert e.value.code in (-2, -3) and str(e.value)


def test_cpu_twin_stand_alone_under_the_sanitizers(tmp_path):
    """tests/cpp/test_attention_backward_cpu.cpp: the edge patterns, the special rows and the refusals through the C boundary, compiled
    together with hsab_cpu.cpp under -fsanitize=address,undefined with the runtimes linked in statically (a program of its own: nothing
    loaded into python is run under a sanitizer)."""
    exe = tmp_path / "attention_backward_cpu"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", f"-I{ROOT}/include", f"-I{ROOT}/hisparse_amd/csrc", f"{ROOT}/tests/cpp/test_attention_backward_cpu.cpp",
                           f"{ROOT}/hisparse_amd/csrc/hsab_cpu.cpp", "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "ATTENTION BACKWARD CPU OK" in out.stdout, out.stdout + out.stderr

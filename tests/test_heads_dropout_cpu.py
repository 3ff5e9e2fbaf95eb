"""The multi-head attention calls with dropout on the attention weights (include/hisparse_heads_dropout.h) without a GPU: the cases of
tests/heads_dropout_cases.py on libhisparse_cpu.so, each in a child process with HISPARSE_HIP_LIB set (as tests/test_heads_bias_cpu.py
runs its cases); hsmhd_keep_mask of both libraries against an independent numpy Philox4x32-10 that is itself held to the header's three
known answers; the kept share against the binomial; the restated references anchored to the bias references at drop_p = 0; the checker
against five planted defects; the CPU twin against torch's float64 autograd of the dense masked multi-head attention with dropout;
header, libraries and binding in agreement on exactly five functions; the CPU twin's source under the sanitizers as a stand-alone
program.  The same cases on the device: tests/test_gpu_heads_dropout.py."""
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
from hisparse_amd import device, heads, heads_bias, heads_dropout
import heads_dropout_cases as hd
assert device._LIB_PATH.endswith("libhisparse_cpu.so")
mem = hd.HostMemory()
%(body)s
print("heads dropout child ok")
"""

NAMES = ["hsmhd_backward", "hsmhd_backward_device", "hsmhd_forward", "hsmhd_forward_device", "hsmhd_keep_mask"]


def run_child(body):
    if not os.path.exists(CPU_LIB):
        subprocess.check_call(["make", "-C", ROOT, "cpu"], stdout=subprocess.DEVNULL)
    env = dict(os.environ, HISPARSE_HIP_LIB=CPU_LIB)
    for k in [k for k in env if k.startswith("HISPARSE_") and k != "HISPARSE_HIP_LIB"]:
        env.pop(k)
    r = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests"), "body": body}], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "heads dropout child ok" in r.stdout, r.stdout[-4000:] + r.stderr[-4000:]
    return r.stdout


def _cases():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import heads_dropout_cases as hd
    return hd


SHAPES = _cases().GENERAL_SHAPES      # heads_cases.SHAPES and (8, 16)


# ---- an independent Philox4x32-10, in numpy uint64 arithmetic ---------------------------------------------------------------------------
def philox4x32_10(counter, key):
    """counter: four arrays (or ints) of 32-bit words, key: two; returns the four output words as uint64 arrays below 2^32"""
    c = [np.atleast_1d(np.asarray(x, dtype=np.uint64)) for x in counter]
    k = [np.uint64(key[0]), np.uint64(key[1])]
    m0, m1, lo32, s32 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0xFFFFFFFF), np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * c[0], m1 * c[2]      # 32 x 32 bits: no overflow of 64
        c = [(p1 >> s32) ^ c[1] ^ k[0], p1 & lo32, (p0 >> s32) ^ c[3] ^ k[1], p0 & lo32]
        k = [(k[0] + np.uint64(0x9E3779B9)) & lo32, (k[1] + np.uint64(0xBB67AE85)) & lo32]
    return c


def numpy_keep_mask(nnz, heads, drop_p, seed, offset):
    """the header's keep decision: (nnz, heads) uint8"""
    thr = np.uint64(int(np.floor(float(np.float32(drop_p)) * 4294967296.0)))
    e = np.arange(nnz, dtype=np.uint64)
    keep = np.zeros((nnz, heads), dtype=np.uint8)
    for quad in range((heads + 3) // 4):
        x = philox4x32_10((e, np.full(nnz, quad, dtype=np.uint64), offset & 0xFFFFFFFF, offset >> 32), (seed & 0xFFFFFFFF, seed >> 32))
        for h in range(4 * quad, min(heads, 4 * quad + 4)):
            keep[:, h] = np.broadcast_to(x[h & 3], (nnz,)) >= thr
    return keep


def test_numpy_philox_gives_the_known_answers():
    known = (((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
             ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
             ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)))
    for counter, key, want in known:
        assert tuple(int(x[0]) for x in philox4x32_10(counter, key)) == want, (counter, key)


@pytest.mark.parametrize("lib", ["libhisparse_cpu.so", "libhisparse_hip.so"])
def test_keep_mask_of_both_libraries_is_the_numpy_philox(lib):
    """hsmhd_keep_mask is host code in both libraries: called through ctypes alone, no object and no device.  Heads 1 ... 9 and 64 (counter
    word h >> 2 up to 15), seeds and offsets with both halves set, drop_p from 0 to just below 1."""
    l = ctypes.CDLL(os.path.join(LIBDIR, lib))
    l.hsmhd_keep_mask.argtypes = [ctypes.c_uint64, ctypes.c_uint32, ctypes.c_float, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p]
    for nnz, heads, p, seed, offset in ((1000, 1, 0.5, 1, 0), (1000, 3, 0.1, 0xDEADBEEFCAFEF00D, 5), (500, 4, 0.9, 7, (9 << 32) + 3), (400, 5, 0.5, 1 << 32, 1 << 32),
                                        (300, 9, 0.25, 0xFFFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFF), (200, 64, 0.5, 12345, 678), (100, 8, 0.0, 3, 4), (100, 8, 0.99999994, 3, 4), (0, 4, 0.5, 1, 1)):
        got = np.full((nnz, heads), 9, dtype=np.uint8)
        assert l.hsmhd_keep_mask(nnz, heads, p, seed, offset, got.ctypes.data if nnz else None) == 0
        assert np.array_equal(got, numpy_keep_mask(nnz, heads, p, seed, offset)), (lib, nnz, heads, p, seed, offset)
    assert l.hsmhd_keep_mask(10, 4, 1.0, 1, 1, got.ctypes.data) == -1 and l.hsmhd_keep_mask(10, 4, float("nan"), 1, 1, got.ctypes.data) == -1


@pytest.mark.parametrize("heads,d", SHAPES)
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_kept_share_is_binomial(heads, d, p):
    """over the general case's 4000 * heads draws the kept share lies within five binomial standard deviations of 1 - thr / 2^32"""
    hd = _cases()
    n = hd.NNZ * heads
    q = 1.0 - hd.threshold(p) / 2.0 ** 32
    kept = int(numpy_keep_mask(hd.NNZ, heads, p, 0x9E3779B97F4A7C15 + heads, (1 << 40) + d).sum())
    assert abs(kept - n * q) <= 5.0 * np.sqrt(n * q * (1.0 - q)), (kept, n * q)


# ---- the cases on the CPU twin ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("heads,d", SHAPES)
def test_general(heads, d):
    """300 x 517, 4000 entries, drop_p 0.1 and 0.5, a bias and NULL, both forms, tight and padded, lse and gbias taken and NULL"""
    print("\n".join(l for l in run_child(f"hd.general(mem, (({heads}, {d}),))").splitlines() if "backward worst" in l))


def test_drop_zero_gives_the_words_of_the_calls_without_dropout():
    run_child("hd.zero_drop(mem)")


def test_forward_and_backward_agree_on_the_mask():
    run_child("hd.mask_agreement(mem)")


def test_fully_dropped_rows():
    run_child("hd.fully_dropped_rows(mem)")


def test_long_rows_and_columns():
    """the host has no grid: 2000 rows and columns hold the long row and the long column"""
    run_child("hd.long_rows_and_columns(mem, 2000)")


def test_edges():
    run_child("hd.edges(mem)")


def test_seeds_and_offsets():
    run_child("hd.seeds_and_offsets(mem)")


def test_a_masking_bias_with_dropout():
    run_child("hd.mask_and_dropout(mem)")


def test_refusals():
    run_child("hd.refusals(mem)")


# ---- the references themselves ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("heads,d", [(3, 8), (4, 16), (5, 4)])
def test_drop_zero_anchors_the_references(heads, d):
    """No library involved.  With every weight 1.0 (drop_p = 0) the restated references' Y, LSE, GQ, GK, GV and GB equal the bias
    references' exactly in float64, and so do the bounds of lse, gQ, gK and gbias; the bound of gV may differ in the last place (w P is
    formed before rho multiplies it) and the bound of Y is the new, uncentred one: at least the summation term, at most 2 rho / (1 - rho) B
    above it."""
    hd = _cases()
    hb = hd.hb
    indptr, indices = hd.random_pattern(hd.ROWS, hd.COLS, hd.NNZ, 1)
    shape = (hd.ROWS, hd.COLS)
    Q, K, V, gY = hd.operands(shape, heads * d, 6100 + 1000 * heads + d)
    bias = hd.biases(hd.NNZ, heads, 6150)
    ones = hd.weights(np.ones((hd.NNZ, heads), dtype=np.uint8), 0.0)
    assert (ones == 1.0).all() and hd.threshold(0.0) == 0
    scores = hd.head_scores(indptr, indices, Q, K, heads)
    for scale in (0.125, -2.0):
        old_f, new_f = hb.forward_refs(scores, V, scale, bias), hd.forward_refs(scores, V, scale, bias, ones)
        lse = hd.rounded_forward(old_f)[1]
        old_b, new_b = hb.backward_refs(scores, V, gY, lse, scale, bias), hd.backward_refs(scores, V, gY, lse, scale, bias, ones)
        for o, n in zip(old_f, new_f):
            assert np.array_equal(o.Y, n.Y) and np.array_equal(o.LSE, n.LSE) and np.array_equal(o.finite, n.finite) and np.array_equal(o.P, n.P)
            assert np.array_equal(o.bound_lse, n.bound_lse) and np.array_equal(o.B, n.B)
            f = o.finite
            assert (n.bound_y[f] >= o.bound_y[f] - 2.0 ** -149).all(), "the uncentred bound is at least the centred one (|V - Y| sums to at most 2 B)"
        for o, n in zip(old_b, new_b):
            assert np.array_equal(o.GQ, n.GQ) and np.array_equal(o.GK, n.GK) and np.array_equal(o.GV, n.GV) and np.array_equal(o.GB, n.GB) and np.array_equal(o.D, n.D)
            for name in ("gq", "gk", "gv"):      # gam grows by 2^-52 |GP|: a bound never shrinks, and grows by less than one part in 2^20
                assert (n.bound[name] >= o.bound[name]).all() and (n.bound[name] <= (1.0 + 2.0 ** -20) * o.bound[name]).all(), name
            assert (n.bound_gb >= o.bound_gb).all() and (n.bound_gb <= (1.0 + 2.0 ** -20) * o.bound_gb).all()


def test_checker_rejects_planted_defects():
    """No library involved (the mask is the numpy Philox's): a correct result (the references' own words, rounded once) passes, and each
    of five defects planted in it is rejected every time: the mask of head h used for head h + 1, the mask indexed by the transposed
    entry index instead of the CSR index, c left out of gV, the row sum l taken over the kept entries only, the backward run at
    offset + 1."""
    hd = _cases()
    indptr, indices = hd.random_pattern(hd.ROWS, hd.COLS, hd.NNZ, 9)
    shape, heads, d, scale, p, seed, offset = (hd.ROWS, hd.COLS), 3, 8, 0.5, 0.5, 2024, 77
    Q, K, V, gY = hd.operands(shape, heads * d, 15000)
    bias = hd.biases(hd.NNZ, heads, 15010)
    scores = hd.head_scores(indptr, indices, Q, K, heads)
    keep = numpy_keep_mask(hd.NNZ, heads, p, seed, offset)
    W = hd.weights(keep, p)
    fwd = hd.forward_refs(scores, V, scale, bias, W)
    y, lse = hd.rounded_forward(fwd)
    assert hd.check_forward(fwd, y, lse, "a correct forward result") <= 1.0
    bwd = hd.backward_refs(scores, V, gY, lse, scale, bias, W)
    gq, gk, gv = hd.rounded_backward(bwd)
    gb = hd.rounded_gbias(bwd)
    assert max(hd.check_backward(bwd, gq, gk, gv, "a correct backward result").values()) <= 1.0 and hd.check_gbias(bwd, gb, "a correct gbias") <= 1.0

    def rejected(wrong_W, what, forward=True, outputs=("gq", "gk", "gv", "gbias")):
        if forward:
            with pytest.raises(AssertionError, match="words of y break"):
                hd.check_forward(fwd, hd.rounded_forward(hd.forward_refs(scores, V, scale, bias, wrong_W))[0], None, what)
        wrong = hd.backward_refs(scores, V, gY, lse, scale, bias, wrong_W)
        wq, wk, wv = hd.rounded_backward(wrong)
        for name, args in (("gq", (wq, gk, gv)), ("gk", (gq, wk, gv)), ("gv", (gq, gk, wv))):
            if name in outputs:
                with pytest.raises(AssertionError, match=f"words of {name} break"):
                    hd.check_backward(bwd, *args, what)
        if "gbias" in outputs:
            with pytest.raises(AssertionError, match="words of gbias break"):
                hd.check_gbias(bwd, hd.rounded_gbias(wrong), what)

    # the mask of head h used for head h + 1
    rejected(np.ascontiguousarray(np.roll(W, 1, axis=1)), "another head's mask")
    # the column side indexes the mask by the transposed entry index: the entry with CSR index perm[e'] is given W[e'].  gQ and D come
    # from the row side and stay right; gK, gV and gbias come from the column side (taken here from references built with the displaced
    # mask throughout)
    perm = bwd[0].perm
    by_column = np.empty_like(W)
    by_column[perm] = W
    wrong = hd.backward_refs(scores, V, gY, lse, scale, bias, by_column)
    _, wk, wv = hd.rounded_backward(wrong)
    with pytest.raises(AssertionError, match="words of gk break"):
        hd.check_backward(bwd, gq, wk, gv, "the mask by the transposed index")
    with pytest.raises(AssertionError, match="words of gv break"):
        hd.check_backward(bwd, gq, gk, wv, "the mask by the transposed index")
    with pytest.raises(AssertionError, match="words of gbias break"):
        hd.check_gbias(bwd, hd.rounded_gbias(wrong), "the mask by the transposed index")
    # c left out of gV: sum keep P gY
    c = hd.scale_c(p)
    no_c = hd.rounded_backward(bwd, [(r.GQ, r.GK, r.GV / c) for r in bwd])[2]
    with pytest.raises(AssertionError, match="words of gv break"):
        hd.check_backward(bwd, gq, gk, no_c, "c left out of gV")
    # the row sum l over the kept entries only: Y = sum keep c P V / sum keep P, lse = LSE + log(sum keep P)
    ys, ls = [], []
    for h, r in enumerate(fwd):
        share = hd.ac._seg_sum(((keep[:, h] != 0) * r.P)[:, None], r.scores.indptr)[:, 0]
        ok = share > 0
        ys.append(np.where(ok[:, None], r.Y / np.where(ok, share, 1.0)[:, None], 0.0).astype(np.float32))
        ls.append(np.where(ok, r.LSE + np.log(np.where(ok, share, 1.0)), -np.inf).astype(np.float32))
    with pytest.raises(AssertionError, match="words of y break"):
        hd.check_forward(fwd, np.concatenate(ys, axis=1), None, "l over the kept entries")
    with pytest.raises(AssertionError):
        hd.check_forward(fwd, y, np.stack(ls, axis=1), "l over the kept entries")
    # the backward run at offset + 1
    rejected(hd.weights(numpy_keep_mask(hd.NNZ, heads, p, seed, offset + 1), p), "the backward at offset + 1", forward=False)


def test_cpu_twin_against_autograd():
    """40 x 50, about 600 entries (no pair twice: a dense mask holds a pair once), 3 heads of d = 8, drop_p = 0.3: hsmhd_backward on the
    CPU twin, with lse from hsmhd_forward on the CPU twin, against torch float64 autograd of
        Y_h = (M_h c softmax(scale Q_h K_h^T + B_h + mask)) V_h
    with M_h the dense keep matrix of head h from the numpy Philox, and the loss sum(gY * Y), g_bias included.  This guards the formulas
    and the layouts themselves, which the references share with the code.

    It is tests/test_heads_bias_cpu.py's comparison with its tolerance.  The operands and the bias are multiples of 1/8 below 4 and scale
    is 1/8, so every fp32 product and t itself are exact; what is left between the contract's function and autograd's is lse,
    P'_e = f_r P_e with f_r = exp(LSE_r - lse_r) and k_r = expm1(bound_lse_r), so (GP and D taken with the weights w)
        |GB'_e - GB_e| <= P'_e (k_r |GP_e| + k_r (2 + k_r) |D'_r|),   |GS'_e - GS_e| <= |scale| times that,   |w P'_e - w P_e| <= k_r w P'_e
    summed over a word's entries times |K_ej|, |Q_ej| or |gY_ej| and added to the contract's bound."""
    import tempfile

    import torch
    body = """
import wide_cases as wc
rng = np.random.default_rng(15100)
rows, cols, H, d, scale, p, seed, offset = 40, 50, 3, 8, 0.125, 0.3, 99, (5 << 32) + 1
flat = np.sort(rng.choice(rows * cols, 600, replace=False))
indptr = np.zeros(rows + 1, dtype=np.uint32); indptr[1:] = np.cumsum(np.bincount(flat // cols, minlength=rows))
indices = (flat % cols).astype(np.uint32)
Q, gY = (wc.grid_values(rng, (rows, H * d)) for _ in range(2)); K, V = (wc.grid_values(rng, (cols, H * d)) for _ in range(2))
bias = wc.grid_values(rng, (600, H))
with heads_dropout.DropoutMultiHeadAttention((indptr, indices, (rows, cols)), H) as mh:
    y, lse = mh.forward(Q, K, V, bias, H, scale, p, seed, offset)
    gq, gk, gv, gb = mh.backward(Q, K, V, gY, lse, bias, H, scale, p, seed, offset)
np.savez(PATH, indptr=indptr, indices=indices, Q=Q, K=K, V=V, gY=gY, bias=bias, y=y, lse=lse, gq=gq, gk=gk, gv=gv, gb=gb)
"""
    hd = _cases()
    ac = hd.ac
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "twin.npz")
        run_child(body.replace("PATH", repr(path)))
        z = dict(np.load(path))
    indptr, indices, Q, K, V, gY, bias, lse = (z[k] for k in ("indptr", "indices", "Q", "K", "V", "gY", "bias", "lse"))
    rows, cols, H, d, scale, p, seed, offset = 40, 50, 3, 8, 0.125, 0.3, 99, (5 << 32) + 1
    assert (np.diff(indptr.astype(np.int64)) > 0).all() and lse.shape == (rows, H) and z["gb"].shape == (600, H)
    keep = numpy_keep_mask(600, H, p, seed, offset)
    assert 0.55 < keep.mean() < 0.85
    W = hd.weights(keep, p)
    scores = hd.head_scores(indptr, indices, Q, K, H)
    fwd = hd.forward_refs(scores, V, scale, bias, W)
    bwd = hd.backward_refs(scores, V, gY, lse, scale, bias, W)
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
        assert (np.abs(f.Y - hd.cut(auto_y, h, d)) <= 2.0 ** -40 * (1.0 + np.abs(f.Y))).all(), f"the forward formula, head {h}"
        k = np.expm1(f.bound_lse)[of]
        d_gb = r.P * (k * np.abs(r.GP) + k * (2.0 + k) * np.abs(r.D[of]))
        d_gs = abs(r.sc) * d_gb
        d_p = k * r.PW
        pm = r.perm
        extra = {"gq": ac._seg_sum(d_gs[:, None] * np.abs(r.K64), s.indptr), "gk": ac._seg_sum((d_gs[:, None] * np.abs(r.Q64))[pm], r.cptr),
                 "gv": ac._seg_sum((d_p[:, None] * np.abs(r.G64))[pm], r.cptr)}
        mine = {"gq": r.GQ, "gk": r.GK, "gv": r.GV}
        r.want = {name: hd.cut(a, h, d) for name, a in zip(hd.bc.OUTPUTS, auto)}
        worst = r.check(*(hd.cut(z[name], h, d) for name in hd.bc.OUTPUTS), f"the CPU twin against autograd, head {h}", extra=extra)
        assert max(worst.values()) <= 1.0
        for name in hd.bc.OUTPUTS:      # the formula alone: the reference's own float64 gradients against autograd's
            assert (np.abs(mine[name] - r.want[name]) <= extra[name] + 2.0 ** -40 * (1.0 + np.abs(mine[name]))).all(), (name, h)
        assert r.check_gbias(np.ascontiguousarray(z["gb"][:, h]), f"the CPU twin's gbias against autograd, head {h}", extra=d_gb, want=auto_gb[:, h]) <= 1.0
        assert (np.abs(r.GB - auto_gb[:, h]) <= d_gb + 2.0 ** -40 * (1.0 + np.abs(r.GB))).all(), f"the formula of gbias, head {h}"
        assert (auto_gb[keep[:, h] == 0, h] != 0).any(), "a dropped entry's gbias is -P D"
    hd.check_forward(fwd, z["y"], lse, "the CPU twin's forward")


# ---- names, sources, the sanitizers ------------------------------------------------------------------------------------------------------
def test_header_libraries_and_binding_agree():
    """exactly five hsmhd_* functions in the header, in both libraries and in the binding's EXPORTS, apart from every other module's
    names; the header includes hisparse_heads.h and hisparse_hip.h names it in its comment only"""
    from hisparse_amd import attention, attention_backward, device, heads, heads16, heads_bias, heads_dropout, pattern, rows, wide
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hisparse_heads_dropout.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\bhsmhd_[a-z0-9_]+\b", header))) == NAMES
    assert sorted(set(re.findall(r"\b(hsmhd_[a-z0-9_]+)\s*\(", header))) == NAMES and len(NAMES) == 5 and '#include "hisparse_heads.h"' in header
    assert set(re.findall(r"\bhsmh_[a-z0-9_]+\b", header)) == {"hsmh_pattern"} and not re.search(r"\bhsmhb_", header)      # no new create, no new type
    assert sorted(heads_dropout.EXPORTS) == NAMES
    others = set(device.EXPORTS) | set(pattern.EXPORTS) | set(rows.EXPORTS) | set(wide.EXPORTS) | set(attention.EXPORTS) | set(attention_backward.EXPORTS) | set(heads.EXPORTS) \
        | set(heads16.EXPORTS) | set(heads_bias.EXPORTS)
    assert not set(NAMES) & others
    for lib in ("libhisparse_hip.so", "libhisparse_cpu.so"):
        exported = subprocess.run(["nm", "-D", "--defined-only", os.path.join(LIBDIR, lib)], capture_output=True, text=True, check=True).stdout
        assert sorted(set(re.findall(r"\b(hsmhd_[a-z0-9_]+)\b", exported))) == NAMES, lib
        l = ctypes.CDLL(os.path.join(LIBDIR, lib))
        for n in NAMES:
            assert hasattr(l, n), (lib, n)
    bound = heads_dropout.lib()
    for n in NAMES:
        assert getattr(bound, n).argtypes is not None, n
    assert bound is heads.lib() and issubclass(heads_dropout.DropoutMultiHeadAttention, heads_bias.BiasedMultiHeadAttention)
    for method in ("forward", "backward", "forward_device", "backward_device", "keep_mask"):
        assert method in vars(heads_dropout.DropoutMultiHeadAttention), method
    import hisparse_amd
    assert hisparse_amd.heads_dropout is heads_dropout and "heads_dropout" in hisparse_amd.__all__
    hip_h = open(os.path.join(ROOT, "include", "hisparse_hip.h")).read()
    assert "hisparse_heads_dropout.h" in hip_h and not re.search(r"\bhsmhd_[a-z_]+\s*\(", re.sub(r"/\*.*?\*/", "", hip_h, flags=re.S))


def test_schedule_is_the_wide_products_unchanged():
    """heads_dropout_attention.{h,hip} add no kWide* constant, the launchers take the classes, teams and grid cap from wide_products.h at
    the width heads * d, the file holds exactly the three kernels under names the other kernel counts do not match, without inline
    assembly or atomics; philox.h holds none either and is plain integer code for host and device"""
    csrc = os.path.join(ROOT, "hisparse_amd", "csrc")
    text = open(os.path.join(csrc, "heads_dropout_attention.h")).read()
    assert '#include "wide_products.h"' in text and '#include "philox.h"' in text and not re.search(r"constexpr\s+\w+\s+kWide", text)
    hip = open(os.path.join(csrc, "heads_dropout_attention.hip")).read()
    code = re.sub(r"//[^\n]*", "", hip)
    assert not re.search(r"constexpr\s+\w+\s+kWide", hip) and "asm" not in code and "atomic" not in code
    for name in ("wide_table(s.count, heads * d)", "wide_group_lanes(heads * d)", "kWideBlocksPerCu", "kWideInFlight", "kWideThreads", "__builtin_nontemporal_load(perm + ei)",
                 "__fadd_rn(", "__fmul_rn(", "philox::keep(", "__ballot("):
        assert name in hip, name
    kernels = re.findall(r"__global__[^\n]*?\bvoid\s+(\w+)\s*\(", hip)
    assert sorted(kernels) == ["dropout_attention_cols_kernel", "dropout_attention_forward_kernel", "dropout_attention_rows_kernel"]
    for k in kernels:
        assert not any(old in k for old in ("biased_attention_", "heads_forward", "heads_backward", "heads16_"))
    philox = re.sub(r"//[^\n]*", "", open(os.path.join(csrc, "philox.h")).read())
    assert "asm" not in philox and "atomic" not in philox
    for word in ("0xD2511F53", "0xCD9E8D57", "0x9E3779B9", "0xBB67AE85", "kRounds = 10"):
        assert word in philox, word
    for old in ("heads_attention.hip", "heads16_attention.hip", "heads_bias_attention.hip"):
        assert "philox" not in open(os.path.join(csrc, old)).read(), old


def test_cpu_twin_stand_alone_under_the_sanitizers(tmp_path):
    """tests/cpp/test_heads_dropout_cpu.cpp: the edge patterns and the refusals through the C boundary, compiled together with
    hsmh_cpu.cpp under -fsanitize=address,undefined with the runtimes linked in statically (a program of its own: nothing loaded into
    python is run under a sanitizer)."""
    exe = tmp_path / "heads_dropout_cpu"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", f"-I{ROOT}/include", f"-I{ROOT}/hisparse_amd/csrc", f"{ROOT}/tests/cpp/test_heads_dropout_cpu.cpp",
                           f"{ROOT}/hisparse_amd/csrc/hsmh_cpu.cpp", "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "HEADS DROPOUT CPU OK" in out.stdout, out.stdout + out.stderr

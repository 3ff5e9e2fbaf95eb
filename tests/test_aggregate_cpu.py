"""The neighbour aggregation (include/hisparse_aggregate.h) without a GPU: the cases of tests/aggregate_cases.py on libhisparse_cpu.so, each
in a child process with HISPARSE_HIP_LIB set (as tests/test_wide_cpu.py runs its cases); the reference's two statements of the winner
rule against each other, and the checker against planted defects; header, libraries and binding in agreement on exactly four functions;
the kernels' source on the unchanged schedule; the CPU twin's source under the sanitizers as a stand-alone program.  The same cases on the
device: tests/test_gpu_aggregate.py."""
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
from hisparse_amd import device, wide, aggregate
import aggregate_cases as ac
assert device._LIB_PATH.endswith("libhisparse_cpu.so")
mem = ac.HostMemory()
%(body)s
print("aggregate child ok")
"""

NAMES = ["hsagg_backward", "hsagg_backward_device", "hsagg_forward", "hsagg_forward_device"]


def run_child(body):
    if not os.path.exists(CPU_LIB):
        subprocess.check_call(["make", "-C", ROOT, "cpu"], stdout=subprocess.DEVNULL)
    env = dict(os.environ, HISPARSE_HIP_LIB=CPU_LIB)
    for k in [k for k in env if k.startswith("HISPARSE_") and k != "HISPARSE_HIP_LIB"]:
        env.pop(k)
    r = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests"), "body": body}], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "aggregate child ok" in r.stdout, r.stdout[-4000:] + r.stderr[-4000:]
    return r.stdout


def _cases():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import aggregate_cases as ac
    return ac


DS = _cases().DS


@pytest.mark.parametrize("d", DS)
def test_general(d):
    """300 x 517, 4000 entries, every legal ops word, pad 0 and 8, args taken and NULL, both forms, forward then backward with the args just
    written"""
    run_child(f"ac.general(mem, ({d},))")


def test_winner_positions():
    run_child("ac.winner_positions(mem)")


def test_ties():
    run_child("ac.ties(mem)")


def test_non_finite_values():
    run_child("ac.non_finite(mem)")


def test_edges():
    run_child("ac.edges(mem)")


def test_backward_identities():
    run_child("ac.backward_identities(mem)")


def test_a_call_leaves_nothing_for_the_next():
    run_child("ac.nothing_carried_over(mem)")


def test_refusals():
    run_child("ac.refusals(mem)")


def _tricky_words(rng, n):
    """n float32 words with many ties, zeros of both signs, infinities and NaNs of several payloads"""
    pool = np.array([0.0, -0.0, 1.0, 1.0, -1.0, 2.5, -2.5, np.inf, -np.inf, np.nan], dtype=np.float32)
    w = pool[rng.integers(0, pool.size, n)].copy()
    bits = w.view(np.uint32)
    nan = np.isnan(w)
    bits[nan] |= rng.integers(0, 1 << 22, int(nan.sum())).astype(np.uint32) | (rng.integers(0, 2, int(nan.sum())).astype(np.uint32) << 31)
    return w


def test_reference_is_the_definition():
    """No library involved: the segment-reduction reference (rank, then the smallest index) names, for rows of tricky words, the winner
    that the entry-by-entry statement of the header's rule names; and a few fixed rows by hand."""
    ac = _cases()
    rng = np.random.default_rng(15000)
    lengths = np.array([0, 1, 2, 3, 7, 0, 33, 200, 1], dtype=np.int64)
    indptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint32)
    for keep_nan in (True, False):
        G = _tricky_words(rng, int(lengths.sum()) * 6).reshape(-1, 6)
        if not keep_nan:
            G[np.isnan(G)] = np.float32(-0.0)
        for is_max in (True, False):
            args, vals = ac.winners(indptr, G, is_max)
            for r, n in enumerate(lengths):
                for j in range(6):
                    if n == 0:
                        assert args[r, j] == ac.NONE and vals[r, j] == 0
                        continue
                    k = ac.winner_by_loop(G[indptr[r]: indptr[r + 1], j], is_max)
                    assert args[r, j] == indptr[r] + k and vals[r, j] == G.view(np.uint32)[indptr[r] + k, j], (r, j, is_max)
    nan = np.float32(np.nan)
    for words, want_max, want_min in (([1.0, 3.0, 3.0, -2.0, -2.0], 1, 3), ([-0.0, 0.0, -0.0], 0, 0), ([0.0, -0.0], 0, 0), ([5.0, nan, 7.0, nan], 1, 1), ([np.inf, nan], 1, 1),
                                      ([-np.inf, np.inf, np.inf, -np.inf], 1, 0), ([2.0], 0, 0)):
        w = np.array(words, dtype=np.float32)
        ip = np.array([0, w.size], dtype=np.uint32)
        assert ac.winners(ip, w[:, None], True)[0][0, 0] == want_max == ac.winner_by_loop(w, True), words
        assert ac.winners(ip, w[:, None], False)[0][0, 0] == want_min == ac.winner_by_loop(w, False), words


def test_checker_rejects_planted_defects():
    """No library involved: the reference's own results pass, and each planted defect is rejected -- a maximum that drops NaNs as fmaxf
    does, the LARGEST index among equals, -0.0 ranked below +0.0, a sum that is 2 ulp off, an empty row that is -0.0, a backward that
    spreads the gradient over every entry that ties with the winner."""
    ac = _cases()
    rng = np.random.default_rng(15100)
    lengths = np.array([0, 1, 4, 9, 40, 0, 300], dtype=np.int64)
    indptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint32)
    cols, d = 20, 6
    indices = rng.integers(0, cols, int(lengths.sum())).astype(np.uint32)
    X = _tricky_words(rng, cols * d).reshape(cols, d)
    X[:, 5] = rng.normal(0.0, 1.0, cols).astype(np.float32)      # one feature of ordinary numbers, for the sums
    ops = ac.MEAN | ac.MAX | ac.MIN
    ref = ac.ForwardRef(indptr, indices, X)
    amax, vmax = ref.part("max")
    amin, vmin = ref.part("min")
    mean = ref.part("mean")
    with np.errstate(all="ignore"):
        good = {"sum": mean.ieee.astype(np.float32), "max": vmax.view(np.float32), "amax": amax, "min": vmin.view(np.float32), "amin": amin}
    good["sum"][mean.finite] = mean.E[mean.finite].astype(np.float32)
    ref.check(good, ops, "the reference's own words")
    G = X[indices]
    live = lengths > 0
    starts = indptr[:-1][live]
    # fmaxf: NaNs dropped
    with np.errstate(all="ignore"):
        dropped = np.fmax.reduceat(G, starts, axis=0)
    bad = dict(good, max=good["max"].copy())
    bad["max"][live] = dropped
    assert np.isnan(good["max"]).any()
    with pytest.raises(AssertionError, match="words of ymax are not the winner's word"):
        ref.check(bad, ops, "NaNs dropped")
    # the largest index among equals
    last = amax.copy()
    for r in np.nonzero(live)[0]:
        for j in range(d):
            seg = ac.rank_of(G[indptr[r]: indptr[r + 1], j], True)
            last[r, j] = indptr[r] + np.nonzero(seg == seg.max())[0][-1]
    assert (last != amax).any()
    with pytest.raises(AssertionError, match="words of amax differ"):
        ref.check(dict(good, amax=last), ops, "the largest index among equals")
    # -0.0 ranked below +0.0: the minimum of a row of zeros becomes the first -0.0, not the first zero
    Z = np.array([[0.0], [-0.0], [0.0]], dtype=np.float32)
    zref = ac.ForwardRef(np.array([0, 3], dtype=np.uint32), np.arange(3, dtype=np.uint32), Z)
    zref.check({"min": np.array([[0.0]], dtype=np.float32), "amin": np.array([[0]], dtype=np.uint32)}, ac.MIN, "zeros")
    with pytest.raises(AssertionError, match="ymin are not the winner's word"):
        zref.check({"min": np.array([[-0.0]], dtype=np.float32), "amin": np.array([[1]], dtype=np.uint32)}, ac.MIN, "-0.0 below +0.0")
    # a sum 2 ulp off
    off = good["sum"].copy()
    r = 6
    assert mean.finite[r, 5] and off[r, 5] != 0
    off[r, 5] = np.nextafter(np.nextafter(off[r, 5], np.float32(np.inf)), np.float32(np.inf))
    with pytest.raises(AssertionError, match="break the float contract"):
        ref.check(dict(good, sum=off), ops, "2 ulp off")
    # an empty row written as -0.0
    neg = good["sum"].copy()
    neg[0] = -0.0
    with pytest.raises(AssertionError, match="an empty row is not"):
        ref.check(dict(good, sum=neg), ops, "an empty row is -0.0")
    # the backward: the gradient of the maximum given to every entry that ties with the winner
    shape = (lengths.size, cols)
    g = ac.gradients(ac.MAX, lengths.size, d, 15110, good)
    g["gmax"][:] = np.abs(g["gmax"]) + 1.0
    bref = ac.BackwardRef(shape, indptr, indices, ac.MAX, g)
    with np.errstate(all="ignore"):
        bref.check(bref.E.astype(np.float32), "the reference's own words")
    rows = ac.entry_rows(indptr)
    ties_too = ac.rank_of(G, True) == ac.rank_of(vmax.view(np.float32), True)[rows]
    spread = np.zeros((cols, d), dtype=np.float64)
    np.add.at(spread, indices, np.where(ties_too, g["gmax"][rows].astype(np.float64), 0.0))
    assert ties_too.sum() > live.sum() * d
    with pytest.raises(AssertionError, match="break the float contract"):
        bref.check(spread.astype(np.float32), "the gradient spread over ties")


def test_header_libraries_and_binding_agree():
    """exactly four hsagg_* functions in the header, in both libraries and in the binding's EXPORTS, apart from every other object's names;
    none of them begins with hsw_ (tests/test_wide_cpu.py pins those twelve); the header includes hisparse_wide.h"""
    from hisparse_amd import aggregate, attention, attention_backward, device, gat, gatv2, heads, heads16, heads16_dropout, heads_bias, heads_dropout, pattern, rows, wide
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hisparse_aggregate.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\bhsagg_[a-z0-9_]+\b", header))) == NAMES
    assert sorted(set(re.findall(r"\b(hsagg_[a-z0-9_]+)\s*\(", header))) == NAMES and len(NAMES) == 4 and '#include "hisparse_wide.h"' in header
    assert set(re.findall(r"\bhsw_[a-z0-9_]+\b", header)) == {"hsw_pattern"}      # the existing object's type and nothing else of it
    values = dict(re.findall(r"#define (HSAGG_[A-Z]+) (\w+)", header))
    assert values == {"HSAGG_SUM": "1u", "HSAGG_MEAN": "2u", "HSAGG_MAX": "4u", "HSAGG_MIN": "8u", "HSAGG_NONE": "0xFFFFFFFFu"}
    assert (aggregate.SUM, aggregate.MEAN, aggregate.MAX, aggregate.MIN, aggregate.NONE) == (1, 2, 4, 8, 0xFFFFFFFF) and len(aggregate.LEGAL_OPS) == 11
    assert sorted(aggregate.EXPORTS) == NAMES
    others = set()
    for m in (attention, attention_backward, device, gat, gatv2, heads, heads16, heads16_dropout, heads_bias, heads_dropout, pattern, rows, wide):
        others |= set(m.EXPORTS)
    assert not set(NAMES) & others and not any(n.startswith("hsw_") for n in NAMES)
    for lib in ("libhisparse_hip.so", "libhisparse_cpu.so"):
        exported = subprocess.run(["nm", "-D", "--defined-only", os.path.join(LIBDIR, lib)], capture_output=True, text=True, check=True).stdout
        assert sorted(set(re.findall(r"\b(hsagg_[a-z0-9_]+)\b", exported))) == NAMES, lib
        l = ctypes.CDLL(os.path.join(LIBDIR, lib))
        for n in NAMES:
            assert hasattr(l, n), (lib, n)
    bound = aggregate.lib()
    for n in NAMES:
        assert getattr(bound, n).argtypes is not None, n
    assert bound is wide.lib() and issubclass(aggregate.NeighborAggregate, wide.WideProducts)
    import hisparse_amd
    assert hisparse_amd.aggregate is aggregate and "aggregate" in hisparse_amd.__all__
    hip_h = open(os.path.join(ROOT, "include", "hisparse_hip.h")).read()
    assert "hisparse_aggregate.h" in hip_h and not re.search(r"\bhsagg_[a-z_]+\s*\(", re.sub(r"/\*.*?\*/", "", hip_h, flags=re.S))


def test_schedule_is_the_wide_products_unchanged():
    """neighbor_aggregate.{h,hip} add no kWide* constant, the launchers take the classes, teams and grid cap from wide_products.h at the
    width d, the file holds exactly the two kernel templates under names the other kernel counts do not match, without inline assembly,
    atomics or the matrix engine, and the (value, index) merge is wide_lanes.h's, which compares explicitly"""
    text = open(os.path.join(ROOT, "hisparse_amd", "csrc", "neighbor_aggregate.h")).read()
    assert '#include "wide_products.h"' in text and not re.search(r"constexpr\s+\w+\s+kWide", text)
    hip = open(os.path.join(ROOT, "hisparse_amd", "csrc", "neighbor_aggregate.hip")).read()
    code = re.sub(r"//[^\n]*", "", hip)
    assert not re.search(r"constexpr\s+\w+\s+kWide", hip) and "asm" not in code and "atomic" not in code and "mfma" not in code
    assert "fmaxf" not in code and "fminf" not in code and "fmax(" not in code and "fmin(" not in code
    for name in ("wide_table(s.count, d)", "wide_group_lanes(d)", "kWideBlocksPerCu", "kWideInFlight", "kWideThreads", "pick(tab, w, ptr, list, group)", "trips_of(wk)",
                 "grid_of(s, t, kWideBlocksPerCu)", "merge_lanes(", "merge_waves(", "merge_best_lanes<", "merge_best_waves<", '#include "wide_lanes.h"'):
        assert name in hip, name
    kernels = re.findall(r"__global__[^\n]*?\bvoid\s+(\w+)\s*\(", hip)
    assert sorted(kernels) == ["neighbor_backward_kernel", "neighbor_forward_kernel"]
    for k in kernels:
        assert not any(old in k for old in ("wide_dot_kernel", "wide_gather_kernel", "gat_", "gatv2_", "heads_forward", "heads_backward", "attention_backward_", "pattern_attention",
                                            "heads16_", "biased_attention_", "dropout_attention_", "bf16_drop_", "row_softmax"))
    lanes = open(os.path.join(ROOT, "hisparse_amd", "csrc", "wide_lanes.h")).read()
    body = lanes[lanes.index("bool outranks("):]
    body = re.sub(r"//[^\n]*", "", body[: body.index("}")])
    assert "v != v" in body and "e < be" in body and "fmax" not in body and "fmin" not in body


def test_cpu_twin_stand_alone_under_the_sanitizers(tmp_path):
    """tests/cpp/test_aggregate_cpu.cpp: the edge patterns and the refusals through the C boundary, compiled together with hsw_cpu.cpp under
    -fsanitize=address,undefined with the runtimes linked in statically (a program of its own: nothing loaded into python is run under
    a sanitizer)."""
    exe = tmp_path / "aggregate_cpu"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", f"-I{ROOT}/include", f"-I{ROOT}/hisparse_amd/csrc", f"{ROOT}/tests/cpp/test_aggregate_cpu.cpp", f"{ROOT}/hisparse_amd/csrc/hsw_cpu.cpp",
                           "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "AGGREGATE CPU OK" in out.stdout, out.stdout + out.stderr

"""The cases of the sampled dense product (include/hisparse_pattern.h), shared by tests/test_pattern_cpu.py (libhisparse_cpu.so, in a
child process) and tests/test_gpu_pattern.py (the HIP library, on the device): numpy references stated from the header's ARITHMETIC
block, pattern builders, and the general / edge / refusal cases written against a small memory interface (host arrays or memory of the HIP runtime).

References.  Fixed point: q_mul = min((a b + 2^23) >> 24, 2^32 - 1) per product, the sum (and, with accumulate, the old word) clamped
once at 2^32 - 1 -- bit exact.  Float: p = the fp32 products (numpy float32), E = math.fsum(p) per entry, A = sum |p|, and
|out - E| <= u |E| + k 2^-52 A + 2^-149 for one call, gamma(S) A + k 2^-52 A + S 2^-149 for S accumulated calls (U and gamma from
tests/float_contract.py); non-finite entries follow the IEEE double sum of p in ascending j.  float_exact() is that double sum itself,
rounded once: the words the header promises for one call."""
import ctypes as C
import math

import numpy as np

from hisparse_amd import host, pattern

import float_contract as fc

SAT = 0xFFFFFFFF
BAD_ARG, BAD_MATRIX = -1, -4
KS = (1, 3, 4, 5, 16, 17, 64)


# ---- memory ------------------------------------------------------------------------------------------------------------------------
class Buf:
    def __init__(self, ptr, keep, n):
        self.ptr, self.keep, self.n = ptr, keep, n


class HostMemory:
    """libhisparse_cpu.so: "device" pointers are host pointers (16-byte aligned numpy storage)"""
    def alloc(self, words):
        words = np.ascontiguousarray(words, dtype=np.uint32).ravel()
        raw = np.zeros(words.size + 8, dtype=np.uint32)
        off = (-raw.ctypes.data % 16) // 4
        view = raw[off: off + max(words.size, 1)]
        view[: words.size] = words
        return Buf(view.ctypes.data, (raw, view), words.size)

    def read(self, sp, buf):
        sp.sync()
        return buf.keep[1][: buf.n].copy()


class _HipBlock:
    def __init__(self, rt, nbytes):
        self.rt, self.ptr = rt, C.c_void_p()
        assert rt.hipMalloc(C.byref(self.ptr), nbytes) == 0

    def __del__(self):
        if self.ptr:
            self.rt.hipFree(self.ptr)


class HipMemory:
    """the HIP library: device memory from the HIP runtime the library itself uses"""
    def __init__(self):
        rt = self.rt = C.CDLL("libamdhip64.so")
        rt.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        rt.hipFree.argtypes = [C.c_void_p]
        rt.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        rt.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
        rt.hipStreamSynchronize.argtypes = [C.c_void_p]
        rt.hipStreamDestroy.argtypes = [C.c_void_p]

    def alloc(self, words):
        words = np.ascontiguousarray(words, dtype=np.uint32).ravel()
        block = _HipBlock(self.rt, max(words.size, 4) * 4)
        assert block.ptr.value % 16 == 0
        if words.size:
            assert self.rt.hipMemcpy(block.ptr, words.ctypes.data, words.nbytes, 1) == 0
        return Buf(block.ptr.value, block, words.size)

    def fetch(self, buf):
        """the buffer's words, after whatever the caller synchronised"""
        out = np.empty(buf.n, dtype=np.uint32)
        if buf.n:
            assert self.rt.hipMemcpy(out.ctypes.data, C.c_void_p(buf.ptr), out.nbytes, 2) == 0
        return out

    def read(self, sp, buf):
        sp.sync()
        return self.fetch(buf)

    def stream(self):
        st = C.c_void_p()
        assert self.rt.hipStreamCreate(C.byref(st)) == 0
        return st


# ---- references --------------------------------------------------------------------------------------------------------------------
def q_mul(a, b):
    p = (np.asarray(a, dtype=np.uint64) * np.asarray(b, dtype=np.uint64) + np.uint64(1 << 23)) >> np.uint64(24)
    return np.minimum(p, np.uint64(SAT))


def entry_rows(indptr):
    return np.repeat(np.arange(len(indptr) - 1, dtype=np.int64), np.diff(np.asarray(indptr, dtype=np.int64)))


def fixed_ref(indptr, indices, U, V, old=None):
    r, c = entry_rows(indptr), np.asarray(indices, dtype=np.int64)
    s = np.zeros(r.size, dtype=np.uint64)
    for j in range(U.shape[0]):
        s += q_mul(U[j, r], V[j, c])                       # at most 64 terms below 2^32: no wrap
    if old is not None:
        s += np.asarray(old, dtype=np.uint64)
    return np.minimum(s, np.uint64(SAT)).astype(np.uint32)


def float_products(indptr, indices, U, V):
    r, c = entry_rows(indptr), np.asarray(indices, dtype=np.int64)
    with np.errstate(all="ignore"):
        return U.view(np.float32)[:, r] * V.view(np.float32)[:, c]           # (k, nnz) float32


def float_exact(p):
    """the header's sum: doubles from +0.0 in ascending j, rounded once"""
    acc = np.zeros(p.shape[1], dtype=np.float64)
    with np.errstate(all="ignore"):
        for j in range(p.shape[0]):
            acc = acc + p[j].astype(np.float64)
        return acc.astype(np.float32)


def same_floats(got_words, want):
    """equal as fp32 values: NaN where NaN, +-0 alike (the sign of a zero result is not promised)"""
    got = np.asarray(got_words, dtype=np.uint32).view(np.float32)
    return got.shape == want.shape and bool(np.all((got == want) | (np.isnan(got) & np.isnan(want))))


def float_check(out_words, p, calls=1, what=""):
    out = np.asarray(out_words, dtype=np.uint32).view(np.float32).astype(np.float64)
    assert out.size == p.shape[1], (what, out.size, p.shape)
    p64 = p.astype(np.float64)
    k = p.shape[0]
    finite = np.isfinite(p64).all(axis=0)
    A = np.abs(np.where(finite, p64, 0.0)).sum(axis=0)
    E = np.array([math.fsum(p64[:, e]) if finite[e] else 0.0 for e in range(p.shape[1])])
    if calls <= 1:
        bound = fc.U * np.abs(E) + k * 2.0 ** -52 * A + 2.0 ** -149
    else:
        bound = fc.gamma(calls) * A + k * 2.0 ** -52 * A + calls * 2.0 ** -149
    bad = finite & ~(np.isfinite(out) & (np.abs(out - E) <= bound))
    ieee = float_exact(p).astype(np.float64)
    with np.errstate(invalid="ignore"):
        bad |= ~finite & ~((out == ieee) | (np.isnan(out) & np.isnan(ieee)))
    if bad.any():
        e = int(np.nonzero(bad)[0][0])
        raise AssertionError(f"{what}: {int(bad.sum())} entries break the float contract, first {e}: out={out[e]!r} E={E[e]!r} bound={bound[e]:.3g} k={k} calls={calls}")


# ---- inputs --------------------------------------------------------------------------------------------------------------------------
def random_pattern(rows, cols, nnz, seed):
    """uniform random entries (a pair drawn twice is two entries), rows ascending, columns ascending inside a row"""
    rng = np.random.default_rng(seed)
    flat = np.sort(rng.integers(0, rows * cols, nnz, dtype=np.int64))
    indptr = np.zeros(rows + 1, dtype=np.uint32)
    indptr[1:] = np.cumsum(np.bincount(flat // cols, minlength=rows))
    return indptr, (flat % cols).astype(np.uint32)


def vectors(impl, k, n, seed, scale=1.0):
    """(k, n) value words: fixed point uniform in [0, 2 scale), float normal"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.0, 2.0 * scale, (k, n)) if impl == 0 else rng.normal(0.0, scale, (k, n))
    return np.stack([host.pack_vector(impl, row.astype(np.float32)) for row in x]).astype(np.uint32)


def check(impl, got, indptr, indices, U, V, what, calls=1, old=None):
    if impl == 0:
        want = fixed_ref(indptr, indices, U, V, old)
        assert np.array_equal(got, want), f"{what}: {int((got != want).sum())} of {want.size} words differ, first at {int(np.nonzero(got != want)[0][0])}"
    else:
        float_check(got, float_products(indptr, indices, U, V), calls, what)


def device_form(mem, sp, U, V, pad=0, accumulate_into=None, out=None):
    """hsp_sddmm_device over fresh buffers with ld = the dimension rounded up to 4 plus `pad`; returns (result words, out buffer)"""
    k = U.shape[0]
    ldu, ldv = sp.ldu + pad, sp.ldv + pad
    fill = 0x7FC00000 if sp.impl else SAT                  # what lies between the columns must never be read: NaN / the largest word
    ub = np.full((k, ldu), fill, dtype=np.uint32)
    vb = np.full((k, ldv), fill, dtype=np.uint32)
    ub[:, : sp.num_rows], vb[:, : sp.num_cols] = U, V
    du, dv = mem.alloc(ub), mem.alloc(vb)
    if out is None:
        out = mem.alloc(np.full(sp.nnz, 0xDEADBEEF, dtype=np.uint32) if accumulate_into is None else accumulate_into)
    sp.sddmm_device(du.ptr, ldu, dv.ptr, ldv, k, out.ptr, accumulate=accumulate_into is not None)
    return mem.read(sp, out), out


# ---- the cases -----------------------------------------------------------------------------------------------------------------------
ROWS, COLS, NNZ = 300, 517, 4000


def general(mem, impls):
    """300 x 517, about 4000 entries, every k of KS through both forms; saturating sums; accumulate 5 + 12 = one call of 17.
    Returns {impl: {k: words}} of the host form (the GPU test compares the two float modes)."""
    indptr, indices = random_pattern(ROWS, COLS, NNZ, 1)
    words = {}
    for impl in impls:
        words[impl] = {}
        with pattern.SampledProduct(impl, (indptr, indices, (ROWS, COLS)), 64) as sp:
            assert sp.nnz == NNZ and sp.info()["nnz"] == NNZ
            for k in KS:
                U, V = vectors(impl, k, ROWS, 10 + k), vectors(impl, k, COLS, 20 + k)
                got = sp.sddmm(U, V)
                check(impl, got, indptr, indices, U, V, f"host form, impl {impl}, k {k}")
                dev, _ = device_form(mem, sp, U, V)
                assert np.array_equal(dev, got), f"device form and host form differ, impl {impl}, k {k}"
                if impl:
                    assert same_floats(got, float_exact(float_products(indptr, indices, U, V))), f"impl {impl}, k {k}: not the double sum in ascending j"
                words[impl][k] = got
            # sums that saturate (fixed point), large magnitudes (float)
            U, V = vectors(impl, 16, ROWS, 31, 4.0), vectors(impl, 16, COLS, 32, 4.0)
            got = sp.sddmm(U, V)
            check(impl, got, indptr, indices, U, V, f"large values, impl {impl}")
            if impl == 0:
                sat = float((got == SAT).mean())
                assert 0.1 < sat < 0.9, sat
            # accumulate: 5 vectors, then 12 more
            for scale in (1.0, 4.0):
                U, V = vectors(impl, 17, ROWS, 41, scale), vectors(impl, 17, COLS, 42, scale)
                first, out = device_form(mem, sp, U[:5], V[:5])
                both, _ = device_form(mem, sp, U[5:], V[5:], accumulate_into=first, out=out)
                check(impl, both, indptr, indices, U, V, f"accumulate 5 + 12, impl {impl}, scale {scale}", calls=2)
                if impl == 0:
                    assert np.array_equal(both, sp.sddmm(U, V))
    return words


def nan_reaches_its_entry(mem, impls):
    """an inf in U against a 0 in V is NaN in exactly that entry's word -- with k = 5 (three padding vectors in the last group), and
    after a wider call whose vectors 5 ... 7 were inf in U (stale staging words must not meet the padding)"""
    indptr, indices = random_pattern(ROWS, COLS, NNZ, 2)
    rows = entry_rows(indptr)
    e0 = 1234
    r0, c0 = int(rows[e0]), int(indices[e0])
    inf = np.float32(np.inf).view(np.uint32)
    for impl in impls:
        with pattern.SampledProduct(impl, (indptr, indices, (ROWS, COLS)), 16) as sp:
            U8, V8 = vectors(impl, 8, ROWS, 51), vectors(impl, 8, COLS, 52)
            U8[5:8, :] = inf
            wide = sp.sddmm(U8, V8)
            assert not np.isfinite(wide.view(np.float32)).any()
            for j0 in (1, 4):
                U, V = vectors(impl, 5, ROWS, 53), vectors(impl, 5, COLS, 54)
                U[j0, r0] = inf
                V[j0, c0] = 0
                for got in (sp.sddmm(U, V), device_form(mem, sp, U, V, pad=4)[0]):
                    f = got.view(np.float32)
                    same_pair = (rows == r0) & (indices == c0)
                    assert np.isnan(f[e0]) and np.array_equal(np.isnan(f), same_pair), (impl, j0, np.nonzero(np.isnan(f))[0][:5])
                    float_check(got, float_products(indptr, indices, U, V), 1, f"nan case impl {impl} j0 {j0}")


def edge_patterns():
    """(name, rows, cols, indptr, indices)"""
    out = [("nnz=0", 5, 7, np.zeros(6, dtype=np.uint32), np.zeros(0, dtype=np.uint32))]
    for n in (1, 2, 3, 5, 7):
        ip, ix = random_pattern(6, 9, n, 60 + n)
        out.append((f"nnz={n}", 6, 9, ip, ix))
    counts = np.zeros(40, dtype=np.int64)                  # rows 0-6 empty, 7-8, a run of empty rows, 20, a run, 31, rows 32-39 empty
    counts[[7, 8, 20, 31]] = (3, 1, 6, 2)
    rng = np.random.default_rng(70)
    ip = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
    out.append(("empty rows at the start, in runs and at the end", 40, 11, ip, rng.integers(0, 11, int(counts.sum())).astype(np.uint32)))
    ip = np.zeros(10, dtype=np.uint32)
    ip[5:] = 301
    out.append(("one row holds every entry", 9, 301, ip, np.arange(301, dtype=np.uint32)))
    ip = np.zeros(8, dtype=np.uint32)
    ip[1:] = 1
    ip[7] = 2
    out.append(("an entry in the last row and column", 7, 13, ip, np.array([0, 12], dtype=np.uint32)))
    ip, ix = random_pattern(20, 50, 200, 71)
    for r in range(20):
        seg = ix[ip[r]: ip[r + 1]]
        ix[ip[r]: ip[r + 1]] = rng.permutation(seg)
    out.append(("unsorted columns", 20, 50, ip, ix))
    out.append(("a pair held twice", 3, 6, np.array([0, 1, 5, 6], dtype=np.uint32), np.array([2, 4, 1, 4, 0, 3], dtype=np.uint32)))
    return out


def edges(mem, impls):
    for name, rows, cols, indptr, indices in edge_patterns():
        for impl in impls:
            with pattern.SampledProduct(impl, (indptr, indices, (rows, cols)), 8) as sp:
                assert sp.nnz == indices.size
                for k in (1, 5):
                    U, V = vectors(impl, k, rows, 80 + k), vectors(impl, k, cols, 90 + k)
                    what = f"{name}, impl {impl}, k {k}"
                    got = sp.sddmm(U, V)
                    check(impl, got, indptr, indices, U, V, what + ", host form")
                    dev, _ = device_form(mem, sp, U, V, pad=8)           # ldu / ldv larger than the dimensions
                    assert np.array_equal(dev, got), what
                    if name == "a pair held twice":
                        assert got[1] == got[3] and got.size == 6, what


def _create(impl, rows, cols, indptr, indices, max_k):
    l = pattern.lib()
    h = C.c_void_p(0xBAD)
    indptr = None if indptr is None else np.ascontiguousarray(indptr, dtype=np.uint32)
    indices = None if indices is None else np.ascontiguousarray(indices, dtype=np.uint32)
    rc = l.hsp_create(C.byref(h), 0, impl, rows, cols, None if indptr is None else indptr.ctypes.data, None if indices is None else indices.ctypes.data, max_k)
    return rc, h


def refusals(mem, impls):
    l = pattern.lib()
    indptr, indices = random_pattern(6, 9, 7, 5)
    for impl in impls:
        bad_index = indices.copy()
        bad_index[3] = 9
        down = np.array([0, 3, 2, 4, 5, 6, 7], dtype=np.uint32)
        shifted = np.array([1, 2, 3, 4, 5, 6, 7], dtype=np.uint32)
        for what, args, code in (("max_k 0", (impl, 6, 9, indptr, indices, 0), BAD_ARG), ("max_k 65", (impl, 6, 9, indptr, indices, 65), BAD_ARG),
                                 ("null indptr", (impl, 6, 9, None, indices, 4), BAD_ARG), ("null indices", (impl, 6, 9, indptr, None, 4), BAD_ARG),
                                 ("impl 9", (9, 6, 9, indptr, indices, 4), BAD_ARG), ("no rows", (impl, 0, 9, indptr, indices, 4), BAD_ARG),
                                 ("index = num_cols", (impl, 6, 9, indptr, bad_index, 4), BAD_MATRIX),
                                 ("indptr decreases", (impl, 6, 9, down, indices, 4), BAD_MATRIX),
                                 ("indptr[0] = 1", (impl, 6, 9, shifted, indices, 4), BAD_MATRIX)):
            rc, h = _create(*args)
            assert rc == code and not h.value and l.hsp_last_error(None), (what, rc, h.value)
        assert l.hsp_create(None, 0, impl, 6, 9, indptr.ctypes.data, indices.ctypes.data, 4) == BAD_ARG and l.hsp_last_error(None)
        assert l.hsp_info(None, None, None) == BAD_ARG and l.hsp_sync(None) == BAD_ARG and l.hsp_set_stream(None, None) == BAD_ARG
        assert l.hsp_destroy(None) == 0
        with pattern.SampledProduct(impl, (indptr, indices, (6, 9)), 4) as sp:
            U, V = vectors(impl, 4, 6, 1), vectors(impl, 4, 9, 2)
            want = sp.sddmm(U, V)
            check(impl, want, indptr, indices, U, V, f"refusals, impl {impl}")
            du, dv, out = mem.alloc(np.zeros((4, 8), np.uint32)), mem.alloc(np.zeros((4, 12), np.uint32)), mem.alloc(np.zeros(8, np.uint32))
            u, v, o, vp = du.ptr, dv.ptr, out.ptr, C.c_void_p
            for what, args in (("k = 0", (u, 8, v, 12, 0, o)), ("k > max_k", (u, 8, v, 12, 5, o)), ("misaligned u", (u + 4, 8, v, 12, 1, o)),
                               ("misaligned v", (u, 8, v + 8, 12, 1, o)), ("misaligned out", (u, 8, v, 12, 1, o + 4)), ("odd ldu", (u, 10, v, 12, 2, o)),
                               ("odd ldv", (u, 8, v, 13, 2, o)), ("ldu < num_rows", (u, 4, v, 12, 2, o)), ("null u", (None, 8, v, 12, 1, o)),
                               ("null v", (u, 8, None, 12, 1, o)), ("null out", (u, 8, v, 12, 1, None))):
                a = args
                rc = l.hsp_sddmm_device(sp._h, vp(a[0]), a[1], vp(a[2]), a[3], a[4], vp(a[5]), 0)
                assert rc == BAD_ARG and l.hsp_last_error(sp._h), (what, rc)
                assert np.array_equal(sp.sddmm(U, V), want), f"unusable after {what}"          # the object stays usable
            hu = np.zeros((5, 8), np.uint32)
            hv = np.zeros((5, 12), np.uint32)
            ho = np.zeros(8, np.uint32)
            for what, args in (("host k = 0", (hu.ctypes.data, hv.ctypes.data, 0, ho.ctypes.data)), ("host k > max_k", (hu.ctypes.data, hv.ctypes.data, 5, ho.ctypes.data)),
                               ("host null u", (None, hv.ctypes.data, 1, ho.ctypes.data)), ("host null out", (hu.ctypes.data, hv.ctypes.data, 1, None))):
                assert l.hsp_sddmm(sp._h, vp(args[0]), vp(args[1]), args[2], vp(args[3])) == BAD_ARG and l.hsp_last_error(sp._h), what
            assert np.array_equal(sp.sddmm(U, V), want)
            sp.set_stream(None)
            sp.sync()

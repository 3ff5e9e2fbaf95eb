"""The cases of the row-major feature products (include/hisparse_wide.h), shared by tests/test_wide_cpu.py (libhisparse_cpu.so, in a child
process) and tests/test_gpu_wide.py (the HIP library, on the device), written against the memory interface of tests/pattern_cases.py.

Reference, from the header's ARITHMETIC block (class D, L = 1 of tests/float_contract.py).  Every call is seen as output words that are
sums over SEGMENTS of a term array T (terms x width, the fp32 products formed in numpy float32 and widened to float64):
    sddmm     T = p.T, p[e][j] = U[row(e)][j] V[col(e)][j]; one segment of d terms, nnz words
    spmm      T[e][j] = w[e] X[col(e)][j]; the segments are the rows
    spmm_t    T[k][j] = w[e_k] X[row(e_k)][j] with the entries in (column, CSR index) order; the segments are the columns
Per word E = the exact sum of its terms, A = the sum of their magnitudes, n their count and
    |result - E| <= U |E| + n 2^-52 A + 2^-149.
E is math.fsum of the terms (exact=True); in the two large cases of the GPU tests it is a float64 sum and the middle term is doubled to
cover that sum's own rounding (n 2^-53 A at the most, half of the term).  Every word is held to the bound; a word with a non-finite
term must equal the IEEE double sum of its terms (NaN where NaN), which no order of summation changes."""
import ctypes as C
import math

import numpy as np

from hisparse_amd import wide

import float_contract as fc
import pattern_cases as pc
from pattern_cases import HipMemory, HostMemory, edge_patterns, entry_rows, random_pattern  # noqa: F401

BAD_ARG, BAD_MATRIX, UNSUPPORTED = -1, -4, -6
SENTINEL = 0xDEADBEEF
NAN_WORD = 0x7FC00000
OPS = ("sddmm", "spmm", "spmm_t")
DS = (1, 3, 4, 5, 16, 17, 63, 64, 65, 128, 256)
ROWS, COLS, NNZ = pc.ROWS, pc.COLS, pc.NNZ


def round_up4(n):
    return -(-n // 4) * 4


# ---- patterns ------------------------------------------------------------------------------------------------------------------------
def transposed_pattern(rows, cols, indptr, indices):
    """(cptr, the row of every entry in column order, the CSR index of every such entry): a column's entries in ascending CSR index"""
    ix = np.asarray(indices, dtype=np.int64)
    order = np.argsort(ix, kind="stable")
    cptr = np.zeros(cols + 1, dtype=np.int64)
    cptr[1:] = np.cumsum(np.bincount(ix, minlength=cols))
    return cptr, entry_rows(indptr)[order], order


def as_csr_of_the_transpose(rows, cols, indptr, indices):
    """the pattern of A^T as CSR arrays (cols x rows)"""
    cptr, trow, _ = transposed_pattern(rows, cols, indptr, indices)
    return cols, rows, cptr.astype(np.uint32), trow.astype(np.uint32)


# ---- reference -----------------------------------------------------------------------------------------------------------------------
def terms(op, shape, indptr, indices, a, b):
    """(T float32 (terms x width), segment pointers, the shape of the result)"""
    rows, cols = shape
    r, c = entry_rows(indptr), np.asarray(indices, dtype=np.int64)
    with np.errstate(all="ignore"):
        if op == "sddmm":
            d = a.shape[1]
            return np.ascontiguousarray((a[r] * b[c]).T), np.array([0, d], dtype=np.int64), (r.size,)
        if op == "spmm":
            return a[:, None] * b[c], np.asarray(indptr, dtype=np.int64), (rows, b.shape[1])
        cptr, trow, order = transposed_pattern(rows, cols, indptr, indices)
        return a[order, None] * b[trow], cptr, (cols, b.shape[1])


class Reference:
    """E, A, n, the bound and the IEEE sums of every output word of one call (computed once, shared by the forms that are checked)"""

    def __init__(self, op, shape, indptr, indices, a, b, exact=True):
        T, ptr, self.shape = terms(op, shape, indptr, indices, a, b)
        assert T.dtype == np.float32
        T64 = T.astype(np.float64)
        segs, width = ptr.size - 1, T.shape[1]
        n = np.diff(ptr)
        live = n > 0
        starts = ptr[:-1][live]
        fin_t = np.isfinite(T64)

        def seg_sum(x):
            out = np.zeros((segs, width), dtype=x.dtype if x.dtype != bool else np.int64)
            if x.shape[0] and live.any():
                out[live] = np.add.reduceat(x, starts, axis=0)
            return out

        with np.errstate(all="ignore"):
            self.ieee = seg_sum(T64)
        self.finite = seg_sum((~fin_t).astype(np.int64)) == 0
        clean = np.where(fin_t, T64, 0.0)
        self.A = seg_sum(np.abs(clean))
        if exact:
            cols_ = clean.T.tolist()
            bounds = ptr.tolist()
            self.E = np.array([[math.fsum(col[bounds[s]: bounds[s + 1]]) for col in cols_] for s in range(segs)], dtype=np.float64).reshape(segs, width)
        else:
            self.E = seg_sum(clean)
        self.n = np.broadcast_to(n[:, None], (segs, width))
        self.bound = fc.U * np.abs(self.E) + (1.0 if exact else 2.0) * self.n * 2.0 ** -52 * self.A + 2.0 ** -149
        self.empty = ~live

    def check(self, got, what):
        got = np.asarray(got, dtype=np.float32)
        assert got.shape == self.shape, (what, got.shape, self.shape)
        g = got.astype(np.float64).reshape(self.E.shape)
        with np.errstate(invalid="ignore"):
            bad = self.finite & ~(np.isfinite(g) & (np.abs(g - self.E) <= self.bound))
            bad |= ~self.finite & ~((g == self.ieee) | (np.isnan(g) & np.isnan(self.ieee)))
        if bad.any():
            s, j = (int(i[0]) for i in np.nonzero(bad))
            raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} words break the float contract, first [{s}][{j}]: got={g[s, j]!r} E={self.E[s, j]!r} "
                                 f"bound={self.bound[s, j]:.3g} n={int(self.n[s, j])} ieee={self.ieee[s, j]!r}")
        if self.empty.any() and got.ndim == 2:      # a row / column without entries: d words of +0.0f
            assert not got.view(np.uint32)[self.empty].any(), f"{what}: an empty row is not +0.0"


# ---- inputs and the two forms --------------------------------------------------------------------------------------------------------
def operands(op, shape, nnz, d, seed, scale=1.0):
    rows, cols = shape
    rng = np.random.default_rng(seed)
    if op == "sddmm":
        return rng.normal(0.0, scale, (rows, d)).astype(np.float32), rng.normal(0.0, scale, (cols, d)).astype(np.float32)
    return rng.normal(0.0, scale, nnz).astype(np.float32), rng.normal(0.0, scale, (cols if op == "spmm" else rows, d)).astype(np.float32)


def host_form(wp, op, a, b):
    return getattr(wp, op)(a, b)


def _features_in(mem, a, pad):
    """a (n, d) on the device with ld = round_up4(d) + pad, the pad words NaN"""
    ld = round_up4(a.shape[1]) + pad
    buf = np.full((a.shape[0], ld), NAN_WORD, dtype=np.uint32)
    buf[:, : a.shape[1]] = a.view(np.uint32)
    return mem.alloc(buf), ld


def _features_out(mem, wp, buf, n, d, ld, what):
    words = mem.read(wp, buf).reshape(n, ld)
    assert (words[:, d:] == SENTINEL).all(), f"{what}: the pad words of the result were written"
    return np.ascontiguousarray(words[:, :d]).view(np.float32)


def device_form(mem, wp, op, a, b, pad=0, what=""):
    """the _device call over fresh buffers: input pads NaN, the result pre-filled with a sentinel whose pad words must survive"""
    if op == "sddmm":
        d = a.shape[1]
        (du, ldu), (dv, ldv) = _features_in(mem, a, pad), _features_in(mem, b, pad)
        out = mem.alloc(np.full(wp.nnz, SENTINEL, dtype=np.uint32))
        wp.sddmm_device(du.ptr, ldu, dv.ptr, ldv, d, out.ptr)
        return mem.read(wp, out).view(np.float32)
    d = b.shape[1]
    n_out = wp.num_rows if op == "spmm" else wp.num_cols
    dw = mem.alloc(a.view(np.uint32))
    (dx, ldx) = _features_in(mem, b, pad)
    ldy = round_up4(d) + pad
    dy = mem.alloc(np.full((n_out, ldy), SENTINEL, dtype=np.uint32))
    getattr(wp, op + "_device")(dw.ptr, dx.ptr, ldx, d, dy.ptr, ldy)
    return _features_out(mem, wp, dy, n_out, d, ldy, what)


def words(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def both_forms(mem, wp, op, shape, indptr, indices, a, b, pads, what, exact=True):
    """the host form and the device form at every pad inside the bound of one reference; returns the host form's result"""
    ref = Reference(op, shape, indptr, indices, a, b, exact)
    got = host_form(wp, op, a, b)
    ref.check(got, f"{what}, host form")
    for pad in pads:
        ref.check(device_form(mem, wp, op, a, b, pad, what), f"{what}, device form, pad {pad}")
    return got


# ---- the cases -------------------------------------------------------------------------------------------------------------------------
def general(mem, ds=DS):
    """300 x 517, 4000 entries, every d of DS, pad 0 and 8, the three calls through both forms"""
    indptr, indices = random_pattern(ROWS, COLS, NNZ, 1)
    shape = (ROWS, COLS)
    with wide.WideProducts((indptr, indices, shape)) as wp:
        assert wp.nnz == NNZ and wp.info()["nnz"] == NNZ
        for d in ds:
            for k, op in enumerate(OPS):
                a, b = operands(op, shape, NNZ, d, 100 * d + k)
                both_forms(mem, wp, op, shape, indptr, indices, a, b, (0, 8), f"general {op}, d {d}")


def edges(mem):
    """every pattern of pattern_cases.edge_patterns() and its transpose at d = 1 and 5: nnz = 0 ... 7, runs of empty rows (columns), one row
    (column) that holds all 301 entries, the last row and column, unsorted columns, a pair held twice"""
    for name, rows, cols, indptr, indices in edge_patterns():
        for tname, (r_, c_, ip, ix) in ((name, (rows, cols, indptr, indices)), (name + ", transposed", as_csr_of_the_transpose(rows, cols, indptr, indices))):
            shape = (r_, c_)
            with wide.WideProducts((ip, ix, shape)) as wp:
                assert wp.nnz == ix.size
                for d in (1, 5):
                    for k, op in enumerate(OPS):
                        a, b = operands(op, shape, ix.size, d, 300 + 10 * d + k)
                        got = both_forms(mem, wp, op, shape, ip, ix, a, b, (8,), f"{tname}: {op}, d {d}")
                        if op == "sddmm" and name == "a pair held twice" and tname == name:
                            assert got.size == 6 and got[1] == got[3], tname


def non_finite(mem):
    """SpMMs: w[e0] = inf against a zero of X at feature j0 is NaN in that one word of e0's row (column), +-inf in the row's other words,
    and every other row is finite.  SDDMM: an inf in U against a 0 in V is NaN in exactly the words of that (row, column) pair."""
    indptr, indices = random_pattern(ROWS, COLS, NNZ, 2)
    shape = (ROWS, COLS)
    rows = entry_rows(indptr)
    e0, d = 1234, 5
    r0, c0 = int(rows[e0]), int(indices[e0])
    with wide.WideProducts((indptr, indices, shape)) as wp:
        for j0 in (1, 4):
            for op, hit_in, hit_out in (("spmm", c0, r0), ("spmm_t", r0, c0)):
                w, X = operands(op, shape, NNZ, d, 400 + j0)
                w[e0] = np.inf
                X[hit_in, j0] = 0.0
                ref = Reference(op, shape, indptr, indices, w, X)
                for got in (host_form(wp, op, w, X), device_form(mem, wp, op, w, X, 4)):
                    ref.check(got, f"non-finite {op}")
                    assert np.isnan(got[hit_out, j0]) and np.isinf(np.delete(got[hit_out], j0)).all(), (op, got[hit_out])
                    assert np.isfinite(np.delete(got, hit_out, axis=0)).all(), op
            U, V = operands("sddmm", shape, NNZ, d, 410 + j0)
            U[r0, j0] = np.inf
            V[c0, j0] = 0.0
            ref = Reference("sddmm", shape, indptr, indices, U, V)
            same_pair = (rows == r0) & (indices == c0)
            for got in (host_form(wp, "sddmm", U, V), device_form(mem, wp, "sddmm", U, V, 4)):
                ref.check(got, "non-finite sddmm")
                assert np.isnan(got[e0]) and np.array_equal(np.isnan(got), same_pair), np.nonzero(np.isnan(got))[0][:5]


def grid_values(rng, shape):
    """multiples of 1/8 of magnitude below 4: six significant bits, so that the product of two of them is exact in fp32"""
    return (rng.integers(-31, 32, shape) / 8.0).astype(np.float32)


def adjoint(mem):
    """<spmm(w, X), G> = <w, sddmm(G, X)> = <X, spmm_t(w, G)> in float64 for random w, X and G.  The three are equal as real numbers only
    where the fp32 products w x, g x and w g carry no rounding of their own, so the operands are random multiples of 1/8 (every product is
    then exact in fp32 and each result word's E is the real sum).  What is left is the rounding of the result words: each side may be off
    by the sum of its words' bounds times the magnitude of the operand it is paired with; the pairings themselves are math.fsum."""
    indptr, indices = random_pattern(ROWS, COLS, NNZ, 3)
    shape = (ROWS, COLS)
    with wide.WideProducts((indptr, indices, shape)) as wp:
        for d in (5, 16):
            rng = np.random.default_rng(500 + d)
            w, X, G = grid_values(rng, NNZ), grid_values(rng, (COLS, d)), grid_values(rng, (ROWS, d))
            sides = []
            for op, a, b, other in (("spmm", w, X, G), ("sddmm", G, X, w), ("spmm_t", w, G, X)):
                ref = Reference(op, shape, indptr, indices, a, b)
                got = device_form(mem, wp, op, a, b, 0)
                ref.check(got, f"adjoint {op}")
                o64 = other.astype(np.float64).ravel()
                sides.append((math.fsum((got.astype(np.float64).ravel() * o64).tolist()), float((ref.bound.ravel() * np.abs(o64)).sum()),
                              math.fsum((ref.E.ravel() * o64).tolist())))
            exact = [s[2] for s in sides]
            assert max(exact) - min(exact) <= 1e-9 * max(1.0, abs(exact[0])), exact      # the identity itself, on the exact sums
            for i in range(3):
                for k in range(i + 1, 3):
                    assert abs(sides[i][0] - sides[k][0]) <= sides[i][1] + sides[k][1], (d, i, k, sides)


def nothing_carried_over(mem):
    """two calls with the same inputs give the same words; a call with other inputs and another d on the same object gives the words of
    a fresh object"""
    indptr, indices = random_pattern(ROWS, COLS, NNZ, 4)
    shape = (ROWS, COLS)
    with wide.WideProducts((indptr, indices, shape)) as wp, wide.WideProducts((indptr, indices, shape)) as fresh:
        for k, op in enumerate(OPS):
            a, b = operands(op, shape, NNZ, 64, 600 + k)
            first = device_form(mem, wp, op, a, b, 0)
            assert np.array_equal(words(first), words(device_form(mem, wp, op, a, b, 0))), op
            a2, b2 = operands(op, shape, NNZ, 5, 610 + k, 3.0)
            second = device_form(mem, wp, op, a2, b2, 4)
            assert np.array_equal(words(second), words(device_form(mem, fresh, op, a2, b2, 4))), op
            Reference(op, shape, indptr, indices, a2, b2).check(second, f"second call, {op}")


def _create(rows, cols, indptr, indices, flags):
    l = wide.lib()
    h = C.c_void_p(0xBAD)
    indptr = None if indptr is None else np.ascontiguousarray(indptr, dtype=np.uint32)
    indices = None if indices is None else np.ascontiguousarray(indices, dtype=np.uint32)
    rc = l.hsw_create(C.byref(h), 0, rows, cols, None if indptr is None else indptr.ctypes.data, None if indices is None else indices.ctypes.data, flags)
    return rc, h


def refusals(mem):
    l = wide.lib()
    vp = C.c_void_p
    indptr, indices = random_pattern(6, 9, 7, 5)
    shape = (6, 9)
    bad_index = indices.copy()
    bad_index[3] = 9
    down = np.array([0, 3, 2, 4, 5, 6, 7], dtype=np.uint32)
    shifted = np.array([1, 2, 3, 4, 5, 6, 7], dtype=np.uint32)
    for what, args, code in (("null indptr", (6, 9, None, indices, 1), BAD_ARG), ("null indices", (6, 9, indptr, None, 1), BAD_ARG),
                             ("no rows", (0, 9, indptr, indices, 1), BAD_ARG), ("no columns", (6, 0, indptr, indices, 1), BAD_ARG),
                             ("index = num_cols", (6, 9, indptr, bad_index, 0), BAD_MATRIX), ("indptr decreases", (6, 9, down, indices, 1), BAD_MATRIX),
                             ("indptr[0] = 1", (6, 9, shifted, indices, 1), BAD_MATRIX), ("flag bit 1", (6, 9, indptr, indices, 2), BAD_ARG),
                             ("flag bits 0 and 4", (6, 9, indptr, indices, 17), BAD_ARG)):
        rc, h = _create(*args)
        assert rc == code and not h.value and l.hsw_last_error(None), (what, rc, h.value)
    assert l.hsw_create(None, 0, 6, 9, indptr.ctypes.data, indices.ctypes.data, 1) == BAD_ARG and l.hsw_last_error(None)
    # null-object calls
    one = np.zeros(4, dtype=np.float32).ctypes.data
    assert l.hsw_info(None, None, None) == BAD_ARG and l.hsw_sync(None) == BAD_ARG and l.hsw_set_stream(None, None) == BAD_ARG
    assert l.hsw_sddmm_device(None, vp(one), 4, vp(one), 4, 1, vp(one)) == BAD_ARG and l.hsw_sddmm(None, vp(one), vp(one), 1, vp(one)) == BAD_ARG
    for f in (l.hsw_spmm_device, l.hsw_spmm_t_device):
        assert f(None, vp(one), vp(one), 4, 1, vp(one), 4) == BAD_ARG
    for f in (l.hsw_spmm, l.hsw_spmm_t):
        assert f(None, vp(one), vp(one), 1, vp(one)) == BAD_ARG
    assert l.hsw_destroy(None) == 0

    d = 5
    with wide.WideProducts((indptr, indices, shape)) as wp, wide.WideProducts((indptr, indices, shape), transposed=False) as plain:
        inputs = {op: operands(op, shape, 7, d, 700 + k) for k, op in enumerate(OPS)}
        want = {op: host_form(wp, op, *inputs[op]) for op in OPS}
        for op in OPS:
            Reference(op, shape, indptr, indices, *inputs[op]).check(want[op], f"refusals, {op}")

        def still_usable(rc, what, obj=wp, code=BAD_ARG):
            assert rc == code and l.hsw_last_error(obj._h), (what, rc)
            for op in OPS if obj is wp else OPS[:2]:
                assert np.array_equal(words(host_form(obj, op, *inputs[op])), words(want[op])), f"unusable after {what}"

        # buffers of 9 rows x 16 words (the larger dimension, ld up to 16), 16-byte aligned; `e` holds entries
        bu, bv, by, be = (mem.alloc(np.zeros(9 * 16, np.uint32)) for _ in range(4))
        u, v, y, e = bu.ptr, bv.ptr, by.ptr, be.ptr
        for what, a in (("d = 0", (u, 8, v, 8, 0, e)), ("d = 257", (u, 260, v, 260, 257, e)), ("null u", (None, 8, v, 8, d, e)), ("null v", (u, 8, None, 8, d, e)),
                        ("null out", (u, 8, v, 8, d, None)), ("misaligned u", (u + 4, 8, v, 8, d, e)), ("misaligned v", (u, 8, v + 8, 8, d, e)),
                        ("misaligned out", (u, 8, v, 8, d, e + 2)), ("ldu % 4", (u, 10, v, 8, d, e)), ("ldv % 4", (u, 8, v, 9, d, e)), ("ldu < d", (u, 4, v, 8, d, e)),
                        ("ldv < d", (u, 8, v, 4, d, e)), ("out is u", (u, 8, v, 8, d, u)), ("out inside v", (u, 8, v, 8, d, v + 16 * 4))):
            still_usable(l.hsw_sddmm_device(wp._h, vp(a[0]), a[1], vp(a[2]), a[3], a[4], vp(a[5])), "sddmm: " + what)
        for name, f in (("spmm", l.hsw_spmm_device), ("spmm_t", l.hsw_spmm_t_device)):
            for what, a in (("d = 0", (e, u, 8, 0, y, 8)), ("d = 257", (e, u, 260, 257, y, 260)), ("null w", (None, u, 8, d, y, 8)), ("null x", (e, None, 8, d, y, 8)),
                            ("null y", (e, u, 8, d, None, 8)), ("misaligned w", (e + 2, u, 8, d, y, 8)), ("misaligned x", (e, u + 4, 8, d, y, 8)),
                            ("misaligned y", (e, u, 8, d, y + 8, 8)), ("ldx % 4", (e, u, 9, d, y, 8)), ("ldy % 4", (e, u, 8, d, y, 10)), ("ldx < d", (e, u, 4, d, y, 8)),
                            ("ldy < d", (e, u, 8, d, y, 4)), ("y is x", (e, u, 8, d, u, 8)), ("y holds w", (e, u, 8, d, e, 8)), ("y's last row in x", (e, u + 16, 8, d, u + 16 + 4 * 8 * 4, 8))):
                still_usable(f(wp._h, vp(a[0]), vp(a[1]), a[2], a[3], vp(a[4]), a[5]), f"{name}: {what}")
        # the host forms
        hu, hv, hw, ho = (np.zeros(9 * 8, np.float32) for _ in range(4))
        for what, a in (("d = 0", (hu.ctypes.data, hv.ctypes.data, 0, ho.ctypes.data)), ("d = 257", (hu.ctypes.data, hv.ctypes.data, 257, ho.ctypes.data)),
                        ("null u", (None, hv.ctypes.data, d, ho.ctypes.data)), ("null v", (hu.ctypes.data, None, d, ho.ctypes.data)), ("null out", (hu.ctypes.data, hv.ctypes.data, d, None))):
            still_usable(l.hsw_sddmm(wp._h, vp(a[0]), vp(a[1]), a[2], vp(a[3])), "host sddmm: " + what)
        for name, f in (("spmm", l.hsw_spmm), ("spmm_t", l.hsw_spmm_t)):
            for what, a in (("d = 0", (hw.ctypes.data, hu.ctypes.data, 0, ho.ctypes.data)), ("d = 257", (hw.ctypes.data, hu.ctypes.data, 257, ho.ctypes.data)),
                            ("null w", (None, hu.ctypes.data, d, ho.ctypes.data)), ("null x", (hw.ctypes.data, None, d, ho.ctypes.data)), ("null y", (hw.ctypes.data, hu.ctypes.data, d, None))):
                still_usable(f(wp._h, vp(a[0]), vp(a[1]), a[2], vp(a[3])), f"host {name}: {what}")
        # hsw_spmm_t* without HSW_TRANSPOSED
        still_usable(l.hsw_spmm_t_device(plain._h, vp(e), vp(u), 8, d, vp(y), 8), "spmm_t_device without the flag", plain, UNSUPPORTED)
        still_usable(l.hsw_spmm_t(plain._h, vp(hw.ctypes.data), vp(hu.ctypes.data), d, vp(ho.ctypes.data)), "spmm_t without the flag", plain, UNSUPPORTED)
        # ranges that touch without sharing a byte are fine
        assert l.hsw_spmm_device(wp._h, vp(e), vp(u), 8, d, vp(u + 9 * 8 * 4), 8) == 0
        wp.set_stream(None)
        wp.sync()

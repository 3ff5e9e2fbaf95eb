"""The cases of the neighbour aggregation (include/hisparse_aggregate.h), shared by tests/test_aggregate_cpu.py (libhisparse_cpu.so, in a
child process) and tests/test_gpu_aggregate.py (the HIP library, on the device), written against the memory interface of
tests/pattern_cases.py.

Reference, numpy, from the header.
  Extremes and args: THE DEFINITION.  Every candidate word gets a rank -- an integer that orders the non-NaN floats as IEEE does (+0.0 and
    -0.0 share one rank), negated for the minimum, with every NaN above all of them -- and the winner of (row, feature) is the entry of
    the largest rank and, among those, of the smallest CSR index: the lexicographic order on (rank, e), taken as one segment maximum of
    an integer that holds the rank above the negated index (winner_by_loop states the same rule entry by entry;
    tests/test_aggregate_cpu.py holds one against the other).  The value is the
    word X[indices[arg]][j].  Both are compared BIT FOR BIT.
  Sums, means and the backward: per output word the terms in float64, E = math.fsum of them (for the mean over n_r), A the sum of their
    magnitudes (over n_r), n their count and
        |result - E| <= U |E| + (n + 16) 2^-52 A + 2^-149;
    in the large GPU-only cases E is a float64 sum and the 2^-52 term is doubled to cover that sum's own rounding, as gat_cases does.  A
    word with a non-finite term must equal the IEEE double sum of its terms (NaN where NaN)."""
import ctypes as C
import math

import numpy as np
import scipy.sparse as sp

from hisparse_amd import aggregate as ag
from hisparse_amd import wide

import float_contract as fc
import pattern_cases as pc
import wide_cases as wc
from pattern_cases import HipMemory, HostMemory, edge_patterns, entry_rows, random_pattern  # noqa: F401

BAD_ARG, UNSUPPORTED = -1, -6
SENTINEL = wc.SENTINEL
NAN_WORD = wc.NAN_WORD
NONE = ag.NONE
SUM, MEAN, MAX, MIN = ag.SUM, ag.MEAN, ag.MAX, ag.MIN
ALL_OPS = ag.LEGAL_OPS
DS = wc.DS
ROWS, COLS, NNZ = pc.ROWS, pc.COLS, pc.NNZ
SLACK = 16      # the header's (n + 16)
NAN_RANK = np.int64(1) << 32


def name_of(ops):
    return "|".join(n for b, n in ((SUM, "SUM"), (MEAN, "MEAN"), (MAX, "MAX"), (MIN, "MIN")) if ops & b)


# ---- the reference of the extremes ---------------------------------------------------------------------------------------------------
def rank_of(v, is_max):
    """the rank of every word of the float32 array v: int64, larger = better; NaN above everything, +0.0 and -0.0 alike"""
    i = np.ascontiguousarray(v, dtype=np.float32).view(np.int32)
    k = np.where(i < 0, -(i & 0x7FFFFFFF), i)              # the integer order of the bit patterns is the IEEE order of the non-NaN words
    return np.where(np.isnan(v), NAN_RANK, (k if is_max else -k).astype(np.int64))


INDEX_BITS = 24      # the patterns of the tests hold fewer than 2^24 entries


def winners(indptr, G, is_max):
    """(args (rows, d) uint32, value words (rows, d) uint32) of the entries' words G (nnz, d) float32: the largest rank, then the smallest
    CSR index -- ONE segment maximum over the integer (rank, -e), rank in the high bits, which is that lexicographic order; a row without
    entries is NONE and +0.0"""
    ptr = np.asarray(indptr, dtype=np.int64)
    n = np.diff(ptr)
    live = n > 0
    d = G.shape[1]
    args = np.full((n.size, d), NONE, dtype=np.uint32)
    vals = np.zeros((n.size, d), dtype=np.uint32)
    if not live.any():
        return args, vals
    assert G.shape[0] < 1 << INDEX_BITS
    last = (1 << INDEX_BITS) - 1
    key = ((rank_of(G, is_max) + (np.int64(1) << 31)) << INDEX_BITS) | (last - np.arange(G.shape[0], dtype=np.int64))[:, None]      # below 2^(34 + 24)
    first = last - (np.maximum.reduceat(key, ptr[:-1][live], axis=0) & last)
    args[live] = first.astype(np.uint32)
    vals[live] = G.view(np.uint32)[first, np.arange(d)[None, :]]
    return args, vals


def winner_by_loop(words, is_max):
    """the header's rule, entry by entry, over the float32 words of one (row, feature) in CSR order: the position of the winner"""
    best = None
    for k, v in enumerate(words):
        if best is None:
            best = k
            continue
        b = words[best]
        if np.isnan(v) != np.isnan(b):
            better = bool(np.isnan(v))
        elif np.isnan(v):
            better = False
        else:
            better = bool(v > b) if is_max else bool(v < b)
        if better:                                         # an equal word never replaces an earlier one
            best = k
    return best


# ---- the reference of the sums -------------------------------------------------------------------------------------------------------
class SumRef:
    """E, A, n, the bound and the IEEE sums of the words that are sums over the segments of T (terms x width float64; a term that does not
    take part is 0.0 there and is not counted in `count`); `over` divides a segment's E and A (the mean)"""

    def __init__(self, T, ptr, count=None, over=None, exact=True, magnitudes=None):
        T = np.asarray(T, dtype=np.float64)
        ptr = np.asarray(ptr, dtype=np.int64)
        segs, width = ptr.size - 1, T.shape[1]
        length = np.diff(ptr)
        live = length > 0
        fin_t = np.isfinite(T)

        def seg_sum(x):
            """the segments' sums, added in ascending order (a product with the segments' 0 / 1 matrix: much faster than reduceat)"""
            if not x.shape[0]:
                return np.zeros((segs, width), dtype=x.dtype)
            return np.asarray(sp.csr_matrix((np.ones(x.shape[0], dtype=x.dtype), np.arange(x.shape[0]), ptr), shape=(segs, x.shape[0])) @ x)

        with np.errstate(all="ignore"):
            self.ieee = seg_sum(T)
        self.finite = seg_sum((~fin_t).astype(np.int64)) == 0
        clean = np.where(fin_t, T, 0.0)
        self.A = seg_sum(np.abs(clean) if magnitudes is None else np.where(fin_t, magnitudes, 0.0))      # magnitudes: of a term that is itself a sum
        if exact:
            cols_, bounds = clean.T.tolist(), ptr.tolist()
            self.E = np.array([[math.fsum(col[bounds[s]: bounds[s + 1]]) for col in cols_] for s in range(segs)], dtype=np.float64).reshape(segs, width)
        else:
            self.E = seg_sum(clean)
        self.n = np.broadcast_to(length[:, None], (segs, width)) if count is None else count
        if over is not None:
            by = np.maximum(np.asarray(over, dtype=np.float64), 1.0)[:, None]
            with np.errstate(all="ignore"):
                self.E, self.A, self.ieee = self.E / by, self.A / by, self.ieee / by
        self.bound = fc.U * np.abs(self.E) + (1.0 if exact else 2.0) * (self.n + SLACK) * 2.0 ** -52 * self.A + 2.0 ** -149
        self.empty = ~live

    def check(self, got, what):
        got = np.asarray(got, dtype=np.float32)
        assert got.shape == self.E.shape, (what, got.shape, self.E.shape)
        g = got.astype(np.float64)
        with np.errstate(invalid="ignore"):
            bad = self.finite & ~(np.isfinite(g) & (np.abs(g - self.E) <= self.bound))
            bad |= ~self.finite & ~((g == self.ieee) | (np.isnan(g) & np.isnan(self.ieee)))
        if bad.any():
            s, j = (int(i[0]) for i in np.nonzero(bad))
            raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} words break the float contract, first [{s}][{j}]: got={g[s, j]!r} E={self.E[s, j]!r} "
                                 f"bound={self.bound[s, j]:.3g} n={int(self.n[s, j])} ieee={self.ieee[s, j]!r}")
        if self.empty.any():      # a row / column without entries: d words of +0.0f
            assert not got.view(np.uint32)[self.empty].any(), f"{what}: an empty row is not +0.0"


class ForwardRef:
    """everything hsagg_forward may be asked for over one pattern and one X, each part computed once when first needed"""

    def __init__(self, indptr, indices, X, exact=True):
        self.indptr, self.indices, self.X, self.exact = np.asarray(indptr), np.asarray(indices, dtype=np.int64), np.ascontiguousarray(X, dtype=np.float32), exact
        self.G = self.X[self.indices]                      # the entries' words, in CSR order: the reference may hold what the library never does
        self.n = np.diff(self.indptr.astype(np.int64))
        self._parts = {}

    def part(self, name):
        if name not in self._parts:
            if name in ("sum", "mean"):
                self._parts[name] = SumRef(self.G.astype(np.float64), self.indptr, over=self.n if name == "mean" else None, exact=self.exact)
            else:
                self._parts[name] = winners(self.indptr, self.G, name == "max")
        return self._parts[name]

    def check(self, out, ops, what, args=True):
        assert sorted(out) == sorted(outputs_of(ops, args)), (what, sorted(out))
        if ops & (SUM | MEAN):
            self.part("mean" if ops & MEAN else "sum").check(out["sum"], f"{what}, {'mean' if ops & MEAN else 'sum'}")
        for bit, name in ((MAX, "max"), (MIN, "min")):
            if not ops & bit:
                continue
            want_a, want_v = self.part(name)
            got_v = np.ascontiguousarray(out[name], dtype=np.float32).view(np.uint32)
            assert got_v.shape == want_v.shape and np.array_equal(got_v, want_v), \
                f"{what}: {int((got_v != want_v).sum())} words of y{name} are not the winner's word, first at {tuple(int(i[0]) for i in np.nonzero(got_v != want_v))}"
            if args:
                got_a = np.asarray(out["a" + name])
                assert got_a.dtype == np.uint32 and np.array_equal(got_a, want_a), \
                    f"{what}: {int((got_a != want_a).sum())} words of a{name} differ, first at {tuple(int(i[0]) for i in np.nonzero(got_a != want_a))}"
                live = got_a != NONE                      # the consequence the header states: the value IS the word the arg names
                r, j = np.nonzero(live)
                assert np.array_equal(got_v[live], self.X.view(np.uint32)[self.indices[got_a[live]], j]), f"{what}: y{name} is not X[indices[a{name}]]"
                assert (live == (self.n > 0)[:, None]).all() and not got_v[~live].any(), f"{what}: rows without entries"


class BackwardRef(SumRef):
    """gx of hsagg_backward over the transposed pattern: per entry k of a column, in (column, CSR index) order, up to three terms"""

    def __init__(self, shape, indptr, indices, ops, grads, exact=True):
        rows, cols = shape
        cptr, trow, order = wc.transposed_pattern(rows, cols, indptr, indices)
        n_r = np.diff(np.asarray(indptr, dtype=np.int64))
        d = next(a.shape[1] for a in grads.values() if a is not None)
        T = np.zeros((order.size, 3, d), dtype=np.float64)
        used = np.zeros((order.size, 3, d), dtype=np.int32)
        with np.errstate(all="ignore"):
            if ops & (SUM | MEAN):
                g = np.asarray(grads["gsum"], dtype=np.float32)[trow].astype(np.float64)
                T[:, 0] = g / n_r[trow][:, None] if ops & MEAN else g
                used[:, 0] = 1
            for slot, bit, gname, aname in ((1, MAX, "gmax", "amax"), (2, MIN, "gmin", "amin")):
                if ops & bit:
                    hit = np.asarray(grads[aname], dtype=np.uint32)[trow] == order.astype(np.uint32)[:, None]
                    T[:, slot] = np.where(hit, np.asarray(grads[gname], dtype=np.float32)[trow].astype(np.float64), 0.0)
                    used[:, slot] = hit
        cptr = np.asarray(cptr, dtype=np.int64)
        count = np.zeros((cols, d), dtype=np.int64)
        if order.size:
            count = np.asarray(sp.csr_matrix((np.ones(order.size, dtype=np.int64), np.arange(order.size), cptr), shape=(cols, order.size)) @ used.sum(axis=1, dtype=np.int64))
        if exact:      # every term on its own: three per entry, those that do not take part 0.0
            super().__init__(T.reshape(-1, d), 3 * cptr, count=count)
        else:          # float64 sums anyway: an entry's terms added first
            super().__init__(T.sum(axis=1), cptr, count=count, exact=False, magnitudes=np.abs(T).sum(axis=1))
        self.cptr = cptr


# ---- inputs and the two forms --------------------------------------------------------------------------------------------------------
def features(n, d, seed, scale=1.0):
    return np.random.default_rng(seed).normal(0.0, scale, (n, d)).astype(np.float32)


def rows_pattern(lengths, seed, cols=None):
    """one row per length with columns of its own, in a shuffled (unsorted) order: (shape, indptr, indices); X[indices[e]] is then entry
    e's alone"""
    rng = np.random.default_rng(seed)
    lengths = np.asarray(lengths, dtype=np.int64)
    indptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint32)
    total = int(lengths.sum())
    indices = np.concatenate([rng.permutation(np.arange(int(a), int(b))) for a, b in zip(indptr[:-1], indptr[1:])] + [np.zeros(0, dtype=np.int64)]).astype(np.uint32)
    return (lengths.size, cols or max(total, 1)), indptr, indices


def outputs_of(ops, args):
    """the names of the arrays a forward call for `ops` returns"""
    return ["sum"] * bool(ops & (SUM | MEAN)) + (["max"] + ["amax"] * bool(args)) * bool(ops & MAX) + (["min"] + ["amin"] * bool(args)) * bool(ops & MIN)


def forward_host(na, X, ops, args=True):
    return na.forward(X, ops, want_args=args)


def forward_device(mem, na, X, ops, pad=0, args=True, what=""):
    """hsagg_forward_device over fresh buffers: X's pad words NaN, every output pre-filled with a sentinel whose pad words must survive,
    the outputs `ops` does not ask for (and the args, with args=False) NULL; the result as forward_host gives it"""
    d = X.shape[1]
    dx, ldx = wc._features_in(mem, X, pad)
    ldy = wc.round_up4(d) + pad
    names = outputs_of(ops, args)
    bufs = {n: mem.alloc(np.full((na.num_rows, ldy), SENTINEL, dtype=np.uint32)) for n in names}
    p = {n: (bufs[n].ptr if n in bufs else None) for n in ("sum", "max", "amax", "min", "amin")}
    na.forward_device(ops, dx.ptr, ldx, d, p["sum"], p["max"], p["amax"], p["min"], p["amin"], ldy)
    out = {}
    for n in names:
        w = wc._features_out(mem, na, bufs[n], na.num_rows, d, ldy, f"{what}: {n}")
        out[n] = w.view(np.uint32) if n[0] == "a" else w
    return out


def _words_in(mem, a, pad, fill):
    ld = wc.round_up4(a.shape[1]) + pad
    buf = np.full((a.shape[0], ld), fill, dtype=np.uint32)
    buf[:, : a.shape[1]] = np.ascontiguousarray(a).view(np.uint32)
    return mem.alloc(buf), ld


def gradients(ops, rows, d, seed, fwd=None, scale=1.0):
    """the operands of a backward call for `ops`: random gradients, and the arg arrays of the forward result `fwd`"""
    g = {"gsum": None, "gmax": None, "amax": None, "gmin": None, "amin": None}
    if ops & (SUM | MEAN):
        g["gsum"] = features(rows, d, seed, scale)
    if ops & MAX:
        g["gmax"], g["amax"] = features(rows, d, seed + 1, scale), fwd["amax"]
    if ops & MIN:
        g["gmin"], g["amin"] = features(rows, d, seed + 2, scale), fwd["amin"]
    return g


def backward_host(na, ops, g):
    return na.backward(ops, **g)


def backward_device(mem, na, ops, g, pad=0, what=""):
    """hsagg_backward_device over fresh buffers: the pad words of the gradients NaN and of the arg arrays 0 (an index that exists), gx
    pre-filled with a sentinel whose pad words must survive"""
    d = next(a.shape[1] for a in g.values() if a is not None)
    p, keep = {}, []
    ldg = wc.round_up4(d) + pad
    for n, a in g.items():
        p[n] = None
        if a is not None:
            buf, ld = _words_in(mem, a, pad, 0 if n[0] == "a" else NAN_WORD)
            assert ld == ldg
            keep.append(buf)
            p[n] = buf.ptr
    ldgx = wc.round_up4(d) + pad
    out = mem.alloc(np.full((na.num_cols, ldgx), SENTINEL, dtype=np.uint32))
    na.backward_device(ops, p["gsum"], p["gmax"], p["amax"], p["gmin"], p["amin"], ldg, d, out.ptr, ldgx)
    return wc._features_out(mem, na, out, na.num_cols, d, ldgx, f"{what}: gx")


def same_words(a, b):
    if isinstance(a, dict):
        return set(a) == set(b) and all(same_words(a[k], b[k]) for k in a)
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def open_pattern(indptr, indices, shape, transposed=True):
    return ag.NeighborAggregate((indptr, indices, shape), transposed=transposed)


# ---- the cases -----------------------------------------------------------------------------------------------------------------------
def general(mem, ds=DS):
    """300 x 517, 4000 entries, every d of DS, every legal ops word: the host form, the device form at pad 0 and 8 with the args taken and
    NULL, then the backward through both forms with the args just written"""
    indptr, indices = random_pattern(ROWS, COLS, NNZ, 1)
    shape = (ROWS, COLS)
    with open_pattern(indptr, indices, shape) as na:
        assert na.nnz == NNZ and na.info()["nnz"] == NNZ
        for d in ds:
            X = features(COLS, d, 14000 + d)
            ref = ForwardRef(indptr, indices, X)
            for ops in ALL_OPS:
                what = f"general {name_of(ops)}, d {d}"
                fwd = forward_host(na, X, ops)
                ref.check(fwd, ops, what + ", host form")
                for pad in (0, 8):
                    for args in (True, False):
                        ref.check(forward_device(mem, na, X, ops, pad, args, what), ops, f"{what}, device form, pad {pad}, args {args}", args)
                ref.check(forward_host(na, X, ops, args=False), ops, what + ", host form without args", False)
                g = gradients(ops, ROWS, d, 14100 + 16 * d + ops, forward_device(mem, na, X, ops, 0, True, what))
                bref = BackwardRef(shape, indptr, indices, ops, g)
                bref.check(backward_host(na, ops, g), what + ", backward, host form")
                for pad in (0, 8):
                    bref.check(backward_device(mem, na, ops, g, pad, what), f"{what}, backward, device form, pad {pad}")


WINNER_LENGTHS = (1, 4, 5, 16, 17, 64, 65, 512, 513, 1025, 3000)


def winner_positions(mem, ds=(256, 4)):
    """one row of each length of WINNER_LENGTHS: feature j has its unique maximum at entry floor(j n / d) of the row and its unique
    minimum at the mirror position n - 1 - floor(j n / d), so one call puts a winner in every lane, trip and wavefront"""
    shape, indptr, indices = rows_pattern(WINNER_LENGTHS, 14200)
    with open_pattern(indptr, indices, shape) as na:
        for d in ds:
            X = np.random.default_rng(14210 + d).uniform(-1.0, 1.0, (shape[1], d)).astype(np.float32)
            want_max = np.zeros((len(WINNER_LENGTHS), d), dtype=np.uint32)
            want_min = np.zeros_like(want_max)
            for r, n in enumerate(WINNER_LENGTHS):
                j = np.arange(d)
                hi = int(indptr[r]) + j * n // d
                lo = int(indptr[r]) + n - 1 - j * n // d
                X[indices[hi], j] = 2.0 + j / 256.0
                apart = hi != lo                           # one entry cannot hold both: where the two positions meet, the maximum is planted alone
                X[indices[lo[apart]], j[apart]] = -2.0 - j[apart] / 256.0
                want_max[r], want_min[r] = hi, lo
                want_min[r][~apart] = NONE               # not planted
            ref = ForwardRef(indptr, indices, X)
            for what, out in ((f"winner positions, d {d}, device form", forward_device(mem, na, X, MAX | MIN, 0, True)), (f"winner positions, d {d}, host form", forward_host(na, X, MAX | MIN))):
                ref.check(out, MAX | MIN, what)
                planted = want_min != NONE
                assert np.array_equal(out["amax"], want_max) and np.array_equal(out["amin"][planted], want_min[planted]), what
            g = gradients(MAX | MIN, shape[0], d, 14220 + d, out)
            BackwardRef(shape, indptr, indices, MAX | MIN, g).check(backward_device(mem, na, MAX | MIN, g, 0), f"winner positions, d {d}, backward")


def wave_of(offset, d):
    """the wavefront of a long row's workgroup that takes the entry at `offset` from the row's start (wide_products.h: group g of the
    workgroup's WIDE_THREADS / group_lanes(d) takes the offsets congruent to g)"""
    lanes = wide.group_lanes(d)
    return (offset % (wide.WIDE_THREADS // lanes)) * lanes // 64


def ties(mem):
    """the smallest-index rule across the merge levels: rows whose entries are all equal, rows of +0.0 and -0.0 mixed, a row of duplicate
    (row, column) pairs, unsorted columns throughout, and in a long row one value at the first entry of wavefront 3's share and the
    last of wavefront 0's (and the other way round), at d = 256, 64 and 4"""
    lengths = (1, 3, 4, 5, 16, 17, 64, 65, 300, 512, 513, 1025, 3000)
    shape, indptr, indices = rows_pattern(lengths, 14300)
    first = indptr[:-1].astype(np.uint32)
    with open_pattern(indptr, indices, shape) as na:
        for d in (256, 64, 4):
            rng = np.random.default_rng(14310 + d)
            # all entries equal: one value per (row, feature)
            per_row = rng.normal(0.0, 1.0, (len(lengths), d)).astype(np.float32)
            X = np.zeros((shape[1], d), dtype=np.float32)
            X[indices] = per_row[entry_rows(indptr)]
            # +0.0 and -0.0 mixed
            Z = np.where(rng.integers(0, 2, (shape[1], d)) == 1, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
            for name, A in (("all entries equal", X), ("zeros of both signs", Z)):
                ref = ForwardRef(indptr, indices, A)
                for form, out in (("device", forward_device(mem, na, A, MEAN | MAX | MIN, 8, True)), ("host", forward_host(na, A, MEAN | MAX | MIN))):
                    ref.check(out, MEAN | MAX | MIN, f"ties: {name}, d {d}, {form} form")
                    assert (out["amax"] == first[:, None]).all() and (out["amin"] == first[:, None]).all(), (name, d, form)
                    assert np.array_equal(out["max"].view(np.uint32), A[indices[first]].view(np.uint32)), (name, d, form)
            # a long row: the same value where two wavefronts' shares meet the row's ends
            r = len(lengths) - 1
            n, lo = lengths[r], int(indptr[r])
            offs = np.arange(n)
            waves = wave_of(offs, d)
            assert set(waves.tolist()) == {0, 1, 2, 3}
            pairs = ((int(offs[waves == 3][0]), int(offs[waves == 0][-1])), (int(offs[waves == 0][0]), int(offs[waves == 3][-1])), (int(offs[waves == 1][-1]), int(offs[waves == 2][0])))
            for a, b in pairs:
                W = rng.uniform(-1.0, 1.0, (shape[1], d)).astype(np.float32)
                W[indices[lo + a]] = W[indices[lo + b]] = 5.0
                W[indices[lo + a], 1::2] = W[indices[lo + b], 1::2] = -5.0      # odd features: the shared minimum
                ref = ForwardRef(indptr, indices, W)
                for form, out in (("device", forward_device(mem, na, W, MAX | MIN, 0, True)), ("host", forward_host(na, W, MAX | MIN))):
                    ref.check(out, MAX | MIN, f"ties: offsets {a} and {b} of a long row, d {d}, {form} form")
                    assert (out["amax"][r, 0::2] == lo + min(a, b)).all() and (out["amin"][r, 1::2] == lo + min(a, b)).all(), (a, b, d, form)
    # duplicate (row, column) pairs: every column of a row held several times, in no order
    rng = np.random.default_rng(14350)
    lengths = (7, 40, 700)
    indptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint32)
    indices = np.concatenate([rng.integers(0, 5, n) for n in lengths]).astype(np.uint32)
    with open_pattern(indptr, indices, (3, 5)) as na:
        for d in (5, 64):
            X = features(5, d, 14360 + d)
            ref = ForwardRef(indptr, indices, X)
            for form, out in (("device", forward_device(mem, na, X, SUM | MAX | MIN, 4, True)), ("host", forward_host(na, X, SUM | MAX | MIN))):
                ref.check(out, SUM | MAX | MIN, f"ties: pairs held many times, d {d}, {form} form")
            g = gradients(SUM | MAX | MIN, 3, d, 14370 + d, out)
            BackwardRef((3, 5), indptr, indices, SUM | MAX | MIN, g).check(backward_device(mem, na, SUM | MAX | MIN, g, 4), f"ties: pairs held many times, d {d}, backward")


def non_finite(mem):
    """a NaN at the first, a middle and the last entry of a row wins both extremes and the arg is the first NaN; +inf and -inf in one row;
    the pad words of X are NaN throughout and reach nothing; a NaN in feature j reaches feature j only"""
    lengths = (1, 3, 9, 40, 700)
    shape, indptr, indices = rows_pattern(lengths, 14400)
    ops = MEAN | MAX | MIN
    with open_pattern(indptr, indices, shape) as na:
        for d, j0 in ((5, 4), (5, 1), (64, 37)):
            for r, n in enumerate(lengths):
                lo = int(indptr[r])
                for where in ((0,), (n // 2, n - 1), (n - 1,), (0, n // 2)):
                    X = features(shape[1], d, 14410 + d + r)
                    X[indices[[lo + k for k in where]], j0] = np.nan
                    ref = ForwardRef(indptr, indices, X)
                    for form, out in (("device", forward_device(mem, na, X, ops, 4, True)), ("host", forward_host(na, X, ops))):
                        what = f"non-finite: NaN at {where} of a row of {n}, d {d}, {form} form"
                        ref.check(out, ops, what)
                        assert np.isnan(out["max"][r, j0]) and np.isnan(out["min"][r, j0]) and np.isnan(out["sum"][r, j0]), what
                        assert out["amax"][r, j0] == out["amin"][r, j0] == lo + min(where), what
                        for k in ("sum", "max", "min"):      # feature j0 of row r, and nothing else
                            nan = np.isnan(out[k])
                            assert nan.sum() == 1 and nan[r, j0], (what, k)
            # both infinities in the longest row: the sum is NaN, the extremes are the infinities
            X = features(shape[1], d, 14450 + d)
            lo = int(indptr[-2])
            X[indices[lo + 5], j0], X[indices[lo + 600], j0], X[indices[lo + 7], 0] = np.inf, -np.inf, np.inf
            ref = ForwardRef(indptr, indices, X)
            for form, out in (("device", forward_device(mem, na, X, ops, 4, True)), ("host", forward_host(na, X, ops))):
                ref.check(out, ops, f"non-finite: infinities, d {d}, {form} form")
                assert np.isnan(out["sum"][-1, j0]) and out["max"][-1, j0] == np.inf and out["min"][-1, j0] == -np.inf and out["sum"][-1, 0] == np.inf
                assert out["amax"][-1, j0] == lo + 5 and out["amin"][-1, j0] == lo + 600
            # the backward: a NaN gradient word reaches the winner's column and that feature alone
            g = gradients(ops, shape[0], d, 14460 + d, out)
            g["gmax"][2, j0] = np.nan
            bref = BackwardRef(shape, indptr, indices, ops, g)
            for form, gx in (("device", backward_device(mem, na, ops, g, 4)), ("host", backward_host(na, ops, g))):
                bref.check(gx, f"non-finite: a NaN gradient, d {d}, {form} form")
                nan = np.isnan(gx)
                assert nan.sum() == 1 and nan[indices[out["amax"][2, j0]], j0], form


def edges(mem):
    """every pattern of pattern_cases.edge_patterns() and its transpose at d = 1 and 5: nnz = 0 ... 7, runs of empty rows (columns), one row
    (column) that holds all 301 entries, the last row and column, unsorted columns, a pair held twice"""
    for name, rows, cols, indptr, indices in edge_patterns():
        for tname, (r_, c_, ip, ix) in ((name, (rows, cols, indptr, indices)), (name + ", transposed", wc.as_csr_of_the_transpose(rows, cols, indptr, indices))):
            shape = (r_, c_)
            with open_pattern(ip, ix, shape) as na:
                assert na.nnz == ix.size
                for d in (1, 5):
                    X = features(c_, d, 14500 + d)
                    ref = ForwardRef(ip, ix, X)
                    for ops in (SUM, MAX, MEAN | MAX | MIN):
                        what = f"{tname}: {name_of(ops)}, d {d}"
                        host = forward_host(na, X, ops)
                        ref.check(host, ops, what + ", host form")
                        dev = forward_device(mem, na, X, ops, 8, True, what)
                        ref.check(dev, ops, what + ", device form")
                        g = gradients(ops, r_, d, 14510 + d, dev)
                        bref = BackwardRef(shape, ip, ix, ops, g)
                        bref.check(backward_host(na, ops, g), what + ", backward, host form")
                        bref.check(backward_device(mem, na, ops, g, 8, what), what + ", backward, device form")
                        if ix.size == 0:
                            assert (dev["amax"] == NONE).all() if ops & MAX else True


def backward_identities(mem):
    """with gmax = ones the column sums of gx are the number of rows that have entries, per feature; garbage arg words contribute nothing,
    whatever the gradient holds; the MEAN backward is the adjoint of the mean: <gsum, mean(X)> = <gx, X> within the two calls' bounds"""
    indptr, indices = random_pattern(ROWS, COLS, NNZ, 3)
    shape = (ROWS, COLS)
    live_rows = int((np.diff(indptr.astype(np.int64)) > 0).sum())
    with open_pattern(indptr, indices, shape) as na:
        for d in (5, 64):
            X = features(COLS, d, 14600 + d)
            fwd = forward_device(mem, na, X, MAX | MIN, 0, True)
            ones = np.ones((ROWS, d), dtype=np.float32)
            for ops, g in ((MAX, dict(gsum=None, gmax=ones, amax=fwd["amax"], gmin=None, amin=None)), (MIN, dict(gsum=None, gmax=None, amax=None, gmin=ones, amin=fwd["amin"]))):
                for gx in (backward_device(mem, na, ops, g, 0), backward_host(na, ops, g)):
                    assert (gx.astype(np.float64).sum(axis=0) == live_rows).all() and set(np.unique(gx)) <= set(np.arange(ROWS + 1, dtype=np.float32)), (d, ops)
            junk = np.full((ROWS, d), SENTINEL, dtype=np.uint32)
            nans = np.full((ROWS, d), np.nan, dtype=np.float32)
            g = dict(gsum=None, gmax=nans, amax=junk, gmin=nans, amin=np.full((ROWS, d), NONE, dtype=np.uint32))
            for gx in (backward_device(mem, na, MAX | MIN, g, 4), backward_host(na, MAX | MIN, g)):
                assert not gx.view(np.uint32).any(), f"garbage arg words reached gx, d {d}"
            # the adjoint identity of the mean
            G = features(ROWS, d, 14610 + d)
            fref = ForwardRef(indptr, indices, X).part("mean")
            mean = forward_device(mem, na, X, MEAN, 0, True)["sum"]
            fref.check(mean, f"identities: mean, d {d}")
            grads = dict(gsum=G, gmax=None, amax=None, gmin=None, amin=None)
            bref = BackwardRef(shape, indptr, indices, MEAN, grads)
            gx = backward_device(mem, na, MEAN, grads, 0)
            bref.check(gx, f"identities: mean backward, d {d}")
            G64, X64 = G.astype(np.float64), X.astype(np.float64)
            left = math.fsum((mean.astype(np.float64) * G64).ravel().tolist())
            right = math.fsum((gx.astype(np.float64) * X64).ravel().tolist())
            # each side's own error, plus that the backward's E holds the ROUNDED quotients g / n (2^-53 of every term)
            slack = float((fref.bound * np.abs(G64)).sum()) + float(((bref.bound + 2.0 ** -52 * bref.A) * np.abs(X64)).sum())
            exact = [math.fsum((fref.E * G64).ravel().tolist()), math.fsum((bref.E * X64).ravel().tolist())]
            assert abs(exact[0] - exact[1]) <= 1e-9 * max(1.0, abs(exact[0])), exact
            assert abs(left - right) <= slack, (d, left, right, slack)


def nothing_carried_over(mem):
    """hsagg, then hsw_spmm_device at another d, then hsagg again on one object: the words of the first time and of a fresh object; the
    device forms check throughout that the sentinel words beyond d are intact"""
    indptr, indices = random_pattern(ROWS, COLS, NNZ, 4)
    shape = (ROWS, COLS)
    ops = MEAN | MAX | MIN
    with open_pattern(indptr, indices, shape) as na, open_pattern(indptr, indices, shape) as fresh:
        X = features(COLS, 61, 14700)
        f1 = forward_device(mem, na, X, ops, 4, True, "first call")
        ForwardRef(indptr, indices, X).check(f1, ops, "first call")
        g = gradients(ops, ROWS, 61, 14710, f1)
        b1 = backward_device(mem, na, ops, g, 4, "first call")
        BackwardRef(shape, indptr, indices, ops, g).check(b1, "first call, backward")
        w, X2 = wc.operands("spmm", shape, NNZ, 5, 14720, 3.0)
        wc.Reference("spmm", shape, indptr, indices, w, X2).check(wc.device_form(mem, na, "spmm", w, X2, 4, "in between"), "hsw_spmm_device in between")
        X3 = features(COLS, 5, 14730, 3.0)
        f3 = forward_device(mem, na, X3, SUM | MIN, 8, False, "other inputs")
        ForwardRef(indptr, indices, X3).check(f3, SUM | MIN, "other inputs", False)
        assert same_words(f3, forward_device(mem, fresh, X3, SUM | MIN, 8, False))
        assert same_words(f1, forward_device(mem, na, X, ops, 4, True)) and same_words(f1, forward_host(na, X, ops)) and same_words(f1, forward_device(mem, fresh, X, ops, 4, True))
        assert same_words(b1, backward_device(mem, na, ops, g, 4)) and same_words(b1, backward_host(na, ops, g)) and same_words(b1, backward_device(mem, fresh, ops, g, 4))


def large(mem, shape, indptr, indices, d, seed, what):
    """the device forms over one large pattern (GPU tests): MEAN | MAX | MIN forward then backward with the args just written, and SUM
    alone; float64 sums in the references.  Returns (forward reference, backward reference)."""
    X = features(shape[1], d, seed)
    ref = ForwardRef(indptr, indices, X, exact=False)
    ops = MEAN | MAX | MIN
    with open_pattern(indptr, indices, shape) as na:
        fwd = forward_device(mem, na, X, ops, 4, True, what)
        ref.check(fwd, ops, what)
        g = gradients(ops, shape[0], d, seed + 1, fwd)
        bref = BackwardRef(shape, indptr, indices, ops, g, exact=False)
        bref.check(backward_device(mem, na, ops, g, 4, what), what + ", backward")
        ref.check(forward_device(mem, na, X, SUM, 0, True, what), SUM, what + ", SUM alone")
    return ref, bref


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def refusals(mem):
    l = ag.lib()
    vp = C.c_void_p
    indptr, indices = random_pattern(6, 9, 7, 5)
    shape = (6, 9)
    one = np.zeros(4, dtype=np.float32).ctypes.data
    # a null object
    assert l.hsagg_forward_device(None, SUM, vp(one), 4, 1, vp(one), None, None, None, None, 4) == BAD_ARG
    assert l.hsagg_backward_device(None, SUM, vp(one), None, None, None, None, 4, 1, vp(one), 4) == BAD_ARG
    assert l.hsagg_forward(None, SUM, vp(one), 1, vp(one), None, None, None, None) == BAD_ARG
    assert l.hsagg_backward(None, SUM, vp(one), None, None, None, None, 1, vp(one)) == BAD_ARG

    d, full = 5, MEAN | MAX | MIN
    with open_pattern(indptr, indices, shape) as na, open_pattern(indptr, indices, shape, transposed=False) as plain:
        X = features(9, d, 14800)
        want = forward_host(na, X, full)
        ForwardRef(indptr, indices, X).check(want, full, "refusals")
        g = gradients(full, 6, d, 14810, want)
        want_gx = backward_host(na, full, g)
        BackwardRef(shape, indptr, indices, full, g).check(want_gx, "refusals, backward")
        before = na.info()

        def still_usable(rc, what, obj=na, code=BAD_ARG):
            assert rc == code and l.hsw_last_error(obj._h), (what, rc)
            assert same_words(forward_host(obj, X, full), want), f"unusable after {what}"
            if obj is na:
                assert same_words(backward_host(na, full, g), want_gx), f"unusable after {what}"

        def forward_call(a, obj=na):
            return l.hsagg_forward_device(obj._h, a["ops"], vp(a["x"]), a["ldx"], a["d"], vp(a["ysum"]), vp(a["ymax"]), vp(a["amax"]), vp(a["ymin"]), vp(a["amin"]), a["ldy"])

        def backward_call(a, obj=na):
            return l.hsagg_backward_device(obj._h, a["ops"], vp(a["gsum"]), vp(a["gmax"]), vp(a["amax"]), vp(a["gmin"]), vp(a["amin"]), a["ldg"], a["d"], vp(a["gx"]), a["ldgx"])

        # buffers of 9 rows x 16 words (the larger dimension, ld up to 16), 16-byte aligned
        fnames = ("x", "ysum", "ymax", "amax", "ymin", "amin")
        bnames = ("gsum", "gmax", "amax", "gmin", "amin", "gx")
        fb = {n: mem.alloc(np.zeros(9 * 16, np.uint32)) for n in fnames}
        bb = {n: mem.alloc(np.zeros(9 * 16, np.uint32)) for n in bnames}
        okf = dict({n: b.ptr for n, b in fb.items()}, ops=full, ldx=8, ldy=8, d=d)
        okb = dict({n: b.ptr for n, b in bb.items()}, ops=full, ldg=8, ldgx=8, d=d)
        assert forward_call(okf) == 0 and backward_call(okb) == 0
        x, ysum, ymax, amax, ymin, amin = (okf[n] for n in fnames)
        bad_ops = [("ops = 0", dict(ops=0)), ("ops = 16", dict(ops=16)), ("an unknown bit beside a known one", dict(ops=MAX | 0x80000000)), ("SUM | MEAN", dict(ops=SUM | MEAN)),
                   ("SUM | MEAN | MAX", dict(ops=SUM | MEAN | MAX)), ("d = 0", dict(d=0)), ("d = 257", dict(d=257, ldx=260, ldy=260, ldg=260, ldgx=260))]
        fcases = bad_ops + [("null x", dict(x=None)), ("null ysum", dict(ysum=None)), ("null ymax", dict(ymax=None)), ("null ymin", dict(ymin=None)),
                            ("null ysum with SUM", dict(ops=SUM, ysum=None)), ("misaligned x", dict(x=x + 4)), ("misaligned ysum", dict(ysum=ysum + 8)),
                            ("misaligned ymax", dict(ymax=ymax + 4)), ("misaligned amax", dict(amax=amax + 4)), ("misaligned ymin", dict(ymin=ymin + 12)),
                            ("misaligned amin", dict(amin=amin + 8)), ("ldx % 4", dict(ldx=10)), ("ldy % 4", dict(ldy=10)), ("ldx < d", dict(ldx=4)), ("ldy < d", dict(ldy=4)),
                            ("ysum is x", dict(ysum=x)), ("ymax is x", dict(ymax=x)), ("amin inside x", dict(amin=x + 16)), ("ymax is ysum", dict(ymax=ysum)),
                            ("amax is ymax", dict(amax=ymax)), ("ymin inside amax", dict(ymin=amax + 32)), ("amin is amax", dict(amin=amax)),
                            ("ymin starts in x's last row", dict(x=ymin + 16, ymin=ymin + 16 + 8 * 8 * 4))]
        for what, change in fcases:
            still_usable(forward_call(dict(okf, **change)), "forward_device: " + what)
        gsum, gmax, bamax, gmin, bamin, gx = (okb[n] for n in bnames)
        bcases = bad_ops + [("null gsum", dict(gsum=None)), ("null gmax", dict(gmax=None)), ("null amax", dict(amax=None)), ("null gmin", dict(gmin=None)), ("null amin", dict(amin=None)),
                            ("null gx", dict(gx=None)), ("null amax with MAX", dict(ops=MAX, amax=None)), ("misaligned gsum", dict(gsum=gsum + 4)), ("misaligned gmax", dict(gmax=gmax + 8)),
                            ("misaligned amax", dict(amax=bamax + 4)), ("misaligned gmin", dict(gmin=gmin + 4)), ("misaligned amin", dict(amin=bamin + 12)),
                            ("misaligned gx", dict(gx=gx + 4)), ("ldg % 4", dict(ldg=10)), ("ldgx % 4", dict(ldgx=10)), ("ldg < d", dict(ldg=4)), ("ldgx < d", dict(ldgx=4)),
                            ("gx is gsum", dict(gx=gsum)), ("gx is gmax", dict(gx=gmax)), ("gx is amax", dict(gx=bamax)), ("gx inside gmin", dict(gx=gmin + 16)),
                            ("gx starts in amin's last row", dict(gx=bamin + 5 * 8 * 4 + 16))]
        for what, change in bcases:
            still_usable(backward_call(dict(okb, **change)), "backward_device: " + what)
        # outputs whose bit is not set are not looked at, the arg arrays may be NULL, and ranges that touch without sharing a byte are fine
        assert forward_call(dict(okf, ops=SUM, ymax=None, amax=x, ymin=x + 4, amin=None)) == 0
        assert forward_call(dict(okf, amax=None, amin=None)) == 0
        assert forward_call(dict(okf, ymin=ysum + (5 * 8 + 8) * 4)) == 0
        assert backward_call(dict(okb, ops=MIN, gsum=None, gmax=None, amax=None)) == 0
        # the host forms
        hf = {n: np.zeros(9 * 8, np.float32) for n in fnames}
        hb = {n: np.zeros(9 * 8, np.float32) for n in bnames}
        okhf = dict({n: a.ctypes.data for n, a in hf.items()}, ops=full, d=d)
        okhb = dict({n: a.ctypes.data for n, a in hb.items()}, ops=full, d=d)

        def forward_host_call(a, obj=na):
            return l.hsagg_forward(obj._h, a["ops"], vp(a["x"]), a["d"], vp(a["ysum"]), vp(a["ymax"]), vp(a["amax"]), vp(a["ymin"]), vp(a["amin"]))

        def backward_host_call(a, obj=na):
            return l.hsagg_backward(obj._h, a["ops"], vp(a["gsum"]), vp(a["gmax"]), vp(a["amax"]), vp(a["gmin"]), vp(a["amin"]), a["d"], vp(a["gx"]))

        assert forward_host_call(okhf) == 0 and backward_host_call(okhb) == 0
        host_ops = [("ops = 0", dict(ops=0)), ("ops = 32", dict(ops=32)), ("SUM | MEAN", dict(ops=SUM | MEAN)), ("d = 0", dict(d=0)), ("d = 257", dict(d=257))]
        for what, change in host_ops + [(f"null {n}", {n: None}) for n in ("x", "ysum", "ymax", "ymin")] + [("ysum is x", dict(ysum=okhf["x"])), ("amax inside ymax", dict(amax=okhf["ymax"] + 8)),
                                                                                                        ("ymin is ysum", dict(ymin=okhf["ysum"])), ("amin inside x", dict(amin=okhf["x"] + 20))]:
            still_usable(forward_host_call(dict(okhf, **change)), "forward: " + what)
        for what, change in host_ops + [(f"null {n}", {n: None}) for n in bnames] + [("gx is gsum", dict(gx=okhb["gsum"])), ("gx inside amax", dict(gx=okhb["amax"] + 8)),
                                                                                   ("gx is gmin", dict(gx=okhb["gmin"]))]:
            still_usable(backward_host_call(dict(okhb, **change)), "backward: " + what)
        assert forward_host_call(dict(okhf, amax=None, amin=None)) == 0
        # the backward on an object created without HSW_TRANSPOSED, in both forms; its forward runs
        still_usable(backward_call(okb, plain), "backward_device without HSW_TRANSPOSED", plain, UNSUPPORTED)
        assert b"HSW_TRANSPOSED" in l.hsw_last_error(plain._h)
        still_usable(backward_host_call(okhb, plain), "backward without HSW_TRANSPOSED", plain, UNSUPPORTED)
        assert forward_call(okf, plain) == 0
        # the messages name the rule, and hsw_info is what it was
        assert forward_call(dict(okf, ops=SUM | MEAN)) == BAD_ARG and b"HSAGG_MEAN" in l.hsw_last_error(na._h)
        assert forward_call(dict(okf, ymax=ysum)) == BAD_ARG and b"overlaps" in l.hsw_last_error(na._h)
        assert na.info() == before
        for obj in (na, plain):
            obj.set_stream(None)
            obj.sync()

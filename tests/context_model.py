"""A model of one hs_context as a caller sees it, a seeded generator of entry-point sequences, and a driver that plays a sequence on an
engine and compares every buffer the caller can observe with the model (a test helper, like cases.py and float_contract.py: no device
code here).  tests/test_context_model_cpu.py runs it against the oracle, a fake engine with planted defects and libhisparse_cpu.so;
tests/test_gpu_sequences.py runs it on the device.  docs/sequence_tests.md records the plans, seeds and what the runs showed.

The model states the CONTRACT of include/hisparse_hip.h, not the implementation: it knows nothing of CarriedCombine, of the batch graph
cache or of any scratch buffer.  It holds the loaded matrix (the stored elements, padded as the load pads them), the CSC matrix of the
SpMSpV extension (separately: it may be another matrix and value updates do not touch it), the bindings, the stream's ownership, and the
full expected contents of every buffer a caller can look at: the library's x and y, the caller's result buffers A and B, the caller's
vector buffer V, the SpMSpV result, the push targets P0 and P1 and the SpMM blocks.

ARITHMETIC.  Fixed point is exact integers: a product is min((a b + 2^23) >> 24, 2^32 - 1), a row min(sum, 2^32 - 1); sums do not depend
on the order, so column slices, passes and partitions change nothing.  In the float modes the model cannot predict words: a write of a
product A x leaves a PENDING segment (matrix, x, rounding class); at the next observation the device's words are checked against
float_contract.Reference with the route's class, against the oracle to 1e-4, and bit for bit against the words the same product gave
earlier on the same route; then the device's words are adopted, so that everything afterwards (feedback, in-place runs, a later
comparison of an untouched buffer) is bit exact again.

OBSERVATION.  On the library's own, un-shared stream a result may be looked at only after a settling call (hs_sync, hs_read_result,
hs_push_result, hs_get_stream) with no step since; on a caller-owned or handed-out stream a hipStreamSynchronize is enough.  At every
observation ALL tracked buffers are compared.
"""
import os
import re
from collections import namedtuple

import numpy as np
import scipy.sparse as sp

from hisparse_amd import device, host

import cases
import float_contract as fc

SAT = 0xFFFFFFFF
GUARD_WORDS = 64
GUARD = 0xDEADBEEF
PATTERN = (0x00C00000, 0x3F000000, 0x3F000000)      # caller-owned buffers start as PATTERN[impl] + index: a word that moves shows, and read as
                                                    # values (hs_feedback from a target no step has written) they are 0.75 ... / 0.5 ...
OB_BANK, VB_BANK = 8, 4096    # 1024 rows per row partition (several partitions at 2,500 rows), 32768 columns per column partition
FIXED_SCALE, FIXED_SHIFT = 0.5, 0.25       # hs_feedback / hs_iterate: x = 0.5 y + 0.25 keeps x in (0.25, ~2) while y stays near 1
FLOAT_SCALE, FLOAT_SHIFT = 0.0625, 0.25
BAD_ARG, HIP_ERROR, NOT_LOADED, UNSUPPORTED = -1, -3, -5, -6


class Mismatch(AssertionError):
    pass


class DeviceFault(RuntimeError):
    """an unexpected HS_ERR_HIP: nothing more may be started on the device"""


# ---- arithmetic --------------------------------------------------------------------------------------------------------------------
def q_mul(a, b):
    """Q8.24 product of value words, AP_RND / AP_SAT: min((a b + 2^23) >> 24, 2^32 - 1).  (2^32 - 1)^2 + 2^23 < 2^64: no wrap."""
    p = (np.asarray(a, dtype=np.uint64) * np.asarray(b, dtype=np.uint64) + np.uint64(1 << 23)) >> np.uint64(24)
    return np.minimum(p, np.uint64(SAT))


def _segment_sums(p, indptr, rows, dtype):
    y = np.zeros(rows, dtype=dtype)
    n = np.diff(indptr)
    if p.size:
        y[n > 0] = np.add.reduceat(p, indptr[:-1][n > 0])
    return y


def feedback_words(impl, y_words, x_words, scale, shift):
    """hs_feedback: x[i] = scale (*) y[i] (+) shift for i < min(len(y), len(x)); the rest of x keeps its value"""
    n = min(len(y_words), len(x_words))
    out = np.array(x_words, dtype=np.uint32)
    if impl == 0:
        out[:n] = np.minimum(q_mul(y_words[:n], np.uint64(scale)) + np.uint64(shift), np.uint64(SAT)).astype(np.uint32)
    else:
        s, b = np.uint32(scale).view(np.float32), np.uint32(shift).view(np.float32)
        with np.errstate(all="ignore"):
            out[:n] = ((s * np.asarray(y_words[:n], dtype=np.uint32).view(np.float32)).astype(np.float32) + b).astype(np.float32).view(np.uint32)
    return out


class Mat:
    """The stored elements of a matrix in its PADDED shape (CSR), with the value words of the numeric mode.  Immutable."""
    _next = [0]

    def __init__(self, impl, rows, cols, indptr, indices, data):
        self.impl, self.rows, self.cols = impl, int(rows), int(cols)
        self.indptr = np.asarray(indptr, dtype=np.int64)
        self.indices = np.asarray(indices, dtype=np.int64)
        self.data = np.ascontiguousarray(data, dtype=np.float32)
        self.words = host.pack_vector(impl, self.data) if self.data.size else np.zeros(0, dtype=np.uint32)   # csr_matrix_convert_from_float
        Mat._next[0] += 1
        self.key = Mat._next[0]
        self._cp = self._t = None

    @classmethod
    def from_scipy(cls, impl, m, rows=None, cols=None):
        m = m.tocsr()
        m.sort_indices()
        rows, cols = rows or m.shape[0], cols or m.shape[1]
        indptr = np.concatenate([m.indptr.astype(np.int64), np.full(rows - m.shape[0], m.indptr[-1], dtype=np.int64)])
        return cls(impl, rows, cols, indptr, m.indices, m.data)

    @property
    def nnz(self):
        return int(self.indptr[-1])

    def scipy(self):
        return sp.csr_matrix((self.data, self.indices, self.indptr), shape=(self.rows, self.cols))

    def with_data(self, data):
        return Mat(self.impl, self.rows, self.cols, self.indptr, self.indices, data)

    def transposed(self):
        """the CSR of the transpose, rows of the original ascending inside a column (csr2csc's order)"""
        if self._t is None:
            t = self.scipy().T.tocsr()
            t.sort_indices()
            self._t = Mat.from_scipy(self.impl, t)
        return self._t

    def spmv(self, x_words):
        """y = A x as value words: exact in fixed point; in the float modes fp32 products summed in double, rounded once (class L = 1)"""
        x_words = np.asarray(x_words, dtype=np.uint32)[: self.cols]
        if self.impl == 0:
            s = _segment_sums(q_mul(self.words, x_words[self.indices]), self.indptr, self.rows, np.uint64)
            return np.minimum(s, np.uint64(SAT)).astype(np.uint32)
        with np.errstate(all="ignore"):
            p = (self.data * x_words.view(np.float32)[self.indices]).astype(np.float64)
            return _segment_sums(p, self.indptr, self.rows, np.float64).astype(np.float32).view(np.uint32)

    def cp(self):
        """the matrix as channel packets (for the oracle)"""
        if self._cp is None:
            csr = host.CSRMatrix.from_arrays(self.rows, self.cols, self.indptr, self.indices, self.data)
            self._cp = host.format_matrix(csr, self.impl, vb_bank=VB_BANK, ob_bank=OB_BANK, skip_empty_rows=True)
            assert (self._cp.num_rows, self._cp.num_cols) == (self.rows, self.cols)
        return self._cp

    def oracle_spmv(self, x_words):
        from oracle import oracle as orc
        cp = self.cp()
        return orc.spmv(self.impl, [cp.channel(c) for c in range(16)], np.asarray(x_words, dtype=np.uint32)[: self.cols], cp.num_rows,
                        cp.num_cols, cp.num_row_partitions, cp.num_col_partitions, cp.ob_bank, cp.vb_bank)


def spmspv_words(t, num_rows, index, words):
    """y = A x for x = {(index[k], words[k])} over A given as t = Mat of A^T (row c of t = column c of A); repeated entries add up"""
    index = np.asarray(index, dtype=np.int64)
    words = np.asarray(words, dtype=np.uint32)
    lens = t.indptr[index + 1] - t.indptr[index]
    total = int(lens.sum())
    if not total:
        return np.zeros(num_rows, dtype=np.uint32)
    e = np.repeat(t.indptr[index] - (np.cumsum(lens) - lens), lens) + np.arange(total)
    xv = np.repeat(words, lens)
    if t.impl == 0:
        y = np.zeros(num_rows, dtype=np.uint64)
        np.add.at(y, t.indices[e], q_mul(t.words[e], xv))
        return np.minimum(y, np.uint64(SAT)).astype(np.uint32)
    y = np.zeros(num_rows, dtype=np.float64)
    with np.errstate(all="ignore"):
        np.add.at(y, t.indices[e], (t.data[e] * xv.view(np.float32)).astype(np.float64))
        return y.astype(np.float32).view(np.uint32)


# ---- buffers -----------------------------------------------------------------------------------------------------------------------
# A pending product (float modes): words [lo, hi) of a buffer hold rows [row0, row0 + hi - lo) of  m x  (m: scipy CSR, x: float32),
# within the bound of L chained fp32 additions and S partials; key: what makes two products the same words (matrix, x, route).
Prov = namedtuple("Prov", "m x L S exact key oracle")
# x[lo, hi) = scale * y + shift of the words buffer `src` holds at the next observation (float hs_feedback)
Fed = namedtuple("Fed", "src scale shift")


class Buf:
    def __init__(self, name, words):
        self.name = name
        self.w = words                 # uint32, the expected contents (a view into fake device memory when a fake engine owns the model)
        self.pend = []                 # [(lo, hi, row0, Prov | Fed)]
        self.product = False           # a whole SpMV has been written here (the input condition looks at such buffers only)

    def clear(self, lo, hi):
        keep = []
        for a, b, r0, p in self.pend:
            if b <= lo or a >= hi:
                keep.append((a, b, r0, p))
                continue
            if a < lo:
                keep.append((a, lo, r0, p))
            if b > hi:
                keep.append((hi, b, r0 + (hi - a), p))
        self.pend = keep

    def put(self, lo, words):
        self.clear(lo, lo + len(words))
        self.w[lo: lo + len(words)] = words

    def put_pending(self, lo, hi, row0, prov):
        self.clear(lo, hi)
        self.pend.append((lo, hi, row0, prov))

    def pending(self, lo=0, hi=None):
        hi = len(self.w) if hi is None else hi
        return any(a < hi and b > lo for a, b, _, _ in self.pend)

    def copy_from(self, src, n, dst_lo=0):
        """words [0, n) of src, pending segments included, to [dst_lo, dst_lo + n) of this buffer"""
        if src is self and dst_lo == 0:
            return
        self.put(dst_lo, src.w[:n].copy())
        for a, b, r0, p in src.pend:
            if a < n:
                self.pend.append((dst_lo + a, dst_lo + min(b, n), r0, p))


class _Faults:
    def __init__(self, player):
        self.player = player

    def __enter__(self):
        return self

    def __exit__(self, kind, e, tb):
        if isinstance(e, device.DeviceError) and e.code == HIP_ERROR:
            p = self.player
            raise DeviceFault(f"{p.label}: HS_ERR_HIP at op {len(p.done) - 1} {p.done[-1:]}: {e}\n{p.replay()}") from e
        return False


class Refused(Exception):
    def __init__(self, code):
        super().__init__(f"refused with {code}")
        self.code = code


class Model:
    """concrete = True: the float modes compute words too (class L = 1: the reference a fake engine hands out)."""

    def __init__(self, impl, concrete=False):
        self.impl, self.concrete = impl, concrete or impl == 0
        self.bufs = {}
        self.mat = None
        self.parts = []
        self.info = {}
        self.perm = None                     # update_values: values in the caller's order -> the order of the held matrix
        self.csc = None                      # Mat of the CSC matrix's transpose (row c = column c)
        self.csc_rows = 0
        self.x_bound = self.y_bound = None   # names of caller buffers
        self.x_len = 0
        self.caller_stream = False
        self.shared = False
        self.dirty = False                   # a step since the last settling call
        self.options = {}
        self.overflow = False

    # ---- helpers ----
    def add(self, name, words):
        self.bufs[name] = Buf(name, words)
        return self.bufs[name]

    @property
    def x_src(self):
        return self.bufs[self.x_bound or "x"]

    @property
    def y_dst(self):
        return self.bufs[self.y_bound or "y"]

    @property
    def private(self):
        return not self.caller_stream and not self.shared

    def observable(self):
        return not (self.private and self.dirty)

    def settle(self):
        self.dirty = False

    def ready(self):
        if self.mat is None:
            raise Refused(NOT_LOADED)
        if not self.x_bound and ("x" not in self.bufs or self.x_len != self.mat.cols):
            raise Refused(NOT_LOADED)

    def _product(self, mat, x_words, route, L=None, S=None, exact=False):
        """('w', words) or ('p', Prov) for mat x"""
        x_words = np.array(x_words[: mat.cols], dtype=np.uint32)
        if self.concrete:
            return "w", mat.spmv(x_words)
        L = self.info.get("L", 1) if L is None else L
        S = self.info.get("slices", 1) if S is None else S
        key = (mat.key, hash(x_words.tobytes()), route)
        return "p", Prov(mat, x_words.view(np.float32), L, S, exact, key, lambda: mat.oracle_spmv(x_words))

    def _write(self, buf, lo, hi, row0, product):
        kind, v = product
        if kind == "w":
            buf.put(lo, v[row0: row0 + hi - lo])
        else:
            buf.put_pending(lo, hi, row0, v)

    def _step(self, route="spmv"):
        x, y = self.x_src, self.y_dst
        assert not x.pending(0, self.mat.cols), "the generator / driver observe before a run reads a pending x"
        self._write(y, 0, self.mat.rows, 0, self._product(self.mat, x.w, route))
        y.product = True
        self.dirty = True

    # ---- the boundary ----
    def load(self, mat, info=None, perm=None):
        self.mat, self.info, self.perm = mat, dict(info or {}), perm
        ob = 128 * OB_BANK
        self.parts = [(lo, min(lo + ob, mat.rows)) for lo in range(0, mat.rows, ob)]
        self.add("y", np.zeros(mat.rows, dtype=np.uint32))      # the load zero-initialises y; a bound result is unbound
        self.y_bound = None
        self.dirty = False

    def load_vector(self, words):
        words = np.asarray(words, dtype=np.uint32)
        if self.mat is not None and len(words) != self.mat.cols:
            raise Refused(BAD_ARG)
        if "x" not in self.bufs or len(self.bufs["x"].w) != len(words):      # (only the words of the last load are the caller's to look at)
            self.add("x", np.zeros(len(words), dtype=np.uint32))
        self.bufs["x"].put(0, words)
        self.x_len = len(words)

    def run(self):
        self.ready()
        self._step()

    def run_batch(self, steps):
        self.ready()
        for _ in range(steps):
            self._step()
        if steps and not self.private:
            self.dirty = False

    def run_partition(self, j, part_len):
        self.ready()
        if j >= len(self.parts):
            raise Refused(BAD_ARG)
        lo, hi = self.parts[j]
        if part_len != (hi - lo) // 16:
            raise Refused(BAD_ARG)
        x, y = self.x_src, self.y_dst
        assert not x.pending(0, self.mat.cols)
        self._write(y, lo, hi, lo, self._product(self.mat, x.w, "part"))
        self.dirty = True

    def feedback(self, scale, shift):
        self.ready()
        x, y = self.x_src, self.y_dst
        n = min(self.mat.rows, self.mat.cols)
        if y.pending(0, n):
            assert x is not y
            x.put_pending(0, n, 0, Fed(y.name, scale, shift))
        else:
            x.put(0, feedback_words(self.impl, y.w[:n], x.w[:n], scale, shift))

    def iterate(self, n, scale, shift):
        self.ready()
        for _ in range(n):
            self._step()
            self.feedback(scale, shift)

    def bind_vector(self, name):
        self.x_bound = name

    def bind_result(self, name):
        self.y_bound = name

    def set_stream(self, caller):
        self.caller_stream = bool(caller)         # (not a settling call of the header's list: `dirty` stays as it is)

    def get_stream(self):
        self.shared = True
        self.dirty = False

    def push(self, names, num_words):
        if self.mat is None:
            raise Refused(NOT_LOADED)
        if num_words > self.mat.rows or num_words % 4:
            raise Refused(BAD_ARG)
        for name in names:
            self.bufs[name].copy_from(self.y_dst, num_words)
        self.dirty = False

    def time_runs(self):
        self.ready()
        self._step()
        self.dirty = False

    time_kernel = time_runs

    def set_option(self, key, value):
        if key.lower() not in ("batch_graph", "iterate_graph", "spmm_fused", "spmm_mfma", "spmspv", "spmspv_crossover", "value_map",
                               "stream_format", "col_slices", "light", "carry_combine", "spmm_vectors"):
            raise Refused(BAD_ARG)
        if value in (None, ""):
            self.options.pop(key.lower(), None)
        else:
            self.options[key.lower()] = str(value)

    def update_values(self, values):
        if self.mat is None:
            raise Refused(NOT_LOADED)
        if not self.info.get("value_map"):
            raise Refused(UNSUPPORTED)
        if len(values) != self.mat.nnz:
            raise Refused(BAD_ARG)
        values = np.asarray(values, dtype=np.float32)
        self.mat = self.mat.with_data(values if self.perm is None else values[self.perm])

    # ---- SpMM ----
    def spmm_routes(self, k):
        """per column of one hs_spmm call: (route, L, S, exact) in the float modes (hs_spmm.cpp's dispatch, from hisparse_hip.h)"""
        fmt, slices = self.info.get("fmt"), self.info.get("slices", 1)
        fused = self.options.get("spmm_fused") != "0"
        out, j = [], 0
        if fused and self.options.get("spmm_mfma") != "0" and self.info.get("mfma") and self.impl != 0:
            while k - j >= 5:
                v = min(16, k - j)
                out += [(("mfma", k, j + i), "n+1", 1, True) for i in range(v)]
                j += v
        for i in range(j, k):
            if fmt == "bitmap":
                out.append((("bitmap", k, i, fused), 8, slices, False))
            elif fmt == "sweep" and self.info.get("spmm_vectors") == 4 and fused:
                out.append((("sweep4", k, i), 1, slices, False))
            else:
                out.append(("spmv", None, None, False))
        return out

    def spmm_columns(self, X):
        """products for the k columns of X (k x cols words)"""
        cols = []
        for j, (route, L, S, exact) in enumerate(self.spmm_routes(len(X))):
            if L == "n+1":
                L = np.diff(self.mat.indptr) + 1
            cols.append(self._product(self.mat, X[j], route, L, S, exact))
        return cols

    def spmm_device(self, xname, ldx, yname, ldy, k):
        if self.mat is None:
            raise Refused(NOT_LOADED)
        if ldx % 4 or ldy % 4 or ldx < self.mat.cols or ldy < self.mat.rows:
            raise Refused(BAD_ARG)
        xb, yb = self.bufs[xname], self.bufs[yname]
        X = [xb.w[j * ldx: j * ldx + self.mat.cols] for j in range(k)]
        for j, product in enumerate(self.spmm_columns(X)):
            self._write(yb, j * ldy, j * ldy + self.mat.rows, 0, product)

    # ---- SpMSpV ----
    def load_csc(self, t, num_rows):
        self.csc, self.csc_rows = t, num_rows
        self.add("sy", np.zeros(num_rows, dtype=np.uint32))
        self.overflow = False

    def same_both_ways(self):
        """the CSC matrix is the loaded matrix (the caller's contract under spmspv = auto | dense)"""
        if self.csc is None or self.mat is None:
            return False
        a, b = self.mat.transposed(), self.csc
        return (a.rows == (b.rows + 7) // 8 * 8 and a.nnz == b.nnz and np.array_equal(a.indptr[: b.rows + 1], b.indptr)
                and np.array_equal(a.indices, b.indices) and np.array_equal(a.words, b.words))

    def spmspv_path(self, index):
        index = np.asarray(index, dtype=np.int64)
        repeats = len(np.unique(index)) != len(index)
        row_div = 128 * (8 if self.impl == 2 else 1)
        possible = (not repeats and self.mat is not None and self.mat.cols == (self.csc.rows + 7) // 8 * 8
                    and self.mat.rows == -(-self.csc_rows // row_div) * row_div)
        force, cross = self.options.get("spmspv"), self.options.get("spmspv_crossover")
        dense = False
        if force in ("sparse", "dense"):
            dense = force == "dense"
        elif cross is not None:
            dense = float(cross) > 0 and len(index) > float(cross) * self.csc.rows
        elif force == "auto" and possible:
            lens = self.csc.indptr[index + 1] - self.csc.indptr[index]
            assert 14.0 + float(lens.sum()) / 45000.0 <= 30.0, "the generator keeps spmspv = auto below the timed rule"
        return "dense" if dense and possible else "sparse"

    def spmspv(self, index, words):
        if self.csc is None:
            raise Refused(NOT_LOADED)
        index = np.asarray(index, dtype=np.int64)
        words = np.asarray(words, dtype=np.uint32)
        if len(index) and index.max() >= self.csc.rows:
            raise Refused(BAD_ARG)
        sy = self.bufs["sy"]
        if self.spmspv_path(index) == "dense":
            x = np.zeros(self.mat.cols, dtype=np.uint32)
            x[index] = words
            self._write(sy, 0, self.csc_rows, 0, self._product(self.mat, x, "spmspv-dense"))
        elif self.concrete:
            sy.put(0, spmspv_words(self.csc, self.csc_rows, index, words))
        elif not len(index):
            sy.put(0, np.zeros(self.csc_rows, dtype=np.uint32))
        else:
            passes = int(np.unique(index, return_counts=True)[1].max())
            csc, rows = self.csc, self.csc_rows
            a = csc.scipy().T.tocsc()[:, index].tocsr()[:rows]      # one column per ENTRY: every entry is its own product
            a.sort_indices()
            key = (csc.key, hash(index.tobytes() + words.tobytes()), "spmspv")

            def oracle():
                from oracle import oracle as orc
                return orc.spmspv(self.impl, csc.indptr.astype(np.uint32), csc.indices.astype(np.uint32), csc.words, rows, csc.rows,
                                  index.astype(np.uint32), words)
            sy.put_pending(0, rows, 0, Prov(_Raw(a), words.view(np.float32).copy(), 1, passes, False, key, oracle))

    def spmspv_device(self, index, words, overflow=False):
        if self.csc is None:
            raise Refused(NOT_LOADED)
        if overflow:                          # every column named three times: every bin that holds a product overflows, its rows are zero
            self.bufs["sy"].put(0, np.zeros(self.csc_rows, dtype=np.uint32))
            self.overflow = True
            return
        saved = dict(self.options)
        self.options.update(spmspv="sparse")  # no dense dispatch from device entries
        self.options.pop("spmspv_crossover", None)
        try:
            self.spmspv(index, words)
        finally:
            self.options = saved


class _Raw:
    """a scipy matrix where Prov wants a Mat"""
    def __init__(self, m):
        self._m = m

    def scipy(self):
        return self._m


# ---- plans -------------------------------------------------------------------------------------------------------------------------
# name, rows x cols at density (of the matrix as the engine holds it), the options set before the load, the float_contract.chain variant,
# and what hs_get_stats must report: format (None: any known one), column slices (None: whatever the plan takes; 0: more than one), light.
Plan = namedtuple("Plan", "name rows cols density options chain fmt slices light")
PLANS = [
    Plan("pairs-1", 2500, 4000, 0.01, dict(stream_format="pairs", light="0", col_slices="1"), "pairs", "pairs", 1, 0),
    Plan("pairs-4-carry", 3000, 33000, 0.003, dict(stream_format="pairs", light="0", col_slices="4", carry_combine="1"), "pairs", "pairs", 4, 0),
    Plan("delta-3-carry", 3000, 33000, 0.003, dict(stream_format="delta", light="0", col_slices="3", carry_combine="1"), "delta", "delta", 3, 0),
    Plan("owner24-5-carry", 3000, 33000, 0.0003, dict(stream_format="owner24", light="0", col_slices="5", carry_combine="1"), "owner24", "owner24", 5, 0),
    Plan("sweep-spmm4", 3000, 33000, 0.003, dict(stream_format="sweep", spmm_vectors="4", col_slices="3", carry_combine="1"), "sweep", "sweep", 3, 0),
    Plan("bitmap", 300, 9000, 0.2, dict(stream_format="bitmap"), "bitmap", "bitmap", 1, 0),
    Plan("bitmap-sliced", 200, 9000, 0.2, dict(stream_format="bitmap", col_slices="4", carry_combine="1"), "bitmap", "bitmap", 0, 0),
    Plan("light", 3000, 20000, 0.005, dict(light="1"), "light", "pairs", 1, 1),
    Plan("planner", 3000, 20000, 0.01, dict(), None, None, None, None),
    Plan("square-inplace", 9216, 9216, 0.003, dict(stream_format="pairs", light="0", col_slices="2", carry_combine="1"), "pairs", "pairs", 2, 0),
]
PLAN = {p.name: p for p in PLANS}
TWO_ENGINES = ("pairs-4-carry", "bitmap")
IMPLS = (0, 1, 2)
SEEDS = (0, 1, 2)            # seed 0: hs_load_matrix_csr with value_map = 1; 1: hs_load_matrix (CPSR); 2: hs_load_matrix_csr_transposed, value_map = 1
LENGTH = 50
ALT_COLS = 64                # the reloaded "other" matrix has this many columns more


def load_kind(seed):
    return ("csr", "cpsr", "transposed")[seed % 3]


_MATS = {}


def _scaled(impl, data, mean_row):
    """Values that keep y = A x at x's magnitude, so that feedback, iterate and in-place runs stay in range over a whole sequence: fixed
    point (0.085, 1.8) / the mean row length (a row's sum stays near x's mean, far from 2^8); float N(0, 1) / its square root (a row's sum
    has x's deviation: the oracle's absolute 1e-4 keeps its meaning)."""
    if impl == 0:
        return (0.1 + data) * 0.85 / max(1.0, mean_row)
    return data / np.sqrt(max(1.0, mean_row))


def plan_matrix(plan, impl, alt=False):
    """The plan's matrix (alt: the one with another column count) as a Mat in padded shape: shared, read-only.  Values: _scaled (the
    input condition of tests/test_context_model_cpu.py)."""
    key = (plan.name, impl, alt)
    if key not in _MATS:
        cols = plan.cols + (ALT_COLS if alt else 0)
        # (cases.random_csr's values; the pattern drawn here, because scipy.sparse.random takes seconds at 10^8 positions)
        rng = np.random.default_rng(1000 + 7 * sum(map(ord, plan.name)) + alt)
        flat = np.sort(rng.choice(plan.rows * cols, size=int(plan.density * plan.rows * cols), replace=False))
        data = rng.uniform(0.0, 2.0, flat.size) if impl == 0 else rng.normal(0.0, 1.0, flat.size)
        data = _scaled(impl, data, flat.size / plan.rows)
        m = sp.csr_matrix((data.astype(np.float32), (flat // cols, flat % cols)), shape=(plan.rows, cols))
        div = 128 * (8 if impl == 2 else 1)
        _MATS[key] = Mat.from_scipy(impl, m, -(-plan.rows // div) * div, -(-cols // 8) * 8)
    return _MATS[key]


def x_words(impl, n, seed):
    return host.pack_vector(impl, cases.random_x(n, 5000 + seed, impl))


def new_values(impl, mat, seed):
    """values for hs_update_values in the distribution of the plan's matrix"""
    rng = np.random.default_rng(9000 + seed)
    data = rng.uniform(0.0, 2.0, mat.nnz) if impl == 0 else rng.normal(0.0, 1.0, mat.nnz)
    return _scaled(impl, data, mat.nnz / plan_rows(mat)).astype(np.float32)


def plan_rows(mat):
    return max(1, int((np.diff(mat.indptr) > 0).sum()))


def scale_shift(impl):
    s, b = (FIXED_SCALE, FIXED_SHIFT) if impl == 0 else (FLOAT_SCALE, FLOAT_SHIFT)
    w = host.pack_vector(impl, np.array([s, b], dtype=np.float32))
    return int(w[0]), int(w[1])


# ---- the operations ----------------------------------------------------------------------------------------------------------------
# An op is a tuple of Python literals (name, args...): a printed sequence is replayable.  Arrays are named by seeds.
OPS = {
    "load_vector": "hs_load_vector",
    "run": "hs_run",
    "run_batch": "hs_run_batch",
    "run_partition": "hs_run_partition",
    "read_result": "hs_read_result",
    "sync_copy": "hs_sync",
    "bind_result": "hs_bind_device_result",
    "bind_vector": "hs_bind_device_vector",
    "set_stream": "hs_set_stream",
    "get_stream": "hs_get_stream",
    "feedback": "hs_feedback",
    "iterate": "hs_iterate",
    "set_option": "hs_set_option",
    "spmm": "hs_spmm",
    "spmm_device": "hs_spmm_device",
    "load_csc": "hs_load_matrix_csc",
    "spmspv": "hs_spmspv",
    "spmspv_device": "hs_spmspv_device",
    "spmspv_overflow": "hs_spmspv_status",
    "update_values": "hs_update_values",
    "update_values_device": "hs_update_values_device",
    "reload": "hs_load_matrix_csr",
    "time_runs": "hs_time_runs",
    "time_kernel": "hs_time_kernel",
    "push_result": "hs_push_result",
    "refused": None,
}
REFUSALS = ("part_len", "row_part_id", "spmspv_column", "update_nnz", "misaligned_result", "misaligned_vector", "unknown_option", "not_loaded")
# entry points the ops reach without being named after them
ALSO_REACHED = {
    "hs_load_matrix": "reload and the first load, on the seeds that load CPSR",
    "hs_load_matrix_csr_transposed": "reload and the first load, on one seed per plan",
    "hs_read_spmspv_result": "every observation once a CSC matrix is loaded; BAD_ARG after spmspv_overflow",
    "hs_device_vector": "every load_vector: the raw copies of the library's x go through it",
    "hs_device_result": "every load: the raw copies of the library's y go through it",
    "hs_get_stats": "every load: the plan is asserted through it",
    "hs_last_error": "every DeviceError carries it",
}
# ... and the ones that stay outside the sequences, with the reason (the ratchet of tests/test_context_model_cpu.py)
EXCLUDED_ENTRY_POINTS = {
    "hs_create": "the life of the engine a sequence runs on",
    "hs_destroy": "the life of the engine a sequence runs on",
    "hs_strerror": "no context state",
    "hs_debug_read_tiles": "debug read of the image: tests/test_gpu_option_matrix.py, tests/test_gpu_retile.py",
    "hs_debug_read_mfma_image": "debug read: used once per load to learn whether the plan has the matrix engine's image, not an op",
    "hs_tiles_build": "host only, no context", "hs_tiles_info": "host only, no context", "hs_tiles_copy": "host only, no context",
    "hs_tiles_mfma": "host only, no context", "hs_tiles_free": "host only, no context", "hs_tiles_last_error": "host only, no context",
}
EXCLUDED_METHODS = {
    "close": "hs_destroy", "stats": "hs_get_stats: read at every load, not an op", "read_tiles": "debug read", "read_mfma_image": "debug read",
    "device_vector": "used by the driver at every load_vector", "device_result": "used by the driver at every load",
    "load_matrix": "the first load and reload (CPSR seeds)", "load_matrix_csr": "the first load and reload (CSR seeds)",
    "spmspv_async": "hs_spmspv without the read: what the spmspv op calls", "read_spmspv_result": "part of every observation",
    "load_matrix_csc": "op load_csc", "bind_device_result": "op bind_result", "bind_device_vector": "op bind_vector", "sync": "op sync_copy",
}

# the ordered pairs behind the ADVICE findings of rounds 3 to 5 (first op, second op): predicates over ops
PAIRS = {
    "run -> run_partition": (lambda a: a[0] == "run", lambda b: b[0] == "run_partition"),
    "run -> bind_device_result": (lambda a: a[0] == "run", lambda b: b[0] == "bind_result"),
    "run -> spmm": (lambda a: a[0] == "run", lambda b: b[0] in ("spmm", "spmm_device")),
    "run -> spmspv(auto)": (lambda a: a[0] == "run", lambda b: b[0] == "spmspv" and b[3] == "auto"),
    "run -> update_values": (lambda a: a[0] == "run", lambda b: b[0] in ("update_values", "update_values_device")),
    "run -> reload": (lambda a: a[0] == "run", lambda b: b[0] == "reload"),
    "run_batch(graph) -> bind_*": (lambda a: a[0] == "run_batch" and a[2], lambda b: b[0] in ("bind_result", "bind_vector")),
    "run_batch(graph) -> set_option": (lambda a: a[0] == "run_batch" and a[2], lambda b: b[0] == "set_option"),
    "run -> set_stream": (lambda a: a[0] == "run", lambda b: b[0] == "set_stream"),
    "spmspv overflow -> spmspv": (lambda a: a[0] == "spmspv_overflow", lambda b: b[0] in ("spmspv", "spmspv_device")),
    "run -> feedback": (lambda a: a[0] == "run", lambda b: b[0] == "feedback"),
    "run -> iterate": (lambda a: a[0] == "run", lambda b: b[0] == "iterate"),
}
MAX_SPMM_DEVICE, MAX_UPDATE_DEVICE, MAX_SPMSPV_DEVICE = 3, 3, 12      # each call gets memory no earlier call of the sequence may still read


def generate(plan, impl, seed, length=LENGTH, flavour="full"):
    """A seeded op sequence for one engine.  flavour: "full"; "shared" (the stream is preset by the two-engine test: no stream ops);
    "cpu" (what libhisparse_cpu.so implements).  The generator keeps a shadow of what decides which ops are LEGAL (the contract of
    hisparse_hip.h) -- never of what the results are."""
    rng = np.random.default_rng([seed, impl, sum(map(ord, plan.name)), {"full": 0, "shared": 1, "cpu": 2}[flavour]])
    csr_family = load_kind(seed) != "cpsr"
    fixed = impl == 0
    div = 128 * (8 if impl == 2 else 1)
    parts = -(-(-(-plan.rows // div) * div) // (128 * OB_BANK))
    square = plan.name == "square-inplace"
    s = dict(alt=False, x_ok=False, x_bound=False, y_bound=None, csc=False, csc_same=False, mode=None, graph=False, caller=False, shared=flavour == "shared",
             overflowed=False, spmm_dev=0, upd_dev=0, spv_dev=0, bigspmm=False, n=0)
    ops = []

    def inplace():
        return s["x_bound"] and s["y_bound"] == "V"

    def runnable():
        return s["x_ok"] or s["x_bound"]

    def emit(*op):
        ops.append(tuple(op))
        s["n"] += 1

    def runs():
        if inplace() and not fixed:
            emit("run")
            return
        n = int(rng.choice([1, 1, 1, 2, 2, 3, 4, 9]))
        fresh = rng.random() < 0.3 and not s["alt"]      # back-to-back runs with changing vectors
        for i in range(n):
            if fresh and i and not s["x_bound"]:
                emit("load_vector", int(rng.integers(1 << 16)))
            emit("run")

    def partition_loop():
        kind = rng.choice(["whole", "single", "reversed"])
        order = list(range(parts))
        if kind == "single":
            order = [int(rng.integers(parts))]
        elif kind == "reversed":
            order = order[::-1]
        for j in order:
            emit("run_partition", j)

    def after_run():
        """the followers behind the ADVICE findings, right behind a run"""
        pick = rng.choice(["run_partition", "bind_result", "spmm", "spmspv_auto", "update", "reload", "set_stream", "feedback", "iterate", "none", "none", "none"])
        if flavour == "cpu":
            pick = rng.choice(["run_partition", "update", "reload", "none"])
        draw(pick)

    def draw(name):
        if name == "none":
            return
        if name == "load_vector":
            emit("load_vector", int(rng.integers(1 << 16)))
            s["x_ok"] = True
        elif name == "run" and runnable():
            runs()
            if rng.random() < 0.6:
                after_run()
        elif name == "run_batch" and runnable():
            k = 1 if inplace() and not fixed else int(rng.choice([1, 2, 7]))
            if flavour != "cpu" and rng.random() < 0.5:
                s["graph"] = not s["graph"]
                emit("set_option", "batch_graph", "1" if s["graph"] else "0")
            emit("run_batch", k, s["graph"])
            if s["graph"] and rng.random() < 0.6:
                draw(rng.choice(["bind_result", "bind_vector", "toggle"]))
        elif name == "run_partition" and runnable():
            partition_loop()
        elif name == "read_result":
            emit("read_result")
        elif name == "sync_copy":
            emit("sync_copy")
        elif name == "bind_result":
            choices = ["A", "B", None] + (["V"] if square and s["x_bound"] and plan.slices != 1 else [])
            emit("bind_result", choices[int(rng.integers(len(choices)))])
            s["y_bound"] = ops[-1][1]
        elif name == "bind_vector" and not s["alt"]:
            if s["x_bound"]:
                if s["y_bound"] == "V":
                    emit("bind_result", None)
                    s["y_bound"] = None
                emit("bind_vector", None)
                s["x_bound"] = False
            else:
                emit("bind_vector", "V")
                s["x_bound"] = True
                if square and plan.slices != 1 and rng.random() < 0.7:
                    emit("bind_result", "V")
                    s["y_bound"] = "V"
        elif name == "set_stream" and flavour == "full":
            s["caller"] = not s["caller"]
            emit("set_stream", s["caller"])
        elif name == "get_stream" and flavour == "full" and s["n"] > length * 0.6:
            emit("get_stream")
            s["shared"] = True
        elif name == "feedback" and runnable() and not inplace():
            emit("feedback")
        elif name == "iterate" and runnable() and not inplace():
            if rng.random() < 0.5:
                emit("set_option", "iterate_graph", str(int(rng.integers(2))))
            emit("iterate", int(rng.choice([1, 2, 31, 32, 33])) if fixed else 1)
        elif name == "toggle":
            key = str(rng.choice(["spmm_fused", "spmm_mfma", "batch_graph", "iterate_graph"]))
            val = str(int(rng.integers(2)))
            emit("set_option", key, val)
            if key == "batch_graph":
                s["graph"] = val == "1"
        elif name == "spmm":
            k = int(rng.integers(1, 7))
            if plan.fmt == "bitmap" and not fixed and not s["bigspmm"] and rng.random() < 0.5:
                k, s["bigspmm"] = int(rng.choice([16, 21])), True
            if rng.random() < 0.5 and s["spmm_dev"] < MAX_SPMM_DEVICE and k <= 6:
                emit("spmm_device", k, int(rng.integers(1 << 16)), s["spmm_dev"])
                s["spmm_dev"] += 1
            else:
                emit("spmm", k, int(rng.integers(1 << 16)))
        elif name == "load_csc":
            same = bool(rng.random() < 0.7)
            emit("load_csc", same)
            s["csc"], s["csc_same"], s["overflowed"] = True, same and not s["alt"], False
        elif name in ("spmspv", "spmspv_auto"):
            if not s["csc"] or (name == "spmspv_auto" and not s["csc_same"]):
                draw("load_csc")
            modes = ["sparse", None] + (["auto", "dense", "crossover"] if s["csc_same"] else [])
            mode = "auto" if name == "spmspv_auto" and s["csc_same"] else modes[int(rng.integers(len(modes)))]
            kind = str(rng.choice(["unique", "unique", "repeated", "empty"]))
            emit("spmspv", kind, int(rng.integers(1 << 16)), mode)
            s["mode"] = mode
        elif name == "spmspv_device":
            if not s["csc"]:
                draw("load_csc")
            if rng.random() < 0.3:
                emit("spmspv_overflow", bool(rng.random() < 0.5))      # True: the report stays pending for the next call
                draw(rng.choice(["spmspv", "spmspv_device"]))
            elif s["spv_dev"] < MAX_SPMSPV_DEVICE:
                emit("spmspv_device", int(rng.integers(1 << 16)), s["spv_dev"])
                s["spv_dev"] += 1
        elif name == "update" and csr_family and not s["alt"]:
            if flavour != "cpu" and rng.random() < 0.5 and s["upd_dev"] < MAX_UPDATE_DEVICE:
                emit("update_values_device", int(rng.integers(1 << 16)), s["upd_dev"])
                s["upd_dev"] += 1
            else:
                emit("update_values", int(rng.integers(1 << 16)))
            s["csc_same"] = False
        elif name == "reload":
            other = bool(rng.random() < 0.4) and not s["x_bound"] and flavour != "cpu"
            if other:
                s["alt"] = not s["alt"]
            emit("reload", s["alt"])
            s["y_bound"] = None
            s["csc_same"] = False
            if other:
                s["x_ok"] = False
                if rng.random() < 0.7:
                    emit("refused", "not_loaded")
                draw("load_vector")
        elif name == "time":
            if runnable() and not inplace():
                emit(str(rng.choice(["time_runs", "time_kernel"])) if flavour != "cpu" else "time_runs")
        elif name == "push_result":
            n = int(rng.integers(1, 3))
            emit("push_result", n, int(rng.choice([4, 128, 1000, 10 ** 9])))
        elif name == "refused":
            kind = str(rng.choice(REFUSALS[:-1]))
            if kind in ("part_len", "row_part_id") and not runnable():
                return
            if kind == "update_nnz" and (not csr_family or s["alt"]):
                return
            if flavour == "cpu" and kind not in ("part_len", "row_part_id", "update_nnz"):
                return
            if kind == "spmspv_column" and not s["csc"]:
                draw("load_csc")
            emit("refused", kind)

    full = ["load_vector"] * 6 + ["run"] * 10 + ["run_batch"] * 6 + ["run_partition"] * 4 + ["read_result"] * 10 + ["sync_copy"] * 10 + \
        ["bind_result"] * 4 + ["bind_vector"] * 3 + ["set_stream"] * 3 + ["get_stream"] + ["feedback"] * 3 + ["iterate"] * 3 + ["toggle"] * 2 + \
        ["spmm"] * 4 + ["load_csc"] + ["spmspv"] * 4 + ["spmspv_device"] * 3 + ["update"] * 3 + ["reload"] * 2 + ["time"] * 2 + \
        ["push_result"] * 3 + ["refused"] * 4
    cpu = ["load_vector"] * 4 + ["run"] * 8 + ["run_batch"] * 4 + ["run_partition"] * 3 + ["read_result"] * 6 + ["update"] * 3 + ["reload"] * 2 + \
        ["time"] * 2 + ["refused"] * 2
    table = cpu if flavour == "cpu" else full
    draw("load_vector")
    while len(ops) < length:
        draw(str(rng.choice(table)))
    ops.append(("read_result",))
    return ops


# ---- the driver --------------------------------------------------------------------------------------------------------------------
class Player:
    """Plays ops on one engine and compares with the model.  `be` (a backend) gives the engine and the device memory:
         be.engine(impl, ob_bank, vb_bank) -> an object with device.SpmvEngine's methods
         be.memory: None (no device memory: only hs_read_result shows anything) or an object with alloc(words) -> address, free(address),
           write(address, uint32 array), read(address, words) -> array, stream_create() -> handle, stream_sync(handle), stream_destroy(handle)
         be.update_values_raw(engine, float32 array, nnz) -> return code (the wrapper's own count check bypassed)"""

    def __init__(self, be, plan, impl, seed, label=None):
        self.be, self.plan, self.impl, self.seed = be, plan, impl, seed
        self.label = label or f"plan {plan.name}, impl {impl}, seed {seed}"
        self.mem = be.memory
        self.model = Model(impl, concrete=getattr(be, "exact_float", False))
        self.eng = None              # created by start()
        self.ptr = {}                # buffer name -> device address
        self.allocs = []             # (address of the allocation, words with guards)
        self.stream = None           # the caller-owned stream (lives as long as the engine)
        self.cur_stream = None       # the stream handle a plain synchronisation may use (None: the library's own, not handed out)
        self.own_stream = None       # the library's own stream, once hs_get_stream has handed it out
        self.done = []               # ops played so far
        self.seen = {}               # Prov.key -> the words that product gave first
        self.stats = None
        self.observations = 0
        self.conditions = []         # (op index, saturated share, zero share, distinct share) of y at observation points (fixed point)
        self.kind = load_kind(seed)
        self.scale, self.shift = scale_shift(impl)

    # ---- set-up ----
    def caller_buffer(self, name, words):
        """a caller-owned buffer of `words` words between two guards, filled with the pattern"""
        total = words + 2 * GUARD_WORDS
        base = self.mem.alloc(total)
        init = np.full(total, GUARD, dtype=np.uint32)
        init[GUARD_WORDS: GUARD_WORDS + words] = (PATTERN[self.impl] + np.arange(words)).astype(np.uint32)
        self.mem.write(base, init)
        self.allocs.append((base, total, name))
        self.ptr[name] = base + 4 * GUARD_WORDS
        self.model.add(name, init[GUARD_WORDS: GUARD_WORDS + words].copy())

    def start(self):
        with self.faults():
            self.eng = self.be.engine(self.impl, OB_BANK, VB_BANK)
            self._start()
        return self

    def faults(self):
        """Around everything that reaches the device: an HS_ERR_HIP from ANY call -- a load, a debug read, hs_create, hs_spmspv_status, not
        only the calls that go through call() -- is a DeviceFault, never an ordinary failure of one test."""
        return _Faults(self)

    def _start(self):
        mat = plan_matrix(self.plan, self.impl)
        for k, v in self.plan.options.items():
            if not getattr(self.be, "no_options", False):
                self.eng.set_option(k, v)
            self.model.set_option(k, v)
        if self.kind != "cpsr" and not getattr(self.be, "no_options", False):
            self.eng.set_option("value_map", "1")
        self.load(mat)
        if self.mem is not None:
            rows, cols = mat.rows, mat.cols + ALT_COLS
            for name in ("A", "B", "P0", "P1"):
                self.caller_buffer(name, rows)
            self.caller_buffer("V", cols)
            self.mem.write(self.ptr["V"], x_words(self.impl, cols, 77))
            self.model.bufs["V"].put(0, x_words(self.impl, cols, 77))
            self.ldx, self.ldy = (cols + 3) // 4 * 4 + 8, rows + 12
            for i in range(MAX_SPMM_DEVICE):
                self.caller_buffer(f"SX{i}", 6 * self.ldx)
                self.caller_buffer(f"SY{i}", 6 * self.ldy)
            self.caller_buffer("E", 2 * (MAX_SPMSPV_DEVICE * 256 + 3 * cols))
            self.caller_buffer("VAL", MAX_UPDATE_DEVICE * (mat.nnz + 4))
            self.stream = self.mem.stream_create()

    def load(self, mat):
        eng, kind = self.eng, self.kind
        perm = None
        if kind == "cpsr":
            eng.load_matrix(self.be.packets(mat))
        elif kind == "csr":
            eng.load_matrix_csr((mat.rows, mat.cols, mat.indptr, mat.indices, mat.data))
        else:
            a = sp.csr_matrix((np.arange(mat.nnz, dtype=np.int64), mat.indices, mat.indptr), shape=(mat.rows, mat.cols)).T.tocsr()
            a.sort_indices()
            order = a.data.copy()                           # element e of A = M^T is element order[e] of M
            perm = np.empty(mat.nnz, dtype=np.int64)
            perm[order] = np.arange(mat.nnz)
            eng.load_matrix_csr((mat.cols, mat.rows, a.indptr, a.indices, mat.data[order]), transpose=True)
        assert (eng.num_rows, eng.num_cols) == (mat.rows, mat.cols), (eng.num_rows, eng.num_cols, mat.rows, mat.cols)
        info = self.be.plan_info(eng, self.plan, self.impl, mat) if hasattr(self.be, "plan_info") else {}
        info["value_map"] = kind != "cpsr"
        if self.plan.options.get("spmm_vectors") == "4":
            info["spmm_vectors"] = 4
        self.stats = info.get("stats")
        self.model.load(mat, info, perm)
        if self.mem is not None:
            self.ptr["y"] = eng.device_result()

    def close(self):
        try:
            if self.mem is not None and self.cur_stream is not None:
                self.mem.stream_sync(self.cur_stream)
            if self.eng is not None:
                self.eng.close()
        finally:
            if self.mem is not None:
                if self.stream is not None:
                    self.mem.stream_destroy(self.stream)
                for base, _, _ in self.allocs:
                    self.mem.free(base)
                self.allocs = []

    # ---- calls ----
    def call(self, fn, *args):
        try:
            return fn(*args)
        except device.DeviceError as e:
            if e.code == HIP_ERROR:
                raise DeviceFault(f"{self.label}: HS_ERR_HIP at op {len(self.done)} {self.done[-1:]}: {e}\n{self.replay()}") from e
            raise

    def expect_refusal(self, code, fn, *args):
        try:
            self.call(fn, *args)
        except device.DeviceError as e:
            if e.code != code:
                self.fail(f"refused with {e.code}, documented is {code}: {e}")
            return
        self.fail(f"the call was accepted; documented is the refusal {code}")

    def replay(self):
        return (f"# replay: context_model.replay(backend, {self.plan.name!r}, {self.impl}, {self.seed}, ops)\nops = [\n" +
                "".join(f"    {op!r},\n" for op in self.done) + "]")

    def fail(self, what):
        raise Mismatch(f"{self.label}, op {len(self.done) - 1} {self.done[-1] if self.done else ''}: {what}\n{self.replay()}")

    # ---- observation ----
    def observe(self, via="sync"):
        m, eng = self.model, self.eng
        got_y = None
        if via == "read" or self.mem is None:
            got_y = self.call(eng.read_result)
        elif m.private and m.observable():
            self.mem.device_sync()       # settled (hs_sync, hs_read_result, hs_push_result, hs_get_stream) and no step since: no library call needed
        elif m.private or self.cur_stream is None:
            self.call(eng.sync)
        else:
            self.mem.stream_sync(self.cur_stream)
        m.settle()
        self.observations += 1
        snap = {}
        if self.mem is not None:
            for name, buf in m.bufs.items():
                if name in self.ptr:
                    snap[name] = self.mem.read(self.ptr[name], len(buf.w))
            if got_y is not None and not np.array_equal(got_y, snap[m.y_dst.name][: len(got_y)]):
                self.fail("hs_read_result returned other words than the result target holds")
        else:
            snap["y"] = got_y
        if m.csc is not None and self.mem is not None:
            if m.overflow:                      # the report of an overflow nobody has read yet comes first, once
                self.expect_refusal(BAD_ARG, eng.read_spmspv_result)
                m.overflow = False
            snap["sy"] = self.call(eng.read_spmspv_result)
        order = sorted(snap, key=lambda n: any(isinstance(p, Fed) for _, _, _, p in m.bufs[n].pend))      # feedback segments need their y adopted first
        for name in order:
            self.compare(m.bufs[name], snap[name])
        for name in ("y", "A", "B", "V") if self.impl == 0 and m.mat is not None else ():
            if name not in m.bufs or not m.bufs[name].product or (name == "V" and m.y_bound != "V"):
                continue
            y = m.bufs[name].w[: m.mat.rows]
            has = np.diff(m.mat.indptr) > 0
            self.conditions.append((len(self.done), float((y == SAT).mean()), float((y[has] == 0).mean()) if has.any() else 0.0,
                                    len(np.unique(y[has])) / max(1, int(has.sum()))))

    def compare(self, buf, dev):
        known = np.ones(len(buf.w), dtype=bool)
        for a, b, _, _ in buf.pend:
            known[a:b] = False
        bad = np.nonzero((dev != buf.w) & known)[0]
        if bad.size:
            i = int(bad[0])
            self.fail(f"buffer {buf.name}: {bad.size} words differ, first at word {i}: expected {int(buf.w[i]):#010x}, observed {int(dev[i]):#010x}")
        pend, buf.pend = buf.pend, []
        for a, b, r0, p in pend:
            got = dev[a:b]
            if isinstance(p, Fed):
                want = feedback_words(self.impl, self.model.bufs[p.src].w[: b - a], got, p.scale, p.shift)
                if not np.array_equal(got, want):
                    i = int(np.nonzero(got != want)[0][0])
                    self.fail(f"buffer {buf.name}: x != fl(fl(scale y) + shift) of the device's y, first at word {a + i}: expected {int(want[i]):#010x}, observed {int(got[i]):#010x}")
            else:
                self.check_float(buf, a, b, r0, p, got)
            buf.w[a:b] = got

    def check_float(self, buf, a, b, r0, p, got):
        ref = _reference(p)
        full = np.zeros(ref.num_rows, dtype=np.uint32)
        full[r0: r0 + b - a] = got
        bad = ref.violations(full, p.L, p.S)
        bad[:r0] = False
        bad[r0 + b - a:] = False
        if bad.any() and getattr(self.be, "float_contract", True):
            i = int(np.nonzero(bad)[0][0])
            self.fail(f"buffer {buf.name}: {int(bad.sum())} rows break the float contract (route {p.key[2]}, L={np.max(p.L)}, S={p.S}), first row {i}: "
                      f"E={ref.E[i]!r}, observed {float(full.view(np.float32)[i])!r}, bound {float(np.atleast_1d(ref.bound(p.L, p.S))[i]):.3g}")
        want = _oracle(p)[r0: r0 + b - a]
        if not cases.float_close(got, want):
            d = np.abs(got.view(np.float32).astype(np.float64) - want.view(np.float32))
            i = int(np.nanargmax(d))
            self.fail(f"buffer {buf.name}: further than 1e-4 from the oracle (route {p.key[2]}), worst row {r0 + i}: expected {float(want.view(np.float32)[i])!r}, "
                      f"observed {float(got.view(np.float32)[i])!r}")
        first = self.seen.setdefault((p.key, r0, b - a), got.copy())
        if not np.array_equal(first, got):
            i = int(np.nonzero(first != got)[0][0])
            self.fail(f"buffer {buf.name}: the same product on the same route (route {p.key[2]}) gave other words than before, first row {r0 + i}: "
                      f"earlier {int(first[i]):#010x}, now {int(got[i]):#010x}")

    def pre_run(self):
        """float modes: a run that reads an x the model only knows as pending (in-place y = A y) observes first and goes on from the device's x"""
        m = self.model
        if m.mat is not None and (m.x_bound or "x" in m.bufs) and m.x_src.pending(0, m.mat.cols):
            self.observe()

    # ---- the ops ----
    def play(self, ops):
        for op in ops:
            self.step(op)
        return self

    def step(self, op):
        self.done.append(tuple(op))
        with self.faults():
            getattr(self, "op_" + op[0])(*op[1:])

    def finish(self):
        """the closing observation and the guards"""
        self.done.append(("finish",))
        with self.faults():
            self._finish()

    def _finish(self):
        self.observe()
        if self.mem is not None:
            for base, total, name in self.allocs:
                w = self.mem.read(base, total)
                for lo, hi in ((0, GUARD_WORDS), (total - GUARD_WORDS, total)):
                    bad = np.nonzero(w[lo:hi] != GUARD)[0]
                    if bad.size:
                        self.fail(f"guard of buffer {name} overwritten at word {lo + int(bad[0]) - GUARD_WORDS}: {int(w[lo + bad[0]]):#010x}")

    def op_load_vector(self, seed):
        xw = x_words(self.impl, self.model.mat.cols, seed)
        self.call(self.eng.load_vector, xw)
        self.model.load_vector(xw)
        if self.mem is not None:
            self.ptr["x"] = self.eng.device_vector()

    def op_run(self):
        self.pre_run()
        self.call(self.eng.run)
        self.model.run()

    def op_run_batch(self, k, graph=False):
        self.pre_run()
        self.call(self.eng.run_batch, k)
        self.model.run_batch(k)

    def op_run_partition(self, j):
        self.pre_run()
        lo, hi = self.model.parts[j]
        self.call(self.eng.run_partition, j, (hi - lo) // 16)
        self.model.run_partition(j, (hi - lo) // 16)

    def op_read_result(self):
        self.observe("read")

    def op_sync_copy(self):
        self.observe("sync")

    def op_bind_result(self, name):
        self.call(self.eng.bind_device_result, self.ptr[name] if name else None)
        self.model.bind_result(name)

    def op_bind_vector(self, name):
        self.call(self.eng.bind_device_vector, self.ptr[name] if name else None)
        self.model.bind_vector(name)

    def op_set_stream(self, caller):
        self.call(self.eng.set_stream, self.stream if caller else None)
        self.model.set_stream(caller)
        self.cur_stream = self.stream if caller else (self.own_stream if self.model.shared else None)

    def op_get_stream(self):
        h = self.call(self.eng.get_stream)
        self.model.get_stream()
        if not self.model.caller_stream:
            self.own_stream = h
        self.cur_stream = h

    def op_feedback(self):
        self.call(self.eng.feedback, self.scale, self.shift)
        self.model.feedback(self.scale, self.shift)
        if not self.model.concrete:
            self.observe("read")

    def op_iterate(self, n):
        self.pre_run()
        self.call(self.eng.iterate, n, self.scale, self.shift)
        self.model.iterate(n, self.scale, self.shift)
        if not self.model.concrete:
            self.observe("read")

    def op_set_option(self, key, value):
        self.call(self.eng.set_option, key, value)
        self.model.set_option(key, value)

    def _spmm_x(self, k, seed):
        cols = self.model.mat.cols
        return np.stack([x_words(self.impl, cols, seed * 31 + j) for j in range(k)])

    def op_spmm(self, k, seed):
        X = self._spmm_x(k, seed)
        Y = self.call(self.eng.spmm, X)
        tmp = Buf("hs_spmm's Y", np.zeros(Y.size, dtype=np.uint32))
        rows = self.model.mat.rows
        for j, product in enumerate(self.model.spmm_columns(X)):
            self.model._write(tmp, j * rows, (j + 1) * rows, 0, product)
        self.compare(tmp, Y.ravel())

    def op_spmm_device(self, k, seed, slot):
        m = self.model
        X = self._spmm_x(k, seed)
        xname, yname = f"SX{slot}", f"SY{slot}"
        for j in range(k):
            self.mem.write(self.ptr[xname] + 4 * j * self.ldx, X[j])
            m.bufs[xname].put(j * self.ldx, X[j])
        self.call(self.eng.spmm_device, self.ptr[xname], self.ldx, self.ptr[yname], self.ldy, k)
        m.spmm_device(xname, self.ldx, yname, self.ldy, k)

    def _csc_arrays(self, t):
        return t.indptr.astype(np.uint32), t.indices.astype(np.uint32), t.words

    def op_load_csc(self, same):
        m = self.model
        plan_mat = plan_matrix(self.plan, self.impl)
        if same:
            src = m.mat
        else:                                   # another matrix of the same shape: the plan's pattern with other values
            src = plan_mat.with_data(new_values(self.impl, plan_mat, 4242))
        rows, cols = self.plan.rows, (self.plan.cols + (ALT_COLS if same and m.mat.cols != plan_mat.cols else 0))
        a = src.scipy()[:rows, :cols].T.tocsr()
        a.sort_indices()
        t = Mat.from_scipy(self.impl, a)
        indptr, ridx, words = self._csc_arrays(t)
        self.call(self.eng.load_matrix_csc, indptr, ridx, words, rows)
        m.load_csc(t, rows)

    def _entries(self, kind, seed):
        t = self.model.csc
        rng = np.random.default_rng(seed)
        if kind == "empty":
            return np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint32)
        n = int(rng.integers(1, 200))
        idx = rng.choice(t.rows, size=min(n, t.rows), replace=False).astype(np.uint32)
        if kind == "repeated":
            idx = np.concatenate([idx, idx[: max(1, len(idx) // 3)], idx[:2], idx[:1]])
            rng.shuffle(idx)
        return idx, x_words(self.impl, len(idx), seed)

    def op_spmspv(self, kind, seed, mode):
        m = self.model
        want = {"crossover": None}.get(mode, mode)
        if m.options.get("spmspv") != want:
            self.op_set_option("spmspv", want)
        cross = "0.001" if mode == "crossover" else None
        if m.options.get("spmspv_crossover") != cross:
            self.op_set_option("spmspv_crossover", cross)
        assert mode in (None, "sparse") or m.same_both_ways(), "the generator draws auto / dense only over the same matrix both ways"
        idx, w = self._entries(kind, seed)
        self.call(self.eng.spmspv_async, idx, w)
        m.spmspv(idx, w)
        if m.overflow:                          # the report of an earlier overflow is still pending: reading it clears it
            self.expect_refusal(BAD_ARG, self.eng.read_spmspv_result)
            m.overflow = False

    def _pairs(self, idx, w):
        pairs = np.empty((len(idx), 2), dtype=np.uint32)
        pairs[:, 0], pairs[:, 1] = idx, w
        return pairs.ravel()

    def op_spmspv_device(self, seed, slot):
        m = self.model
        idx, w = self._entries("unique", seed)
        at = self.ptr["E"] + slot * 256 * 8
        self.mem.write(at, self._pairs(idx, w))
        m.bufs["E"].put(slot * 512, self._pairs(idx, w))
        self.call(self.eng.spmspv_device, at, len(idx))
        m.spmspv_device(idx, w)
        if m.overflow:
            self.expect_refusal(BAD_ARG, self.eng.read_spmspv_result)
            m.overflow = False

    def op_spmspv_overflow(self, pending=False):
        m = self.model
        if m.overflow:
            self.expect_refusal(BAD_ARG, self.eng.read_spmspv_result)
        cols = m.csc.rows
        idx = np.tile(np.arange(cols, dtype=np.uint32), 3)
        pairs = self._pairs(idx, x_words(self.impl, len(idx), 5))
        at = self.ptr["E"] + MAX_SPMSPV_DEVICE * 256 * 8
        self.mem.write(at, pairs)
        m.bufs["E"].put(MAX_SPMSPV_DEVICE * 512, pairs)
        self.call(self.eng.spmspv_device, at, len(idx))
        m.spmspv_device(None, None, overflow=True)
        if m.csc.nnz and self.be.spmspv_status(self.eng) != 1:
            self.fail("hs_spmspv_status does not report the overflow")
        if pending:           # nobody reads the result: the next hs_spmspv* must be clean all the same, and the report comes with the next read
            return
        self.expect_refusal(BAD_ARG, self.eng.read_spmspv_result)
        m.overflow = False
        if self.be.spmspv_status(self.eng) != 0:
            self.fail("hs_spmspv_status still reports an overflow after hs_read_spmspv_result cleared it")

    def op_update_values(self, seed):
        v = new_values(self.impl, self.model.mat, seed)
        self.call(self.eng.update_values, v)
        self.model.update_values(v)

    def op_update_values_device(self, seed, slot):
        m = self.model
        v = new_values(self.impl, m.mat, seed)
        at = slot * (len(v) + 4)
        self.mem.write(self.ptr["VAL"] + 4 * at, v.view(np.uint32))
        m.bufs["VAL"].put(at, v.view(np.uint32))
        self.call(self.eng.update_values_device, self.ptr["VAL"] + 4 * at, len(v))
        m.update_values(v)

    def op_reload(self, alt):
        self.load(plan_matrix(self.plan, self.impl, alt))

    def op_time_runs(self):
        self.pre_run()
        self.call(self.eng.time_runs, 1, 3)
        self.model.time_runs()

    def op_time_kernel(self):
        self.pre_run()
        self.call(self.eng.time_kernel, 1, 3)
        self.model.time_kernel()

    def op_push_result(self, n, words):
        words = min(words, self.model.mat.rows) // 4 * 4
        names = ["P0", "P1"][:n]
        self.call(self.eng.push_result, [self.ptr[x] for x in names], words)
        self.model.push(names, words)

    def op_refused(self, kind):
        m, eng = self.model, self.eng
        if kind == "part_len":
            lo, hi = m.parts[0]
            self.expect_refusal(BAD_ARG, eng.run_partition, 0, (hi - lo) // 16 + 1)
        elif kind == "row_part_id":
            lo, hi = m.parts[-1]
            self.expect_refusal(BAD_ARG, eng.run_partition, len(m.parts), (hi - lo) // 16)
        elif kind == "spmspv_column":
            idx, w = self._entries("unique", 3)
            idx = np.concatenate([idx, [m.csc.rows]]).astype(np.uint32)
            self.expect_refusal(BAD_ARG, eng.spmspv_async, idx, np.concatenate([w, w[:1]]))
        elif kind == "update_nnz":
            v = new_values(self.impl, m.mat, 1)
            rc = self.be.update_values_raw(eng, v, m.mat.nnz - 1)
            if rc == HIP_ERROR:
                raise DeviceFault(f"{self.label}: HS_ERR_HIP from a refused hs_update_values\n{self.replay()}")
            if rc != BAD_ARG:
                self.fail(f"hs_update_values with a wrong count answered {rc}, documented is {BAD_ARG}")
        elif kind == "misaligned_result":
            self.expect_refusal(BAD_ARG, eng.bind_device_result, self.ptr["A"] + 4)
        elif kind == "misaligned_vector":
            self.expect_refusal(BAD_ARG, eng.bind_device_vector, self.ptr["V"] + 4)
        elif kind == "unknown_option":
            self.expect_refusal(BAD_ARG, eng.set_option, "carry_combined", "1")
        elif kind == "not_loaded":
            self.expect_refusal(NOT_LOADED, eng.run)


_REFS = {}


def _reference(p):
    key = (p.key[0], p.key[1], p.exact, p.key[2] if p.key[2] in ("spmspv",) else None)
    if key not in _REFS:
        if len(_REFS) > 64:
            _REFS.clear()
        m = p.m.scipy()
        _REFS[key] = (fc.Reference(m, p.x[: m.shape[1]], exact_products=p.exact), p.oracle())
    return _REFS[key][0]


def _oracle(p):
    _reference(p)
    return _REFS[(p.key[0], p.key[1], p.exact, p.key[2] if p.key[2] in ("spmspv",) else None)][1]


def replay(be, plan_name, impl, seed, ops):
    """play a printed sequence again (a failing sequence is reduced by deleting ops from the list)"""
    p = Player(be, PLAN[plan_name], impl, seed)
    try:
        p.start()
        p.play(ops)
        p.finish()
    finally:
        p.close()
    return p


def play_sequence(be, plan, impl, seed, length=LENGTH, flavour="full"):
    p = Player(be, plan, impl, seed)
    try:
        p.start()
        p.play(generate(plan, impl, seed, length, flavour))
        p.finish()
    finally:
        p.close()
    return p


def play_two_engines(be, impl, seed, length=LENGTH):
    """Two engines on one device, the second on the first's stream (set_stream(first.get_stream())), ops interleaved by the seed: what
    bench.py's round-robin over several matrices relies on"""
    a = Player(be, PLAN[TWO_ENGINES[0]], impl, seed, label=f"two-engines first ({TWO_ENGINES[0]}), impl {impl}, seed {seed}")
    try:
        a.start()
        b = Player(be, PLAN[TWO_ENGINES[1]], impl, seed, label=f"two-engines second ({TWO_ENGINES[1]}), impl {impl}, seed {seed}")
        try:
            b.start()
            a.step(("get_stream",))
            b.done.append(("set_stream", "first.get_stream()"))
            b.call(b.eng.set_stream, a.cur_stream)
            b.model.set_stream(True)
            b.cur_stream = a.cur_stream
            seqs = [generate(a.plan, impl, seed, length // 2, "shared"), generate(b.plan, impl, seed + 300, length // 2, "shared")]
            rng = np.random.default_rng(seed)
            at = [0, 0]
            players = (a, b)
            while at[0] < len(seqs[0]) or at[1] < len(seqs[1]):
                i = int(rng.integers(2))
                if at[i] >= len(seqs[i]):
                    i = 1 - i
                for _ in range(int(rng.integers(1, 4))):      # a few ops of one engine, then the other
                    if at[i] < len(seqs[i]):
                        players[i].step(seqs[i][at[i]])
                        at[i] += 1
            a.finish()
            b.finish()
        finally:
            b.close()
    finally:
        a.close()
    return a, b


# ---- a fake engine: the model behind device.SpmvEngine's methods, with one planted defect at a time ----------------------------------
class FakeMemory:
    def __init__(self):
        self.blocks = {}            # base address -> uint32 array
        self.next = 0x10000

    def alloc(self, words):
        return self.adopt(np.zeros(words, dtype=np.uint32))

    def adopt(self, array):
        base = self.next
        self.next += (4 * len(array) + 4095) // 4096 * 4096 + 4096
        self.blocks[base] = array
        return base

    def free(self, base):
        del self.blocks[base]

    def view(self, addr):
        for base, a in self.blocks.items():
            if base <= addr < base + 4 * len(a):
                assert (addr - base) % 4 == 0
                return a[(addr - base) // 4:]
        raise KeyError(hex(addr))

    def write(self, addr, words):
        self.view(addr)[: len(words)] = words

    def read(self, addr, words):
        return self.view(addr)[:words].copy()

    def stream_create(self):
        return 0x5000

    def stream_sync(self, handle):
        pass

    def device_sync(self):
        pass

    def stream_destroy(self, handle):
        pass


DEFECTS = {
    "a": "read_result after two back-to-back runs with different x returns the earlier y",
    "b": "run_batch keeps the x or y target it saw first",
    "c": "run_partition zeroes the other partitions' rows",
    "d": "a second spmspv adds onto the first's result",
    "e": "feedback writes all of x instead of the first min(rows, cols) words",
    "f": "the sum of a run before bind_device_result lands in the new target",
    "g": "a refused call still performs its action",
}


class FakeEngine:
    """device.SpmvEngine's methods over a Model of its own whose buffers live in a FakeMemory; `defect`: a key of DEFECTS or None"""

    def __init__(self, memory, impl, defect=None):
        self.mem, self.impl, self.defect = memory, impl, defect
        self.m = Model(impl, concrete=True)
        self.num_rows = self.num_cols = 0
        self.addr = {}
        self.ys = []                 # (d) / (a): the y of each run since something else happened
        self.batch_first = None
        self.last = None
        self.csc_rows = 0
        self.value_map = False
        self.status = 0              # the overflow word of hs_spmspv_status

    def _buf(self, addr):
        if addr is None:
            return None
        name = f"@{addr:#x}"
        if name not in self.m.bufs:
            self.m.add(name, self.mem.view(addr))
        return name

    def _guard(self, fn, *args, after=None):
        try:
            out = fn(*args)
        except AssertionError:
            raise
        except Refused as r:
            if self.defect == "g" and after is not None:
                after()
            raise device.DeviceError(r.code, "refused")
        return out

    def _note(self, what):
        if what not in ("run", "load_vector"):
            self.ys = []
        self.last = what

    def close(self):
        pass

    def set_option(self, key, value=None):
        self._guard(self.m.set_option, key, value)

    def _loaded(self, mat, perm=None):
        self.m.load(mat, {"value_map": self.value_map}, perm)
        self.num_rows, self.num_cols = mat.rows, mat.cols
        self.addr["y"] = self.mem.adopt(self.m.bufs["y"].w)
        self._note("load")

    def load_matrix(self, cp):
        self.value_map = False
        self._loaded(cp.fake_mat)

    def load_matrix_csr(self, csr, transpose=False):
        rows, cols, indptr, indices, data = csr
        self.value_map = self.m.options.get("value_map") == "1"
        mat = Mat(self.impl, rows, cols, indptr, indices, data)
        if not transpose:
            return self._loaded(mat)
        a = sp.csr_matrix((np.arange(mat.nnz, dtype=np.int64), mat.indices, mat.indptr), shape=(rows, cols)).T.tocsr()
        a.sort_indices()
        div = 128 * (8 if self.impl == 2 else 1)
        t = Mat(self.impl, -(-cols // div) * div, -(-rows // 8) * 8, np.concatenate([a.indptr, np.full(-(-cols // div) * div - cols, a.indptr[-1])]),
                a.indices, mat.data[a.data])
        self._loaded(t, perm=a.data.copy())

    def load_vector(self, words):
        self._guard(self.m.load_vector, words)
        if self.addr.get("xw") is not self.m.bufs["x"].w:
            self.addr["xw"] = self.m.bufs["x"].w
            self.addr["x"] = self.mem.adopt(self.addr["xw"])
        self._note("load_vector")

    def device_vector(self):
        return self.addr["x"]

    def device_result(self):
        return self.addr["y"]

    def run(self):
        self._guard(self.m.run)
        self.ys.append(self.m.y_dst.w[: self.m.mat.rows].copy())
        self._note("run")

    def run_batch(self, steps):
        m = self.m
        if self.defect == "b" and steps:
            if self.batch_first is None:
                self.batch_first = (m.x_bound, m.y_bound)
            saved = (m.x_bound, m.y_bound)
            m.x_bound, m.y_bound = self.batch_first
            if m.y_bound is not None and len(m.bufs[m.y_bound].w) < m.mat.rows:
                m.y_bound = None
            try:
                self._guard(m.run_batch, steps)
            finally:
                m.x_bound, m.y_bound = saved
        else:
            self._guard(m.run_batch, steps)
        self._note("run_batch")

    def run_partition(self, j, part_len):
        m = self.m

        def anyway():
            if m.mat is not None and (m.x_bound or "x" in m.bufs):
                jj = min(j, len(m.parts) - 1)
                m.run_partition(jj, (m.parts[jj][1] - m.parts[jj][0]) // 16)
        self._guard(m.run_partition, j, part_len, after=anyway)
        if self.defect == "c":
            lo, hi = m.parts[j]
            y = m.y_dst.w
            y[:lo] = 0
            y[hi: m.mat.rows] = 0
        self._note("run_partition")

    def sync(self):
        self._note("sync")

    def read_result(self):
        m = self.m
        y = m.y_dst.w[: m.mat.rows].copy()
        if self.defect == "a" and len(self.ys) >= 2 and not np.array_equal(self.ys[-1], self.ys[-2]):
            y = self.ys[-2].copy()
        self._note("read_result")
        return y

    def bind_device_result(self, ptr):
        if ptr is not None and ptr & 15:
            if self.defect == "g":
                self.m.bind_result(self._buf(ptr))
            raise device.DeviceError(BAD_ARG, "misaligned")
        old = self.m.y_dst if self.m.mat is not None else None
        self.m.bind_result(self._buf(ptr))
        if self.defect == "f" and self.last == "run" and old is not None and old is not self.m.y_dst:
            self.m.y_dst.put(0, old.w[: self.m.mat.rows].copy())
        self._note("bind")

    def bind_device_vector(self, ptr):
        if ptr is not None and ptr & 15:
            if self.defect == "g":
                self.m.bind_vector(self._buf(ptr))
            raise device.DeviceError(BAD_ARG, "misaligned")
        self.m.bind_vector(self._buf(ptr))
        self._note("bind")

    def set_stream(self, handle):
        self.m.set_stream(bool(handle))
        self._note("stream")

    def get_stream(self):
        self.m.get_stream()
        self._note("stream")
        return 0x6000

    def feedback(self, scale, shift):
        m = self.m
        self._guard(m.feedback, scale, shift)
        if self.defect == "e":
            n = min(m.mat.rows, m.mat.cols)
            x = m.x_src.w
            x[n: m.mat.cols] = feedback_words(self.impl, np.zeros(m.mat.cols - n, dtype=np.uint32), x[n: m.mat.cols], scale, shift)
        self._note("feedback")

    def iterate(self, n, scale, shift):
        self._guard(self.m.iterate, n, scale, shift)
        self._note("iterate")

    def push_result(self, ptrs, words):
        self._guard(self.m.push, [self._buf(p) for p in ptrs], words)
        self._note("push")

    def time_runs(self, warmup, runs, kernel=True):
        self._guard(self.m.time_runs)
        self._note("time")
        return 1.0, 1.0

    def time_kernel(self, warmup, runs):
        self._guard(self.m.time_kernel)
        self._note("time")
        return 1.0

    def spmm(self, X):
        m = self.m
        if m.mat is None:
            raise device.DeviceError(NOT_LOADED, "no matrix")
        self._note("spmm")
        return np.stack([m.mat.spmv(x) for x in X])

    def spmm_device(self, xp, ldx, yp, ldy, k):
        self._guard(self.m.spmm_device, self._buf(xp), ldx, self._buf(yp), ldy, k)
        self._note("spmm")

    def load_matrix_csc(self, indptr, ridx, words, num_rows):
        t = Mat(self.impl, len(indptr) - 1, num_rows, indptr, ridx, np.zeros(len(ridx), dtype=np.float32))
        t.words = np.asarray(words, dtype=np.uint32)
        t.data = t.words.view(np.float32) if self.impl else (t.words.astype(np.float64) / (1 << 24)).astype(np.float32)
        self.m.load_csc(t, num_rows)
        self.csc_rows = num_rows
        self.status = 0
        self._note("csc")

    def _spmspv(self, fn, idx, w):
        m = self.m
        before = m.bufs["sy"].w.copy() if "sy" in m.bufs else None

        def anyway():
            keep = np.asarray(idx) < m.csc.rows
            m.spmspv(np.asarray(idx)[keep], np.asarray(w)[keep])
        self._guard(fn, idx, w, after=anyway)
        if self.defect == "d" and self.last == "spmspv" and before is not None:
            sy = m.bufs["sy"].w
            if self.impl == 0:
                sy[:] = np.minimum(sy.astype(np.uint64) + before, SAT).astype(np.uint32)
            else:
                sy[:] = (sy.view(np.float32) + before.view(np.float32)).view(np.uint32)
        self._note("spmspv")

    def spmspv_async(self, idx, w):
        self._spmspv(self.m.spmspv, idx, w)

    def spmspv(self, idx, w):
        self.spmspv_async(idx, w)
        return self.read_spmspv_result()

    def spmspv_device(self, ptr, count):
        pairs = self.mem.read(ptr, 2 * count).reshape(count, 2)
        idx = pairs[:, 0].astype(np.int64)
        if len(np.unique(idx)) != len(idx):
            self.m.spmspv_device(None, None, overflow=True)
            self.status = 1
            self._note("spmspv")
            return
        self._spmspv(self.m.spmspv_device, idx, pairs[:, 1].copy())

    def read_spmspv_result(self):
        if self.status:
            self.status = 0
            self.m.overflow = False
            raise device.DeviceError(BAD_ARG, "more products than the matrix has non-zeros")
        return self.m.bufs["sy"].w.copy()

    def update_values(self, values):
        def anyway():
            if self.m.mat is not None and self.m.info.get("value_map"):
                v = np.zeros(self.m.mat.nnz, dtype=np.float32)
                v[: len(values)] = values[: len(v)]
                self.m.update_values(v)
        self._guard(self.m.update_values, values, after=anyway)
        self._note("update")

    def update_values_device(self, ptr, nnz):
        self.update_values(self.mem.read(ptr, nnz).view(np.float32))


class FakeBackend:
    """the backend of Player over FakeEngine: the whole op table without a GPU, in all three numeric modes"""
    exact_float = True

    def __init__(self, defect=None):
        self.memory = FakeMemory()
        self.defect = defect

    def engine(self, impl, ob_bank, vb_bank):
        return FakeEngine(self.memory, impl, self.defect)

    def packets(self, mat):
        return fake_cp(mat)

    def update_values_raw(self, eng, values, nnz):
        try:
            eng.update_values(values[:nnz])
        except device.DeviceError as e:
            return e.code
        return 0

    def spmspv_status(self, eng):
        return eng.status


class _FakePackets:
    """what FakeEngine.load_matrix takes in place of channel packets"""
    def __init__(self, mat):
        self.fake_mat = mat


def fake_cp(mat):
    return _FakePackets(mat)


def header_entry_points():
    root = os.path.dirname(os.path.dirname(os.path.abspath(device.__file__)))
    text = open(os.path.join(root, "include", "hisparse_hip.h")).read()
    return sorted(set(re.findall(r"^[A-Za-z_][\w \t\*]*?[ \t\*](hs_[a-z0-9_]+)\(", text, flags=re.M)))

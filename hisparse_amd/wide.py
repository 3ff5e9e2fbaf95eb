"""hisparse_amd.wide — ctypes binding of include/hisparse_wide.h: the three products of the attention / sparse-training chain over a CSR
pattern, with ROW-MAJOR dense operands ([index][feature], 1 <= d <= 256 features, fp32).

    sddmm     out[e]  = sum_j U[row(e)][j] V[col(e)][j]                 for every entry e, in CSR order
    spmm      Y[r][j] = sum_{e in row r} w[e] X[col(e)][j]
    spmm_t    Y[c][j] = sum_{e: col(e) = c} w[e] X[row(e)][j]           w in the same CSR order

`WideProducts` holds the pattern (and, with transposed=True, the transposed pattern) on the device; the values w come from the caller on
every call, in the order `RowSoftmax` reads and writes.  The symbols are bound on the handle `device.lib()` returns, so HISPARSE_HIP_LIB
selects libhisparse_cpu.so here as elsewhere (a second implementation on the host, where "device" pointers are host pointers) -- there
is no Python compute path and no fallback.
"""
import ctypes as C

import numpy as np

from . import device
from .device import DeviceError
from .pattern import _pattern_arrays

EXPORTS = ["hsw_create", "hsw_destroy", "hsw_last_error", "hsw_info", "hsw_set_stream", "hsw_sync", "hsw_sddmm_device", "hsw_spmm_device",
           "hsw_spmm_t_device", "hsw_sddmm", "hsw_spmm", "hsw_spmm_t"]

HSW_TRANSPOSED = 1
MAX_D = 256
# launch geometry of the kernels (hisparse_amd/csrc/wide_products.h): at most compute_units * WIDE_BLOCKS_PER_CU workgroups of
# WIDE_THREADS lanes; a group of group_lanes(d) lanes covers a feature row, a row of class c = 1, 2, 3 (at most 4, 16, WIDE_LONG
# entries) has a team of min(64, 4^c group_lanes(d)) lanes, a longer row a workgroup of its own; a group takes WIDE_IN_FLIGHT entries
# per trip -- a schedule of more virtual workgroups goes round the stride loop
WIDE_THREADS = 256
WIDE_BLOCKS_PER_CU = 8
WIDE_IN_FLIGHT = 4
WIDE_LONG = 512

_bound = None


def group_lanes(d):
    """the lanes that cover a feature row of d words: ceil(d / 4) rounded up to a power of two"""
    g = 1
    while g * 4 < d:
        g *= 2
    return g


def team_lanes(row_class, d):
    """the lanes that work on one row of class 1, 2 or 3"""
    return min(64, 4 ** row_class * group_lanes(d))


def rows_per_trip(compute_units, row_class, d):
    """the most rows of one class that one trip of the grid covers on a device of `compute_units` CUs"""
    return compute_units * WIDE_BLOCKS_PER_CU * (WIDE_THREADS // team_lanes(row_class, d))


def lib():
    """device.lib() with the hsw_* prototypes set."""
    global _bound
    l = device.lib()
    if _bound is not l:
        vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
        l.hsw_create.argtypes = [C.POINTER(vp), C.c_int, u32, u32, vp, vp, u32]
        l.hsw_destroy.argtypes = [vp]
        l.hsw_last_error.restype = C.c_char_p
        l.hsw_last_error.argtypes = [vp]
        l.hsw_info.argtypes = [vp, C.POINTER(u64), C.POINTER(u64)]
        l.hsw_set_stream.argtypes = [vp, vp]
        l.hsw_sync.argtypes = [vp]
        l.hsw_sddmm_device.argtypes = [vp, vp, u64, vp, u64, u32, vp]
        l.hsw_spmm_device.argtypes = [vp, vp, vp, u64, u32, vp, u64]
        l.hsw_spmm_t_device.argtypes = [vp, vp, vp, u64, u32, vp, u64]
        l.hsw_sddmm.argtypes = [vp, vp, vp, u32, vp]
        l.hsw_spmm.argtypes = [vp, vp, vp, u32, vp]
        l.hsw_spmm_t.argtypes = [vp, vp, vp, u32, vp]
        _bound = l
    return l


class WideProducts:
    def __init__(self, csr_or_arrays, transposed=True, device_id=0):
        """csr_or_arrays: a host.CSRMatrix, a scipy CSR matrix or an (indptr, indices, (rows, cols)) tuple; transposed: keep the transposed
        pattern too (HSW_TRANSPOSED), which spmm_t needs."""
        self._h = C.c_void_p()
        rows, cols, indptr, indices = _pattern_arrays(csr_or_arrays)
        indptr = np.ascontiguousarray(indptr, dtype=np.uint32)
        indices = np.ascontiguousarray(indices, dtype=np.uint32)
        if indptr.size != rows + 1:
            raise DeviceError(-1, f"indptr holds {indptr.size} words for {rows} rows")
        if indptr.size and indices.size < int(indptr.max()):      # (keeps short arrays from being over-read; the library checks the rest)
            raise DeviceError(-4, f"indices holds {indices.size} entries, indptr reaches {int(indptr.max())}")
        rc = lib().hsw_create(C.byref(self._h), device_id, rows, cols, indptr.ctypes.data, indices.ctypes.data if indices.size else None,
                              HSW_TRANSPOSED if transposed else 0)
        if rc != 0:
            raise DeviceError(rc, lib().hsw_last_error(None).decode())
        self.num_rows, self.num_cols, self.transposed = int(rows), int(cols), bool(transposed)
        self.nnz = self.info()["nnz"]

    def _check(self, rc):
        if rc != 0:
            raise DeviceError(rc, lib().hsw_last_error(self._h).decode() or device.lib().hs_strerror(rc).decode())

    def close(self):
        if self._h:
            lib().hsw_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def info(self):
        nnz, nbytes = C.c_uint64(), C.c_uint64()
        self._check(lib().hsw_info(self._h, C.byref(nnz), C.byref(nbytes)))
        return {"nnz": nnz.value, "device_bytes": nbytes.value}

    def set_stream(self, hip_stream):
        self._check(lib().hsw_set_stream(self._h, C.c_void_p(hip_stream or None)))

    def sync(self):
        self._check(lib().hsw_sync(self._h))

    def _features(self, a, n, what):
        a = np.ascontiguousarray(a, dtype=np.float32)
        if a.ndim != 2 or a.shape[0] != n:
            raise DeviceError(-1, f"{what} must be ({n}, d) float32, not {a.shape}")
        return a

    def _values(self, w):
        w = np.ascontiguousarray(w, dtype=np.float32).ravel()
        if w.size != self.nnz:
            raise DeviceError(-1, f"w holds {w.size} values, the pattern {self.nnz} entries")
        return w if w.size else np.zeros(1, dtype=np.float32)

    def sddmm(self, U, V):
        """hsw_sddmm, the host form: U (num_rows, d) and V (num_cols, d); returns the nnz products (float32) in CSR order."""
        U, V = self._features(U, self.num_rows, "U"), self._features(V, self.num_cols, "V")
        if U.shape[1] != V.shape[1]:
            raise DeviceError(-1, f"sddmm: U has {U.shape[1]} features, V {V.shape[1]}")
        out = np.zeros(max(self.nnz, 1), dtype=np.float32)
        self._check(lib().hsw_sddmm(self._h, U.ctypes.data, V.ctypes.data, U.shape[1], out.ctypes.data))
        return out[:self.nnz]

    def spmm(self, w, X):
        """hsw_spmm, the host form: nnz values in CSR order and X (num_cols, d); returns Y (num_rows, d) float32."""
        w, X = self._values(w), self._features(X, self.num_cols, "X")
        Y = np.zeros((self.num_rows, X.shape[1]), dtype=np.float32)
        self._check(lib().hsw_spmm(self._h, w.ctypes.data, X.ctypes.data, X.shape[1], Y.ctypes.data))
        return Y

    def spmm_t(self, w, X):
        """hsw_spmm_t, the host form: nnz values in the same CSR order and X (num_rows, d); returns Y (num_cols, d) float32."""
        w, X = self._values(w), self._features(X, self.num_rows, "X")
        Y = np.zeros((self.num_cols, X.shape[1]), dtype=np.float32)
        self._check(lib().hsw_spmm_t(self._h, w.ctypes.data, X.ctypes.data, X.shape[1], Y.ctypes.data))
        return Y

    def sddmm_device(self, u_ptr, ldu, v_ptr, ldv, d, out_ptr):
        """hsw_sddmm_device: pointers (int) into device memory, features 16-byte aligned, ld in words; asynchronous on the object's stream."""
        self._check(lib().hsw_sddmm_device(self._h, C.c_void_p(u_ptr or None), int(ldu), C.c_void_p(v_ptr or None), int(ldv), int(d), C.c_void_p(out_ptr or None)))

    def spmm_device(self, w_ptr, x_ptr, ldx, d, y_ptr, ldy):
        """hsw_spmm_device; asynchronous on the object's stream."""
        self._check(lib().hsw_spmm_device(self._h, C.c_void_p(w_ptr or None), C.c_void_p(x_ptr or None), int(ldx), int(d), C.c_void_p(y_ptr or None), int(ldy)))

    def spmm_t_device(self, w_ptr, x_ptr, ldx, d, y_ptr, ldy):
        """hsw_spmm_t_device (needs transposed=True); asynchronous on the object's stream."""
        self._check(lib().hsw_spmm_t_device(self._h, C.c_void_p(w_ptr or None), C.c_void_p(x_ptr or None), int(ldx), int(d), C.c_void_p(y_ptr or None), int(ldy)))

"""hisparse_amd.attention — ctypes binding of include/hisparse_attention.h: the attention step over a CSR pattern in one call, with
ROW-MAJOR dense operands ([index][feature], 1 <= d <= 256 features, fp32) and no per-entry array.

    forward   t[e] = scale * sum_j Q[row(e)][j] K[col(e)][j],   P = the row softmax of t,   Y[r][j] = sum_{e in row r} P[e] V[col(e)][j]
              lse[r] = max_r t + log sum_{e in r} exp(t[e] - max_r t)      (one word per row: P[e] = exp(t[e] - lse[row(e)]))

`PatternAttention` holds the pattern on the device.  The symbols are bound on the handle `device.lib()` returns, so HISPARSE_HIP_LIB
selects libhisparse_cpu.so here as elsewhere (a second implementation on the host, where "device" pointers are host pointers) -- there
is no Python compute path and no fallback.
"""
import ctypes as C

import numpy as np

from . import device
from .device import DeviceError
from .pattern import _pattern_arrays

EXPORTS = ["hsat_create", "hsat_destroy", "hsat_last_error", "hsat_info", "hsat_set_stream", "hsat_sync", "hsat_forward_device", "hsat_forward"]

MAX_D = 256

_bound = None


def lib():
    """device.lib() with the hsat_* prototypes set."""
    global _bound
    l = device.lib()
    if _bound is not l:
        vp, u32, u64, f32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_float
        l.hsat_create.argtypes = [C.POINTER(vp), C.c_int, u32, u32, vp, vp]
        l.hsat_destroy.argtypes = [vp]
        l.hsat_last_error.restype = C.c_char_p
        l.hsat_last_error.argtypes = [vp]
        l.hsat_info.argtypes = [vp, C.POINTER(u64), C.POINTER(u64)]
        l.hsat_set_stream.argtypes = [vp, vp]
        l.hsat_sync.argtypes = [vp]
        l.hsat_forward_device.argtypes = [vp, vp, u64, vp, u64, vp, u64, u32, f32, vp, u64, vp]
        l.hsat_forward.argtypes = [vp, vp, vp, vp, u32, f32, vp, vp]
        _bound = l
    return l


class PatternAttention:
    def __init__(self, csr_or_arrays, device_id=0):
        """csr_or_arrays: a host.CSRMatrix, a scipy CSR matrix or an (indptr, indices, (rows, cols)) tuple"""
        self._h = C.c_void_p()
        rows, cols, indptr, indices = _pattern_arrays(csr_or_arrays)
        indptr = np.ascontiguousarray(indptr, dtype=np.uint32)
        indices = np.ascontiguousarray(indices, dtype=np.uint32)
        if indptr.size != rows + 1:
            raise DeviceError(-1, f"indptr holds {indptr.size} words for {rows} rows")
        if indptr.size and indices.size < int(indptr.max()):      # (keeps short arrays from being over-read; the library checks the rest)
            raise DeviceError(-4, f"indices holds {indices.size} entries, indptr reaches {int(indptr.max())}")
        rc = lib().hsat_create(C.byref(self._h), device_id, rows, cols, indptr.ctypes.data, indices.ctypes.data if indices.size else None)
        if rc != 0:
            raise DeviceError(rc, lib().hsat_last_error(None).decode())
        self.num_rows, self.num_cols = int(rows), int(cols)
        self.nnz = self.info()["nnz"]

    def _check(self, rc):
        if rc != 0:
            raise DeviceError(rc, lib().hsat_last_error(self._h).decode() or device.lib().hs_strerror(rc).decode())

    def close(self):
        if self._h:
            lib().hsat_destroy(self._h)
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
        self._check(lib().hsat_info(self._h, C.byref(nnz), C.byref(nbytes)))
        return {"nnz": nnz.value, "device_bytes": nbytes.value}

    def set_stream(self, hip_stream):
        self._check(lib().hsat_set_stream(self._h, C.c_void_p(hip_stream or None)))

    def sync(self):
        self._check(lib().hsat_sync(self._h))

    def _features(self, a, n, what):
        a = np.ascontiguousarray(a, dtype=np.float32)
        if a.ndim != 2 or a.shape[0] != n:
            raise DeviceError(-1, f"{what} must be ({n}, d) float32, not {a.shape}")
        return a

    def forward(self, Q, K, V, scale, want_lse=True):
        """hsat_forward, the host form: Q (num_rows, d), K and V (num_cols, d); returns (Y (num_rows, d), lse (num_rows,)) float32, or Y
        alone with want_lse=False (the call then passes NULL for lse)."""
        Q, K, V = self._features(Q, self.num_rows, "Q"), self._features(K, self.num_cols, "K"), self._features(V, self.num_cols, "V")
        if not Q.shape[1] == K.shape[1] == V.shape[1]:
            raise DeviceError(-1, f"forward: Q has {Q.shape[1]} features, K {K.shape[1]}, V {V.shape[1]}")
        Y = np.zeros((self.num_rows, Q.shape[1]), dtype=np.float32)
        lse = np.zeros(self.num_rows, dtype=np.float32) if want_lse else None
        self._check(lib().hsat_forward(self._h, Q.ctypes.data, K.ctypes.data, V.ctypes.data, Q.shape[1], float(scale), Y.ctypes.data, lse.ctypes.data if want_lse else None))
        return (Y, lse) if want_lse else Y

    def forward_device(self, q_ptr, ldq, k_ptr, ldk, v_ptr, ldv, d, scale, y_ptr, ldy, lse_ptr=None):
        """hsat_forward_device: pointers (int) into device memory, features 16-byte aligned, ld in words, lse_ptr may be None; one kernel
        launch, asynchronous on the object's stream."""
        self._check(lib().hsat_forward_device(self._h, C.c_void_p(q_ptr or None), int(ldq), C.c_void_p(k_ptr or None), int(ldk), C.c_void_p(v_ptr or None), int(ldv), int(d),
                                              float(scale), C.c_void_p(y_ptr or None), int(ldy), C.c_void_p(lse_ptr or None)))

"""hisparse_amd.attention_backward — ctypes binding of include/hisparse_attention_backward.h: the backward of the attention step over a
CSR pattern in one call (two kernel launches), with ROW-MAJOR dense operands ([index][feature], 1 <= d <= 256 features, fp32) and no
per-entry array.

    backward   P[e] = exp(scale * sum_j Q[row(e)][j] K[col(e)][j] - lse[row(e)]),   GP[e] = sum_j gY[row(e)][j] V[col(e)][j],
               D[r] = sum_{e in r} P[e] GP[e],   GS[e] = scale P[e] (GP[e] - D[row(e)])
               gQ[r] = sum_{e in r} GS[e] K[col(e)],   gK[c] = sum_{col(e) = c} GS[e] Q[row(e)],   gV[c] = sum_{col(e) = c} P[e] gY[row(e)]

lse is what attention.PatternAttention.forward wrote.  `PatternAttentionBackward` holds the pattern and its transpose on the device.  The
symbols are bound on the handle `device.lib()` returns, so HISPARSE_HIP_LIB selects libhisparse_cpu.so here as elsewhere (a second
implementation on the host, where "device" pointers are host pointers) -- there is no Python compute path and no fallback.
"""
import ctypes as C

import numpy as np

from . import device
from .device import DeviceError
from .pattern import _pattern_arrays

EXPORTS = ["hsab_create", "hsab_destroy", "hsab_last_error", "hsab_info", "hsab_set_stream", "hsab_sync", "hsab_backward_device", "hsab_backward"]

MAX_D = 256

_bound = None


def lib():
    """device.lib() with the hsab_* prototypes set."""
    global _bound
    l = device.lib()
    if _bound is not l:
        vp, u32, u64, f32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_float
        l.hsab_create.argtypes = [C.POINTER(vp), C.c_int, u32, u32, vp, vp]
        l.hsab_destroy.argtypes = [vp]
        l.hsab_last_error.restype = C.c_char_p
        l.hsab_last_error.argtypes = [vp]
        l.hsab_info.argtypes = [vp, C.POINTER(u64), C.POINTER(u64)]
        l.hsab_set_stream.argtypes = [vp, vp]
        l.hsab_sync.argtypes = [vp]
        l.hsab_backward_device.argtypes = [vp, vp, u64, vp, u64, vp, u64, vp, u64, vp, u32, f32, vp, u64, vp, u64, vp, u64]
        l.hsab_backward.argtypes = [vp, vp, vp, vp, vp, vp, u32, f32, vp, vp, vp]
        _bound = l
    return l


class PatternAttentionBackward:
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
        rc = lib().hsab_create(C.byref(self._h), device_id, rows, cols, indptr.ctypes.data, indices.ctypes.data if indices.size else None)
        if rc != 0:
            raise DeviceError(rc, lib().hsab_last_error(None).decode())
        self.num_rows, self.num_cols = int(rows), int(cols)
        self.nnz = self.info()["nnz"]

    def _check(self, rc):
        if rc != 0:
            raise DeviceError(rc, lib().hsab_last_error(self._h).decode() or device.lib().hs_strerror(rc).decode())

    def close(self):
        if self._h:
            lib().hsab_destroy(self._h)
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
        self._check(lib().hsab_info(self._h, C.byref(nnz), C.byref(nbytes)))
        return {"nnz": nnz.value, "device_bytes": nbytes.value}

    def set_stream(self, hip_stream):
        self._check(lib().hsab_set_stream(self._h, C.c_void_p(hip_stream or None)))

    def sync(self):
        self._check(lib().hsab_sync(self._h))

    def _features(self, a, n, what):
        a = np.ascontiguousarray(a, dtype=np.float32)
        if a.ndim != 2 or a.shape[0] != n:
            raise DeviceError(-1, f"{what} must be ({n}, d) float32, not {a.shape}")
        return a

    def backward(self, Q, K, V, gY, lse, scale):
        """hsab_backward, the host form: Q and gY (num_rows, d), K and V (num_cols, d), lse (num_rows,); returns (gQ (num_rows, d),
        gK (num_cols, d), gV (num_cols, d)) float32."""
        Q, gY = self._features(Q, self.num_rows, "Q"), self._features(gY, self.num_rows, "gY")
        K, V = self._features(K, self.num_cols, "K"), self._features(V, self.num_cols, "V")
        d = Q.shape[1]
        if not d == K.shape[1] == V.shape[1] == gY.shape[1]:
            raise DeviceError(-1, f"backward: Q has {d} features, K {K.shape[1]}, V {V.shape[1]}, gY {gY.shape[1]}")
        lse = np.ascontiguousarray(lse, dtype=np.float32)
        if lse.shape != (self.num_rows,):
            raise DeviceError(-1, f"lse must be ({self.num_rows},) float32, not {lse.shape}")
        gQ = np.zeros((self.num_rows, d), dtype=np.float32)
        gK, gV = (np.zeros((self.num_cols, d), dtype=np.float32) for _ in range(2))
        self._check(lib().hsab_backward(self._h, Q.ctypes.data, K.ctypes.data, V.ctypes.data, gY.ctypes.data, lse.ctypes.data, d, float(scale), gQ.ctypes.data, gK.ctypes.data,
                                        gV.ctypes.data))
        return gQ, gK, gV

    def backward_device(self, q_ptr, ldq, k_ptr, ldk, v_ptr, ldv, gy_ptr, ldgy, lse_ptr, d, scale, gq_ptr, ldgq, gk_ptr, ldgk, gv_ptr, ldgv):
        """hsab_backward_device: pointers (int) into device memory, features 16-byte aligned, ld in words; two kernel launches,
        asynchronous on the object's stream; one call in flight per object."""
        vp = C.c_void_p
        self._check(lib().hsab_backward_device(self._h, vp(q_ptr or None), int(ldq), vp(k_ptr or None), int(ldk), vp(v_ptr or None), int(ldv), vp(gy_ptr or None), int(ldgy),
                                               vp(lse_ptr or None), int(d), float(scale), vp(gq_ptr or None), int(ldgq), vp(gk_ptr or None), int(ldgk), vp(gv_ptr or None),
                                               int(ldgv)))
